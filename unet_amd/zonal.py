"""Zonal statistics of a class mask on the device (csrc/zonal.hip): the pixels, and optionally the objects, of every class per
polygon zone -- canopy cover per parcel, sealed surface per district, crowns per stand -- and the writers of that table.
tests/zonal_ref.py restates the rules below in NumPy; the device tables equal it bit for bit.

Zone plane  int32 [H, W]; -1 means no zone, the zones are 0 .. Z - 1.  A pixel belongs to at most one zone.  With polygon zones the rules of
            unet_amd/rasterize.py decide (rasterize_ids): the pixel centre, even-odd fill over all rings of a feature, a centre on a left or
            top border inside, and where zones overlap the LAST feature of the file wins.  A zone that lies partly outside the raster counts
            only its pixels inside it; one that lies wholly outside, or covers no pixel centre, has no pixels.
Counts      counts[z, c] = the number of pixels with zone z and mask value c: int64 [Z, C], 1 <= C <= 256.
Objects     optional, when a label image is given: labels[p] is the smallest linear index y * W + x of the pixels of p's component or
            instance (the convention of postprocess.label_components and instances.split_instances).  Pixel p is an anchor iff
            labels[p] == p, and objects[z, c] = the number of anchors with zone z and class c.  AN OBJECT THEREFORE BELONGS TO THE ZONE
            THAT HOLDS ITS FIRST PIXEL IN ROW-MAJOR ORDER, whole, however many of its pixels lie in other zones; an object whose first pixel
            lies in no zone is counted nowhere.  Assignment by centroid or by the largest overlap is out of scope.
Bad input   a pixel whose mask value is >= C, or whose zone lies outside -1 .. Z - 1, is counted nowhere and sets a word that the host reads
            once after the launch: ValueError.
Limits      Z < 2^23 (the rasterizer's feature limit), Z * C < 2^31, H and W within ops.check_raster_shape, H * W < 2^31 with labels (all
            ValueError, before any launch).
Determinism every accumulation is an integer add, so the tables are a function of the inputs alone, independent of scheduling.

The kernel has two forms behind one entry point: up to ops.zonal_lds_bins() bins every workgroup counts into a private uint32 table in LDS
and adds its non-zero bins to the int64 table at the end; beyond that the adds go to the int64 table directly.  In both, equal keys are
merged before anything is added: among the 4 pixels of a lane, along the lanes of a wavefront (the head of a run of lanes adds the run),
and from step to step -- a wavefront whose 256 pixels hold one key carries (key, count) in registers along its contiguous span of the
plane and writes it when the key changes.  Memory: 4 bytes per pixel for the zone plane next to the rasterizer's own buffers (unet_amd/rasterize.py),
16 Z C bytes for the two tables.  Every buffer that a kernel writes comes from _alloc.

Float planes (zonal_values, csrc/zonal_values.hip): count, mean, standard deviation, minimum, maximum and sum of a float32 plane
-- a regression output, the probability of one class -- per zone.  tests/zonal_values_ref.py restates these rules; the device tables equal
it bit for bit.
Inputs      the zone plane as above, a value plane float32 [H, W], an optional nodata (a number, or None).  H * W <= 2^31 - 1 and Z < 2^23
            (ValueError before any launch).
Valid       a pixel is valid iff its zone is >= 0, its value is finite and its value does not equal nodata.  pixels[z] counts all pixels of
            zone z, valid[z] the valid ones: NaN, +-inf and nodata pixels count in pixels only.
Fixed point floating adds depend on their order, integer adds do not: A = the largest |v| over the valid pixels, E = 0 when A = 0, else the
            frexp exponent, 2^(E-1) <= A < 2^E; the shift is s = 30 - E (-98 .. 178), and every valid value becomes q = rint(double(v) * 2^s),
            half to even, |q| <= 2^30.  float32 -> double and the scaling by a power of two are exact, so
            np.rint(np.ldexp(v.astype(np.float64), s)).astype(np.int64) gives the same integers.  shift= fixes s instead, so that the tables
            of several rasters, tiles or ranks add up; a valid pixel with |q| > 2^30 then sets a word that the host reads once after the
            launch: ValueError.
Tables      pixels, valid, sum_q = sum q, sq_lo = sum lo and sq_hi = sum hi with q^2 = hi * 2^30 + lo, 0 <= lo < 2^30: int64 [Z].  Each term is
            at most 2^30 and a plane holds fewer than 2^31 pixels, so every sum stays within 2^61 and nothing wraps.  min and max
            (float32 [Z]) are the exact extremes of the valid pixels, by unsigned atomic minimum and maximum on the order-preserving image
            of the float bits (-0.0 lies below +0.0); a zone without a valid pixel holds +inf and -inf on the device.
Derived     on the host, in Python integers and one division (zonal_value_rows): mean = sum_q / valid * 2^-s, population std =
            sqrt(SQ * valid - sum_q^2) / valid * 2^-s with SQ = sq_hi * 2^30 + sq_lo, sum = sum_q * 2^-s; a zone with valid == 0 has None
            for mean, std, min, max and sum.
Accuracy    |q * 2^-s - v| <= 2^(E-31) for every valid pixel, so the mean differs from the float64 mean of the raw floats by at most
            2^(E-31) plus float64 rounding: 2^-31 of the plane's largest magnitude, 128 times finer than a float32 ulp at that magnitude.
Bad input   a zone outside -1 .. Z - 1 is counted nowhere, indexes nothing and raises ValueError after the launch, as in zonal_counts.

write_zonal and read_zones are host code on the json and csv modules.  Out of scope: several float planes at once (all_classes), median,
percentiles and histograms, weighted or fractional pixel coverage, float64 and integer value planes, per-object float statistics (objects.object_values
has them), overlapping zones counted more than once, ALL_TOUCHED, line and point zones, reprojection, Shapefile and
GeoPackage, per-tile outputs, tables accumulated across ranks (the stage runs on rank 0's assembled output, as the vector stage does), and a
host fallback (without a device the device calls raise)."""
from __future__ import annotations

import csv
import json
import math
import os
import re
import time
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops
from .rasterize import Rings, _device_rings, _host_rings, _load_collection, _parse_features, _priority_plane
from .vectorize import _Stages, check_geojson_args, epsg_of_tags


def _alloc(shape, dtype, device) -> torch.Tensor:
    """every device buffer that a kernel of this module writes (the tests put guard bands around them here)"""
    return torch.empty(tuple(shape), dtype=dtype, device=device)


@dataclass
class ZonalStats:
    """the tables of zonal_counts: int64 [Z, C] each, objects None when no labels were given"""
    counts: torch.Tensor
    objects: Optional[torch.Tensor] = None

    def cpu(self) -> "ZonalStats":
        return ZonalStats(self.counts.cpu(), None if self.objects is None else self.objects.cpu())


def rasterize_ids(rings_or_polygons, shape, stages: Optional[dict] = None) -> torch.Tensor:
    """int32 [H, W] device tensor: the index of the feature (Rings, or Polygons) that owns each pixel under the rasterizer's rules, -1 where
    no feature covers it.  It runs the passes of rasterize() and resolves the priority plane into indices instead of burn values (the burn
    values play no part).  stages: as in rasterize()."""
    H, W = ops.check_raster_shape("rasterize_ids", tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else shape)
    rings = _device_rings("rasterize_ids", rings_or_polygons)
    st = _Stages(stages)
    plane, M, wrong = _priority_plane(rings, H, W, st)
    ids = _alloc((H, W), torch.int32, plane.device)
    ops.ras_resolve_ids(plane, ids)
    st.mark("resolve")
    if stages is not None:
        stages.update(crossings=M, features=rings.n_features, pair_mismatch=wrong)
    return ids


def _plane(a, dtype, name: str, device=None, what: str = "zonal_counts") -> torch.Tensor:
    """a contiguous [H, W] device tensor of `dtype` from a device tensor, a host tensor or a NumPy array (host input is uploaded)"""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not isinstance(a, torch.Tensor) or a.dtype != dtype or a.dim() != 2:
        raise ValueError(f"{what}: {name} must be a {dtype} [H, W] tensor or array, got {getattr(a, 'dtype', type(a).__name__)} "
                         f"{tuple(getattr(a, 'shape', ()))}")
    if not a.is_cuda:
        a = a.to(device if device is not None else "cuda")
    return a.contiguous()


def zonal_counts(zones, mask, n_zones: int, n_classes: int, labels=None, stages: Optional[dict] = None) -> ZonalStats:
    """ZonalStats (device tensors) of a zone plane (int32 [H, W], -1 = no zone) and a class mask (uint8 [H, W]) under the rules of the module
    docstring; labels (int32 [H, W], or None): the objects are counted too.  Host inputs are uploaded.  ValueError for a mask value
    >= n_classes or a zone outside -1 .. n_zones - 1 (read from the device after the launch) and for every limit (before it).
    stages: a dict that receives the milliseconds of `count` (this synchronises the device: for measurements only)."""
    Z, C = ops.check_zonal_sizes("zonal_counts", n_zones, n_classes)
    H, W = ops.check_raster_shape("zonal_counts", tuple(getattr(zones, "shape", ())))
    for name, t in (("mask", mask), ("labels", labels)):
        if t is not None and tuple(getattr(t, "shape", ())) != (H, W):
            raise ValueError(f"zonal_counts: {name} has shape {tuple(getattr(t, 'shape', ()))}, the zones {(H, W)}")
    if labels is not None and H * W > ops.VEC_MAX_COUNT:
        raise ValueError(f"zonal_counts: int32 labels index at most 2^31 - 1 pixels, got {H} x {W}")
    if not torch.cuda.is_available():
        raise ValueError("zonal_counts runs on the GPU and there is no device (it has no host fallback)")
    dev = next((t.device for t in (zones, mask, labels) if isinstance(t, torch.Tensor) and t.is_cuda), None)
    z, m = _plane(zones, torch.int32, "zones", dev), _plane(mask, torch.uint8, "mask", dev)
    lab = None if labels is None else _plane(labels, torch.int32, "labels", dev)
    dev = z.device
    st = _Stages(stages)
    counts, bad = _alloc((Z, C), torch.int64, dev).zero_(), _alloc((1,), torch.int64, dev)
    objects = None if lab is None else _alloc((Z, C), torch.int64, dev).zero_()
    ops.zonal_counts(z, m, lab, Z, C, counts, objects, bad)
    word = ops.vec_read(bad, 0, 1)[0]          # the host read
    st.mark("count")
    if word & 1:
        raise ValueError(f"zonal_counts: the mask holds a value >= {C}, the number of classes")
    if word:
        raise ValueError(f"zonal_counts: the zone plane holds a value outside -1..{Z - 1}")
    return ZonalStats(counts, objects)


# ------------------------------------------------------------------------------------------------------------------ float planes

Q_BITS = 30          # |q| <= 2^30


@dataclass
class ZonalValues:
    """the tables of zonal_values: pixels, valid, sum_q, sq_lo, sq_hi int64 [Z], min and max float32 [Z] (+inf / -inf for a zone without a
    valid pixel), and the shift s of q = rint(v * 2^s).  Tables of one shift add up (min and max combine by minimum and maximum).  table:
    the one int64 [6, Z] allocation that the seven are views of (row 5 holds min and max), so that one copy moves them all"""
    pixels: torch.Tensor
    valid: torch.Tensor
    sum_q: torch.Tensor
    sq_lo: torch.Tensor
    sq_hi: torch.Tensor
    min: torch.Tensor
    max: torch.Tensor
    shift: int
    table: Optional[torch.Tensor] = None

    @staticmethod
    def of_table(table: torch.Tensor, shift: int) -> "ZonalValues":
        Z = table.shape[1]
        mm = table[5].view(torch.float32).view(2, Z)
        return ZonalValues(table[0], table[1], table[2], table[3], table[4], mm[0], mm[1], shift, table)

    def cpu(self) -> "ZonalValues":
        if self.table is not None:
            return ZonalValues.of_table(self.table.cpu(), self.shift)          # the one copy
        return ZonalValues(*(t.cpu() for t in (self.pixels, self.valid, self.sum_q, self.sq_lo, self.sq_hi, self.min, self.max)), self.shift)


_NUMPY_DTYPE = {torch.int32: np.dtype(np.int32), torch.float32: np.dtype(np.float32)}


def _has_dtype(a, dtype) -> bool:
    """whether a tensor or a NumPy array holds elements of the torch `dtype`"""
    return a.dtype == dtype if isinstance(a, torch.Tensor) else isinstance(a, np.ndarray) and a.dtype == _NUMPY_DTYPE[dtype]


def shift_of_absmax(bits: int) -> int:
    """the shift 30 - E of the largest |v|, given as its float32 bit pattern: E = 0 for 0, else the frexp exponent, 2^(E-1) <= A < 2^E"""
    a = float(np.array([bits], dtype=np.uint32).view(np.float32)[0])
    if not np.isfinite(a):
        raise ValueError(f"zonal_values: the largest |value| is not finite (bits {bits:#x})")
    return Q_BITS - (math.frexp(a)[1] if a else 0)


def zonal_values(zones, values, n_zones: int, nodata=None, shift: Optional[int] = None, stages: Optional[dict] = None) -> ZonalValues:
    """ZonalValues (device tensors) of a zone plane (int32 [H, W], -1 = no zone) and a value plane (float32 [H, W]) under the rules of the
    module docstring.  nodata: a number whose pixels are not valid, or None.  shift: None derives it from the largest |value| of the valid
    pixels (one more pass and one host read); an int fixes it, so that the tables of several rasters or tiles add up -- a valid pixel with
    |q| > 2^30 is then a ValueError.  Host inputs are uploaded.  ValueError for a zone outside -1 .. n_zones - 1 (read from the device after
    the launch) and for every limit (before it).  stages: a dict that receives the milliseconds of `absmax` and `values` (this synchronises
    the device: for measurements only)."""
    what = "zonal_values"
    H, W, Z = ops.check_zonal_values_sizes(what, tuple(getattr(zones, "shape", ())), n_zones)
    if tuple(getattr(values, "shape", ())) != (H, W):
        raise ValueError(f"{what}: values has shape {tuple(getattr(values, 'shape', ()))}, the zones {(H, W)}")
    ops.check_zonal_nodata(what, nodata)
    if shift is not None:
        ops.check_zonal_shift(what, shift)
    for name, t, dtype in (("zones", zones, torch.int32), ("values", values, torch.float32)):          # before the device is asked for
        if not _has_dtype(t, dtype):
            raise ValueError(f"{what}: {name} must be a {dtype} [H, W] tensor or array, got {getattr(t, 'dtype', type(t).__name__)}")
    if not torch.cuda.is_available():
        raise ValueError("zonal_values runs on the GPU and there is no device (it has no host fallback)")
    dev = next((t.device for t in (zones, values) if isinstance(t, torch.Tensor) and t.is_cuda), None)
    z, v = _plane(zones, torch.int32, "zones", dev, what), _plane(values, torch.float32, "values", dev, what)
    dev = z.device
    st = _Stages(stages)
    words = _alloc((2,), torch.int64, dev)          # the largest |v|, the bad word
    if shift is None:
        ops.zonal_absmax(z, v, Z, nodata, words[0:1])
        shift = shift_of_absmax(ops.vec_read(words, 0, 1)[0])          # a host read
        st.mark("absmax")
    table = _alloc((6, Z), torch.int64, dev)
    out = ZonalValues.of_table(table, shift)
    ops.zonal_values(z, v, Z, nodata, shift, table[:5], table[5].view(torch.float32).view(2, Z), words[1:2])
    word = ops.vec_read(words, 1, 1)[0]          # the host read
    st.mark("values")
    if word & 2:
        raise ValueError(f"{what}: the zone plane holds a value outside -1..{Z - 1}")
    if word:
        raise ValueError(f"{what}: a value times 2^{shift} exceeds 2^{Q_BITS}: shift={shift} is too large for this plane")
    return out


def zonal_value_rows(stats: ZonalValues, pixel_area: float = 1.0) -> list:
    """the added properties of every zone, one ordered dict each: pixels (all pixels of the zone inside the raster), area (pixels x
    pixel_area), valid (the pixels with a finite value other than nodata) and mean, std (population), min, max, sum of those.  The sums are
    Python integers up to one division: mean = sum_q / valid * 2^-s, std = sqrt(SQ * valid - sum_q^2) / valid * 2^-s with SQ = sq_hi * 2^30
    + sq_lo.  A zone without a valid pixel has None for all five."""
    host = [(t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)) for t in
            (stats.pixels, stats.valid, stats.sum_q, stats.sq_lo, stats.sq_hi, stats.min, stats.max)]
    if any(a.ndim != 1 or a.shape != host[0].shape for a in host):
        raise ValueError(f"the tables must be [Z] each, got {[a.shape for a in host]}")
    s = int(stats.shift)
    rows = []
    for pixels, valid, sum_q, lo, hi, mn, mx in zip(*(a.tolist() for a in host)):
        row = {"pixels": pixels, "area": pixels * float(pixel_area), "valid": valid}
        if valid:
            sq = (hi << Q_BITS) + lo
            row.update(mean=math.ldexp(sum_q / valid, -s), std=math.ldexp(math.sqrt(sq * valid - sum_q * sum_q) / valid, -s), min=mn, max=mx,
                       sum=math.ldexp(float(sum_q), -s))
        else:
            row.update(mean=None, std=None, min=None, max=None, sum=None)
        rows.append(row)
    return rows


# ------------------------------------------------------------------------------------------------------------------ files (host)

class ZoneFeatures(list):
    """the read features of a zones file in file order, each {"properties": dict, "geometry": dict} as the file holds them; crs: the
    file's "crs" member or None"""
    crs = None


def read_zones(path, geotransform=None):
    """(Rings, ZoneFeatures) of a FeatureCollection of Polygon and MultiPolygon zones: rasterize.read_geojson without a burn attribute.  All
    burn values are 0; features with a null geometry are skipped, so zone z is the z-th feature WITH a geometry; any other geometry type
    raises ValueError.  Every read feature keeps its `properties` and its raw `geometry`.  geotransform: as in read_geojson."""
    check_geojson_args(geotransform)
    doc = _load_collection(path)
    feats = ZoneFeatures()
    feats.crs = doc.get("crs")

    def keep(index, feat):
        props = feat.get("properties")
        feats.append({"properties": dict(props) if isinstance(props, dict) else {}, "geometry": feat["geometry"]})

    xy, length, ring_count = _parse_features(doc["features"], geotransform, keep)
    return _host_rings(xy, length, ring_count, np.zeros(len(feats), dtype=np.uint8)), feats


def epsg_of_crs(crs) -> Optional[int]:
    """the EPSG code of a GeoJSON "crs" member of type name (urn:ogc:def:crs:EPSG::25832, EPSG:25832); anything else is unknown (None)"""
    name = crs.get("properties", {}).get("name") if isinstance(crs, dict) and isinstance(crs.get("properties"), dict) else None
    m = re.search(r"EPSG:{1,2}(\d+)$", name) if isinstance(name, str) else None
    return int(m.group(1)) if m else None


def _class_names(C: int, codes, class_zero: bool) -> list:
    """the name of every class in the added properties: codes[c], else the id as the raster on disk holds it; class 0 under class_zero is
    `nodata`"""
    if codes is not None and len(codes) < C:
        raise ValueError(f"codes names {len(codes)} classes, the tables hold {C}")
    return ["nodata" if class_zero and c == 0 else str(codes[c]) if codes is not None else str(c - 1 if class_zero else c) for c in range(C)]


def zonal_rows(stats, codes=None, pixel_area: float = 1.0, class_zero: bool = False) -> list:
    """the added properties of every zone, one ordered dict each: pixels (all pixels of the zone inside the raster), area (pixels x
    pixel_area), px_<name> and frac_<name> per class, majority (the id, as the raster on disk holds it, of the class with the most pixels,
    ties to the smallest id) and n_<name> when objects were counted.  Under class_zero class 0 is NO_Data: px_nodata, no frac, left out of
    the denominator of the other fractions and of majority.  A zone whose denominator is 0 has majority and every frac None."""
    counts = stats.counts.cpu().numpy() if isinstance(stats.counts, torch.Tensor) else np.asarray(stats.counts)
    objects = None if stats.objects is None else (stats.objects.cpu().numpy() if isinstance(stats.objects, torch.Tensor) else np.asarray(stats.objects))
    if counts.ndim != 2 or (objects is not None and objects.shape != counts.shape):
        raise ValueError(f"the tables must be [Z, C], got {counts.shape}" + ("" if objects is None else f" and {objects.shape}"))
    Z, C = counts.shape
    names = _class_names(C, codes, class_zero)
    first = 1 if class_zero else 0
    rows = []
    for z in range(Z):
        c = [int(v) for v in counts[z]]
        pixels, valid = sum(c), sum(c[first:])
        row = {"pixels": pixels, "area": pixels * float(pixel_area)}
        for k in range(C):
            row[f"px_{names[k]}"] = c[k]
            if k >= first:
                row[f"frac_{names[k]}"] = c[k] / valid if valid else None
        best = max(range(first, C), key=lambda k: (c[k], -k)) if valid else None
        row["majority"] = None if best is None else best - first
        if objects is not None:
            for k in range(first, C):
                row[f"n_{names[k]}"] = int(objects[z, k])
        rows.append(row)
    return rows


def write_zonal(path, features, stats, codes=None, pixel_area: float = 1.0, class_zero: bool = False, crs=None, values=None) -> int:
    """The table of zonal_rows as a file; the suffix decides: .geojson -- one FeatureCollection of the zone features with their geometry
    and their own properties, the added ones behind them (an added name replaces an own property of that name); .csv -- one row per zone,
    the zones' own properties first (the union of their names in order of appearance, empty where a zone lacks one), None as an empty
    field.  features: read_zones' list, one entry per row of the tables.  crs: the "crs" member to write (None: the one read_zones kept).
    values: a ZonalValues whose zonal_value_rows are written behind the class rows (pixels and area are common to both), or alone where
    stats is None.  Returns the number of zones.  Host code."""
    suffix = os.path.splitext(os.fspath(path))[1].lower()
    if suffix not in (".geojson", ".csv"):
        raise ValueError(f"{path}: the zonal table is written as .geojson or .csv")
    if values is None:
        rows = zonal_rows(stats, codes, pixel_area, class_zero)
    else:
        rows = zonal_value_rows(values, pixel_area)
        if stats is not None:
            own = zonal_rows(stats, codes, pixel_area, class_zero)
            if len(own) != len(rows) or any(a["pixels"] != b["pixels"] for a, b in zip(own, rows)):
                raise ValueError("the class tables and the value tables are not of the same zones")
            rows = [{**a, **b} for a, b in zip(own, rows)]
    if len(rows) != len(features):
        raise ValueError(f"the tables hold {len(rows)} zones, the features {len(features)}")
    crs = getattr(features, "crs", None) if crs is None else crs
    if suffix == ".geojson":
        feats = [json.dumps({"type": "Feature", "properties": {**{k: v for k, v in f["properties"].items() if k not in row}, **row},
                             "geometry": f["geometry"]}) for f, row in zip(features, rows)]
        head = '{"type":"FeatureCollection",' + ("" if crs is None else '"crs":' + json.dumps(crs) + ",")
        with open(os.fspath(path), "w") as f:
            f.write(head + '"features":[\n' + ",\n".join(feats) + "\n]}\n")
        return len(rows)
    added = list(rows[0]) if rows else []
    own = []
    for f in features:
        own += [k for k in f["properties"] if k not in own and k not in added]
    with open(os.fspath(path), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(own + added)
        for feat, row in zip(features, rows):
            cells = [feat["properties"].get(k) for k in own] + [row[k] for k in added]
            w.writerow(["" if v is None else json.dumps(v) if isinstance(v, (dict, list)) else v for v in cells])
    return len(rows)


# ------------------------------------------------------------------------------------------------------------------ entry points

def check_zones(zones, zonal_objects=False) -> bool:
    """the zones_path= / zones= and zonal_objects= arguments of predict_raster / save_predictions -> whether a zonal table is wanted.  Which
    outputs can be summarised is predict.check_outputs' rule"""
    if zones is None:
        if zonal_objects:
            raise ValueError("zonal_objects without zones")
        return False
    if not isinstance(zones, (str, os.PathLike)):
        raise ValueError(f"zones must be None or the path of a GeoJSON file, got {type(zones).__name__}")
    return True


def zonal_mask(mask, zones_path, out_path, geotransform=None, tags=None, codes=None, class_zero: bool = False, labels=None, objects: bool = False,
               timing: Optional[dict] = None) -> ZonalStats:
    """The output stage of an assembled class mask (device or host): read_zones on the raster's grid, rasterize_ids, zonal_counts -- with
    objects=True also the objects: `labels` where given (the instance labels), else the 4-connected components --, one copy of the tables to
    the host, write_zonal.  The classes are those of codes, else 0 .. the mask's largest value.  A zones file that names an EPSG code other
    than the raster's (epsg_of_tags) is refused: there is no reprojection.  timing gains zonal_seconds, zonal_zones and zonal_pixels (the
    pixels in any zone).  Returns the host tables."""
    t0 = time.perf_counter()
    if not torch.cuda.is_available():
        raise ValueError("zonal statistics run on the GPU and there is no device (they have no host fallback)")
    rings, feats = read_zones(zones_path, geotransform)
    theirs, ours = epsg_of_crs(feats.crs), epsg_of_tags(tags)
    if theirs is not None and ours is not None and theirs != ours:
        raise ValueError(f"{zones_path}: the zones are in EPSG:{theirs}, the raster in EPSG:{ours} (there is no reprojection)")
    if not len(feats):
        raise ValueError(f"{zones_path}: no Polygon or MultiPolygon zone")
    m = _plane(mask, torch.uint8, "mask")
    C = len(codes) if codes is not None else int(m.max()) + 1
    ids = rasterize_ids(rings.to(m.device), m.shape)
    if objects and labels is None:
        from .postprocess import label_components
        labels = label_components(m, 4)
    stats = zonal_counts(ids, m, len(feats), C, labels if objects else None)
    tables = (stats.counts if stats.objects is None else torch.stack([stats.counts, stats.objects])).cpu()          # the one copy
    host = ZonalStats(tables, None) if stats.objects is None else ZonalStats(tables[0], tables[1])
    gt = None if geotransform is None else tuple(float(v) for v in geotransform)
    write_zonal(out_path, feats, host, codes, 1.0 if gt is None else abs(gt[1] * gt[5]), class_zero)
    if timing is not None:
        timing.update(zonal_seconds=time.perf_counter() - t0, zonal_zones=len(feats), zonal_pixels=int(host.counts.sum()))
    return host


def zonal_plane(out, zones_path, out_path, geotransform=None, tags=None, nodata=None, timing: Optional[dict] = None) -> ZonalValues:
    """The output stage of an assembled float plane (regression, or the probability of one class; device or host), the twin of zonal_mask:
    read_zones on the raster's grid, the EPSG check, rasterize_ids, zonal_values with a derived shift, one copy of the tables to the host,
    write_zonal (pixels, area, valid, mean, std, min, max, sum per zone).  nodata: the value of the plane's pixels without a prediction
    (-9999 under regression), or None.  timing gains zonal_seconds, zonal_zones and zonal_pixels (the pixels in any zone).  Returns the
    host tables."""
    t0 = time.perf_counter()
    if not torch.cuda.is_available():
        raise ValueError("zonal statistics run on the GPU and there is no device (they have no host fallback)")
    rings, feats = read_zones(zones_path, geotransform)
    theirs, ours = epsg_of_crs(feats.crs), epsg_of_tags(tags)
    if theirs is not None and ours is not None and theirs != ours:
        raise ValueError(f"{zones_path}: the zones are in EPSG:{theirs}, the raster in EPSG:{ours} (there is no reprojection)")
    if not len(feats):
        raise ValueError(f"{zones_path}: no Polygon or MultiPolygon zone")
    v = _plane(out, torch.float32, "values", None, "zonal_values")
    ids = rasterize_ids(rings.to(v.device), v.shape)
    host = zonal_values(ids, v, len(feats), nodata).cpu()          # the one copy
    gt = None if geotransform is None else tuple(float(x) for x in geotransform)
    write_zonal(out_path, feats, None, pixel_area=1.0 if gt is None else abs(gt[1] * gt[5]), values=host)
    if timing is not None:
        timing.update(zonal_seconds=time.perf_counter() - t0, zonal_zones=len(feats), zonal_pixels=int(host.pixels.sum()))
    return host
