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

write_zonal and read_zones are host code on the json and csv modules.  Out of scope: statistics of float planes, overlapping zones counted
more than once, ALL_TOUCHED, line and point zones, reprojection, Shapefile and GeoPackage, per-tile outputs, tables accumulated across ranks
(the stage runs on rank 0's assembled mask, as the vector stage does), and a host fallback (without a device the device calls raise)."""
from __future__ import annotations

import csv
import json
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


def _plane(a, dtype, name: str, device=None) -> torch.Tensor:
    """a contiguous [H, W] device tensor of `dtype` from a device tensor, a host tensor or a NumPy array (host input is uploaded)"""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not isinstance(a, torch.Tensor) or a.dtype != dtype or a.dim() != 2:
        raise ValueError(f"zonal_counts: {name} must be a {dtype} [H, W] tensor or array, got {getattr(a, 'dtype', type(a).__name__)} "
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


def write_zonal(path, features, stats, codes=None, pixel_area: float = 1.0, class_zero: bool = False, crs=None) -> int:
    """The table of zonal_rows as a file; the suffix decides: .geojson -- one FeatureCollection of the zone features with their geometry
    and their own properties, the added ones behind them (an added name replaces an own property of that name); .csv -- one row per zone,
    the zones' own properties first (the union of their names in order of appearance, empty where a zone lacks one), None as an empty
    field.  features: read_zones' list, one entry per row of the tables.  crs: the "crs" member to write (None: the one read_zones kept).
    Returns the number of zones.  Host code."""
    suffix = os.path.splitext(os.fspath(path))[1].lower()
    if suffix not in (".geojson", ".csv"):
        raise ValueError(f"{path}: the zonal table is written as .geojson or .csv")
    rows = zonal_rows(stats, codes, pixel_area, class_zero)
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
