"""Attributes of every object of a class mask, measured on the device (csrc/objects.hip): size, centre, extent, perimeter and
one position inside each object -- crown diameter and a tree list, roof compactness, parcel extents -- and the writers of that table.
tests/objects_ref.py restates the rules below sequentially in NumPy; the device tables equal it bit for bit.

Inputs      mask uint8 [H, W]; labels int32 [H, W] in the convention of postprocess.label_components and instances.split_instances
            (labels[p] is the smallest linear index y * W + x of the pixels of p's object), None means label_components(mask, 4); exclude
            None, a class id or ids (vectorize.check_exclude).  H and W within ops.check_raster_shape and H * W <= 2^31 - 1.
Objects     pixel L is an anchor iff labels[L] == L.  The objects are the anchors whose class mask[L] is not excluded, in ascending L:
            object k = 0 .. P - 1.  This is the order, and without simplification the set, of Polygons.poly_label from polygonize(mask,
            exclude) / polygonize_labels(mask, labels, exclude).  Pixels of excluded classes contribute to no object, but they are "other"
            pixels for the edges below.
Table       ObjectTable, all exact integers:
              label   int32 [P]     the anchor L
              cls     uint8 [P]     mask[L]
              pixels  int64 [P]     the number of pixels p with labels[p] == L
              sum_x, sum_y  int64 [P]  the sums of the column and row indices of those pixels
              bbox    int32 [P, 4]  x0, y0, x1, y1, half open (x1 and y1 are one past the last column and row)
              edges_v, edges_h  int64 [P]  boundary edge counts, below
              point   int32 [P]     the linear index of the representative pixel, below
Edges       edges_v counts the unit edges between a pixel of the object and its left or right neighbour when that neighbour has another
            label or lies outside the raster; edges_h the same for the upper and lower neighbour.  For every polygon of the unsimplified
            polygonize result edges_v + edges_h is the summed Manhattan length of its rings, exterior and holes.
Point       cx = sum_x // pixels, cy = sum_y // pixels; point is the pixel of the object that minimises ((x - cx)^2 + (y - cy)^2, y * W + x)
            lexicographically.  It lies in the object by construction; the centroid of a ring or a U does not.
Bad input   a label outside 0 .. H * W - 1, labels[labels[p]] != labels[p], or mask[p] != mask[labels[p]]: each sets a bit of one word that
            the host reads once after the launches: ValueError.  Nothing is stored outside the tables in that case.  Every size limit raises
            ValueError before any launch; so does a call without a device (there is no host fallback, as in zonal.py).
Determinism every accumulation is an integer add, minimum or maximum, so the table is a function of (mask, labels, exclude) alone.

Launches: the anchors of the kept classes are marked as a byte plane (ops.inst_marks with the kept classes) and scanned (ops.vec_scan; P is
the scan's total: a host read); obj_compact fills label and cls; obj_accumulate walks the label plane once and merges equal (label, class)
keys among a lane's 4 pixels, along the lanes and along a wavefront's span before the head of a run adds it (five 64-bit adds, four 32-bit
minima / maxima, the latter only where a plain read of the extent says they would change it) and checks the labels there; obj_point walks
it again after the sums are complete (and does nothing when that check failed): once where (H - 1)^2 + (W - 1)^2 < 2^33, so that squared
distance and index share one 64-bit key, else twice.  Memory next to the inputs: 5 bytes per pixel (marks and their scan), 68 bytes per object.
Every buffer that a kernel writes comes from _alloc.

Float planes (object_values, csrc/object_values.hip): count, mean, standard deviation, sum, minimum and maximum of a float32
plane -- a canopy height model, the merged probability of the chosen class -- per object, and the pixel of each extreme (the treetop).
tests/object_values_ref.py restates these rules; the device tables equal it bit for bit.
Objects     exactly those of measure_objects(mask, labels, exclude), in its order, from the same marks and scan (_object_index).
Valid       pixel p contributes to object offs[labels[p]] iff mask[p] is not excluded, values[p] is finite and values[p] != float32(nodata)
            (ops.check_zonal_nodata; None: no nodata).
Fixed point as zonal.zonal_values: A = the largest |v| over the valid pixels (obj_absmax reads the mask and the values only), s = 30 - E
            (zonal.shift_of_absmax), q = rint(double(v) * 2^s), half to even, |q| <= 2^30; valid, sum_q = sum q, sq_lo = sum lo and sq_hi = sum
            hi with q^2 = hi * 2^30 + lo are int64 [P] and cannot wrap below 2^31 pixels.  shift= fixes s; a valid pixel with |q| > 2^30 is then
            left out and the call raises ValueError.
Extremes    one 64-bit atomic each: max takes key(v) << 32 | (0xFFFFFFFF - p) by maximum, min takes key(v) << 32 | p by minimum, key the
            order-preserving unsigned image of the float bits (-0.0 below +0.0) and p the linear index.  So max / argmax are the largest
            value and the smallest linear index that attains it, min / argmin likewise.  An object without a valid pixel has valid 0, min
            +inf, max -inf and argmin = argmax = -1.
Bad input   the three checks of measure_objects, made at every flush, and the same ValueErrors.
Launches    the index stage of measure_objects, obj_absmax (unless shift is given; one host read), obj_values (initialise, walk, decode), one
            host read of the word.  Memory next to the inputs: the 5 bytes per pixel of the index stage and 53 bytes per object.

object_rows, object_value_rows and write_objects are host code on the json and csv modules.  Out of scope: second moments, orientation and
ellipse axes (sum x^2 can exceed 64 bits at the raster limits), median and percentiles per object, float64 planes, resampling a value
raster onto the mask's grid, the peak as the feature's geometry, the pole of inaccessibility (it needs a distance transform on labels),
8-connectivity, per-tile outputs, tables across ranks (the stage runs on rank 0's assembled mask), Shapefile and GeoPackage, and a host
fallback."""
from __future__ import annotations

import csv
import json
import math
import os
import time
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np
import torch

from . import ops
from .vectorize import _Stages, check_exclude, check_geojson_args


def _alloc(shape, dtype, device) -> torch.Tensor:
    """every device buffer that a kernel of this module writes (the tests put guard bands around them here)"""
    return torch.empty(tuple(shape), dtype=dtype, device=device)


@dataclass
class ObjectTable:
    """the table of measure_objects, one entry per object in ascending label order (the module docstring has the rules)"""
    label: torch.Tensor            # int32 [P]
    cls: torch.Tensor              # uint8 [P]
    pixels: torch.Tensor           # int64 [P]
    sum_x: torch.Tensor            # int64 [P]
    sum_y: torch.Tensor            # int64 [P]
    bbox: torch.Tensor             # int32 [P, 4]
    edges_v: torch.Tensor          # int64 [P]
    edges_h: torch.Tensor          # int64 [P]
    point: torch.Tensor            # int32 [P]
    shape: tuple = (0, 0)          # (H, W) of the raster

    def cpu(self) -> "ObjectTable":
        return ObjectTable(**{f.name: (v.cpu() if isinstance(v, torch.Tensor) else v) for f in fields(self) for v in (getattr(self, f.name),)})

    @property
    def n_objects(self) -> int:
        return int(self.label.shape[0])


def _plane(a, dtype, name: str, device=None) -> torch.Tensor:
    """a contiguous [H, W] device tensor of `dtype` from a device tensor, a host tensor or a NumPy array (host input is uploaded)"""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not isinstance(a, torch.Tensor) or a.dtype != dtype or a.dim() != 2:
        raise ValueError(f"measure_objects: {name} must be a {dtype} [H, W] tensor or array, got {getattr(a, 'dtype', type(a).__name__)} "
                         f"{tuple(getattr(a, 'shape', ()))}")
    if not a.is_cuda:
        a = a.to(device if device is not None else "cuda")
    return a.contiguous()


def _object_index(m: torch.Tensor, lab: torch.Tensor, exclude: tuple) -> tuple:
    """the index stage that measure_objects and object_values share: (offs int32 [H, W], P, label int32 [P], cls uint8 [P]) -- the anchors of
    the kept classes are marked (ops.inst_marks), scanned (ops.vec_scan; P is the scan's total: a host read) and compacted (obj_compact)"""
    H, W = m.shape
    n, dev = H * W, m.device
    kept = tuple(c for c in range(256) if c not in exclude)
    mark, offs = _alloc((H, W), torch.uint8, dev), _alloc((H, W), torch.int32, dev)
    blocks = _alloc((ops.vec_scan_words(n),), torch.int64, dev)
    ops.inst_marks(m, lab, kept, mark)
    ops.vec_scan(mark, offs, blocks)
    P = ops.vec_read(blocks, ops.vec_scan_words(n) - 1, 1)[0]          # a host read
    label, cls = _alloc((P,), torch.int32, dev), _alloc((P,), torch.uint8, dev)
    if P:
        ops.obj_compact(m, mark, offs, P, label, cls)
    return offs, P, label, cls


def measure_objects(mask, labels=None, exclude=None, stages: Optional[dict] = None) -> ObjectTable:
    """ObjectTable (device tensors) of a class mask (uint8 [H, W]) and a label image (int32 [H, W], or None: the 4-connected components)
    under the rules of the module docstring.  Host inputs are uploaded.  ValueError for labels that break the convention (read from the
    device after the launches) and for every limit (before them).  stages: a dict that receives the milliseconds of `index`, `accumulate`
    and `point` (this synchronises the device after each: for measurements only)."""
    exclude = check_exclude(exclude)
    for name, t, dtype in (("mask", mask, (torch.uint8, np.uint8)), ("labels", labels, (torch.int32, np.int32))):
        if (t is not None or name == "mask") and (not isinstance(t, (torch.Tensor, np.ndarray)) or t.dtype not in dtype or t.ndim != 2):
            raise ValueError(f"measure_objects: {name} must be a {dtype[0]} [H, W] tensor or array, got {getattr(t, 'dtype', type(t).__name__)} "
                             f"{tuple(getattr(t, 'shape', ()))}")
    H, W = ops.check_objects_shape("measure_objects", tuple(mask.shape))
    if labels is not None and tuple(labels.shape) != (H, W):
        raise ValueError(f"measure_objects: labels has shape {tuple(labels.shape)}, the mask {(H, W)}")
    if not torch.cuda.is_available():
        raise ValueError("measure_objects runs on the GPU and there is no device (it has no host fallback)")
    dev = next((t.device for t in (mask, labels) if isinstance(t, torch.Tensor) and t.is_cuda), None)
    m = _plane(mask, torch.uint8, "mask", dev)
    dev = m.device
    if labels is None:
        from .postprocess import label_components
        lab = label_components(m, 4)
    else:
        lab = _plane(labels, torch.int32, "labels", dev)
    st = _Stages(stages)
    n = H * W
    offs, P, label, cls = _object_index(m, lab, exclude)
    st.mark("index")
    sums, bbox = _alloc((P, 5), torch.int64, dev), _alloc((P, 4), torch.int32, dev)
    point, bad = _alloc((P,), torch.int32, dev), _alloc((1,), torch.int64, dev)
    ops.obj_accumulate(m, lab, offs, exclude, P, sums if P else None, bbox if P else None, bad)
    st.mark("accumulate")
    if P:
        ops.obj_point(m, lab, offs, exclude, P, sums, bad, _alloc((P,), torch.int64, dev), point)
    word = ops.vec_read(bad, 0, 1)[0]          # the host read
    st.mark("point")
    if word & 1:
        raise ValueError(f"measure_objects: the labels hold a value outside 0..{n - 1}")
    if word & 2:
        raise ValueError("measure_objects: the labels are not canonical (labels[labels[p]] != labels[p] for some pixel p)")
    if word:
        raise ValueError("measure_objects: a pixel's class differs from the class of its label's anchor (mask[p] != mask[labels[p]])")
    return ObjectTable(label, cls, sums[:, 0], sums[:, 1], sums[:, 2], bbox, sums[:, 3], sums[:, 4], point, (H, W))


# ------------------------------------------------------------------------------------------------------------------ float planes

Q_BITS = 30          # |q| <= 2^30, as zonal.Q_BITS


@dataclass
class ObjectValues:
    """the tables of object_values, one entry per object of measure_objects in its order (the module docstring has the rules): tables of
    one shift add up, min and max combine by minimum and maximum"""
    label: torch.Tensor            # int32 [P]     the anchor L
    valid: torch.Tensor            # int64 [P]     the pixels with a finite value other than nodata
    sum_q: torch.Tensor            # int64 [P]
    sq_lo: torch.Tensor            # int64 [P]
    sq_hi: torch.Tensor            # int64 [P]
    min: torch.Tensor              # float32 [P]   +inf without a valid pixel
    max: torch.Tensor              # float32 [P]   -inf without a valid pixel
    argmin: torch.Tensor           # int32 [P]     the smallest linear index that attains min, -1 without a valid pixel
    argmax: torch.Tensor           # int32 [P]
    shift: int = 0                 # q = rint(v * 2^shift)
    shape: tuple = (0, 0)          # (H, W) of the raster

    @staticmethod
    def of_table(label: torch.Tensor, table: torch.Tensor, shift: int, shape: tuple) -> "ObjectValues":
        """from the int64 [6, P] table of ops.obj_values: rows 4 and 5 hold the float bits in the low half and the index in the high half"""
        halves = table[4:6].view(torch.int32).view(2, table.shape[1], 2)          # little-endian words
        return ObjectValues(label, table[0], table[1], table[2], table[3], halves[0, :, 0].view(torch.float32), halves[1, :, 0].view(torch.float32),
                            halves[0, :, 1], halves[1, :, 1], int(shift), tuple(shape))

    def cpu(self) -> "ObjectValues":
        return ObjectValues(**{f.name: (v.cpu() if isinstance(v, torch.Tensor) else v) for f in fields(self) for v in (getattr(self, f.name),)})

    @property
    def n_objects(self) -> int:
        return int(self.label.shape[0])


def object_values(mask, values, labels=None, exclude=None, nodata=None, shift: Optional[int] = None, stages: Optional[dict] = None) -> ObjectValues:
    """ObjectValues (device tensors) of a class mask (uint8 [H, W]), a value plane (float32 [H, W]) and a label image (int32 [H, W], or None:
    the 4-connected components) under the rules of the module docstring: the objects are those of measure_objects(mask, labels, exclude).
    nodata: a number whose pixels are not valid, or None.  shift: None derives it from the largest |value| of the valid pixels (one more pass
    and one host read); an int fixes it, and a valid pixel with |q| > 2^30 is then a ValueError.  Host inputs are uploaded.  ValueError for
    labels that break the convention (read from the device after the launches) and for every limit (before them).  stages: a dict that
    receives the milliseconds of `index`, `absmax` and `values` (this synchronises the device after each: for measurements only)."""
    what = "object_values"
    exclude = check_exclude(exclude)
    for name, t, dtype in (("mask", mask, (torch.uint8, np.uint8)), ("values", values, (torch.float32, np.float32)),
                           ("labels", labels, (torch.int32, np.int32))):
        if (t is not None or name != "labels") and (not isinstance(t, (torch.Tensor, np.ndarray)) or t.dtype not in dtype or t.ndim != 2):
            raise ValueError(f"{what}: {name} must be a {dtype[0]} [H, W] tensor or array, got {getattr(t, 'dtype', type(t).__name__)} "
                             f"{tuple(getattr(t, 'shape', ()))}")
    H, W = ops.check_objects_shape(what, tuple(mask.shape))
    for name, t in (("values", values), ("labels", labels)):
        if t is not None and tuple(t.shape) != (H, W):
            raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, the mask {(H, W)}")
    ops.check_zonal_nodata(what, nodata)
    if shift is not None:
        ops.check_zonal_shift(what, shift)
    if not torch.cuda.is_available():
        raise ValueError(f"{what} runs on the GPU and there is no device (it has no host fallback)")
    from .zonal import shift_of_absmax
    dev = next((t.device for t in (mask, values, labels) if isinstance(t, torch.Tensor) and t.is_cuda), None)
    m = _plane(mask, torch.uint8, "mask", dev)
    dev = m.device
    v = _plane(values, torch.float32, "values", dev)
    if labels is None:
        from .postprocess import label_components
        lab = label_components(m, 4)
    else:
        lab = _plane(labels, torch.int32, "labels", dev)
    st = _Stages(stages)
    offs, P, label, _ = _object_index(m, lab, exclude)
    st.mark("index")
    words = _alloc((2,), torch.int64, dev)          # the largest |v|, the bad word
    if shift is None:
        ops.obj_absmax(m, v, exclude, nodata, words[0:1])
        shift = shift_of_absmax(ops.vec_read(words, 0, 1)[0])          # a host read
        st.mark("absmax")
    table = _alloc((6, P), torch.int64, dev)
    ops.obj_values(m, lab, v, offs, exclude, P, nodata, shift, table if P else None, words[1:2])
    word = ops.vec_read(words, 1, 1)[0]          # the host read
    st.mark("values")
    n = H * W
    if word & 1:
        raise ValueError(f"{what}: the labels hold a value outside 0..{n - 1}")
    if word & 2:
        raise ValueError(f"{what}: the labels are not canonical (labels[labels[p]] != labels[p] for some pixel p)")
    if word & 4:
        raise ValueError(f"{what}: a pixel's class differs from the class of its label's anchor (mask[p] != mask[labels[p]])")
    if word:
        raise ValueError(f"{what}: a value times 2^{shift} exceeds 2^{Q_BITS}: shift={shift} is too large for this plane")
    return ObjectValues.of_table(label, table, shift, (H, W))


def object_value_rows(stats, geotransform=None, name: str = "value") -> list:
    """One ordered dict per object of an ObjectValues (device or host): <name>_valid, <name>_mean, <name>_std (population), <name>_sum,
    <name>_min, <name>_max and <name>_peak_x, <name>_peak_y, the centre of the argmax pixel in map units (in pixels without a geotransform).
    The sums are Python integers up to one division, exactly as zonal.zonal_value_rows: mean = sum_q / valid * 2^-s, std = sqrt(SQ * valid -
    sum_q^2) / valid * 2^-s with SQ = sq_hi * 2^30 + sq_lo, sum = sum_q * 2^-s.  An object without a valid pixel has None for all of them."""
    check_geojson_args(geotransform)
    if not isinstance(name, str) or not name:
        raise ValueError(f"name must be a non-empty string, got {name!r}")
    host = [(t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)) for t in
            (stats.valid, stats.sum_q, stats.sq_lo, stats.sq_hi, stats.min, stats.max, stats.argmax)]
    if any(a.ndim != 1 or a.shape != host[0].shape for a in host):
        raise ValueError(f"the tables must be [P] each, got {[a.shape for a in host]}")
    W = int(stats.shape[1])
    gt = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0) if geotransform is None else tuple(float(x) for x in geotransform)
    s = int(stats.shift)
    keys = [f"{name}_{k}" for k in ("valid", "mean", "std", "sum", "min", "max", "peak_x", "peak_y")]
    rows = []
    for valid, sum_q, lo, hi, mn, mx, peak in zip(*(a.tolist() for a in host)):
        if valid:
            sq = (hi << Q_BITS) + lo
            cells = (valid, math.ldexp(sum_q / valid, -s), math.ldexp(math.sqrt(sq * valid - sum_q * sum_q) / valid, -s),
                     math.ldexp(float(sum_q), -s), mn, mx, gt[0] + (peak % W + 0.5) * gt[1], gt[3] + (peak // W + 0.5) * gt[5])
        else:
            cells = (None,) * 8
        rows.append(dict(zip(keys, cells)))
    return rows


# ------------------------------------------------------------------------------------------------------------------ rows and files (host)

_TABLE_ARRAYS = ("label", "cls", "pixels", "sum_x", "sum_y", "bbox", "edges_v", "edges_h", "point")


def _host_table(table) -> dict:
    """ObjectTable (device or host) or a mapping of arrays -> NumPy arrays and the raster's shape"""
    out = {}
    for k in _TABLE_ARRAYS:
        v = table[k] if isinstance(table, dict) else getattr(table, k)
        out[k] = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    shape = table["shape"] if isinstance(table, dict) else table.shape
    out["shape"] = (int(shape[0]), int(shape[1]))
    return out


def object_rows(table, geotransform=None, codes=None, class_zero: bool = False, instance=None, values=None) -> list:
    """One ordered dict per object, in ascending label order: class (the id as the raster on disk holds it: class - 1 under
    class_zero), name (codes[class], if codes are given), pixels, area (pixels |gt1 gt5|), perimeter (edges_h |gt1| + edges_v |gt5|),
    centroid_x = gt0 + (sum_x / pixels + 0.5) gt1 and centroid_y likewise (pixel centres, float64), bbox [xmin, ymin, xmax, ymax] in map
    units, diameter 2 sqrt(area / pi), compactness 4 pi area / perimeter^2, point_x, point_y (the centre of the representative pixel),
    on_edge (the bbox touches the raster frame) and instance (one id per object) when given.  Without a geotransform the units are pixels.
    values: None or a mapping {name: ObjectValues} of tables of the same objects (object_values on the same mask, labels and exclude);
    the keys of object_value_rows(stats, geotransform, name) follow in the mapping's order."""
    check_geojson_args(geotransform)
    a = _host_table(table)
    added = []
    for name, stats in (values or {}).items():
        theirs = stats.label.cpu().numpy() if isinstance(stats.label, torch.Tensor) else np.asarray(stats.label)
        if tuple(stats.shape) != a["shape"] or not np.array_equal(theirs, a["label"]):
            raise ValueError(f"values[{name!r}] is not a table of the same objects (its labels or its raster shape differ)")
        added.append(object_value_rows(stats, geotransform, name))
    H, W = a["shape"]
    gt = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0) if geotransform is None else tuple(float(v) for v in geotransform)
    P = len(a["label"])
    if codes is not None and P and int(a["cls"].max()) >= len(codes):
        raise ValueError(f"codes names {len(codes)} classes, the objects hold class {int(a['cls'].max())}")
    inst = None if instance is None else (instance.cpu().numpy() if isinstance(instance, torch.Tensor) else np.asarray(instance)).tolist()
    if inst is not None and len(inst) != P:
        raise ValueError(f"instance holds {len(inst)} ids for {P} objects")
    rows = []
    for k in range(P):
        cls, pixels = int(a["cls"][k]), int(a["pixels"][k])
        x0, y0, x1, y1 = (int(v) for v in a["bbox"][k])
        point = int(a["point"][k])
        row = {"class": cls - 1 if class_zero else cls}
        if codes is not None:
            row["name"] = str(codes[cls])
        area = pixels * abs(gt[1] * gt[5])
        perimeter = int(a["edges_h"][k]) * abs(gt[1]) + int(a["edges_v"][k]) * abs(gt[5])
        xs, ys = sorted((gt[0] + x0 * gt[1], gt[0] + x1 * gt[1])), sorted((gt[3] + y0 * gt[5], gt[3] + y1 * gt[5]))
        row.update(pixels=pixels, area=area, perimeter=perimeter,
                   centroid_x=gt[0] + (int(a["sum_x"][k]) / pixels + 0.5) * gt[1], centroid_y=gt[3] + (int(a["sum_y"][k]) / pixels + 0.5) * gt[5],
                   bbox=[xs[0], ys[0], xs[1], ys[1]], diameter=2.0 * math.sqrt(area / math.pi),
                   compactness=4.0 * math.pi * area / (perimeter * perimeter),
                   point_x=gt[0] + (point % W + 0.5) * gt[1], point_y=gt[3] + (point // W + 0.5) * gt[5],
                   on_edge=bool(x0 == 0 or y0 == 0 or x1 == W or y1 == H))
        if inst is not None:
            row["instance"] = int(inst[k])
        for more in added:
            row.update(more[k])
        rows.append(row)
    return rows


def rows_by_label(table, rows) -> dict:
    """the attributes= argument of vectorize.write_geojson: the rows of object_rows(table, ...) keyed by the objects' labels"""
    return dict(zip(_host_table(table)["label"].tolist(), rows))


def write_objects(path, table_or_rows, geotransform=None, epsg=None, codes=None, class_zero: bool = False, instance=None, values=None) -> int:
    """The rows of object_rows (or such rows themselves) as a file; the suffix decides: .geojson -- one FeatureCollection with one Point
    feature per object at (point_x, point_y), the row as its properties, in ascending label order, with the "crs" member as
    vectorize.write_geojson writes it; .csv -- one row per object (bbox as xmin, ymin, xmax, ymax; None as an empty field).  Under class_zero
    class 0 -- NO_Data -- gets no feature.  values: object_rows' mapping of float tables, for a table.  Returns the number of objects
    written.  Host code."""
    suffix = os.path.splitext(os.fspath(path))[1].lower()
    if suffix not in (".geojson", ".csv"):
        raise ValueError(f"{path}: the object table is written as .geojson or .csv")
    check_geojson_args(geotransform, epsg)
    rows = table_or_rows if isinstance(table_or_rows, list) else object_rows(table_or_rows, geotransform, codes, class_zero, instance, values)
    if class_zero:
        rows = [row for row in rows if row["class"] >= 0]
    if suffix == ".geojson":
        feats = ['{"type":"Feature","properties":' + json.dumps(row) + ',"geometry":{"type":"Point","coordinates":[' +
                 f"{row['point_x']!r},{row['point_y']!r}" + "]}}" for row in rows]
        head = '{"type":"FeatureCollection",'
        if epsg is not None:
            head += '"crs":{"type":"name","properties":{"name":"urn:ogc:def:crs:EPSG::%d"}},' % int(epsg)
        with open(os.fspath(path), "w") as f:
            f.write(head + '"features":[\n' + ",\n".join(feats) + "\n]}\n")
        return len(rows)
    names = []
    for k in (rows[0] if rows else ()):
        names += ["xmin", "ymin", "xmax", "ymax"] if k == "bbox" else [k]
    with open(os.fspath(path), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(names)
        for row in rows:
            cells = []
            for k, v in row.items():
                cells += [repr(c) for c in v] if k == "bbox" else [repr(v) if isinstance(v, float) else "" if v is None else v]
            w.writerow(cells)
    return len(rows)


# ------------------------------------------------------------------------------------------------------------------ entry points

def check_objects(objects, objects_exclude=None, class_zero: bool = False) -> Optional[tuple]:
    """the objects_path= / objects= and objects_exclude= arguments of predict_raster / save_predictions -> the classes to exclude (a tuple),
    or None when no object table is wanted.  Under class_zero class 0 -- NO_Data -- is always excluded.  Which outputs can be measured is
    predict.check_outputs' rule"""
    if objects is None or objects is False:
        if objects_exclude is not None:
            raise ValueError("objects_exclude without an objects output")
        return None
    if objects is not True and not isinstance(objects, (str, os.PathLike)):
        raise ValueError(f"objects must be None, a bool or the path of the file to write, got {type(objects).__name__}")
    exclude = check_exclude(objects_exclude)
    return tuple(sorted(set(exclude) | {0})) if class_zero else exclude


def check_object_planes(values, name="value", confidence=False, objects: bool = False) -> Optional[str]:
    """the objects_values_path= / objects_values=, objects_values_name= and objects_confidence= arguments of predict_raster / save_predictions
    -> the prefix of the value raster's columns, or None when no value raster is given.  objects: whether an objects output is asked for;
    both options need one"""
    if values is not None and not isinstance(values, (str, os.PathLike)):
        raise ValueError(f"objects_values must be None or the path of a GeoTIFF, got {type(values).__name__}")
    if values is not None and not objects:
        raise ValueError("objects_values without an objects output")
    if confidence and not objects:
        raise ValueError("objects_confidence without an objects output")
    if not isinstance(name, str) or not name:
        raise ValueError(f"objects_values_name must be a non-empty string, got {name!r}")
    if values is not None and confidence and name == "confidence":
        raise ValueError("objects_values_name 'confidence' is taken by objects_confidence")
    return name if values is not None else None


_VALUE_RASTER_TYPES = ("float32", "uint8", "uint16", "int16")          # float32 as it is; the integers convert to float32 exactly


def read_value_raster(path, shape, geotransform=None) -> tuple:
    """(float32 [H, W] array, nodata or None) of a one-band GeoTIFF that lies on the grid of the output: `shape` and, where the output is
    georeferenced, its six geotransform numbers exactly -- there is no resampling, and a mismatch is a ValueError that names both grids.
    float32 is taken as it is; uint8, uint16 and int16 are converted to float32 (exact); any other sample type is a ValueError.  nodata is the
    file's.  Host code on tiffio.read_tiff."""
    from .tiffio import read_tiff
    a, meta = read_tiff(path)
    if a.ndim != 2:
        raise ValueError(f"{path}: the value raster must have one band, got {a.shape[0]}")
    ours = None if geotransform is None else tuple(float(v) for v in geotransform)
    theirs = meta.get("geotransform")
    theirs = None if theirs is None else tuple(float(v) for v in theirs)
    if tuple(a.shape) != tuple(shape) or (ours is not None and theirs != ours):
        raise ValueError(f"{path}: the value raster is {a.shape[0]} x {a.shape[1]} px with geotransform {theirs}, the output {shape[0]} x {shape[1]} px "
                         f"with {ours} (there is no resampling)")
    if a.dtype.name not in _VALUE_RASTER_TYPES:
        raise ValueError(f"{path}: the value raster holds {a.dtype.name} samples; float32, uint8, uint16 and int16 are read")
    return np.ascontiguousarray(a, dtype=np.float32), meta.get("nodata")


def objects_mask(mask, path, exclude=(), geotransform=None, epsg=None, codes=None, class_zero: bool = False, labels=None, ids=None,
                 timing: Optional[dict] = None, values=None) -> dict:
    """The output stage of an assembled class mask (device or host): measure_objects -- of `labels` where given (the instance labels, with
    ids their dense ids per pixel, written as `instance`), else of the 4-connected components --, one copy of the table to the host,
    object_rows, write_objects.  values: None or a mapping {name: (float32 [H, W] plane on the mask's grid, nodata or None)}: object_values
    of every plane on the same mask and labels, its columns <name>_* behind the others.  timing gains objects_seconds and objects (the
    number written), with values also objects_values_seconds.  Returns the rows keyed by label (the attributes= argument of
    vectorize.write_geojson)."""
    t0 = time.perf_counter()
    if values and labels is None:          # one labelling for the table and the planes
        from .postprocess import label_components
        mask = _plane(mask, torch.uint8, "mask")
        labels = label_components(mask, 4)
    table = measure_objects(mask, labels, exclude)
    instance = None if ids is None else ids.view(-1)[table.label.to(torch.int64)]
    table = table.cpu()
    stats = None
    if values:
        t1 = time.perf_counter()
        stats = {name: object_values(mask, plane, labels, exclude, nodata).cpu() for name, (plane, nodata) in values.items()}
        if timing is not None:
            timing["objects_values_seconds"] = time.perf_counter() - t1
    rows = object_rows(table, geotransform, codes, class_zero, instance, stats)
    n = write_objects(path, rows, geotransform, epsg, class_zero=class_zero)
    if timing is not None:
        timing.update(objects_seconds=time.perf_counter() - t0, objects=n)
    return rows_by_label(table, rows)
