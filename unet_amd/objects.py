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

object_rows and write_objects are host code on the json and csv modules.  Out of scope: second moments, orientation and ellipse axes (sum
x^2 can exceed 64 bits at the raster limits), statistics of float planes per object, the pole of inaccessibility (it needs a distance
transform on labels), 8-connectivity, per-tile outputs, tables across ranks (the stage runs on rank 0's assembled mask), Shapefile and
GeoPackage, and a host fallback."""
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
    kept = tuple(c for c in range(256) if c not in exclude)
    mark, offs = _alloc((H, W), torch.uint8, dev), _alloc((H, W), torch.int32, dev)
    blocks = _alloc((ops.vec_scan_words(n),), torch.int64, dev)
    ops.inst_marks(m, lab, kept, mark)
    ops.vec_scan(mark, offs, blocks)
    P = ops.vec_read(blocks, ops.vec_scan_words(n) - 1, 1)[0]          # a host read
    label, cls = _alloc((P,), torch.int32, dev), _alloc((P,), torch.uint8, dev)
    if P:
        ops.obj_compact(m, mark, offs, P, label, cls)
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


def object_rows(table, geotransform=None, codes=None, class_zero: bool = False, instance=None) -> list:
    """One ordered dict per object, in ascending label order: class (the id as the raster on disk holds it: class - 1 under
    class_zero), name (codes[class], if codes are given), pixels, area (pixels |gt1 gt5|), perimeter (edges_h |gt1| + edges_v |gt5|),
    centroid_x = gt0 + (sum_x / pixels + 0.5) gt1 and centroid_y likewise (pixel centres, float64), bbox [xmin, ymin, xmax, ymax] in map
    units, diameter 2 sqrt(area / pi), compactness 4 pi area / perimeter^2, point_x, point_y (the centre of the representative pixel),
    on_edge (the bbox touches the raster frame) and instance (one id per object) when given.  Without a geotransform the units are pixels."""
    check_geojson_args(geotransform)
    a = _host_table(table)
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
        rows.append(row)
    return rows


def rows_by_label(table, rows) -> dict:
    """the attributes= argument of vectorize.write_geojson: the rows of object_rows(table, ...) keyed by the objects' labels"""
    return dict(zip(_host_table(table)["label"].tolist(), rows))


def write_objects(path, table_or_rows, geotransform=None, epsg=None, codes=None, class_zero: bool = False, instance=None) -> int:
    """The rows of object_rows (or such rows themselves) as a file; the suffix decides: .geojson -- one FeatureCollection with one Point
    feature per object at (point_x, point_y), the row as its properties, in ascending label order, with the "crs" member as
    vectorize.write_geojson writes it; .csv -- one row per object (bbox as xmin, ymin, xmax, ymax).  Under class_zero class 0 -- NO_Data --
    gets no feature.  Returns the number of objects written.  Host code."""
    suffix = os.path.splitext(os.fspath(path))[1].lower()
    if suffix not in (".geojson", ".csv"):
        raise ValueError(f"{path}: the object table is written as .geojson or .csv")
    check_geojson_args(geotransform, epsg)
    rows = table_or_rows if isinstance(table_or_rows, list) else object_rows(table_or_rows, geotransform, codes, class_zero, instance)
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
                cells += [repr(c) for c in v] if k == "bbox" else [repr(v) if isinstance(v, float) else v]
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


def objects_mask(mask, path, exclude=(), geotransform=None, epsg=None, codes=None, class_zero: bool = False, labels=None, ids=None,
                 timing: Optional[dict] = None) -> dict:
    """The output stage of an assembled class mask (device or host): measure_objects -- of `labels` where given (the instance labels, with
    ids their dense ids per pixel, written as `instance`), else of the 4-connected components --, one copy of the table to the host,
    object_rows, write_objects.  timing gains objects_seconds and objects (the number written).  Returns the rows keyed by label (the
    attributes= argument of vectorize.write_geojson)."""
    t0 = time.perf_counter()
    table = measure_objects(mask, labels, exclude)
    instance = None if ids is None else ids.view(-1)[table.label.to(torch.int64)]
    table = table.cpu()
    rows = object_rows(table, geotransform, codes, class_zero, instance)
    n = write_objects(path, rows, geotransform, epsg, class_zero=class_zero)
    if timing is not None:
        timing.update(objects_seconds=time.perf_counter() - t0, objects=n)
    return rows_by_label(table, rows)
