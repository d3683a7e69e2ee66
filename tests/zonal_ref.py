"""NumPy restatement of the rules of unet_amd/zonal.py.

Zone plane  int32 [H, W]; -1 = no zone, zones 0 .. Z - 1; a pixel belongs to at most one zone.  Of polygon zones the rasterizer's rules
            decide (tests/rasterize_ref.py: pixel centre, even-odd fill, left / top border inside), the last feature wins, and only the
            pixels inside the raster count.
Counts      counts[z, c] = the pixels with zone z and mask value c, int64 [Z, C].
Objects     labels[p] = the smallest linear index of the object of pixel p; p is an anchor iff labels[p] == p; objects[z, c] = the anchors
            with zone z and class c: an object belongs to the zone of its first pixel in row-major order.
Bad input   a mask value >= C or a zone outside -1 .. Z - 1 is counted nowhere (the device call raises ValueError for it)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))

import rasterize_ref as RR  # noqa: E402


def _keys(zones, mask, Z: int, C: int):
    z, m = np.asarray(zones).astype(np.int64).ravel(), np.asarray(mask).astype(np.int64).ravel()
    assert z.shape == m.shape
    good = (z >= 0) & (z < Z) & (m < C)
    bad = bool(((z < -1) | (z >= Z) | (m >= C)).any())
    return z * C + m, good, bad


def counts(zones, mask, Z: int, C: int):
    """(int64 [Z, C], whether any pixel was bad)"""
    key, good, bad = _keys(zones, mask, Z, C)
    table = np.zeros(Z * C, dtype=np.int64)
    np.add.at(table, key[good], 1)
    return table.reshape(Z, C), bad


def objects(zones, mask, labels, Z: int, C: int) -> np.ndarray:
    """int64 [Z, C]: the anchors labels[p] == p per zone and class"""
    key, good, _ = _keys(zones, mask, Z, C)
    lab = np.asarray(labels).astype(np.int64).ravel()
    anchor = lab == np.arange(lab.size, dtype=np.int64)
    table = np.zeros(Z * C, dtype=np.int64)
    np.add.at(table, key[good & anchor], 1)
    return table.reshape(Z, C)


def ids(xy, ring_start, feature_ring_start, shape) -> np.ndarray:
    """int32 [H, W]: the index of the last feature whose even-odd fill holds the pixel's centre, -1 where there is none"""
    H, W = shape
    xy = [(int(x), int(y)) for x, y in np.asarray(xy).reshape(-1, 2).tolist()]
    rs, frs = [int(v) for v in ring_start], [int(v) for v in feature_ring_start]
    res = np.full((H, W), -1, dtype=np.int32)
    for f in range(len(frs) - 1):
        rings = [xy[rs[r]:rs[r + 1]] for r in range(frs[f], frs[f + 1])]
        for y, xs in RR.feature_rows(rings, H, W).items():
            res[y, xs] = f
    return res


def rows(count_table, object_table=None, names=None, pixel_area: float = 1.0, class_zero: bool = False) -> list:
    """the added properties of write_zonal per zone, restated: pixels, area, px_ / frac_ per class, majority, n_ per class"""
    out = []
    first = 1 if class_zero else 0
    for z, c in enumerate(np.asarray(count_table).tolist()):
        C = len(c)
        name = [("nodata" if class_zero and k == 0 else str(names[k]) if names is not None else str(k - first)) for k in range(C)]
        valid = sum(c[first:])
        row = {"pixels": sum(c), "area": sum(c) * pixel_area}
        for k in range(C):
            row["px_" + name[k]] = c[k]
            if k >= first:
                row["frac_" + name[k]] = c[k] / valid if valid else None
        row["majority"] = None
        for k in range(first, C):
            if valid and (row["majority"] is None or c[k] > c[row["majority"] + first]):
                row["majority"] = k - first
        if object_table is not None:
            for k in range(first, C):
                row["n_" + name[k]] = int(object_table[z][k])
        out.append(row)
    return out
