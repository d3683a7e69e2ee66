"""Plain Python restatement of the burning rules (unet_amd/rasterize.py): sequential, Python ints only, written for small rasters.  The
pixel centre decides, the fill is even-odd over all rings of a feature, the feature with the highest index wins.  Vertices are fixed point
with 8 fractional bits."""
import math

import numpy as np

ONE = 256
HALF = 128
MAX_COORD = 2 ** 21 * ONE


def quantise(v: float) -> int:
    """floor(256 v + 0.5)"""
    return int(math.floor(256.0 * float(v) + 0.5))


def ceil_div(a: int, b: int) -> int:
    """ceil(a / b) for b > 0 by a floor division"""
    assert b > 0
    return -((-a) // b)


def ring_crossings(ring, H: int, W: int):
    """[(row, k)] of one ring [(X, Y), ...] in fixed point: for every edge and every row y of 0 .. H - 1 with min(Y0, Y1) <= 256 y + 128 <
    max(Y0, Y1), the first column k (clamped to 0 .. W) whose centre lies at or right of the crossing"""
    n = len(ring)
    out = []
    if n < 3:
        return out
    for i in range(n):
        (X0, Y0), (X1, Y1) = ring[i], ring[(i + 1) % n]
        X0, Y0, X1, Y1 = int(X0), int(Y0), int(X1), int(Y1)
        assert max(abs(X0), abs(Y0), abs(X1), abs(Y1)) <= MAX_COORD
        lo, hi = min(Y0, Y1), max(Y0, Y1)
        for y in range(max(0, ceil_div(lo - HALF, ONE)), min(H, ceil_div(hi - HALF, ONE))):
            Yc = ONE * y + HALF
            assert lo <= Yc < hi
            num, den = (Yc - Y0) * (X1 - X0), Y1 - Y0
            if den < 0:
                num, den = -num, -den
            # X* = X0 + num / den; k = ceil((X* - 128) / 256) = ceil(((X0 - 128) den + num) / (256 den))
            k = ceil_div((X0 - HALF) * den + num, ONE * den)
            out.append((y, min(max(k, 0), W)))
    return out


def feature_rows(rings, H: int, W: int) -> dict:
    """{row: [columns]}: the pixels inside the even-odd fill of the rings of one feature.  Every crossing toggles the columns >= its k; left
    of the smallest k of a row nothing is toggled and right of the largest an even number of times, so only the columns between them are
    walked"""
    by_row = {}
    for ring in rings:
        for y, k in ring_crossings(ring, H, W):
            by_row.setdefault(y, []).append(k)
    rows = {}
    for y, ks in by_row.items():
        assert len(ks) % 2 == 0, (y, ks)          # a closed ring crosses a row centre an even number of times
        toggles = {}
        for k in ks:
            toggles[k] = toggles.get(k, 0) ^ 1
        state, inside = 0, []
        for x in range(min(ks), min(max(ks), W)):
            state ^= toggles.get(x, 0)
            if state:
                inside.append(x)
        rows[y] = inside
    return rows


def feature_mask(rings, H: int, W: int) -> np.ndarray:
    """bool [H, W]: the pixels inside the even-odd fill of the rings of one feature"""
    inside = np.zeros((H, W), dtype=bool)
    for y, xs in feature_rows(rings, H, W).items():
        inside[y, xs] = True
    return inside


def rasterize(xy, ring_start, feature_ring_start, values, shape, fill: int = 0, out=None) -> np.ndarray:
    """uint8 [H, W]: features painted in index order over `fill`, or over a copy of `out`"""
    H, W = shape
    xy = [(int(x), int(y)) for x, y in np.asarray(xy).reshape(-1, 2).tolist()]
    rs, frs, vals = [int(v) for v in ring_start], [int(v) for v in feature_ring_start], [int(v) for v in values]
    res = np.full((H, W), fill, dtype=np.uint8) if out is None else np.array(out, dtype=np.uint8, copy=True)
    for f in range(len(vals)):
        rings = [xy[rs[r]:rs[r + 1]] for r in range(frs[f], frs[f + 1])]
        for y, xs in feature_rows(rings, H, W).items():
            res[y, xs] = vals[f]
    return res


def rings_of_polygons(p: dict, values=None):
    """(xy, ring_start, feature_ring_start, values) of the arrays of vectorize_ref.polygonize: the poly_rings indirection resolved, the
    pixel corners scaled by 256"""
    xy, rs, frs = [], [0], [0]
    for i in range(len(p["poly_label"])):
        for r in p["poly_rings"][p["poly_ring_start"][i]:p["poly_ring_start"][i + 1]]:
            xy += [(int(x) * ONE, int(y) * ONE) for x, y in p["xy"][p["ring_start"][r]:p["ring_start"][r + 1]]]
            rs.append(len(xy))
        frs.append(len(rs) - 1)
    vals = p["poly_class"] if values is None else values
    return (np.array(xy, dtype=np.int32).reshape(-1, 2), np.array(rs, dtype=np.int64), np.array(frs, dtype=np.int64),
            np.asarray(vals, dtype=np.uint8))


def pack(features):
    """[(value, [ring, ...]), ...] with rings as [(X, Y), ...] in fixed point -> (xy, ring_start, feature_ring_start, values)"""
    xy, rs, frs, vals = [], [0], [0], []
    for value, rings in features:
        for ring in rings:
            xy += [(int(x), int(y)) for x, y in ring]
            rs.append(len(xy))
        frs.append(len(rs) - 1)
        vals.append(value)
    return (np.array(xy, dtype=np.int32).reshape(-1, 2), np.array(rs, dtype=np.int64), np.array(frs, dtype=np.int64),
            np.array(vals, dtype=np.uint8))
