"""Sequential restatement of the rules of unet_amd/objects.py in plain Python / NumPy: `table` is one plain loop over the pixels, `point` the
lexicographic minimum written out, `rows` the derivation of the written attributes.  `table_fast` states the same table with NumPy's
keyed reductions for the rasters that are too large for a Python loop; tests/test_objects_cpu.py holds the two equal on the small cases.
Everything is exact integer arithmetic.  Labels come from tests/postprocess_ref.label_components (4-adjacency) unless a test makes its own."""
import math

import numpy as np

FIELDS = ("label", "cls", "pixels", "sum_x", "sum_y", "bbox", "edges_v", "edges_h", "point")
BAD_RANGE, BAD_CANONICAL, BAD_CLASS = 1, 2, 4


def exclude_set(exclude):
    if exclude is None:
        return set()
    if isinstance(exclude, (int, np.integer)):
        return {int(exclude)}
    return {int(c) for c in exclude}


def bad_bits(mask: np.ndarray, labels: np.ndarray) -> int:
    """the word of the Bad input rule: bit 0 a label outside 0 .. H W - 1, bit 1 labels[labels[p]] != labels[p], bit 2 mask[p] != mask[labels[p]]"""
    n = mask.size
    lab, m = labels.ravel().tolist(), mask.ravel().tolist()
    word = 0
    for p in range(n):
        L = lab[p]
        if not 0 <= L < n:
            word |= BAD_RANGE
        elif lab[L] != L:
            word |= BAD_CANONICAL
        elif m[L] != m[p]:
            word |= BAD_CLASS
    return word


def _arrays(label, cls, pixels, sum_x, sum_y, bbox, edges_v, edges_h, point, shape) -> dict:
    return {"label": np.array(label, dtype=np.int32).reshape(-1), "cls": np.array(cls, dtype=np.uint8).reshape(-1),
            "pixels": np.array(pixels, dtype=np.int64).reshape(-1), "sum_x": np.array(sum_x, dtype=np.int64).reshape(-1),
            "sum_y": np.array(sum_y, dtype=np.int64).reshape(-1), "bbox": np.array(bbox, dtype=np.int32).reshape(-1, 4),
            "edges_v": np.array(edges_v, dtype=np.int64).reshape(-1), "edges_h": np.array(edges_h, dtype=np.int64).reshape(-1),
            "point": np.array(point, dtype=np.int32).reshape(-1), "shape": (int(shape[0]), int(shape[1]))}


def table(mask: np.ndarray, labels: np.ndarray, exclude=None) -> dict:
    """the ObjectTable as NumPy arrays (plus "shape"), by one loop over the pixels and one more for the point"""
    H, W = mask.shape
    n = H * W
    excl = exclude_set(exclude)
    lab, m = labels.ravel().tolist(), mask.ravel().tolist()
    anchors = [L for L in range(n) if lab[L] == L and m[L] not in excl]
    index = {L: k for k, L in enumerate(anchors)}
    P = len(anchors)
    pixels, sum_x, sum_y, edges_v, edges_h = ([0] * P for _ in range(5))
    bbox = [[W, H, 0, 0] for _ in range(P)]
    for p in range(n):
        k = index.get(lab[p])
        if k is None:
            continue
        y, x = divmod(p, W)
        pixels[k] += 1
        sum_x[k] += x
        sum_y[k] += y
        b = bbox[k]
        b[0], b[1], b[2], b[3] = min(b[0], x), min(b[1], y), max(b[2], x + 1), max(b[3], y + 1)
        if x == 0 or lab[p - 1] != lab[p]:
            edges_v[k] += 1
        if x == W - 1 or lab[p + 1] != lab[p]:
            edges_v[k] += 1
        if y == 0 or lab[p - W] != lab[p]:
            edges_h[k] += 1
        if y == H - 1 or lab[p + W] != lab[p]:
            edges_h[k] += 1
    best = [None] * P
    for p in range(n):
        k = index.get(lab[p])
        if k is None:
            continue
        y, x = divmod(p, W)
        cx, cy = sum_x[k] // pixels[k], sum_y[k] // pixels[k]
        key = ((x - cx) ** 2 + (y - cy) ** 2, p)
        if best[k] is None or key < best[k]:
            best[k] = key
    return _arrays(anchors, [m[L] for L in anchors], pixels, sum_x, sum_y, bbox, edges_v, edges_h, [b[1] for b in best], (H, W))


def table_fast(mask: np.ndarray, labels: np.ndarray, exclude=None) -> dict:
    """the same table by NumPy's keyed reductions (int64 throughout), for rasters of millions of pixels"""
    H, W = mask.shape
    n = H * W
    flat, m = labels.ravel().astype(np.int64), mask.ravel()
    kept = ~np.isin(m, sorted(exclude_set(exclude)))
    anchors = np.flatnonzero((flat == np.arange(n)) & kept)
    P = len(anchors)
    index = np.full(n, -1, dtype=np.int64)
    index[anchors] = np.arange(P)
    k = index[flat]
    sel = k >= 0
    p = np.arange(n, dtype=np.int64)
    yy, xx = np.divmod(p, W)
    lab2 = labels.reshape(H, W)
    ev, eh = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    ev[:, 0] += 1
    ev[:, -1] += 1
    eh[0] += 1
    eh[-1] += 1
    dv, dh = (lab2[:, 1:] != lab2[:, :-1]), (lab2[1:] != lab2[:-1])
    ev[:, 1:] += dv
    ev[:, :-1] += dv
    eh[1:] += dh
    eh[:-1] += dh
    ks = k[sel]

    def total(values):
        out = np.zeros(P, dtype=np.int64)
        np.add.at(out, ks, values[sel])
        return out

    pixels, sum_x, sum_y = total(np.ones(n, dtype=np.int64)), total(xx), total(yy)
    edges_v, edges_h = total(ev.ravel()), total(eh.ravel())
    bbox = np.empty((P, 4), dtype=np.int64)
    bbox[:, 0], bbox[:, 1], bbox[:, 2], bbox[:, 3] = W, H, 0, 0
    np.minimum.at(bbox[:, 0], ks, xx[sel])
    np.minimum.at(bbox[:, 1], ks, yy[sel])
    np.maximum.at(bbox[:, 2], ks, xx[sel] + 1)
    np.maximum.at(bbox[:, 3], ks, yy[sel] + 1)
    cx, cy = sum_x // np.maximum(pixels, 1), sum_y // np.maximum(pixels, 1)
    d2 = (xx[sel] - cx[ks]) ** 2 + (yy[sel] - cy[ks]) ** 2
    ps = p[sel]
    order = np.lexsort((ps, d2, ks))
    first = np.ones(len(order), dtype=bool)
    first[1:] = ks[order][1:] != ks[order][:-1]
    point = np.empty(P, dtype=np.int64)
    point[ks[order][first]] = ps[order][first]
    return _arrays(anchors, m[anchors], pixels, sum_x, sum_y, bbox, edges_v, edges_h, point, (H, W))


def same(a: dict, b: dict) -> bool:
    return all(np.array_equal(a[f], b[f]) and a[f].dtype == b[f].dtype for f in FIELDS)


def host(table_obj) -> dict:
    """an unet_amd.objects.ObjectTable as the dict of arrays that `table` returns"""
    t = table_obj.cpu()
    out = {f: getattr(t, f).numpy() for f in FIELDS}
    out["shape"] = tuple(t.shape)
    return out


def rows(t: dict, geotransform=None, codes=None, class_zero=False, instance=None) -> list:
    """the written attributes of every object, in the order of the module's object_rows"""
    H, W = t["shape"]
    g = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0) if geotransform is None else tuple(float(v) for v in geotransform)
    out = []
    for k in range(len(t["label"])):
        cls, px = int(t["cls"][k]), int(t["pixels"][k])
        x0, y0, x1, y1 = (int(v) for v in t["bbox"][k])
        py, pxx = divmod(int(t["point"][k]), W)
        area = px * abs(g[1] * g[5])
        perimeter = int(t["edges_h"][k]) * abs(g[1]) + int(t["edges_v"][k]) * abs(g[5])
        xa, xb, ya, yb = g[0] + x0 * g[1], g[0] + x1 * g[1], g[3] + y0 * g[5], g[3] + y1 * g[5]
        row = {"class": cls - 1 if class_zero else cls}
        if codes is not None:
            row["name"] = str(codes[cls])
        row["pixels"] = px
        row["area"] = area
        row["perimeter"] = perimeter
        row["centroid_x"] = g[0] + (int(t["sum_x"][k]) / px + 0.5) * g[1]
        row["centroid_y"] = g[3] + (int(t["sum_y"][k]) / px + 0.5) * g[5]
        row["bbox"] = [min(xa, xb), min(ya, yb), max(xa, xb), max(ya, yb)]
        row["diameter"] = 2.0 * math.sqrt(area / math.pi)
        row["compactness"] = 4.0 * math.pi * area / (perimeter * perimeter)
        row["point_x"] = g[0] + (pxx + 0.5) * g[1]
        row["point_y"] = g[3] + (py + 0.5) * g[5]
        row["on_edge"] = bool(x0 == 0 or y0 == 0 or x1 == W or y1 == H)
        if instance is not None:
            row["instance"] = int(instance[k])
        out.append(row)
    return out


def ring_lengths(polys: dict) -> np.ndarray:
    """int64 [P]: the summed Manhattan length of the rings of every polygon of a Polygons-like dict of arrays (closed rings)"""
    xy, rs = np.asarray(polys["xy"]).astype(np.int64), np.asarray(polys["ring_start"]).tolist()
    prs, pr = np.asarray(polys["poly_ring_start"]).tolist(), np.asarray(polys["poly_rings"]).tolist()
    out = []
    for i in range(len(prs) - 1):
        total = 0
        for r in pr[prs[i]:prs[i + 1]]:
            v = xy[rs[r]:rs[r + 1]]
            total += int(np.abs(v - np.roll(v, -1, axis=0)).sum())
        out.append(total)
    return np.array(out, dtype=np.int64)
