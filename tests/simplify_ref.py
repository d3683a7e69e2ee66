"""Plain Python restatement of the ring simplification rules (unet_amd/vectorize.py), written from the rules: nodes from the
label image, the candidates of every ring, arcs between nodes, closed arcs split at the point farthest from their anchor, and a sequential
Douglas-Peucker with the exact integer tolerance test.  The rings themselves come from tests/vectorize_ref.py.  Everything is Python
integer arithmetic; written for small rasters.  The checks at the end (segment balance, doubled areas, tolerance) do not use the tracer."""
import math

import numpy as np

import postprocess_ref as R
import vectorize_ref as V

ARRAYS = V.ARRAYS
MAX_TOLERANCE = 4096


def quantise(tolerance) -> int:
    """the tolerance in sixteenths of a pixel: q = floor(16 t + 0.5)"""
    t = float(tolerance)
    if not math.isfinite(t) or not 0 <= t <= MAX_TOLERANCE:
        raise ValueError(f"tolerance must be a finite number in 0..{MAX_TOLERANCE}, got {tolerance!r}")
    return int(math.floor(16.0 * t + 0.5))


def kept(c: int, d2: int, q: int) -> bool:
    """is a point with cross product c against a chord of squared length d2 farther than q / 16 from the chord's LINE?"""
    return 256 * c * c > q * q * d2


def node_map(lab, H: int, W: int):
    """is_node(x, y) for the pixel corners of a label image (nested lists); outside the raster is one label of its own"""
    def at(y, x):
        return lab[y][x] if 0 <= y < H and 0 <= x < W else -1

    def is_node(x, y):
        if x in (0, W) and y in (0, H):
            return True
        nw, ne, sw, se = at(y - 1, x - 1), at(y - 1, x), at(y, x - 1), at(y, x)
        return (nw != ne) + (sw != se) + (nw != sw) + (ne != se) >= 3
    return is_node


def ring_candidates(mask: np.ndarray, exclude=None):
    """-> (rings of vectorize_ref.trace, each with "cand": [(x, y, is_node), ...] in walk order from the leader on, info)"""
    H, W = mask.shape
    rings, info = V.trace(mask, exclude)
    is_node = node_map(R.label_components(mask, 4).tolist(), H, W)
    for r in rings:
        walk, cand = r["edges"], []
        for i, e in enumerate(walk):
            p, s = divmod(e, 4)
            x, y = V.end_vertex(p // W, p % W, s)
            node = is_node(x, y)
            if walk[(i + 1) % len(walk)] % 4 != s or node:
                cand.append((x, y, node))
        r["cand"] = cand
    return rings, info


def _yx(p):
    return (p[1], p[0])


def douglas_peucker(pts, q: int, keep: set, depth0: int = 0) -> int:
    """pts: the candidates (x, y, ...) of one open arc, both ends kept already; adds the kept interior indices to `keep` (as the points
    themselves, which are unique within a ring) and returns the recursion depth (0: no interior)"""
    deepest = 0
    stack = [(0, len(pts) - 1, 1)]
    while stack:
        i, j, depth = stack.pop()
        if j - i < 2:
            continue
        deepest = max(deepest, depth)
        (px, py), (qx, qy) = pts[i][:2], pts[j][:2]
        best, best_key = None, None
        for k in range(i + 1, j):
            zx, zy = pts[k][:2]
            c = (qx - px) * (zy - py) - (qy - py) * (zx - px)
            key = (-abs(c), zy, zx)
            if best_key is None or key < best_key:
                best, best_key = k, key
        d2 = (qx - px) ** 2 + (qy - py) ** 2
        if kept(-best_key[0], d2, q):
            keep.add(pts[best][:2])
            stack.append((i, best, depth + 1))
            stack.append((best, j, depth + 1))
    return depth0 + deepest


def simplify_ring(cand, q: int):
    """-> (kept vertices [(x, y), ...] in walk order, recursion depth, arcs with an interior that wrap past the first candidate)"""
    n = len(cand)
    nodes = [i for i, c in enumerate(cand) if c[2]]
    keep = {cand[i][:2] for i in nodes}
    arcs = []                                             # index lists, cyclic
    if len(nodes) >= 2:
        for a, b in zip(nodes, nodes[1:] + nodes[:1]):
            arcs.append([(a + t) % n for t in range((b - a) % n + 1)])
    else:
        a = nodes[0] if nodes else min(range(n), key=lambda i: _yx(cand[i]))
        ax, ay = cand[a][:2]
        far = min((i for i in range(n) if i != a), key=lambda i: (-((cand[i][0] - ax) ** 2 + (cand[i][1] - ay) ** 2), _yx(cand[i])))
        keep.add(cand[a][:2])
        keep.add(cand[far][:2])
        arcs.append([(a + t) % n for t in range((far - a) % n + 1)])
        arcs.append([(far + t) % n for t in range((a - far) % n + 1)])
    depth = wraps = 0
    for arc in arcs:
        depth = max(depth, douglas_peucker([cand[i] for i in arc], q, keep))
        if len(arc) > 2 and any(arc[t + 1] < arc[t] for t in range(len(arc) - 1)):
            wraps += 1
    return [c[:2] for c in cand if c[:2] in keep], depth, wraps


def area2(xy) -> int:
    """twice the signed area (positive: counter-clockwise on screen, y down)"""
    return sum(xy[(i + 1) % len(xy)][0] * xy[i][1] - xy[i][0] * xy[(i + 1) % len(xy)][1] for i in range(len(xy)))


def half(a2: int) -> int:
    """a2 / 2 rounded towards zero (a ring of integer vertices can have a half-integer area)"""
    return a2 // 2 if a2 >= 0 else -((-a2) // 2)


def prepare(mask: np.ndarray, exclude=None):
    """the part of simplify() that does not depend on the tolerance: pass it as `prepared` to share it between tolerances"""
    rings = ring_candidates(mask, exclude)[0]
    pixels = {}
    for r in rings:          # the signed areas of a component's traced rings sum to its pixel count
        pixels[r["label"]] = pixels.get(r["label"], 0) + r["area"]
    return rings, pixels


def simplify(mask: np.ndarray, tolerance, exclude=None, prepared=None) -> dict:
    """the arrays of unet_amd.vectorize.polygonize(mask, exclude, simplify=tolerance) as NumPy arrays, plus: "q", "depth" (the deepest
    recursion of any arc = the device's rounds), "wraps", "orphans" (holes that outlive their exterior; they are not in the output),
    "dropped_rings", "dropped_polygons", "raw_vertices" (the candidate count), "cand" / "label" / "leader" / "kept" per traced ring"""
    q = quantise(tolerance)
    H, W = mask.shape
    rings, pixels = prepared if prepared is not None else prepare(mask, exclude)
    out, depth, wraps = [], 0, 0
    for r in rings:
        xy, d, w = simplify_ring(r["cand"], q)
        depth, wraps = max(depth, d), wraps + w
        out.append(xy)
    alive = [len(xy) >= 3 for xy in out]
    exterior = {r["label"]: alive[i] for i, r in enumerate(rings) if r["leader"] == 4 * r["label"]}
    orphans = sum(1 for i, r in enumerate(rings) if alive[i] and not exterior[r["label"]])
    final = [i for i, r in enumerate(rings) if alive[i] and exterior[r["label"]]]
    new = {i: j for j, i in enumerate(final)}
    labels = sorted({rings[i]["label"] for i in final})
    order = sorted(final, key=lambda i: (rings[i]["label"], rings[i]["leader"]))
    counts = {l: 0 for l in labels}
    for i in final:
        counts[rings[i]["label"]] += 1
    flat = mask.ravel()
    return {
        "xy": np.array([v for i in final for v in out[i]], dtype=np.int32).reshape(-1, 2),
        "ring_start": np.cumsum([0] + [len(out[i]) for i in final]).astype(np.int64),
        "ring_label": np.array([rings[i]["label"] for i in final], dtype=np.int32).reshape(-1),
        "ring_area": np.array([half(area2(out[i])) for i in final], dtype=np.int64).reshape(-1),
        "poly_label": np.array(labels, dtype=np.int32).reshape(-1),
        "poly_class": np.array([flat[l] for l in labels], dtype=np.uint8).reshape(-1),
        "poly_pixels": np.array([pixels[l] for l in labels], dtype=np.int64).reshape(-1),
        "poly_ring_start": np.cumsum([0] + [counts[l] for l in labels]).astype(np.int64),
        "poly_rings": np.array([new[i] for i in order], dtype=np.int64).reshape(-1),
        "shape": (H, W), "q": q, "depth": depth, "wraps": wraps, "orphans": orphans, "dropped_rings": len(rings) - len(final),
        "dropped_polygons": len(pixels) - len(labels), "raw_vertices": sum(len(r["cand"]) for r in rings),
        "cand": [r["cand"] for r in rings], "label": [r["label"] for r in rings], "leader": [r["leader"] for r in rings], "kept": out,
        "final": final,
    }


# ------------------------------------------------------------------------------------------------------------ checks without the tracer

def ring_lists(polys: dict):
    """the vertex lists [(x, y), ...] of every ring of a set of Polygons arrays"""
    rs, xy = polys["ring_start"], polys["xy"]
    return [[(int(x), int(y)) for x, y in xy[rs[r]:rs[r + 1]]] for r in range(len(rs) - 1)]


def unbalanced_segments(polys: dict, H: int, W: int) -> dict:
    """directed segments (a, b) off the raster frame whose count differs from that of (b, a): empty when every shared border is shared"""
    count = {}
    for ring in ring_lists(polys):
        for i, a in enumerate(ring):
            b = ring[(i + 1) % len(ring)]
            on_frame = (a[0] == b[0] and a[0] in (0, W)) or (a[1] == b[1] and a[1] in (0, H))
            if not on_frame:
                count[(a, b)] = count.get((a, b), 0) + 1
    return {s: n for s, n in count.items() if count.get((s[1], s[0]), 0) != n}


def doubled_area_sum(polys: dict) -> int:
    return sum(area2(ring) for ring in ring_lists(polys))


def within_tolerance(cand, ring, q: int) -> bool:
    """does every candidate (x, y, ...) of a ring lie within q / 16 of the line of the output segment that replaced it?  `ring` is the
    kept subsequence of `cand`, in the same cyclic order"""
    pts = [c[:2] for c in cand]
    at = [pts.index(v) for v in ring]
    n = len(pts)
    for a, b in zip(at, at[1:] + at[:1]):
        (px, py), (qx, qy) = pts[a], pts[b]
        d2 = (qx - px) ** 2 + (qy - py) ** 2
        for t in range(1, (b - a) % n if b != a else n):
            zx, zy = pts[(a + t) % n]
            if kept((qx - px) * (zy - py) - (qy - py) * (zx - px), d2, q):
                return False
    return True
