"""Plain Python / NumPy restatement of the ring-tracing rules (unet_amd/vectorize.py): a sequential tracer over a dict of successors, the
saddle swap pass, the walk that collects the corners, and an independent even-odd rasteriser of a ring set.  Written for small rasters;
everything is exact integer arithmetic.  Labels come from tests/postprocess_ref.label_components (4-adjacency)."""
import numpy as np

import postprocess_ref as R

N, W_, S, E = 0, 1, 2, 3
# side -> (dy, dx) of the neighbour across it
_ACROSS = {N: (-1, 0), W_: (0, -1), S: (1, 0), E: (0, 1)}
# side -> (dy, dx) of the next pixel along the walk, and of the pixel diagonally ahead on the outer side relative to that one
_AHEAD = {N: (0, -1), W_: (1, 0), S: (0, 1), E: (-1, 0)}
_OUTER = {N: (-1, 0), W_: (0, -1), S: (1, 0), E: (0, 1)}


def end_vertex(y, x, s):
    """the END vertex (x, y) of the directed edge on side s of pixel (y, x)"""
    return {N: (x, y), W_: (x, y + 1), S: (x + 1, y + 1), E: (x + 1, y)}[s]


def exclude_set(exclude):
    if exclude is None:
        return set()
    if isinstance(exclude, (int, np.integer)):
        return {int(exclude)}
    return {int(c) for c in exclude}


def trace(mask: np.ndarray, exclude=None):
    """-> (rings, info).  rings: list of {"leader": dense edge id, "label", "xy": [(x, y), ...] corners in walk order, "area": signed,
    "edges": dense ids in walk order from the leader}, in ascending leader order.  info = {"swaps": saddle swaps done, "edges": E}"""
    H, W = mask.shape
    lab = R.label_components(mask, 4).tolist()
    m = mask.tolist()
    excl = exclude_set(exclude)

    def label_at(y, x):
        return lab[y][x] if 0 <= y < H and 0 <= x < W else -1

    edges = set()
    for y in range(H):
        for x in range(W):
            if m[y][x] in excl:
                continue
            for s in range(4):
                dy, dx = _ACROSS[s]
                if label_at(y + dy, x + dx) != lab[y][x]:
                    edges.add(4 * (y * W + x) + s)

    def eid(y, x, s):
        return 4 * (y * W + x) + s

    succ = {}
    for e in edges:
        p, s = divmod(e, 4)
        y, x = divmod(p, W)
        L = lab[y][x]
        ay, ax = y + _AHEAD[s][0], x + _AHEAD[s][1]
        oy, ox = ay + _OUTER[s][0], ax + _OUTER[s][1]
        cands = [(y, x, (s + 1) % 4), (ay, ax, s), (oy, ox, (s - 1) % 4)]
        for cy, cx, cs in cands:
            if label_at(cy, cx) == L and eid(cy, cx, cs) in edges:
                succ[e] = eid(cy, cx, cs)
                break
        else:
            raise AssertionError(f"edge {e} has no successor")

    def identify():
        ring = {}
        for e in sorted(edges):
            if e in ring:
                continue
            c = e
            while c not in ring:          # e is the smallest id of its cycle: the sorted scan reaches it first
                ring[c] = e
                c = succ[c]
        return ring

    ring = identify()
    swaps = 0
    for vy in range(1, H):
        for vx in range(1, W):
            a, b, c, d = lab[vy - 1][vx - 1], lab[vy - 1][vx], lab[vy][vx - 1], lab[vy][vx]
            if a == d and b != a and c != a and m[vy][vx] not in excl:
                ea, ed = eid(vy - 1, vx - 1, S), eid(vy, vx, N)          # the two edges that END at the vertex
                if ring[ea] == ring[ed]:
                    succ[ea], succ[ed] = succ[ed], succ[ea]
                    swaps += 1
            if b == c and a != b and d != b and m[vy - 1][vx] not in excl:
                eb, ec = eid(vy - 1, vx, W_), eid(vy, vx - 1, E)
                if ring[eb] == ring[ec]:
                    succ[eb], succ[ec] = succ[ec], succ[eb]
                    swaps += 1
    ring = identify()

    rings = []
    for leader in sorted(set(ring.values())):
        walk, e = [], leader
        while True:
            walk.append(e)
            e = succ[e]
            if e == leader:
                break
        xy, area2 = [], 0
        for e in walk:
            p, s = divmod(e, 4)
            y, x = divmod(p, W)
            x1, y1 = end_vertex(y, x, s)
            x0, y0 = end_vertex(y, x, (s - 1) % 4)          # an edge starts where the previous side of its pixel ends
            area2 += x1 * y0 - x0 * y1
            if succ[e] % 4 != s:
                xy.append((x1, y1))
        assert area2 % 2 == 0
        rings.append({"leader": leader, "label": lab[(leader // 4) // W][(leader // 4) % W], "xy": xy, "area": area2 // 2, "edges": walk})
    return rings, {"swaps": swaps, "edges": len(edges)}


def polygonize(mask: np.ndarray, exclude=None) -> dict:
    """the arrays of unet_amd.vectorize.Polygons as NumPy arrays (plus "swaps")"""
    H, W = mask.shape
    rings, info = trace(mask, exclude)
    xy = [v for r in rings for v in r["xy"]]
    ring_start = np.cumsum([0] + [len(r["xy"]) for r in rings]).astype(np.int64)
    ring_label = np.array([r["label"] for r in rings], dtype=np.int32).reshape(-1)
    ring_area = np.array([r["area"] for r in rings], dtype=np.int64).reshape(-1)
    order = sorted(range(len(rings)), key=lambda i: (rings[i]["label"], rings[i]["leader"]))
    labels = sorted({r["label"] for r in rings})
    counts = {l: 0 for l in labels}
    pixels = {l: 0 for l in labels}
    for r in rings:
        counts[r["label"]] += 1
        pixels[r["label"]] += r["area"]
    flat = mask.ravel()
    return {
        "xy": np.array(xy, dtype=np.int32).reshape(-1, 2),
        "ring_start": ring_start,
        "ring_label": ring_label,
        "ring_area": ring_area,
        "poly_label": np.array(labels, dtype=np.int32).reshape(-1),
        "poly_class": np.array([flat[l] for l in labels], dtype=np.uint8).reshape(-1),
        "poly_pixels": np.array([pixels[l] for l in labels], dtype=np.int64).reshape(-1),
        "poly_ring_start": np.cumsum([0] + [counts[l] for l in labels]).astype(np.int64),
        "poly_rings": np.array(order, dtype=np.int64).reshape(-1),
        "swaps": info["swaps"],
        "shape": (H, W),
    }


ARRAYS = ("xy", "ring_start", "ring_label", "ring_area", "poly_label", "poly_class", "poly_pixels", "poly_ring_start", "poly_rings")


def rings_of(polys: dict, i: int):
    """the vertex lists [(x, y), ...] of polygon i: exterior first, then holes"""
    out = []
    for r in polys["poly_rings"][polys["poly_ring_start"][i]:polys["poly_ring_start"][i + 1]]:
        out.append([tuple(int(c) for c in v) for v in polys["xy"][polys["ring_start"][r]:polys["ring_start"][r + 1]]])
    return out


def fill_even_odd(rings, H: int, W: int) -> np.ndarray:
    """bool [H, W]: the pixels whose centre lies inside the ring set by the even-odd rule.  A ray from a pixel centre towards -x crosses
    only vertical segments: every vertical segment toggles the pixels of its rows from its column to the right end.  Vertices may be any
    rectilinear closed lists (collinear points allowed); independent of the tracer above."""
    toggle = np.zeros((H, W + 1), dtype=np.int64)
    for ring in rings:
        n = len(ring)
        for i in range(n):
            (x0, y0), (x1, y1) = ring[i], ring[(i + 1) % n]
            assert (x0 == x1) != (y0 == y1), "rings must be rectilinear without repeated points"
            if x0 == x1:
                toggle[min(y0, y1):max(y0, y1), x0] += 1
    return (np.cumsum(toggle, axis=1)[:, :W] % 2).astype(bool)


def vertex_visits_once(ring_edges, W: int) -> bool:
    """property (a): no vertex is the end of two edges of one ring"""
    seen = set()
    for e in ring_edges:
        p, s = divmod(e, 4)
        v = end_vertex(p // W, p % W, s)
        if v in seen:
            return False
        seen.add(v)
    return True
