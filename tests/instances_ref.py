"""The instance split of unet_amd/instances.py, restated sequentially in NumPy / plain Python: heights, flat zones, ascent, merge rounds and
canonical labels, one after the other, with dictionaries where the device uses atomic maxima.  The device result equals split() bit for
bit.  Only the distance comes from a library (scipy.ndimage.distance_transform_edt; heights_brute is the O(n^2) definition itself)."""
import numpy as np
from scipy import ndimage


def quantise(min_depth) -> int:
    return int(np.floor(16.0 * float(min_depth) + 0.5))


def shallow(peak: int, pas: int, q: int) -> bool:
    """sqrt(peak) - sqrt(pas) < q / 16 in integers"""
    L = 256 * (int(peak) - int(pas)) - q * q
    return L < 0 or L * L < 1024 * q * q * int(pas)


def heights(mask: np.ndarray, classes, R: int) -> np.ndarray:
    """int64 [H, W]: min(R^2, squared distance to the nearest pixel of another value inside the raster) on the split classes, 0 elsewhere"""
    h = np.zeros(mask.shape, dtype=np.int64)
    for c in sorted(set(int(c) for c in classes)):
        own = mask == c
        if not own.any():
            continue
        if own.all():
            h[own] = R * R
            continue
        d2 = np.rint(ndimage.distance_transform_edt(own) ** 2).astype(np.int64)          # exact: the squares are integers far below 2^52
        h[own] = np.minimum(d2[own], R * R)
    return h


def heights_brute(mask: np.ndarray, classes, R: int) -> np.ndarray:
    """the definition, a minimum over all pixels per pixel"""
    H, W = mask.shape
    ys, xs = np.mgrid[0:H, 0:W]
    h = np.zeros(mask.shape, dtype=np.int64)
    split = set(int(c) for c in classes)
    for y in range(H):
        for x in range(W):
            if int(mask[y, x]) not in split:
                continue
            other = mask != mask[y, x]
            d2 = ((ys - y) ** 2 + (xs - x) ** 2)[other]
            h[y, x] = min(R * R, int(d2.min())) if d2.size else R * R
    return h


def _neighbours(p: int, H: int, W: int):
    y, x = divmod(p, W)
    if x > 0:
        yield p - 1
    if x < W - 1:
        yield p + 1
    if y > 0:
        yield p - W
    if y < H - 1:
        yield p + W


def flood(key: np.ndarray) -> np.ndarray:
    """int64 [H, W]: the smallest linear index of every pixel's 4-connected set of equal keys (pixels are visited in index order, so the
    first pixel of a set is its smallest)"""
    H, W = key.shape
    k = key.ravel().tolist()
    lab = [-1] * (H * W)
    for s in range(H * W):
        if lab[s] >= 0:
            continue
        lab[s] = s
        stack = [s]
        while stack:
            p = stack.pop()
            for r in _neighbours(p, H, W):
                if lab[r] < 0 and k[r] == k[s]:
                    lab[r] = s
                    stack.append(r)
    return np.array(lab, dtype=np.int64).reshape(H, W)


def components(mask: np.ndarray) -> np.ndarray:
    """label_components(mask, 4), restated"""
    return flood(mask.astype(np.int64))


def split(mask: np.ndarray, classes, radius: int = 64, min_depth=2.0, max_rounds: int = 64, h=None):
    """(labels int32 [H, W], info) by the rules of unet_amd/instances.py; h: heights computed elsewhere (the brute-force ones)"""
    classes = [classes] if isinstance(classes, (int, np.integer)) else list(classes)
    H, W = mask.shape
    n = H * W
    q = quantise(min_depth)
    h = heights(mask, classes, radius) if h is None else h
    cls = mask.ravel().astype(np.int64).tolist()
    hh = h.ravel().tolist()
    zone = flood(mask.astype(np.int64) * 65536 + h).ravel().tolist()

    # ascent: per zone the adjacent pixel of its class with the largest (h, -index) above it
    up = {}
    for u in range(n):
        for v in _neighbours(u, H, W):
            if cls[v] == cls[u] and hh[v] < hh[u]:
                z = zone[v]
                if z not in up or (hh[u], -u) > up[z]:
                    up[z] = (hh[u], -u)
    roots = sorted(set(zone))
    point = {z: (zone[-up[z][1]] if z in up else z) for z in roots}
    seeds = sum(1 for z in roots if point[z] == z)

    def end(table, a):
        while table[a] != a:
            a = table[a]
        return a

    seg = [end(point, zone[p]) for p in range(n)]

    merged = []
    while len(merged) < max_rounds:
        peak, best = {}, {}
        for p in range(n):
            a = seg[p]
            peak[a] = max(peak.get(a, 0), hh[p])
        for p in range(n):
            for r in _neighbours(p, H, W):
                a, b = seg[p], seg[r]
                if cls[r] != cls[p] or a == b:
                    continue
                key = (min(hh[p], hh[r]), -b)
                if a not in best or key > best[a]:
                    best[a] = key
        to = {a: a for a in peak}
        for a, (pas, nb) in best.items():
            b = -nb
            if shallow(peak[a], pas, q) and (peak[a], -a) < (peak[b], -b):
                to[a] = b
        count = sum(1 for a in to if to[a] != a)
        merged.append(count)
        if count == 0:
            break
        seg = [end(to, s) for s in seg]

    lowest = {}
    for p in range(n):
        lowest.setdefault(seg[p], p)
    labels = np.array([lowest[s] for s in seg], dtype=np.int32).reshape(H, W)
    return labels, {"seeds": seeds, "segments": len(lowest), "rounds": len(merged), "merged": merged}


def dense_ids(mask: np.ndarray, labels: np.ndarray, classes) -> np.ndarray:
    """uint32 [H, W]: 1..N in ascending label order on the split classes, 0 elsewhere"""
    classes = [classes] if isinstance(classes, (int, np.integer)) else list(classes)
    on = np.isin(mask, classes)
    roots = np.unique(labels[on])
    ids = np.zeros(mask.shape, dtype=np.uint32)
    ids[on] = (np.searchsorted(roots, labels[on]) + 1).astype(np.uint32)
    return ids


def discs(H: int, W: int, centres, r2: int = 100, value: int = 1) -> np.ndarray:
    ys, xs = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), dtype=np.uint8)
    for cy, cx in centres:
        m[(ys - cy) ** 2 + (xs - cx) ** 2 <= r2] = value
    return m


def blobs(H: int, W: int, seed: int = 3, sigma: float = 3.0) -> np.ndarray:
    """three classes: a Gaussian-filtered noise field thresholded at two levels"""
    f = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal((H, W)), sigma)
    lo, hi = np.quantile(f, [0.4, 0.7])
    return (f > lo).astype(np.uint8) + (f > hi).astype(np.uint8)
