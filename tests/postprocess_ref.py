"""NumPy restatement of the post-processing rules (unet_amd/postprocess.py): canonical connected-component labels, component sizes, the
majority filter and the sieve rounds with their info.  Written for small rasters; everything is exact integer arithmetic."""
from collections import deque

import numpy as np

_N4 = ((0, -1), (0, 1), (-1, 0), (1, 0))
_N8 = _N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def label_components(mask: np.ndarray, connectivity: int = 4) -> np.ndarray:
    """int32 [H, W]: the smallest linear index y * W + x of every pixel's component (breadth-first fill from the pixels in index order, so
    the first pixel that reaches a component is its smallest index)"""
    assert connectivity in (4, 8) and mask.ndim == 2
    H, W = mask.shape
    nb = _N4 if connectivity == 4 else _N8
    m = mask.tolist()
    lab = [[-1] * W for _ in range(H)]
    for y0 in range(H):
        for x0 in range(W):
            if lab[y0][x0] >= 0:
                continue
            root, c = y0 * W + x0, m[y0][x0]
            lab[y0][x0] = root
            todo = deque([(y0, x0)])
            while todo:
                y, x = todo.popleft()
                for dy, dx in nb:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and lab[yy][xx] < 0 and m[yy][xx] == c:
                        lab[yy][xx] = root
                        todo.append((yy, xx))
    return np.array(lab, dtype=np.int32).reshape(H, W)


def component_sizes(labels: np.ndarray) -> np.ndarray:
    """int32 [H, W]: the pixel count of a component at the index that is its label, 0 elsewhere"""
    return np.bincount(labels.ravel(), minlength=labels.size).astype(np.int32).reshape(labels.shape)


def _box_counts(hit: np.ndarray, k: int) -> np.ndarray:
    """number of True pixels in the k x k window around every pixel; pixels outside the raster do not exist"""
    H, W = hit.shape
    r = k // 2
    s = np.zeros((H + 1, W + 1), dtype=np.int64)
    s[1:, 1:] = hit.astype(np.int64).cumsum(0).cumsum(1)
    y0, y1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    return s[y1][:, x1] - s[y0][:, x1] - s[y1][:, x0] + s[y0][:, x0]


def majority_filter(mask: np.ndarray, k: int, frozen_class=None) -> np.ndarray:
    assert k % 2 == 1 and 3 <= k <= 15
    classes = [int(c) for c in np.unique(mask) if c != frozen_class]          # ascending: argmax below returns the smallest id of a tie
    if not classes:
        return mask.copy()
    counts = np.stack([_box_counts(mask == c, k) for c in classes])
    top = counts.max(axis=0)
    winner = np.array(classes, dtype=np.uint8)[counts.argmax(axis=0)]
    own = np.zeros(mask.shape, dtype=np.int64)
    for i, c in enumerate(classes):
        own[mask == c] = counts[i][mask == c]
    out = np.where(own == top, mask, winner).astype(np.uint8)
    if frozen_class is not None:
        out[mask == frozen_class] = frozen_class
    return out


def sieve_round(mask: np.ndarray, min_pixels: int, connectivity: int = 4, frozen_class=None):
    """one round -> (new mask, components merged, small components that did not merge)"""
    H, W = mask.shape
    n = H * W
    lab = label_components(mask, connectivity).astype(np.int64)
    size = component_sizes(lab.astype(np.int32)).astype(np.int64).ravel()
    cls = mask.ravel().astype(np.int64)
    frozen = -1 if frozen_class is None else int(frozen_class)
    key = size * (n + 1) + (n - np.arange(n))          # (size, -label) as one integer, valid at root indices
    best = np.zeros(n, dtype=np.int64)
    L = lab
    pairs = [(L[:, :-1].ravel(), L[:, 1:].ravel()), (L[:-1, :].ravel(), L[1:, :].ravel())]          # edge adjacency at either connectivity
    for a, b in pairs:
        for s, t in ((a, b), (b, a)):
            ok = (s != t) & (size[s] < min_pixels) & (cls[s] != frozen) & (cls[t] != frozen)
            np.maximum.at(best, s[ok], key[t[ok]])
    roots = np.flatnonzero(size > 0)
    small = roots[(size[roots] < min_pixels) & (cls[roots] != frozen)]
    merging = small[best[small] > key[small]]
    target = n - best[merging] % (n + 1)                 # the best neighbour's label: one of its pixels
    new_cls = cls.copy()
    lut = np.full(n, -1, dtype=np.int64)
    lut[merging] = cls[target]
    hit = lut[lab.ravel()] >= 0
    new_cls[hit] = lut[lab.ravel()][hit]
    return new_cls.astype(np.uint8).reshape(H, W), int(len(merging)), int(len(small) - len(merging))


def count_small(mask: np.ndarray, min_pixels: int, connectivity: int = 4, frozen_class=None) -> int:
    lab = label_components(mask, connectivity)
    size = component_sizes(lab).ravel()
    roots = np.flatnonzero(size > 0)
    cls = mask.ravel()[roots]
    return int(((size[roots] < min_pixels) & (cls != (-1 if frozen_class is None else frozen_class))).sum())


def sieve(mask: np.ndarray, min_pixels: int, connectivity: int = 4, max_rounds: int = 16, frozen_class=None):
    """(mask, info): info["rounds"] counts the rounds run, the one that merged nothing included; info["small_left"] the small components
    of the returned mask"""
    if min_pixels <= 1:
        return mask.copy(), {"rounds": 0, "merged": [], "small_left": 0}
    cur, merged, left = mask.copy(), [], None
    for _ in range(max_rounds):
        nxt, m, l = sieve_round(cur, min_pixels, connectivity, frozen_class)
        merged.append(m)
        if m == 0:
            left = l
            break
        cur = nxt
    if left is None:
        left = count_small(cur, min_pixels, connectivity, frozen_class)
    return cur, {"rounds": len(merged), "merged": merged, "small_left": left}


def postprocess(mask: np.ndarray, majority: int = 0, sieve_px: int = 0, connectivity: int = 4, max_rounds: int = 16, frozen_class=None):
    out = majority_filter(mask, majority, frozen_class) if majority else mask.copy()
    return sieve(out, sieve_px, connectivity, max_rounds, frozen_class)


# ------------------------------------------------------------------------------------------------------------ test patterns

def spiral(H: int, W: int) -> np.ndarray:
    """a one-pixel-wide rectangular spiral of class 1 on class 0 that winds from the outer border to the middle (arms two pixels apart)"""
    m = np.zeros((H, W), dtype=np.uint8)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    y, x = 0, 0
    m[0, 0] = 1
    while top <= bottom and left <= right:
        for x in range(x, right + 1):
            m[y, x] = 1
        top += 2
        if y + 1 > bottom:
            break
        for y in range(y, bottom + 1):
            m[y, x] = 1
        right -= 2
        if x - 1 < left:
            break
        for x in range(x, left - 1, -1):
            m[y, x] = 1
        bottom -= 2
        if y - 1 < top:
            break
        for y in range(y, top - 1, -1):
            m[y, x] = 1
        left += 2
        if x + 1 > right:
            break
    return m


def comb(H: int, W: int) -> np.ndarray:
    """a serpentine: every other row is class 1, joined alternately at the right and at the left end"""
    m = np.zeros((H, W), dtype=np.uint8)
    m[::2] = 1
    for i, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if i % 2 == 0 else 0] = 1
    return m


def patterns(H: int, W: int, seed: int = 0) -> dict:
    rng = np.random.default_rng([seed, H, W])
    yy, xx = np.mgrid[:H, :W]
    blocks = ((yy // 16) * 3 + (xx // 16) * 5) % 4
    salt = rng.random((H, W)) < 0.10
    return {
        "constant": np.full((H, W), 3, dtype=np.uint8),
        "checker": ((yy + xx) % 2).astype(np.uint8),
        "spiral": spiral(H, W),
        "comb": comb(H, W),
        "diag": ((xx + yy) % 3 == 0).astype(np.uint8),
        "antidiag": ((xx - yy) % 3 == 0).astype(np.uint8),
        "noise2": rng.integers(0, 2, (H, W)).astype(np.uint8),
        "noise5": rng.integers(0, 5, (H, W)).astype(np.uint8),
        "noise256": rng.integers(0, 256, (H, W)).astype(np.uint8),
        "blocks": np.where(salt, rng.integers(0, 4, (H, W)), blocks).astype(np.uint8),
    }
