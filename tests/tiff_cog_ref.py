"""NumPy / plain-Python restatement of the overview pyramid rule of tiled GeoTIFF output (unet_amd/tiffenc.py, module docstring), one
output sample at a time.  Integers are Python ints (exact), float32 sums are np.float32 scalars added one after the other.

Level k + 1 is computed from level k and has ceil(H_k / 2) x ceil(W_k / 2) samples per plane; levels are added while
max(H_k, W_k) > tile.  An output sample looks at the up-to-2x2 block of its parent (clipped at odd edges), in row-major order TL, TR,
BL, BR.  A sample is valid if no nodata was given or it differs from nodata (NaN nodata: valid means not NaN); a block without a valid
sample gives nodata.
  nearest  the top-left sample, valid or not
  mode     the valid value with the highest count, ties to the value that occurs first
  average  integers: floor((2 s + n) / (2 n)) with the exact sum s of the n valid samples; float32: the valid samples summed
           sequentially in fp32 starting from +0, divided by float32(n) (correctly rounded)"""
import math

import numpy as np


def level_shapes(H: int, W: int, tile: int):
    out = []
    while max(H, W) > tile:
        H, W = (H + 1) // 2, (W + 1) // 2
        out.append((H, W))
    return out


def _nodata(nodata, dtype):
    """nodata as a sample of dtype, None when no sample of that type can equal it"""
    if nodata is None:
        return None
    if dtype.kind == "f":
        return np.float32(nodata)
    f = float(nodata)
    if math.isnan(f) or f != int(f) or not np.iinfo(dtype).min <= int(f) <= np.iinfo(dtype).max:
        return None
    return int(f)


def _valid(v, nd) -> bool:
    if nd is None:
        return True
    if isinstance(nd, np.float32) and np.isnan(nd):
        return not np.isnan(v)
    return bool(v != nd)


def reduce_block(block, resampling: str, nd, is_float: bool):
    """block: the samples of one clipped 2x2 block in row-major order; nd: nodata as a sample, or None"""
    if resampling == "nearest":
        return block[0]
    ok = [v for v in block if _valid(v, nd)]
    if not ok:
        return nd
    if resampling == "mode":
        best, best_n = None, 0
        for v in ok:                                   # row-major order: a later value needs strictly more occurrences
            n = sum(1 for u in ok if u == v)
            if n > best_n:
                best, best_n = v, n
        return best
    assert resampling == "average"
    n = len(ok)
    if is_float:
        acc = np.float32(0.0)
        for v in ok:
            acc = np.float32(acc + np.float32(v))
        return np.float32(acc / np.float32(n))
    return (2 * sum(ok) + n) // (2 * n)                # Python's // floors


def reduce_level(a: np.ndarray, resampling: str, nodata=None) -> np.ndarray:
    a3 = a[None] if a.ndim == 2 else a
    C, H, W = a3.shape
    h, w = (H + 1) // 2, (W + 1) // 2
    nd = _nodata(nodata, a3.dtype)
    is_float = a3.dtype.kind == "f"
    out = np.zeros((C, h, w), a3.dtype)
    for p in range(C):
        rows = [[np.float32(v) for v in r] for r in a3[p]] if is_float else a3[p].tolist()
        for y in range(h):
            for x in range(w):
                block = [rows[yy][xx] for yy in (2 * y, 2 * y + 1) if yy < H for xx in (2 * x, 2 * x + 1) if xx < W]
                with np.errstate(invalid="ignore", over="ignore"):
                    out[p, y, x] = reduce_block(block, resampling, nd, is_float)
    return out[0] if a.ndim == 2 else out


def pyramid(a: np.ndarray, tile: int, resampling: str, nodata=None):
    """[level 1, level 2, ...] of a [C, H, W] or [H, W] array"""
    out = []
    for _ in level_shapes(a.shape[-2], a.shape[-1], tile):
        a = reduce_level(a, resampling, nodata)
        out.append(a)
    return out


def tile_blocks(a: np.ndarray, tile: int):
    """the whole [tile, tile] blocks of a [C, H, W] array in TIFF tile order (plane-major, tile rows, tile columns), zero beyond the edges"""
    C, H, W = a.shape
    out = []
    for p in range(C):
        for j in range(0, H, tile):
            for i in range(0, W, tile):
                b = np.zeros((tile, tile), a.dtype)
                part = a[p, j:j + tile, i:i + tile]
                b[:part.shape[0], :part.shape[1]] = part
                out.append(b)
    return out


def image(dtype, shape, seed, nodata=None):
    """a test image: few distinct values (ties and majorities in most blocks), the type's extremes, and patches of `nodata` of 1 to 5
    samples a side"""
    g = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        a = (g.integers(0, 7, shape) * np.float32(0.3) + g.random(shape, dtype=np.float32) * (g.random(shape) < 0.3)).astype(np.float32)
    else:
        info = np.iinfo(dt)
        vals = np.array([info.min, info.min + 1, -3 if info.min < 0 else 3, 0, 1, 2, 5, info.max - 1, info.max], dtype=dt)
        a = vals[g.integers(0, len(vals), shape)]
    if nodata is not None:
        H, W = shape[-2:]
        for _ in range(max(1, H * W // 40)):
            y, x, s = g.integers(0, H), g.integers(0, W), g.integers(1, 6)
            a[..., y:y + s, x:x + s] = nodata
    return a
