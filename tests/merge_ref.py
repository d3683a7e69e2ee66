"""Plain numpy restatement of the sliding-window merge (csrc/raster.hip, predict.py), for the kernel tests.

* cut / scale: the window of a band-sequential raster and data.py:24 + IntToFloatTensor scaling (int32 -> float32 -> / 255 [/ 255]);
* softmax64: softmax over the last axis in float64;
* accumulate_f32: per-window values [C, h, w] added into a float32 mosaic one window after the other, in placement order, with the
  strip clipping of unet_mosaic_accumulate_windows (mosaic row Y = y0 - origin_y + ty kept when row_lo <= Y < row_hi and inside MH x MW);
* finalize: mean over the hits in float32, optional fill where nothing was placed, numpy argmax (first maximum).
"""
import numpy as np


def cut(raster: np.ndarray, y0: int, x0: int, th: int, tw: int) -> np.ndarray:
    """[C, th, tw] window of a [C, H, W] raster; the window must lie inside it"""
    C, H, W = raster.shape
    assert 0 <= y0 and y0 + th <= H and 0 <= x0 and x0 + tw <= W, (y0, x0, th, tw, H, W)
    return raster[:, y0:y0 + th, x0:x0 + tw]


def scale(a: np.ndarray, div255_twice: bool = False) -> np.ndarray:
    x = a.astype(np.int32).astype(np.float32)
    if div255_twice:
        x = x / np.float32(255.0)
    return x / np.float32(255.0)


def softmax64(z: np.ndarray, axis: int = -1) -> np.ndarray:
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def accumulate_f32(mosaic: np.ndarray, count: np.ndarray, values, wins, origin=(0, 0), row_lo=0, row_hi=None):
    """values[k]: float32 [C, h, w] of the window at wins[k] = (y0, x0); adds them in order (mosaic / count updated in place)"""
    _, MH, MW = mosaic.shape
    row_hi = MH if row_hi is None else row_hi
    for v, (y0, x0) in zip(values, wins):
        _, h, w = v.shape
        Y0, X0 = int(y0) - origin[0], int(x0) - origin[1]
        r0, r1 = max(Y0, row_lo, 0), min(Y0 + h, row_hi, MH)
        c0, c1 = max(X0, 0), min(X0 + w, MW)
        if r1 <= r0 or c1 <= c0:
            continue
        mosaic[:, r0:r1, c0:c1] += v[:, r0 - Y0:r1 - Y0, c0 - X0:c1 - X0].astype(np.float32)
        count[r0:r1, c0:c1] += 1
    return mosaic, count


def finalize(mosaic: np.ndarray, count: np.ndarray, row0: int, nrows: int, fill=None):
    """(mosaic after finalisation, argmax [nrows, MW] uint8) of rows [row0, row0 + nrows); rows outside are returned unchanged"""
    m = mosaic.copy()
    part, cnt = m[:, row0:row0 + nrows], count[row0:row0 + nrows]
    hit = cnt > 0
    part[:, hit] = part[:, hit] / cnt[hit].astype(np.float32)
    if fill is not None:
        part[:, ~hit] = np.float32(fill)
    return m, part.argmax(axis=0).astype(np.uint8)
