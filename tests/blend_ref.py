"""Plain numpy float32 restatement of the Gaussian-blended merge (blend="gaussian": csrc/raster.hip, csrc/elementwise.hip,
predict._Merge), for the kernel tests and the CPU fakes.

* weights: w = fl32(gy[ty] * gx[tx]) of two float32 profile tables;
* accumulate_weighted_f32: per-window values [C, h, w] added as fl32(w * v) into a float32 mosaic, w into a float32 weight sum and 1 into
  the hit counter, one window after the other in placement order, with the strip clipping of merge_ref.accumulate_f32;
* finalize_weighted: acc / wsum in float32 where the hit count is positive, optional fill elsewhere, numpy argmax (first maximum).
"""
import numpy as np


def weights(gy, gx, h: int, w: int) -> np.ndarray:
    """float32 [h, w]: the weights of a window of h x w from the first h / w entries of its profile tables"""
    gy, gx = np.asarray(gy, np.float32), np.asarray(gx, np.float32)
    assert gy.shape[0] >= h and gx.shape[0] >= w, (gy.shape, h, gx.shape, w)
    return gy[:h, None] * gx[None, :w]


def accumulate_weighted_f32(mosaic, count, wsum, values, wins, tables, origin=(0, 0), row_lo=0, row_hi=None):
    """values[k]: float32 [C, h, w] of the window at wins[k] = (y0, x0), weighted with tables[k] = (gy, gx); mosaic / count / wsum
    updated in place, window by window"""
    _, MH, MW = mosaic.shape
    row_hi = MH if row_hi is None else row_hi
    for v, (y0, x0), (gy, gx) in zip(values, wins, tables):
        _, h, w = v.shape
        Y0, X0 = int(y0) - origin[0], int(x0) - origin[1]
        r0, r1 = max(Y0, row_lo, 0), min(Y0 + h, row_hi, MH)
        c0, c1 = max(X0, 0), min(X0 + w, MW)
        if r1 <= r0 or c1 <= c0:
            continue
        wt = weights(gy, gx, h, w)[r0 - Y0:r1 - Y0, c0 - X0:c1 - X0]
        mosaic[:, r0:r1, c0:c1] += wt * v[:, r0 - Y0:r1 - Y0, c0 - X0:c1 - X0].astype(np.float32)
        wsum[r0:r1, c0:c1] += wt
        count[r0:r1, c0:c1] += 1
    return mosaic, count, wsum


def finalize_weighted(mosaic, count, wsum, row0: int, nrows: int, fill=None):
    """(mosaic after finalisation, argmax [nrows, MW] uint8) of rows [row0, row0 + nrows); rows outside are returned unchanged"""
    m = mosaic.copy()
    part, cnt, ws = m[:, row0:row0 + nrows], count[row0:row0 + nrows], wsum[row0:row0 + nrows]
    hit = cnt > 0
    part[:, hit] = part[:, hit] / ws[hit].astype(np.float32)
    if fill is not None:
        part[:, ~hit] = np.float32(fill)
    return m, part.argmax(axis=0).astype(np.uint8)
