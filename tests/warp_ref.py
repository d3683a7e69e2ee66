"""fp64 numpy restatement of the affine warp of ``unet_warp_affine`` / ``unet_warp_affine_mask`` (cv2.warpAffine with an inverse map)
used by the geometric-augmentation tests: output pixel (x, y) takes the source value at (m0 x + m1 y + m2, m3 x + m4 y + m5); bilinear or
nearest (floor(s + 0.5)); borders 0 constant, 1 replicate, 2 reflect, 4 reflect-101 written as cv2.borderInterpolate's loop."""
import numpy as np


def source_coords(m, H: int, W: int):
    """the source coordinates (sx, sy) [H, W] of every output pixel under one map (6 entries, evaluated in fp64)"""
    m = np.asarray(m, dtype=np.float64)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]


def border_interpolate(p: np.ndarray, n: int, border: int):
    """cv2.borderInterpolate on an int array: (index in [0, n), valid); invalid (constant border) indices come back as 0"""
    p = p.astype(np.int64).copy()
    if border == 0:
        valid = (p >= 0) & (p < n)
        return np.where(valid, p, 0), valid
    if border == 1:
        return np.clip(p, 0, n - 1), np.ones(p.shape, bool)
    assert border in (2, 4), border
    if n == 1:
        return np.zeros_like(p), np.ones(p.shape, bool)
    delta = 1 if border == 4 else 0
    out = (p < 0) | (p >= n)
    while out.any():
        p = np.where(p < 0, -p - 1 + delta, np.where(p >= n, n - 1 - (p - n) - delta, p))
        out = (p < 0) | (p >= n)
    return p, np.ones(p.shape, bool)


def _taps(plane: np.ndarray, ix, iy, W: int, H: int, border: int, fill: float):
    jx, vx = border_interpolate(ix, W, border)
    jy, vy = border_interpolate(iy, H, border)
    return np.where(vx & vy, plane[jy, jx], fill)


def warp_ref(img: np.ndarray, maps: np.ndarray, interp: int, border: int, fill: float = 0.0) -> np.ndarray:
    """img [n, C, H, W] -> fp64 [n, C, H, W]"""
    n, C, H, W = img.shape
    out = np.empty((n, C, H, W), np.float64)
    for j in range(n):
        sx, sy = source_coords(maps[j], H, W)
        for c in range(C):
            plane = img[j, c].astype(np.float64)
            if interp == 0:
                out[j, c] = _taps(plane, np.floor(sx + 0.5), np.floor(sy + 0.5), W, H, border, fill)
                continue
            x0, y0 = np.floor(sx), np.floor(sy)
            fx, fy = sx - x0, sy - y0
            out[j, c] = ((1 - fx) * (1 - fy) * _taps(plane, x0, y0, W, H, border, fill)
                         + fx * (1 - fy) * _taps(plane, x0 + 1, y0, W, H, border, fill)
                         + (1 - fx) * fy * _taps(plane, x0, y0 + 1, W, H, border, fill)
                         + fx * fy * _taps(plane, x0 + 1, y0 + 1, W, H, border, fill))
    return out


def warp_mask_ref(mask: np.ndarray, maps: np.ndarray, border: int, fill=0) -> np.ndarray:
    """mask [n, H, W] (any dtype) -> same dtype, nearest"""
    n, H, W = mask.shape
    out = np.empty_like(mask)
    for j in range(n):
        sx, sy = source_coords(maps[j], H, W)
        jx, vx = border_interpolate(np.floor(sx + 0.5), W, border)
        jy, vy = border_interpolate(np.floor(sy + 0.5), H, border)
        out[j] = np.where(vx & vy, mask[j][jy, jx], fill)
    return out


def tie_pixels(maps: np.ndarray, H: int, W: int, tol: float = 1e-3) -> np.ndarray:
    """bool [n, H, W]: the source coordinate is within tol of a nearest-neighbour rounding tie (k + 0.5) on either axis"""
    out = np.empty((len(maps), H, W), bool)
    for j, m in enumerate(maps):
        sx, sy = source_coords(m, H, W)
        near = lambda s: np.abs(s - (np.floor(s) + 0.5)) <= tol
        out[j] = near(sx) | near(sy)
    return out
