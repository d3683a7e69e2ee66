"""fp64 numpy restatement of the pixel-level augmentations (``unet_pixel_ops`` / ``unet_blur_separable``, csrc/pixel_aug.hip), written
from their definitions in include/unet_hip.h: Philox4x32-10 and the normal field built on it, cv2's Gaussian taps, a separable
reflect-101 filter by explicit index arithmetic, and the pointwise ops.  The oracle of tests/test_augment_pixel_*.py."""
import math

import numpy as np

MASK32 = (1 << 32) - 1


def philox_ref(counter, key):
    """Philox4x32-10 of one counter (4 words) under one key (2 words), in python integers: 4 words"""
    c0, c1, c2, c3 = (int(v) & MASK32 for v in counter)
    k0, k1 = (int(v) & MASK32 for v in key)
    for _ in range(10):
        a, b = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (b >> 32) ^ c1 ^ k0, b & MASK32, (a >> 32) ^ c3 ^ k1, a & MASK32
        k0, k1 = (k0 + 0x9E3779B9) & MASK32, (k1 + 0xBB67AE85) & MASK32
    return c0, c1, c2, c3


def philox_block(q: np.ndarray, key):
    """the same rounds on counters (q, 0, 0, 0) for an array of q, in uint64 lanes: [len(q), 4] words"""
    c = [q.astype(np.uint64), np.zeros(len(q), np.uint64), np.zeros(len(q), np.uint64), np.zeros(len(q), np.uint64)]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    lo = np.uint64(MASK32)
    sh = np.uint64(32)
    for _ in range(10):
        a, b = c[0] * np.uint64(0xD2511F53), c[2] * np.uint64(0xCD9E8D57)
        c = [(b >> sh) ^ c[1] ^ np.uint64(k0), b & lo, (a >> sh) ^ c[3] ^ np.uint64(k1), a & lo]
        k0, k1 = (k0 + 0x9E3779B9) & MASK32, (k1 + 0xBB67AE85) & MASK32
    return np.stack(c, 1)


def noise_field(key, count: int) -> np.ndarray:
    """z of elements 0 .. count - 1: element 4q + 2h + s comes from words (2h, 2h + 1) of counter (q, 0, 0, 0): u = ((w >> 8) + 0.5) / 2^24,
    r = sqrt(-2 ln u_first), angle = 2 pi u_second, cos for s = 0 and sin for s = 1"""
    e = np.arange(count)
    w = philox_block(np.arange((count + 3) // 4), key)
    u = ((w >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    q, h, s = e // 4, (e // 2) % 2, e % 2
    r = np.sqrt(-2.0 * np.log(u[q, 2 * h]))
    ang = 2.0 * math.pi * u[q, 2 * h + 1]
    return np.where(s == 0, r * np.cos(ang), r * np.sin(ang))


def gaussian_taps_ref(k: int, sigma: float) -> np.ndarray:
    """cv2.getGaussianKernel(k, sigma) in fp64"""
    fixed = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
             7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}
    if sigma <= 0 and k in fixed:
        return np.array(fixed[k])
    if sigma <= 0:
        sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    t = np.array([math.exp(-((i - (k - 1) / 2) ** 2) / (2 * sigma * sigma)) for i in range(k)])
    return t / t.sum()


def reflect101(i: int, N: int) -> int:
    """cv2 BORDER_REFLECT_101 for an index any distance outside [0, N): gfedcb|abcdefg|fedcba"""
    if N == 1:
        return 0
    while i < 0 or i >= N:
        i = -i if i < 0 else 2 * (N - 1) - i
    return i


def separable_ref(x: np.ndarray, taps) -> np.ndarray:
    """x [C, H, W] filtered along the width, then along the height, with the same taps; fp64"""
    taps = np.asarray(taps, dtype=np.float64)
    k = len(taps)
    r = k // 2
    C, H, W = x.shape
    x = x.astype(np.float64)
    rows = np.zeros_like(x)
    for t in range(k):
        idx = [reflect101(c + t - r, W) for c in range(W)]
        rows += taps[t] * x[:, :, idx]
    out = np.zeros_like(x)
    for t in range(k):
        idx = [reflect101(c + t - r, H) for c in range(H)]
        out += taps[t] * rows[:, idx, :]
    return out


def program_ref(img: np.ndarray, prog) -> np.ndarray:
    """the ops of ``ops.pixel_ops`` on one image [C, H, W] (fp32 values) -> fp64.  Brightness / contrast is the one op defined in fp32
    (two separately rounded operations); the others are evaluated in fp64."""
    C, H, W = img.shape
    x = img.astype(np.float64)
    for op in prog:
        kind = op[0]
        if kind == "bc":
            t = x.astype(np.float32) * np.float32(op[1])
            if np.float32(op[2]) != 0:
                t = t + np.float32(op[2])
            x = np.clip(t, np.float32(0), np.float32(1)).astype(np.float64)
        elif kind == "gamma":
            x = np.maximum(x, 0.0) ** float(np.float32(op[1]))
        elif kind == "noise":
            _, k0, k1, mean, sigma, per_channel = op
            z = noise_field((k0, k1), C * H * W).reshape(C, H, W) if per_channel else noise_field((k0, k1), H * W).reshape(1, H, W)
            x = np.clip(x + float(np.float32(mean)) + float(np.float32(sigma)) * z, 0.0, 1.0)
        elif kind == "rects":
            for y0, x0, y1, x1 in op[1]:
                x[:, y0:y1, x0:x1] = float(np.float32(op[2]))
        elif kind == "drop":
            for c in op[1]:
                x[c] = float(np.float32(op[2]))
        elif kind == "permute":
            x = x[list(op[1])]
        else:
            raise ValueError(kind)
    return x
