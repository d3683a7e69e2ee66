"""Inputs of the object-attribute tests (plain NumPy, seeded): class masks with their label images in the convention of
postprocess.label_components (labels[p] = the smallest linear index of p's object)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))

import postprocess_ref as R  # noqa: E402
import rasterize_cases as RC  # noqa: E402

SHAPES = [(1, 1), (1, 5), (5, 1), (3, 17), (7, 6), (33, 300), (40, 56), (2, 1027)]


def own_labels(key: np.ndarray) -> np.ndarray:
    """a label image without a connectivity rule: the pixels of one key form one object, labelled by its first pixel"""
    _, first, inverse = np.unique(key.ravel(), return_index=True, return_inverse=True)
    return first[inverse.ravel()].astype(np.int32).reshape(key.shape)


def ring(H: int = 9, W: int = 11) -> np.ndarray:
    """class 1 as a frame one pixel inside the raster's border, two pixels thick, around a hole of class 0: its centroid lies in the hole"""
    m = np.zeros((H, W), dtype=np.uint8)
    m[1:H - 1, 1:W - 1] = 1
    m[3:H - 3, 3:W - 3] = 0
    return m


def u_shape(H: int = 9, W: int = 10) -> np.ndarray:
    """class 2 as a U open to the top: the floored centroid lies between the arms"""
    m = np.zeros((H, W), dtype=np.uint8)
    m[1:H - 1, 1:3] = 2
    m[1:H - 1, W - 3:W - 1] = 2
    m[H - 3:H - 1, 1:W - 1] = 2
    return m


def cross() -> np.ndarray:
    """8 x 8: a symmetric cross of class 1 with arms two pixels wide; the floored centroid (3, 3) is in it, the true one (3.5, 3.5) a corner"""
    m = np.zeros((8, 8), dtype=np.uint8)
    m[3:5, 0:8] = 1
    m[0:8, 3:5] = 1
    return m


def patterns(H: int, W: int, seed: int) -> dict:
    """{name: (mask uint8 [H, W], labels int32 [H, W])}"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    p = {}
    p["one"] = (np.full((H, W), 3), np.zeros((H, W)))
    p["checker"] = ((yy + xx) % 2 + 1, yy * W + xx)
    p["hstripes"] = (yy % 3, (yy * W + 0 * xx))
    p["vstripes"] = (xx % 3, xx + 0 * yy)
    p["blocks"] = ((yy // 2 + xx // 2) % 4, (yy // 2 * 2) * W + xx // 2 * 2)
    noise = rng.integers(0, 3, (H, W)).astype(np.uint8)
    p["noise"] = (noise, None)
    # one rectangle of one class over the whole raster, cut by hand into objects side by side and one above the other
    cut = np.zeros((H, W), dtype=np.int64)
    cut[:, W // 2:] = 1
    cut[H // 2:, :] += 2
    p["split"] = (np.full((H, W), 2), own_labels(cut))
    out = {}
    for name, (m, lab) in p.items():
        m = np.ascontiguousarray(m, dtype=np.uint8)
        lab = R.label_components(m, 4) if lab is None else np.ascontiguousarray(lab, dtype=np.int32)
        out[name] = (m, lab)
    return out


def placed(shape, small: np.ndarray, at=(0, 0), background: int = 0) -> np.ndarray:
    """`small` pasted into a raster of `shape` and one background class (cropped where it does not fit)"""
    m = np.full(shape, background, dtype=np.uint8)
    y, x = at
    h, w = min(small.shape[0], shape[0] - y), min(small.shape[1], shape[1] - x)
    m[y:y + h, x:x + w] = small[:h, :w]
    return m


def noise_mask(H: int = 67, W: int = 93, seed: int = 21) -> np.ndarray:
    """the 5-class blocks, holes, islands and salt of tests/rasterize_cases.mask"""
    return RC.mask(H, W, seed=seed, salt=0.01)


def two_blobs(H: int = 40, W: int = 64) -> np.ndarray:
    """two overlapping discs of class 1 on class 0: one component that the instance split cuts at its neck"""
    yy, xx = np.mgrid[0:H, 0:W]
    m = (((yy - 20) ** 2 + (xx - 20) ** 2 <= 144) | ((yy - 20) ** 2 + (xx - 40) ** 2 <= 144)).astype(np.uint8)
    return m


def carry_case(H: int = 1100, W: int = 2052):
    """2.26 M pixels, more groups of 4 than the largest grid has lanes, so that a wavefront walks several steps: the first 400 rows are one
    object (steps of one label on end, across rows), a label change in the middle of such a span, rows that are no multiple of 256, blocks of
    90 x 700 pixels below and a little salt"""
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:H, 0:W]
    m = ((yy // 90 + xx // 700) % 4).astype(np.uint8)
    m[:400] = 4
    m[200, 1000:1300] = 1
    key = (yy // 90) * 8 + xx // 700 + 16
    key[:400] = 0
    key[200, 1000:1300] = 1
    salt = rng.random((H, W)) < 0.0005
    m[salt] = 5
    key[salt] = 1000 + np.flatnonzero(salt.ravel())
    return m, own_labels(key)
