"""NumPy / scipy restatement of the two-object rules of unet_amd/border.py (distance_to_objects, border_weight_map(objects=True)).  It does
NOT use the kernels' shortcut of two candidates per column: every object is measured on its own, against every pixel within reach.

Masks are [B, H, W]; the images of a batch are independent.
Background  a pixel whose value equals `background`.
Excluded    a pixel whose value equals `exclude`, or lies outside [0, n_classes) (n_classes None: 256).  Neither background nor object,
            transparent, no term.
Object      a 4-connected component of equal value among the remaining pixels (scipy.ndimage.label per value and image).
delta(p, L) = min over the pixels q of object L of |p - q|^2, an exact integer; L counts for p only if delta(p, L) <= radius^2.
D1, D2      for a background pixel the smallest and the second smallest delta over the DISTINCT objects that count (equal distances give
            D2 = D1); NO_OBJECT = 2^31 - 1 where there is none, and at object and excluded pixels.
Weight      class_w[y] + w0 exp(-(sqrt D1 + sqrt D2)^2 / (2 sigma^2)) in float64; the second term is 0 where D2 is NO_OBJECT; a target outside
            [0, n_classes) gives 0.
Radius      radius None means ceil(6 sigma)."""
import math

import numpy as np

NO_OBJECT = np.iinfo(np.int32).max

_FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
_EXHAUSTIVE = 1 << 23        # elements of the largest temporary of the exhaustive search


def kinds(mask, background=0, exclude=None, n_classes=None):
    """(background, object) bool arrays; what is neither is excluded"""
    m = np.asarray(mask).astype(np.int64)
    ex = (m < 0) | (m >= (256 if n_classes is None else n_classes))
    if exclude is not None:
        ex |= m == exclude
    bg = ~ex & (m == background)
    return bg, ~ex & ~bg


def components(img, obj):
    """list of bool [H, W]-shaped (y, x) index arrays, one per object of one image"""
    from scipy.ndimage import label
    out = []
    for v in np.unique(img[obj]):
        lab, n = label((img == v) & obj, structure=_FOUR)
        order = np.argsort(lab, axis=None, kind="stable")
        counts = np.bincount(lab.ravel(), minlength=n + 1)
        ends = np.cumsum(counts)
        ys, xs = np.unravel_index(order, lab.shape)
        for k in range(1, n + 1):
            out.append((ys[ends[k - 1]:ends[k]], xs[ends[k - 1]:ends[k]]))
    return out


def _delta_window(qy, qx, y0, y1, x0, x1):
    """int64 [y1 - y0, x1 - x0]: min over the object's pixels q of |p - q|^2 for every p of the window.  Exhaustive (every p against every
    q, the minimum taken one axis at a time) up to _EXHAUSTIVE temporaries; above that scipy's exact transform of the window, squared and
    rounded (the window holds the whole object)"""
    h, w = y1 - y0, x1 - x0
    if len(qy) * h * w <= _EXHAUSTIVE:
        ys, xs = np.arange(y0, y1, dtype=np.int64), np.arange(x0, x1, dtype=np.int64)
        return ((ys[None, :, None] - qy[:, None, None]) ** 2 + (xs[None, None, :] - qx[:, None, None]) ** 2).min(0)
    E = np.zeros((h, w), dtype=bool)
    E[qy - y0, qx - x0] = True
    if max(h * h * w, h * w * w) <= _EXHAUSTIVE:
        ys, xs = np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64)
        pen = np.where(E, 0, np.int64(1) << 40)
        g2 = ((ys[:, None, None] - ys[None, :, None]) ** 2 + pen[None]).min(1)             # [y, x']: the object's nearest pixel of column x'
        return ((xs[:, None] - xs[None, :]) ** 2 + g2[:, None, :]).min(2)
    from scipy.ndimage import distance_transform_edt
    return np.rint(distance_transform_edt(~E) ** 2).astype(np.int64)


def d1d2(mask, background=0, exclude=None, radius=30, n_classes=None):
    """(D1, D2) int32 [B, H, W]"""
    m = np.asarray(mask)
    single = m.ndim == 2
    m = (m[None] if single else m).astype(np.int64)
    B, H, W = m.shape
    R, R2 = int(radius), int(radius) ** 2
    bg, obj = kinds(m, background, exclude, n_classes)
    D1 = np.full((B, H, W), NO_OBJECT, dtype=np.int64)
    D2 = D1.copy()
    for b in range(B):
        for qy, qx in components(m[b], obj[b]):
            y0, y1 = max(0, qy.min() - R), min(H, qy.max() + R + 1)
            x0, x1 = max(0, qx.min() - R), min(W, qx.max() + R + 1)
            d = _delta_window(qy, qx, y0, y1, x0, x1)
            d = np.where(d <= R2, d, NO_OBJECT)
            a, c = D1[b, y0:y1, x0:x1], D2[b, y0:y1, x0:x1]                                # views: every object is offered once
            c[...] = np.where(d < a, a, np.minimum(c, d))
            a[...] = np.minimum(a, d)
    D1[~bg] = NO_OBJECT
    D2[~bg] = NO_OBJECT
    D1, D2 = D1.astype(np.int32), D2.astype(np.int32)
    return (D1[0], D2[0]) if single else (D1, D2)


def default_radius(sigma):
    return max(1, math.ceil(6.0 * sigma))


def weight_map(mask, D1, D2, class_w, w0, sigma, n_classes):
    """float64: class_w[y] + w0 exp(-(sqrt D1 + sqrt D2)^2 / (2 sigma^2)); 0 second term where D2 is NO_OBJECT; 0 outside [0, n_classes)"""
    m = np.asarray(mask).astype(np.int64)
    ok = (m >= 0) & (m < n_classes)
    cw = np.ones(n_classes) if class_w is None else np.asarray(class_w, dtype=np.float64)
    base = cw[np.where(ok, m, 0)]
    both = D2 != NO_OBJECT
    s = np.sqrt(np.where(both, D1, 0).astype(np.float64)) + np.sqrt(np.where(both, D2, 0).astype(np.float64))
    term = np.where(both, w0 * np.exp(-(s * s) / (2.0 * sigma * sigma)), 0.0)
    return np.where(ok, base + term, 0.0)


# ------------------------------------------------------------------------------------------------------------ masks

def blocky(rng, B, H, W, n_classes=4, block=8, dtype=np.uint8, p_background=0.5):
    """blocks of one class each; about p_background of them are background (0)"""
    shape = (B, -(-H // block), -(-W // block))
    small = np.where(rng.random(shape) < p_background, 0, rng.integers(1, max(2, n_classes), size=shape))
    return np.repeat(np.repeat(small, block, 1), block, 2)[:, :H, :W].astype(dtype)


def salt(rng, B, H, W, n_classes=4, density=0.15, dtype=np.uint8):
    """background with single object pixels of random classes: many one-pixel objects"""
    return np.where(rng.random((B, H, W)) < density, rng.integers(1, max(2, n_classes), size=(B, H, W)), 0).astype(dtype)
