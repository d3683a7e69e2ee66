"""NumPy / torch-float64 restatement of the rules of unet_amd/border.py: the border set, the squared distance to it (two ways), the weight
map of the U-Net paper and the per-pixel-weighted cross-entropy."""
import numpy as np
import torch

SENTINEL = np.iinfo(np.int32).max

# [B, H, W]: one pixel, one row, one column, odd sizes, whole tiles, one past a tile, both sides of a 1024-wide chunk, the headline tile
SHAPES = [(1, 1, 1), (1, 1, 70), (1, 70, 1), (2, 37, 53), (3, 64, 64), (1, 65, 130), (1, 8, 1030), (1, 1030, 8), (2, 512, 512)]


def edge_set(mask, exclude=None):
    """bool [..., H, W]: a pixel is a border pixel when one of its 4-neighbours inside the image has another value; with `exclude` a pair of
    neighbours in which either value equals it does not count"""
    m = np.asarray(mask).astype(np.int64)
    e = np.zeros(m.shape, dtype=bool)

    def pair(a, b):
        d = a != b
        if exclude is not None:
            d &= (a != exclude) & (b != exclude)
        return d
    dv = pair(m[..., 1:, :], m[..., :-1, :])
    e[..., 1:, :] |= dv
    e[..., :-1, :] |= dv
    dh = pair(m[..., :, 1:], m[..., :, :-1])
    e[..., :, 1:] |= dh
    e[..., :, :-1] |= dh
    return e


def d2_brute(mask, exclude=None):
    """int32 [B, H, W]: min over EVERY border pixel q of the same image of |p - q|^2, SENTINEL in an image without one.  Exhaustive, no
    pruning; the minimum is taken one axis at a time (min over q = min over q's column of the min over q's row in that column), which
    keeps the temporaries at rows x W x W"""
    E = edge_set(mask, exclude)
    B, H, W = E.shape
    big = np.int64(1) << 40
    out = np.full((B, H, W), SENTINEL, dtype=np.int32)
    ys, xs = np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                              # [x, x']
    step = max(1, (1 << 24) // max(1, max(H, W) * W))
    for b in range(B):
        if not E[b].any():
            continue
        pen = np.where(E[b], 0, big)                                     # [y', x]
        for y0 in range(0, H, step):
            y = ys[y0:y0 + step]
            g2 = ((y[:, None, None] - ys[None, :, None]) ** 2 + pen[None]).min(1)           # [y, x']: nearest border pixel of column x'
            out[b, y0:y0 + step] = (dx2[None] + g2[:, None, :]).min(2).astype(np.int32)
    return out


def d2_scipy(mask, exclude=None):
    from scipy.ndimage import distance_transform_edt
    E = edge_set(mask, exclude)
    out = np.full(E.shape, SENTINEL, dtype=np.int32)
    for b in range(E.shape[0]):
        if E[b].any():
            out[b] = np.rint(distance_transform_edt(~E[b]) ** 2).astype(np.int32)
    return out


def weight_map(mask, d2, class_w, w0, sigma, n_classes):
    """float64: class_w[y] + w0 exp(-d2 / (2 sigma^2)); the sentinel's border term is 0; a target outside [0, n_classes) gives 0"""
    m = np.asarray(mask).astype(np.int64)
    ok = (m >= 0) & (m < n_classes)
    cw = np.ones(n_classes) if class_w is None else np.asarray(class_w, dtype=np.float64)
    base = cw[np.where(ok, m, 0)]
    border = np.where(d2 == SENTINEL, 0.0, w0 * np.exp(-d2.astype(np.float64) / (2.0 * sigma * sigma)))
    return np.where(ok, base + border, 0.0)


def blocky(rng, B, H, W, n_classes=4, block=8, dtype=np.uint8):
    small = rng.integers(0, n_classes, size=(B, -(-H // block), -(-W // block)))
    return np.repeat(np.repeat(small, block, 1), block, 2)[:, :H, :W].astype(dtype)


def salt(rng, B, H, W, n_classes=4, dtype=np.uint8):
    return rng.integers(0, n_classes, size=(B, H, W)).astype(dtype)


def corner(B, H, W, dtype=np.uint8):
    """the only border pixels are (0, 0) and its neighbours: the farthest search"""
    m = np.zeros((B, H, W), dtype=dtype)
    m[:, 0, 0] = 1
    return m


def pw_ce(z, y, pw):
    """(loss, d loss / dz, numerator, denominator) of sum pw nll / sum pw in torch float64; z [P, C], y [P], pw [P]; a target outside
    [0, C) is ignored whatever its weight is"""
    z = torch.as_tensor(z).double().clone().requires_grad_(True)
    y = torch.as_tensor(y).long()
    ok = (y >= 0) & (y < z.shape[1])
    w = torch.as_tensor(pw).double() * ok
    nll = -torch.log_softmax(z, 1).gather(1, y.clamp(0, z.shape[1] - 1)[:, None])[:, 0]
    num, den = (w * nll).sum(), w.sum()
    loss = num / den
    g, = torch.autograd.grad(loss, z)
    return loss.detach(), g, num.detach(), den.detach()
