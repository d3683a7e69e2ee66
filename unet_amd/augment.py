"""On-device batch augmentation with the semantics of the reference's ``SegmentationAlbumentationsTransform`` (``utils.py:170-295``)
and of the albumentations transforms its configuration names (``params_and_main.py:105-115``: ``A.Compose([A.HorizontalFlip(p=0.5),
A.VerticalFlip(p=0.5), # A.RandomBrightnessContrast(...), # A.CoarseDropout(p=0.5)])``).  albumentations is not installed here and
its transforms run on the host per image; these run on the GPU on the already scaled float batch.  A pipeline written for the
reference ports by changing the import: ``from unet_amd import augment as A``.

Kept quirks: only the FIRST ``ceil(B * n_transform_imgs) - B`` images of a batch are candidates (python slice semantics of
``utils.py:255-256``), so the shipped default ``n_transform_imgs = 1`` augments NOTHING (quirk Q7).  The reference augments the
image in [0, 1] (``img / 255`` for int8 data, ``utils.py:262-265``) -- the same domain as the batches here.  Random draws come from
a seeded numpy generator (albumentations uses python's ``random``): the streams differ, the distributions are the same.

Geometric transforms (``RandomRotate90``, ``Transpose``, ``Rotate``, ``ShiftScaleRotate``) are affine warps on the device
(``unet_warp_affine`` / ``unet_warp_affine_mask``, csrc/warp.hip): output pixel p takes the source value at M^-1 p, M being cv2's
``getRotationMatrix2D`` about the pixel-grid centre ((W - 1) / 2, (H - 1) / 2) -- the centre current albumentations uses; older releases
rotated about (W / 2, H / 2).  Known difference: bilinear weights are fp32, without cv2's quantisation of them to 1/32 pixel.  Images use
the transform's interpolation (0 nearest, 1 bilinear), masks always nearest (floor(s + 0.5)); border modes are cv2's 0 constant,
1 replicate, 2 reflect and 4 reflect-101.  Wrap borders, bicubic interpolation, ``crop_border=True`` and per-channel fill values are
refused with NotImplementedError.

Non-rigid transforms (``ElasticTransform``, ``GridDistortion``, ``OpticalDistortion``) are remaps on the device: output pixel p takes the
source value at p + d(p) (``unet_warp_field`` / ``unet_warp_field_mask``, csrc/warp_field.hip), with the interpolation, border and fill
rules of the affine warps.  The grid and optical displacements are evaluated per pixel from a few numbers per image; the elastic field is
made on the device from two key words per image (``unet_elastic_field``: Philox noise smoothed by a separable Gaussian of up to 401 taps)
and does not depend on how the batch is split into launches.  Their class docstrings state the maps in full and list what differs from
albumentations; ``alpha_affine``, ``normalized=True`` and kernel sizes above 401 are refused with NotImplementedError.

Pixel-level transforms (``RandomBrightnessContrast``, ``CoarseDropout``, ``RandomGamma``, ``GaussNoise``, ``ChannelDropout``,
``ChannelShuffle``) are pointwise: ``BatchAugment`` turns each maximal run of them into one short program per fired image and runs the
programs of the whole batch in one launch (``unet_pixel_ops``, csrc/pixel_aug.hip).  ``GaussianBlur`` and ``Blur`` are one separable
filter launch (``unet_blur_separable``, border reflect-101 as cv2's default).  Masks are untouched by all of them (``CoarseDropout``
with ``mask_fill_value`` aside).  The Gaussian noise is a pure function of two key words drawn from the seeded generator and the element
index (Philox4x32-10 and Box-Muller, include/unet_hip.h), so it does not depend on how the batch is split into launches.  Known
difference: ``GaussNoise.var_limit`` and ``mean`` are on the 8-bit scale the defaults (10 - 50) are meant for -- on the [0, 1] batches
here sigma = sqrt(var) / 255 and mean / 255; older albumentations releases applied the unscaled sigma to float images.  A scalar
``GaussianBlur.blur_limit`` v means kernel sizes 3..v (what albumentations makes of it when ``sigma_limit`` is 0); a ``blur_limit`` that
holds 0 (kernel size from sigma) or an even bound, and kernel sizes above 31, are refused with NotImplementedError.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np
import torch


class _Transform:
    """A transform fires with probability ``p`` (drawn first); only then are its parameters drawn (``get_params``) and applied
    (``apply_params``).  The split lets ``BatchAugment`` draw a whole batch before anything runs."""

    channels = False             # True: get_params takes the number of channels as well (ChannelDropout, ChannelShuffle)

    def __init__(self, p: float = 0.5, always_apply: bool = False):
        self.p = 1.0 if always_apply else float(p)

    def get_params(self, g: np.random.Generator, H: int, W: int):
        """the random parameters of one application to an H x W image (none by default)"""
        return None

    def draw_params(self, g: np.random.Generator, C, H: int, W: int):
        return self.get_params(g, H, W, C) if self.channels else self.get_params(g, H, W)

    def apply_params(self, img: torch.Tensor, mask: torch.Tensor, prm) -> Tuple[torch.Tensor, torch.Tensor]:
        raise NotImplementedError

    def apply(self, img: torch.Tensor, mask: torch.Tensor, g: np.random.Generator) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.apply_params(img, mask, self.draw_params(g, img.shape[-3] if img.dim() >= 3 else 1, *img.shape[-2:]))

    def __call__(self, img, mask, g):
        return self.apply(img, mask, g) if g.random() < self.p else (img, mask)


class _Geometric(_Transform):
    """a transform that moves pixels: ``matrix`` is its forward map (3 x 3 fp64, homogeneous (x, y, 1) with x along the width)"""
    interpolating = False        # True: samples between pixels (Rotate, ShiftScaleRotate); False: a permutation of the grid (D4)

    def matrix(self, prm, H: int, W: int) -> np.ndarray:
        raise NotImplementedError

    def modes(self):
        """(interpolation, border_mode, image fill, mask fill) of the warp"""
        return 0, 4, 0.0, 0.0

    def apply_params(self, img, mask, prm):
        H, W = img.shape[-2:]
        inv = inverse_map(self.matrix(prm, H, W))
        x, y = _warp(img[None], None if mask is None else mask[None], inv[None], *self.modes())
        return x[0], None if y is None else y[0]


class HorizontalFlip(_Geometric):
    """albumentations ``HorizontalFlip``: image [C,H,W] and mask [H,W] mirrored along the width"""
    def apply_params(self, img, mask, prm):
        return img.flip(-1), mask.flip(-1)

    def matrix(self, prm, H, W):
        return np.array([[-1.0, 0.0, W - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


class VerticalFlip(_Geometric):
    def apply_params(self, img, mask, prm):
        return img.flip(-2), mask.flip(-2)

    def matrix(self, prm, H, W):
        return np.array([[1.0, 0.0, 0.0], [0.0, -1.0, H - 1.0], [0.0, 0.0, 1.0]])


def _square(name: str, H: int, W: int):
    if H != W:
        raise ValueError(f"{name} needs square tiles: an H x W = {H} x {W} result would not stack into the batch")


class RandomRotate90(_Geometric):
    """albumentations ``RandomRotate90``: ``np.rot90(img, factor)`` in the (H, W) plane, factor = integers(0, 4); for factor 1 the source
    pixel (x, y) lands on (y, W - 1 - x).  Square tiles only."""

    def get_params(self, g, H, W):
        return int(g.integers(0, 4))

    def matrix(self, factor, H, W):
        _square("RandomRotate90", H, W)
        r = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, W - 1.0], [0.0, 0.0, 1.0]])
        return np.linalg.matrix_power(r, int(factor) % 4)


class Transpose(_Geometric):
    """albumentations ``Transpose``: x and y swapped.  Square tiles only."""

    def matrix(self, prm, H, W):
        _square("Transpose", H, W)
        return np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def _limit(v) -> Tuple[float, float]:
    return (-abs(float(v)), abs(float(v))) if np.isscalar(v) else (float(v[0]), float(v[1]))


def rotation_matrix(angle: float, scale: float, H: int, W: int) -> np.ndarray:
    """cv2 ``getRotationMatrix2D(c, angle, scale)`` about the pixel-grid centre c = ((W - 1) / 2, (H - 1) / 2), as a 3 x 3 forward map"""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    th = math.radians(angle)
    a, b = scale * math.cos(th), scale * math.sin(th)
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy], [0.0, 0.0, 1.0]])


class _Warp(_Geometric):
    """the cv2.warpAffine options shared by Rotate and ShiftScaleRotate"""
    interpolating = True

    def __init__(self, interpolation, border_mode, value, mask_value, p, always_apply):
        super().__init__(p, always_apply)
        name = type(self).__name__
        if interpolation not in (0, 1):
            raise NotImplementedError(f"{name}: interpolation={interpolation} is not supported (0 nearest, 1 bilinear; no bicubic)")
        if border_mode not in (0, 1, 2, 4):
            what = "wrap (3)" if border_mode == 3 else str(border_mode)
            raise NotImplementedError(f"{name}: border_mode {what} is not supported (0 constant, 1 replicate, 2 reflect, 4 reflect-101)")
        for k, v in (("value", value), ("mask_value", mask_value)):
            if v is not None and not np.isscalar(v):
                raise NotImplementedError(f"{name}: a per-channel {k} {v!r} is not supported (one scalar fill)")
        self.interpolation, self.border_mode = int(interpolation), int(border_mode)
        self.value, self.mask_value = value, mask_value

    def modes(self):
        return (self.interpolation, self.border_mode, 0.0 if self.value is None else float(self.value),
                0.0 if self.mask_value is None else float(self.mask_value))


class Rotate(_Warp):
    """albumentations ``Rotate``: rotation by angle = U(limit) degrees (counter-clockwise for positive angles) about the pixel-grid centre
    ((W - 1) / 2, (H - 1) / 2); the output keeps the input's size"""

    def __init__(self, limit=90, interpolation=1, border_mode=4, value=None, mask_value=None, crop_border=False, p=0.5, always_apply=False):
        super().__init__(interpolation, border_mode, value, mask_value, p, always_apply)
        if crop_border:
            raise NotImplementedError("Rotate: crop_border=True is not supported (it changes the tile shape)")
        self.limit = _limit(limit)

    def get_params(self, g, H, W):
        return float(g.uniform(*self.limit))

    def matrix(self, angle, H, W):
        return rotation_matrix(angle, 1.0, H, W)


class ShiftScaleRotate(_Warp):
    """albumentations ``ShiftScaleRotate``: ``getRotationMatrix2D(c, angle, scale)`` about the pixel-grid centre ((W - 1) / 2, (H - 1) / 2)
    with angle = U(rotate_limit), scale = 1 + U(scale_limit), then a shift of (dx W, dy H), dx = U(shift_limit_x), dy = U(shift_limit_y)
    (both default to shift_limit)"""

    def __init__(self, shift_limit=0.0625, scale_limit=0.1, rotate_limit=45, interpolation=1, border_mode=4, value=None, mask_value=None,
                 shift_limit_x=None, shift_limit_y=None, p=0.5, always_apply=False):
        super().__init__(interpolation, border_mode, value, mask_value, p, always_apply)
        self.rotate, self.scale = _limit(rotate_limit), _limit(scale_limit)
        self.shift_x = _limit(shift_limit if shift_limit_x is None else shift_limit_x)
        self.shift_y = _limit(shift_limit if shift_limit_y is None else shift_limit_y)

    def get_params(self, g, H, W):
        angle = float(g.uniform(*self.rotate))
        scale = 1.0 + float(g.uniform(*self.scale))
        dx, dy = float(g.uniform(*self.shift_x)), float(g.uniform(*self.shift_y))
        return angle, scale, dx, dy

    def matrix(self, prm, H, W):
        angle, scale, dx, dy = prm
        m = rotation_matrix(angle, scale, H, W)
        m[0, 2] += dx * W
        m[1, 2] += dy * H
        return m


IDENTITY_MAP = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


class _Field(_Warp):
    """a non-rigid warp: output pixel p takes the source value at p + d(p) (cv2.remap with the map p + d), through ``ops.warp_field`` /
    ``ops.warp_field_mask`` (csrc/warp_field.hip).  ``kind`` names the kernel's displacement kind and ``field_params`` turns the drawn
    parameters of a batch (None for an image that did not fire) into what the kernel takes for it.  A field transform closes its
    geometric segment (``BatchAugment.segments``)."""
    kind = ""

    def field_params(self, prms: list, H: int, W: int, device):
        raise NotImplementedError

    def matrix(self, prm, H, W):
        raise TypeError(f"{type(self).__name__} is not an affine map")

    def warp_batch(self, img: torch.Tensor, mask, prms: list, pre_maps=None):
        """image batch [n, C, H, W] and mask batch [n, H, W] (or None) sampled at pre_maps[j] * (p + d_j(p)) into new tensors; prms[j] is
        None for an image that did not fire (d_j = 0)"""
        from . import ops
        H, W = img.shape[-2:]
        fired = [prm is not None for prm in prms]
        params = self.field_params(prms, H, W, img.device)
        interp, border, fill, mask_fill = self.modes()
        return _warp_pair(img, mask, lambda src, dst: ops.warp_field(src, dst, self.kind, params, fired, pre_maps, interp, border, fill),
                          lambda src, dst: ops.warp_field_mask(src, dst, self.kind, params, fired, pre_maps, border, mask_fill))

    def apply_params(self, img, mask, prm):
        x, y = self.warp_batch(img[None], None if mask is None else mask[None], [prm])
        return x[0], None if y is None else y[0]


MAX_ELASTIC_KSIZE = 401


def elastic_ksize(sigma: float, approximate: bool = False) -> int:
    """the Gaussian kernel size of ElasticTransform: 17 when approximate, else cv2's rule for float images round(8 sigma + 1) | 1"""
    return 17 if approximate else int(round(8.0 * float(sigma) + 1.0)) | 1


def elastic_taps(sigma: float, ksize: int) -> np.ndarray:
    """g[i] proportional to exp(-i^2 / (2 sigma^2)), i = -(ksize // 2) .. ksize // 2, normalised in fp64 and rounded to fp32"""
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    t = np.exp(-(x * x) / (2.0 * float(sigma) ** 2))
    return (t / t.sum()).astype(np.float32)


class ElasticTransform(_Field):
    """albumentations ``ElasticTransform(alpha=1, sigma=50, interpolation=1, border_mode=4, value=None, mask_value=None,
    approximate=False, same_dxdy=False, alpha_affine=None, p)``, as this project defines it: two planes of uniform noise in (-1, 1), dx and
    dy, are smoothed by a Gaussian of standard deviation ``sigma`` and multiplied by ``alpha``; output pixel (x, y) takes the source value
    at (x + dx, y + dy).  The parameters are two Philox key words drawn from the seeded generator.  Noise plane q (0 = dx, 1 = dy) at
    element e = y W + x is 2 u - 1, u = ((w >> 8) + 0.5) 2^-24, w = word e % 4 of Philox4x32-10 under the key at counter (e / 4, q, 0, 0):
    the field is a pure function of the key and the pixel.  Each plane is filtered along rows, then along columns, with the taps
    g[i] ~ exp(-i^2 / (2 sigma^2)) (``elastic_taps``: normalised in fp64, rounded to fp32) of a kernel of ``elastic_ksize`` entries --
    round(8 sigma + 1) | 1, or 17 with ``approximate=True`` -- and border reflect-101, repeated as often as the radius needs.  With
    ``same_dxdy`` dy is dx.

    Known differences (albumentations and cv2 are not installed here, nothing was compared against them): albumentations draws the noise
    from numpy's generator, so the fields differ draw by draw; the kernel-size rule is cv2's for float images as recalled, cv2 itself
    may pick a smaller kernel for the same sigma; bilinear weights are fp32, without cv2's quantisation to 1/32 pixel.  A non-zero
    ``alpha_affine`` (the random affine part of old releases) is refused: put a ``ShiftScaleRotate`` in front instead.  Kernel sizes
    above 401 (sigma above 50 without ``approximate``) are refused."""
    kind = "dense"

    def __init__(self, alpha=1, sigma=50, interpolation=1, border_mode=4, value=None, mask_value=None, approximate=False, same_dxdy=False,
                 alpha_affine=None, p=0.5, always_apply=False):
        super().__init__(interpolation, border_mode, value, mask_value, p, always_apply)
        if alpha_affine:
            raise NotImplementedError(f"ElasticTransform: alpha_affine={alpha_affine!r} is not supported (only None or 0): put a "
                                      "ShiftScaleRotate in front of it for the random affine part")
        if not (float(sigma) > 0 and math.isfinite(float(sigma)) and math.isfinite(float(alpha))):
            raise ValueError(f"ElasticTransform: alpha={alpha!r}, sigma={sigma!r} (finite, sigma > 0)")
        self.alpha, self.sigma, self.same_dxdy = float(alpha), float(sigma), bool(same_dxdy)
        self.ksize = elastic_ksize(sigma, approximate)
        if self.ksize > MAX_ELASTIC_KSIZE:
            raise NotImplementedError(f"ElasticTransform: sigma={sigma!r} needs a kernel of {self.ksize} taps, at most {MAX_ELASTIC_KSIZE} "
                                      "are supported (sigma <= 50, or approximate=True)")
        self.taps = elastic_taps(self.sigma, self.ksize)

    def get_params(self, g, H, W):
        return int(g.integers(0, 2 ** 32)), int(g.integers(0, 2 ** 32))

    def field_params(self, prms, H, W, device):
        from . import ops
        field = torch.empty(len(prms), 2, H, W, dtype=torch.float32, device=device)
        ops.elastic_field(field, torch.empty_like(field), [(0, 0) if prm is None else prm for prm in prms], self.alpha,
                          [prm is not None for prm in prms], self.same_dxdy, self.taps)
        return field


MAX_GRID_CELLS = 16


def grid_nodes(N: int, num_steps: int, factors) -> Tuple[int, np.ndarray]:
    """(step, nodes) of one axis of GridDistortion: step = N // num_steps (at least 1) entries per cell and the node values 0 = nodes[0],
    nodes[1], ... of albumentations' loop -- ``cur = prev + step * factors[i]``, or N where cell i was clipped at N -- as the 17 fp32
    values the kernel takes (unused ones 0)"""
    step = max(N // num_steps, 1)
    cells = -(-N // step)
    if cells > len(factors) or cells > MAX_GRID_CELLS:
        raise ValueError(f"GridDistortion: {N} pixels in steps of {step} are {cells} cells, more than the {len(factors)} factors of "
                         f"num_steps={num_steps} (albumentations fails on this as well)")
    nodes, prev = np.zeros(MAX_GRID_CELLS + 1, dtype=np.float64), 0.0
    for i in range(cells):
        prev = float(N) if i * step + step > N else prev + step * float(factors[i])
        nodes[i + 1] = prev
    return step, nodes.astype(np.float32)


class GridDistortion(_Field):
    """albumentations ``GridDistortion(num_steps=5, distort_limit=0.3, interpolation=1, border_mode=4, value=None, mask_value=None,
    normalized=False, p)``: num_steps + 1 factors 1 + U(distort_limit) per axis (x first); the source column table xx is albumentations'
    loop -- step = W // num_steps, cell i covers [i step, min(i step + step, W)), ``cur = prev + step * f_i`` (W where the cell was
    clipped) and the cell is filled with ``np.linspace(prev, cur, len)``, endpoint included, so a cell of one pixel gets prev -- rows the
    same with H; output pixel (x, y) takes the source value at (xx[x], yy[y]).  The node values prev / cur go to the kernel as fp32.

    Known differences (nothing was compared against the package): a tile narrower than num_steps uses step 1, where albumentations
    divides by a zero step; ``normalized=True`` is refused, and so is a ``num_steps`` outside 1..15 (16 cells per axis)."""
    kind = "grid"

    def __init__(self, num_steps=5, distort_limit=0.3, interpolation=1, border_mode=4, value=None, mask_value=None, normalized=False, p=0.5,
                 always_apply=False):
        super().__init__(interpolation, border_mode, value, mask_value, p, always_apply)
        if normalized:
            raise NotImplementedError("GridDistortion: normalized=True is not supported")
        if not 1 <= int(num_steps) <= MAX_GRID_CELLS - 1 or int(num_steps) != num_steps:
            raise NotImplementedError(f"GridDistortion: num_steps={num_steps!r} is not supported (1..{MAX_GRID_CELLS - 1})")
        self.num_steps, self.limit = int(num_steps), _limit(distort_limit)

    def get_params(self, g, H, W):
        fx = [1.0 + float(g.uniform(*self.limit)) for _ in range(self.num_steps + 1)]
        fy = [1.0 + float(g.uniform(*self.limit)) for _ in range(self.num_steps + 1)]
        return fx, fy

    def field_params(self, prms, H, W, device):
        nodes = np.zeros((len(prms), 2, MAX_GRID_CELLS + 1), dtype=np.float32)
        step_x, step_y = max(W // self.num_steps, 1), max(H // self.num_steps, 1)
        for j, prm in enumerate(prms):
            if prm is not None:
                nodes[j, 0], nodes[j, 1] = grid_nodes(W, self.num_steps, prm[0])[1], grid_nodes(H, self.num_steps, prm[1])[1]
        return step_x, step_y, nodes


class OpticalDistortion(_Field):
    """albumentations ``OpticalDistortion(distort_limit=0.05, shift_limit=0.05, interpolation=1, border_mode=4, value=None,
    mask_value=None, p)``, as this project defines it: k = U(distort_limit), dx = U(shift_limit) W, dy = U(shift_limit) H; with
    c = ((W - 1) / 2, (H - 1) / 2), u' = (x - c_x) / W, v' = (y - c_y) / H, r^2 = u'^2 + v'^2 and kappa = 1 + k r^2 + k r^4, output pixel
    (x, y) takes the source value at (W u' kappa + c_x + dx, H v' kappa + c_y + dy): the identity at k = 0, dx = dy = 0.

    Known differences (nothing was compared against the package): cv2's own map (initUndistortRectifyMap with focal lengths W, H), as
    far as recalled, places the projection centre at (W / 2, H / 2) and so shifts by half a pixel; albumentations 1.3 rounds the shift
    to whole pixels."""
    kind = "optical"

    def __init__(self, distort_limit=0.05, shift_limit=0.05, interpolation=1, border_mode=4, value=None, mask_value=None, p=0.5,
                 always_apply=False):
        super().__init__(interpolation, border_mode, value, mask_value, p, always_apply)
        self.distort, self.shift = _limit(distort_limit), _limit(shift_limit)

    def get_params(self, g, H, W):
        k = float(g.uniform(*self.distort))
        return k, float(g.uniform(*self.shift)) * W, float(g.uniform(*self.shift)) * H

    def field_params(self, prms, H, W, device):
        return np.array([(0.0, 0.0, 0.0) if prm is None else prm for prm in prms], dtype=np.float32).reshape(len(prms), 3)


def _device_geometric(t) -> bool:
    """a geometric transform that is not one of the two flips: it exists as a device warp only"""
    return isinstance(t, _Geometric) and not isinstance(t, (HorizontalFlip, VerticalFlip))


def inverse_map(forward: np.ndarray) -> np.ndarray:
    """the output -> source map of a 3 x 3 forward map as the 6 fp32 entries the warp kernels take.  Inverted in fp64; entries within
    1e-9 of a multiple of 0.5 are snapped to it, so that D4 maps and multiples of 90 degrees are exact permutations of the grid."""
    inv = np.linalg.inv(np.asarray(forward, dtype=np.float64))[:2].reshape(6)
    half = np.round(inv * 2.0) / 2.0
    inv = np.where(np.abs(inv - half) <= 1e-9, half, inv)
    return inv.astype(np.float32)


def _warp_pair(img: torch.Tensor, mask, warp_image, warp_mask):
    """image batch [n, C, H, W] fp32 and mask batch [n, H, W] (or None) warped into new tensors by warp_image(src, dst) and, when there
    is a mask, warp_mask(src, dst)"""
    out = torch.empty_like(img, memory_format=torch.contiguous_format)
    warp_image(img.contiguous(), out)
    if mask is None:
        return out, None
    mout = torch.empty_like(mask, memory_format=torch.contiguous_format)
    warp_mask(mask.contiguous(), mout)
    return out, mout


def _warp(img: torch.Tensor, mask, inv_maps: np.ndarray, interp: int, border: int, fill: float, mask_fill: float):
    """image batch [n, C, H, W] fp32 and mask batch [n, H, W] (or None) warped by inv_maps [n, 6] into new tensors"""
    from . import ops
    return _warp_pair(img, mask, lambda src, dst: ops.warp_affine(src, dst, inv_maps, interp, border, fill),
                      lambda src, dst: ops.warp_affine_mask(src, dst, inv_maps, border, mask_fill))


class _Pointwise(_Transform):
    """a transform of each pixel on its own: ``program`` gives its ops for ``ops.pixel_ops`` (None: it needs the whole image and runs per
    image), ``mask_rects`` the (rectangles, fill) it sets in the mask, if any"""

    def program(self, prm, C: int, H: int, W: int):
        raise NotImplementedError

    def mask_rects(self, prm):
        return None

    def check(self, C: int, H: int, W: int):
        """raises for an image this transform cannot take"""

    def _cpu(self, img: torch.Tensor, prm) -> torch.Tensor:
        raise NotImplementedError

    def apply_params(self, img, mask, prm):
        self.check(img.shape[-3], *img.shape[-2:])
        if not img.is_cuda:
            return self._cpu(img, prm), mask
        from . import ops
        out = img.contiguous().clone()[None]
        ops.pixel_ops(out, {0: self.program(prm, *out.shape[1:])})
        return out[0], mask


class RandomBrightnessContrast(_Pointwise):
    """albumentations ``RandomBrightnessContrast(brightness_limit, contrast_limit, brightness_by_max=True, p)`` on a float image in
    [0, 1]: ``img * alpha + beta * (1 if brightness_by_max else mean(img))`` with alpha = 1 + U(contrast_limit), beta = U(brightness_limit),
    clipped to [0, 1]; the mask is untouched."""

    def __init__(self, brightness_limit=0.2, contrast_limit=0.2, brightness_by_max=True, p=0.5, always_apply=False):
        super().__init__(p, always_apply)
        self.b, self.c, self.by_max = _limit(brightness_limit), _limit(contrast_limit), brightness_by_max

    def get_params(self, g, H, W):
        alpha = 1.0 + g.uniform(*self.c)
        beta = g.uniform(*self.b)
        return alpha, beta

    def apply_params(self, img, mask, prm):
        alpha, beta = prm
        out = img * alpha
        if beta != 0:
            out = out + (beta if self.by_max else beta * img.mean())
        return out.clamp_(0.0, 1.0), mask

    def program(self, prm, C, H, W):
        return [("bc", prm[0], prm[1])] if self.by_max else None


class CoarseDropout(_Pointwise):
    """albumentations ``CoarseDropout(max_holes=8, max_height=8, max_width=8, min_holes=None, min_height=None, min_width=None,
    fill_value=0, mask_fill_value=None, p)``: between min_holes and max_holes rectangles of the image set to fill_value (the mask
    only when mask_fill_value is given); the unset minima default to the maxima."""

    def __init__(self, max_holes=8, max_height=8, max_width=8, min_holes=None, min_height=None, min_width=None, fill_value=0,
                 mask_fill_value=None, p=0.5, always_apply=False):
        super().__init__(p, always_apply)
        self.holes = (max_holes if min_holes is None else min_holes, max_holes)
        self.h = (max_height if min_height is None else min_height, max_height)
        self.w = (max_width if min_width is None else min_width, max_width)
        self.fill, self.mask_fill = fill_value, mask_fill_value

    def get_params(self, g, H, W):
        holes = []
        for _ in range(int(g.integers(self.holes[0], self.holes[1] + 1))):
            hh, ww = int(g.integers(self.h[0], self.h[1] + 1)), int(g.integers(self.w[0], self.w[1] + 1))
            hh, ww = min(hh, H), min(ww, W)
            y1, x1 = int(g.integers(0, H - hh + 1)), int(g.integers(0, W - ww + 1))
            holes.append((y1, x1, hh, ww))
        return holes

    def apply_params(self, img, mask, holes):
        img = img.clone()
        mask = mask if self.mask_fill is None else mask.clone()
        for y1, x1, hh, ww in holes:
            img[..., y1:y1 + hh, x1:x1 + ww] = self.fill
            if self.mask_fill is not None:
                mask[y1:y1 + hh, x1:x1 + ww] = self.mask_fill
        return img, mask

    def program(self, holes, C, H, W):
        return [("rects", [(y1, x1, y1 + hh, x1 + ww) for y1, x1, hh, ww in holes if hh > 0 and ww > 0], self.fill)]

    def mask_rects(self, holes):
        if self.mask_fill is None:
            return None
        return [(y1, x1, y1 + hh, x1 + ww) for y1, x1, hh, ww in holes if hh > 0 and ww > 0], self.mask_fill


def _range(v, low) -> Tuple[float, float]:
    """albumentations ``to_tuple(v, low)``: a scalar v means (low, v)"""
    return (float(low), float(v)) if np.isscalar(v) else (float(v[0]), float(v[1]))


class RandomGamma(_Pointwise):
    """albumentations ``RandomGamma(gamma_limit=(80, 120), p)``: ``img ** gamma`` with gamma = U(gamma_limit) / 100"""

    def __init__(self, gamma_limit=(80, 120), p=0.5, always_apply=False):
        super().__init__(p, always_apply)
        self.limit = _range(gamma_limit, gamma_limit)

    def get_params(self, g, H, W):
        return float(g.uniform(*self.limit)) / 100.0

    def program(self, gamma, C, H, W):
        return [("gamma", gamma)]

    def _cpu(self, img, gamma):
        return img.clamp(min=0.0).double().pow(gamma).float()


PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)


def philox4x32_10(counter: np.ndarray, key) -> np.ndarray:
    """Philox4x32-10 on counters [..., 4] (uint32) under the two key words: [..., 4] uint32"""
    c = [np.asarray(counter[..., k], dtype=np.uint64) for k in range(4)]
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    m32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M[0]) * c[0], np.uint64(PHILOX_M[1]) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + PHILOX_W[0]) & 0xffffffff, (k1 + PHILOX_W[1]) & 0xffffffff
    return np.stack(c, axis=-1).astype(np.uint32)


def normal_field(key, count: int) -> np.ndarray:
    """the normal deviates of elements 0 .. count - 1 under a key (fp64): words (0, 1) of counter (q, 0, 0, 0) give elements 4q, 4q + 1 as
    r cos(2 pi u1), r sin(2 pi u1), r = sqrt(-2 ln u0), words (2, 3) elements 4q + 2, 4q + 3; u = ((w >> 8) + 0.5) 2^-24"""
    nq = -(-count // 4)
    ctr = np.zeros((nq, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(nq, dtype=np.uint32)
    u = ((philox4x32_10(ctr, key) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u[:, 0::2]))                          # [nq, 2]: from words 0 and 2
    th = 2.0 * np.pi * u[:, 1::2]
    return np.stack([r * np.cos(th), r * np.sin(th)], axis=-1).reshape(-1)[:count]


class GaussNoise(_Pointwise):
    """albumentations ``GaussNoise(var_limit=(10, 50), mean=0, per_channel=True, p)``: ``clip(img + N(mean, var))`` with var =
    U(var_limit), var and mean on the 8-bit scale (sigma = sqrt(var) / 255 on a [0, 1] image); per_channel=False adds one field to every
    channel.  The parameters are (var, key word 0, key word 1)."""

    def __init__(self, var_limit=(10.0, 50.0), mean=0, per_channel=True, p=0.5, always_apply=False):
        super().__init__(p, always_apply)
        self.var = _range(var_limit, 0)
        if self.var[0] < 0 or self.var[1] < self.var[0]:
            raise ValueError(f"GaussNoise: var_limit {var_limit!r} must be a non-negative range")
        self.mean, self.per_channel = float(mean), bool(per_channel)

    def get_params(self, g, H, W):
        var = float(g.uniform(*self.var))
        return var, int(g.integers(0, 2 ** 32)), int(g.integers(0, 2 ** 32))

    def program(self, prm, C, H, W):
        var, k0, k1 = prm
        return [("noise", k0, k1, self.mean / 255.0, math.sqrt(var) / 255.0, self.per_channel)]

    def _cpu(self, img, prm):
        var, k0, k1 = prm
        C, H, W = img.shape
        z = normal_field((k0, k1), C * H * W).reshape(C, H, W) if self.per_channel else normal_field((k0, k1), H * W).reshape(1, H, W)
        out = img.double() + self.mean / 255.0 + math.sqrt(var) / 255.0 * torch.from_numpy(z)
        return out.clamp_(0.0, 1.0).float()


class ChannelDropout(_Pointwise):
    """albumentations ``ChannelDropout(channel_drop_range=(1, 1), fill_value=0, p)``: a number of channels in the range, drawn without
    replacement, set to fill_value"""
    channels = True

    def __init__(self, channel_drop_range=(1, 1), fill_value=0, p=0.5, always_apply=False):
        super().__init__(p, always_apply)
        self.range = (int(channel_drop_range[0]), int(channel_drop_range[1]))
        if not 1 <= self.range[0] <= self.range[1]:
            raise ValueError(f"Invalid channel_drop_range. Got: {channel_drop_range}")
        self.fill = fill_value

    def check(self, C, H, W):
        if C == 1:
            raise ValueError("Images has one channel. ChannelDropout is not defined.")
        if self.range[1] >= C:
            raise ValueError("Can not drop all channels in ChannelDropout.")

    def get_params(self, g, H, W, C):
        self.check(C, H, W)
        count = int(g.integers(self.range[0], self.range[1] + 1))
        return [int(c) for c in g.choice(C, size=count, replace=False)]

    def program(self, drop, C, H, W):
        return [("drop", drop, self.fill)]

    def _cpu(self, img, drop):
        out = img.clone()
        out[list(drop)] = self.fill
        return out


class ChannelShuffle(_Pointwise):
    """albumentations ``ChannelShuffle(p)``: the channels in a random order, channel c taking channel perm[c]"""
    channels = True

    def check(self, C, H, W):
        if C > 16:
            raise ValueError(f"ChannelShuffle: at most 16 channels are supported, the image has {C}")

    def get_params(self, g, H, W, C):
        self.check(C, H, W)
        return [int(c) for c in g.permutation(C)]

    def program(self, perm, C, H, W):
        return [("permute", perm)]

    def _cpu(self, img, perm):
        return img[list(perm)].clone()


def gaussian_taps(k: int, sigma: float) -> np.ndarray:
    """cv2 ``getGaussianKernel(k, sigma)`` as fp32: the fixed tables for sigma <= 0 and k in 1, 3, 5, 7; else exp(-x^2 / (2 sigma^2)) with
    sigma = 0.3 ((k - 1) / 2 - 1) + 0.8 when it is not given, normalised in fp64"""
    small = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
             7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}
    if sigma <= 0 and k in small:
        return np.array(small[k], dtype=np.float32)
    if sigma <= 0:
        sigma = 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8
    x = np.arange(k, dtype=np.float64) - (k - 1) * 0.5
    t = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(np.float32)


MAX_BLUR = 31


def _reflect101(i: np.ndarray, N: int) -> np.ndarray:
    if N == 1:
        return np.zeros_like(i)
    r = np.mod(i, 2 * N - 2)
    return np.where(r < N, r, 2 * N - 2 - r)


class _Blur(_Transform):
    """a separable filter with per-image taps: kernel sizes are the odd numbers in blur_limit"""

    def __init__(self, blur_limit, p, always_apply):
        super().__init__(p, always_apply)
        name = type(self).__name__
        lo, hi = (3, int(blur_limit)) if np.isscalar(blur_limit) else (int(blur_limit[0]), int(blur_limit[1]))
        if lo == 0 or hi == 0 or lo % 2 == 0 or hi % 2 == 0:
            raise NotImplementedError(f"{name}: blur_limit={blur_limit!r} is not supported (odd bounds; 0, the kernel size from sigma, is not)")
        if lo < 1 or hi < lo:
            raise ValueError(f"{name}: blur_limit={blur_limit!r} is not a range of kernel sizes")
        if hi > MAX_BLUR:
            raise NotImplementedError(f"{name}: kernel sizes above {MAX_BLUR} are not supported (blur_limit={blur_limit!r})")
        self.blur = (lo, hi)

    def ksize(self, g) -> int:
        return self.blur[0] + 2 * int(g.integers(0, (self.blur[1] - self.blur[0]) // 2 + 1))

    def taps(self, prm) -> np.ndarray:
        raise NotImplementedError

    def apply_params(self, img, mask, prm):
        taps = self.taps(prm)
        if img.is_cuda:
            from . import ops
            src = img.contiguous()[None]
            out = torch.empty_like(src)
            ops.blur_separable(src, out, [taps])
            return out[0], mask
        C, H, W = img.shape
        r, t = len(taps) // 2, taps.astype(np.float64)
        x = img.double().numpy()
        cols = _reflect101(np.arange(W)[:, None] + np.arange(-r, r + 1)[None], W)       # [W, k]
        rows = _reflect101(np.arange(H)[:, None] + np.arange(-r, r + 1)[None], H)       # [H, k]
        x = (x[:, :, cols] * t).sum(-1)
        x = (x[:, rows, :] * t[None, None, :, None]).sum(2)
        return torch.from_numpy(x).float(), mask


class GaussianBlur(_Blur):
    """albumentations ``GaussianBlur(blur_limit=(3, 7), sigma_limit=0, p)``: cv2.GaussianBlur with a kernel size uniform over the odd
    sizes in blur_limit and sigma = U(sigma_limit) (a scalar v means (0, v); sigma 0: cv2's rule for the size), border reflect-101"""

    def __init__(self, blur_limit=(3, 7), sigma_limit=0, p=0.5, always_apply=False):
        super().__init__(blur_limit, p, always_apply)
        self.sigma = _range(sigma_limit, 0)

    def get_params(self, g, H, W):
        return self.ksize(g), float(g.uniform(*self.sigma))

    def taps(self, prm):
        return gaussian_taps(*prm)


class Blur(_Blur):
    """albumentations ``Blur(blur_limit=7, p)``: a k x k box filter, k uniform over the odd sizes in 3..blur_limit (or the given range)"""

    def __init__(self, blur_limit=7, p=0.5, always_apply=False):
        super().__init__(blur_limit, p, always_apply)

    def get_params(self, g, H, W):
        return self.ksize(g)

    def taps(self, k):
        return np.full(k, 1.0 / k, dtype=np.float32)


class Compose:
    """albumentations ``Compose``: the transforms in order, each with its own probability; ``p`` gates the whole pipeline"""

    def __init__(self, transforms: Sequence[_Transform], p: float = 1.0):
        self.transforms: List[_Transform] = list(transforms)
        self.p = float(p)

    def __call__(self, img, mask, g):
        if g.random() >= self.p:
            return img, mask
        for t in self.transforms:
            img, mask = t(img, mask, g)
        return img, mask


class BatchAugment:
    """``SegmentationAlbumentationsTransform.encodes`` on a device batch: pipeline ``aug`` on the first ``ceil(B * n_transform_imgs) - B``
    images (``utils.py:239-291``), the rest unchanged."""

    def __init__(self, aug: Compose, n_transform_imgs: float = 1.0, seed: int = 0):
        if not (0 <= n_transform_imgs <= 1):
            raise ValueError(f"The n_transform_imgs parameter ({n_transform_imgs}) must be between 1 and 0.")       # utils.py:235-237
        self.aug, self.n, self.g = aug, n_transform_imgs, np.random.default_rng(seed)

    def __call__(self, xb: torch.Tensor, yb: torch.Tensor):
        """augments xb [B, C, H, W] / yb [B, H, W] in place and returns them"""
        if any(_device_geometric(t) for t in self.aug.transforms) or (xb.is_cuda and not self.flips_only):
            return self._batched(xb, yb)
        B = xb.shape[0]
        n_transform = math.ceil(B * self.n)
        for i in list(range(B))[:n_transform - B]:
            xi, yi = self.aug(xb[i], yb[i], self.g)
            xb[i], yb[i] = xi, yi
        return xb, yb

    def draw(self, B: int, H: int, W: int, C=None) -> dict:
        """every random draw of ``__call__`` for a batch, image-major in the order of per-image ``Compose`` calls: {(image, transform
        index): parameters} for the transforms that fired"""
        fired = {}
        for i in list(range(B))[:math.ceil(B * self.n) - B]:
            if self.g.random() >= self.aug.p:            # Compose.__call__
                continue
            for k, t in enumerate(self.aug.transforms):
                if self.g.random() < t.p:                # _Transform.__call__
                    fired[i, k] = t.draw_params(self.g, C, H, W)
        return fired

    def segments(self) -> list:
        """the pipeline in execution order: a list of transform indices for each geometric segment (one warp launch over the batch), an
        int for each other transform (run per image).  A segment is a maximal run of geometric transforms with at most one
        interpolating transform.  A field transform (ElasticTransform, GridDistortion, OpticalDistortion) closes its segment, and only D4
        transforms may stand in front of it there: the next geometric transform starts a new segment.

        Composing inside a segment equals applying its transforms one after another: a D4 map (flip, transpose, multiple of 90 degrees)
        permutes the grid exactly, and on a square grid bilinear interpolation and the four border modes commute with it -- the
        bilinear weights and the constant / replicate / reflect / reflect-101 extensions are symmetric under the D4 symmetries of the
        image square.  Sampling a D4-permuted image at q is sampling the image at the permuted q, and permuting a warped image permutes
        its sample points.  Two interpolations in a row are not one interpolation of the composed map, hence one per segment.

        The same argument covers D4 transforms in front of a field transform: with Minv the inverse of the composed D4 maps that fired
        for an image, the field transform samples the permuted image at p + d(p), which is the image itself at Minv (p + d(p)) -- one
        launch that applies Minv to the displaced point.  A transform BEHIND a field transform would have to permute the displacement
        field as well, hence the closed segment."""
        out, seg, interp, closed = [], None, False, False
        for k, t in enumerate(self.aug.transforms):
            if not isinstance(t, _Geometric):
                out.append(k)
                seg = None
                continue
            if seg is None or closed or (t.interpolating and interp):
                seg, interp = [], False
                out.append(seg)
            seg.append(k)
            interp |= t.interpolating
            closed = isinstance(t, _Field)
        return out

    def plan(self) -> list:
        """the launches of ``__call__`` in pipeline order: ("warp", [k, ...]) for a geometric segment (``segments``), ("pixel", [k, ...])
        for a maximal run of pointwise transforms (one ``unet_pixel_ops`` launch over the batch), ("blur", k) for a separable filter
        and ("image", k) for what runs image by image: RandomBrightnessContrast(brightness_by_max=False), which needs the mean of the
        image, and transforms this module does not know"""
        out = []
        for seg in self.segments():
            if not isinstance(seg, int):
                out.append(("warp", seg))
                continue
            t = self.aug.transforms[seg]
            if isinstance(t, _Blur):
                out.append(("blur", seg))
            elif isinstance(t, _Pointwise) and not (isinstance(t, RandomBrightnessContrast) and not t.by_max):
                if out and out[-1][0] == "pixel" and out[-1][1][-1] == seg - 1:
                    out[-1][1].append(seg)
                else:
                    out.append(("pixel", [seg]))
            else:
                out.append(("image", seg))
        return out

    def _pixel_run(self, x, y, run, fired):
        """one launch for the pointwise transforms `run` of every image they fired for (and one per CoarseDropout that fills masks)"""
        from . import ops
        B, C, H, W = x.shape
        ts = self.aug.transforms
        progs = {i: [op for k in run if (i, k) in fired for op in ts[k].program(fired[i, k], C, H, W)] for i in range(B)}
        if any(progs.values()):
            ops.pixel_ops(x, progs)
        for k in run:
            rects = {i: ts[k].mask_rects(fired[i, k]) for i in range(B) if (i, k) in fired}
            rects = {i: r for i, r in rects.items() if r is not None and r[0]}
            if rects:
                ops.fill_rects_mask(y, {i: r[0] for i, r in rects.items()}, next(iter(rects.values()))[1])

    def _batched(self, xb, yb):
        B, C, H, W = xb.shape
        ts = self.aug.transforms
        if H != W:
            for t in ts:
                if isinstance(t, (RandomRotate90, Transpose)):
                    _square(type(t).__name__, H, W)
        for t in ts:
            if isinstance(t, _Pointwise):
                t.check(C, H, W)
        fired = self.draw(B, H, W, C)
        x, y = xb, yb
        for kind, seg in self.plan():
            if kind == "pixel" and x.is_cuda:
                if any((i, k) in fired for i in range(B) for k in seg):
                    if not x.is_contiguous() or (y is not None and not y.is_contiguous()):
                        x, y = x.contiguous(), y.contiguous()
                    self._pixel_run(x, y, seg, fired)
                continue
            if kind == "blur" and x.is_cuda:
                if any((i, seg) in fired for i in range(B)):
                    from . import ops
                    one = np.ones(1, dtype=np.float32)
                    out = torch.empty_like(x, memory_format=torch.contiguous_format)
                    ops.blur_separable(x.contiguous(), out, [ts[seg].taps(fired[i, seg]) if (i, seg) in fired else one for i in range(B)])
                    x = out
                continue
            if kind != "warp":                            # image by image: a transform that needs the whole image, or a batch on the host
                for k in (seg if kind == "pixel" else [seg]):
                    for i in range(B):
                        if (i, k) in fired:
                            x[i], y[i] = ts[k].apply_params(x[i], y[i], fired[i, k])
                continue
            if not any((i, k) in fired for i in range(B) for k in seg):
                continue
            last = ts[seg[-1]]
            maps = np.empty((B, 6), dtype=np.float32)
            for i in range(B):
                fwd = np.eye(3)
                for k in (seg[:-1] if isinstance(last, _Field) else seg):
                    if (i, k) in fired:
                        fwd = ts[k].matrix(fired[i, k], H, W) @ fwd
                maps[i] = inverse_map(fwd)
            if isinstance(last, _Field):               # the D4 maps of the segment go in as the pre-map of the field warp
                x, y = last.warp_batch(x, y, [fired.get((i, seg[-1])) for i in range(B)], maps)
                continue
            lead = next((ts[k] for k in seg if ts[k].interpolating), ts[seg[0]])
            x, y = _warp(x, y, maps, *lead.modes())
        if x is not xb:
            xb.copy_(x)
        if y is not yb:
            yb.copy_(y)
        return xb, yb

    @property
    def flips_only(self) -> bool:
        return all(type(t) in (HorizontalFlip, VerticalFlip) for t in self.aug.transforms)

    def __getattr__(self, name):
        # `flip_flags` exists only for pipelines made of flips (the reference's default, params_and_main.py:105-115): the device feed
        # (learner.DataLoader) then folds the flips into its staging kernels instead of running torch ops per image
        if name == "flip_flags" and self.flips_only:
            return self._flip_flags
        raise AttributeError(name)

    def _flip_flags(self, B: int) -> list:
        """the random draws of ``__call__`` in its order, reduced to (mirror along the width, mirror along the height) per image"""
        fired = self.draw(B, 0, 0)                     # flips draw no parameters: exactly the fire draws of ``__call__``

        def odd(i, flip):
            return sum(type(t) is flip and (i, k) in fired for k, t in enumerate(self.aug.transforms)) % 2 == 1
        return [(odd(i, HorizontalFlip), odd(i, VerticalFlip)) for i in range(B)]


def default_pipeline() -> Compose:
    """the reference's shipped ``aug_pipe`` (params_and_main.py:105-115)"""
    return Compose([HorizontalFlip(p=0.5), VerticalFlip(p=0.5)])
