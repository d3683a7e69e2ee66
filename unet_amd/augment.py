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
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np
import torch


class _Transform:
    """A transform fires with probability ``p`` (drawn first); only then are its parameters drawn (``get_params``) and applied
    (``apply_params``).  The split lets ``BatchAugment`` draw a whole batch before anything runs."""

    def __init__(self, p: float = 0.5, always_apply: bool = False):
        self.p = 1.0 if always_apply else float(p)

    def get_params(self, g: np.random.Generator, H: int, W: int):
        """the random parameters of one application to an H x W image (none by default)"""
        return None

    def apply_params(self, img: torch.Tensor, mask: torch.Tensor, prm) -> Tuple[torch.Tensor, torch.Tensor]:
        raise NotImplementedError

    def apply(self, img: torch.Tensor, mask: torch.Tensor, g: np.random.Generator) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.apply_params(img, mask, self.get_params(g, *img.shape[-2:]))

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


_NEW_GEOMETRIC = (RandomRotate90, Transpose, Rotate, ShiftScaleRotate)


def inverse_map(forward: np.ndarray) -> np.ndarray:
    """the output -> source map of a 3 x 3 forward map as the 6 fp32 entries the warp kernels take.  Inverted in fp64; entries within
    1e-9 of a multiple of 0.5 are snapped to it, so that D4 maps and multiples of 90 degrees are exact permutations of the grid."""
    inv = np.linalg.inv(np.asarray(forward, dtype=np.float64))[:2].reshape(6)
    half = np.round(inv * 2.0) / 2.0
    inv = np.where(np.abs(inv - half) <= 1e-9, half, inv)
    return inv.astype(np.float32)


def _warp(img: torch.Tensor, mask, inv_maps: np.ndarray, interp: int, border: int, fill: float, mask_fill: float):
    """image batch [n, C, H, W] fp32 and mask batch [n, H, W] (or None) warped by inv_maps [n, 6] into new tensors"""
    from . import ops
    out = torch.empty_like(img)
    ops.warp_affine(img.contiguous(), out, inv_maps, interp, border, fill)
    if mask is None:
        return out, None
    mout = torch.empty_like(mask)
    ops.warp_affine_mask(mask.contiguous(), mout, inv_maps, border, mask_fill)
    return out, mout


class RandomBrightnessContrast(_Transform):
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


class CoarseDropout(_Transform):
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
        if any(isinstance(t, _NEW_GEOMETRIC) for t in self.aug.transforms):
            return self._batched(xb, yb)
        B = xb.shape[0]
        n_transform = math.ceil(B * self.n)
        for i in list(range(B))[:n_transform - B]:
            xi, yi = self.aug(xb[i], yb[i], self.g)
            xb[i], yb[i] = xi, yi
        return xb, yb

    def draw(self, B: int, H: int, W: int) -> dict:
        """every random draw of ``__call__`` for a batch, image-major in the order of per-image ``Compose`` calls: {(image, transform
        index): parameters} for the transforms that fired"""
        fired = {}
        for i in list(range(B))[:math.ceil(B * self.n) - B]:
            if self.g.random() >= self.aug.p:            # Compose.__call__
                continue
            for k, t in enumerate(self.aug.transforms):
                if self.g.random() < t.p:                # _Transform.__call__
                    fired[i, k] = t.get_params(self.g, H, W)
        return fired

    def segments(self) -> list:
        """the pipeline in execution order: a list of transform indices for each geometric segment (one warp launch over the batch), an
        int for each other transform (run per image).  A segment is a maximal run of geometric transforms with at most one
        interpolating transform.

        Composing inside a segment equals applying its transforms one after another: a D4 map (flip, transpose, multiple of 90 degrees)
        permutes the grid exactly, and on a square grid bilinear interpolation and the four border modes commute with it -- the
        bilinear weights and the constant / replicate / reflect / reflect-101 extensions are symmetric under the D4 symmetries of the
        image square.  Sampling a D4-permuted image at q is sampling the image at the permuted q, and permuting a warped image permutes
        its sample points.  Two interpolations in a row are not one interpolation of the composed map, hence one per segment."""
        out, seg, interp = [], None, False
        for k, t in enumerate(self.aug.transforms):
            if not isinstance(t, _Geometric):
                out.append(k)
                seg = None
                continue
            if seg is None or (t.interpolating and interp):
                seg, interp = [], False
                out.append(seg)
            seg.append(k)
            interp |= t.interpolating
        return out

    def _batched(self, xb, yb):
        B, H, W = xb.shape[0], xb.shape[-2], xb.shape[-1]
        ts = self.aug.transforms
        if H != W:
            for t in ts:
                if isinstance(t, (RandomRotate90, Transpose)):
                    _square(type(t).__name__, H, W)
        fired = self.draw(B, H, W)
        x, y = xb, yb
        for seg in self.segments():
            if isinstance(seg, int):
                t = ts[seg]
                for i in range(B):
                    if (i, seg) in fired:
                        x[i], y[i] = t.apply_params(x[i], y[i], fired[i, seg])
                continue
            if not any((i, k) in fired for i in range(B) for k in seg):
                continue
            maps = np.empty((B, 6), dtype=np.float32)
            for i in range(B):
                fwd = np.eye(3)
                for k in seg:
                    if (i, k) in fired:
                        fwd = ts[k].matrix(fired[i, k], H, W) @ fwd
                maps[i] = inverse_map(fwd)
            lead = next((ts[k] for k in seg if ts[k].interpolating), ts[seg[0]])
            x, y = _warp(x, y, maps, *lead.modes())
        if x is not xb:
            xb.copy_(x)
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
        n_transform = math.ceil(B * self.n)
        flags = [(False, False)] * B
        for i in list(range(B))[:n_transform - B]:
            h = v = False
            if self.g.random() < self.aug.p:           # Compose.__call__: `if g.random() >= self.p: return`
                for t in self.aug.transforms:          # _Transform.__call__: `if g.random() < self.p: apply`
                    if self.g.random() < t.p:
                        if type(t) is HorizontalFlip:
                            h = not h
                        else:
                            v = not v
            flags[i] = (h, v)
        return flags


def default_pipeline() -> Compose:
    """the reference's shipped ``aug_pipe`` (params_and_main.py:105-115)"""
    return Compose([HorizontalFlip(p=0.5), VerticalFlip(p=0.5)])
