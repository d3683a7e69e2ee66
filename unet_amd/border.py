"""Distance to the class borders of a batch of masks, and the weight map of the U-Net paper built on it, on the device (csrc/edt.hip,
DESIGN 3.15).  tests/border_ref.py restates every rule below in NumPy; the distances equal it bit for bit.

Masks are [B, H, W] (or one [H, W] image), uint8 or int64, with 1 <= H, W <= 8192 (ValueError above that, from the shape alone: the
squared distance is int32 and 2 * 8191^2 < 2^31).  Every function takes a device tensor, a host tensor or a NumPy array; host input is
uploaded and the result comes back as the same kind.

Border    A pixel is a BORDER pixel of its image when one of its 4-neighbours inside the image has another value.
exclude   With exclude = v, a pair of neighbours in which either value equals v does not count: edges against the NO_Data class
          (exclude=0 for models trained with class_zero) draw no weight.  None: every pair counts.
Distance  D2(p) = min over the border pixels q of the same image of |p - q|^2, an exact integer; 0 on a border pixel.
No border Every pixel of an image without a border pixel gets NO_BORDER = 2^31 - 1.  The images of a batch are independent.
Weight    pw(p) = class_w[y(p)] + w0 * exp(-D2(p) / (2 sigma^2)) in float32 (Ronneberger et al. 2015, eq. 2, with the distance to the
          nearest border in place of the sum of the distances to the two nearest objects).  class_w None: ones.  A target outside
          [0, n_classes) gives 0 (the pixel is ignored, as in the cross-entropy); NO_BORDER gives a border term of exactly 0.

Memory: the result (4 bytes per pixel) and an intermediate of 2 bytes per pixel; the weight map converts a uint8 mask to int64 (8 bytes
per pixel) for the kernel that the loss path shares.

The paper's own form, the distances to the two nearest OBJECTS (csrc/object_edt.hip): distance_to_objects, and
border_weight_map(objects=True).  tests/object_border_ref.py restates these rules; D1 and D2 equal it bit for bit.  Masks as above, with
B * H * W <= 2^31 - 1.

Background  A pixel whose value equals `background` (default 0; a class id 0 ... 255).
Excluded    A pixel whose value equals `exclude` (default None; never the background), or whose value lies outside [0, n_classes)
            (n_classes <= 256; None stands for 256: an object's value is one byte).  It is neither background nor object, it is
            transparent (it blocks nothing) and it gets no term.
Object      A 4-connected component of equal value among the remaining pixels of an image.  Two touching regions of different classes are
            two objects, two touching regions of one class are one.  Instance ids from a separate plane are out of scope; the paper's data
            separates touching cells by a background gap.
delta(p, L) = min over the pixels q of object L in the same image of |p - q|^2, an exact integer.  An object counts for p only if
            delta(p, L) <= radius^2; radius is an int in 1 ... 255.
D1, D2      For a background pixel p: the smallest and the second smallest of delta(p, L) over the DISTINCT objects L that count.  Two
            objects at the same distance give D2 = D1.  NO_OBJECT = 2^31 - 1 stands where there is no such object; D1 alone may be finite.
            At object pixels and excluded pixels both are NO_OBJECT.  Both are functions of the mask and the arguments alone: no tie-break
            enters.  The images of a batch are independent.
Weight      pw(p) = class_w[y(p)] + w0 * exp(-(sqrt D1 + sqrt D2)^2 / (2 sigma^2)) in float32 (Ronneberger et al. 2015, eq. 2).  The second
            term is exactly 0 wherever D2 is NO_OBJECT; a target outside [0, n_classes) gives 0.  The exponent is formed in fp64 from the
            exact integers, as D1 + D2 + 2 sqrt(D1 D2), and rounded to fp32 once.
Radius      radius=None in the weight map means ceil(6 sigma): what the cap drops is below w0 * e^-18.  ceil(6 sigma) > 255 raises a
            ValueError that asks for an explicit radius.

Memory of the object form: a workspace of 18 bytes per pixel (key 4, label 4, two candidates per pixel of 1 + 4 bytes each) besides the
results."""
from __future__ import annotations

from typing import Optional

import math

import numpy as np
import torch

from . import ops

NO_BORDER = ops.EDT_NO_BORDER
NO_OBJECT = ops.OBJ_NO_OBJECT


def _alloc(shape, dtype, device) -> torch.Tensor:
    """every device buffer of this module (the tests put guard bands around them here)"""
    return torch.empty(tuple(shape), dtype=dtype, device=device)


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _check_exclude(exclude):
    if exclude is not None and (not _is_int(exclude) or not 0 <= exclude < 2 ** 31):
        raise ValueError(f"exclude must be None or a class id >= 0, got {exclude!r}")
    return None if exclude is None else int(exclude)


def check_border_params(w0, sigma, exclude=None):
    """(w0, sigma, exclude) of a weight map, validated: w0 >= 0, sigma > 0, exclude None or a class id"""
    if isinstance(w0, bool) or not isinstance(w0, (int, float, np.integer, np.floating)) or not w0 >= 0:
        raise ValueError(f"border weight: w0 must be a number >= 0, got {w0!r}")
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not sigma > 0:
        raise ValueError(f"border weight: sigma must be a number > 0, got {sigma!r}")
    return float(w0), float(sigma), _check_exclude(exclude)


def check_object_params(sigma, objects=False, background=0, radius=None, exclude=None):
    """(objects, background, radius) of a weight map, validated.  objects False: the other two are checked and otherwise unused.  radius
    None: ceil(6 sigma); the radius is an int in 1 ... 255, the background a class id 0 ... 255 other than `exclude`"""
    if not isinstance(objects, (bool, np.bool_)):
        raise ValueError(f"border weight: objects must be True or False, got {objects!r}")
    if not _is_int(background) or not 0 <= background <= 255:
        raise ValueError(f"border weight: background must be a class id 0 ... 255, got {background!r}")
    if radius is not None and (not _is_int(radius) or not 1 <= radius <= ops.OBJ_MAX_RADIUS):
        raise ValueError(f"border weight: radius must be None or an int in 1 ... {ops.OBJ_MAX_RADIUS}, got {radius!r}")
    if objects:
        if exclude is not None and int(exclude) == int(background):
            raise ValueError(f"border weight: exclude and background are both {background}: with objects=True name another background class")
        if radius is None and math.ceil(6.0 * float(sigma)) > ops.OBJ_MAX_RADIUS:
            raise ValueError(f"border weight: ceil(6 sigma) = {math.ceil(6.0 * float(sigma))} exceeds {ops.OBJ_MAX_RADIUS}: give an explicit "
                             f"radius in 1 ... {ops.OBJ_MAX_RADIUS}")
    return bool(objects), int(background), None if radius is None else int(radius)


def object_radius(sigma: float, radius=None) -> int:
    """the radius a weight map with objects=True uses: `radius`, or ceil(6 sigma) (at least 1)"""
    return int(radius) if radius is not None else max(1, math.ceil(6.0 * float(sigma)))


def _to_device(a, what: str):
    """(contiguous device tensor [B, H, W], back) -- back(t) returns t shaped and placed as `a` (device tensor, host tensor, NumPy array)"""
    shape = tuple(getattr(a, "shape", ()))
    single = len(shape) == 2
    ops.check_edt_shape(what, (1,) + shape if single else shape)
    if isinstance(a, np.ndarray):
        if a.dtype not in (np.dtype("uint8"), np.dtype("int64")):
            raise ValueError(f"{what}: expected uint8 or int64 samples, got {a.dtype}")
        t, kind = torch.from_numpy(np.ascontiguousarray(a)), "numpy"
    elif isinstance(a, torch.Tensor):
        if a.dtype not in (torch.uint8, torch.int64):
            raise ValueError(f"{what}: expected uint8 or int64 samples, got {a.dtype}")
        if not a.is_cuda and a.device.type != "cpu":
            raise ValueError(f"{what}: tensor on device {a.device}")
        t, kind = a, "device" if a.is_cuda else "host"
    else:
        raise ValueError(f"{what}: expected a torch tensor or a NumPy array, got {type(a).__name__}")
    t = t.contiguous()
    if not t.is_cuda:
        t = t.cuda()
    if single:
        t = t.unsqueeze(0)

    def back(r: torch.Tensor):
        r = r.reshape(shape)
        return r if kind == "device" else r.cpu() if kind == "host" else r.cpu().numpy()
    return t, back


def _distance(m: torch.Tensor, exclude) -> torch.Tensor:
    B, H, W = m.shape
    d2 = _alloc(m.shape, torch.int32, m.device)
    ws = _alloc((ops.edt_workspace(B, H, W),), torch.uint8, m.device)
    ops.border_edt(m, d2, ws, exclude)
    return d2


def distance_to_border(mask, exclude: Optional[int] = None):
    """int32, shaped as the mask: the squared Euclidean distance of every pixel to the nearest border pixel of its image; NO_BORDER where
    the image has none (the module docstring has the rules)"""
    exclude = _check_exclude(exclude)
    m, back = _to_device(mask, "distance_to_border")
    return back(_distance(m, exclude))


def _object_workspace(m: torch.Tensor) -> torch.Tensor:
    B, H, W = m.shape
    return _alloc((ops.object_edt_workspace(B, H, W),), torch.uint8, m.device)


def _check_labelling(ws: torch.Tensor):
    """the give-up word of the labelling (the last 16 bytes of the workspace): an error, never a retry"""
    ops.postprocess_counters(ws[ws.numel() - 16:].view(torch.int32))


def distance_to_objects(mask, background: int = 0, exclude: Optional[int] = None, radius: int = 30, n_classes: Optional[int] = None):
    """(D1, D2), int32, shaped as the mask: for every background pixel the squared Euclidean distances to the nearest and the second nearest
    distinct object of its image within `radius`; NO_OBJECT where there is none, and at object and excluded pixels (the module docstring
    has the rules)"""
    exclude = _check_exclude(exclude)
    if radius is None:
        raise ValueError("distance_to_objects: radius must be an int in 1 ... 255")
    _, background, radius = check_object_params(1.0, True, background, radius, exclude)
    if n_classes is not None and (not _is_int(n_classes) or not 1 <= n_classes <= ops.OBJ_MAX_CLASSES):
        raise ValueError(f"distance_to_objects: n_classes must be None or an int in 1 ... {ops.OBJ_MAX_CLASSES}, got {n_classes!r}")
    shape = tuple(getattr(mask, "shape", ()))
    ops.check_object_shape("distance_to_objects", (1,) + shape if len(shape) == 2 else shape)
    m, back = _to_device(mask, "distance_to_objects")
    d1, d2 = _alloc(m.shape, torch.int32, m.device), _alloc(m.shape, torch.int32, m.device)
    ws = _object_workspace(m)
    ops.object_edt(m, d1, d2, ws, background, exclude, ops.OBJ_MAX_CLASSES if n_classes is None else int(n_classes), radius)
    _check_labelling(ws)
    return back(d1), back(d2)


def border_weight_map(mask, class_weights=None, w0: float = 10.0, sigma: float = 5.0, exclude: Optional[int] = None,
                      n_classes: Optional[int] = None, objects: bool = False, background: int = 0, radius: Optional[int] = None):
    """float32, shaped as the mask: class_weights[y] + w0 * exp(-D2 / (2 sigma^2)) (the module docstring has the rules).  class_weights:
    None (ones) or n_classes numbers; n_classes: their count, needed when class_weights is None -- targets outside [0, n_classes) weigh 0.
    objects=True: the border term is w0 * exp(-(sqrt D1 + sqrt D2)^2 / (2 sigma^2)) of the two nearest objects around the `background`
    class within `radius` (None: ceil(6 sigma)); `exclude` then names the class that is neither; n_classes <= 256."""
    w0, sigma, exclude = check_border_params(w0, sigma, exclude)
    objects, background, radius = check_object_params(sigma, objects, background, radius, exclude)
    if class_weights is not None:
        cw = torch.as_tensor(class_weights, dtype=torch.float32).reshape(-1)
        if n_classes is None:
            n_classes = cw.numel()
        if cw.numel() != n_classes:
            raise ValueError(f"border_weight_map: {cw.numel()} class weights for n_classes = {n_classes}")
    if not _is_int(n_classes) or n_classes < 1:
        raise ValueError(f"border_weight_map: n_classes must be an int >= 1 (or give class_weights), got {n_classes!r}")
    if objects and n_classes > ops.OBJ_MAX_CLASSES:
        raise ValueError(f"border_weight_map: objects=True supports at most {ops.OBJ_MAX_CLASSES} classes, got {n_classes}")
    m, back = _to_device(mask, "border_weight_map")
    if objects:
        ops.check_object_shape("border_weight_map", tuple(m.shape))
        cwd = None
        if class_weights is not None:
            cwd = _alloc((n_classes,), torch.float32, m.device)
            cwd.copy_(cw)
        pw = _alloc(m.shape, torch.float32, m.device)
        ws = _object_workspace(m)
        ops.object_border_weight(m, cwd, int(n_classes), w0, sigma, pw, ws, background, exclude, object_radius(sigma, radius))
        _check_labelling(ws)
        return back(pw)
    d2 = _distance(m, exclude)
    if m.dtype != torch.int64:
        y = _alloc(m.shape, torch.int64, m.device)
        y.copy_(m)
    else:
        y = m
    cwd = None
    if class_weights is not None:
        cwd = _alloc((n_classes,), torch.float32, m.device)
        cwd.copy_(cw)
    pw = _alloc(m.shape, torch.float32, m.device)
    ops.border_weight(d2, y, cwd, int(n_classes), w0, sigma, pw)
    return back(pw)
