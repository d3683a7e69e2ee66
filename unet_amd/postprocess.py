"""Clean-up of a merged uint8 class mask on the device: connected components, a majority filter and a small-region sieve
(csrc/postprocess.hip).  tests/postprocess_ref.py restates every rule below in NumPy; the device results equal it bit for bit.

Masks are contiguous uint8 [H, W] with class ids 0..255 and H * W <= 2^31 - 1 (ValueError above that, from the shape alone).  Every
function takes a device tensor, a host tensor or a NumPy array; host input is uploaded and the result comes back as the same kind.

Components  A component is a maximal set of equal-class pixels connected by 4- or 8-adjacency.  Its label is the smallest linear index
            y * W + x of its pixels: canonical, so the result does not depend on how the kernels were scheduled.
Majority    k x k window (k odd, 3..15) clipped to the raster, only pixels that exist vote; the class with the highest count wins, on
            a tie the centre's own class if it is among the tied ones, else the smallest id.  One Jacobi pass (reads the input, writes
            a separate output).  Pixels of frozen_class neither vote nor change.
Sieve       Rounds of: label the mask; a component is SMALL if it has fewer than min_pixels pixels and its class is not frozen_class;
            its neighbours are the components that hold a pixel EDGE-adjacent (4-adjacency, also at connectivity 8, as GDAL's sieve)
            to one of its pixels and whose class is not frozen_class; best = the neighbour with the largest (size, -label); the
            component merges iff it has a neighbour and (size, -label) of best exceeds its own; all merges of a round happen at once
            and every pixel of a merging component takes the class best had in the round's input.  Rounds repeat until one merges nothing
            or max_rounds rounds are done: simultaneous merges do not provably shrink the component count, the cap is what ends the run,
            and components still small when it is hit stay as they are.
            NOT bit-compatible with gdal_sieve, which iterates and merges differently.

Memory: labels (int32) + sizes (int32) + keys (uint64) are 16 bytes per pixel -- 6.4 GB for a 20000 x 20000 scene -- beside two mask
buffers of the sieve (1 byte per pixel each)."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import ops

_NO_SIEVE = {"rounds": 0, "merged": [], "small_left": 0}


def _alloc(shape, dtype, device) -> torch.Tensor:
    """every device buffer of this module (the tests put guard bands around them here)"""
    return torch.empty(tuple(shape), dtype=dtype, device=device)


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _check_k(k):
    if not _is_int(k) or k < 3 or k > 15 or k % 2 == 0:
        raise ValueError(f"majority filter: k must be an odd int in 3..15, got {k!r}")
    return int(k)


def _check_conn(connectivity):
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def _check_frozen(frozen_class):
    if frozen_class is not None and (not _is_int(frozen_class) or not 0 <= frozen_class <= 255):
        raise ValueError(f"frozen_class must be None or an int in 0..255, got {frozen_class!r}")
    return None if frozen_class is None else int(frozen_class)


def _check_sieve(min_pixels, max_rounds):
    if not _is_int(min_pixels) or min_pixels < 0:
        raise ValueError(f"sieve: min_pixels must be an int >= 0, got {min_pixels!r}")
    if not _is_int(max_rounds) or max_rounds < 1:
        raise ValueError(f"sieve: max_rounds must be an int >= 1, got {max_rounds!r}")
    return int(min_pixels), int(max_rounds)


def _to_device(a, dtype, what: str):
    """(contiguous device tensor, back) -- back(t) returns t as the kind of `a` (device tensor, host tensor, NumPy array)"""
    ops.check_mask_shape(what, getattr(a, "shape", ()))
    if isinstance(a, np.ndarray):
        if a.dtype != np.dtype(str(dtype).split(".")[-1]):
            raise ValueError(f"{what}: expected {dtype} samples, got {a.dtype}")
        return torch.from_numpy(np.ascontiguousarray(a)).cuda(), lambda t: t.cpu().numpy()
    if not isinstance(a, torch.Tensor):
        raise ValueError(f"{what}: expected a torch tensor or a NumPy array, got {type(a).__name__}")
    if a.dtype != dtype:
        raise ValueError(f"{what}: expected {dtype} samples, got {a.dtype}")
    if a.is_cuda:
        return a.contiguous(), lambda t: t
    if a.device.type != "cpu":
        raise ValueError(f"{what}: tensor on device {a.device}")
    return a.contiguous().cuda(), lambda t: t.cpu()


def _label(mask: torch.Tensor, connectivity: int) -> torch.Tensor:
    labels = _alloc(mask.shape, torch.int32, mask.device)
    counters = _alloc((4,), torch.int32, mask.device)
    ops.cc_label(mask, connectivity, labels, counters)
    ops.postprocess_counters(counters)          # the give-up word: an error, never a retry
    return labels


def label_components(mask, connectivity: int = 4):
    """int32 [H, W]: every pixel's label is the smallest linear index y * W + x of its component (equal class, 4- / 8-adjacency)"""
    connectivity = _check_conn(connectivity)
    m, back = _to_device(mask, torch.uint8, "label_components")
    return back(_label(m, connectivity))


def component_sizes(labels):
    """int32 [H, W] from the labels of label_components: the pixel count of a component at the index that is its label, 0 elsewhere"""
    l, back = _to_device(labels, torch.int32, "component_sizes")
    sizes = _alloc(l.shape, torch.int32, l.device)
    ops.cc_sizes(l, sizes)
    return back(sizes)


def _majority(m: torch.Tensor, k: int, frozen_class) -> torch.Tensor:
    out = _alloc(m.shape, torch.uint8, m.device)
    ops.majority_filter(m, out, k, frozen_class)
    return out


def majority_filter(mask, k: int, frozen_class: Optional[int] = None):
    """k x k majority vote, k odd in 3..15 (the module docstring has the rule); returns a new mask"""
    k, frozen_class = _check_k(k), _check_frozen(frozen_class)
    m, back = _to_device(mask, torch.uint8, "majority_filter")
    return back(_majority(m, k, frozen_class))


def _copy(m: torch.Tensor) -> torch.Tensor:
    out = _alloc(m.shape, m.dtype, m.device)
    out.copy_(m)
    return out


def _sieve(m: torch.Tensor, min_pixels: int, connectivity: int, max_rounds: int, frozen_class) -> Tuple[torch.Tensor, dict]:
    if min_pixels <= 1:
        return _copy(m), dict(_NO_SIEVE, merged=[])
    dev = m.device
    labels, sizes = _alloc(m.shape, torch.int32, dev), _alloc(m.shape, torch.int32, dev)
    keys = _alloc(m.shape, torch.int64, dev)
    counters = _alloc((4,), torch.int32, dev)
    bufs = [_alloc(m.shape, torch.uint8, dev), None]
    cur, merged, small_left = m, [], None
    for r in range(max_rounds):
        nxt = bufs[r % 2]
        if nxt is None:
            nxt = bufs[r % 2] = _alloc(m.shape, torch.uint8, dev)
        ops.sieve_round(cur, nxt, connectivity, min_pixels, frozen_class, labels, sizes, keys, counters)
        n_merged, n_left = ops.postprocess_counters(counters)          # the only host sync of a round
        merged.append(n_merged)
        if n_merged == 0:              # nxt equals cur; every small component is one that stays
            small_left = n_left
            break
        cur = nxt
    if small_left is None:             # the cap ended the run: count what is still small in the result
        ops.sieve_round(cur, None, connectivity, min_pixels, frozen_class, labels, sizes, None, counters)
        small_left = ops.postprocess_counters(counters)[1]
    out = _copy(m) if cur is m else cur
    return out, {"rounds": len(merged), "merged": merged, "small_left": small_left}


def sieve(mask, min_pixels: int, connectivity: int = 4, max_rounds: int = 16, frozen_class: Optional[int] = None):
    """Small-region sieve (the module docstring has the rule).  Returns (mask, info) with info = {"rounds": rounds run (the one that merged
    nothing included), "merged": [components merged per round], "small_left": small components of the returned mask}.  min_pixels <= 1 is
    a no-op.  Components still small after max_rounds rounds stay as they are.  Not bit-compatible with gdal_sieve."""
    (min_pixels, max_rounds), connectivity, frozen_class = _check_sieve(min_pixels, max_rounds), _check_conn(connectivity), _check_frozen(frozen_class)
    m, back = _to_device(mask, torch.uint8, "sieve")
    out, info = _sieve(m, min_pixels, connectivity, max_rounds, frozen_class)
    return back(out), info


class PostProcess:
    """majority filter (majority = k, 0: off), then sieve (sieve = min_pixels, 0: off) of a class mask.  frozen_class: a class that
    neither votes, changes, merges nor is merged into -- 0, the NO_Data class, for models trained with class_zero.  Works on the
    model's class ids (before store_tif shifts them)."""

    def __init__(self, majority: int = 0, sieve: int = 0, connectivity: int = 4, max_rounds: int = 16, frozen_class: Optional[int] = None):
        if not (_is_int(majority) and majority == 0):
            _check_k(majority)
        self.sieve, self.max_rounds = _check_sieve(sieve, max_rounds)
        self.majority, self.connectivity, self.frozen_class = int(majority), _check_conn(connectivity), _check_frozen(frozen_class)

    def __repr__(self):
        return (f"PostProcess(majority={self.majority}, sieve={self.sieve}, connectivity={self.connectivity}, max_rounds={self.max_rounds}, "
                f"frozen_class={self.frozen_class})")

    def run(self, mask):
        """(mask, info of the sieve)"""
        m, back = _to_device(mask, torch.uint8, "PostProcess")
        out = _majority(m, self.majority, self.frozen_class) if self.majority else m
        out, info = _sieve(out, self.sieve, self.connectivity, self.max_rounds, self.frozen_class)
        return back(out), info

    def __call__(self, mask):
        return self.run(mask)[0]


def check_postprocess(postprocess):
    """the postprocess= argument of predict_raster / save_predictions (None | PostProcess | dict of its arguments) -> PostProcess or None;
    which outputs take one is predict.check_outputs' rule"""
    if postprocess is None:
        return None
    if isinstance(postprocess, dict):
        try:
            postprocess = PostProcess(**postprocess)
        except TypeError as e:
            raise ValueError(f"postprocess={postprocess!r}: {e}") from None
    if not isinstance(postprocess, PostProcess):
        raise ValueError(f"postprocess must be None, a PostProcess or a dict of its arguments, got {type(postprocess).__name__}")
    return postprocess
