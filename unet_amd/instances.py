"""Touching objects of one class split into instances on the device (csrc/instances.hip): a watershed of a capped distance
transform whose shallow basins are merged back.  tests/instances_ref.py restates every rule below sequentially in NumPy / plain Python; the
device result equals it bit for bit, whatever the schedule.

split_instances(mask, classes, radius=64, min_depth=2.0, max_rounds=64) -> (labels, info).  mask is a contiguous uint8 [H, W] with
H * W <= 2^31 - 1 (a device tensor, a host tensor or a NumPy array; host input is uploaded and the labels come back as the same kind).  The
result is a function of (mask, classes, radius, min_depth, max_rounds) alone.

Arguments   classes: an int or an iterable of class ids 0..255, the classes to split.  radius R: an int in 1..255.  min_depth: a number in
            0..255, quantised to q = floor(16 min_depth + 0.5) sixteenths of a pixel.  max_rounds: an int >= 1.  Bad values raise
            ValueError before anything touches the GPU.
Height      for a pixel p of a split class, h(p) = min(R^2, min |p - r|^2 over the pixels r INSIDE the raster with mask[r] != mask[p]):
            an exact integer <= 65025.  Outside the raster there is no pixel, so the raster frame lowers nothing, and a mask of one
            class has h = R^2 everywhere.  Every pixel of a class that is not split has h = 0.
Flat zones  a zone is a maximal 4-connected set of pixels with equal (class, h); its label is the smallest linear index y * W + x of its
            pixels.  A class that is not split has exactly its components as zones, with the labels of label_components(mask, 4).
Ascent      zone Z looks at every pixel u that is 4-adjacent to one of its pixels, has its class and has h(u) greater than Z's height.
            The u with the largest (h(u), -index(u)) wins and Z points to the zone of that u.  A zone without such a pixel is a SEED.
            Heights strictly increase along the pointers, so following them ends in a seed; a segment is the set of pixels whose zones
            end in one seed, its id is that seed's zone label, and it is 4-connected by construction.
Merging     in rounds, on the current segments.  peak(A) = the largest h in A.  Every 4-adjacent pixel pair (p in A, r in B) of equal
            class with A != B has the pass min(h(p), h(r)).  best(A) = the neighbour B with the largest (pass, -id(B)) over all such
            pairs.  A merges into B = best(A) iff A is SHALLOW against that pass and (peak(A), -id(A)) < (peak(B), -id(B)),
            lexicographically.  Shallow means sqrt(peak(A)) - sqrt(pass) < q / 16, evaluated exactly in int64: with
            L = 256 (peak - pass) - q^2, A is shallow iff L < 0 or L^2 < 1024 q^2 pass.  With q = 0 nothing is ever shallow: the plain
            watershed of the distance.  All merges of a round happen at once; chains A -> B -> C are followed to their end (the strict
            order rules out cycles) and the merged segment carries the id of that end.  Rounds repeat until one merges nothing or
            max_rounds rounds are done.
Result      labels[p] (int32 [H, W]) = the smallest linear index of p's final segment, the convention of label_components: canonical.
            info = {"seeds": the number of seeds, "segments": the final count, "rounds": the rounds run (the one that merged nothing
            included), "merged": [segments that merged, per round]}.  Seeds and segments count the components of the classes that are
            not split as well: each is one zone, one seed and one segment.
Not offered markers from probability maps; compact or 8-connected watersheds; smoothing of the height; identity with
            skimage.segmentation.watershed / h_maxima, which iterate sequentially and break ties differently.

Passes: the capped distance (a row pass into a byte image g = the horizontal distance capped at R, then a column pass that takes the
minimum over |dy| <= R of dy^2 + g(y + dy, x)^2, or dy^2 alone at a row of another value, where a direction ends; both stage their
rows / columns in LDS with a halo of R); the zones (the labelling kernels of postprocess.hip on the keys class << 16 | h); the ascent (a
64-bit atomic maximum per zone of h(u) << 32 | ~index(u), then pointer doubling over the zone roots in groups with the convergence words
of vectorize.py, then a gather); per merge round one pass for peak and best (atomic maxima; best takes pass << 32 | ~id(B)), the decision
per segment, ceil(log2 segments) doubling launches over the merge pointers (those behind a round that moved nothing return at once) and a
gather; the canonical labels (an atomic minimum per segment, a gather).  Atomics take maxima and minima of integers only; counts are block
sums added up with torch.  Host reads: the give-up word of the labelling, the seeds, one word per doubling group of the ascent, one word
per merge round read once per group of 4 rounds, the segments; none per segment.

Memory: 30 bytes per pixel at the peak -- the mask 1, g 1 (freed after the distance), keys 4, zones / segments 4, the 64-bit maxima 8, two
pointer buffers 8 (they end as the minima and the labels), peak 4 -- 12 GB for a 20000 x 20000 scene.  Every buffer that a kernel
writes comes from _alloc.

instance_ids(mask, labels, classes) numbers the segments of the split classes 1..N in ascending label order (0 on every other pixel):
root marks, the byte scan of vectorize.py and a gather.  Instances / check_instances are the instances= argument of predict_raster and
save_predictions."""
from __future__ import annotations

import math
import time
from typing import Optional

import numpy as np
import torch

from . import ops
from .postprocess import _is_int, _to_device
from .vectorize import _Stages, _doubling, check_exclude

_ROUND_GROUP = 4          # merge rounds per host look at their merge counts
MAX_RADIUS = 255
MAX_DEPTH = 255


def _alloc(shape, dtype, device) -> torch.Tensor:
    """every device buffer that a kernel of this module writes (the tests put guard bands around them here)"""
    return torch.empty(tuple(shape), dtype=dtype, device=device)


def check_classes(classes) -> tuple:
    """an int or an iterable of class ids 0..255 -> a sorted tuple (never empty)"""
    if classes is None:
        raise ValueError("classes must be an int or an iterable of class ids 0..255, got None")
    try:
        out = check_exclude(classes)
    except ValueError as e:
        raise ValueError(str(e).replace("exclude", "classes")) from None
    if not out:
        raise ValueError("classes names no class to split")
    return out


def check_split(radius, min_depth, max_rounds) -> tuple:
    """-> (radius, q = floor(16 min_depth + 0.5), max_rounds)"""
    if not _is_int(radius) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius must be an int in 1..{MAX_RADIUS}, got {radius!r}")
    if isinstance(min_depth, bool) or not isinstance(min_depth, (int, float, np.integer, np.floating)) or not math.isfinite(min_depth) \
            or not 0 <= min_depth <= MAX_DEPTH:
        raise ValueError(f"min_depth must be a number in 0..{MAX_DEPTH} pixels, got {min_depth!r}")
    if not _is_int(max_rounds) or max_rounds < 1:
        raise ValueError(f"max_rounds must be an int >= 1, got {max_rounds!r}")
    return int(radius), int(math.floor(16.0 * float(min_depth) + 0.5)), int(max_rounds)


def _total(partial: torch.Tensor) -> int:
    return ops.vec_read(partial.sum().reshape(1), 0, 1)[0]          # a host read


def _split(m: torch.Tensor, classes: tuple, R: int, q: int, max_rounds: int, stages: Optional[dict] = None):
    st = _Stages(stages)
    dev = m.device
    H, W = m.shape
    n = H * W
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    g, keys = _alloc((H, W), u8, dev), _alloc((H, W), i32, dev)
    ops.inst_distance(m, classes, R, g, keys)
    del g
    st.mark("distance")
    seg, counters = _alloc((H, W), i32, dev), _alloc((4,), i32, dev)
    ops.cc_label_keys(keys, seg, counters)
    ops.postprocess_counters(counters)          # the give-up word: an error, never a retry
    st.mark("zones")
    best = _alloc((H, W), i64, dev)
    pa, pb = _alloc((H, W), i32, dev), _alloc((H, W), i32, dev)
    partial = _alloc((_ROUND_GROUP, ops.inst_partials()), i64, dev)
    changed = _alloc((32,), i64, dev)
    ch32 = changed.view(i32)
    ops.inst_ascent(keys, seg, best, pa, partial[0])
    seeds = _total(partial[0])
    ptr, _ = _doubling(n, lambda a, b, k: ops.inst_ptr_rounds(seg, a, b, k, ch32), pa, pb, changed)
    ops.inst_gather(seg, ptr, seg)
    st.mark("ascent")
    peak = _alloc((H, W), i32, dev)
    merged, segments = [], seeds
    while len(merged) < max_rounds:
        k = min(_ROUND_GROUP, max_rounds - len(merged))
        doublings = max(1, (segments - 1).bit_length())          # a chain of merges is shorter than the segment count
        for r in range(k):
            ops.inst_merge_round(keys, seg, q, doublings, peak, best, pa, pb, ch32, partial[r])
        counts = ops.vec_read(partial[:k].sum(1), 0, k)          # a host read: one word per round of the group
        done = False
        for c in counts:          # the rounds behind one that merged nothing found the same segments and merged nothing either
            merged.append(c)
            segments -= c
            if c == 0:
                done = True
                break
        if done:
            break
    st.mark("merge")
    ops.inst_canonical(seg, pa, pb, partial[0])
    final = _total(partial[0])
    st.mark("canonical")
    return pb, {"seeds": seeds, "segments": final, "rounds": len(merged), "merged": merged}


def split_instances(mask, classes, radius: int = 64, min_depth: float = 2.0, max_rounds: int = 64, stages: Optional[dict] = None):
    """(labels, info) of the module docstring: int32 [H, W] labels of the kind of `mask` (device tensor, host tensor, NumPy array) and
    {"seeds", "segments", "rounds", "merged"}.  stages: a dict that receives the milliseconds of distance, zones, ascent, merge and
    canonical (this synchronises the device after each: for measurements only)."""
    classes = check_classes(classes)
    R, q, max_rounds = check_split(radius, min_depth, max_rounds)
    m, back = _to_device(mask, torch.uint8, "split_instances")
    labels, info = _split(m, classes, R, q, max_rounds, stages)
    return back(labels), info


def instance_ids(mask, labels, classes):
    """(ids, N): ids int32 [H, W] on the device (non-negative: read them as uint32) = the dense id 1..N, in ascending label order, of every
    pixel's segment for the classes in `classes`, 0 on every other pixel.  mask and labels are device tensors (uint8, int32)"""
    classes = check_classes(classes)
    dev = mask.device
    n = mask.numel()
    mark, offs = _alloc(mask.shape, torch.uint8, dev), _alloc(mask.shape, torch.int32, dev)
    blocks = _alloc((ops.vec_scan_words(n),), torch.int64, dev)
    ops.inst_marks(mask, labels, classes, mark)
    ops.vec_scan(mark, offs, blocks)
    count = ops.vec_read(blocks, ops.vec_scan_words(n) - 1, 1)[0]          # a host read
    ids = _alloc(mask.shape, torch.int32, dev)
    ops.inst_ids(mask, labels, offs, classes, ids)
    return ids, count


class Instances:
    """the instances= argument of predict_raster / save_predictions: split_instances(mask, classes, radius, min_depth, max_rounds) of the merged
    class mask, after the post-processing.  classes are the model's class ids (before store_tif shifts them under class_zero)."""

    def __init__(self, classes, radius: int = 64, min_depth: float = 2.0, max_rounds: int = 64):
        self.classes = check_classes(classes)
        check_split(radius, min_depth, max_rounds)
        self.radius, self.min_depth, self.max_rounds = int(radius), float(min_depth), int(max_rounds)

    def __repr__(self):
        return f"Instances(classes={self.classes}, radius={self.radius}, min_depth={self.min_depth}, max_rounds={self.max_rounds})"

    def run(self, mask: torch.Tensor, timing: Optional[dict] = None):
        """(labels, ids, info) of a device mask; timing gains instances_seconds and instances (the info, with the instance count)"""
        t0 = time.perf_counter()
        labels, info = split_instances(mask, self.classes, self.radius, self.min_depth, self.max_rounds)
        ids, count = instance_ids(mask, labels, self.classes)
        info = dict(info, instances=count)
        if timing is not None:
            torch.cuda.synchronize()
            timing.update(instances_seconds=time.perf_counter() - t0, instances=info)
        return labels, ids, info


def check_instances(instances) -> Optional[Instances]:
    """the instances= argument (None | Instances | dict of its arguments) -> Instances or None; which outputs take one, and that it needs
    somewhere to go, are predict.check_outputs' rules"""
    if instances is None:
        return None
    if isinstance(instances, dict):
        try:
            instances = Instances(**instances)
        except TypeError as e:
            raise ValueError(f"instances={instances!r}: {e}") from None
    if not isinstance(instances, Instances):
        raise ValueError(f"instances must be None, an Instances or a dict of its arguments, got {type(instances).__name__}")
    return instances
