"""Overlap merge of per-window predictions into one mosaic, partitioned by ROWS over the ranks.

Reference (single process, host): ``predict.py:257-334`` -- a ``[C, H, W]`` float mosaic of summed softmax probabilities plus a hit
counter, every tile added at ``round((ulx - ulx_full) / xres)``, divided where the counter is positive, argmax over the classes.  The
windows themselves follow ``slidingwindow.generate`` as ``create_tiles_unet.py:30-56`` calls it.

Here the merge order is fixed -- placements sorted by (row, column) -- so that every mosaic pixel receives its contributions in one
defined order whatever the number of ranks:

* the ordered placement list is cut into ``world`` contiguous ranges of equal length (tiles are the unit of work);
* rank r OWNS the mosaic rows from the end of rank r-1's coverage to the end of its own coverage, and keeps only that strip in HBM;
* a placement of rank r that starts above its strip (it overlaps rows owned by rank r-1) contributes those rows as a *slab* of per-window
  probabilities that is sent to rank r-1, which adds the slabs in order AFTER its own windows -- exactly the order a single process uses,
  so the N-rank result equals the 1-rank result bit for bit, and the only exchange is the overlap rows (cfg5: <= 300 MB per boundary
  instead of an 8 GB all-reduce of whole mosaics);
* every rank finalises its strip (divide, argmax) and only the requested band(s) travel to rank 0.

Gaussian blending (``blend="gaussian"``, beyond the reference): window k adds fl(w * p) for every value p it would add, with the
centre-peaked weight w = fl(g_h[Y - y0] * g_w[X - x0]) of ``blend_profile``, and w goes into a per-pixel weight sum that takes the
place of the hit counter as divisor.  The receiver of a slab applies the weights (rows [0, rows) of the sender window's vertical profile),
so the slabs and the ordering argument above stay as they are: N ranks still equal 1 rank bit for bit.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np


BLENDS = ("mean", "gaussian")


def blend_profile(n: int) -> np.ndarray:
    """float32 [n]: the 1-D Gaussian importance profile of a window side of n pixels, g[t] = exp(-(t - (n-1)/2)^2 / (2 sigma^2)) with
    sigma = n / 8 (nnU-Net's sliding-window predictor, MONAI's sigma_scale = 0.125), computed in float64, divided by its maximum, rounded
    to float32.  Its smallest entry is exp(-8 (n-1)^2 / n^2) >= ~3.4e-4: no weight is zero."""
    n = int(n)
    if n < 1:
        raise ValueError(f"blend profile of {n} pixels")
    t = np.arange(n, dtype=np.float64)
    sigma = n / 8.0
    g = np.exp(-((t - (n - 1) / 2.0) ** 2) / (2.0 * sigma * sigma))
    return (g / g.max()).astype(np.float32)


def check_blend(blend: str, large_file: bool = False, merge: bool = True) -> str:
    """the blend= argument of predict_raster / save_predictions, validated before anything is uploaded"""
    if blend not in BLENDS:
        raise ValueError(f"blend={blend!r}: expected one of {BLENDS}")
    if blend != "mean" and large_file:
        raise ValueError(f"blend={blend!r} with large_file=True: the int8 merge divides integers, it has no weighted form")
    if blend != "mean" and not merge:
        raise ValueError(f"blend={blend!r} needs merge=True: per-tile predictions have no overlap to blend")
    return blend


def window_offsets(length: int, size: int, step: int) -> List[int]:
    """slidingwindow 0.0.14 as create_tiles_unet.py:52-54 calls it: 0, step, ... while the window fits, plus one window flush with the
    far edge when the raster is not covered (20000 px, 512 px windows, overlap 0.2 -> 0, 410, ..., 19270, 19488: 49 per axis)"""
    offs = list(range(0, length - size + 1, step))
    if offs[-1] + size < length:
        offs.append(length - size)
    return offs


def sliding_windows(height: int, width: int, size: int, overlap: float) -> np.ndarray:
    """int64 [n, 2] = (y0, x0) of every window, row-major (the index order of the reference's tile files)"""
    if overlap > 1:
        raise ValueError(f"Patch overlap {overlap} must be between 0 - 1")
    if height < size or width < size:
        raise ValueError(f"Patch size of {size} is larger than the image dimensions {[height, width]}")
    step = size - int(size * overlap)
    ys, xs = window_offsets(height, size, step), window_offsets(width, size, step)
    return np.array([(y, x) for y in ys for x in xs], dtype=np.int64).reshape(-1, 2)


def keep_windows(nonzero: np.ndarray, bands: int, size_h: int, size_w: int, max_empty: float) -> np.ndarray:
    """create_tiles_unet.py:379: a window is dropped when np.sum(crop != 0) < np.prod(crop.shape) * (1 - max_empty)"""
    return ~(np.asarray(nonzero, dtype=np.int64) < np.prod((size_h, size_w, bands)) * (1 - max_empty))


def merge_order(places: np.ndarray) -> np.ndarray:
    """permutation that sorts placements [n, >=2] = (y0, x0, ...) by row, then column (stable)"""
    p = np.asarray(places)
    return np.lexsort((p[:, 1], p[:, 0]))


class MergePlan:
    """places: int [n, 4] = (y0, x0, h, w) in mosaic pixel coordinates, already in merge order (sorted by y0, then x0)."""

    def __init__(self, places: np.ndarray, MH: int, MW: int, world: int = 1):
        p = np.asarray(places, dtype=np.int64).reshape(-1, 4)
        if len(p) and (np.diff(p[:, 0]) < 0).any():
            raise ValueError("placements must be sorted by row (merge_order)")
        self.places, self.MH, self.MW, self.world = p, int(MH), int(MW), int(world)
        n = len(p)
        end = p[:, 0] + p[:, 2]
        for active in range(max(1, min(world, n)), 0, -1):
            cuts = [n * r // active for r in range(active + 1)]
            own_lo, own_hi = [0] * active, [0] * active
            for r in range(active):
                own_lo[r] = 0 if r == 0 else own_hi[r - 1]
                own_hi[r] = self.MH if r == active - 1 else max(own_lo[r], int(end[cuts[r]:cuts[r + 1]].max()))
            # a rank's windows may reach into the strip of the rank before it, never further up
            if all(int(p[cuts[r], 0]) >= own_lo[r - 1] for r in range(1, active)):
                break
        self.active = active
        self.ranges: List[Tuple[int, int]] = [(cuts[r], cuts[r + 1]) for r in range(active)] + [(n, n)] * (world - active)
        self.own: List[Tuple[int, int]] = [(own_lo[r], own_hi[r]) for r in range(active)] + [(self.MH, self.MH)] * (world - active)

    def slabs(self, rank: int) -> List[Tuple[int, int]]:
        """[(placement index, rows)] of rank's placements that start above its strip: their first `rows` rows belong to rank - 1"""
        if rank == 0 or rank >= self.active:
            return []
        a, b = self.ranges[rank]
        lo = self.own[rank][0]
        out = []
        for i in range(a, b):
            y0, _, h, _ = self.places[i]
            if y0 >= lo:
                break           # sorted by y0: nothing further starts above the strip
            out.append((i, int(min(y0 + h, lo) - y0)))
        return out

    def slab_floats(self, rank: int, C: int) -> int:
        return int(sum(C * rows * int(self.places[i, 3]) for i, rows in self.slabs(rank)))

    def batches(self, rank: int, batch: int) -> List[Tuple[int, int]]:
        """(first, n) runs of at most `batch` consecutive placements of one size inside the rank's range"""
        a, b = self.ranges[rank]
        out, i = [], a
        while i < b:
            n = 1
            while n < batch and i + n < b and tuple(self.places[i + n, 2:]) == tuple(self.places[i, 2:]):
                n += 1
            out.append((i, n))
            i += n
        return out
