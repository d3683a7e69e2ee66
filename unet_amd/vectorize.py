"""Polygons of a merged uint8 class mask, traced on the device (csrc/vectorize.hip), and their GeoJSON file.
tests/vectorize_ref.py restates every rule below in plain Python; the device arrays equal it bit for bit.

polygonize(mask) labels the 4-connected components (label_components), traces the rings of every component and returns them as
Polygons: only the corner vertices leave the device.  polygonize_labels(mask, image) traces the segments of a label image instead (the
instances of unet_amd/instances.py): wherever the rules below say component or label_components, read segment and that image.  Connectivity 8 is out of scope: its components pinch at vertices and its holes
would need a point-in-polygon assignment.

Vertices    pixel corners (x, y), 0 <= x <= W, 0 <= y <= H, y down; pixel (y, x) covers [x, x + 1] x [y, y + 1].
Edges       pixel p = y * W + x with label L has a boundary edge on side s (N=0 W=1 S=2 E=3) if the neighbour across that side is
            outside the raster or has another label.  Dense edge id 4 p + s.  Edges are directed with the pixel on the LEFT of the walk as
            seen on screen: N (x+1, y) -> (x, y), W (x, y) -> (x, y+1), S (x, y+1) -> (x+1, y+1), E (x+1, y+1) -> (x+1, y).  Exterior
            rings run counter-clockwise on screen, and for a north-up geotransform counter-clockwise in map coordinates (RFC 7946).
Successor   another boundary edge of the same label, the first that exists of: left (same pixel, side (s + 1) % 4), straight (the next
            pixel along the walk, same side), right (the pixel diagonally ahead on the outer side, side (s - 1) % 4).
Saddles     a saddle vertex is a 2 x 2 block whose diagonal pixels share a label while the other two differ from it.  Rings are the
            cycles of the successor; after a first identification, at every saddle vertex whose two incoming edges of the diagonal pair
            lie in the SAME ring their successors are swapped (in different rings they stay), and the rings are identified again.  Then no
            ring visits a vertex twice, every component has exactly one ring of positive area whose smallest edge id is 4 * label, the
            signed areas of its rings sum to its pixel count, and an even-odd fill of its rings is exactly its pixels.
Rings       a ring's leader is its smallest edge id.  Its vertices are the END vertices of the edges whose successor has another side
            code (corners only), in walk order from the first such edge at or after the leader; the closing point is not repeated.
Area        1/2 sum(x[i+1] y[i] - x[i] y[i+1]) as int64: +1 for one pixel, negative for holes.
Order       rings by ascending leader; polygons by ascending label; within a polygon the exterior ring, then the holes by leader.

Passes: labels, side flags, a scan to compact edge indices, successors, cycle minimum by pointer doubling, saddle swaps, cycle minimum
again, list ranking (with the area terms), ring info, placement in ring order, a scan of the corner marks, vertices.  Doubling runs at
most ceil(log2 E) + 1 rounds, in groups after each of which one word says whether the last round still changed anything.  Host reads per
call: E, R, V, P and those words.  Ring- and polygon-level bookkeeping (a sort and a few scans over R entries) uses torch.

Memory: 10 bytes per pixel (labels 4, flags 1, edge offsets 4, the mask 1) and 42 bytes per edge (six int32 arrays, two int64 arrays of
area terms, two byte arrays), beside 28 bytes per ring and 8 per vertex.  Every buffer that a kernel writes comes from _alloc.

polygonize(mask, simplify=t) simplifies the rings on the device before they leave it (csrc/simplify.hip): a Douglas-Peucker
on the ARCS between the junctions of the borders, in exact integer arithmetic, so that every shared border is simplified once and
identically from both sides and neighbouring polygons keep one common border.  The result is a function of the mask, exclude and t alone;
tests/simplify_ref.py restates the rules below in plain Python and the device arrays equal it bit for bit.  simplify=None launches what
is described above and nothing else.  Crossings between two different simplified arcs and self-intersections at large tolerances
(mapshaper's default behaviour as well), validity repair, Visvalingam simplification, dissolve by class and tolerances in map units are out
of scope.

Nodes       four unit segments meet at a pixel corner; a segment is a border if the two pixels beside it have different labels (those of
            label_components; excluded classes are labelled like any other; outside the raster is one label of its own).  A corner is
            a node if at least 3 of its segments are borders (T-junctions, crossings, saddle vertices) or if it is one of the four raster
            corners.  Nodes are never removed.
Candidates  of a ring: its corner vertices and the nodes it passes -- a ring can run straight through a node (the far side of a
            T-junction), which the plain rings do not list but these do -- in walk order from the leader on.
Arcs        the run of candidates from one node to the next along a ring.  The two rings that share a border see the same arc in opposite
            directions, so every choice below depends on geometry alone; the raster frame is exact (every frame arc is a straight
            segment between nodes).  A ring without a node is one closed arc whose anchor is its candidate with the smallest (y, x); a
            ring with one node has that node as anchor.  A closed arc is split at the candidate farthest from the anchor (squared
            distance in int64, ties to the smallest (y, x)); that vertex is kept without a test and the halves are ordinary arcs.
Douglas-Peucker  on an arc P .. Q: among the interior candidates Z the one with the largest |c|, c = (Q - P) x (Z - P) in int64, ties to
            the smallest (y, x), is kept iff 256 c^2 > q^2 |Q - P|^2, evaluated in 128 bits, where q = floor(16 t + 0.5) is the tolerance
            in sixteenths of a pixel, 0 <= t <= 4096.  This is the distance to the LINE through P and Q, not to the segment.  If Z is
            kept both parts recurse, else the whole interior is dropped.  At t = 0 every candidate is kept.
Afterwards  a ring with fewer than 3 vertices is dropped (both rings of a small island go together and its area falls to its
            surroundings: a one-pixel island disappears from t = 0.75 on); a polygon whose exterior ring is dropped is dropped with its
            holes (a hole that outlives its exterior is an orphan; the reference counts them).
Result      Polygons of the same layout and orders: vertices in walk order from the leader on, rings by leader, polygons by label;
            ring_area is recomputed from the kept vertices (half the shoelace sum, towards zero: integer vertices can enclose a
            half-integer area), poly_pixels stays the true pixel count, edges is unchanged.

Passes: node marks per edge; the candidates placed in ring order by the placement, scan and emit passes above; ring index and node mark
per candidate; per-ring minima / maxima for the anchors and far points; the nearest kept candidate before and after each candidate (lo /
hi, cyclic within the ring) by pointer doubling; then rounds, in groups of 8 after each of which the host reads one word per round: every
live candidate takes |c| against its chord lo .. hi, a 64-bit atomic maximum per segment of (|c| << 32 | ~(y (W + 1) + x)) finds the winner
with its tie-break (a maximum does not depend on the order of arrival), the winner is tested, and its segment splits there or dies.  The
number of rounds is the recursion depth of the deepest arc.  Then the scan of the keep marks, the kept vertices of the surviving rings,
and the areas (exact integer sums).  Extra host reads: one per group of rounds and the new totals; none per ring.
Memory per candidate: 46 bytes (coordinates 8, ring index 4, node and keep marks 2, the four int32 lo / hi arrays of the two doubling sets
16 -- two of them serve later as the winners and the vertex offsets --, the keys 8 and the per-segment maxima 8), beside one more byte per
edge (the candidate marks; their ring-order copy and their scan reuse buffers of the tracer), 36 bytes per ring and 12 per kept vertex."""
from __future__ import annotations

import json
import math
import os
import time
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np
import torch

from . import ops
from .postprocess import _is_int, _to_device

_GROUP = 4                    # doubling rounds per host look at the convergence words
_SIMPLIFY_GROUP = 8           # Douglas-Peucker rounds per host look
MAX_TOLERANCE = 4096          # pixels


def _alloc(shape, dtype, device) -> torch.Tensor:
    """every device buffer that a kernel of this module writes (the tests put guard bands around them here)"""
    return torch.empty(tuple(shape), dtype=dtype, device=device)


@dataclass
class Polygons:
    """rings in ascending leader order, polygons in ascending label order (the module docstring has the rules)"""
    xy: torch.Tensor                   # int32 [V, 2]
    ring_start: torch.Tensor           # int64 [R + 1]
    ring_label: torch.Tensor           # int32 [R]
    ring_area: torch.Tensor            # int64 [R]
    poly_label: torch.Tensor           # int32 [P]
    poly_class: torch.Tensor           # uint8 [P]
    poly_pixels: torch.Tensor          # int64 [P]
    poly_ring_start: torch.Tensor      # int64 [P + 1]
    poly_rings: torch.Tensor           # int64 [R]: ring indices, per polygon the exterior first, then the holes by leader
    edges: int = 0                     # boundary edges traced
    raw_vertices: int = 0              # simplify: the vertices that polygonize gives without it (else 0)
    candidates: int = 0                # simplify: corners and passed nodes = the vertices at tolerance 0 (else 0)
    rounds: int = 0                    # simplify: Douglas-Peucker rounds = the recursion depth of the deepest arc (else 0)

    def cpu(self) -> "Polygons":
        return Polygons(**{f.name: (v.cpu() if isinstance(v, torch.Tensor) else v) for f in fields(self) for v in (getattr(self, f.name),)})

    @property
    def n_polygons(self) -> int:
        return int(self.poly_label.shape[0])

    @property
    def n_rings(self) -> int:
        return int(self.ring_label.shape[0])

    @property
    def n_vertices(self) -> int:
        return int(self.xy.shape[0])


def check_exclude(exclude) -> tuple:
    """None | int | iterable of class ids 0..255 -> a sorted tuple"""
    if exclude is None:
        return ()
    if _is_int(exclude):
        exclude = (exclude,)
    try:
        ids = [c for c in exclude]
    except TypeError:
        raise ValueError(f"exclude must be None, an int or an iterable of class ids 0..255, got {exclude!r}") from None
    for c in ids:
        if not _is_int(c) or not 0 <= c <= 255:
            raise ValueError(f"exclude: class ids must be ints in 0..255, got {c!r}")
    return tuple(sorted({int(c) for c in ids}))


def _empty(dev) -> Polygons:
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)          # noqa: E731
    return Polygons(z((0, 2), torch.int32), z((1,), torch.int64), z((0,), torch.int32), z((0,), torch.int64), z((0,), torch.int32),
                    z((0,), torch.uint8), z((0,), torch.int64), z((1,), torch.int64), z((0,), torch.int64), 0)


def _scan_total(src: torch.Tensor, out: torch.Tensor, blocks: torch.Tensor) -> int:
    ops.vec_scan(src, out, blocks)
    return ops.vec_read(blocks, ops.vec_scan_words(src.numel()) - 1, 1)[0]          # a host read


def _max_rounds(E: int) -> int:
    return (E - 1).bit_length() + 1          # ceil(log2 E) + 1


def _settled(changed: torch.Tensor, g: int) -> bool:
    """did the last of the g rounds change nothing?  (one host read; the words are int32 pairs)"""
    words = ops.vec_read(changed, 0, (g + 1) // 2)
    return not (words[(g - 1) // 2] >> (32 * ((g - 1) % 2))) & 0xFFFFFFFF


def _doubling(E: int, run, a, b, changed: torch.Tensor):
    """groups of doubling rounds a -> b -> a ... until one changes nothing or ceil(log2 E) + 1 are done; returns (newest set, other)"""
    left = _max_rounds(E)
    while left > 0:
        g = min(_GROUP, left)
        run(a, b, g)
        left -= g
        if g % 2:
            a, b = b, a
        if _settled(changed, g):
            break
    return a, b


class _Stages:
    """milliseconds per stage for scripts/vectorize_bench.py: a device synchronise at every mark, so only when a dict is passed in"""

    def __init__(self, out: Optional[dict]):
        self.out = out
        if out is not None:
            torch.cuda.synchronize()
            self.t = time.perf_counter()

    def mark(self, name: str):
        if self.out is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            self.out[name] = self.out.get(name, 0.0) + (now - self.t) * 1e3
            self.t = now


def check_simplify(simplify) -> Optional[int]:
    """None | a tolerance in pixels, 0..4096 -> None | q = floor(16 tolerance + 0.5), the tolerance in sixteenths of a pixel"""
    if simplify is None:
        return None
    if isinstance(simplify, bool) or not isinstance(simplify, (int, float, np.integer, np.floating)) or not math.isfinite(simplify):
        raise ValueError(f"simplify must be None or a finite number of pixels, got {simplify!r}")
    if not 0 <= simplify <= MAX_TOLERANCE:
        raise ValueError(f"simplify must lie in 0..{MAX_TOLERANCE} pixels, got {simplify!r}")
    return int(math.floor(16.0 * float(simplify) + 0.5))


def _flags_of(changed: torch.Tensor, g: int) -> list:
    """the changed words of g rounds (one host read; int32 pairs in int64 words)"""
    words = ops.vec_read(changed, 0, (g + 1) // 2)
    return [(words[r // 2] >> (32 * (r % 2))) & 0xFFFFFFFF for r in range(g)]


def _simplify(st: _Stages, q: int, m, labels, flags, offs, corner, ring, steps, ridx, ring_base, ring_len, ring_label, ring_area, pos, free,
              mark, blocks, changed, E: int, R: int) -> Polygons:
    """the passes of DESIGN 3.19 on the traced rings; `free` (int32 [E]) and `mark` (uint8 [E]) are buffers the tracer no longer needs"""
    dev = m.device
    H, W = m.shape
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    ch32 = changed.view(i32)
    tail = lambda v: torch.tensor([v], dtype=i64, device=dev)          # noqa: E731
    cand = _alloc((E,), u8, dev)
    ops.simp_marks(labels, flags, offs, corner, E, cand)
    st.mark("simp_marks")
    cand_ord, coff = mark, free
    ops.vec_place(ring, steps, ridx, ring_base, ring_len, cand, E, R, pos, cand_ord)
    C = _scan_total(cand_ord, coff, blocks)
    cxy, cring, cnode = _alloc((C, 2), i32, dev), _alloc((C,), i32, dev), _alloc((C,), u8, dev)
    ops.vec_emit(flags, offs, cand, pos, coff, E, C, cxy)
    ops.simp_gather(ring, ridx, pos, coff, cand, E, R, C, cring, cnode)
    cs = coff[ring_base]
    cn = torch.cat([cs[1:], tail(C).to(i32)]) - cs
    st.mark("simp_candidates")
    keep = _alloc((C,), u8, dev)
    near = [_alloc((C,), i32, dev) for _ in range(4)]
    ops.simp_closed(cxy, cring, cnode, cs, cn, C, R, W, _alloc((R,), i32, dev), _alloc((3, R), i64, dev), keep, near[0], near[1])
    st.mark("simp_closed")
    (lo, hi), (win, koff) = _doubling(C, lambda a, b, g: ops.simp_near_rounds(C, a, b, g, ch32), (near[0], near[1]), (near[2], near[3]), changed)
    st.mark("simp_near")
    key, slot = _alloc((C,), i64, dev), _alloc((C,), i64, dev)
    rounds, first = 0, True
    while rounds <= C:          # an arc of n candidates is settled after at most n rounds
        ops.simp_dp_rounds(cxy, cring, cn, C, R, W, q, first, _SIMPLIFY_GROUP, keep, lo, hi, key, slot, win, ch32)
        first = False
        live = sum(1 for f in _flags_of(changed, _SIMPLIFY_GROUP) if f)
        rounds += live
        if live < _SIMPLIFY_GROUP:
            break
    st.mark("simp_rounds")
    K = _scan_total(keep, koff, blocks)
    kstart = koff[cs.to(i64)]
    kcount = torch.cat([kstart[1:], tail(K).to(i32)]) - kstart

    # ring and polygon level, in torch as in _polygonize: rings with fewer than 3 vertices go, and polygons whose exterior ring goes
    order = torch.argsort(ring_label.to(i64) * R + torch.arange(R, dtype=i64, device=dev))
    by_label = ring_label[order]
    first_of = torch.ones(R, dtype=torch.bool, device=dev)
    first_of[1:] = by_label[1:] != by_label[:-1]
    starts = torch.nonzero(first_of).flatten()
    poly = torch.cumsum(first_of.to(i64), 0) - 1
    exterior = (kcount >= 3)[order[starts]]                              # the exterior ring of a polygon is its first ring by leader
    stays = (kcount >= 3)[order] & exterior[poly]                        # in (label, leader) order
    final = torch.zeros(R, dtype=torch.bool, device=dev)
    final[order] = stays
    newring = torch.where(final, torch.cumsum(final.to(i64), 0) - 1, torch.full((R,), -1, dtype=i64, device=dev)).to(i32)
    count = torch.where(final, kcount, torch.zeros_like(kcount)).to(i64)
    vbase = torch.cumsum(count, 0) - count
    V, R2, raw = ops.vec_read(torch.stack([count.sum(), final.sum(), corner.sum(dtype=i64)]), 0, 3)          # a host read: the new totals
    if V == 0:
        out = _empty(dev)
        out.edges, out.raw_vertices, out.candidates, out.rounds = E, raw, C, rounds
        return out
    xy, vring = _alloc((V, 2), i32, dev), _alloc((V,), i32, dev)
    ops.simp_emit(cxy, cring, keep, koff, kstart, vbase, newring, C, R, V, xy, vring)
    ring_start = torch.cat([vbase[final], tail(V)])
    area2 = _alloc((R2,), i64, dev)
    ops.simp_area(xy, vring, ring_start, V, R2, area2)
    st.mark("simp_emit")
    poly_ring_start = torch.cat([starts, tail(R)])
    run = torch.cat([tail(0), torch.cumsum(ring_area[order], 0)])
    pixels = run[poly_ring_start[1:]] - run[poly_ring_start[:-1]]          # the true pixel counts: the areas of the traced rings
    run = torch.cat([tail(0), torch.cumsum(stays.to(i64), 0)])
    rings_of = (run[poly_ring_start[1:]] - run[poly_ring_start[:-1]])[exterior]
    poly_label = by_label[starts][exterior]
    st.mark("simp_polygons")
    return Polygons(xy, ring_start, ring_label[final], torch.div(area2, 2, rounding_mode="trunc"), poly_label, m.view(-1)[poly_label.to(i64)],
                    pixels[exterior], torch.cat([tail(0), torch.cumsum(rings_of, 0)]), newring[order[stays]].to(i64), E, raw, C, rounds)


def _polygonize(m: torch.Tensor, exclude: tuple, stages: Optional[dict] = None, q: Optional[int] = None,
                given: Optional[torch.Tensor] = None) -> Polygons:
    st = _Stages(stages)
    dev = m.device
    H, W = m.shape
    n = H * W
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    if given is None:
        labels, counters = _alloc((H, W), i32, dev), _alloc((4,), i32, dev)
        ops.cc_label(m, 4, labels, counters)
        ops.postprocess_counters(counters)
    else:
        labels, bad = given, _alloc((1,), i64, dev)
        ops.inst_check_labels(m, labels, bad)
        if ops.vec_read(bad, 0, 1)[0]:          # a host read
            raise ValueError("polygonize_labels: labels must name, for every pixel, a pixel of the same class at or before it that names itself "
                             "(the smallest linear index of its segment)")
    st.mark("label")
    flags, offs = _alloc((H, W), u8, dev), _alloc((H, W), i32, dev)
    ops.vec_flags(m, labels, exclude, flags)
    E = _scan_total(flags, offs, _alloc((ops.vec_scan_words(n),), i64, dev))
    st.mark("flags_scan")
    if E > ops.VEC_MAX_COUNT:
        raise ValueError(f"polygonize: {E} boundary edges exceed 2^31 - 1 (edge indices are int32)")
    if E == 0:
        return _empty(dev)
    succ, corner = _alloc((E,), i32, dev), _alloc((E,), u8, dev)
    ops.vec_succ(flags, offs, E, succ, corner)
    st.mark("succ")
    w = [_alloc((E,), i32, dev) for _ in range(5)]
    changed = _alloc((32,), i64, dev)
    ch32 = changed.view(i32)

    def identify():
        first = [True]

        def run(a, b, g):
            ops.vec_min_rounds(succ, E, a, b, first[0], g, ch32)
            first[0] = False
        return _doubling(E, run, (w[0], w[1]), (w[2], w[3]), changed)

    (ring, _), _ = identify()
    st.mark("rings_first")
    ops.vec_swap(labels, flags, offs, ring, succ, E)
    st.mark("swap")
    (ring, free0), (free1, free2) = identify()
    st.mark("rings_second")

    mark = _alloc((E,), u8, dev)
    area_a, area_b = _alloc((E,), i64, dev), _alloc((E,), i64, dev)
    ops.vec_rank_init(flags, offs, succ, ring, E, free0, free1, area_a, mark)
    (steps, free0, area), (free1, free2, _) = _doubling(E, lambda a, b, g: ops.vec_rank_rounds(E, a, b, g, ch32), (free0, free1, area_a),
                                                        (free2, w[4], area_b), changed)
    st.mark("rank")
    blocks = _alloc((ops.vec_scan_words(E),), i64, dev)
    ridx = free1
    R = _scan_total(mark, ridx, blocks)
    ring_label, ring_len, ring_area = _alloc((R,), i32, dev), _alloc((R,), i64, dev), _alloc((R,), i64, dev)
    ops.vec_ring_info(flags, offs, labels, succ, ring, ridx, steps, area, E, R, ring_label, ring_len, ring_area)
    ring_base = torch.cumsum(ring_len, 0) - ring_len
    if q is not None:
        st.mark("ring_info")
        return _simplify(st, q, m, labels, flags, offs, corner, ring, steps, ridx, ring_base, ring_len, ring_label, ring_area, free2, free0, mark,
                         blocks, changed, E, R)
    pos, corner_ord = free2, mark
    ops.vec_place(ring, steps, ridx, ring_base, ring_len, corner, E, R, pos, corner_ord)
    voff = free0
    V = _scan_total(corner_ord, voff, blocks)
    xy = _alloc((V, 2), i32, dev)
    ops.vec_emit(flags, offs, corner, pos, voff, E, V, xy)
    st.mark("place_emit")
    ring_start = torch.cat([voff[ring_base].to(i64), torch.tensor([V], dtype=i64, device=dev)])

    # polygon level: a sort of R keys (label, leader) -- rings are in leader order, so their index stands for the leader
    order = torch.argsort(ring_label.to(i64) * R + torch.arange(R, dtype=i64, device=dev))
    by_label = ring_label[order]
    first = torch.ones(R, dtype=torch.bool, device=dev)
    first[1:] = by_label[1:] != by_label[:-1]
    starts = torch.nonzero(first).flatten()
    poly_label = by_label[starts]
    poly_ring_start = torch.cat([starts, torch.tensor([R], dtype=i64, device=dev)])
    run = torch.cat([torch.zeros(1, dtype=i64, device=dev), torch.cumsum(ring_area[order], 0)])
    st.mark("polygons")
    return Polygons(xy, ring_start, ring_label, ring_area, poly_label, m.view(-1)[poly_label.to(i64)], run[poly_ring_start[1:]] - run[poly_ring_start[:-1]],
                    poly_ring_start, order, E)


def check_labels(labels, m: torch.Tensor) -> torch.Tensor:
    """the labels argument of polygonize_labels: a contiguous int32 device tensor of the mask's shape on the mask's device"""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or not labels.is_cuda:
        raise ValueError(f"labels must be an int32 [H, W] device tensor, got {getattr(labels, 'dtype', type(labels).__name__)} on "
                         f"{getattr(labels, 'device', 'the host')}")
    if tuple(labels.shape) != tuple(m.shape) or labels.device != m.device:
        raise ValueError(f"labels has shape {tuple(labels.shape)} on {labels.device}, the mask {tuple(m.shape)} on {m.device}")
    return labels.contiguous()


def polygonize(mask, exclude=None, simplify=None, stages: Optional[dict] = None) -> Polygons:
    """Polygons (device tensors) of the 4-connected components of a contiguous uint8 [H, W] class mask (device tensor, host tensor or NumPy
    array; host input is uploaded).  exclude: None, an int or an iterable of class ids 0..255 whose components get no polygon.
    Connectivity 8 is not offered: its components pinch at vertices and holes would need a point-in-polygon assignment.
    simplify: None, or the tolerance in pixels (0..4096) of the arc-based Douglas-Peucker simplification of the module docstring; None
    launches what it launched before the simplification existed.
    stages: a dict that receives the milliseconds of every stage (this synchronises the device after each: for measurements only); with
    simplify the stages after the ring info are ring_info and simp_*."""
    exclude = check_exclude(exclude)
    q = check_simplify(simplify)
    m, _ = _to_device(mask, torch.uint8, "polygonize")
    return _polygonize(m, exclude, stages, q)


def polygonize_labels(mask, labels, exclude=None, simplify=None, stages: Optional[dict] = None) -> Polygons:
    """polygonize with the given label image in the place of the component labels, so that the polygons are those of its segments.  labels: an
    int32 [H, W] device tensor of the mask's shape; every segment must be 4-connected and of one class, and its label the smallest linear
    index of its pixels (split_instances of unet_amd/instances.py gives such an image).  The last two are checked (ValueError), the
    connectivity is the caller's word.  Every rule of the module docstring is stated on labels, so instances of one class that touch keep
    one common, identically simplified border.  polygonize itself keeps its arguments and launches what it launched before this existed."""
    exclude = check_exclude(exclude)
    q = check_simplify(simplify)
    m, _ = _to_device(mask, torch.uint8, "polygonize_labels")
    return _polygonize(m, exclude, stages, q, check_labels(labels, m))


# ------------------------------------------------------------------------------------------------------------------ GeoJSON (host)

_ARRAYS = ("xy", "ring_start", "poly_label", "poly_class", "poly_pixels", "poly_ring_start", "poly_rings")


def _host_arrays(polys) -> dict:
    """Polygons (device or host) or a mapping of arrays -> NumPy arrays"""
    out = {}
    for k in _ARRAYS:
        v = polys[k] if isinstance(polys, dict) else getattr(polys, k)
        out[k] = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    return out


def epsg_of_tags(tags) -> Optional[int]:
    """the EPSG code in the GeoKeyDirectory (tag 34735) of read_tiff's meta["tags"]: key 3072 (projected), else 2048 (geographic); 32767
    (user-defined) and values stored in another tag count as unknown"""
    if not tags or 34735 not in tags:
        return None
    d = [int(v) for v in tags[34735]]
    keys = {}
    for i in range(d[3] if len(d) >= 4 else 0):
        entry = d[4 + 4 * i:8 + 4 * i]
        if len(entry) == 4 and entry[1] == 0 and entry[2] == 1:          # the value sits in the entry itself
            keys[entry[0]] = entry[3]
    for k in (3072, 2048):
        if k in keys and keys[k] not in (0, 32767):
            return keys[k]
    return None


def check_geojson_args(geotransform=None, epsg=None):
    if geotransform is not None:
        gt = tuple(float(v) for v in geotransform)
        if len(gt) != 6 or gt[1] == 0 or gt[5] == 0:
            raise ValueError(f"geotransform must be six numbers with non-zero pixel sizes, got {geotransform!r}")
        if gt[2] != 0 or gt[4] != 0:
            raise ValueError("geotransform with rotation terms is not supported")
    if epsg is not None and (not _is_int(epsg) or epsg <= 0):
        raise ValueError(f"epsg must be None or a positive int, got {epsg!r}")


ATTRIBUTE_KEYS = ("perimeter", "centroid_x", "centroid_y", "diameter", "compactness", "on_edge", "point_x", "point_y")
# the other keys of a row of object_rows(values=None): a feature has them already, or (bbox) the geometry says it
_OWN_ROW_KEYS = frozenset(ATTRIBUTE_KEYS + ("class", "name", "pixels", "area", "bbox", "instance"))


def write_geojson(path, polys, geotransform=None, epsg: Optional[int] = None, codes=None, class_zero: bool = False, instance=None,
                  attributes=None) -> int:
    """One FeatureCollection with one Polygon feature per component, in poly_label order: the exterior ring, then the holes, each closed by
    repeating its first point.  Coordinates are X = gt[0] + x gt[1], Y = gt[3] + y gt[5] in float64, written with repr; integer pixel
    coordinates without a geotransform.  Properties: class (the id as the raster on disk holds it: class - 1 under class_zero, where
    class 0 -- NO_Data -- gets no feature), name (codes[class], if codes are given), pixels, area (pixels |gt[1] gt[5]|).  With an EPSG code
    the legacy "crs" member names urn:ogc:def:crs:EPSG::<code>.  instance: None, or one id per polygon, written as the property `instance`
    behind the others.  attributes: None, or a mapping from a polygon's label to its row of unet_amd/objects.object_rows; a feature whose label
    has a row gains the ATTRIBUTE_KEYS of that row behind its other properties (joined by label: with a simplification some polygons get
    no feature), and behind them whatever the row holds beyond the keys of object_rows itself: the <name>_* columns of
    object_rows(values=).  Returns the number of features.  Host code."""
    check_geojson_args(geotransform, epsg)
    a = _host_arrays(polys)
    labels = a["poly_label"].tolist() if attributes is not None else None
    gt = None if geotransform is None else tuple(float(v) for v in geotransform)
    xy = a["xy"].astype(np.int64)
    if gt is None:
        pts = [f"[{x},{y}]" for x, y in xy.tolist()]
    else:
        X, Y = gt[0] + xy[:, 0].astype(np.float64) * gt[1], gt[3] + xy[:, 1].astype(np.float64) * gt[5]
        pts = [f"[{x!r},{y!r}]" for x, y in zip(X.tolist(), Y.tolist())]
    if codes is not None and a["poly_class"].size and int(a["poly_class"].max()) >= len(codes):
        raise ValueError(f"codes names {len(codes)} classes, the polygons hold class {int(a['poly_class'].max())}")
    rs, prs, rings = a["ring_start"].tolist(), a["poly_ring_start"].tolist(), a["poly_rings"].tolist()
    px_area = 1.0 if gt is None else abs(gt[1] * gt[5])
    inst = None if instance is None else (instance.cpu().numpy() if isinstance(instance, torch.Tensor) else np.asarray(instance)).tolist()
    if inst is not None and len(inst) != len(a["poly_class"]):
        raise ValueError(f"instance holds {len(inst)} ids for {len(a['poly_class'])} polygons")
    feats = []
    for i, (cls, pixels) in enumerate(zip(a["poly_class"].tolist(), a["poly_pixels"].tolist())):
        if class_zero and cls == 0:
            continue
        props = {"class": cls - 1 if class_zero else cls}
        if codes is not None:
            props["name"] = str(codes[cls])
        props["pixels"] = pixels
        props["area"] = pixels * px_area
        if inst is not None:
            props["instance"] = int(inst[i])
        row = attributes.get(labels[i]) if attributes is not None else None
        if row is not None:
            props.update((k, row[k]) for k in ATTRIBUTE_KEYS)
            props.update((k, v) for k, v in row.items() if k not in _OWN_ROW_KEYS)
        coords = ",".join("[" + ",".join(pts[rs[r]:rs[r + 1]] + pts[rs[r]:rs[r] + 1]) + "]" for r in rings[prs[i]:prs[i + 1]])
        feats.append('{"type":"Feature","properties":' + json.dumps(props) + ',"geometry":{"type":"Polygon","coordinates":[' + coords + "]}}")
    head = '{"type":"FeatureCollection",'
    if epsg is not None:
        head += '"crs":{"type":"name","properties":{"name":"urn:ogc:def:crs:EPSG::%d"}},' % int(epsg)
    with open(os.fspath(path), "w") as f:
        f.write(head + '"features":[\n' + ",\n".join(feats) + "\n]}\n")
    return len(feats)


# ------------------------------------------------------------------------------------------------------------------ entry points

def check_vector(vector, vector_exclude=None, class_zero: bool = False, simplify=None) -> Optional[tuple]:
    """the vector_path= / vector= and vector_exclude= arguments of predict_raster / save_predictions -> the classes to exclude (a tuple), or
    None when no vector file is wanted.  simplify (vector_simplify=): None or a finite tolerance of 0..4096 pixels, only with a vector output.
    Which outputs can be polygonized is predict.check_outputs' rule"""
    if vector is None or vector is False:
        if vector_exclude is not None:
            raise ValueError("vector_exclude without a vector output")
        if simplify is not None:
            raise ValueError("vector_simplify without a vector output")
        return None
    check_simplify(simplify)
    exclude = check_exclude(vector_exclude)
    return tuple(sorted(set(exclude) | {0})) if class_zero else exclude


def vectorize_mask(mask, path, exclude=(), geotransform=None, epsg=None, codes=None, class_zero: bool = False, timing: Optional[dict] = None,
                   simplify=None, labels=None, ids=None, attributes=None) -> Polygons:
    """polygonize + write_geojson of an assembled class mask (device or host); timing gains vector_seconds / _polygons / _vertices and
    vector_vertices_raw (the vertices before the simplification; equal to vector_vertices without one).  labels / ids (device tensors of
    unet_amd/instances.py: the instance labels and their dense ids per pixel): one feature per instance, with the id of its pixels as the
    property `instance` (0 for the components of a class that is not split).  attributes: as in write_geojson"""
    t0 = time.perf_counter()
    if labels is None:
        polys = polygonize(mask, exclude, simplify)
        n = write_geojson(path, polys, geotransform, epsg, codes, class_zero, attributes=attributes)
    else:
        polys = polygonize_labels(mask, labels, exclude, simplify)
        n = write_geojson(path, polys, geotransform, epsg, codes, class_zero, instance=ids.view(-1)[polys.poly_label.to(torch.int64)],
                          attributes=attributes)
    if timing is not None:
        timing.update(vector_seconds=time.perf_counter() - t0, vector_polygons=n, vector_vertices=polys.n_vertices,
                      vector_vertices_raw=polys.n_vertices if simplify is None else polys.raw_vertices)
    return polys
