"""Vector labels burnt into a uint8 class mask on the device (csrc/rasterize.hip), and the reader of the GeoJSON dialect that
unet_amd.vectorize.write_geojson writes.  tests/rasterize_ref.py restates every rule below in plain Python; the device mask equals it bit for
bit, and rasterize(polygonize(mask), mask.shape) is the mask.  Everything is exact integer arithmetic; the result is a function of the inputs
alone.

Coordinates  the pixel conventions of unet_amd/vectorize.py: x right, y down, pixel (y, x) covers [x, x + 1] x [y, y + 1].  A vertex is int32
            fixed point with 8 fractional bits, X = floor(256 x + 0.5); |x|, |y| <= 2^21 pixels is checked (ValueError), so that every product
            below stays under 2^60.  Map coordinates become pixel coordinates on the host in float64, x = (X_map - gt[0]) / gt[1],
            y = (Y_map - gt[3]) / gt[5], then that quantisation; geotransforms with rotation terms are refused (check_geojson_args).
Features    a feature is an ordered set of rings with one burn value 0..255; exterior and holes are not distinguished: the fill is even-odd
            over ALL rings of the feature, so a MultiPolygon is one feature that holds the rings of all its parts.  A ring is closed
            implicitly (a repeated closing point is dropped on reading); rings with fewer than 3 vertices are ignored.
Coverage    the pixel centre decides (the default rule of GDAL).  Row y has the centre ordinate Yc = 256 y + 128.  An edge
            (X0, Y0) -> (X1, Y1) crosses row y iff min(Y0, Y1) <= Yc < max(Y0, Y1): half-open, so horizontal edges never cross, and every
            closed ring crosses a row an even number of times.  Its crossing abscissa is the exact rational
            X* = X0 + (Yc - Y0)(X1 - X0) / (Y1 - Y0); it toggles every pixel of the row whose centre lies at or right of it, the columns
            >= k = ceil((X* - 128) / 256), by an int64 floor division on a sign-normalised denominator, clamped to [0, W]; rows are clipped
            to [0, H - 1].  A pixel is inside the feature iff the number of its row's crossings with k <= x is odd.  A centre exactly on a
            left or top border is inside, one exactly on a right or bottom border outside, so two features that share a border partition
            the pixels along it: no pixel belongs to both or to neither.
Order       where features overlap the one with the highest index wins (the painter's order of gdal_rasterize).  Pixels that no feature
            covers keep `fill`, or what `out` held.
Limits      H, W < 2^20; fewer than 2^23 features; fewer than 2^31 crossings (all ValueError).

Passes: (count) one thread per edge -- vertex i to the next vertex of its ring -- counts the row centres it crosses after clipping; (scan) an
exclusive int64 scan of the counts, whose total M is the one host read of that stage, together with the word that says whether a coordinate
was out of range; (emit) one thread per edge writes its crossings as int64 keys feature << 40 | row << 20 | k; (sort) one torch.sort of the M
keys -- equal keys are identical, so stability does not matter; (spans) sorted keys 2j and 2j + 1 belong to one (feature, row) and bound the
span [k_2j, k_2j+1): one wavefront per pair, lanes striding the columns, takes the atomic maximum of the uint32 word (feature + 1) << 8 | value
into an [H, W] priority plane zeroed beforehand (a maximum does not depend on the order of arrival) and counts the pairs whose keys differ
above bit 20 in one word, which the host reads once (RuntimeError if it is not 0); (resolve) out = word ? word & 255 : (out or fill), in
16-byte accesses.  Ring bookkeeping (the ring of every vertex, the feature of every ring: two searches over the CSR arrays) uses torch.

Memory: 4 bytes per pixel for the plane and 1 for the mask; 8 bytes per crossing for the keys, 8 more for their sorted copy and 8 for the
permutation that torch.sort returns beside it, plus that sort's own workspace; per vertex 8 (coordinates), 4 (its ring), 4 (its count) and 8
(its offset).  Every buffer that a kernel writes comes from _alloc.

Out of scope: ALL_TOUCHED, lines and points, non-zero winding, float burn values and regression masks, Shapefile and GeoPackage,
reprojection, and a host fallback (without a device rasterize raises)."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops
from .postprocess import _is_int
from .vectorize import Polygons, _Stages, check_geojson_args

FRACTION_BITS = 8
ONE = 1 << FRACTION_BITS                  # fixed-point units per pixel
MAX_PIXELS_COORD = 2 ** 21                # |x|, |y| in pixels


def _alloc(shape, dtype, device) -> torch.Tensor:
    """every device buffer that a kernel of this module writes (the tests put guard bands around them here)"""
    return torch.empty(tuple(shape), dtype=dtype, device=device)


@dataclass
class Rings:
    """the rings of F features: vertices in 1/256 pixel, the rings of a feature contiguous (the module docstring has the rules)"""
    xy: torch.Tensor                      # int32 [V, 2], fixed point with 8 fractional bits
    ring_start: torch.Tensor              # int64 [R + 1]
    feature_ring_start: torch.Tensor      # int64 [F + 1]
    values: torch.Tensor                  # uint8 [F]

    def to(self, device) -> "Rings":
        return Rings(self.xy.to(device), self.ring_start.to(device), self.feature_ring_start.to(device), self.values.to(device))

    @property
    def n_vertices(self) -> int:
        return int(self.xy.shape[0])

    @property
    def n_rings(self) -> int:
        return int(self.ring_start.shape[0]) - 1

    @property
    def n_features(self) -> int:
        return int(self.values.shape[0])


def check_rings(rings: Rings) -> Rings:
    """types, shapes and the feature limit of a Rings; for host tensors also the CSR arrays and the coordinate limit (on the device the count
    pass checks those two)"""
    if not isinstance(rings, Rings):
        raise ValueError(f"expected Rings or Polygons, got {type(rings).__name__}")
    for name, dtype, dims in (("xy", torch.int32, 2), ("ring_start", torch.int64, 1), ("feature_ring_start", torch.int64, 1), ("values", torch.uint8, 1)):
        t = getattr(rings, name)
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != dims:
            raise ValueError(f"Rings.{name} must be a {dtype} tensor of {dims} dimension(s), got {getattr(t, 'dtype', type(t).__name__)} "
                             f"{tuple(getattr(t, 'shape', ()))}")
        if t.device != rings.xy.device:
            raise ValueError(f"Rings.{name} lives on {t.device}, xy on {rings.xy.device}")
    V, R, F = rings.n_vertices, rings.n_rings, rings.n_features
    if rings.xy.shape[1] != 2 or R < 0 or rings.feature_ring_start.shape[0] != F + 1:
        raise ValueError(f"Rings: xy must be [V, 2], ring_start [R + 1] and feature_ring_start [F + 1] for F = {F} values, got "
                         f"{tuple(rings.xy.shape)}, {tuple(rings.ring_start.shape)}, {tuple(rings.feature_ring_start.shape)}")
    if F >= ops.RAS_MAX_FEATURES:
        raise ValueError(f"Rings: {F} features, the limit is 2^23 - 1")
    if V > ops.VEC_MAX_COUNT:
        raise ValueError(f"Rings: {V} vertices exceed 2^31 - 1")
    if not rings.xy.is_cuda:
        for name, csr, end in (("ring_start", rings.ring_start, V), ("feature_ring_start", rings.feature_ring_start, R)):
            a = csr.numpy()
            if a[0] != 0 or a[-1] != end or (np.diff(a) < 0).any():
                raise ValueError(f"Rings.{name} must rise from 0 to {end} without falling")
        if V and int(rings.xy.abs().max()) > ops.RAS_MAX_COORD:
            raise ValueError("Rings: a coordinate lies outside +-2^21 pixels")
    return rings


def rings_from_polygons(polys: Polygons, values=None) -> Rings:
    """Rings of a Polygons, on the device or the host (where polys lives): one feature per polygon, its rings -- the poly_rings indirection
    resolved -- contiguous, its pixel-corner vertices scaled by 256.  values: one burn value 0..255 per polygon (uint8 tensor or array);
    None takes poly_class"""
    if not isinstance(polys, Polygons):
        raise ValueError(f"expected Polygons, got {type(polys).__name__}")
    dev = polys.xy.device
    i64 = torch.int64
    P = polys.n_polygons
    if values is None:
        values = polys.poly_class
    else:
        values = torch.as_tensor(np.asarray(values) if not isinstance(values, torch.Tensor) else values)
        if values.dtype != torch.uint8 or tuple(values.shape) != (P,):
            raise ValueError(f"values must be uint8 [{P}] (one burn value per polygon), got {values.dtype} {tuple(values.shape)}")
        values = values.to(dev)
    order = polys.poly_rings.to(i64)
    start = polys.ring_start[:-1][order]
    length = polys.ring_start[1:][order] - start
    new_start = torch.cat([torch.zeros(1, dtype=i64, device=dev), torch.cumsum(length, 0)])
    V = int(polys.xy.shape[0]) if order.shape[0] == polys.n_rings else None          # every ring once: no host read for the vertex count
    if V is None:
        V = int(new_start[-1])
    ring_of = torch.searchsorted(new_start[1:].contiguous(), torch.arange(V, dtype=i64, device=dev), right=True)
    src = start[ring_of] + torch.arange(V, dtype=i64, device=dev) - new_start[:-1][ring_of]
    return Rings((polys.xy[src] * ONE).to(torch.int32).contiguous(), new_start, polys.poly_ring_start.to(i64).contiguous(), values.contiguous())


def _check_out(out, H: int, W: int, dev) -> Optional[torch.Tensor]:
    if out is None:
        return None
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (H, W):
        raise ValueError(f"out must be a contiguous uint8 [{H}, {W}] device tensor, got {getattr(out, 'dtype', type(out).__name__)} "
                         f"{tuple(getattr(out, 'shape', ()))} on {getattr(out, 'device', 'the host')}")
    if out.device != dev:
        raise ValueError(f"out lives on {out.device}, the rings on {dev}")
    return out


def _device_rings(what: str, rings_or_polygons, device=None) -> Rings:
    """checked Rings on the device: Polygons are converted, host Rings uploaded (to `device`, or the current one)"""
    rings = rings_from_polygons(rings_or_polygons) if isinstance(rings_or_polygons, Polygons) else rings_or_polygons
    check_rings(rings)
    if not torch.cuda.is_available():
        raise ValueError(f"{what} runs on the GPU and there is no device (it has no host fallback)")
    if not rings.xy.is_cuda:
        rings = rings.to(device if device is not None else "cuda")
    return rings


def _priority_plane(rings: Rings, H: int, W: int, st: _Stages):
    """the count / scan / emit / sort / spans passes, shared by rasterize() and unet_amd.zonal.rasterize_ids(): (plane, M, wrong) with plane
    the int32 [H, W] priority plane, (feature + 1) << 8 | value on every covered pixel and 0 elsewhere, M the crossings and wrong the
    pair-mismatch word (0, or this raises)"""
    dev = rings.xy.device
    i32, i64 = torch.int32, torch.int64
    V, R, F = rings.n_vertices, rings.n_rings, rings.n_features
    xy, ring_start, values = rings.xy.contiguous(), rings.ring_start.contiguous(), rings.values.contiguous()
    M = 0
    if V and R and F:
        vring = torch.searchsorted(ring_start[1:].contiguous(), torch.arange(V, dtype=i64, device=dev), right=True).to(i32)
        ring_feature = torch.searchsorted(rings.feature_ring_start[1:].contiguous(), torch.arange(R, dtype=i64, device=dev), right=True).to(i32)
        counts, info = _alloc((V,), i32, dev), _alloc((2,), i64, dev)
        ops.ras_count(xy, ring_start, vring, V, R, H, counts, info)
        st.mark("count")
        offs, blocks = _alloc((V,), i64, dev), _alloc((ops.ras_scan_words(V),), i64, dev)
        ops.ras_scan(counts, V, offs, blocks, info)
        M, bad = ops.vec_read(info, 0, 2)          # the host read of this stage
        st.mark("scan")
        if bad & 2:
            raise ValueError("Rings: ring_start must rise from 0 to the number of vertices without falling")
        if bad:
            raise ValueError("Rings: a coordinate lies outside +-2^21 pixels")
        if M >= ops.RAS_MAX_CROSSINGS:
            raise ValueError(f"rasterize: {M} crossings, the limit is 2^31 - 1")
        if M % 2:
            raise RuntimeError(f"rasterize: {M} crossings -- closed rings cross the row centres an even number of times")
    keys = None
    if M:
        keys = _alloc((M,), i64, dev)
        ops.ras_emit(xy, ring_start, vring, ring_feature, V, R, H, W, offs, M, keys)
        st.mark("emit")
        keys = torch.sort(keys).values
        st.mark("sort")
    plane, mismatch = _alloc((H, W), i32, dev), _alloc((1,), i64, dev)
    ops.ras_spans(keys, M, values if M else None, F, plane, mismatch)
    wrong = ops.vec_read(mismatch, 0, 1)[0] if M else 0          # a host read
    st.mark("spans")
    if wrong:
        raise RuntimeError(f"rasterize: {wrong} pair(s) of sorted crossings do not belong to one feature and row")
    return plane, M, wrong


def rasterize(rings_or_polygons, shape, fill: int = 0, out: Optional[torch.Tensor] = None, stages: Optional[dict] = None) -> torch.Tensor:
    """uint8 [H, W] device tensor: the burn values of the features (Rings, or Polygons: rings_from_polygons) under the rules of the module
    docstring, `fill` (0..255) where no feature covers a pixel.  Host Rings are uploaded.  out: a contiguous uint8 [H, W] device tensor that
    is burnt into in place and returned; uncovered pixels keep what it held.  stages: a dict that receives the milliseconds of count, scan,
    emit, sort, spans and resolve (this synchronises the device after each: for measurements only), and the counts `crossings`, `features`
    and `pair_mismatch`."""
    H, W = ops.check_raster_shape("rasterize", tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else shape)
    if not _is_int(fill) or not 0 <= fill <= 255:
        raise ValueError(f"fill must be an int in 0..255, got {fill!r}")
    rings = _device_rings("rasterize", rings_or_polygons, out.device if isinstance(out, torch.Tensor) and out.is_cuda else None)
    out = _check_out(out, H, W, rings.xy.device)
    st = _Stages(stages)
    plane, M, wrong = _priority_plane(rings, H, W, st)
    keep = out is not None
    if out is None:
        out = _alloc((H, W), torch.uint8, plane.device)
    ops.ras_resolve(plane, int(fill), keep, out)
    st.mark("resolve")
    if stages is not None:
        stages.update(crossings=M, features=rings.n_features, pair_mismatch=wrong)
    return out


# ------------------------------------------------------------------------------------------------------------------ GeoJSON (host)

def quantise(a: np.ndarray) -> np.ndarray:
    """float64 pixel coordinates -> int32 fixed point, floor(256 x + 0.5); ValueError beyond +-2^21 pixels and for non-finite values"""
    a = np.asarray(a, dtype=np.float64)
    if a.size and not (np.isfinite(a).all() and (np.abs(a) <= MAX_PIXELS_COORD).all()):
        raise ValueError("a coordinate lies outside +-2^21 pixels (or is not finite)")
    return np.floor(a * ONE + 0.5).astype(np.int32)


def _burn_value(props, attribute: str, class_zero: bool, index: int) -> int:
    v = props.get(attribute) if isinstance(props, dict) else None
    if isinstance(v, float) and v.is_integer():
        v = int(v)
    if not _is_int(v):
        raise ValueError(f"feature {index}: the attribute {attribute!r} must be an integer, got {v!r}")
    top = 254 if class_zero else 255
    if not 0 <= v <= top:
        raise ValueError(f"feature {index}: the attribute {attribute!r} must lie in 0..{top}, got {v}")
    return int(v) + (1 if class_zero else 0)


def _load_collection(path) -> dict:
    with open(os.fspath(path)) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or doc.get("type") != "FeatureCollection" or not isinstance(doc.get("features"), list):
        raise ValueError(f"{path}: expected a GeoJSON FeatureCollection")
    return doc


def _parse_features(features: list, geotransform, on_feature):
    """the one ring parser of read_geojson and unet_amd.zonal.read_zones: (quantised vertices [V, 2] with repeated closing points dropped,
    the vertices per ring, the rings per read feature).  on_feature(index, feature) is called for every Polygon / MultiPolygon feature in
    file order, after its geometry type was accepted and before its rings are parsed; features with a null geometry are skipped."""
    pts, ring_len, ring_count = [], [], []
    for index, feat in enumerate(features):
        geom = feat.get("geometry") if isinstance(feat, dict) else None
        if geom is None:
            continue
        kind = geom.get("type") if isinstance(geom, dict) else None
        if kind == "Polygon":
            rings = geom.get("coordinates")
        elif kind == "MultiPolygon":
            rings = [ring for part in geom.get("coordinates") for ring in part]
        else:
            raise ValueError(f"feature {index}: geometry type {kind!r} is not supported (Polygon and MultiPolygon are)")
        on_feature(index, feat)
        ring_count.append(len(rings))
        for ring in rings:
            try:
                flat = [(float(p[0]), float(p[1])) for p in ring]
            except (TypeError, ValueError, IndexError):
                raise ValueError(f"feature {index}: a ring is not a list of [x, y] positions") from None
            pts.extend(flat)
            ring_len.append(len(flat))
    xy = np.array(pts, dtype=np.float64).reshape(-1, 2)
    if geotransform is not None:
        gt = tuple(float(v) for v in geotransform)
        xy = np.stack([(xy[:, 0] - gt[0]) / gt[1], (xy[:, 1] - gt[3]) / gt[5]], axis=1)
    q = quantise(xy)
    # a repeated closing point is dropped
    start = np.concatenate([[0], np.cumsum(ring_len)]).astype(np.int64)
    first, last = start[:-1], start[1:] - 1
    length = np.asarray(ring_len, dtype=np.int64)
    closed = (length > 1) & (q[np.minimum(first, max(len(q) - 1, 0))] == q[np.maximum(last, 0)]).all(axis=1) if len(q) else np.zeros(len(ring_len), bool)
    keep = np.ones(len(q), dtype=bool)
    keep[last[closed]] = False
    return q[keep], length - closed, ring_count


def _host_rings(xy: np.ndarray, length, ring_count, values) -> Rings:
    return check_rings(Rings(torch.from_numpy(np.ascontiguousarray(xy)).reshape(-1, 2),
                             torch.from_numpy(np.concatenate([[0], np.cumsum(length)]).astype(np.int64)),
                             torch.from_numpy(np.concatenate([[0], np.cumsum(ring_count)]).astype(np.int64)),
                             torch.from_numpy(np.asarray(values, dtype=np.uint8))))


def read_geojson(path, geotransform=None, attribute: str = "class", class_zero: bool = False) -> Rings:
    """Rings (host tensors) of a FeatureCollection of Polygon and MultiPolygon geometries: one feature each, in file order, holding all rings
    of all its parts, with the integer property `attribute` (0..255) as its burn value.  Features with a null geometry are skipped; any other
    geometry type, a missing or non-integer attribute or one outside 0..255 raises ValueError naming the feature index.  class_zero adds 1
    to the attribute (the inverse of write_geojson's class_zero, so the attribute must be 0..254).  geotransform: map coordinates become
    pixel coordinates in float64; without one the coordinates are pixel coordinates.  Uses the json module only."""
    check_geojson_args(geotransform)
    doc = _load_collection(path)
    values = []
    xy, length, ring_count = _parse_features(doc["features"], geotransform,
                                             lambda index, feat: values.append(_burn_value(feat.get("properties"), attribute, class_zero, index)))
    return _host_rings(xy, length, ring_count, values)


def rasterize_geojson(path, shape, geotransform=None, attribute: str = "class", fill: int = 0, class_zero: bool = False) -> torch.Tensor:
    """read_geojson + rasterize: the uint8 [H, W] device mask of a GeoJSON file on the grid that shape and geotransform give"""
    return rasterize(read_geojson(path, geotransform, attribute, class_zero), shape, fill)
