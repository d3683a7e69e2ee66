"""LZW-compressed GeoTIFFs of device tensors, encoded on the device (csrc/tiff_encode.hip).  The file is the one
tiffio.write_tiff(compress="lzw") writes from the same samples, byte for byte: same layout (tiffio.StripWriter), same code stream.

The image is walked in bands of strips.  A band is encoded into a scratch buffer of one capacity slot per strip (launch A), packed into
one contiguous buffer at the exclusive prefix sum of the strip sizes (launch B), and only that buffer and the sizes travel to the host:
into pinned memory on a copy stream, then into the file, while the next band is being encoded.  The band size bounds the device memory:
BAND_BYTES (128 MiB) of slots + two compact buffers of the same size = 384 MiB at most beside the image, whatever its size; a band is
never smaller than one strip.  The file does not depend on the band size.

Tiled files with overviews (tile=, overviews=; the layout is tiffio.TileWriter, the file again write_tiff's byte for byte).
The pyramid is built first, on the device (csrc/tiff_pyramid.hip, one launch per level over all planes); then the banded loop above runs
over the square tiles of all levels in file order, the smallest level first (unet_tiff_encode_tile_levels: the same encoder, one
wavefront per tile).  Level 0 is read in place; the lower levels are dense tensors of at most (1/3 + edge rounding) of the image together --
sum over k >= 1 of ceil(H / 2^k) * ceil(W / 2^k) samples per plane -- beside the 384 MiB above, which hold for tiles as they do for
strips.  A band of tiles runs through the levels in file order, so the small levels of a pyramid share launches instead of costing one
tile's latency each; every tile is as long as every other, so a default band that holds at least one round of the encoders resident at
once (4 per compute unit) is cut down to whole rounds.  A band is never smaller than one tile.

The pyramid rule.  Level k + 1 is computed from level k, never from level 0, and has ceil(H_k / 2) x ceil(W_k / 2) samples per plane; levels
are added while max(H_k, W_k) > tile, so the last level fits one tile and a raster no larger than one tile has no overviews.  An output
sample looks at the up-to-2x2 block of its parent, clipped at odd edges to 1 or 2 samples, in row-major order (TL, TR, BL, BR).  A sample
is valid if no nodata was given or if it differs from nodata (NaN nodata: valid means not NaN; a nodata that no sample of an integer
type can equal leaves every sample valid).  A block without a valid sample gives nodata.
  "nearest"  the top-left sample, valid or not
  "mode"     the valid value with the highest count; ties go to the value that occurs first in row-major order (integer samples only; no
             claim of bit-compatibility with GDAL's mode)
  "average"  integers: floor((2 s + n) / (2 n)), s the exact sum of the n valid samples (round half up, also for negative values);
             float32: the valid samples summed one after the other in fp32, starting from +0, in row-major order, then divided by
             float(n) with a correctly rounded division
tiffio.reduce_level is the same rule in NumPy for host arrays, tests/tiff_cog_ref.py its restatement sample by sample."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import ops
from .tiffio import RESAMPLINGS, StripWriter, TileWriter, check_compress, check_tiling, overview_shapes

BAND_BYTES = 128 << 20

_NP = {torch.uint8: np.uint8, torch.int8: np.int8, torch.int16: np.int16, torch.uint16: np.uint16, torch.int32: np.int32,
       torch.float32: np.float32}
_CAST = {torch.bool: torch.uint8, torch.int64: torch.int32, torch.float64: torch.float32}          # as tiffio.write_tiff casts


def _alloc(shape, dtype, device) -> torch.Tensor:
    """every device buffer of this module (the tests put guard bands around them here)"""
    return torch.empty(tuple(shape), dtype=dtype, device=device)


def write_tiff_device(path, t: torch.Tensor, geotransform=None, tags: Optional[Dict[int, tuple]] = None, nodata=None,
                      bigtiff: Optional[bool] = None, compress="lzw", predictor: int = 1, rows_per_strip=None, band_strips: Optional[int] = None,
                      timing: Optional[dict] = None, tile: Optional[int] = None, overviews: Optional[str] = None) -> int:
    """tiffio.write_tiff(compress="lzw") of a device tensor [C, H, W] or [H, W] (rows contiguous; row and plane strides are free, so a
    row slice or one plane of a larger tensor is encoded in place) -> the file's size in bytes.  band_strips: strips per band (None:
    as many as fit BAND_BYTES of scratch).  timing gains encode_seconds (launch A + B, waited for), copy_seconds, file_seconds.
    tile (a multiple of 16 in 16..1024): square LZW tiles instead of strips; overviews "mode" | "average" | "nearest" (needs tile): the
    overview pyramid behind the full-resolution image (module docstring).  band_strips then counts tiles, and timing also gains
    reduce_seconds (the pyramid launches, waited for) and levels (the samples per plane side of every level written)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("write_tiff_device: expected a tensor on the GPU")
    if compress != "lzw":
        raise ValueError(f"write_tiff_device: compress must be 'lzw', got {compress!r}")
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3:
        raise ValueError(f"write_tiff_device: expected [C, H, W] or [H, W], got shape {tuple(t.shape)}")
    if t.dtype in _CAST:
        t = t.to(_CAST[t.dtype])
    if t.dtype not in _NP:
        raise ValueError(f"write_tiff_device: {t.dtype} samples are not written")
    check_compress(compress, predictor, t.dtype.is_floating_point)
    tile, overviews = check_tiling(compress, tile, overviews, t.dtype.is_floating_point)
    if tile is not None and rows_per_strip is not None:
        raise ValueError("rows_per_strip is for strips: a tiled file (tile=) has none")
    if t.stride(2) != 1 or t.stride(1) < t.shape[2] or (t.shape[0] > 1 and t.stride(0) < 1):
        t = t.contiguous()
    C, H, W = (int(v) for v in t.shape)
    if tile is not None:
        return _write_tiled(path, t, tile, overviews, geotransform, tags, nodata, bigtiff, predictor, band_strips, timing)
    w = StripWriter(path, C, H, W, _NP[t.dtype], rows_per_strip, predictor, geotransform, tags, nodata, bigtiff)
    try:
        slot = ops.tiff_slot_bytes(w.rows_per_strip * w.W * t.element_size())
        _encode_bands(w, lambda first, n, scratch, sizes: ops.tiff_encode_strips(t, w.rows_per_strip, w.predictor, first, n, scratch, sizes),
                      len(w.strips), slot, t.device, band_strips, timing)
    except BaseException:
        w.f.close()
        raise
    return w.close()


def build_overviews(t: torch.Tensor, resampling: str, nodata=None, tile: int = 256) -> list:
    """The overview levels of a device tensor [C, H, W] or [H, W] (strides as write_tiff_device takes them: level 0 is read in place) by
    the pyramid rule of the module docstring: [level 1, level 2, ...], dense tensors of t's dtype, each computed from the one before it,
    down to the first level that fits one tile (none for a raster no larger than a tile).  One launch per level over all planes."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("build_overviews: expected a tensor on the GPU")
    if resampling not in RESAMPLINGS:
        raise ValueError(f"build_overviews: resampling must be one of {RESAMPLINGS}, got {resampling!r}")
    flat = t.dim() == 2
    if flat:
        t = t[None]
    if t.dim() != 3 or t.dtype not in _NP:
        raise ValueError(f"build_overviews: expected [C, H, W] or [H, W] samples of {sorted(str(d) for d in _NP)}, got {tuple(t.shape)} {t.dtype}")
    check_tiling("lzw", tile, resampling, t.dtype.is_floating_point)
    out = []
    with torch.cuda.device(t.device):
        for h, w in overview_shapes(int(t.shape[1]), int(t.shape[2]), tile):
            t = ops.tiff_reduce_level(t, resampling, nodata, _alloc((t.shape[0], h, w), t.dtype, t.device))
            out.append(t)
    return [l[0] for l in out] if flat else out


def _write_tiled(path, t, tile, overviews, geotransform, tags, nodata, bigtiff, predictor, band_tiles, timing) -> int:
    import time
    t0 = time.perf_counter()
    levels = [t] + (build_overviews(t, overviews, nodata, tile) if overviews is not None else [])
    if len(levels) > 1:
        torch.cuda.synchronize(t.device)
    reduce_seconds = time.perf_counter() - t0
    w = TileWriter(path, int(t.shape[0]), [l.shape[1:] for l in levels], _NP[t.dtype], tile, predictor, geotransform, tags, nodata, bigtiff)
    slot = ops.tiff_slot_bytes(tile * tile * t.element_size())
    sec = {}
    in_file_order = [levels[k] for k in w.order]                                   # the smallest level first, the full resolution last
    try:
        _encode_bands(w, lambda first, n, scratch, sizes: ops.tiff_encode_tiles(in_file_order, tile, predictor, first, n, scratch, sizes),
                      sum(w.per_level), slot, t.device, band_tiles, sec, _encoders(t.device))
    except BaseException:
        w.f.close()
        raise
    if timing is not None:
        timing.update(sec, reduce_seconds=reduce_seconds, levels=[tuple(int(v) for v in l.shape[1:]) for l in levels])
    return w.close()


def _encoders(dev) -> int:
    """encoder wavefronts that are resident at once: 35 KiB of LDS each, four per compute unit"""
    return 4 * torch.cuda.get_device_properties(dev).multi_processor_count


def _encode_bands(w, encode, total: int, slot: int, dev, band_strips: Optional[int], timing: Optional[dict], whole_rounds: int = 0):
    """the banded loop over `total` blocks (strips, or the tiles of all levels in file order) of `slot` bytes of scratch each:
    encode(first, n, scratch, sizes) launches the encoder for blocks [first, first + n); w.append takes their streams in order.
    whole_rounds: a default band of at least that many blocks is cut down to a multiple of it"""
    import time
    per = max(1, BAND_BYTES // slot) if band_strips is None else int(band_strips)
    if per < 1:
        raise ValueError(f"band_strips must be None or >= 1, got {band_strips!r}")
    if band_strips is None and whole_rounds and per >= whole_rounds:
        per = per // whole_rounds * whole_rounds
    per = min(per, total)
    scratch = _alloc((per * slot,), torch.uint8, dev)
    ring = [(_alloc((per,), torch.int32, dev), _alloc((per * slot,), torch.uint8, dev)) for _ in range(2 if total > per else 1)]
    copy_stream = torch.cuda.Stream(dev)
    pinned = [None]
    sec = {"encode_seconds": 0.0, "copy_seconds": 0.0, "file_seconds": 0.0}

    def launch(k, first, n):
        sizes, compact = ring[k % len(ring)]
        encode(first, n, scratch, sizes)
        offsets = torch.cumsum(sizes[:n].to(torch.int64) & 0xFFFFFFFF, 0)          # (sizes are unsigned words)
        excl = _alloc((n,), torch.int64, dev)
        excl[0] = 0
        excl[1:] = offsets[:-1]
        ops.tiff_compact_strips(scratch, slot, sizes, excl, n, compact)
        ev = torch.cuda.Event()
        ev.record()
        return n, sizes, compact, ev

    def finish(job):
        n, sizes, compact, ev = job
        t0 = time.perf_counter()
        ev.synchronize()
        t1 = time.perf_counter()
        with torch.cuda.stream(copy_stream):
            host_sizes = (sizes[:n].cpu().numpy().astype(np.int64) & 0xFFFFFFFF)
            if (host_sizes > slot).any():
                raise RuntimeError("tiff_encode_strips: a strip overran its capacity slot")
            nbytes = int(host_sizes.sum())
            if pinned[0] is None or pinned[0].numel() < nbytes:
                pinned[0] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
            pinned[0][:nbytes].copy_(compact[:nbytes], non_blocking=True)
        copy_stream.synchronize()
        t2 = time.perf_counter()
        w.append(pinned[0][:nbytes].numpy().data, host_sizes)
        t3 = time.perf_counter()
        sec["encode_seconds"] += t1 - t0
        sec["copy_seconds"] += t2 - t1
        sec["file_seconds"] += t3 - t2

    with torch.cuda.device(dev):
        prev = None
        for k, first in enumerate(range(0, total, per)):
            job = launch(k, first, min(per, total - first))
            if prev is not None:
                finish(prev)
            prev = job
        finish(prev)
    if timing is not None:
        timing.update(sec)
