"""LZW-compressed GeoTIFFs of device tensors, encoded on the device (csrc/tiff_encode.hip).  The file is the one
tiffio.write_tiff(compress="lzw") writes from the same samples, byte for byte: same layout (tiffio.StripWriter), same code stream.

The image is walked in bands of strips.  A band is encoded into a scratch buffer of one capacity slot per strip (launch A), packed into
one contiguous buffer at the exclusive prefix sum of the strip sizes (launch B), and only that buffer and the sizes travel to the host:
into pinned memory on a copy stream, then into the file, while the next band is being encoded.  The band size bounds the device memory:
BAND_BYTES (128 MiB) of slots + two compact buffers of the same size = 384 MiB at most beside the image, whatever its size; a band is
never smaller than one strip.  The file does not depend on the band size."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import ops
from .tiffio import StripWriter, check_compress

BAND_BYTES = 128 << 20

_NP = {torch.uint8: np.uint8, torch.int8: np.int8, torch.int16: np.int16, torch.uint16: np.uint16, torch.int32: np.int32,
       torch.float32: np.float32}
_CAST = {torch.bool: torch.uint8, torch.int64: torch.int32, torch.float64: torch.float32}          # as tiffio.write_tiff casts


def _alloc(shape, dtype, device) -> torch.Tensor:
    """every device buffer of this module (the tests put guard bands around them here)"""
    return torch.empty(tuple(shape), dtype=dtype, device=device)


def write_tiff_device(path, t: torch.Tensor, geotransform=None, tags: Optional[Dict[int, tuple]] = None, nodata=None,
                      bigtiff: Optional[bool] = None, compress="lzw", predictor: int = 1, rows_per_strip=None, band_strips: Optional[int] = None,
                      timing: Optional[dict] = None) -> int:
    """tiffio.write_tiff(compress="lzw") of a device tensor [C, H, W] or [H, W] (rows contiguous; row and plane strides are free, so a
    row slice or one plane of a larger tensor is encoded in place) -> the file's size in bytes.  band_strips: strips per band (None:
    as many as fit BAND_BYTES of scratch).  timing gains encode_seconds (launch A + B, waited for), copy_seconds, file_seconds."""
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
    if t.stride(2) != 1 or t.stride(1) < t.shape[2] or (t.shape[0] > 1 and t.stride(0) < 1):
        t = t.contiguous()
    C, H, W = (int(v) for v in t.shape)
    w = StripWriter(path, C, H, W, _NP[t.dtype], rows_per_strip, predictor, geotransform, tags, nodata, bigtiff)
    try:
        _encode_bands(w, t, band_strips, timing)
    except BaseException:
        w.f.close()
        raise
    return w.close()


def _encode_bands(w: StripWriter, t: torch.Tensor, band_strips: Optional[int], timing: Optional[dict]):
    import time
    dev, total = t.device, len(w.strips)
    slot = ops.tiff_slot_bytes(w.rows_per_strip * w.W * t.element_size())
    per = max(1, BAND_BYTES // slot) if band_strips is None else int(band_strips)
    if per < 1:
        raise ValueError(f"band_strips must be None or >= 1, got {band_strips!r}")
    per = min(per, total)
    scratch = _alloc((per * slot,), torch.uint8, dev)
    ring = [(_alloc((per,), torch.int32, dev), _alloc((per * slot,), torch.uint8, dev)) for _ in range(2 if total > per else 1)]
    copy_stream = torch.cuda.Stream(dev)
    pinned = [None]
    sec = {"encode_seconds": 0.0, "copy_seconds": 0.0, "file_seconds": 0.0}

    def launch(k, first, n):
        sizes, compact = ring[k % len(ring)]
        ops.tiff_encode_strips(t, w.rows_per_strip, w.predictor, first, n, scratch, sizes)
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
