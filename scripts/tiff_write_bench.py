"""Cost of writing a merged prediction that sits in HBM: uncompressed (the path before compress= existed) against LZW on the host and
LZW on the device (unet_amd/tiffenc.py).
usage: python scripts/tiff_write_bench.py [side=20000] [reps=3] [dir=<tempdir>]
Prints one JSON line per measurement and writes them all to profiles/tiff_write_bench.json.
Inputs, resident on the device: the 5-class mask with 2 % salt noise of scripts/postprocess_bench.py, the same mask without noise, and
one float32 plane of smooth probabilities with fp32 rounding noise in the low mantissa bits (the bad case for LZW).
Per input, alternating in one process, `reps` times after one warm-up each, tensor-in-HBM -> file closed (no fsync: the page cache takes it):
  a  .cpu().numpy() + the uncompressed write_tiff
  b  .cpu().numpy() + write_tiff(compress="lzw") on UNET_TIFF_THREADS=16 host threads
  c  write_tiff_device (encode kernel, compaction, copy of the compact bytes, file write)
and for c the breakdown, measured band by band without overlap: encode kernel and compaction (device events), copy, file write; the
encode kernel's input GB/s and the compression ratio."""
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("UNET_TIFF_THREADS", "16")
import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "tiff_write_bench.json")
RESULTS = []


def emit(rec):
    RESULTS.append(rec)
    print(json.dumps(rec), flush=True)


def spread(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def prob_plane(side: int) -> torch.Tensor:
    g = torch.Generator(device="cuda").manual_seed(1)
    coarse = torch.rand((1, 1, side // 128 + 2, side // 128 + 2), device="cuda", generator=g)
    return torch.nn.functional.interpolate(coarse, size=(side, side), mode="bilinear", align_corners=False)[0, 0].contiguous()


def breakdown(t: torch.Tensor, path: str):
    """one pass of the device path with every stage waited for on its own: seconds of encode kernel, compaction, copy, file write"""
    from unet_amd import ops, tiffenc
    from unet_amd.tiffio import StripWriter
    t3 = t[None] if t.dim() == 2 else t
    C, H, W = t3.shape
    w = StripWriter(path, C, H, W, tiffenc._NP[t3.dtype])
    slot = ops.tiff_slot_bytes(w.rows_per_strip * W * t3.element_size())
    per = min(max(1, tiffenc.BAND_BYTES // slot), len(w.strips))
    scratch = torch.empty(per * slot, dtype=torch.uint8, device="cuda")
    compact = torch.empty(per * slot, dtype=torch.uint8, device="cuda")
    sizes = torch.empty(per, dtype=torch.int32, device="cuda")
    pinned = torch.empty(per * slot, dtype=torch.uint8, pin_memory=True)
    sec = {"encode_kernel": 0.0, "compaction": 0.0, "copy": 0.0, "file": 0.0}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for first in range(0, len(w.strips), per):
        n = min(per, len(w.strips) - first)
        ev[0].record()
        ops.tiff_encode_strips(t3, w.rows_per_strip, 1, first, n, scratch, sizes)
        ev[1].record()
        sz = sizes[:n].to(torch.int64)
        excl = torch.cumsum(sz, 0) - sz
        ops.tiff_compact_strips(scratch, slot, sizes, excl, n, compact)
        ev[2].record()
        torch.cuda.synchronize()
        sec["encode_kernel"] += ev[0].elapsed_time(ev[1]) * 1e-3
        sec["compaction"] += ev[1].elapsed_time(ev[2]) * 1e-3
        t0 = time.perf_counter()
        host = sz.cpu().numpy()
        nbytes = int(host.sum())
        pinned[:nbytes].copy_(compact[:nbytes])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        w.append(pinned[:nbytes].numpy().data, host)
        sec["copy"] += t1 - t0
        sec["file"] += time.perf_counter() - t1
    t0 = time.perf_counter()
    size = w.close()
    sec["file"] += time.perf_counter() - t0
    return sec, size


def main():
    from postprocess_bench import synthetic_mask
    from unet_amd.tiffenc import write_tiff_device
    from unet_amd.tiffio import write_tiff
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    d = sys.argv[3] if len(sys.argv) > 3 else tempfile.gettempdir()
    path = os.path.join(d, "tiff_write_bench.tif")
    emit({"what": "setup", "side": side, "reps": reps, "dir": d, "host_threads": int(os.environ["UNET_TIFF_THREADS"]),
          "device": torch.cuda.get_device_name(0)})
    inputs = [("mask_salt2", lambda: synthetic_mask(side)), ("mask_clean", lambda: synthetic_mask(side, salt=0.0)), ("prob_f32", lambda: prob_plane(side))]
    for name, make in inputs:
        t = make()
        torch.cuda.synchronize()
        paths = {
            "a_uncompressed": lambda: write_tiff(path, t.cpu().numpy()),
            "b_host_lzw": lambda: write_tiff(path, t.cpu().numpy(), compress="lzw"),
            "c_device_lzw": lambda: write_tiff_device(path, t),
        }
        times, sizes = {k: [] for k in paths}, {}
        for r in range(reps + 1):
            for k, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                sizes[k] = os.path.getsize(path)
                if r:
                    times[k].append(dt)
        nbytes = t.numel() * t.element_size()
        assert sizes["b_host_lzw"] == sizes["c_device_lzw"]
        for k in paths:
            emit({"what": "write", "input": name, "path": k, "input_bytes": nbytes, "file_bytes": sizes[k], "seconds": spread(times[k])})
        sec, size = breakdown(t, path)          # second pass: kernels warm
        sec, size = breakdown(t, path)
        emit({"what": "device_breakdown", "input": name, "seconds": {k: round(v, 4) for k, v in sec.items()},
              "encode_input_GBps": round(nbytes / sec["encode_kernel"] / 1e9, 2), "compression_ratio": round(nbytes / size, 2)})
        del t
        torch.cuda.empty_cache()
    os.remove(path)
    with open(OUT, "w") as f:
        json.dump(RESULTS, f, indent=1)


if __name__ == "__main__":
    main()
