"""Cost of writing a merged prediction that sits in HBM as a tiled GeoTIFF with overviews (unet_amd/tiffenc.py) against the
striped LZW file of DESIGN 3.16 and against what users do today.
usage: python scripts/tiff_cog_bench.py [side=20000] [reps=3] [dir=<tempdir>]
Prints one JSON line per measurement and writes them all to profiles/tiff_cog_bench.json.
Inputs, resident on the device: the 5-class mask with 2 % salt noise of scripts/postprocess_bench.py and the float32 probability plane of
scripts/tiff_write_bench.py.  Per input, alternating in one process, `reps` times after one warm-up each, tensor-in-HBM -> file closed
(no fsync: the page cache takes it):
  s  write_tiff_device: LZW strips (the path of DESIGN 3.16, unchanged)
  t  write_tiff_device(tile=256)
  o  write_tiff_device(tile=256, overviews="mode" for the mask, "average" for the float plane)
  h  .cpu().numpy() + the uncompressed write_tiff: the file users run gdaladdo / gdal_translate -of COG over today.  GDAL is not
     installed, so that second step cannot be timed here: h is a lower bound of the host alternative
Bars, on the medians: (1) t <= s * padded share (ceil(side / 256) * 256)^2 / side^2 + (max - min of s) -- the same encoder over the same
bytes plus padding; (2) o <= 4/3 * t + the same spread -- the pyramid adds a third more samples to encode.
For o the breakdown, every stage waited for on its own: the reduce launch of every level, the encode kernel of every level (device
events), and the copy / file seconds of the overlapped loop."""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "tiff_cog_bench.json")
RESULTS = []
TILE = 256


def emit(rec):
    RESULTS.append(rec)
    print(json.dumps(rec), flush=True)


def breakdown(t: torch.Tensor, how: str):
    """milliseconds of every reduce launch and of every level's encode kernel, each level on its own in the writer's bands (the writer
    itself encodes the levels in one run of bands), device events"""
    from unet_amd import ops, tiffenc
    from unet_amd.tiffio import overview_shapes
    t3 = t[None] if t.dim() == 2 else t
    levels, reduce_ms = [t3], []
    for h, w in overview_shapes(t3.shape[1], t3.shape[2], TILE):
        out = torch.empty((t3.shape[0], h, w), dtype=t3.dtype, device=t3.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.tiff_reduce_level(levels[-1], how, None, out)
        e1.record()
        torch.cuda.synchronize()
        reduce_ms.append(round(e0.elapsed_time(e1), 3))
        levels.append(out)
    slot = ops.tiff_slot_bytes(TILE * TILE * t3.element_size())
    per = max(1, tiffenc.BAND_BYTES // slot)
    if per >= tiffenc._encoders(t3.device):
        per = per // tiffenc._encoders(t3.device) * tiffenc._encoders(t3.device)
    scratch = torch.empty(per * slot, dtype=torch.uint8, device=t3.device)
    sizes = torch.empty(per, dtype=torch.int32, device=t3.device)
    encode_ms = []
    for lv in levels:
        total = lv.shape[0] * -(-lv.shape[1] // TILE) * -(-lv.shape[2] // TILE)
        ms = 0.0
        for first in range(0, total, per):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.tiff_encode_tiles(lv, TILE, 1, first, min(per, total - first), scratch, sizes)
            e1.record()
            torch.cuda.synchronize()
            ms += e0.elapsed_time(e1)
        encode_ms.append(round(ms, 3))
    return {"levels": [list(lv.shape[1:]) for lv in levels], "reduce_ms": reduce_ms, "encode_ms": encode_ms}


def main():
    from postprocess_bench import synthetic_mask
    from tiff_write_bench import prob_plane, spread
    from unet_amd.tiffenc import write_tiff_device
    from unet_amd.tiffio import write_tiff
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    d = sys.argv[3] if len(sys.argv) > 3 else tempfile.gettempdir()
    path = os.path.join(d, "tiff_cog_bench.tif")
    padded = (-(-side // TILE) * TILE) ** 2 / side ** 2
    emit({"what": "setup", "side": side, "reps": reps, "dir": d, "tile": TILE, "padded_share": round(padded, 5),
          "device": torch.cuda.get_device_name(0), "gdaladdo_timed": False})
    for name, make, how in (("mask_salt2", lambda: synthetic_mask(side), "mode"), ("prob_f32", lambda: prob_plane(side), "average")):
        t = make()
        torch.cuda.synchronize()
        tm = {}
        paths = {
            "s_device_strips": lambda: write_tiff_device(path, t),
            "t_device_tiles": lambda: write_tiff_device(path, t, tile=TILE),
            "o_device_tiles_overviews": lambda: write_tiff_device(path, t, tile=TILE, overviews=how, timing=tm),
            "h_cpu_uncompressed": lambda: write_tiff(path, t.cpu().numpy()),
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
        stat = {k: spread(v) for k, v in times.items()}
        for k in paths:
            emit({"what": "write", "input": name, "path": k, "input_bytes": nbytes, "file_bytes": sizes[k], "seconds": stat[k]})
        s, tt, o = stat["s_device_strips"], stat["t_device_tiles"], stat["o_device_tiles_overviews"]
        slack = s["max"] - s["min"]
        lim1, lim2 = s["median"] * padded + slack, 4.0 / 3.0 * tt["median"] + slack
        emit({"what": "bars", "input": name, "spread_of_s": round(slack, 4),
              "bar1_t_vs_s": {"limit": round(lim1, 4), "t_median": tt["median"], "met": bool(tt["median"] <= lim1)},
              "bar2_o_vs_t": {"limit": round(lim2, 4), "o_median": o["median"], "met": bool(o["median"] <= lim2)}})
        emit({"what": "o_loop_seconds", "input": name, "resampling": how,
              **{k: (round(v, 4) if isinstance(v, float) else v) for k, v in tm.items()}})
        breakdown(t, how)
        emit({"what": "o_breakdown", "input": name, "resampling": how, **breakdown(t, how)})
        del t
        torch.cuda.empty_cache()
    os.remove(path)
    with open(OUT, "w") as f:
        json.dump(RESULTS, f, indent=1)


if __name__ == "__main__":
    main()
