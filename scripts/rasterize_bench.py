"""Cost of the rasterizer (unet_amd/rasterize.py) on the polygons of a 20000 x 20000 mask.
usage: python scripts/rasterize_bench.py [side=20000] [reps=3] [crop=1000]
Prints one JSON line per measurement and writes them to profiles/rasterize_bench.json.
  rings    the fixed-seed synthetic 5-class mask of scripts/vectorize_bench.py (smooth regions + 2 % salt), raw and after
           PostProcess(majority=5, sieve=64): rasterize(rings_from_polygons(polygonize(mask))) in milliseconds in total (best of `reps` after
           one warm-up, device synchronised) and per stage -- count, scan, emit, sort, spans, resolve: a second set of runs that synchronises
           after every stage --, with the crossings M, the features, the peak device memory of one call above what the rings hold, and whether
           the mask came back
  geojson  the cleaned mask polygonized with simplify=1, written by write_geojson: seconds of read_geojson (host, the json module) and of
           rasterize on what it read, with the share of pixels that differ from the cleaned mask (simplified borders move)
  host     the plain-Python reference tests/rasterize_ref.py -- the only other rasterizer at hand -- on the polygons of a crop x crop corner
           of both masks, as ns per pixel next to the device's"""
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, HERE)
import torch  # noqa: E402

OUT = os.path.join(HERE, "..", "profiles", "rasterize_bench.json")
RESULTS = []
GT = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)


def emit(rec):
    """print the record and rewrite the file, so that a run that ends early leaves what it measured"""
    from unet_amd.build import source_hash
    RESULTS.append(rec)
    print(json.dumps(rec), flush=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": RESULTS, "kernel_source_hash": source_hash(),
                   "command": "python scripts/rasterize_bench.py " + " ".join(sys.argv[1:])}, f, indent=1)
        f.write("\n")


def timed(fn, reps):
    best, out = None, None
    for r in range(reps + 1):
        out = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        if r and (best is None or dt < best):
            best = dt
    return best, out


def one_mask(name, mask, reps):
    from unet_amd import rasterize as RZ
    from unet_amd import vectorize as VZ
    n = mask.numel()
    rings = RZ.rings_from_polygons(VZ.polygonize(mask))
    torch.cuda.empty_cache()
    ms, out = timed(lambda: RZ.rasterize(rings, mask.shape, fill=255), reps)
    same = bool(torch.equal(out, mask))
    del out
    stages = None
    for _ in range(reps):          # per stage: the smallest of each over the runs (these runs wait for the device after every stage)
        s = {}
        RZ.rasterize(rings, mask.shape, fill=255, stages=s)
        stages = s if stages is None else {k: min(v, stages[k]) for k, v in s.items()}
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    RZ.rasterize(rings, mask.shape, fill=255)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    counts = {k: stages.pop(k) for k in ("crossings", "features", "pair_mismatch")}
    emit({"what": f"rasterize(polygonize(mask)), {name}", "mask": f"{mask.shape[0]} x {mask.shape[1]}", "reps": reps, "vertices": rings.n_vertices,
          "rings": rings.n_rings, **counts, "ms": round(ms, 3), "ns_per_pixel": round(ms * 1e6 / n, 4),
          "stage_ms": {k: round(v, 3) for k, v in stages.items()}, "peak_bytes_of_one_call": int(peak), "mask_came_back": same})
    return ms * 1e6 / n


def geojson(clean, reps):
    from unet_amd import rasterize as RZ
    from unet_amd import vectorize as VZ
    polys = VZ.polygonize(clean, simplify=1)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.geojson")
        feats = VZ.write_geojson(path, polys, GT, 32632)
        size = os.path.getsize(path)
        del polys
        t0 = time.perf_counter()
        rings = RZ.read_geojson(path, GT)
        read_s = time.perf_counter() - t0
    dev = rings.to("cuda")
    ms, out = timed(lambda: RZ.rasterize(dev, clean.shape, fill=255), reps)
    emit({"what": "GeoJSON of the cleaned mask, simplified at 1 px: read_geojson (host) and rasterize of its rings", "features": feats,
          "geojson_bytes": size, "vertices": rings.n_vertices, "read_geojson_seconds": round(read_s, 2), "rasterize_seconds": round(ms / 1e3, 4),
          "pixels_that_differ_from_the_cleaned_mask": round(float((out != clean).float().mean()), 6), "uncovered_pixels": int((out == 255).sum())})


def host(masks, crop):
    from unet_amd import rasterize as RZ
    from unet_amd import vectorize as VZ
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    import rasterize_ref as RR
    for name, m, dev_ns in masks:
        a = m[:crop, :crop].contiguous()
        r = RZ.rings_from_polygons(VZ.polygonize(a)).to("cpu")
        t0 = time.perf_counter()
        ref = RR.rasterize(r.xy.numpy(), r.ring_start.numpy(), r.feature_ring_start.numpy(), r.values.numpy(), tuple(a.shape), 255)
        dt = time.perf_counter() - t0
        emit({"what": f"host baseline: the plain-Python reference rasterizer (tests/rasterize_ref.py), {crop} x {crop} crop of the {name} mask",
              "seconds": round(dt, 2), "ns_per_pixel": round(dt * 1e9 / a.numel(), 1), "features": r.n_features,
              "equals_the_crop": bool((torch.from_numpy(ref) == a.cpu()).all()), "device_ns_per_pixel_full_mask": round(dev_ns, 4)})


if __name__ == "__main__":
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    crop = min(side, int(sys.argv[3]) if len(sys.argv) > 3 else 1000)
    if not torch.cuda.is_available():
        sys.exit("rasterize_bench.py measures on the GPU and there is no device")
    from postprocess_bench import synthetic_mask
    from unet_amd.postprocess import PostProcess
    mask = synthetic_mask(side)
    raw_ns = one_mask("5 classes, smooth regions + 2 % salt", mask, reps)
    clean = PostProcess(majority=5, sieve=64)(mask)
    torch.cuda.empty_cache()
    clean_ns = one_mask("the same after PostProcess(majority=5, sieve=64)", clean, reps)
    host((("raw", mask, raw_ns), ("cleaned", clean, clean_ns)), crop)
    del mask
    torch.cuda.empty_cache()
    geojson(clean, reps)
