"""Cost of the zonal statistics (unet_amd/zonal.py) on a 20000 x 20000 mask.
usage: python scripts/zonal_bench.py [kernels|predict|all] [side=20000] [reps=3] [crop=1000]
Prints one JSON line per measurement and writes them to profiles/zonal_bench.json.
  kernels  the fixed-seed synthetic 5-class mask of scripts/postprocess_bench.py (smooth regions + 2 % salt), raw and after
           PostProcess(majority=5, sieve=64), and three zone sets: (a) a 10 x 10 grid of square zones on the cleaned mask (the LDS form),
           (b) the cleaned mask's own polygons, (c) the raw mask's polygons on the raw mask (the direct form, hardly any wavefront with one
           key).  Per set: rasterize_ids in milliseconds in total (best of `reps` after one warm-up, device synchronised) and per stage (a
           second set of runs that synchronises after every stage); zonal_counts without and with labels (the components of the mask,
           labelled beforehand), with the bytes it must read -- 5 per pixel, 9 with labels --, the rate that makes and its share of the
           6.29 TB/s a float4 copy reaches on this GPU (8.0 TB/s is the specification); and the baseline a user would write,
           torch.bincount(zones.long() * C + mask.long(), minlength=Z * C) over the pixels inside a zone, in the same process, with
           whether the two tables are equal
  host     the NumPy restatement tests/zonal_ref.py (np.add.at) on a crop x crop corner of set (b)
  predict  predict_raster end to end (xresnet34 4 -> 5 bf16, 512 px windows): zones_path=None against the polygons of the cleaned synthetic
           mask as zones (set (b), a GeoJSON file in pixel coordinates), with zonal_seconds and what read_zones alone takes on that file"""
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, HERE)
import torch  # noqa: E402

OUT = os.path.join(HERE, "..", "profiles", "zonal_bench.json")
RESULTS = []
COPY_TBS, SPEC_TBS = 6.29, 8.0          # MI355X: a float4 copy as measured, and the HBM3E specification


def emit(rec):
    """print the record and rewrite the file, so that a run that ends early leaves what it measured"""
    from unet_amd.build import source_hash
    RESULTS.append(rec)
    print(json.dumps(rec), flush=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": RESULTS, "kernel_source_hash": source_hash(),
                   "command": "python scripts/zonal_bench.py " + " ".join(sys.argv[1:])}, f, indent=1)
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


def grid_rings(side: int, k: int = 10):
    """k x k square zones that tile the raster"""
    import numpy as np
    from unet_amd import rasterize as RZ
    edges = [round(i * side / k) * RZ.ONE for i in range(k + 1)]
    xy = [[(edges[i], edges[j]), (edges[i], edges[j + 1]), (edges[i + 1], edges[j + 1]), (edges[i + 1], edges[j])] for j in range(k) for i in range(k)]
    n = k * k
    return RZ.Rings(torch.tensor(xy, dtype=torch.int32).reshape(-1, 2), torch.arange(0, 4 * n + 1, 4, dtype=torch.int64),
                    torch.arange(0, n + 1, dtype=torch.int64), torch.from_numpy(np.zeros(n, dtype=np.uint8))).to("cuda")


def rate(n: int, per_pixel: int, ms: float) -> dict:
    tbs = n * per_pixel / (ms * 1e-3) / 1e12
    return {"ms": round(ms, 3), "bytes_read": n * per_pixel, "TB_per_s": round(tbs, 3), "share_of_copy_rate": round(tbs / COPY_TBS, 3),
            "share_of_spec": round(tbs / SPEC_TBS, 3)}


def one_set(name, rings, mask, labels, reps, C=5):
    from unet_amd import ops
    from unet_amd import zonal as ZN
    n, Z = mask.numel(), rings.n_features
    torch.cuda.empty_cache()
    ids_ms, ids = timed(lambda: ZN.rasterize_ids(rings, mask.shape), reps)
    stages = None
    for _ in range(reps):
        s = {}
        ZN.rasterize_ids(rings, mask.shape, stages=s)
        stages = s if stages is None else {k: min(v, stages[k]) for k, v in s.items()}
    info = {k: stages.pop(k) for k in ("crossings", "features", "pair_mismatch")}
    plain_ms, stats = timed(lambda: ZN.zonal_counts(ids, mask, Z, C), reps)
    both_ms, with_objects = timed(lambda: ZN.zonal_counts(ids, mask, Z, C, labels), reps)
    assert torch.equal(with_objects.counts, stats.counts)

    def baseline():
        inside = ids >= 0
        return torch.bincount(ids[inside].long() * C + mask[inside].long(), minlength=Z * C)

    def baseline_dense():          # every pixel lies in a zone: the one-liner as a user would write it
        return torch.bincount(ids.view(-1).long() * C + mask.view(-1).long(), minlength=Z * C)

    covered = bool((ids >= 0).all())
    base_ms, table = timed(baseline_dense if covered else baseline, reps)
    equal = bool(torch.equal(table.view(Z, C), stats.counts))
    del table
    emit({"what": f"zone set {name}", "mask": f"{mask.shape[0]} x {mask.shape[1]}", "reps": reps, "zones": Z, "classes": C, "bins": Z * C,
          "form": "LDS" if Z * C <= ops.zonal_lds_bins() else "direct", "pixels_in_a_zone": int(stats.counts.sum()), "objects": int(with_objects.objects.sum()),
          **info, "rasterize_ids_ms": round(ids_ms, 3), "rasterize_ids_stage_ms": {k: round(v, 3) for k, v in stages.items()},
          "zonal_counts": rate(n, 5, plain_ms), "zonal_counts_with_labels": rate(n, 9, both_ms),
          "torch_bincount_ms": round(base_ms, 3), "bincount_over_kernel": round(base_ms / plain_ms, 2), "every_pixel_in_a_zone": covered,
          "tables_equal": equal})
    return ids


def host(ids, mask, Z, crop, C=5):
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    import zonal_ref as ZR
    z, m = ids[:crop, :crop].cpu().numpy(), mask[:crop, :crop].cpu().numpy()
    t0 = time.perf_counter()
    ref, _ = ZR.counts(z, m, Z, C)
    dt = time.perf_counter() - t0
    from unet_amd import zonal as ZN
    got = ZN.zonal_counts(ids[:crop, :crop].contiguous(), mask[:crop, :crop].contiguous(), Z, C).counts.cpu().numpy()
    emit({"what": f"host baseline: the NumPy restatement (tests/zonal_ref.py, np.add.at), {crop} x {crop} crop of zone set (b)", "seconds": round(dt, 3),
          "ns_per_pixel": round(dt * 1e9 / z.size, 1), "equals_the_device": bool((ref == got).all())})


def kernels(side, reps, crop):
    from postprocess_bench import synthetic_mask
    from unet_amd import rasterize as RZ
    from unet_amd import vectorize as VZ
    from unet_amd.postprocess import PostProcess, label_components
    mask = synthetic_mask(side)
    clean = PostProcess(majority=5, sieve=64)(mask)
    labels = label_components(clean, 4)
    one_set("(a): a 10 x 10 grid of squares, cleaned mask", grid_rings(side), clean, labels, reps)
    rings = RZ.rings_from_polygons(VZ.polygonize(clean))
    ids = one_set("(b): the cleaned mask's own polygons", rings, clean, labels, reps)
    host(ids, clean, rings.n_features, crop)
    del ids, rings, labels, clean
    torch.cuda.empty_cache()
    labels = label_components(mask, 4)
    one_set("(c): the raw mask's own polygons (2 % salt), raw mask", RZ.rings_from_polygons(VZ.polygonize(mask)), mask, labels, reps)


def predict(side, reps):
    import predict as P
    from postprocess_bench import synthetic_mask
    from unet_amd import vectorize as VZ
    from unet_amd import zonal as ZN
    from unet_amd.postprocess import PostProcess
    from vectorize_bench import _model_and_raster
    with tempfile.TemporaryDirectory() as tmp:
        zones = os.path.join(tmp, "zones.geojson")
        clean = PostProcess(majority=5, sieve=64)(synthetic_mask(side))
        features = VZ.write_geojson(zones, VZ.polygonize(clean))
        del clean
        torch.cuda.empty_cache()
        t0 = time.perf_counter()
        ZN.read_zones(zones)
        read_s = time.perf_counter() - t0
        model, img = _model_and_raster(side)
        times, tm = {"none": [], "zones": []}, {}
        for r in range(reps + 1):
            for name, kw in (("none", {}), ("zones", dict(zones_path=zones, zonal_path=os.path.join(tmp, "t.geojson")))):
                tm = {} if kw else tm
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                P.predict_raster(model, img, 512, 0.2, batch_size=16, timing=tm if kw else None, **kw)
                torch.cuda.synchronize()
                if r:
                    times[name].append(round(time.perf_counter() - t0, 4))
        emit({"what": f"predict_raster end to end, xresnet34 4->5 bf16, {side} x {side}, 512 px windows, overlap 0.2, batch 16 (random raster, untrained "
                      "model), zones = the polygons of the cleaned synthetic mask as a GeoJSON file", "seconds_none": times["none"],
              "seconds_zones": times["zones"], "zonal_seconds_last": round(tm.get("zonal_seconds", float("nan")), 4), "zonal_zones": tm.get("zonal_zones"),
              "zonal_pixels": tm.get("zonal_pixels"), "zones_file_bytes": os.path.getsize(zones), "zones_file_features": features,
              "read_zones_alone_seconds": round(read_s, 3), "table_file_bytes": os.path.getsize(os.path.join(tmp, "t.geojson"))})


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    crop = min(side, int(sys.argv[4]) if len(sys.argv) > 4 else 1000)
    if not torch.cuda.is_available():
        sys.exit("zonal_bench.py measures on the GPU and there is no device")
    if mode in ("kernels", "all"):
        kernels(side, reps, crop)
    if mode in ("predict", "all"):
        predict(side, reps)
