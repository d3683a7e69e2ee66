"""Cost of the polygonizer (unet_amd/vectorize.py) on a 20000 x 20000 mask, and of predict_raster with it.
usage: python scripts/vectorize_bench.py [kernels|predict|all] [side=20000] [reps=3]
       python scripts/vectorize_bench.py tree DIR [side=20000] [reps=3]
Prints one JSON line per measurement; kernels / predict / all write them to profiles/vectorize_bench.json.
  kernels  the fixed-seed synthetic 5-class mask of scripts/postprocess_bench.py (smooth regions + 2 % salt), raw and after
           PostProcess(majority=5, sieve=64): edges, rings, polygons, vertices, milliseconds in total (best of `reps` after one warm-up,
           device synchronised) and per stage (a second set of runs that synchronises after every stage), bytes copied to the host by
           Polygons.cpu(), seconds of write_geojson (host text formatting, not the hot path); the host baseline -- the plain-Python
           reference tests/vectorize_ref.py, the only other polygonizer at hand -- on a 1000 x 1000 crop as ns per pixel next to the device's
  predict  BASELINE configs[4] (xresnet34 4 -> 5, bf16 storage, 512 px windows, overlap 0.2, batch 16) on a side x side raster end to end,
           vector_path=None against a vector_path, alternated
  tree     predict_raster without a vector output from the checkout at DIR (this tree or another commit's, built), a fresh process per call:
           one JSON line with the seconds of `reps` runs after a warm-up and the SHA-1 of the mask, to compare trees in alternation"""
import hashlib
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
if len(sys.argv) > 2 and sys.argv[1] == "tree":
    ROOT = sys.argv[2]
sys.path.insert(0, os.path.abspath(ROOT))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(HERE, "..", "profiles", "vectorize_bench.json")
RESULTS = []


def emit(rec):
    RESULTS.append(rec)
    print(json.dumps(rec), flush=True)


def timed(fn, reps):
    best, out = None, None
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        if r and (best is None or dt < best):
            best = dt
    return best, out


def one_mask(name, mask, reps, tmp, write=True):
    from unet_amd import vectorize as VZ
    n = mask.numel()
    ms, polys = timed(lambda: VZ.polygonize(mask), reps)
    stages = None
    for _ in range(reps):          # per stage: the smallest of each over the runs (these runs wait for the device after every stage)
        s = {}
        VZ.polygonize(mask, stages=s)
        stages = s if stages is None else {k: min(v, stages[k]) for k, v in s.items()}
    t0 = time.perf_counter()
    host = polys.cpu()
    torch.cuda.synchronize()
    copy_s = time.perf_counter() - t0
    nbytes = sum(getattr(host, k).numel() * getattr(host, k).element_size() for k in
                 ("xy", "ring_start", "ring_label", "ring_area", "poly_label", "poly_class", "poly_pixels", "poly_ring_start", "poly_rings"))
    rec = {"what": f"polygonize, {name}", "mask": f"{mask.shape[0]} x {mask.shape[1]}", "reps": reps, "edges": polys.edges, "rings": polys.n_rings,
           "polygons": polys.n_polygons, "vertices": polys.n_vertices, "ms": round(ms, 3), "ns_per_pixel": round(ms * 1e6 / n, 4),
           "stage_ms": {k: round(v, 3) for k, v in stages.items()}, "bytes_to_host": nbytes, "copy_seconds": round(copy_s, 3)}
    if write:
        path = os.path.join(tmp, "bench.geojson")
        t0 = time.perf_counter()
        feats = VZ.write_geojson(path, host, (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5), 32632)
        rec.update(write_geojson_seconds=round(time.perf_counter() - t0, 2), features=feats, geojson_bytes=os.path.getsize(path))
        os.remove(path)
    else:
        rec["write_geojson_seconds"] = "not measured: millions of one-pixel polygons, a file nobody wants"
    emit(rec)
    return ms * 1e6 / n


def kernels(side: int, reps: int):
    from postprocess_bench import synthetic_mask
    from unet_amd.postprocess import PostProcess
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    import vectorize_ref as V
    mask = synthetic_mask(side)
    with tempfile.TemporaryDirectory() as tmp:
        raw_ns = one_mask("5 classes, smooth regions + 2 % salt", mask, reps, tmp, write=side <= 4000)
        clean = PostProcess(majority=5, sieve=64)(mask)
        torch.cuda.empty_cache()
        clean_ns = one_mask("the same after PostProcess(majority=5, sieve=64)", clean, reps, tmp)
    crop = min(side, 1000)
    for name, m, dev_ns in (("raw", mask, raw_ns), ("cleaned", clean, clean_ns)):
        a = m[:crop, :crop].cpu().numpy()
        t0 = time.perf_counter()
        ref = V.polygonize(a)
        dt = time.perf_counter() - t0
        emit({"what": f"host baseline: the plain-Python reference tracer (tests/vectorize_ref.py), {crop} x {crop} crop of the {name} mask",
              "seconds": round(dt, 2), "ns_per_pixel": round(dt * 1e9 / a.size, 1), "polygons": int(len(ref["poly_label"])),
              "device_ns_per_pixel_full_mask": round(dev_ns, 4)})


def _model_and_raster(side):
    from unet_amd.model import HipDynamicUnet
    torch.manual_seed(0)
    model = HipDynamicUnet("xresnet34", 4, 5, (512, 512), act_dtype="bf16")
    model.eval()
    img = torch.randint(1, 256, (4, side, side), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    return model, img


def predict(side: int, reps: int):
    import predict as P
    model, img = _model_and_raster(side)
    times = {"none": [], "vector": []}
    tm = {}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(reps + 1):
            for name, arg in (("none", None), ("vector", os.path.join(tmp, "v.geojson"))):
                tm = {} if arg is not None else tm
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                P.predict_raster(model, img, 512, 0.2, batch_size=16, vector_path=arg, timing=tm if arg is not None else None)
                torch.cuda.synchronize()
                if r:
                    times[name].append(round(time.perf_counter() - t0, 4))
    emit({"what": f"predict_raster end to end, xresnet34 4->5 bf16, {side} x {side}, 512 px windows, overlap 0.2, batch 16 (random raster, untrained "
                  "model: the mask is a few very large regions)", "seconds_none": times["none"], "seconds_vector": times["vector"],
          "vector_seconds_last": round(tm.get("vector_seconds", float("nan")), 4), "vector_polygons": tm.get("vector_polygons"),
          "vector_vertices": tm.get("vector_vertices")})


def tree(root: str, side: int, reps: int):
    import predict as P
    assert os.path.samefile(os.path.dirname(os.path.abspath(P.__file__)), root), P.__file__
    model, img = _model_and_raster(side)
    secs, sha = [], None
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = P.predict_raster(model, img, 512, 0.2, batch_size=16)
        torch.cuda.synchronize()
        if r:
            secs.append(round(time.perf_counter() - t0, 4))
        sha = hashlib.sha1(np.ascontiguousarray(out).tobytes()).hexdigest()
    print(json.dumps({"tree": root, "side": side, "seconds": secs, "best": min(secs), "mask_sha1": sha}), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "tree":
        tree(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 20000, int(sys.argv[4]) if len(sys.argv) > 4 else 3)
        sys.exit(0)
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    if mode in ("kernels", "all"):
        kernels(side, reps)
    if mode in ("predict", "all"):
        predict(side, reps)
    from unet_amd.build import source_hash
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": RESULTS, "kernel_source_hash": source_hash(),
                   "command": "python scripts/vectorize_bench.py " + " ".join(sys.argv[1:])}, f, indent=1)
        f.write("\n")
