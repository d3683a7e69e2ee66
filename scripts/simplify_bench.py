"""Cost of the ring simplification (unet_amd/vectorize.py) on the 20000 x 20000 masks of scripts/vectorize_bench.py.
usage: python scripts/simplify_bench.py [kernels|predict|all] [side=20000] [reps=3]
       python scripts/simplify_bench.py tree DIR [side=20000] [reps=3]
Prints one JSON line per measurement; kernels / predict / all write them to profiles/simplify_bench.json.
  kernels  the synthetic 5-class mask, raw and after PostProcess(majority=5, sieve=64), at tolerances 0.5, 1 and 2 pixels: vertices before
           and after, polygons dropped, Douglas-Peucker rounds, milliseconds in total (best of `reps` after a warm-up, device synchronised)
           next to polygonize without a tolerance in the same process, milliseconds per stage (runs that synchronise after every stage),
           bytes copied to the host, seconds and size of write_geojson; the host baseline tests/simplify_ref.py on 1000 x 1000 crops
  predict  BASELINE configs[4] end to end on a side x side raster with a vector_path: vector_simplify None against 1.0, alternated
  tree     predict_raster with a vector_path and no tolerance from the checkout at DIR (this tree or another commit's, built), a fresh
           process per call: the seconds of `reps` runs after a warm-up, the SHA-1 of the mask and of the GeoJSON file"""
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

OUT = os.path.join(HERE, "..", "profiles", "simplify_bench.json")
RESULTS = []
TOLERANCES = (0.5, 1.0, 2.0)
ARRAYS = ("xy", "ring_start", "ring_label", "ring_area", "poly_label", "poly_class", "poly_pixels", "poly_ring_start", "poly_rings")
GT = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)


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


def one_mask(name, mask, reps, tmp):
    from unet_amd import vectorize as VZ
    plain_ms, plain = timed(lambda: VZ.polygonize(mask), reps)
    emit({"what": f"polygonize without a tolerance, {name}", "mask": f"{mask.shape[0]} x {mask.shape[1]}", "ms": round(plain_ms, 3),
          "edges": plain.edges, "polygons": plain.n_polygons, "vertices": plain.n_vertices})
    n_plain = plain.n_polygons
    del plain
    for tol in TOLERANCES:
        torch.cuda.empty_cache()
        ms, polys = timed(lambda: VZ.polygonize(mask, simplify=tol), reps)
        stages = None
        for _ in range(reps):
            s = {}
            VZ.polygonize(mask, simplify=tol, stages=s)
            stages = s if stages is None else {k: min(v, stages[k]) for k, v in s.items()}
        simp = sum(v for k, v in stages.items() if k.startswith("simp_"))
        t0 = time.perf_counter()
        host = polys.cpu()
        torch.cuda.synchronize()
        copy_s = time.perf_counter() - t0
        nbytes = sum(getattr(host, k).numel() * getattr(host, k).element_size() for k in ARRAYS)
        rec = {"what": f"polygonize(simplify={tol}), {name}", "reps": reps, "vertices_before": polys.raw_vertices, "candidates": polys.candidates,
               "vertices_after": polys.n_vertices, "polygons": polys.n_polygons, "polygons_dropped": n_plain - polys.n_polygons,
               "rings": polys.n_rings, "rounds": polys.rounds, "ms": round(ms, 3), "ms_without": round(plain_ms, 3),
               "ratio_to_without": round(ms / plain_ms, 3), "simplify_stages_ms": round(simp, 3),
               "simplify_stages_ratio_to_without": round(simp / plain_ms, 3), "stage_ms": {k: round(v, 3) for k, v in stages.items()},
               "bytes_to_host": nbytes, "copy_seconds": round(copy_s, 3)}
        if polys.n_polygons <= 1_000_000:
            path = os.path.join(tmp, "bench.geojson")
            t0 = time.perf_counter()
            feats = VZ.write_geojson(path, host, GT, 32632)
            rec.update(write_geojson_seconds=round(time.perf_counter() - t0, 2), features=feats, geojson_bytes=os.path.getsize(path))
            os.remove(path)
        else:
            rec["write_geojson_seconds"] = "not measured: millions of one-pixel polygons"
        emit(rec)
        del polys, host


def kernels(side: int, reps: int):
    from postprocess_bench import synthetic_mask
    from unet_amd.postprocess import PostProcess
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    import simplify_ref as S
    mask = synthetic_mask(side)
    clean = PostProcess(majority=5, sieve=64)(mask)
    with tempfile.TemporaryDirectory() as tmp:
        one_mask("5 classes, smooth regions + 2 % salt", mask, reps, tmp)
        torch.cuda.empty_cache()
        one_mask("the same after PostProcess(majority=5, sieve=64)", clean, reps, tmp)
    crop = min(side, 1000)
    for name, m in (("raw", mask), ("cleaned", clean)):
        a = m[:crop, :crop].cpu().numpy()
        t0 = time.perf_counter()
        prep = S.prepare(a)
        trace_s = time.perf_counter() - t0
        for tol in TOLERANCES:
            t0 = time.perf_counter()
            ref = S.simplify(a, tol, None, prep)
            dt = time.perf_counter() - t0
            emit({"what": f"host baseline: tests/simplify_ref.py at tolerance {tol}, {crop} x {crop} crop of the {name} mask (after {round(trace_s, 2)} s "
                          "of tracing and candidate lists)", "seconds": round(dt, 2), "candidates": ref["raw_vertices"],
                  "ns_per_candidate": round(dt * 1e9 / max(ref["raw_vertices"], 1), 1), "vertices_after": int(len(ref["xy"])), "depth": ref["depth"]})


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
    times, last = {"none": [], "simplify": []}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(reps + 1):
            for name, tol in (("none", None), ("simplify", 1.0)):
                tm = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                P.predict_raster(model, img, 512, 0.2, batch_size=16, vector_path=os.path.join(tmp, "v.geojson"), vector_simplify=tol, timing=tm)
                torch.cuda.synchronize()
                if r:
                    times[name].append(round(time.perf_counter() - t0, 4))
                last[name] = dict(tm, file_bytes=os.path.getsize(os.path.join(tmp, "v.geojson")))
    pick = lambda d: {k: (round(v, 4) if isinstance(v, float) else v) for k, v in d.items() if k.startswith("vector_") or k == "file_bytes"}  # noqa: E731
    emit({"what": f"predict_raster end to end with a vector_path, xresnet34 4->5 bf16, {side} x {side}, 512 px windows, overlap 0.2, batch 16 (random "
                  "raster, untrained model)", "seconds_simplify_none": times["none"], "seconds_simplify_1.0": times["simplify"],
          "last_none": pick(last["none"]), "last_simplify_1.0": pick(last["simplify"])})


def tree(root: str, side: int, reps: int):
    import predict as P
    assert os.path.samefile(os.path.dirname(os.path.abspath(P.__file__)), root), P.__file__
    model, img = _model_and_raster(side)
    secs, sha, fsha = [], None, None
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "v.geojson")
        for r in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = P.predict_raster(model, img, 512, 0.2, batch_size=16, vector_path=path)
            torch.cuda.synchronize()
            if r:
                secs.append(round(time.perf_counter() - t0, 4))
            sha = hashlib.sha1(np.ascontiguousarray(out).tobytes()).hexdigest()
            fsha = hashlib.sha1(open(path, "rb").read()).hexdigest()
    print(json.dumps({"tree": root, "side": side, "seconds": secs, "best": min(secs), "mask_sha1": sha, "geojson_sha1": fsha}), flush=True)


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
                   "command": "python scripts/simplify_bench.py " + " ".join(sys.argv[1:])}, f, indent=1)
        f.write("\n")
