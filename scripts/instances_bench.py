"""Cost of the instance split (unet_amd/instances.py) on the 20000 x 20000 masks of scripts/vectorize_bench.py.
usage: python scripts/instances_bench.py kernels [side=20000] [reps=3]
       python scripts/instances_bench.py tree DIR [side=20000] [reps=3]
       python scripts/instances_bench.py noop LINES
Prints one JSON line per measurement; kernels writes them to profiles/instances_bench.json.
  kernels  the synthetic 5-class mask, raw and after PostProcess(majority=5, sieve=64), classes 1 and 3 split: milliseconds in total (best of
           `reps` after a warm-up, device synchronised) and per stage (runs that synchronise after every stage) at radius 64, min_depth 2;
           the distance stage alone at radius 16, 64 and 255; seeds, segments, rounds; polygonize_labels next to the plain polygonize;
           the host route (scipy.ndimage.distance_transform_edt, then the sequential restatement tests/instances_ref.py) on a 1000 x 1000 crop
  tree     predict_raster with a vector_path and instances=None from the checkout at DIR (this tree or the parent commit's, built), a fresh
           process per call: the seconds of `reps` runs after a warm-up, the SHA-1 of the mask and of the GeoJSON file
  noop     LINES holds the lines of alternated tree calls (parent / this / parent / this): they are added to the JSON file as the no-op
           comparison against the parent commit"""
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

OUT = os.path.join(HERE, "..", "profiles", "instances_bench.json")
RESULTS = []
CLASSES = (1, 3)


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


def one_mask(name, mask, reps):
    from unet_amd import instances as IN
    from unet_amd import ops
    from unet_amd import vectorize as VZ
    n = mask.numel()
    ms, (labels, info) = timed(lambda: IN.split_instances(mask, CLASSES, 64, 2.0), reps)
    stages = None
    for _ in range(reps):
        s = {}
        IN.split_instances(mask, CLASSES, 64, 2.0, stages=s)
        stages = s if stages is None else {k: min(v, stages[k]) for k, v in s.items()}
    emit({"what": f"split_instances(classes={list(CLASSES)}, radius=64, min_depth=2.0), {name}", "mask": f"{mask.shape[0]} x {mask.shape[1]}", "reps": reps,
          "ms": round(ms, 3), "ns_per_pixel": round(ms * 1e6 / n, 3), "stage_ms": {k: round(v, 3) for k, v in stages.items()},
          "merge_ms_per_round": round(stages["merge"] / max(info["rounds"], 1), 3), **info})
    g, keys = torch.empty_like(mask), torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    for R in (16, 64, 255):
        d_ms, _ = timed(lambda: ops.inst_distance(mask, CLASSES, R, g, keys), reps)
        emit({"what": f"capped distance alone (row pass + column pass) at radius {R}, {name}", "ms": round(d_ms, 3), "ns_per_pixel": round(d_ms * 1e6 / n, 4)})
    del g, keys
    torch.cuda.empty_cache()
    plain_ms, plain = timed(lambda: VZ.polygonize(mask), reps)
    rec = {"what": f"polygonize(mask) next to polygonize_labels(mask, instances), {name}", "ms_plain": round(plain_ms, 3), "polygons_plain": plain.n_polygons,
           "vertices_plain": plain.n_vertices}
    del plain
    torch.cuda.empty_cache()
    inst_ms, polys = timed(lambda: VZ.polygonize_labels(mask, labels), reps)
    rec.update(ms_labels=round(inst_ms, 3), polygons_labels=polys.n_polygons, vertices_labels=polys.n_vertices, ratio=round(inst_ms / plain_ms, 3))
    emit(rec)
    ids_ms, (ids, count) = timed(lambda: IN.instance_ids(mask, labels, CLASSES), reps)
    emit({"what": f"instance_ids (root marks, scan, gather), {name}", "ms": round(ids_ms, 3), "instances": count})


def kernels(side: int, reps: int):
    from postprocess_bench import synthetic_mask
    from unet_amd.postprocess import PostProcess
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    import instances_ref as I
    from scipy import ndimage
    mask = synthetic_mask(side)
    clean = PostProcess(majority=5, sieve=64)(mask)
    one_mask("5 classes, smooth regions + 2 % salt", mask, reps)
    torch.cuda.empty_cache()
    one_mask("the same after PostProcess(majority=5, sieve=64)", clean, reps)
    crop = min(side, 1000)
    for name, m in (("raw", mask), ("cleaned", clean)):
        a = m[:crop, :crop].cpu().numpy()
        t0 = time.perf_counter()
        for c in CLASSES:
            ndimage.distance_transform_edt(a == c)
        edt_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, info = I.split(a, CLASSES, 64, 2.0)
        ref_s = time.perf_counter() - t0
        emit({"what": f"host route, {crop} x {crop} crop of the {name} mask: scipy.ndimage.distance_transform_edt per split class, then the sequential "
                      "restatement tests/instances_ref.py (plain Python: an upper bound for a compiled watershed)", "edt_seconds": round(edt_s, 3),
              "edt_ns_per_pixel": round(edt_s * 1e9 / a.size, 1), "restatement_seconds": round(ref_s, 2),
              "restatement_ns_per_pixel": round(ref_s * 1e9 / a.size, 1), **info})


def tree(root: str, side: int, reps: int):
    import predict as P
    assert os.path.samefile(os.path.dirname(os.path.abspath(P.__file__)), root), P.__file__
    from unet_amd.model import HipDynamicUnet
    torch.manual_seed(0)
    model = HipDynamicUnet("xresnet34", 4, 5, (512, 512), act_dtype="bf16")
    model.eval()
    img = torch.randint(1, 256, (4, side, side), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
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
    this = os.path.samefile(root, os.path.join(HERE, ".."))
    print(json.dumps({"tree": "this commit" if this else "parent commit", "side": side, "seconds": secs, "best": min(secs), "mask_sha1": sha,
                      "geojson_sha1": fsha}), flush=True)


def noop(lines_path: str):
    runs = [json.loads(l) for l in open(lines_path) if l.startswith("{")]
    parent = [r["best"] for r in runs if r["tree"] == "parent commit"]
    this = [r["best"] for r in runs if r["tree"] == "this commit"]
    doc = json.load(open(OUT))
    doc["predict_raster_instances_none_vs_parent"] = {
        "what": "predict_raster(vector_path=..., instances=None) end to end, xresnet34 4->5 bf16, random uint8 raster, 512 px windows, overlap 0.2, batch "
                "16: the parent commit's tree and this one alternated (python scripts/instances_bench.py tree DIR), a fresh process each, timed runs "
                "after a warm-up, one machine",
        "runs": runs, "parent_best": parent, "this_best": this, "spread_of_parent_runs": round(max(parent) - min(parent), 4),
        "this_inside_parent_spread": min(parent) <= min(this) <= max(parent), "this_best_not_above_parent_runs": min(this) <= max(parent),
        "this_best_over_parent_best": round(min(this) / min(parent), 4),
        "equal_mask_and_geojson": len({(r["mask_sha1"], r["geojson_sha1"]) for r in runs}) == 1}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["predict_raster_instances_none_vs_parent"]))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if mode == "tree":
        tree(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 20000, int(sys.argv[4]) if len(sys.argv) > 4 else 3)
        sys.exit(0)
    if mode == "noop":
        noop(sys.argv[2])
        sys.exit(0)
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    kernels(side, reps)
    from unet_amd.build import source_hash
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": RESULTS, "kernel_source_hash": source_hash(),
                   "command": "python scripts/instances_bench.py " + " ".join(sys.argv[1:])}, f, indent=1)
        f.write("\n")
