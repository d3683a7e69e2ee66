"""The two-object border weight (BorderWeightedCrossEntropy(objects=True), csrc/object_edt.hip) at cfg2 (batch 16 of 4x512x512 tiles,
xresnet34, 5 classes, radius 30 = ceil(6 sigma)), two timings:
  kernels: one call of unet_object_edt with the map fused (keys, three labelling launches, column pass, row pass) on int64 masks of
           three kinds -- blocky classes, 2 % salt on background (the many-objects case), all background -- and beside each, in the same
           process and alternating round by round, the nearest-border map (unet_border_edt + unet_border_weight).  Device events around
           `iters` calls.  Bytes moved are computed from the shapes; their share of the HBM peak (8.0 TB/s) is a share of bandwidth.
  step:    whole training steps (TrainStep, resident batch) with the plain cross-entropy, the nearest-border loss and objects=True,
           interleaved (every loss twice: drift shows as a difference between the two), fp32 and bf16 storage.
usage: python scripts/object_border_bench.py [kernels|step|both] [steps=10] [out.json]   -- one JSON line per measurement on stdout; with
out.json the lines are also collected into that file (profiles/object_border_bench.json is such a file)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, N_IN, C, S = 16, 4, 5, 512
W0, SIGMA, RADIUS = 10.0, 5.0, 30
HBM_PEAK = 8.0e12
RESULTS = []


def emit(d):
    RESULTS.append(d)
    print(json.dumps(d), flush=True)


def masks():
    rng = np.random.default_rng(0)
    small = rng.integers(0, C, size=(B, S // 8, S // 8))
    blocky = np.repeat(np.repeat(small, 8, 1), 8, 2).astype(np.int64)
    salt = np.where(rng.random((B, S, S)) < 0.02, rng.integers(1, C, size=(B, S, S)), 0).astype(np.int64)
    return {"blocky": blocky, "salt2pct": salt, "background": np.zeros((B, S, S), dtype=np.int64)}


def kernels(iters=100, rounds=5):
    from unet_amd import ops
    P = B * S * S
    # bytes per call from the shapes.  objects: keys read the int64 mask and write int32; the labelling reads the keys and writes, merges
    # and flattens the labels (about 4 + 3 * 4); the column pass reads keys and labels three times (summaries, down, up: the repeats are
    # mostly cache hits, counted here all the same) and writes, reads and rewrites 10 bytes of candidates; the row pass reads mask and
    # candidates and writes fp32.  nearest border: as in scripts/border_bench.py
    obj_bytes = P * ((8 + 4) + (4 + 3 * 4) + (3 * 8 + 3 * 10) + (8 + 10 + 4))
    near_bytes = P * (8 + 3 * 2) + P * (2 + 4) + P * (4 + 8 + 4)
    ms = {k: torch.from_numpy(v).cuda() for k, v in masks().items()}
    d2 = torch.empty((B, S, S), dtype=torch.int32, device="cuda")
    pw = torch.empty(P, dtype=torch.float32, device="cuda")
    ws = torch.empty(ops.edt_workspace(B, S, S), dtype=torch.uint8, device="cuda")
    wo = torch.empty(ops.object_edt_workspace(B, S, S), dtype=torch.uint8, device="cuda")
    cw = torch.full((C,), 1.0 / C, device="cuda")

    def nearest(m):
        ops.border_edt(m, d2, ws, None)
        ops.border_weight(d2, m, cw, C, W0, SIGMA, pw)

    fns = {"objects": lambda m: ops.object_border_weight(m, cw, C, W0, SIGMA, pw, wo, 0, None, RADIUS), "nearest": nearest}
    times = {(k, f): [] for k in ms for f in fns}
    for m in ms.values():
        for f in fns.values():
            for _ in range(5):
                f(m)
    torch.cuda.synchronize()
    ops.postprocess_counters(wo[wo.numel() - 16:].view(torch.int32))          # the labelling did not give up
    for _ in range(rounds):
        for k, m in ms.items():
            for name, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    f(m)
                e1.record()
                torch.cuda.synchronize()
                times[(k, name)].append(1e3 * e0.elapsed_time(e1) / iters)
    out = {}
    for (k, name), t in times.items():
        us = statistics.median(t)
        nbytes = obj_bytes if name == "objects" else near_bytes
        out[f"{name}_{k}"] = {"us": round(us, 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2), "bytes": nbytes,
                              "share_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)}
    emit({"what": "weight map of 16 x 512^2 int64 masks per call: objects=True (7 launches, radius 30) beside the nearest-border map (3 launches)",
          "iters": iters, "rounds": rounds, **out,
          "objects_over_nearest": {k: round(out[f"objects_{k}"]["us"] / out[f"nearest_{k}"]["us"], 3) for k in ms}})


def steps(n_steps=10, warmup=3, dtypes=("f32", "bf16"), names=("ce", "border", "objects", "ce2", "border2", "objects2")):
    from unet_amd.learner import BorderWeightedCrossEntropy
    from unet_amd.model import HipDynamicUnet
    from unet_amd.optimizer import FlatAdam
    from unet_amd.trainer import TrainStep
    g = torch.Generator().manual_seed(1234)
    x = (torch.randint(0, 256, (B, N_IN, S, S), generator=g).float() / 255).cuda()
    y = torch.from_numpy(masks()["blocky"]).cuda()
    losses = {"ce": None, "border": BorderWeightedCrossEntropy(w0=W0, sigma=SIGMA),
              "objects": BorderWeightedCrossEntropy(w0=W0, sigma=SIGMA, objects=True, radius=RADIUS)}
    for dtype in dtypes:
        torch.manual_seed(0)
        model = HipDynamicUnet("xresnet34", N_IN, C, (S, S), act_dtype=dtype)
        model.train()
        opt = FlatAdam(model, [1e-5, 1e-4 / 10 ** 0.5, 1e-4])
        step = TrainStep(model, opt, torch.full((C,), 1.0 / C, device="cuda"), 1)
        res = {}
        for name in names:
            step.border = losses[name.rstrip("2")]
            for _ in range(warmup):
                step(x, y)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                loss = step(x, y)
            torch.cuda.synchronize()
            res[name] = round(B * n_steps / (time.perf_counter() - t0), 2)
            assert torch.isfinite(loss).all()
        best = {k: max(res[k], res.get(k + "2", 0)) for k in losses}
        emit({"what": "train step tiles/s, blocky masks", "dtype": dtype, "steps": n_steps, **res,
              "objects_over_ce": round(best["objects"] / best["ce"], 4), "objects_over_border": round(best["objects"] / best["border"], 4),
              "border_over_ce": round(best["border"] / best["ce"], 4)})
        del model, opt, step
        torch.cuda.empty_cache()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "both"
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    if not torch.cuda.is_available():
        raise SystemExit("object_border_bench.py measures on the GPU: none is visible")
    if mode in ("kernels", "both"):
        kernels()
    if mode in ("step", "both"):
        steps(k)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump(RESULTS, f, indent=1)
            f.write("\n")
