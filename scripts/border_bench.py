"""Border-weighted cross-entropy at cfg2 (batch 16 of 4x512x512 tiles, xresnet34, 5 classes), two timings:
  kernels: the border distance (unet_border_edt: column pass + row pass) and the weight map (unet_border_weight) on int64 masks of three
           kinds -- blocky classes, salt noise, a single border in one corner (the farthest search) -- device events around `iters`
           calls, the three inputs alternating round by round.  Bytes moved are computed from the shapes; their share of the HBM peak
           (8.0 TB/s) is a share of bandwidth, not of anything the kernels compute.
  step:    whole training steps (TrainStep, resident batch) with BorderWeightedCrossEntropy against CrossEntropyLossFlat, interleaved,
           fp32 and bf16 storage.
usage: python scripts/border_bench.py [kernels|step|both] [steps=10] [out.json]   -- one JSON line per measurement on stdout; with
out.json the lines are also collected into that file"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, N_IN, C, S = 16, 4, 5, 512
W0, SIGMA = 10.0, 5.0
HBM_PEAK = 8.0e12
RESULTS = []


def emit(d):
    RESULTS.append(d)
    print(json.dumps(d), flush=True)


def masks():
    rng = np.random.default_rng(0)
    small = rng.integers(0, C, size=(B, S // 8, S // 8))
    blocky = np.repeat(np.repeat(small, 8, 1), 8, 2).astype(np.int64)
    salt = rng.integers(0, C, size=(B, S, S)).astype(np.int64)
    corner = np.zeros((B, S, S), dtype=np.int64)
    corner[:, 0, 0] = 1
    return {"blocky": blocky, "salt": salt, "corner": corner}


def kernels(iters=100, rounds=5):
    from unet_amd import ops
    P = B * S * S
    # bytes per call from the shapes: the column pass reads the int64 mask once (neighbours come from the cache) and writes, reads and
    # rewrites the uint16 intermediate; the row pass reads it and writes int32; the weight map reads int32 + int64 and writes fp32
    edt_bytes = P * (8 + 3 * 2) + P * (2 + 4)
    weight_bytes = P * (4 + 8 + 4)
    ms = {k: torch.from_numpy(v).cuda() for k, v in masks().items()}
    d2 = torch.empty((B, S, S), dtype=torch.int32, device="cuda")
    pw = torch.empty(P, dtype=torch.float32, device="cuda")
    ws = torch.empty(ops.edt_workspace(B, S, S), dtype=torch.uint8, device="cuda")
    cw = torch.full((C,), 1.0 / C, device="cuda")
    fns = {"edt": lambda m: ops.border_edt(m, d2, ws, None), "weight": lambda m: ops.border_weight(d2, m, cw, C, W0, SIGMA, pw)}
    times = {(k, f): [] for k in ms for f in fns}
    for k, m in ms.items():
        for f in fns.values():
            for _ in range(5):
                f(m)
    torch.cuda.synchronize()
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
        nbytes = edt_bytes if name == "edt" else weight_bytes
        out[f"{name}_{k}"] = {"us": round(us, 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2), "bytes": nbytes,
                              "share_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)}
    tot = {k: out[f"edt_{k}"]["us"] + out[f"weight_{k}"]["us"] for k in ms}
    emit({"what": "border distance (2 launches) and weight map (1 launch), 16 x 512^2 int64 masks", "iters": iters, "rounds": rounds, **out,
          "edt_plus_weight_us": {k: round(v, 2) for k, v in tot.items()}, "corner_over_blocky": round(tot["corner"] / tot["blocky"], 3),
          "salt_over_blocky": round(tot["salt"] / tot["blocky"], 3)})


def steps(n_steps=10, warmup=3, dtypes=("f32", "bf16"), names=("ce", "border", "ce2", "border2")):
    from unet_amd.learner import BorderWeightedCrossEntropy
    from unet_amd.model import HipDynamicUnet
    from unet_amd.optimizer import FlatAdam
    from unet_amd.trainer import TrainStep
    g = torch.Generator().manual_seed(1234)
    x = (torch.randint(0, 256, (B, N_IN, S, S), generator=g).float() / 255).cuda()
    y = torch.from_numpy(masks()["blocky"]).cuda()
    for dtype in dtypes:
        torch.manual_seed(0)
        model = HipDynamicUnet("xresnet34", N_IN, C, (S, S), act_dtype=dtype)
        model.train()
        opt = FlatAdam(model, [1e-5, 1e-4 / 10 ** 0.5, 1e-4])
        step = TrainStep(model, opt, torch.full((C,), 1.0 / C, device="cuda"), 1)
        res = {}
        for name in names:          # interleaved: drift shows as ce != ce2
            step.border = BorderWeightedCrossEntropy(w0=W0, sigma=SIGMA) if name.startswith("border") else None
            for _ in range(warmup):
                step(x, y)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                loss = step(x, y)
            torch.cuda.synchronize()
            res[name] = round(B * n_steps / (time.perf_counter() - t0), 2)
            assert torch.isfinite(loss).all()
        ratio = {"border_over_ce": round(max(res["border"], res.get("border2", 0)) / max(res["ce"], res.get("ce2", 0)), 4)}
        emit({"what": "train step tiles/s, blocky masks", "dtype": dtype, **res, **ratio})
        del model, opt, step
        torch.cuda.empty_cache()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "both"
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    if not torch.cuda.is_available():
        raise SystemExit("border_bench.py measures on the GPU: none is visible")
    if mode in ("kernels", "both"):
        kernels()
    if mode in ("step", "both"):
        steps(k)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump(RESULTS, f, indent=1)
            f.write("\n")
