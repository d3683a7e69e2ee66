"""Test-time augmentation cost of predict.predict_raster (xresnet34, 4 -> 5 classes, windows of 512, overlap 0.2, batch 16).
usage: python scripts/tta_bench.py [bench|profile] [reps=3]   -- one JSON line per measurement on stdout
  bench    tta None / "flips" / "d4" in fp32 and bf16 storage, alternated `reps` times after one warm-up run each: tiles/s (windows per
           second end to end, mask to the host included) and ratio = rate / (plain rate / k) -- 1.0 means the k forwards are the whole cost
  profile  one fp32 d4 run after a warm-up (what a `rocprofv3 --kernel-trace --stats` run wraps)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

N_IN, C, S, H = 4, 5, 512, 4700          # 11 x 11 = 121 windows of 512


def _model(dtype):
    from unet_amd.model import HipDynamicUnet
    torch.manual_seed(0)
    m = HipDynamicUnet("xresnet34", N_IN, C, (S, S), act_dtype=dtype)
    m.eval()
    return m


def _run(model, img, tta):
    import predict as P
    tm = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = P.predict_raster(model, img, S, 0.2, batch_size=16, tta=tta, timing=tm)
    torch.cuda.synchronize()
    return tm["kept_windows"] / (time.perf_counter() - t0), out, tm["kept_windows"]


def bench(reps=3):
    img = torch.from_numpy(np.random.default_rng(0).integers(1, 256, (N_IN, H, H)).astype(np.uint8)).cuda()
    for dtype in ("f32", "bf16"):
        model = _model(dtype)
        rates = {None: [], "flips": [], "d4": []}
        for r in range(reps + 1):
            for tta in rates:
                v, _, n = _run(model, img, tta)
                if r:
                    rates[tta].append(round(v, 2))
        best = {k: max(v) for k, v in rates.items()}
        k_of = {None: 1, "flips": 4, "d4": 8}
        res = {"what": "predict_raster windows/s end to end, xresnet34 4->5, 512 px windows, overlap 0.2, batch 16", "dtype": dtype,
               "windows": n, "plain": rates[None], "flips": rates["flips"], "d4": rates["d4"],
               "ratio_flips": round(best["flips"] / (best[None] / 4), 4), "ratio_d4": round(best["d4"] / (best[None] / 8), 4),
               "spread": {str(k): round((max(v) - min(v)) / max(v), 4) for k, v in rates.items()}, "k": {str(k): v for k, v in k_of.items()}}
        print(json.dumps(res), flush=True)
        del model
        torch.cuda.empty_cache()


def profile():
    img = torch.from_numpy(np.random.default_rng(0).integers(1, 256, (N_IN, H, H)).astype(np.uint8)).cuda()
    model = _model("f32")
    _run(model, img, "d4")
    v, _, n = _run(model, img, "d4")
    print(json.dumps({"what": "profiled fp32 d4 run", "windows": n, "tiles_per_s": round(v, 2)}), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "bench"
    if mode == "bench":
        bench(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    else:
        profile()
