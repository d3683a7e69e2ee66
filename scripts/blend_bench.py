"""Cost of Gaussian window blending in predict.predict_raster (xresnet34, 4 -> 5 classes, windows of 512, overlap 0.2, batch 16).
usage: python scripts/blend_bench.py [bench|profile] [reps=3]   -- one JSON line per measurement on stdout
  bench    blend "mean" / "gaussian" in fp32 and bf16 storage, alternated `reps` times after one warm-up run each: windows per second
           end to end (mask to the host included) and ratio = gaussian / mean of the best rates
  profile  one fp32 run of each blend after a warm-up of each (what a `rocprofv3 --kernel-trace --stats` run wraps: the weighted and the
           plain accumulate / finalise kernels appear side by side in one stats file)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

N_IN, C, S, H = 4, 5, 512, 4700          # 12 x 12 = 144 windows of 512
BLENDS = ("mean", "gaussian")


def _model(dtype):
    from unet_amd.model import HipDynamicUnet
    torch.manual_seed(0)
    m = HipDynamicUnet("xresnet34", N_IN, C, (S, S), act_dtype=dtype)
    m.eval()
    return m


def _run(model, img, blend):
    import predict as P
    tm = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = P.predict_raster(model, img, S, 0.2, batch_size=16, blend=blend, timing=tm)
    torch.cuda.synchronize()
    return tm["kept_windows"] / (time.perf_counter() - t0), out, tm["kept_windows"]


def _image():
    return torch.from_numpy(np.random.default_rng(0).integers(1, 256, (N_IN, H, H)).astype(np.uint8)).cuda()


def bench(reps=3):
    img = _image()
    for dtype in ("f32", "bf16"):
        model = _model(dtype)
        rates = {b: [] for b in BLENDS}
        masks = {}
        for r in range(reps + 1):
            for b in BLENDS:
                v, out, n = _run(model, img, b)
                masks[b] = out
                if r:
                    rates[b].append(round(v, 2))
        best = {k: max(v) for k, v in rates.items()}
        res = {"what": "predict_raster windows/s end to end, xresnet34 4->5, 512 px windows, overlap 0.2, batch 16", "dtype": dtype,
               "windows": n, "mean": rates["mean"], "gaussian": rates["gaussian"], "ratio": round(best["gaussian"] / best["mean"], 4),
               "spread": {k: round((max(v) - min(v)) / max(v), 4) for k, v in rates.items()},
               "mask_pixels_changed": float(np.mean(masks["mean"] != masks["gaussian"]))}
        print(json.dumps(res), flush=True)
        del model
        torch.cuda.empty_cache()


def profile():
    img = _image()
    model = _model("f32")
    for b in BLENDS:
        _run(model, img, b)
    for b in BLENDS:
        v, _, n = _run(model, img, b)
        print(json.dumps({"what": "profiled fp32 run", "blend": b, "windows": n, "tiles_per_s": round(v, 2)}), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "bench"
    if mode == "bench":
        bench(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    else:
        profile()
