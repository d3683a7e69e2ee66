"""Geometric augmentation at cfg2 (batch 16 of 4 x 512 x 512 tiles, xresnet34, 5 classes).
usage: python scripts/aug_bench.py [warp|fit|both|profile] [reps=3]   -- one JSON line per measurement on stdout
  warp     unet_warp_affine (bilinear, reflect-101) + unet_warp_affine_mask (int64) over the whole batch, all 16 images with a
           shift-scale-rotate map: device-event time per image + mask pair and the bytes it moves
  fit      Learner.fit_one_cycle over .npy tile files with the default flips and with flips + RandomRotate90 + ShiftScaleRotate (both
           n_transform_imgs = 0.5), alternated `reps` times in one process, in fp32 and in bf16 storage: tiles/s of each run
  profile  the warp pairs only (what a `rocprofv3 --kernel-trace --stats` run wraps)"""
import json
import math
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, N_IN, C, S = 16, 4, 5, 512


def warp(iters=50):
    from unet_amd import augment as A
    from unet_amd import ops
    g = np.random.default_rng(0)
    x = torch.from_numpy(g.random((B, N_IN, S, S), dtype=np.float32)).cuda()
    y = torch.from_numpy(g.integers(0, C, (B, S, S))).cuda()
    t = A.ShiftScaleRotate(p=1.0)
    maps = np.stack([A.inverse_map(t.matrix(t.get_params(g, S, S), S, S)) for _ in range(B)])
    xo, yo = torch.empty_like(x), torch.empty_like(y)
    pair = lambda: (ops.warp_affine(x, xo, maps, 1, 4, 0.0), ops.warp_affine_mask(y, yo, maps, 4, 0))
    for _ in range(5):
        pair()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(iters):
        pair()
    ev[1].record()
    torch.cuda.synchronize()
    us = 1e3 * ev[0].elapsed_time(ev[1]) / iters
    nbytes = 2 * (x.numel() * 4 + y.numel() * 8)
    print(json.dumps({"what": "warp image + mask launches, cfg2, 16 of 16 images fired", "us_per_pair": round(us, 2),
                      "MB_moved": round(nbytes / 1e6, 1), "TB_per_s": round(nbytes / us / 1e6, 2)}), flush=True)


def fit(reps=3, n_train=64, n_valid=16):
    from unet_amd import augment as A
    from unet_amd.learner import CrossEntropyLossFlat, DataLoaders, Learner, TileDataset
    from unet_amd.model import HipDynamicUnet
    g = np.random.default_rng(1)
    tmp = tempfile.TemporaryDirectory()
    pi, pm = [], []
    for i in range(n_train + n_valid):
        np.save(os.path.join(tmp.name, f"i{i}.npy"), g.integers(0, 256, (N_IN, S, S)).astype(np.uint8))
        np.save(os.path.join(tmp.name, f"m{i}.npy"), g.integers(0, C, (S, S)).astype(np.uint8))
        pi.append(os.path.join(tmp.name, f"i{i}.npy"))
        pm.append(os.path.join(tmp.name, f"m{i}.npy"))
    pipes = {"flips": lambda: A.default_pipeline(),
             "rotate": lambda: A.Compose([A.HorizontalFlip(p=0.5), A.VerticalFlip(p=0.5), A.RandomRotate90(p=0.5), A.ShiftScaleRotate(p=0.5)])}
    for dtype in ("f32", "bf16"):
        torch.manual_seed(0)
        model = HipDynamicUnet("xresnet34", N_IN, C, (S, S), act_dtype=dtype)
        runs = {k: [] for k in pipes}
        for r in range(reps + 1):                  # run 0 of each pipeline warms up (kernel selection, staging ring, graphs)
            for name, mk in pipes.items():
                dls = DataLoaders(TileDataset(pi[:n_train], pm[:n_train], "int8"), TileDataset(pi[n_train:], pm[n_train:], "int8"), B,
                                  vocab=list("abcde"), seed=r, train_tfm=A.BatchAugment(mk(), n_transform_imgs=0.5, seed=r))
                learn = Learner(dls, model, loss_func=CrossEntropyLossFlat(axis=1), path=tmp.name)
                learn._no_logging = True
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                learn.fit_one_cycle(1, lr_max=1e-4)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert all(math.isfinite(v) for v in learn.recorder.losses)
                if r:
                    runs[name].append(round(n_train / dt, 2))
        best = {k: max(v) for k, v in runs.items()}
        spread = {k: round((max(v) - min(v)) / max(v), 4) for k, v in runs.items()}
        print(json.dumps({"what": "fit_one_cycle(1) over files, train tiles/s (incl. validation)", "dtype": dtype, **runs,
                          "spread": spread, "rotate_over_flips": round(best["rotate"] / best["flips"], 4)}), flush=True)
        del model
        torch.cuda.empty_cache()
    tmp.cleanup()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "both"
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    if mode in ("warp", "both"):
        warp()
    if mode in ("fit", "both"):
        fit(k)
    if mode == "profile":
        warp(iters=20)
