"""Pixel-level augmentation at cfg2 (batch 16 of 4 x 512 x 512 tiles, xresnet34, 5 classes).
usage: python scripts/pixel_aug_bench.py [kernels|fit|both] [reps=3]   -- one JSON line per measurement on stdout
  kernels  unet_pixel_ops with a full program (8 ops, every opcode) on all 16 images, and unet_blur_separable at k = 7 and k = 31:
           device-event time per pass over the batch, the bytes it moves (one read + one write) and the rate, also as a fraction of
           the 4.5 TB/s the streaming kernels of the step reach
  fit      Learner.fit_one_cycle over .npy tile files with the default flips, with RandomBrightnessContrast + CoarseDropout and with the
           full pixel pipeline (all n_transform_imgs = 0.5), alternated `reps` times in one process, in fp32 and in bf16 storage: tiles/s
           of each run.  On a checkout without the new transforms the full pipeline is left out: that run is the baseline."""
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
HBM_STREAM = 4.5e12


def _time(f, iters=50, warm=10):
    for _ in range(warm):
        f()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(iters):
        f()
    ev[1].record()
    torch.cuda.synchronize()
    return 1e3 * ev[0].elapsed_time(ev[1]) / iters


def kernels():
    from unet_amd import augment as A
    from unet_amd import ops
    g = np.random.default_rng(0)
    x = torch.from_numpy(g.random((B, N_IN, S, S), dtype=np.float32)).cuda()
    nbytes = 2 * x.numel() * 4
    cd = A.CoarseDropout()
    full = {i: [("bc", 1.1, 0.05), ("gamma", 0.9), ("noise", 11 + i, 7, 0.0, 0.02, True), cd.program(cd.get_params(g, S, S), N_IN, S, S)[0],
                ("drop", [i % N_IN], 0.0), ("permute", [int(c) for c in g.permutation(N_IN)]), ("noise", i, 3, 0.0, 0.02, False),
                ("bc", 0.95, 0.0)] for i in range(B)}
    light = {i: [("bc", 1.1, 0.05), full[i][3]] for i in range(B)}
    for name, progs in (("full program: 8 ops, every opcode", full), ("RandomBrightnessContrast + CoarseDropout", light)):
        us = _time(lambda: ops.pixel_ops(x, progs))
        print(json.dumps({"what": f"unet_pixel_ops, cfg2, 16 of 16 images, {name}", "us_per_batch": round(us, 2), "launches": 2,
                          "MB_moved": round(nbytes / 1e6, 1), "GB_per_s": round(nbytes / us / 1e3, 1),
                          "of_4.5_TB_per_s": round(nbytes / us * 1e6 / HBM_STREAM, 3)}), flush=True)
    out = torch.empty_like(x)
    for k in (7, 31):
        taps = [A.gaussian_taps(k, 0.0)] * B
        us = _time(lambda: ops.blur_separable(x, out, taps))
        print(json.dumps({"what": f"unet_blur_separable, cfg2, 16 of 16 images, k = {k}", "us_per_batch": round(us, 2),
                          "MB_moved": round(nbytes / 1e6, 1), "GB_per_s": round(nbytes / us / 1e3, 1),
                          "of_4.5_TB_per_s": round(nbytes / us * 1e6 / HBM_STREAM, 3)}), flush=True)


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
             "rbc_cd": lambda: A.Compose([A.RandomBrightnessContrast(p=0.5), A.CoarseDropout(p=0.5)])}
    if hasattr(A, "GaussNoise"):
        pipes["pixel"] = lambda: A.Compose([A.RandomBrightnessContrast(p=0.5), A.GaussNoise(p=0.5), A.GaussianBlur(p=0.5), A.RandomGamma(p=0.5),
                                            A.CoarseDropout(p=0.5), A.ChannelDropout(p=0.5), A.ChannelShuffle(p=0.5)])
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
        spread = {k: round((max(v) - min(v)) / max(v), 4) for k, v in runs.items()}
        print(json.dumps({"what": "fit_one_cycle(1) over files, train tiles/s (incl. validation)", "dtype": dtype, **runs,
                          "median": {k: float(np.median(v)) for k, v in runs.items()}, "spread": spread}), flush=True)
        del model
        torch.cuda.empty_cache()
    tmp.cleanup()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "both"
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    if mode in ("kernels", "both"):
        kernels()
    if mode in ("fit", "both"):
        fit(k)
