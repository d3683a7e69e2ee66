"""Non-rigid augmentation at cfg2 (batch 16 of 4 x 512 x 512 tiles, xresnet34, 5 classes).
usage: python scripts/field_aug_bench.py [kernels|fit|both] [reps=3] [--out profiles/field_aug_bench.json]
One JSON line per measurement on stdout, and all of them as a list in the --out file.
  kernels  unet_warp_field (dense, grid, optical; bilinear, reflect-101, all 16 images fired) next to unet_warp_affine (bilinear,
           reflect-101) on the same batch in the same run, alternated: device-event time per pass over the batch, the bytes it must move
           (one read + one write of the images, plus 8 bytes per pixel of field for the dense kind) and each kind's ratio to the affine
           warp; then unet_elastic_field at sigma = 6 (49 taps) and sigma = 50 (401 taps) with its FMAs per second
  fit      Learner.fit_one_cycle over .npy tile files with the default flips, with Rotate + ShiftScaleRotate behind them, and with
           ElasticTransform(alpha=120, sigma=6) + GridDistortion + OpticalDistortion behind them (all p = 0.5, n_transform_imgs = 0.5),
           alternated `reps` times in one process, in fp32 and in bf16 storage: tiles/s of each run and the ratios to flips only.  512 + 16
           tiles, so that a bf16 run lasts over a second: with 64 tiles it lasts 0.14 s and the three repeats of one pipeline spread by 23 %"""
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
RESULTS = []


def emit(rec):
    RESULTS.append(rec)
    print(json.dumps(rec), flush=True)


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


def kernels(reps=3):
    from unet_amd import augment as A
    from unet_amd import ops
    g = np.random.default_rng(0)
    x = torch.from_numpy(g.random((B, N_IN, S, S), dtype=np.float32)).cuda()
    out = torch.empty_like(x)
    image_bytes = 2 * x.numel() * 4
    fired = [True] * B
    maps = np.stack([A.inverse_map(A.ShiftScaleRotate().matrix(A.ShiftScaleRotate().get_params(g, S, S), S, S)) for _ in range(B)])
    et = A.ElasticTransform(alpha=120, sigma=6)
    field = et.field_params([et.get_params(g, S, S) for _ in range(B)], S, S, x.device)
    gd, od = A.GridDistortion(), A.OpticalDistortion()
    grid = gd.field_params([gd.get_params(g, S, S) for _ in range(B)], S, S, x.device)
    optical = od.field_params([od.get_params(g, S, S) for _ in range(B)], S, S, x.device)
    runs = {"unet_warp_affine": lambda: ops.warp_affine(x, out, maps, 1, 4, 0.0),
            "unet_warp_field dense": lambda: ops.warp_field(x, out, "dense", field, fired, None, 1, 4, 0.0),
            "unet_warp_field grid": lambda: ops.warp_field(x, out, "grid", grid, fired, None, 1, 4, 0.0),
            "unet_warp_field optical": lambda: ops.warp_field(x, out, "optical", optical, fired, None, 1, 4, 0.0)}
    us = {k: [] for k in runs}
    for _ in range(reps):                              # alternated: every kernel sees the same neighbours on the machine
        for k, f in runs.items():
            us[k].append(_time(f))
    med = {k: float(np.median(v)) for k, v in us.items()}
    for k in runs:
        nbytes = image_bytes + (field.numel() * 4 if "dense" in k else 0)
        emit({"what": f"{k}, cfg2, 16 of 16 images, bilinear, reflect-101", "us_per_batch": [round(v, 2) for v in us[k]],
              "median_us": round(med[k], 2), "MB_moved": round(nbytes / 1e6, 1), "GB_per_s": round(nbytes / med[k] / 1e3, 1),
              "ratio_to_warp_affine": round(med[k] / med["unet_warp_affine"], 3)})
    ws = torch.empty_like(field)
    for sigma in (6, 50):
        t = A.ElasticTransform(alpha=120, sigma=sigma)
        keys = g.integers(0, 2 ** 32, (B, 2))
        v = [_time(lambda: ops.elastic_field(field, ws, keys, t.alpha, fired, False, t.taps), iters=20, warm=3) for _ in range(reps)]
        fma = 2 * field.numel() * t.ksize
        emit({"what": f"unet_elastic_field, 16 x 2 x 512 x 512, sigma = {sigma}, {t.ksize} taps (row pass + column pass)",
              "us_per_batch": [round(u, 2) for u in v], "median_us": round(float(np.median(v)), 2),
              "GFMA_per_s": round(fma / float(np.median(v)) / 1e3, 1), "MB_written_and_read": round(3 * field.numel() * 4 / 1e6, 1)})


def fit(reps=3, n_train=512, n_valid=16):
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
    flips = lambda: [A.HorizontalFlip(p=0.5), A.VerticalFlip(p=0.5)]
    pipes = {"flips": lambda: A.Compose(flips()),
             "affine": lambda: A.Compose(flips() + [A.Rotate(p=0.5), A.ShiftScaleRotate(p=0.5)]),
             "field": lambda: A.Compose(flips() + [A.ElasticTransform(alpha=120, sigma=6, p=0.5), A.GridDistortion(p=0.5),
                                                   A.OpticalDistortion(p=0.5)])}
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
        med = {k: float(np.median(v)) for k, v in runs.items()}
        spread = {k: round((max(v) - min(v)) / max(v), 4) for k, v in runs.items()}
        emit({"what": "fit_one_cycle(1) over files, train tiles/s (incl. validation)", "dtype": dtype, **runs, "median": med, "spread": spread,
              "affine_over_flips": round(med["affine"] / med["flips"], 4), "field_over_flips": round(med["field"] / med["flips"], 4)})
        del model
        torch.cuda.empty_cache()
    tmp.cleanup()


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "field_aug_bench.json")
    if "--out" in args:
        out = args[args.index("--out") + 1]
        del args[args.index("--out"):args.index("--out") + 2]
    mode = args[0] if args else "both"
    k = int(args[1]) if len(args) > 1 else 3
    if not torch.cuda.is_available():
        raise SystemExit("field_aug_bench: no GPU (the measurement has no CPU fallback)")
    if mode in ("kernels", "both"):
        kernels(k)
    if mode in ("fit", "both"):
        fit(k)
    from unet_amd.build import source_hash
    with open(out, "w") as fh:
        json.dump({"source_hash": source_hash(), "device": torch.cuda.get_device_name(0), "results": RESULTS}, fh, indent=1)
        fh.write("\n")
