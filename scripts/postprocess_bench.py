"""Cost of the class-mask post-processing (unet_amd/postprocess.py) on a 20000 x 20000 mask, and of predict_raster with it.
usage: python scripts/postprocess_bench.py [kernels|predict|all] [side=20000] [reps=3]
Prints one JSON line per measurement and writes them all to profiles/postprocess_bench.json.
  kernels  fixed-seed synthetic 5-class mask made on the device (smooth regions + 2 % salt noise): milliseconds (best of `reps` after one
           warm-up, device synchronised) for labelling at connectivity 4 and 8, sizes, majority k = 5, and the sieve at min_pixels = 64 with
           its round count; label + sizes of a constant mask (one component: the worst case of the atomics) and of one-pixel concentric
           rings (long chains across tiles); the host baseline scipy.ndimage.label per class + bincount on a 4000 x 4000 crop, as ns per pixel next to the
           device's
  predict  BASELINE configs[4] (xresnet34 4 -> 5, bf16 storage, 512 px windows, overlap 0.2, batch 16) on a side x side raster end to end,
           postprocess=None against PostProcess(majority=5, sieve=64), alternated"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "postprocess_bench.json")
RESULTS = []


def emit(rec):
    RESULTS.append(rec)
    print(json.dumps(rec), flush=True)


def synthetic_mask(side: int, classes: int = 5, salt: float = 0.02, seed: int = 0) -> torch.Tensor:
    """uint8 [side, side] on the device: the argmax of `classes` smooth random fields (coarse noise upsampled bilinearly: regions of a
    few hundred pixels across) with `salt` of the pixels redrawn at random"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    coarse = torch.rand((1, classes, side // 128 + 2, side // 128 + 2), device="cuda", generator=g)
    best = torch.full((side, side), -1.0, device="cuda")
    mask = torch.zeros((side, side), dtype=torch.uint8, device="cuda")
    for c in range(classes):          # one class plane at a time: 1.6 GB each at 20000 x 20000
        f = torch.nn.functional.interpolate(coarse[:, c:c + 1], size=(side, side), mode="bilinear", align_corners=False)[0, 0]
        mask = torch.where(f > best, torch.full_like(mask, c), mask)
        best = torch.maximum(best, f)
        del f
    del best
    rows = 2000
    for y in range(0, side, rows):
        n = min(rows, side - y)
        hit = torch.rand((n, side), device="cuda", generator=g) < salt
        rnd = torch.randint(0, classes, (n, side), device="cuda", generator=g, dtype=torch.uint8)
        mask[y:y + n] = torch.where(hit, rnd, mask[y:y + n])
    return mask


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


def kernels(side: int, reps: int):
    from unet_amd import ops
    from unet_amd import postprocess as PP
    mask = synthetic_mask(side)
    n = side * side
    labels = torch.empty((side, side), dtype=torch.int32, device="cuda")
    sizes = torch.empty_like(labels)
    counters = torch.empty(4, dtype=torch.int32, device="cuda")
    out = torch.empty_like(mask)
    base = {"mask": f"{side} x {side}, 5 classes, smooth regions + 2 % salt", "reps": reps}

    def label(conn):
        ops.cc_label(mask, conn, labels, counters)
        ops.postprocess_counters(counters)

    dev_label_ns = None
    for conn in (4, 8):
        ms, _ = timed(lambda: label(conn), reps)
        emit(dict(base, what=f"label connectivity {conn}", ms=round(ms, 3), ns_per_pixel=round(ms * 1e6 / n, 4),
                  components=int((labels.view(-1) == torch.arange(n, device="cuda", dtype=torch.int32)).sum())))
        if conn == 4:
            dev_label_ns = ms * 1e6 / n
    label(4)
    ms_sizes, _ = timed(lambda: ops.cc_sizes(labels, sizes), reps)
    emit(dict(base, what="sizes", ms=round(ms_sizes, 3), ns_per_pixel=round(ms_sizes * 1e6 / n, 4)))
    ms, _ = timed(lambda: ops.majority_filter(mask, out, 5), reps)
    emit(dict(base, what="majority k=5", ms=round(ms, 3), ns_per_pixel=round(ms * 1e6 / n, 4)))
    flat = torch.full_like(mask, 2)          # one component of side^2 pixels: every size add goes to one address, every union to one root
    ms_l, _ = timed(lambda: (ops.cc_label(flat, 4, labels, counters), ops.postprocess_counters(counters)), reps)
    ms_s, _ = timed(lambda: ops.cc_sizes(labels, sizes), reps)
    assert int(sizes[0, 0]) == n
    emit({"what": "constant mask (one component): label connectivity 4 / sizes", "mask": f"{side} x {side}", "label_ms": round(ms_l, 3), "sizes_ms": round(ms_s, 3)})
    del flat
    idx = torch.arange(side, device="cuda", dtype=torch.int32)
    edge = torch.minimum(idx, side - 1 - idx)
    rings = (torch.minimum(edge[:, None], edge[None, :]) & 1).to(torch.uint8)          # one-pixel concentric rings: each crosses every tile on its way round
    ms_r, _ = timed(lambda: (ops.cc_label(rings, 4, labels, counters), ops.postprocess_counters(counters)), reps)
    emit({"what": "one-pixel concentric rings (side / 2 components that each cross thousands of tiles): label connectivity 4", "mask": f"{side} x {side}",
          "label_ms": round(ms_r, 3), "components": int((labels.view(-1) == torch.arange(n, device="cuda", dtype=torch.int32)).sum())})
    del labels, sizes, out, rings, edge
    torch.cuda.empty_cache()
    ms, res = timed(lambda: PP.sieve(mask, 64), reps)
    emit(dict(base, what="sieve min_pixels=64 connectivity 4", ms=round(ms, 3), ns_per_pixel=round(ms * 1e6 / n, 4), info=res[1]))
    ms, res = timed(lambda: PP.PostProcess(majority=5, sieve=64).run(mask), reps)
    emit(dict(base, what="PostProcess(majority=5, sieve=64)", ms=round(ms, 3), ns_per_pixel=round(ms * 1e6 / n, 4), info=res[1]))
    try:
        from scipy import ndimage
    except ImportError:
        emit({"what": "host baseline", "note": "scipy is not installed: not measured"})
        return
    crop = mask[:4000, :4000].cpu().numpy()
    t0 = time.perf_counter()
    for c in range(5):
        lab, k = ndimage.label(crop == c)
        np.bincount(lab.ravel(), minlength=k + 1)
    dt = time.perf_counter() - t0
    emit({"what": "host baseline: scipy.ndimage.label per class + bincount, 4000 x 4000 crop", "seconds": round(dt, 3),
          "ns_per_pixel": round(dt * 1e9 / crop.size, 3), "device_label_plus_sizes_ns_per_pixel": round(dev_label_ns + ms_sizes * 1e6 / n, 4)})


def predict(side: int, reps: int):
    import predict as P
    from unet_amd.model import HipDynamicUnet
    from unet_amd.postprocess import PostProcess
    torch.manual_seed(0)
    model = HipDynamicUnet("xresnet34", 4, 5, (512, 512), act_dtype="bf16")
    model.eval()
    img = torch.randint(1, 256, (4, side, side), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    pp = PostProcess(majority=5, sieve=64)
    times = {"none": [], "postprocess": []}
    tm = {}
    for r in range(reps + 1):
        for name, arg in (("none", None), ("postprocess", pp)):
            tm = {} if arg is None else tm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P.predict_raster(model, img, 512, 0.2, batch_size=16, postprocess=arg, timing=tm if arg is not None else None)
            torch.cuda.synchronize()
            if r:
                times[name].append(round(time.perf_counter() - t0, 4))
    emit({"what": f"predict_raster end to end, xresnet34 4->5 bf16, {side} x {side}, 512 px windows, overlap 0.2, batch 16 (random raster, untrained "
                  "model: the mask is a few very large regions)", "seconds_none": times["none"], "seconds_postprocess": times["postprocess"],
          "postprocess_seconds_last": round(tm.get("postprocess_seconds", float("nan")), 4), "info": tm.get("postprocess")})


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    side = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    if mode in ("kernels", "all"):
        kernels(side, reps)
    if mode in ("predict", "all"):
        predict(side, reps)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": RESULTS}, f, indent=1)
        f.write("\n")
