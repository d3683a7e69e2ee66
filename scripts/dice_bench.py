"""DiceLoss against the cross-entropy at cfg2 (batch 16 of 4x512x512 tiles, xresnet34, 5 classes): the loss kernel pairs alone (forward +
backward on the logits slice, fp32 and bf16 gradient) and whole training steps (TrainStep, resident batch) with each loss.
usage: python scripts/dice_bench.py [loss|step|both|profile] [steps=10]   -- one JSON line per measurement on stdout
profile: the loss pairs, then fp32 steps with DiceLoss only (what a `rocprofv3 --kernel-trace --stats` run of a Dice step wraps)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

B, N_IN, C, S = 16, 4, 5, 512


def loss_pairs(iters=50):
    from unet_amd import ops
    g = torch.Generator().manual_seed(0)
    z = ops.TS((torch.randn(B, S, S, 8, generator=g) * 2).cuda(), 0, C)
    y = torch.randint(0, C, (B, S, S), generator=g).cuda()
    w = torch.full((C,), 1.0 / C, device="cuda")
    loss, denom = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    coef = torch.zeros(2 * B * C, device="cuda")
    ws = torch.empty(max(ops.ce_workspace(z.P), ops.dice_workspace(B, S * S, C)), device="cuda")
    out = {}
    for dt in (torch.float32, torch.bfloat16):
        dz = ops.TS(torch.zeros(B, S, S, 8, dtype=dt, device="cuda"), 0, C)
        pairs = {"ce": (lambda: ops.ce_fwd(z, y, w, loss, denom, ws), lambda: ops.ce_bwd(z, y, w, denom, 1.0, dz)),
                 "dice": (lambda: ops.dice_fwd(z, y, 1e-6, False, 0, loss, coef, ws), lambda: ops.dice_bwd(z, y, False, coef, 1.0, dz))}
        for name, (fwd, bwd) in pairs.items():
            for _ in range(5):
                fwd(); bwd()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            tf = tb = 0.0
            for _ in range(iters):
                ev[0].record(); fwd(); ev[1].record(); bwd(); ev[2].record()
                torch.cuda.synchronize()
                tf += ev[0].elapsed_time(ev[1]); tb += ev[1].elapsed_time(ev[2])
            out[f"{name}_{'f32' if dt == torch.float32 else 'bf16'}"] = {"fwd_us": round(1e3 * tf / iters, 2), "bwd_us": round(1e3 * tb / iters, 2),
                                                                           "pair_us": round(1e3 * (tf + tb) / iters, 2)}
    for d in ("f32", "bf16"):
        out[f"ratio_{d}"] = round(out[f"dice_{d}"]["pair_us"] / out[f"ce_{d}"]["pair_us"], 3)
    print(json.dumps({"what": "loss kernel pairs, cfg2 logits", **out}), flush=True)


def steps(n_steps=10, warmup=3, dtypes=("f32", "bf16"), names=("ce", "dice", "ce2", "dice2")):
    from unet_amd.learner import DiceLoss
    from unet_amd.model import HipDynamicUnet
    from unet_amd.optimizer import FlatAdam
    from unet_amd.trainer import TrainStep
    g = torch.Generator().manual_seed(1234)
    x = (torch.randint(0, 256, (B, N_IN, S, S), generator=g).float() / 255).cuda()
    y = torch.randint(0, C, (B, S, S), generator=g).cuda()
    for dtype in dtypes:
        torch.manual_seed(0)
        model = HipDynamicUnet("xresnet34", N_IN, C, (S, S), act_dtype=dtype)
        model.train()
        opt = FlatAdam(model, [1e-5, 1e-4 / 10 ** 0.5, 1e-4])
        step = TrainStep(model, opt, torch.full((C,), 1.0 / C, device="cuda"), 1)
        res = {}
        for name in names:          # interleaved: drift shows as ce != ce2
            step.dice = DiceLoss() if name.startswith("dice") else None
            for _ in range(warmup):
                step(x, y)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                loss = step(x, y)
            torch.cuda.synchronize()
            res[name] = round(B * n_steps / (time.perf_counter() - t0), 2)
            assert torch.isfinite(loss).all()
        ratio = {}
        if "ce" in res and "dice" in res:
            ratio["dice_over_ce"] = round(max(res["dice"], res.get("dice2", 0)) / max(res["ce"], res.get("ce2", 0)), 4)
        print(json.dumps({"what": "train step tiles/s", "dtype": dtype, **res, **ratio}), flush=True)
        del model, opt, step
        torch.cuda.empty_cache()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "both"
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    if mode in ("loss", "both"):
        loss_pairs()
    if mode in ("step", "both"):
        steps(k)
    if mode == "profile":
        loss_pairs(iters=10)
        steps(k, warmup=2, dtypes=("f32",), names=("dice",))
