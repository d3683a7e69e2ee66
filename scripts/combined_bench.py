"""CombinedLoss (focal + alpha * Dice) at cfg2 (batch 16 of 4x512x512 tiles, xresnet34, 5 classes), two timings:
  loss: the fused forward + backward pair on the logits slice against the four launches it replaces (focal_fwd, focal_bwd, dice_fwd,
        dice_bwd: without the fused pair a user pays all four, and the second backward would still overwrite the first), fp32 and bf16
        gradient, the two variants alternating round by round;
  step: whole training steps (TrainStep, resident batch) with CombinedLoss against CrossEntropyLossFlat, interleaved.
usage: python scripts/combined_bench.py [loss|step|both] [steps=10]   -- one JSON line per measurement on stdout"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

B, N_IN, C, S = 16, 4, 5, 512
GAMMA, SMOOTH, ALPHA = 2.0, 1.0, 1.0


def loss_pairs(iters=200, rounds=5):
    from unet_amd import ops
    g = torch.Generator().manual_seed(0)
    z = ops.TS((torch.randn(B, S, S, 8, generator=g) * 2).cuda(), 0, C)
    y = torch.randint(0, C, (B, S, S), generator=g).cuda()
    w = torch.full((C,), 1.0 / C, device="cuda")
    loss, terms = torch.zeros(1, device="cuda"), torch.zeros(2, device="cuda")
    coef = torch.zeros(2 * B * C, device="cuda")
    ws = torch.empty(max(ops.ce_workspace(z.P), ops.dice_workspace(B, S * S, C), ops.combined_workspace(B, S * S, C)), device="cuda")
    out = {}
    for dt in (torch.float32, torch.bfloat16):
        dz = ops.TS(torch.zeros(B, S, S, 8, dtype=dt, device="cuda"), 0, C)

        def fused():
            ops.combined_fwd(z, y, w, GAMMA, SMOOTH, False, 0, terms, coef, ws)
            ops.combined_bwd(z, y, w, GAMMA, False, coef, 1.0, ALPHA, dz)

        def separate():
            ops.focal_fwd(z, y, w, GAMMA, loss, ws)
            ops.focal_bwd(z, y, w, GAMMA, 1.0, dz)
            ops.dice_fwd(z, y, SMOOTH, False, 0, loss, coef, ws)
            ops.dice_bwd(z, y, False, coef, ALPHA, dz)

        times = {"fused": [], "separate": []}
        for fn in (fused, separate):
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, fn in (("fused", fused), ("separate", separate)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(1e3 * e0.elapsed_time(e1) / iters)
        d = "f32" if dt == torch.float32 else "bf16"
        for name, t in times.items():
            out[f"{name}_{d}"] = {"us": round(statistics.median(t), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2)}
        out[f"fused_over_separate_{d}"] = round(out[f"fused_{d}"]["us"] / out[f"separate_{d}"]["us"], 3)
    print(json.dumps({"what": "loss launches per step, cfg2 logits: combined fwd + bwd against focal fwd + bwd + dice fwd + bwd", "iters": iters,
                      "rounds": rounds, **out}), flush=True)


def steps(n_steps=10, warmup=3, dtypes=("f32", "bf16"), names=("ce", "combined", "ce2", "combined2")):
    from unet_amd.learner import CombinedLoss
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
            step.combined = CombinedLoss(1, SMOOTH, ALPHA, gamma=GAMMA) if name.startswith("combined") else None
            for _ in range(warmup):
                step(x, y)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                loss = step(x, y)
            torch.cuda.synchronize()
            res[name] = round(B * n_steps / (time.perf_counter() - t0), 2)
            assert torch.isfinite(loss).all()
        ratio = {"combined_over_ce": round(max(res["combined"], res.get("combined2", 0)) / max(res["ce"], res.get("ce2", 0)), 4)}
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
