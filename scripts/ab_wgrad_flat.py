"""A/B of wgrad_flat_kernel's two load paths, isolated launches in ONE process: LDS-DMA (unet_tuning.wgrad_narrow = 1, the default where the
planner allows it) against register staging (wgrad_narrow = 4), alternating, REPS timings each.  A timing covers the kernel, the split
reduction and the bias reduction as the step issues them.  Shapes: the final ResBlock pair (100 -> 100 at 16 x 512^2, <6, 5, sliver>) and the
last UnetBlock's convs (192 -> 96 and 96 -> 96 at 16 x 256^2, <6, 7>).  Prints every timing, then medians and max - min per form: the DMA
form counts as faster only where its median beats the register form's by more than the register form's own max - min.

    python scripts/ab_wgrad_flat.py [--sliver]     (--sliver: the older A/B of the 4-row sliver against seven tiles, wgrad_narrow 1 against 2)"""
import os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch
from unet_amd import ops
from unet_amd.ops import TS

REPS = 7
g = torch.Generator(device="cuda").manual_seed(0)


def timed(x, dy, Cin, Cout, narrow):
    with ops.tuning(wgrad_narrow=narrow):
        ws = torch.empty(ops.wgrad_workspace(x, dy, 3, 1, with_bias=True), device="cuda")
        dw = torch.empty((Cout, Cin, 3, 3), device="cuda"); db = torch.empty(Cout, device="cuda")
        for _ in range(2):
            ops.conv2d_wgrad(x, dy, dw, 3, 1, ws, dbias=db)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            ops.conv2d_wgrad(x, dy, dw, 3, 1, ws, dbias=db)
        e1.record(); torch.cuda.synchronize()
        dma = ops.wgrad_uses_dma(x, dy, 3, 1)
    return e0.elapsed_time(e1) / 4, dw, db, dma


def operands(N, H, Cin, Cout):
    x = TS(torch.randn((N, H, H, ops.rup4(Cin)), device="cuda", generator=g), 0, Cin)
    dy = TS(torch.randn((N, H, H, ops.rup4(Cout)), device="cuda", generator=g), 0, Cout)
    return x, dy


if "--sliver" in sys.argv:
    for Cin, Cout in [(100, 100), (96, 100), (100, 96)]:
        x, dy = operands(16, 512, Cin, Cout)
        res = {}
        for narrow in (1, 2, 1, 2):
            ms, dw, _, _ = timed(x, dy, Cin, Cout, narrow)
            fl = 2.0 * 16 * 512 * 512 * Cin * Cout * 9
            res.setdefault(narrow, []).append(dw.clone())
            print(f"[wgrad_narrow {narrow}] {Cin:4d}->{Cout:4d}  {ms:7.3f} ms  {fl / ms / 1e9:6.1f} TF  checksum {dw.double().sum().item():.9e}", flush=True)
        a, b = res[1][0], res[2][0]
        print(f"   max |sliver - seven tiles| / max |dw| = {(a - b).abs().max().item() / b.abs().max().item():.2e}")
    sys.exit(0)

for N, H, Cin, Cout in [(16, 512, 100, 100), (16, 256, 192, 96), (16, 256, 96, 96)]:
    x, dy = operands(N, H, Cin, Cout)
    fl = 2.0 * N * H * H * Cin * Cout * 9
    ms = {1: [], 4: []}
    out = {}
    for rep in range(REPS):
        for narrow in (4, 1):
            t, dw, db, dma = timed(x, dy, Cin, Cout, narrow)
            assert dma == (narrow == 1), "the planner did not pick the form under test"
            ms[narrow].append(t)
            out[narrow] = (dw, db)
            print(f"[{'dma' if dma else 'reg'}] {Cin:4d}->{Cout:4d} at {N} x {H}^2  {t:7.3f} ms  {fl / t / 1e9:6.1f} TF", flush=True)
    same_w = torch.equal(out[1][0].view(torch.int32), out[4][0].view(torch.int32))
    db_err = (out[1][1] - out[4][1]).abs().max().item() / out[4][1].abs().max().item()
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    verdict = "DMA wins" if med[4] - med[1] > spread[4] else "no win beyond the register form's spread"
    print(f"== {Cin}->{Cout} at {N} x {H}^2: reg median {med[4]:.3f} ms (max - min {spread[4]:.3f}), dma median {med[1]:.3f} ms (max - min {spread[1]:.3f}), "
          f"dma / reg = {med[1] / med[4]:.4f}: {verdict}; dw bit-equal: {same_w}; max |dbias diff| / max |dbias| = {db_err:.1e}", flush=True)
