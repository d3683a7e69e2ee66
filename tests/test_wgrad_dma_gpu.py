"""The LDS-DMA form of wgrad_flat_kernel against its register-staged form (unet_tuning.wgrad_narrow = 4) and against fp64.

Every shape runs with the bias gradient requested, on the integer operands of wgrad_cases (every partial sum exact in fp32 in any order), as
channel slices of canary-filled buffers inside guard bands and over a NaN workspace: dw and dbias of the default run, of its repetition and
of the register-staged run are the same bits, and equal the fp64 reference.  The shapes are the smallest that reach each path of the DMA
pipeline: a tile that starts a column strip refills synchronously, a tile one row further down rolls (one new input row into the ring slot
its column block does not read, the dy row into the other dy tile)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import wgrad_cases as wc  # noqa: E402
from guard import guarded  # noqa: E402

NAN = float("nan")

# (N, H, W, Cin, Cout, tuning, the planner picks DMA, what it exercises)
SHAPES = [
    (2, 1, 32, 100, 100, {}, True, "one-row image: every tile is a strip start"),
    (2, 2, 33, 96, 96, {}, True, "ragged second column strip, <6,7>"),
    (2, 3, 64, 100, 100, {}, True, "ring wraps once"),
    (2, 5, 40, 192, 96, dict(wgrad_wgs=20), True, "two chunks, rolling tiles, a split boundary inside a strip"),
    (3, 5, 32, 112, 101, {}, True, "<7,5>, four column blocks"),
    (2, 4, 32, 100, 97, {}, True, "sliver with one real row"),
    (2, 3, 32, 36, 100, {}, False, "narrow chunk: a block reads all three tap rows -> registers"),
]
IDS = [f"{N}x{H}x{W}-{Cin}to{Cout}" for N, H, W, Cin, Cout, _, _, _ in SHAPES]
FAMILY = ["flat<6,5,sliver>", "flat<6,7>", "flat<6,5,sliver>", "flat<6,7>", "flat<7,5>", "flat<6,5,sliver>", "flat<6,5,sliver>"]


def _case(i):
    N, H, W, Cin, Cout, tune, _, _ = SHAPES[i]
    return wc.Case(N, H, W, Cin, Cout, 3, 1, "f32", wc.LAYOUTS[(i + 1) % len(wc.LAYOUTS)], tuple(sorted(tune.items())))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(got, ref, what):
    got = got.cpu().double()
    if torch.equal(got, ref):
        return
    bad = ~(got == ref)
    first = bad.nonzero()[0].tolist()
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the fp64 reference, {int(got.isnan().sum())} of them "
                         f"NaN; first at {first}: got {got[tuple(first)].item()!r}, expected {ref[tuple(first)].item()!r}")


def _run(ops, c, xt, dyt, narrow, checks, what):
    """(dw, dbias) of one launch under c.tuning + wgrad_narrow, over a NaN workspace, everything guard-banded"""
    with ops.tuning(**dict(c.tuning), wgrad_narrow=narrow):
        n = ops.wgrad_workspace(xt, dyt, 3, 1, with_bias=True)
        assert n == wc.workspace_floats(c, wc.plan(c)), what
        ws, wscheck = guarded((n,), torch.float32, fill=NAN)
        dw, dwcheck = guarded((c.Cout, c.Cin, 3, 3), torch.float32, fill=NAN)
        db, dbcheck = guarded((c.Cout,), torch.float32, fill=NAN)
        ops.conv2d_wgrad(xt, dyt, dw, 3, 1, ws, dbias=db)
        torch.cuda.synchronize()
    for name, chk in (("workspace", wscheck), ("dw", dwcheck), ("dbias", dbcheck)) + checks:
        chk(f"{what}: {name}")
    return dw, db


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_dma_form_is_exact_and_equals_the_register_form(i):
    from unet_amd import ops
    c = _case(i)
    N, H, W, Cin, Cout, tune, dma, why = SHAPES[i]
    p = wc.plan(c)
    assert p["family"] == FAMILY[i], (p["family"], why)
    assert wc.exact_bound(c) < 2 ** 24
    if "split boundary" in why:
        assert p["splits"] > 1 and p["tpb"] % H != 0, p
    x, dy = wc.exact_inputs(c, 7000 + i)
    ref_w, ref_b = wc.reference(c, x, dy)
    (xt, xcheck), (dyt, dycheck) = wc.operands(c, x, dy)
    checks = (("x", xcheck), ("dy", dycheck))

    outs = {}
    for run, narrow in (("default", 1), ("register-staged", 4), ("default again", 1)):
        what = f"{IDS[i]} [{p['family']}, {why}] {run}"
        with ops.tuning(**dict(c.tuning), wgrad_narrow=narrow):
            assert ops.wgrad_uses_dma(xt, dyt, 3, 1) == (dma and narrow == 1), what
        dw, db = _run(ops, c, xt, dyt, narrow, checks, what)
        _same(dw, ref_w, f"{what}: dw")
        _same(db, ref_b, f"{what}: dbias")
        outs[run] = (_bits(dw), _bits(db))
    for run in ("register-staged", "default again"):
        assert torch.equal(outs["default"][0], outs[run][0]), f"{IDS[i]}: dw of the default run and of '{run}' differ"
        assert torch.equal(outs["default"][1], outs[run][1]), f"{IDS[i]}: dbias of the default run and of '{run}' differ"


def test_dma_form_on_gaussian_operands():
    """the two-chunk rolling case at the tolerances of test_wgrad_gpu (test_conv_wgrad: 3e-4 of the scale + 1e-4), both forms"""
    from unet_amd import ops
    i = 3
    c = _case(i)
    x, dy = wc.gauss_inputs(c, 7100)
    ref_w, ref_b = wc.reference(c, x, dy)
    (xt, xcheck), (dyt, dycheck) = wc.operands(c, x, dy)
    for narrow in (1, 4):
        what = f"{IDS[i]} Gaussian operands, wgrad_narrow {narrow}"
        dw, db = _run(ops, c, xt, dyt, narrow, (("x", xcheck), ("dy", dycheck)), what)
        for got, ref, name in ((dw, ref_w, "dw"), (db, ref_b, "dbias")):
            err = (got.cpu().double() - ref).abs().max().item()
            scale = ref.abs().max().item()
            bound = 3e-4 * scale + 1e-4
            assert math.isfinite(err) and err <= bound, f"{what}: {name}: max abs err {err:.3e} over the bound {bound:.3e} at scale {scale:.3e}"
