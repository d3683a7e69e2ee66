"""Every weight-gradient kernel of csrc/conv_wgrad.hip, as training runs it and with nowhere to hide (cases, planner mirror and operand
builders: tests/wgrad_cases.py; what the table covers: tests/test_wgrad_cases_cpu.py):

  * the operands are channel slices of wider buffers whose other channels hold a loud canary (pad lanes zero), inside guard bands;
  * the workspace is exactly as large as planned, its BODY poisoned with NaN (training hands over a buffer full of another layer's
    partials: a partial element that no workgroup writes reads as NaN here, not as the zero of a fresh allocation) and guard-banded, as
    are dw and dbias (in training, views into one flat gradient buffer);
  * the operands are small integers, so dw, dbias and every partial sum are exact in fp32 in any order: the results are compared with
    the fp64 reference bit for bit -- one dropped or doubled pixel, or a multiply at reduced precision, fails;
  * the accumulate form adds to a prefilled dw exactly;
  * Gaussian operands at the tolerances of test_conv_wgrad / test_bf16_gpu, twice: over a NaN and over a 1e30 workspace the result
    must be the same bits.

The test id names the kernel instantiation the planner mirror predicts for the case."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import wgrad_cases as wc  # noqa: E402
from guard import guarded  # noqa: E402
from wgrad_cases import CASES, case_id, plan  # noqa: E402

NAN = float("nan")


def _same(got, ref, what):
    got = got.cpu().double()
    if torch.equal(got, ref):
        return
    bad = ~(got == ref)
    first = bad.nonzero()[0].tolist()
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the fp64 reference, {int(got.isnan().sum())} of them "
                         f"NaN; first at {first}: got {got[tuple(first)].item()!r}, expected {ref[tuple(first)].item()!r}")


def _close(c, got, ref, what, bias=False):
    err = (got.cpu().double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    if c.dtype == "bf16":          # test_conv_forward_dgrad_wgrad_bf16
        bound = 5e-5 * scale + (1e-5 if bias else 0.0)
    else:                          # test_conv_wgrad (tests.util.assert_close)
        bound = 3e-4 * scale + 1e-4
    assert err <= bound, f"{what}: max abs err {err:.3e} (NaN: not finite) over the bound {bound:.3e} at scale {scale:.3e}"
    assert math.isfinite(err), what


@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(i) for i in range(len(CASES))])
def test_wgrad_case(i):
    from unet_amd import ops
    c = CASES[i]
    p = plan(c)
    what = f"{case_id(i)} [{p['family']}, splits {p['splits']} x {p['nsub']}, reduce {p['reduce']}, grid height {p['grid_y']}]"
    shape = (c.Cout, c.Cin, c.ks, c.ks)
    x, dy = wc.exact_inputs(c, i)
    ref_w, ref_b = wc.reference(c, x, dy)
    (xt, xcheck), (dyt, dycheck) = wc.operands(c, x, dy)
    x0, dy0 = xt.buf.clone(), dyt.buf.clone()

    with ops.tuning(**dict(c.tuning)):
        n = ops.wgrad_workspace(xt, dyt, c.ks, c.stride, with_bias=True)
        assert n == wc.workspace_floats(c, p), f"{what}: the library plans {n} workspace floats, the mirror {wc.workspace_floats(c, p)}"
        ws, wscheck = guarded((n,), torch.float32, fill=NAN)
        dw, dwcheck = guarded(shape, torch.float32, fill=NAN)
        db, dbcheck = guarded((c.Cout,), torch.float32, fill=NAN)

        def bands(stage, *more):
            for name, chk in (("workspace", wscheck), ("x", xcheck), ("dy", dycheck)) + more:
                chk(f"{what}: {stage}: {name}")

        # 1-3: dw and dbias over a poisoned workspace, exactly
        ops.conv2d_wgrad(xt, dyt, dw, c.ks, c.stride, ws, dbias=db)
        torch.cuda.synchronize()
        _same(dw, ref_w, f"{what}: dw")
        _same(db, ref_b, f"{what}: dbias")
        bands("first launch", ("dw", dwcheck), ("dbias", dbcheck))

        # 4: accumulate into a prefilled dw, no bias gradient
        acc, acccheck = guarded(shape, torch.float32, fill=wc.PREFILL)
        ws.fill_(NAN)
        ops.conv2d_wgrad(xt, dyt, acc, c.ks, c.stride, ws, accumulate=True)
        torch.cuda.synchronize()
        _same(acc, ref_w + wc.PREFILL, f"{what}: accumulate")
        bands("accumulate", ("dw", acccheck))
        assert torch.equal(xt.buf.view(torch.int32 if c.dtype == "f32" else torch.int16), x0.view(torch.int32 if c.dtype == "f32" else torch.int16))
        assert torch.equal(dyt.buf.view(torch.int32 if c.dtype == "f32" else torch.int16), dy0.view(torch.int32 if c.dtype == "f32" else torch.int16))

        # 5: Gaussian operands over a NaN and over a 1e30 workspace: the same bits, within the project's tolerances of fp64
        gx, gdy = wc.gauss_inputs(c, 1000 + i)
        gref_w, gref_b = wc.reference(c, gx, gdy)
        (gxt, gxcheck), (gdyt, gdycheck) = wc.operands(c, gx, gdy)
        outs = []
        for fill in (NAN, 1e30):
            ws.fill_(fill)
            gw, gwcheck = guarded(shape, torch.float32, fill=NAN)
            gb, gbcheck = guarded((c.Cout,), torch.float32, fill=NAN)
            ops.conv2d_wgrad(gxt, gdyt, gw, c.ks, c.stride, ws, dbias=gb)
            torch.cuda.synchronize()
            for name, chk in (("workspace", wscheck), ("x", gxcheck), ("dy", gdycheck), ("dw", gwcheck), ("dbias", gbcheck)):
                chk(f"{what}: Gaussian operands, workspace of {fill}: {name}")
            _close(c, gw, gref_w, f"{what}: Gaussian dw over a workspace of {fill}")
            _close(c, gb, gref_b, f"{what}: Gaussian dbias over a workspace of {fill}", bias=True)
            outs.append((gw.cpu(), gb.cpu()))
        assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), f"{what}: dw depends on what the workspace held"
        assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)), f"{what}: dbias depends on what the workspace held"
