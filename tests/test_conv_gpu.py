"""Every forward and input-gradient conv kernel behind unet_conv2d (csrc/conv_igemm.hip, conv_bf16.hip, conv1x1.hip and the split-K
reduce), one stand-alone launch per case of tests/conv_cases.py, as training runs it and with nowhere to hide (what the table covers:
tests/test_conv_cases_cpu.py):

  * x, the packed filters, bias, res and mask sit in guard-banded allocations; the activations are channel slices of wider buffers whose
    other channels hold a loud finite canary (pad lanes zero); the filters are packed by the library's own packing kernels;
  * y is a channel slice of a guard-banded buffer that starts as NaN everywhere: an element no lane stores reads as NaN, a store outside
    the produced channels or past the tensor destroys a sentinel;
  * a split-K launch brings a workspace of exactly the planned floats, poisoned with NaN and guard-banded (training hands over one buffer
    full of another layer's partial sums); then the same launch over a workspace full of 1e30 must give the same bits, and over a
    workspace one float short the unsplit plan and the same exact result;
  * the operands are integers whose every partial sum is exact in fp32 (conv_cases.exact_bound), so the result is compared with the fp64
    reference bit for bit: one dropped product, a tap read one pixel off, a multiply at reduced precision fails; a bf16 output is the exact
    value rounded once;
  * Gaussian operands at the tolerances of test_conv_fwd / test_conv_forward_dgrad_wgrad_bf16; a split launch twice, over a NaN and over
    a 1e30 workspace, with identical bits.

The test id names the kernel instantiation(s) that follow from the variant the case states; the launch asserts that variant."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_cases as cc  # noqa: E402
from conv_cases import CASES, case_id, has  # noqa: E402
from guard import guarded  # noqa: E402

NAN = float("nan")
_INT = {2: torch.int16, 4: torch.int32}


def _bits(t):
    return t.view(_INT[t.element_size()])


def _flat(n, dtype, fill):
    """a guard-banded 1-D buffer whose start stays 16-byte aligned whatever n is (the default band is n elements long)"""
    return guarded((n,), dtype, fill=fill, guard=cc.rup(max(n, 32768), 64))


def _same(got, ref, what):
    got = got.double()
    if torch.equal(got, ref):
        return
    bad = ~(got == ref)
    first = bad.nonzero()[0].tolist()
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the fp64 reference, {int(got.isnan().sum())} of them "
                         f"NaN; first at {first}: got {got[tuple(first)].item()!r}, expected {ref[tuple(first)].item()!r}")


def _close(c, got, ref, what):
    err = (got.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    if c.dtype == "f32":            # test_conv_fwd (tests.util.assert_close at rtol 2e-4)
        bound = 2e-4 * scale + 1e-5
    elif has(c, "y_f32"):           # test_conv_forward_dgrad_wgrad_bf16, fp32 output
        bound = 2e-5 * scale
    else:                           # ... bf16 output
        bound = 2.0 ** -8 * scale + 1e-6
    assert err <= bound, f"{what}: max abs err {err:.3e} (NaN: not finite) over the bound {bound:.3e} at scale {scale:.3e}"
    assert math.isfinite(err), what


class Launch:
    """the device operands of one case (built once per operand set) and its launches into fresh outputs"""

    def __init__(self, c, host, what):
        from unet_amd import _lib as L
        from unet_amd import ops
        self.c, self.what, self.L, self.ops = c, what, L, ops
        dt = cc.torch_dtype(c)
        s = cc.strides(c)
        self.checks = {}
        self.x, self.checks["x"] = cc.device_slice(host["x"], *s["x"], dt)
        self.res = self.mask = self.bias = self.tail = None
        if "res" in host:
            self.res, self.checks["res"] = cc.device_slice(host["res"], *s["res"], dt)
        if "mask" in host:
            self.mask, self.checks["mask"] = cc.device_slice(host["mask"], *s["mask"], dt)
        if "bias" in host:
            self.bias, self.checks["bias"] = _flat(c.Cout, torch.float32, cc.canary(torch.float32))
            self.bias.copy_(host["bias"])
        if "tail" in host:
            v = ops.vec_of(dt)
            self.tail, self.checks["tail"] = cc.device_slice(host["tail"], v, 3 * v, dt)
        # the packed filter image(s), by the library's packing kernels: mode 0 forward, 1 input gradient, 2 pixel-shuffle column order
        mode = 2 if has(c, "ps") else (1 if c.kind == "dgrad" else 0)
        w = host["w"].cuda().contiguous()
        imgs = list(w) if has(c, "wimg") else [w]
        size = (L.lib.unet_pack_weights_size_bf16 if c.dtype == "bf16" else L.lib.unet_pack_weights_size)
        self.img = int(size(imgs[0].shape[0], imgs[0].shape[1], c.ks, mode))
        self.wp, self.checks["packed filters"] = _flat(self.img * len(imgs), dt, cc.canary(dt))
        for n, wi in enumerate(imgs):
            out = ops.pack_weights(wi.contiguous(), mode, out=self.wp[n * self.img:(n + 1) * self.img], dtype=dt)
            assert out.data_ptr() == self.wp.data_ptr() + n * self.img * self.wp.element_size()
        self.before = {k: _bits(t).clone() for k, t in self._operand_buffers().items()}

    def _operand_buffers(self):
        bufs = dict(x=self.x.buf, wp=self.wp)
        for k in ("res", "mask", "tail"):
            if getattr(self, k) is not None:
                bufs[k] = getattr(self, k).buf
        if self.bias is not None:
            bufs["bias"] = self.bias
        return bufs

    def run(self, ws, ws_floats, want_variant, stage):
        """one launch into a fresh y (and fresh column-sum buffers); returns (y buffer on the host, colsum, colsumsq) after checking the variant,
        every sentinel channel, every guard band and that no operand changed"""
        c, L, ops = self.c, self.L, self.ops
        what = f"{self.what}: {stage}"
        _, _, OH, OW = cc.dims(c)
        ydt = torch.float32 if cc.y_vec(c) == 4 else torch.bfloat16
        co, cs = cc.strides(c)["y"]
        yh, yw = (2 * c.H, 2 * c.W) if has(c, "ps") else (OH, OW)
        ybuf, ycheck = guarded((c.N, yh, yw, cs), ydt, fill=NAN)
        y = ops.TS(ybuf, co, cc.y_channels(c))
        colsum = colsumsq = None
        checks = dict(self.checks, y=ycheck)
        if has(c, "colsum"):
            colsum, checks["colsum"] = guarded((c.rows, c.Cout), torch.float32, fill=NAN)
        if has(c, "colsumsq"):
            colsumsq, checks["colsumsq"] = guarded((c.rows, c.Cout), torch.float32, fill=NAN)
        if has(c, "ps"):
            d = ops._ps_desc(self.x, self.wp, y, self.bias, has(c, "relu"))
            if self.tail is not None:
                d.ps_tail, d.ps_tail_cs, d.ps_tail_co, d.ps_tail_c, d.ps_tail_at = self.tail.ptr, self.tail.cs, self.tail.co, self.tail.C, cc.tail_at(c)
        else:
            d = ops._conv_desc(self.x, self.wp, y, c.ks, c.stride, L.CONV_DGRAD if c.kind == "dgrad" else L.CONV_FWD, self.bias, self.res, self.mask,
                               has(c, "relu"), colsum, colsumsq)
            d.cout_begin, d.cout_count = c.begin, c.count
            if has(c, "wimg"):
                d.wp_img_stride = self.img
        if ws is not None:
            d.splitk_ws, d.splitk_ws_floats = ws.data_ptr(), ws_floats
        assert int(L.lib.unet_conv2d_splitk_workspace(C.byref(d))) == c.ws_floats, what
        got_variant = int(L.lib.unet_conv2d_variant(C.byref(d)))
        if want_variant is None:          # the unsplit plan of a launch whose workspace is too small
            assert 0 <= got_variant < 1000000, f"{what}: the library plans variant {got_variant} over a workspace that is too small to split"
        else:
            assert got_variant == want_variant, f"{what}: the library plans variant {got_variant}, the case states {want_variant}"
        if has(c, "colsum"):
            assert int(L.lib.unet_conv2d_colsum_rows(C.byref(d))) == c.rows, what
        L.check(L.lib.unet_conv2d(C.byref(d), ops._stream()), what)
        torch.cuda.synchronize()
        for name, chk in checks.items():
            chk(f"{what}: {name}")
        for k, t in self._operand_buffers().items():
            assert torch.equal(_bits(t), self.before[k]), f"{what}: the launch changed its operand {k}"
        got = ybuf.cpu()
        self._sentinels(got, what)
        return got, (None if colsum is None else colsum.cpu()), (None if colsumsq is None else colsumsq.cpu())

    def _sentinels(self, got, what):
        """every channel of y's buffer the launch does not produce still holds the NaN it started with (the channels of other ranges among
        them).  The pad lanes behind the last channel (up to the next multiple of the 4- or 8-channel vector) belong to the slice, in either
        storage type: a kernel that stores whole vectors (the 256-pixel tile and its fp32 sliver at Cout = 97) puts zeros there -- the
        filter columns and the bias beyond Cout are zero -- so they hold their sentinel or +0.0, nothing else"""
        c = self.c
        co, cs = cc.strides(c)["y"]
        b, n = (0, cc.y_channels(c)) if has(c, "ps") else cc.produced(c)
        C_ = cc.y_channels(c)
        keep = torch.ones(cs, dtype=torch.bool)
        keep[co + b:co + b + n] = False
        pad = torch.zeros(cs, dtype=torch.bool)
        if b + n == C_:
            pad[co + C_:co + cc.rup(C_, cc.y_vec(c))] = True
        tq = cc.rup(cc.tail_channels(c), 4)
        if tq:
            keep[cc.tail_at(c):cc.tail_at(c) + tq] = False
        sent = _bits(torch.full((1,), NAN, dtype=got.dtype)).item()
        bits = _bits(got)
        other = bits[..., keep & ~pad]
        assert bool((other == sent).all()), (f"{what}: {int((other != sent).sum())} elements of channels the launch does not produce were overwritten "
                                             f"(buffer channels {sorted(set((other != sent).nonzero()[:, -1].tolist()))[:8]} of those kept)")
        pads = bits[..., pad]
        assert bool(((pads == sent) | (pads == 0)).all()), f"{what}: pad lanes of the output slice hold neither their sentinel nor zero"

    def produced(self, got):
        c = self.c
        co, _ = cc.strides(c)["y"]
        b, n = (0, cc.y_channels(c)) if has(c, "ps") else cc.produced(c)
        return got[..., co + b:co + b + n].float()

    def check_tail(self, got, what):
        tq = cc.rup(cc.tail_channels(self.c), 4)
        if tq:
            at = cc.tail_at(self.c)
            src = self.tail.buf.cpu()[..., self.tail.co:self.tail.co + tq]
            assert torch.equal(_bits(got[..., at:at + tq].contiguous()), _bits(src.contiguous())), f"{what}: the tail channels behind the shuffled ones"


def _ref_produced(c, ref):
    b, n = (0, ref.shape[-1]) if has(c, "ps") else cc.produced(c)
    return ref[..., b:b + n]


def _check_colsums(c, out, cs_, cq_, what, exact):
    """the library's partial rows, summed in fp64, against the per-channel sums over pixels of the STORED output and of its square"""
    if cs_ is None:
        return
    y = out.double()
    for name, rows, want in (("colsum", cs_, y.sum((0, 1, 2))), ("colsumsq", cq_, (y * y).sum((0, 1, 2)))):
        if rows is None:
            continue
        assert bool(rows.isfinite().all()), f"{what}: {int((~rows.isfinite()).sum())} elements of the {name} rows were never written"
        got = rows.double().sum(0)
        if exact:
            _same(got, want, f"{what}: {name}")
        else:                           # test_conv_fwd_slices_relu_res_colsum
            err, scale = (got - want).abs().max().item(), want.abs().max().item()
            assert err <= 2e-4 * scale + 1e-2, f"{what}: {name}: max abs err {err:.3e} at scale {scale:.3e}"


@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(i) for i in range(len(CASES))])
def test_conv_case(i):
    from unet_amd import ops
    c = CASES[i]
    what = case_id(i)
    split = cc.splits_of(c) >= 2

    with ops.tuning(**dict(c.tuning)):
        # 1, 2: exact operands over a poisoned workspace of exactly the planned size (or the case's short / missing one)
        host = cc.exact_inputs(c, i)
        ref = cc.stored(c, cc.reference(c, host))
        want = _ref_produced(c, ref)
        run = Launch(c, host, what)
        n = c.ws_floats - (1 if c.ws == "short" else 0)
        ws = wscheck = None
        if c.ws_floats and c.ws != "none":
            ws, wscheck = _flat(n, torch.float32, NAN)
            run.checks["workspace"] = wscheck
        got, cs_, cq_ = run.run(ws, n, c.variant, "exact operands")
        _same(run.produced(got), want, f"{what}: exact operands")
        run.check_tail(got, what)
        _check_colsums(c, run.produced(got), cs_, cq_, f"{what}: exact operands", exact=True)

        # 3: a workspace full of another layer's partial sums, then one that is a float short
        if split:
            ws.fill_(1e30)
            again, _, _ = run.run(ws, n, c.variant, "exact operands over a workspace of 1e30")
            assert torch.equal(_bits(again), _bits(got)), f"{what}: the result depends on what the workspace held"
            del run.checks["workspace"]
            short, run.checks["short workspace"] = _flat(n - 1, torch.float32, NAN)
            got_s, _, _ = run.run(short, n - 1, None, "exact operands, a workspace one float short")
            _same(run.produced(got_s), want, f"{what}: exact operands, a workspace one float short")
            del run.checks["short workspace"]
            run.checks["workspace"] = wscheck

        # 4: Gaussian operands in the same placement
        ghost = cc.gauss_inputs(c, 100000 + i)
        gref = _ref_produced(c, cc.reference(c, ghost))
        grun = Launch(c, ghost, what)
        if ws is not None:
            grun.checks["workspace"] = wscheck
        outs = []
        for fill in ((NAN, 1e30) if split else (NAN,)):
            if ws is not None:
                ws.fill_(fill)
            stage = f"Gaussian operands, workspace of {fill}" if split else "Gaussian operands"
            g, gcs, gcq = grun.run(ws, n, c.variant, stage)
            _close(c, grun.produced(g), gref, f"{what}: {stage}")
            grun.check_tail(g, what)
            _check_colsums(c, grun.produced(g), gcs, gcq, f"{what}: {stage}", exact=False)
            outs.append(g)
        if split:
            assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"{what}: the Gaussian result depends on what the workspace held"
