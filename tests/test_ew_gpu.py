"""Every form of the BatchNorm, elementwise, pooling, shuffle and resize kernels of csrc/elementwise.hip, one stand-alone launch (or forward /
adjoint pair) per case of tests/ew_cases.py, with nowhere to hide (what the table covers: tests/test_ew_cases_cpu.py):

  * every tensor operand is a channel slice of a guard-banded buffer (tests/guard.py) whose other channels and bands hold a loud finite
    canary (pad lanes zero); per-channel vectors sit in guard-banded buffers too; the base addresses are 16-byte aligned, as ew_cases.form
    assumes, and that is asserted;
  * every output is a slice of a guard-banded buffer that starts as NaN everywhere (an accumulating launch finds exact integers in the slice):
    an element no lane stores reads as NaN, a store beside the slice, one pixel or one image past the tensor destroys a sentinel;
  * the operands are integers and dyadic numbers whose every intermediate and partial sum is exact in fp32 (ew_cases.exact_bound), so the
    result is compared with the fp64 reference exactly: a value for a value, NaN for NaN; a bf16 output is the exact value rounded once;
    no input buffer changes a bit;
  * reductions: the partial rows are folded in fp64 over `rows` and compared exactly (how the sums are dealt to the rows is not part of the
    contract).  bn_finalize and bn_bwd_finalize are fed those exact partials: dgamma and dbeta are compared exactly, save_mean, c1 and c2
    exactly where the quotient is an fp32 number (elsewhere: its rounding, within one ulp), and scale, shift, invstd and the running
    statistics at 4 fp32 ulp of the largest term of
    the fp64 expression they come from -- one fp64 -> fp32 rounding plus at most two fp32 operations, contracted or not, each of them at most
    half an ulp of a term no larger than that one, with room for the rounding of an intermediate to carry into the next operation;
    num_batches_tracked goes up by one;
  * the same launch on Gaussian operands at the tolerances of test_batchnorm_train_fwd_bwd, test_maxpool, test_avgpool_ceil,
    test_shuffle_blur, test_resize_nearest, test_layout_and_slices (fp32) and test_elementwise_twins_bf16 (bf16);
  * a second launch of the exact operands into fresh outputs gives identical bits.

The test id names the op, the storage type, the kernel form (ew_cases.form) and the shape."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import ew_cases as ec  # noqa: E402
from ew_cases import CASES, case_id, has  # noqa: E402
from guard import guarded  # noqa: E402

NAN = float("nan")
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _bits(t):
    return t.view(_INT[t.element_size()])


def _flat(n, dtype, fill):
    """a guard-banded 1-D buffer whose start stays 16-byte aligned whatever n is"""
    return guarded((n,), dtype, fill=fill, guard=ec.rup(max(n, 32768), 64))


def _vector(v, fill=None):
    t, check = _flat(v.numel(), v.dtype, ec.canary(torch.float32) if fill is None else fill)
    t.copy_(v)
    return t, check


def _same(got, ref, what):
    """exactly the reference: a value for a value (-0.0 is 0.0), NaN for NaN"""
    got, ref = got.double(), ref.double().to(got.device)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~((got == ref) | (got.isnan() & ref.isnan()))
    if not bool(bad.any()):
        return
    first = bad.nonzero()[0].tolist()
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the fp64 reference, {int((got.isnan() & ~ref.isnan()).sum())} "
                         f"of them NaN; first at {first}: got {got[tuple(first)].item()!r}, expected {ref[tuple(first)].item()!r}")


def _close(got, ref, tol, what):
    got, ref = got.double(), ref.double().to(got.device)
    if tol is None:
        return _same(got, ref, what)
    rtol, atol = tol
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"{what}: max abs err {err:.3e} at scale {scale:.3e}, bound {rtol * scale + atol:.3e}")
    assert err <= rtol * scale + atol and math.isfinite(err), f"{what}: max abs err {err:.3e} over the bound {rtol * scale + atol:.3e} at scale {scale:.3e}"


def _ulp32(v):
    """the spacing of fp32 at |v|"""
    v = v.double().abs().clamp_min(2.0 ** -126)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.floor(torch.log2(v)) - 23)


def _within(got, want, largest, what, ulps=4):
    got, want = got.double().cpu(), want.double()
    err, bound = (got - want).abs(), ulps * _ulp32(largest)
    print(f"{what}: max err {(err / _ulp32(largest)).max().item():.2f} ulp of the largest term")
    assert bool((err <= bound).all()), f"{what}: {(err / _ulp32(largest)).max().item():.2f} ulp of the largest term, over {ulps}"


def _quotient(got, want, what):
    """exact where the fp64 quotient is an fp32 number, else its rounding"""
    got, want = got.double().cpu(), want.double()
    rep = want.float().double() == want
    assert torch.equal(got[rep], want[rep]), what
    _within(got, want, want, what, ulps=1)


# the Gaussian run: (rtol, atol) of tests.util.assert_close as the named tests state them; None: equal
_TOL_F32 = {("affine_act", "y"): (1e-5, 1e-5), ("bn_bwd_apply", "dx"): (2e-4, 1e-5), ("maxpool", "y"): None, ("maxpool", "dx"): (1e-6, 1e-6),
            ("avgpool", "y"): (1e-6, 1e-6), ("avgpool", "dx"): (1e-6, 1e-6), ("shuffle", "X"): (1e-6, 1e-6), ("shuffle", "dyc"): (1e-5, 1e-6),
            ("resize", "y"): None, ("resize", "dx"): (1e-6, 1e-6), ("relu_mask", "y"): None}
_SELECTS = {("maxpool", "y"), ("resize", "y"), ("relu_mask", "y")}          # bf16: values are passed on, not computed


def _tol(c, name, ref):
    copies = (c.op, name) in _SELECTS or (c.op == "copy_slice" and not has(c, "accumulate")) or \
        (c.op == "bn_bwd_apply" and name == "gout" and not has(c, "g_acc"))
    if copies:
        return None
    if c.dtype == "bf16":                                  # test_elementwise_twins_bf16: one output rounding
        return (2.0 ** -8, 1e-6)
    if c.op == "copy_slice" or name == "gout":             # test_layout_and_slices: "copy accumulate"
        return (1e-6, 1e-6)
    return _TOL_F32[(c.op, name)]


def _sum_tol(c):
    if c.op == "bn_bwd_reduce":                            # test_batchnorm_train_fwd_bwd dgamma / dbeta; test_elementwise_twins_bf16
        return (2e-4, 1e-4) if c.dtype == "f32" else (1e-5, 0.0)
    return (1e-5, 1e-5)                                    # test_layout_and_slices: colsum


class Launch:
    """the device operands of one case (built once per operand set) and its launches into fresh outputs"""

    def __init__(self, c, host, what):
        from unet_amd import ops
        self.c, self.host, self.what, self.ops = c, host, what, ops
        self.lay = ec.layout(c)
        self.ts, self.vec, self.checks = {}, {}, {}
        for name, role, shape, dt in ec.operands(c):
            if role == "in":
                self.ts[name], self.checks[name] = ec.device_slice(host[name], *self.lay[name], dt)
                assert self.ts[name].ptr % 16 == 0 and tuple(self.ts[name].buf.shape[:3]) == shape[:3], name
        for k, v in host.items():
            if torch.is_tensor(v) and v.dim() == 1:
                self.vec[k], self.checks[k] = _vector(v)
                assert self.vec[k].data_ptr() % 16 == 0
        self.before = {k: _bits(b).clone() for k, b in self._inputs().items()}

    def _inputs(self):
        return {**{k: t.buf for k, t in self.ts.items()}, **self.vec}

    def run(self, stage):
        """one launch (pair) into fresh outputs: ({output: TS}, {output: its buffer before the launch}, {partial | ws | total | idx: tensor})
        after checking every guard band and that no input changed"""
        c, ops, host = self.c, self.ops, self.host
        what = f"{self.what}: {stage}"
        out, init, res, checks = {}, {}, {}, dict(self.checks)
        for name, role, shape, dt in ec.operands(c):
            if role != "in":
                out[name], checks[name] = ec.output_slice(shape, *self.lay[name], dt, init=host[name + "0"] if role == "acc" else None)
                assert out[name].ptr % 16 == 0, name
                init[name] = out[name].buf.clone()
        T, V = {**self.ts, **out}, self.vec
        P, op = c.N * c.H * c.W, c.op
        acc = has(c, "accumulate")
        if op == "affine_act":
            ops.affine_act(T["x"], T["y"], V["scale"], V["shift"], x2=T.get("x2"), scale2=V.get("scale2"), shift2=V.get("shift2"), relu=has(c, "relu"))
        elif op in ("bn_stats", "bn_bwd_reduce"):
            rows = ops.bn_stats_rows(P)
            assert rows == ec.stats_rows(P)
            res["partial"], checks["partial"] = _flat(2 * rows * c.C, torch.float32, NAN)
            if op == "bn_stats":
                ops.bn_stats(T["x"], res["partial"])
            else:
                ops.bn_bwd_reduce(T["dout"], T.get("out"), T["x"], V["mean"], V["invstd"], res["partial"])
        elif op == "bn_bwd_apply":
            ops.bn_bwd_apply(T["dout"], T.get("out"), T["x"], V["mean"], V["invstd"], V["gamma"], V["c1"], V["c2"], T["dx"], gout=T.get("gout"),
                             g_accumulate=has(c, "g_acc"))
        elif op == "maxpool":
            if has(c, "idx"):
                res["idx"], checks["idx"] = _flat(math.prod(ec._shape(c, "y")), torch.uint8, 255)
            ops.maxpool(T["x"], T["y"], res.get("idx"))
            if has(c, "idx"):
                ops.maxpool_bwd(T["dy"], res["idx"], T["dx"], accumulate=acc)
        elif op == "avgpool":
            ops.avgpool(T["x"], T["y"])
            ops.avgpool_bwd(T["dy"], T["dx"], accumulate=acc)
        elif op == "shuffle":
            ops.shuffle_blur(T["yc"], T["X"], has(c, "blur"))
            ops.shuffle_blur_bwd(T["dX"], T["yc"], T["dyc"], has(c, "blur"))
        elif op == "resize":
            ops.resize_nearest(T["x"], T["y"])
            ops.resize_nearest_bwd(T["dy"], T["dx"])
        elif op == "copy_slice":
            ops.copy_slice(T["x"], T["y"], accumulate=acc)
        elif op == "relu_mask":
            ops.relu_mask(T["g"], T["ref"], T["y"])
        elif op == "cast_slice":
            ops.cast_slice(T["x"], T["y"])
        elif op in ("colsum", "dot"):
            rows, Cp = ops.bn_stats_rows(P), ec.rup(c.C, 4)
            assert rows == ec.stats_rows(P) and ops.colsum_workspace(P, c.C) == rows * Cp
            res["ws"], checks["workspace"] = _flat(rows * Cp, torch.float32, NAN)
            res["total"], checks["result"] = _flat(c.C if op == "colsum" else 1, torch.float32, NAN)
            if op == "colsum":
                ops.colsum(T["x"], res["total"], res["ws"])
            else:
                ops.dot(T["x"], T["y"], res["total"], res["ws"])
        else:
            raise KeyError(op)
        torch.cuda.synchronize()
        for name, check in checks.items():
            check(f"{what}: {name}")
        for k, b in self._inputs().items():
            assert torch.equal(_bits(b), self.before[k]), f"{what}: the launch changed its input {k}"
        return out, init, res

    def outside_untouched(self, out, init, stage):
        """every channel beside the slice still holds the bits it started with"""
        for name, ts in out.items():
            keep = torch.ones(ts.cs, dtype=torch.bool, device=ts.buf.device)
            keep[ts.co:ts.co + ts.C] = False
            assert torch.equal(_bits(ts.buf)[..., keep], _bits(init[name])[..., keep]), f"{self.what}: {stage}: stored beside the slice of {name}"

    def folded(self, res):
        """{sum0, sum1 | total}: the partial rows folded in fp64"""
        c = self.c
        P = c.N * c.H * c.W
        rows = ec.stats_rows(P)
        if "partial" in res:
            assert not bool(res["partial"].isnan().any()), f"{self.what}: a partial row was not written"
            s = res["partial"].view(2, rows, c.C).double().sum(1)
            return dict(sum0=s[0], sum1=s[1])
        ws = res["ws"].view(rows, ec.rup(c.C, 4)).double()
        assert not bool(ws.isnan().any()), f"{self.what}: a partial row was not written"
        assert bool((ws[:, c.C:] == 0).all()), f"{self.what}: pad lanes of the partial rows"
        f = dict(sum0=ws.sum(0)[:c.C])
        if c.op == "dot":
            f["total"] = res["total"].double()[0]
        else:
            f["result"] = res["total"].double()
        return f

    def compare(self, out, res, ref, exact, stage):
        c = self.c
        what = f"{self.what}: {stage}"
        for name, _role, _shape, dt in ec.operands(c):
            if name in out:
                want = ec.stored(dt, ref[name]) if exact else ref[name]
                _close(out[name].view(), want, None if exact else _tol(c, name, ref[name]), f"{what}: {name}")
        if "idx" in res and res["idx"] is not None:
            assert torch.equal(res["idx"].view(ref["idx"].shape).cpu(), ref["idx"]), f"{what}: index codes"
        if c.op in ec.REDUCTION_OPS:
            f = self.folded(res)
            tol = None if exact else _sum_tol(c)
            for k in ("sum0", "sum1"):
                if k in ref:
                    _close(f[k], ref[k], tol, f"{what}: {k} folded over the rows")
            if c.op == "colsum":
                _close(f["result"], ref["sum0"].float() if exact else ref["sum0"], tol, f"{what}: colsum")
            if c.op == "dot":
                _close(f["total"], ref["total"].float() if exact else ref["total"], tol, f"{what}: dot")

    # ---- the finalize kernels behind the two BatchNorm reductions, fed the exact partials of this case

    def finalize(self, res, ref):
        c, ops = self.c, self.ops
        C, P = c.C, c.N * c.H * c.W
        rows = ec.stats_rows(P)
        part = res["partial"]
        s, q = ref["sum0"], ref["sum1"]
        checks = {}

        def fresh(n=C):
            t, checks[len(checks)] = _flat(n, torch.float32, NAN)
            return t
        if c.op == "bn_stats":
            g = torch.Generator().manual_seed(77)
            host = dict(gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g), rm=torch.randn(C, generator=g) * 0.1,
                        rv=torch.rand(C, generator=g) + 0.5)
            dev = {}
            for k, v in host.items():
                dev[k], checks[k] = _vector(v)
            scale, shift, smean, sinv = fresh(), fresh(), fresh(), fresh()
            tracked = torch.full((), 7, dtype=torch.int64, device="cuda")
            ops.bn_finalize(part, part[rows * C:], rows, P, C, dev["gamma"], dev["beta"], dev["rm"], dev["rv"], ec.MOMENTUM, ec.EPS, scale, shift,
                            smean, sinv, tracked)
            torch.cuda.synchronize()
            f = ec.bn_finalize_ref(s, q, P, host["gamma"], host["beta"], host["rm"], host["rv"])
            m, gm, bt = f["m"], host["gamma"].double(), host["beta"].double()
            what = f"{self.what}: bn_finalize"
            assert int(tracked.item()) == 8, f"{what}: num_batches_tracked"
            _quotient(smean, f["mean"], f"{what}: save_mean")
            _within(sinv, f["invstd"], f["invstd"], f"{what}: save_invstd")
            _within(scale, f["scale"], gm * f["invstd"], f"{what}: scale")
            _within(shift, f["shift"], torch.maximum(bt.abs(), (f["mean"] * f["scale"]).abs()), f"{what}: shift")
            _within(dev["rm"], f["running_mean"], torch.maximum(((1 - m) * host["rm"].double()).abs(), (m * f["mean"]).abs()), f"{what}: running_mean")
            _within(dev["rv"], f["running_var"], torch.maximum(((1 - m) * host["rv"].double()).abs(), (m * f["unbiased"]).abs()), f"{what}: running_var")
            for k in ("gamma", "beta"):
                assert torch.equal(dev[k].cpu(), host[k]), f"{what}: changed {k}"
                checks.pop(k)("")
            for k in ("rm", "rv"):
                checks.pop(k)(f"{what}: {k}")
        else:
            dgamma, dbeta, c1, c2 = fresh(), fresh(), fresh(), fresh()
            ops.bn_bwd_finalize(part, rows, P, C, dgamma, dbeta, c1, c2)
            torch.cuda.synchronize()
            what = f"{self.what}: bn_bwd_finalize"
            _same(dbeta, s, f"{what}: dbeta")
            _same(dgamma, q, f"{what}: dgamma")
            _quotient(c1, s / P, f"{what}: c1")
            _quotient(c2, q / P, f"{what}: c2")
        for k, check in checks.items():
            check(f"{self.what}: finalize output {k}")


@pytest.mark.parametrize("i", range(len(CASES)), ids=[case_id(i) for i in range(len(CASES))])
def test_ew_case(i):
    c = CASES[i]
    what = case_id(i)
    assert ec.form(c) in what
    # ---- exact operands: the fp64 reference, value for value; then the same bits again
    host = ec.exact_inputs(c, i)
    ref = ec.reference(c, host)
    run = Launch(c, host, what)
    out, init, res = run.run("exact")
    run.compare(out, res, ref, True, "exact")
    run.outside_untouched(out, init, "exact")
    if c.op in ("bn_stats", "bn_bwd_reduce"):
        run.finalize(res, ref)
    out2, init2, res2 = run.run("repeat")
    for name in out:
        assert torch.equal(_bits(out2[name].buf), _bits(out[name].buf)), f"{what}: {name} differs between two launches"
    for k, t in res.items():
        assert torch.equal(_bits(res2[k]), _bits(t)), f"{what}: {k} differs between two launches"
    del run, out, out2, res, res2
    # ---- Gaussian operands at the tolerances of the first unit tests
    host = ec.gauss_inputs(c, 1000 + i)
    ref = ec.reference(c, host)
    run = Launch(c, host, what)
    out, init, res = run.run("gauss")
    run.compare(out, res, ref, False, "gauss")
    run.outside_untouched(out, init, "gauss")
