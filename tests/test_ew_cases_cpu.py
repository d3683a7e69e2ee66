"""What tests/ew_cases.py covers, as assertions (no GPU): every kernel form the dispatch code of csrc/elementwise.hip can select, every loop
state of the QuadWalk and of the reductions, every option both ways, exact operands for every case, bf16 results that need rounding, and the
fp64 reference against torch's own BatchNorm, autograd and its own adjoints."""
import pytest
import torch
import torch.nn.functional as F

import ew_cases as ec
from ew_cases import CASES, case_id, form, has, walk

IDS = [case_id(i) for i in range(len(CASES))]


def _some(pred, what):
    hit = [case_id(i) for i, c in enumerate(CASES) if pred(c)]
    assert hit, f"no case with {what}"
    return hit


# ------------------------------------------------------------------------------------------------------------------------ coverage

def test_table_size_and_ids():
    assert 150 <= len(CASES) <= 200, len(CASES)
    assert len(set(IDS)) == len(IDS)
    for c in CASES:
        assert c.C * c.N * c.H * c.W * (4 if c.op == "shuffle" else 1) <= 4_300_000, c          # the largest tensor: 4.2 M elements
        assert (c.to is not None) == (c.op == "resize")
        assert not has(c, "scale2") or has(c, "x2")
        assert not has(c, "g_acc") or has(c, "gout")
        assert not has(c, "accumulate") or c.op != "maxpool" or has(c, "idx")


def test_every_form_of_the_dispatch_is_hit():
    want = set()
    for op in ("affine_act", "bn_bwd_reduce", "bn_bwd_apply"):
        want |= {(op, "f32", "quad"), (op, "bf16", "quad"), (op, "bf16", "oct")}
    for op in ("bn_stats", "dot", "maxpool", "avgpool", "resize", "copy_slice", "relu_mask"):
        want |= {(op, "f32", "quad"), (op, "bf16", "quad")}
    want |= {("colsum", "f32", "quad"), ("cast_slice", "bf16", "quad")}
    got = {(c.op, c.dtype, form(c)) for c in CASES if c.op != "shuffle"}
    assert got == want, (want - got, got - want)
    for dt in ("f32", "bf16"):
        for blur in (False, True):
            forms = {form(c) for c in CASES if c.op == "shuffle" and c.dtype == dt and has(c, "blur") == blur}
            # the forward vec form runs without blur only; the adjoint has both forms either way
            assert forms == ({"scalar+scalar", "scalar+vec"} if blur else {"scalar+scalar", "vec+vec"}), (dt, blur, forms)
    # form selection by offset alone: the same bf16 shape and options in oct / vec form at 8-aligned offsets and in quad / scalar form at 4 mod 8
    for op in ("affine_act", "bn_bwd_reduce", "bn_bwd_apply"):
        by = {}
        for c in CASES:
            if c.op == op and c.dtype == "bf16" and c.C % 8 == 0:
                by.setdefault((c.N, c.H, c.W, c.C, c.opts), set()).add((c.lay, form(c)))
        assert any({("s8", "oct"), ("s4", "quad")} <= v for v in by.values()), op
    assert any(c.op == "shuffle" and c.dtype == "bf16" and c.C == 24 and c.lay == "s4" and form(c) == "scalar+scalar" for c in CASES)
    assert any(c.op == "shuffle" and c.dtype == "bf16" and c.C == 24 and c.lay == "s8" and form(c).endswith("vec") for c in CASES)
    # an oct form on a true slice, a bf16 quad form at an offset of 4 mod 8; one operand alone (offset, or channel stride) decides
    for op in ("affine_act", "bn_bwd_reduce", "bn_bwd_apply"):
        _some(lambda c: c.op == op and form(c) == "oct" and c.lay == "s8", f"{op} oct on a slice")
        _some(lambda c: c.op == op and c.dtype == "bf16" and c.C % 8 == 0 and form(c) == "quad" and c.lay == "s4", f"{op} bf16 quad at 4 mod 8")
    for op in ("affine_act", "bn_bwd_apply"):
        _some(lambda c: c.op == op and c.dtype == "bf16" and c.C % 8 == 0 and form(c) == "quad" and c.lay == "mix", f"{op}: one operand at 4 mod 8")
        _some(lambda c: c.op == op and c.dtype == "bf16" and c.C % 8 == 0 and form(c) == "quad" and c.lay == "cs4", f"{op}: strides 4 mod 8")


def test_quadwalk_states():
    for op in ec.QUADWALK_OPS:
        for dt, fm in {(c.dtype, form(c)) for c in CASES if c.op == op}:
            _some(lambda c: c.op == op and c.dtype == dt and form(c) == fm and walk(c)["carry"], f"{op} {dt} {fm}: QuadWalk carry")
            _some(lambda c: c.op == op and c.dtype == dt and form(c) == fm and not walk(c)["strides"], f"{op} {dt} {fm}: no striding")
        _some(lambda c: c.op == op and walk(c)["strides"] and not walk(c)["carry"] and walk(c)["cq"] == 16, f"{op}: striding without carry, Cq = 16")
    # the issue's shapes, by the arithmetic
    w = walk(ec._mk("affine_act", "f32", 2, 104, 104, 100))
    assert w == dict(cq=25, strides=True, carry=True)
    w = walk(ec._mk("affine_act", "bf16", 2, 148, 148, 96))
    assert w == dict(cq=12, strides=True, carry=True)
    assert walk(ec._mk("affine_act", "bf16", 2, 104, 104, 100, lay="s4"))["carry"]


def test_reduction_states():
    combos = {(c.op, c.dtype, form(c)) for c in CASES if c.op in ec.REDUCTION_OPS}
    assert ("bn_bwd_reduce", "bf16", "oct") in combos
    for op, dt, fm in sorted(combos):
        ws = [walk(c) for c in CASES if (c.op, c.dtype, form(c)) == (op, dt, fm)]
        what = f"{op} {dt} {fm}"
        assert any(w["unrolled"] > 0 and w["tail"] > 0 for w in ws), what
        assert any(w["unrolled"] == 0 and w["tail"] > 0 for w in ws), what
        assert {w["passes"] for w in ws} >= {1, 2}, what
        assert any(w["idle"] > 0 for w in ws) and any(w["idle"] == 0 for w in ws), what
        rows = {w["rows"] for w in ws}
        assert rows >= {1, 2, 512} and rows & set(range(25, 32)), (what, rows)
        if op != "dot" and fm != "oct":                 # (dot folds its partial rows in sum_all_kernel, not in rows_reduce2; C % 32 == 4 is no oct width)
            assert any(w["last_block"] == 4 for w in ws), what
    assert {walk(c)["rows"] for c in CASES if c.op == "bn_stats"} >= set(range(25, 32))        # each side of `r + 24 < rows`, for all 8 row lanes
    # the issue's shapes, by the arithmetic
    w = walk(ec._mk("bn_stats", "f32", 2, 104, 104, 100))
    assert (w["rows"], w["tc"], w["idle"], w["unrolled"], w["tail"], w["last_block"]) == (512, 32, 7, 1, 2, 4)
    w = walk(ec._mk("bn_bwd_reduce", "bf16", 2, 148, 148, 96))
    assert (w["cq"], w["tc"], w["unrolled"], w["tail"]) == (12, 16, 3, 1)
    w = walk(ec._mk("bn_bwd_reduce", "bf16", 2, 12, 20, 64))
    assert (w["rows"], w["unrolled"], w["tail"]) == (15, 0, 1)
    w = walk(ec._mk("bn_bwd_reduce", "bf16", 1, 5, 10, 1024))
    assert (w["passes"], w["idle"]) == (2, 0)
    w = walk(ec._mk("bn_bwd_reduce", "bf16", 1, 5, 10, 776))
    assert (w["passes"], w["idle"]) == (2, 31)
    w = walk(ec._mk("bn_stats", "f32", 1, 5, 10, 400))
    assert (w["passes"], w["tc"]) == (2, 64)
    assert walk(ec._mk("colsum", "f32", 1, 4, 5, 3))["tc"] == 1
    for P, rows in ((20, 1), (50, 2), (900, 29)):
        assert ec.stats_rows(P) == rows


def test_every_option_both_ways():
    takes = dict(relu=("affine_act",), x2=("affine_act",), scale2=("affine_act",), out=("bn_bwd_reduce", "bn_bwd_apply"), gout=("bn_bwd_apply",),
                 g_acc=("bn_bwd_apply",), accumulate=("maxpool", "avgpool", "copy_slice"), blur=("shuffle",), idx=("maxpool",))
    assert set(takes) == set(ec.OPT_NAMES)
    for opt, ops_ in takes.items():
        for op in ops_:
            for dt, fm in {(c.dtype, form(c)) for c in CASES if c.op == op}:
                if op == "shuffle":
                    fm = None
                for on in (True, False):
                    _some(lambda c: c.op == op and c.dtype == dt and (fm is None or form(c) == fm) and has(c, opt) == on,
                          f"{op} {dt} {fm}: {opt} {'on' if on else 'off'}")
    for c in CASES:
        assert all(any(c.op == op for op in takes[o]) for o in c.opts), c


def test_contiguous_and_sliced():
    for op in {c.op for c in CASES}:
        _some(lambda c: c.op == op and c.lay == "c", f"{op}: all operands contiguous")
        hit = _some(lambda c: c.op == op and c.lay in ec.SLICED, f"{op}: every operand a true slice")
        assert hit
    for c in CASES:
        for name, (co, cs) in ec.layout(c).items():
            C = ec._shape(c, name)[3]
            assert co % 4 == 0 and cs % 4 == 0 and co + ec.rup(C, 4) <= cs
            assert c.lay == "c" or (co > 0 and cs > co + ec.rup(C, 4)), (c, name)       # neighbours on both sides, behind the pad lanes


def test_minimum_shapes():
    def sides(op):
        return {(c.dtype, c.H, c.W) for c in CASES if c.op == op}
    for dt in ("f32", "bf16"):
        assert sides("maxpool") >= {(dt, 7, 7), (dt, 8, 8), (dt, 1, 5), (dt, 5, 1), (dt, 2, 2)}
        assert sides("avgpool") >= {(dt, 5, 7), (dt, 1, 1), (dt, 6, 6)}
        assert {(c.H, c.W, c.C, has(c, "blur")) for c in CASES if c.op == "shuffle" and c.dtype == dt} == {
            (h, w, cu, b) for (h, w) in ((1, 6), (6, 1), (5, 7)) for cu in (24, 20, 6) for b in (False, True)}
        assert {(c.H, c.to) for c in CASES if c.op == "resize" and c.dtype == dt} == {(26, 25), (50, 52), (1, 3)}


# ------------------------------------------------------------------------------------------------------------------------ exact operands

def _representable(t, dt):
    t = t.double()
    r = t.float().double() if dt == torch.float32 else t.float().to(torch.bfloat16).double()
    return (r == t) | t.isnan()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_exact_operands(i):
    """the bound of the operands actually built is below 2^24; every operand is representable in its storage type; the reference is exact in
    fp32; pool and blur results keep their quarter steps"""
    c = CASES[i]
    d = ec.exact_inputs(c, i)
    assert ec.exact_bound(c, d) < 2.0 ** 24
    for name, _role, shape, dt in ec.operands(c):
        if name in d:
            assert tuple(d[name].shape) == shape and bool(_representable(d[name], dt).all()), name
    for k, v in d.items():
        if torch.is_tensor(v) and v.dim() == 1:
            assert bool(_representable(v, torch.float32).all())
    for k, r in ec.reference(c, d).items():
        if r.dtype == torch.float64:
            assert bool(_representable(r, torch.float32).all()), k
    if c.op == "maxpool" and c.dtype == "f32":
        x = d["x"]
        assert int(x.isnan().sum()) == 1 and bool((x[0, :2, :2, 2] == float("-inf")).all()) and bool((x[~x.isnan()] < 0).all())


def _rounding(c, d):
    """(values of the bf16 outputs that bf16 cannot hold, exact ties among them)"""
    n = ties = 0
    for name, role, _shape, dt in ec.operands(c):
        if role == "in" or dt != torch.bfloat16:
            continue
        v = ec.reference(c, d)[name].flatten()
        v = v[v.isfinite()]
        r = v.float().to(torch.bfloat16).double()
        off = (v - r).abs()
        _m, e = torch.frexp(v)
        half = torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 9).double())          # half the spacing of bf16 at v
        n += int((off > 0).sum())
        ties += int(((off > 0) & (off == half)).sum())
    return n, ties


def test_bf16_results_need_rounding():
    """per arithmetic op, over its small bf16 cases: outputs that bf16 cannot hold, exact ties (such as 257, midway between 256 and 258) among them"""
    for op in ec.ARITHMETIC_OPS:
        n = ties = 0
        for i, c in enumerate(CASES):
            if c.op == op and c.dtype == "bf16" and c.N * c.H * c.W * c.C <= 100_000:
                a, b = _rounding(c, ec.exact_inputs(c, i))
                n, ties = n + a, ties + b
        assert n > 0 and ties > 0, (op, n, ties)
    assert ec.stored(torch.bfloat16, torch.tensor([257.0, 259.0], dtype=torch.float64)).tolist() == [256.0, 260.0]        # to nearest EVEN


# ------------------------------------------------------------------------------------------------------------------------ the reference against itself

def _rand_like(d, g):
    return {k: (torch.randn(v.shape, generator=g, dtype=torch.float64) if torch.is_tensor(v) else v) for k, v in d.items()}


@pytest.mark.parametrize("c", [ec._mk("maxpool", "f32", 2, 7, 8, 4, opts="idx"), ec._mk("maxpool", "f32", 2, 1, 5, 4, opts="idx"),
                               ec._mk("avgpool", "f32", 2, 5, 7, 4), ec._mk("avgpool", "f32", 2, 1, 1, 4), ec._mk("resize", "f32", 2, 26, 26, 4, to=25),
                               ec._mk("resize", "f32", 2, 5, 5, 4, to=13), ec._mk("shuffle", "f32", 2, 5, 7, 6), ec._mk("shuffle", "f32", 2, 5, 7, 6, opts="blur"),
                               ec._mk("shuffle", "f32", 2, 1, 6, 6, opts="blur"), ec._mk("shuffle", "f32", 2, 6, 1, 6, opts="blur")],
                         ids=lambda c: f"{c.op}-{c.H}x{c.W}-{'+'.join(c.opts)}")
def test_reference_adjoints(c):
    """<A x, y> = <x, A^T y> in fp64 on random operands (max pool: A = the selection the forward pass made)"""
    g = torch.Generator().manual_seed(3)
    d = _rand_like(ec.gauss_inputs(c, 1), g)
    if c.op == "shuffle":
        d["yc"] = d["yc"].abs() + 0.1                 # every ReLU gate open
    r = ec.reference(c, d)
    fwd, x, dy, adj = (("X", "yc", "dX", "dyc") if c.op == "shuffle" else ("y", "x", "dy", "dx"))
    lhs, rhs = (r[fwd] * d[dy]).sum().item(), (d[x] * r[adj]).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), (lhs, rhs)


def test_reference_batchnorm_is_torchs():
    """affine_act o bn_finalize reproduces F.batch_norm(training=True) in fp64, running statistics included; bn_bwd_reduce -> finalize ->
    bn_bwd_apply reproduces its autograd gradients"""
    g = torch.Generator().manual_seed(5)
    N, H, W, C = 3, 5, 7, 8
    P = N * H * W
    x = (torch.randn(N, H, W, C, generator=g, dtype=torch.float64) * 2 + 0.5)
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    c = ec._mk("bn_stats", "f32", N, H, W, C)
    s = ec.reference(c, dict(x=x))
    f = ec.bn_finalize_ref(s["sum0"], s["sum1"], P, gamma, beta, rm, rv)
    y = ec.reference(ec._mk("affine_act", "f32", N, H, W, C), dict(x=x, scale=f["scale"], shift=f["shift"]))["y"]
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm2, rv2 = rm.clone(), rv.clone()
    want = F.batch_norm(xn, rm2, rv2, gm, bt, training=True, momentum=f["m"], eps=torch.tensor(ec.EPS, dtype=torch.float32).double().item())
    assert (ec._h(want.detach()) - y).abs().max().item() <= 1e-12
    assert (rm2 - f["running_mean"]).abs().max().item() <= 1e-13 and (rv2 - f["running_var"]).abs().max().item() <= 1e-13
    dout = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    want.backward(ec._n(dout))
    ops_ = dict(dout=dout, x=x, mean=f["mean"], invstd=f["invstd"])
    r = ec.reference(ec._mk("bn_bwd_reduce", "f32", N, H, W, C), ops_)
    assert (r["sum0"] - bt.grad).abs().max().item() <= 1e-12 and (r["sum1"] - gm.grad).abs().max().item() <= 1e-11
    dx = ec.reference(ec._mk("bn_bwd_apply", "f32", N, H, W, C), dict(ops_, gamma=gamma, c1=r["sum0"] / P, c2=r["sum1"] / P))["dx"]
    assert (dx - ec._h(xn.grad)).abs().max().item() <= 1e-12


@pytest.mark.parametrize("hw", [(7, 7), (8, 8), (1, 5), (5, 1), (2, 2)])
def test_index_code_round_trip(hw):
    """the code derived from torch's flat index names the winner (first in row-major scan order on ties, a NaN takes over, an all -inf window
    keeps its first tap): scattering dy by code equals autograd's x.grad, and gathering x by code gives the pooled values"""
    H, W = hw
    c = ec._mk("maxpool", "f32", 2, H, W, 4, opts="idx")
    d = ec.exact_inputs(c, 7)
    r = ec.reference(c, d)
    code, x = ec._n(r["idx"]), ec._n(d["x"].double())
    dx = ec.scatter_by_code(ec._n(d["dy"].double()), code, H, W)
    assert torch.equal(ec._h(dx), r["dx"])
    OH, OW = code.shape[2:]
    oy, ox = torch.arange(OH).view(1, 1, OH, 1), torch.arange(OW).view(1, 1, 1, OW)
    iy, ix = 2 * oy - 1 + code.long() // 3, 2 * ox - 1 + code.long() % 3
    assert bool(((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).all())
    got = x.reshape(2, 4, -1).gather(2, (iy * W + ix).reshape(2, 4, -1)).view(2, 4, OH, OW)
    y = ec._n(r["y"])
    assert bool(((got == y) | (got.isnan() & y.isnan())).all())
    # first on ties: no earlier tap of the window holds the same value
    xp = F.pad(x, (1, 1, 1, 1), value=float("-inf"))
    for k in range(9):
        tap = xp[:, :, k // 3:k // 3 + 2 * OH:2, k % 3:k % 3 + 2 * OW:2][:, :, :OH, :OW]
        inside = ((2 * oy - 1 + k // 3 >= 0) & (2 * oy - 1 + k // 3 < H) & (2 * ox - 1 + k % 3 >= 0) & (2 * ox - 1 + k % 3 < W)).expand_as(tap)
        earlier = (k < code.long()) & inside & ~y.isnan()
        assert not bool((earlier & (tap == y) & (y != float("-inf"))).any())
        assert not bool((earlier & (y == float("-inf"))).any()), "an all -inf window keeps its first tap"
