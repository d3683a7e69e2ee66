"""The weight-gradient case table of tests/wgrad_cases.py, without a GPU:

  * the planner mirror agrees with the library on the one number the library reports, the workspace size, for every case and for a wide
    random sweep of geometries and switches (small and full-size problems: the 3 GFLOP threshold of the 1x1 GEMM kernel and the
    256-workgroup rule of the bf16 3x3 launches only show at full size);
  * the table reaches every kernel instantiation, reduce kernel, partial-image count and plan edge that test_wgrad_gpu.py is there for,
    so that an edit of the table cannot silently lose one;
  * every case keeps the exactness bound of its integer operands, and their fp64 reference is integer-valued.
"""
import ctypes as C
import random
import sys
from pathlib import Path

import pytest
import torch

import wgrad_cases as wc
from wgrad_cases import CASES, Case, plan

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def L():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    ge.build()
    import unet_amd._lib as lib
    return lib


def _lib_workspace(L, c, tuning):
    fake = 0x100000            # never dereferenced: the query only plans
    t = L.Tuning.default(**tuning)
    OH, OW = wc.out_hw(c)
    x_co, x_cs, dy_co, dy_cs = wc.strides(c)
    d = L.WgradDesc()
    for k, v in dict(x=fake, x_cs=x_cs, x_co=x_co, dy=fake, dy_cs=dy_cs, dy_co=dy_co, dw=fake, N=c.N, IH=c.H, IW=c.W, Cin=c.Cin, OH=OH, OW=OW,
                     Cout=c.Cout, ks=c.ks, stride=c.stride, dtype=L.BF16 if c.dtype == "bf16" else L.F32).items():
        setattr(d, k, v)
    d.tuning = C.pointer(t)
    return int(L.lib.unet_conv2d_wgrad_workspace(C.byref(d)))


def test_defaults_are_the_library_defaults(L, monkeypatch):
    monkeypatch.delenv("UNET_WGRAD_WGS", raising=False)
    t = L.Tuning.default()
    got = {k: getattr(t, k) for k in wc.DEFAULTS}
    if got["wgrad_wgs"] != wc.DEFAULTS["wgrad_wgs"]:       # (the library read UNET_WGRAD_WGS when it was loaded: not this table's business)
        got["wgrad_wgs"] = wc.DEFAULTS["wgrad_wgs"]
    assert got == wc.DEFAULTS


def test_mirror_matches_the_library_on_every_case(L):
    for i, c in enumerate(CASES):
        tune = dict(wc.DEFAULTS)
        tune.update(c.tuning)
        assert _lib_workspace(L, c, tune) == wc.workspace_floats(c, plan(c)), wc.case_id(i)


def test_mirror_matches_the_library_on_a_random_sweep(L):
    rnd = random.Random(20240611)
    chans = [1, 3, 4, 5, 8, 9, 12, 13, 16, 17, 31, 32, 33, 36, 48, 63, 64, 65, 70, 80, 81, 96, 97, 100, 101, 112, 113, 127, 128, 129, 130, 192,
             224, 225, 230, 256, 300, 384, 508, 509, 512, 513, 516, 1024]
    sizes = [1, 2, 3, 4, 5, 7, 8, 9, 13, 15, 16, 17, 19, 31, 32, 33, 37, 40, 56, 63, 64, 65, 70, 128, 129, 256]
    n = 0
    for _ in range(6000):
        ks, stride = rnd.choice([(3, 1), (3, 1), (3, 2), (1, 1)])
        c = Case(rnd.choice([1, 2, 3, 5, 16, 33]), rnd.choice(sizes), rnd.choice(sizes), rnd.choice(chans), rnd.choice(chans), ks, stride,
                 rnd.choice(["f32", "bf16"]), rnd.choice(wc.LAYOUTS), ())
        if wc.pixels(c) == 0:
            continue
        tune = dict(wgrad_mfma_shape=rnd.choice([32, 32, 16]), wgrad_bf16_k4=rnd.choice([1, 0]), wgrad_1x1=rnd.choice([1, 1, 0, 2]),
                    wgrad_narrow=rnd.choice([1, 1, 0, 2, 3]), wgrad_wgs=rnd.choice([0, 0, 0, 1, 7, 8, 9, 31, 32, 33, 100, 256, 700, 5000]))
        assert _lib_workspace(L, c, tune) == wc.workspace_floats(c, plan(c, tune)), (c, tune, plan(c, tune))
        n += 1
    assert n > 5000


def test_table_covers_every_kernel_and_plan_edge():
    plans = [plan(c) for c in CASES]
    both = list(zip(CASES, plans))
    fam = {p["family"] for p in plans}
    forms = [(ptw, s, ks) for ptw in (8, 16, 32) for s, ks in ((1, 1), (1, 3), (2, 3))]
    want = {f"{k}<{a},{b},{c}>" for k in ("wgrad", "wgrad16", "bf16") for a, b, c in forms}
    want |= {"flat<6,7>", "flat<7,5>", "flat<6,5,sliver>", "gemm1x1"} | {f"small1x1<{k}>" for k in (1, 2, 3, 4)}
    want |= {f"bf16_k4<{kv},{ks}>" for kv in (1, 2, 3, 4) for ks in (1, 3)}
    assert fam == want, (sorted(want - fam), sorted(fam - want))

    def some(pred, what):
        assert any(pred(c, p) for c, p in both), f"no case with {what}"

    def is_(prefix):
        return lambda c, p: p["family"].startswith(prefix + "<") or p["family"] == prefix

    # every operand is a slice with a neighbour behind it, and offsets of zero and above occur on both operands
    for c in CASES:
        x_co, x_cs, dy_co, dy_cs = wc.strides(c)
        v = wc.vec_of(c.dtype)
        assert x_cs > x_co + wc.rup(c.Cin, v) and dy_cs > dy_co + wc.rup(c.Cout, v) and x_co % v == 0 and dy_co % v == 0
    for k in ("wgrad", "wgrad16", "flat", "gemm1x1", "small1x1", "bf16", "bf16_k4"):
        fams = [(c, p) for c, p in both if p["family"].split("<")[0] == k]
        assert any(c.layout[0] > 0 for c, _ in fams) and any(c.layout[2] > 0 for c, _ in fams) and any(c.layout[0] == 0 for c, _ in fams), k

    assert {p["reduce"] for p in plans} == {"rows", "q8", "q4", "plain"}
    assert {p["nsub"] for p in plans} == {1, 2, 4}
    # wgrad / wgrad16 / bf16: the channel pairs on both sides of the 64-wide block and its 32-wide halves, in all nine forms
    for k in ("wgrad", "bf16"):
        for a, b, c_ in forms:
            got = {(c.Cin, c.Cout) for c, p in both if p["family"] == f"{k}<{a},{b},{c_}>"}
            assert {(3, 32), (32, 100), (100, 32), (65, 63), (100, 100)} <= got, (k, a, b, c_)
    got16 = {(c.Cin, c.Cout) for c, p in both if p["family"].startswith("wgrad16<")}
    assert {(3, 32), (32, 100), (100, 32), (65, 63), (100, 100)} <= got16
    for k in ("wgrad", "wgrad16", "bf16"):
        some(lambda c, p: is_(k)(c, p) and wc.out_hw(c)[0] < p["pth"], f"{k}: an output shorter than the tile")
        some(lambda c, p: is_(k)(c, p) and wc.out_hw(c)[0] > p["pth"] and wc.out_hw(c)[0] % p["pth"], f"{k}: a ragged second tile row")
        some(lambda c, p: is_(k)(c, p) and c.stride == 2 and c.H % 2 == 1 and c.W % 2 == 1, f"{k}: odd extents at stride 2")
        some(lambda c, p: is_(k)(c, p) and c.stride == 2 and c.W % 2 == 0, f"{k}: an even width at stride 2")
        assert {wc.out_hw(c)[1] for c, p in both if is_(k)(c, p)} >= {7, 19, 37}
    assert {(c.Cin <= 32, c.Cout <= 32) for c, p in both if is_("wgrad")(c, p)} == {(True, True), (True, False), (False, True), (False, False)}

    # flat: every output-tile form at the channel counts on both sides of its edges, short chunks, images of 1 / 2 / 3 / 5 rows
    flat = [(c, p) for c, p in both if is_("flat")(c, p)]
    assert {c.Cout for c, _ in flat} == {81, 96, 97, 100, 101, 112}
    assert any(c.Cout == 100 and p["family"] == "flat<7,5>" for c, p in flat)
    assert {c.Cin for c, _ in flat} == {9, 36, 112, 113, 230}
    assert {c.H for c, _ in flat} == {1, 2, 3, 5} and {c.W for c, _ in flat} == {32, 33, 40, 64}
    assert all(c.N >= 2 for c, _ in flat)
    assert {p["chunks"] for _, p in flat} == {1, 2, 3} and any(p["last_chunk"] < p["cw"] for _, p in flat)
    assert all(p["tpb"] > c.H or p["tpb"] % c.H for c, p in flat)                          # blocks whose tiles cross a column strip ...
    assert any(p["tpb"] % (c.H * wc.cdiv(c.W, 32)) and p["splits"] > 1 for c, p in flat)       # ... and split an image
    assert {7, 8, 9} <= {p["splits"] for _, p in flat} and any(p["grid_y"] - p["splits"] >= 7 for _, p in flat)

    # gemm1x1: ragged pixel tiles and channel counts around its 128-wide block
    gemm = [(c, p) for c, p in both if p["family"] == "gemm1x1"]
    assert all(p["P"] % 64 for _, p in gemm) and any(p["P"] < 64 for _, p in gemm) and any(p["splits"] > 1 for _, p in gemm)
    assert {c.Cin for c, _ in gemm} >= {127, 129, 130, 70} and {c.Cout for c, _ in gemm} >= {127, 129, 130, 70}

    # small1x1: output channel counts on both sides of every K4, the three input widths, the LDS cap, ragged pixel ranges; 516 leaves
    small = [(c, p) for c, p in both if is_("small1x1")(c, p)]
    assert {c.Cout for c, _ in small} == {1, 4, 5, 8, 9, 12, 13, 16} and {c.Cin for c, _ in small} == {3, 100, 512}
    assert {(c.Cin, p["lds_capped"]) for c, p in small} >= {(3, True), (3, False), (100, True), (512, True), (512, False)}
    assert {p["ps"] for _, p in small} >= {256, 204, 10, 2, 1}
    assert any(p["P"] < p["ps"] * 64 for _, p in small) and any(p["splits"] > 1 and p["P"] % p["ppb"] for _, p in small)
    assert any(p["ppb"] % p["ps"] for _, p in small)
    some(lambda c, p: c.Cin == 516 and c.ks == 1 and c.Cout <= 16 and is_("wgrad")(c, p), "516 input channels on the general kernel")

    # bf16_k4: every width of the output-channel block
    k4 = {(c.Cout, p["family"]) for c, p in both if is_("bf16_k4")(c, p)}
    for cout, kv in ((16, 1), (24, 2), (40, 3), (64, 4), (80, 3), (100, 4), (112, 4)):
        assert any(co == cout and f.startswith(f"bf16_k4<{kv},") for co, f in k4), (cout, kv)
    assert {c.Cin for c, p in both if is_("bf16_k4")(c, p)} >= {8, 36, 100, 104}

    # split counts: both sides of the renumbered grid (8 splits) and of the reduce kernels (8 and 32 partial images)
    f32 = [p for c, p in both if c.dtype == "f32" and c[:4] == (346, 2, 9, 36)]
    assert [p["splits"] for p in f32] == [s for _, s in wc.SPLITS["f32"]] == [1, 7, 8, 9, 31, 32, 33]
    assert all(p["nsub"] == 1 and p["total_tiles"] >= 132 for p in f32)
    assert [p["reduce"] for p in f32] == ["plain", "plain", "q4", "q4", "q4", "q8", "q8"]
    b16 = [p for c, p in both if is_("bf16_k4")(c, p) and c[1:4] == (5, 33, 36)]
    assert [p["splits"] for p in b16] == [s for _, _, s in wc.SPLITS["bf16"]] == [1, 7, 8, 9, 31, 32, 33]
    assert [p["grid_y"] for p in b16] == [1, 7, 8, 16, 32, 32, 40]
    assert sorted(p["splits"] for c, p in both if is_("bf16")(c, p) and c[1:4] == (5, 33, 36)) == [7, 8, 9]
    sub4 = [p["slices"] for c, p in both if p["nsub"] == 4 and c.tuning and dict(c.tuning).get("wgrad_wgs")]
    assert sub4 == [4, 8, 28, 32, 36]
    assert any(p["splits"] == 1 for p in plans)


def test_every_case_keeps_the_exactness_bound():
    for i, c in enumerate(CASES):
        assert wc.exact_bound(c) < 2 ** 24, (wc.case_id(i), wc.exact_bound(c))
    assert wc.EXACT_RANGE["f32"] == (511, 2) and wc.EXACT_RANGE["bf16"] == (15, 3)
    # 511 needs nine significant bits: not a bf16 value, while every bf16-storage operand is one
    assert torch.tensor(511.0).to(torch.bfloat16).item() != 511.0
    r = torch.arange(-15, 16).float()
    assert torch.equal(r.to(torch.bfloat16).float(), r)


def test_exact_reference_is_integer_valued_and_in_range():
    for i, c in enumerate(CASES):
        if i % 4 and wc.pixels(c) * c.Cin * c.Cout > 5e7:         # (the fp64 conv of the larger cases on one in four)
            continue
        x, dy = wc.exact_inputs(c, i)
        mx, md = wc.EXACT_RANGE[c.dtype]
        assert x.abs().max() <= mx and dy.abs().max() <= md and torch.equal(x, x.round()) and torch.equal(dy, dy.round())
        dw, db = wc.reference(c, x, dy)
        assert torch.equal(dw, dw.round()) and torch.equal(db, db.round()), wc.case_id(i)
        assert dw.abs().max() + wc.PREFILL < 2 ** 24 and dw.abs().max() > 0
        assert tuple(dw.shape) == (c.Cout, c.Cin, c.ks, c.ks) and tuple(db.shape) == (c.Cout,)


def test_operand_slices_hold_data_zero_pads_and_canaries():
    import guard
    c = Case(2, 3, 5, 5, 9, 3, 1, "f32", (1, 1, 2, 1), ())
    x, dy = wc.exact_inputs(c, 0)
    for dt, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        cc = c._replace(dtype=name)
        x_co, x_cs, dy_co, dy_cs = wc.strides(cc)
        (xt, xcheck), (dyt, dycheck) = wc.operands(cc, x.clamp(-15, 15), dy, device="cpu")
        v = wc.vec_of(name)
        assert (xt.co, xt.cs, xt.C, dyt.co, dyt.cs, dyt.C) == (x_co, x_cs, 5, dy_co, dy_cs, 9) and xt.buf.dtype == dt
        assert torch.equal(xt.view().float(), x.clamp(-15, 15)) and torch.equal(dyt.view().float(), dy)
        canary = torch.tensor(guard.CANARY[torch.float32]).to(dt)
        for t in (xt, dyt):
            pad = t.buf[..., t.co + t.C:t.co + wc.rup(t.C, v)]
            assert pad.numel() and bool((pad == 0).all())
            rest = torch.cat([t.buf[..., :t.co], t.buf[..., t.co + wc.rup(t.C, v):]], dim=-1)
            assert rest.numel() and bool((rest == canary).all())
        xcheck("x")
        dycheck("dy")
