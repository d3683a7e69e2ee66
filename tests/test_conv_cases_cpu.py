"""The forward / dgrad conv case table of tests/conv_cases.py, without a GPU:

  * every case states what the library plans for it: unet_conv2d_variant, unet_conv2d_splitk_workspace and unet_conv2d_colsum_rows are
    asked again here, over fake aligned addresses (tests/test_conv_dispatch_cpu.py pins those three against the parent build);
  * the table reaches every class of launches and every kernel instantiation, tail, split and edge that tests/test_conv_gpu.py is there
    for -- each assertion a loop over the table, so that a case deleted later fails here by name;
  * the integer operands of every case keep the exactness condition (computed from the operands actually built), and the fp32 ones carry
    the 13-bit values in every kernel family.
"""
import json
import sys
import time
from pathlib import Path

import pytest
import torch

import conv_cases as cc
import conv_plan_cases as P
from conv_cases import CASES, cdiv, family, has, kernels, splits_of

ROOT = Path(__file__).resolve().parent.parent
BOTH = ("f32", "bf16")
KINDS = ("fwd", "dgrad")
TY = {"f32": "float", "bf16": "bf16"}


@pytest.fixture(scope="module")
def L():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    ge.build()
    import unet_amd._lib as lib
    return lib


def ids(pred):
    return [cc.case_id(i) for i, c in enumerate(CASES) if pred(c)]


def some(pred, what):
    assert any(pred(c) for c in CASES), f"no case with {what}"


def klass(c):
    return (0 if c.dtype == "f32" else 1, 0 if c.kind == "fwd" else 1, c.variant % 1000000, c.variant >= 1000000)


# ------------------------------------------------------------------------------------------------------------------------ the stated plans

def test_every_case_states_what_the_library_plans(L):
    bad = []
    for i, c in enumerate(CASES):
        got = cc.query(L, c)
        if got != [c.variant, c.ws_floats, c.rows]:
            bad.append(f"{cc.case_id(i)}: the library answers (variant, workspace floats, colsum rows) = {got}")
        if c.ws != "exact":         # the plan splits, and without the whole workspace the launch runs the unsplit plan
            full = cc.query(L, c, ws="exact")
            assert full[0] >= 2000000 and c.ws_floats > 0 and 0 <= c.variant < 1000000 and full[0] % 1000000 != 0, cc.case_id(i)
    assert not bad, f"{len(bad)} of {len(CASES)} cases\n" + "\n".join(bad[:20])


def test_ids_are_unique_and_name_family_and_variant():
    all_ids = [cc.case_id(i) for i in range(len(CASES))]
    assert len(set(all_ids)) == len(all_ids)
    assert len(set(CASES)) == len(CASES), "a case appears twice"
    for i, c in enumerate(CASES):
        assert f"-v{c.variant}-" in all_ids[i] and all(k in all_ids[i] for k in kernels(c))
        assert c.variant >= 0 and family(c) in ("gemm1x1", "smallk", "smallcin", "head1x1", "t256", "generic")
        assert c.ws in ("exact", "short", "none") and all(e in cc.EP_NAMES for e in c.ep)


def test_cases_are_small():
    wide = []
    for i, c in enumerate(CASES):
        assert 1 <= c.N <= 3, cc.case_id(i)
        assert c.H <= 40, cc.case_id(i)
        if c.W > 40:
            wide.append(c)
        if c.Cin > 256:             # the deep reductions sit on 8 x 8 or 7 x 9 pixels; the split classes of 16- and 32-wide tiles need the width: 1x1 there
            assert c.H * c.W <= 64 or (c.ks == 1 and c.H * c.W <= 17 * 19), cc.case_id(i)
    # the one exception: a stride-2 forward launch runs 32-wide tiles from 32 output columns = 63 input columns on; those images are a few rows high
    assert wide and all(c.stride == 2 and c.kind == "fwd" and c.W <= 65 and c.H <= 5 and c.variant % 1000000 // 10000 == 32 for c in wide)
    assert sum(c.N * c.H * c.W * c.Cin * c.Cout * c.ks * c.ks for c in CASES) < 1e10


# ------------------------------------------------------------------------------------------------------------------------ coverage

# classes of the recorded sweep that no launch of at most 3 images of 40 pixels reaches
UNREACHABLE = {
    # variant ...7 is the id of the 256-pixel kernel at 512 tiles or more (the launches bench.py's roofline follows): the same instantiations as
    # ...6.  A split plan wants fewer than 400 128-pixel blocks from unet_tuning.plan_batch images while the launch's own images fill 512
    # 256-pixel tiles: with N = 3 against plan_batch = 1 on 32 x 32 pixels that takes 43 channel blocks (5504 outputs) over at least
    # 8 chunks of 32 channels, 3e10 products.  The unsplit ...7 classes are in the table (18 channel blocks on 30 pixel tiles).
    (1, 0, 321287, True): "bf16 forward, split, 512 tiles",
    (1, 1, 321287, True): "bf16 dgrad, split, 512 tiles",
}


def test_table_reaches_every_class_of_the_recorded_sweep():
    doc = json.loads((ROOT / "tests" / "golden" / "conv_plans.json").read_text())
    sweep = P.cases()
    assert len(sweep) == len(doc["results"])
    want, plain = set(), set()
    for pc, r in zip(sweep, doc["results"]):
        if pc is None or r[0] < 0 or pc["dtype"] not in (0, 1):
            continue
        k = (pc["dtype"], pc["kind"], r[0] % 1000000, r[0] >= 1000000)
        want.add(k)
        if pc["tuning"] is None or (isinstance(pc["tuning"], dict) and set(pc["tuning"]) <= {"plan_batch"}):
            plain.add(k)
    assert len(want) >= 140 and plain <= want
    have = {klass(c) for c in CASES}
    missing = sorted(want - have - set(UNREACHABLE))
    assert not missing, f"classes (dtype, kind, variant % 1000000, split) of the recorded sweep without a case: {missing}"
    assert not (set(UNREACHABLE) & have), "a class listed as unreachable has a case: take it off the list"
    assert set(UNREACHABLE) <= want
    # the last digit 6 has two meanings (variant_id: 1 + 5 on a stride-2 forward launch of the 64-pixel tile, 6 for the 256-pixel tile): both occur
    for dt in BOTH:
        some(lambda c: c.dtype == dt and c.variant % 10 == 6 and c.stride == 2 and family(c) == "generic", f"{dt}: digit 6 on the stride-2 64-pixel tile")
        some(lambda c: c.dtype == dt and c.variant % 10 == 6 and c.stride == 1 and family(c) == "t256", f"{dt}: digit 6 on the 256-pixel tile")


def t256_launch_tiles(c):
    """pixel tiles x channel blocks of each launch of a 256-pixel case (launch_t256 issues a narrower last block on its own)"""
    v = c.variant % 1000000
    tw, bn = v // 10000, v % 10000 // 10
    pix = c.N * cdiv(c.H, 256 // tw) * cdiv(c.W, tw)
    nblk = cdiv(cc.produced(c)[1], bn)
    return [pix * nblk] if len(kernels(c)) == 1 else [pix * (nblk - 1), pix]


def test_table_covers_the_256_pixel_kernel():
    t256 = [c for c in CASES if family(c) == "t256"]
    names = {k for c in t256 for k in kernels(c)}
    for dt in BOTH:
        mine = [c for c in t256 if c.dtype == dt]
        for tw in (32, 16):
            for tiles in range(1, 9):
                assert f"t256<{tiles},{tw},{TY[dt]}>" in names, (dt, tw, tiles)
            for kind in KINDS:          # forward and dgrad tap order
                assert any(c.kind == kind and c.variant % 1000000 // 10000 == tw for c in mine), (dt, tw, kind)
            # the last patch row and the last patch column partly outside the image
            assert any(c.variant % 1000000 // 10000 == tw and c.H % (256 // tw) and c.W % tw for c in mine), (dt, tw)
        # a full block followed by a narrower last block
        for cout in (232, 228):
            two = [c for c in mine if c.Cout == cout and not c.count and len(kernels(c)) == 2]
            assert two and all(kernels(c)[0] == f"t256<8,32,{TY[dt]}>" for c in two), (dt, cout)
        for tpw in (2, 3):
            assert any(dict(c.tuning).get("t256_tiles_per_wg") == tpw and all(t % tpw and t > tpw for t in t256_launch_tiles(c)) for c in mine), (dt, tpw)
        assert any(dict(c.tuning).get("t256_tiles_per_wg") and len(kernels(c)) == 2 for c in mine), dt
        assert any(has(c, "wimg") for c in mine), dt
    # the fp32 sliver <7, 32, float, true>: 100 outputs and the last block of 228, both directions; the same shapes with t256_sliver = 0
    for kind in KINDS:
        for cout, count in ((100, 0), (228, 100)):
            on = [c for c in t256 if c.kind == kind and c.Cout == cout and c.count == count and kernels(c) == ["t256<7,32,float,sliver>"]]
            assert on, (kind, cout)
            off = [c for c in t256 if dict(c.tuning).get("t256_sliver") == 0 and kernels(c) == ["t256<7,32,float>"]]
            assert any(a[:11] == b[:11] for a in on for b in off), (kind, cout)
    assert "t256<7,32,float,sliver>" in kernels(next(c for c in t256 if c.dtype == "f32" and c.Cout == 228 and not c.count))
    some(lambda c: family(c) == "t256" and c.dtype == "f32" and c.Cout == 100 and c.variant // 10000 % 100 == 16, "100 fp32 outputs on 16-pixel patches (no sliver)")
    # reduction tails
    f32 = [c for c in t256 if c.dtype == "f32"]
    assert {c.Cin % 16 for c in f32} >= {0, 4, 8, 13} and any(c.Cin < 16 for c in f32)
    assert {c.kind for c in f32 if c.Cin % 16} == set(KINDS)
    bf = [c for c in t256 if c.dtype == "bf16"]
    assert {c.Cin % 32 for c in bf} >= set(range(0, 9)), "bf16 folded tails: Cin % 32 in 1..8"
    assert len({c.Cin % 32 for c in bf if c.Cin % 32 >= 9}) >= 4 and any(c.Cin < 32 and c.Cin >= 9 for c in bf), "bf16 unfolded tails"
    assert {c.kind for c in bf if 1 <= c.Cin % 32 <= 8} == set(KINDS) and {c.kind for c in bf if c.Cin % 32 >= 9} == set(KINDS)
    assert any(c.Cin > 32 and 1 <= c.Cin % 32 <= 8 for c in bf) and any(c.Cin <= 8 for c in bf)


SHAPES = ("1,1,4,1", "2,1,2,2", "2,2,2,2", "1,1,2,2", "1,2,2,2")        # launch_bn: bm 128 x bn 32 / 64 / 128, bm 64 x bn 64 / 128


def test_table_covers_the_generic_kernels():
    names = {k for c in CASES if family(c) == "generic" for k in kernels(c)}
    for kern in ("conv_igemm16", "conv_igemm", "conv_bf16"):
        for tw in (8, 16, 32):
            for shape in SHAPES:
                for hit in (4, 10):
                    assert f"{kern}<{tw},{shape},{hit}>" in names, (kern, tw, shape, hit)
    # the conv_igemm16 sliver: Cout % 16 in 1..4 on the 128 x 128 tile in the launch that produces the last channels; column sums switch it off
    def sliver_shape(c):
        return (family(c) == "generic" and c.dtype == "f32" and kernels(c)[0].startswith("conv_igemm16<") and kernels(c)[0].endswith(",2,2,2,2,4>")
                and 1 <= c.Cout % 16 <= 4 and c.Cout >= 16 and sum(cc.produced(c)) == c.Cout and not has(c, "wimg") and splits_of(c) == 0)
    for r in (1, 2, 3, 4):
        on = [c for c in CASES if sliver_shape(c) and c.Cout % 16 == r and not has(c, "colsum")]
        off = [c for c in CASES if sliver_shape(c) and c.Cout % 16 == r and has(c, "colsum")]
        assert on and off and {c.ks for c in on} == {1, 3} and {c.kind for c in on} == set(KINDS), r
        assert any(a[:9] == b[:9] and a.tuning == b.tuning for a in on for b in off), r
    some(lambda c: sliver_shape(c) and c.begin > 0, "the sliver in a channel-range launch")
    # column sums: rows per pixel tile 4 (the 128 x 32 tile) and 2, both fp32 kernels, both directions, the four parity classes
    col = [c for c in CASES if has(c, "colsum")]
    assert all(c.dtype == "f32" and family(c) == "generic" and splits_of(c) == 0 and c.rows > 0 for c in col)
    for kern in ("conv_igemm16<", "conv_igemm<"):
        mine = [c for c in col if kernels(c)[0].startswith(kern)]
        assert {kernels(c)[0].split(",", 1)[1][:7] for c in mine} >= {"1,1,4,1", "1,1,2,2"} and {c.kind for c in mine} == set(KINDS), kern
        assert any(c.kind == "dgrad" and c.stride == 2 for c in mine) and any(c.kind == "fwd" and c.stride == 2 for c in mine), kern
        assert any(has(c, "colsumsq") for c in mine) and any(not has(c, "colsumsq") for c in mine) and any(c.ks == 1 for c in mine), kern
    some(lambda c: has(c, "colsum") and dict(c.tuning).get("plan_batch") == 64 and c.ks == 3 and c.W == 32, "column sums keeping a launch off the 256-pixel tile")
    some(lambda c: has(c, "colsum") and c.Cin >= 256 and c.H * c.W <= 64, "column sums keeping a launch unsplit")


def test_table_covers_split_k():
    sp = [c for c in CASES if splits_of(c) >= 2]
    for dt in BOTH:
        mine = [c for c in sp if c.dtype == dt]
        kc = 16 if dt == "f32" else 32
        got = {splits_of(c) for c in mine}
        assert {2, 3, 32} <= got and any(4 <= s <= 31 for s in got), (dt, sorted(got))
        assert any(cdiv(c.Cin, kc) % splits_of(c) for c in mine), f"{dt}: a chunk count the split count does not divide"
        assert any(cc.produced(c)[1] % 4 for c in mine), f"{dt}: slab rows wider than the produced range"
        assert any(c.begin > 0 for c in mine), f"{dt}: a channel range with n_base > 0"
        assert {(c.ks, c.kind) for c in mine} == {(1, "fwd"), (1, "dgrad"), (3, "fwd"), (3, "dgrad")}, dt
        # (an fp32 launch never splits on the 256-pixel tile: below 256 of its blocks the planner narrows the channel block or leaves the tile)
        assert {family(c) for c in mine} == ({"generic", "t256"} if dt == "bf16" else {"generic"}), dt
        for ep in (("bias",), ("res",), ("relu",), ("mask",), ("bias", "res", "relu", "mask"), ()):
            assert any(c.ep == ep and c.kind == "fwd" for c in mine), (dt, ep)
        for ep in (("res",), ("mask",), ("res", "mask"), ()):
            assert any(c.ep == ep and c.kind == "dgrad" for c in mine), (dt, ep)
        for ws in ("short", "none"):
            short = [c for c in CASES if c.dtype == dt and c.ws == ws]
            assert {c.ks for c in short} == {1, 3} and {c.kind for c in short} == set(KINDS) and any(c.begin for c in short), (dt, ws)
            assert all(c.ws_floats > 0 and c.variant < 1000000 for c in short)
        assert any(has(c, "wimg") for c in mine), dt
    bf = [c for c in sp if c.dtype == "bf16"]
    y32 = [c for c in bf if has(c, "y_f32")]
    assert y32 and all(not has(c, "res") and not has(c, "mask") for c in y32), "the reduce kernel refuses res and mask with an fp32 output of bf16 storage"
    assert {c.kind for c in y32} == set(KINDS) and any(has(c, "bias") and has(c, "relu") for c in y32)
    assert any(not has(c, "y_f32") and has(c, "res") and has(c, "mask") for c in bf)


def test_table_covers_stride_2_dgrad():
    for dt in BOTH:
        mine = [c for c in CASES if c.dtype == dt and c.kind == "dgrad" and c.stride == 2]
        assert {(c.H % 2, c.W % 2) for c in mine} == {(0, 0), (0, 1), (1, 0), (1, 1)}, dt
        assert any(cc.out_hw(c)[0] == 1 and c.H == 1 for c in mine) and any(cc.out_hw(c)[0] == 1 and c.H == 2 for c in mine), f"{dt}: a 1-pixel-high gradient"
        assert any(c.W == 2 for c in mine), dt
        assert all(c.variant % 10 in (0, 5) for c in mine), "four parity classes of stride-1 tap sets: four halo items"


def test_table_covers_the_1x1_families():
    for dt in BOTH:
        ty = TY[dt]
        smallk = [c for c in CASES if c.dtype == dt and family(c) == "smallk"]
        assert {c.Cin for c in smallk} >= {1, 5, 8} and {c.kind for c in smallk} == set(KINDS) and any(c.Cout % 8 for c in smallk), dt
        assert any(has(c, "res") and has(c, "mask") for c in smallk)
        head = [c for c in CASES if c.dtype == dt and family(c) == "head1x1"]
        for y32 in ((False,) if dt == "f32" else (False, True)):
            got = {(c.Cout, c.Cin) for c in head if has(c, "y_f32") == y32}
            assert got >= {(co, ci) for co in (1, 2, 5, 16) for ci in (9, 100, 128)}, (dt, y32)
        assert {k for c in head for k in kernels(c)} == {f"conv1x1_head<{ty},2>", f"conv1x1_head<{ty},4>"}, dt
        for mt in (2, 4):              # more than one block of 64 mt pixels, the last one ragged
            assert any(c.N * c.H * c.W > 64 * mt and (c.N * c.H * c.W) % (64 * mt) for c in head if kernels(c) == [f"conv1x1_head<{ty},{mt}>"]), (dt, mt)
        gemm = [c for c in CASES if c.dtype == dt and family(c) == "gemm1x1" and not has(c, "ps")]
        for form in ("direct", "staged"):
            mine = [c for c in gemm if kernels(c) == [f"conv1x1_gemm<{ty},{form}>"]]
            assert {c.kind for c in mine} == set(KINDS), (dt, form)
            assert any((c.N * c.H * c.W) % 128 and (c.N * c.H * c.W) > 256 for c in mine), f"{dt} {form}: a ragged last pixel tile behind full ones"
            assert any(c.begin == 128 for c in mine) and any(c.Cout > 256 for c in mine), (dt, form)
        ps = [c for c in CASES if c.dtype == dt and has(c, "ps")]
        for form in ("direct", "staged"):
            mine = [c for c in ps if kernels(c) == [f"conv1x1_gemm<{ty},{form}>+ps"]]
            assert {c.Cout // 4 for c in mine} >= {16, 32, 48} and {cc.tail_channels(c) for c in mine} == {0, 3, 4}, (dt, form)
            assert all(c.H % 2 and c.W % 2 and c.N > 1 for c in mine) and {cc.tail_channels(c) for c in mine if c.Cout == 64} == {0, 3, 4}
            assert any(has(c, "relu") for c in mine) and any(not has(c, "relu") for c in mine) and any(not has(c, "bias") for c in mine)
    some(lambda c: c.dtype == "bf16" and family(c) == "gemm1x1" and not has(c, "ps") and "conv1x1_gemm" not in dict(c.tuning), "bf16 on the GEMM kernel by default")
    some(lambda c: c.dtype == "bf16" and family(c) == "gemm1x1" and has(c, "y_f32"), "the GEMM kernel with an fp32 output of bf16 storage")


def test_pixel_shuffle_wants_whole_16_channel_groups(L):
    """unet_conv_desc.pixel_shuffle takes Cout = 4 nf with nf a multiple of 16: 24 shuffled channels are refused, so the table holds 16, 32 and 48"""
    c = next(c for c in CASES if has(c, "ps") and c.Cout == 64)
    assert cc.query(L, c)[0] == 8
    assert cc.query(L, c._replace(Cout=96))[0] == -1


def test_table_covers_the_small_cin_kernel():
    for dt in BOTH:
        mine = [c for c in CASES if c.dtype == dt and family(c) == "smallcin"]
        assert {c.Cin for c in mine} == {1, 3, 4, 8} and {c.Cout for c in mine} == {16, 24, 32}, dt
        for st in (1, 2):
            got = [c for c in mine if c.stride == st and c.H % 2 and c.W % 2]          # odd sizes
            assert {c.Cin for c in got} == {1, 3, 4, 8} and {c.Cout for c in got} == {16, 24, 32}, (dt, st)
        assert {k for c in mine for k in kernels(c)} == {f"conv3x3_smallcin<{TY[dt]},1>", f"conv3x3_smallcin<{TY[dt]},{8 // cc.vec_of(dt)}>"}


def test_table_covers_per_image_filters_and_slices():
    for dt in BOTH:
        mine = [c for c in CASES if c.dtype == dt and has(c, "wimg")]
        assert mine and all(c.N == 3 for c in mine) and {family(c) for c in mine} == {"generic", "t256"}, dt
    sliced = [c for c in CASES if c.lay in cc.SLICED]
    assert 3 * len(sliced) >= len(CASES)
    for lay in cc.SLICED:
        assert all(co > 0 and tail > 0 for co, tail in cc.LAYOUTS[lay])
    for c in CASES:
        s = cc.strides(c)
        v = cc.vec_of(c.dtype)
        for name, C_, vec in (("x", c.Cin, v), ("y", cc.y_channels(c), cc.y_vec(c)), ("res", c.Cout, v), ("mask", c.Cout, v)):
            co, cs = s[name]
            assert co % vec == 0 and cs % vec == 0 and cs >= co + cc.rup(C_, vec)
            if c.lay in cc.SLICED:
                assert co > 0 and cs > co + cc.rup(C_, vec)
    # every family and both storage types as true slices, with channel counts that are no multiple of the vector width among them
    for dt in BOTH:
        for fam in ("generic", "t256", "gemm1x1", "smallk", "smallcin", "head1x1"):
            mine = [c for c in sliced if c.dtype == dt and family(c) == fam]
            assert mine and any(c.lay == 0 for c in CASES if c.dtype == dt and family(c) == fam), (dt, fam)
            if fam not in ("smallcin", "gemm1x1"):
                assert any(c.Cin % cc.vec_of(dt) for c in mine) and any(c.Cout % cc.vec_of(dt) for c in mine), (dt, fam)
        assert any(splits_of(c) >= 2 for c in sliced if c.dtype == dt)
        assert any(has(c, "res") and has(c, "mask") and c.Cout % cc.vec_of(dt) for c in sliced if c.dtype == dt)


# ------------------------------------------------------------------------------------------------------------------------ operands

def test_exact_operands_keep_the_exactness_condition():
    t0 = time.time()
    big = {}
    rounds = 0
    for i, c in enumerate(CASES):
        host = cc.exact_inputs(c, i)
        bound, sums = cc.exact_bound(c, host)          # from the operands actually built
        assert bound < 2 ** 24 and sums < 2 ** 24, (cc.case_id(i), bound, sums)
        lim, wlim = (256, 4) if c.dtype == "bf16" else (cc.BIG, 2)
        for k in ("x", "w", "bias", "res", "tail"):
            if k in host:
                t = host[k]
                assert torch.equal(t, t.round()) and t.abs().max() <= (wlim if k == "w" else lim), (cc.case_id(i), k)
                if c.dtype == "bf16" and k != "bias":
                    assert torch.equal(t.to(torch.bfloat16).float(), t)
        assert host["x"].abs().max() > 0 and host["w"].abs().max() > 0, cc.case_id(i)
        if has(c, "mask"):
            m = host["mask"]
            assert bool((m > 0).any()) and bool((m < 0).any()) and bool((m == 0).any()) and bool(torch.signbit(m[m == 0]).any()) \
                and not bool(torch.signbit(m[m == 0]).all()), cc.case_id(i)
            assert torch.equal(m.to(torch.bfloat16).float(), m)
        ref = cc.reference(c, host)
        assert torch.equal(ref, ref.round()) and ref.abs().max() < 2 ** 24 and ref.abs().max() > 0, cc.case_id(i)
        _, _, OH, OW = cc.dims(c)
        assert tuple(ref.shape) == ((c.N, 2 * c.H, 2 * c.W, c.Cout // 4) if has(c, "ps") else (c.N, OH, OW, c.Cout))
        if c.dtype == "f32" and bool((host["x"].abs() == cc.BIG).any()):
            big.setdefault("split" if splits_of(c) >= 2 else family(c), []).append(i)
            assert torch.tensor(cc.BIG).to(torch.bfloat16).item() != cc.BIG and torch.tensor(cc.BIG).to(torch.float16).item() != cc.BIG
        if cc.y_vec(c) == 8 and ref.abs().max() > 256 and not torch.equal(cc.stored(c, ref), ref):
            rounds += 1
    # 13 significant bits in the fp32 operands of every kernel family
    assert set(big) == {"generic", "t256", "gemm1x1", "smallk", "smallcin", "head1x1", "split"}, sorted(big)
    assert all(len(v) >= 3 for v in big.values())
    # bf16 outputs beyond 256, where the single rounding of the store changes the value
    assert rounds >= 50, rounds
    print(f"operands and references of {len(CASES)} cases in {time.time() - t0:.1f} s")


def test_gauss_operands_and_slices():
    import guard
    c = next(c for c in CASES if c.dtype == "bf16" and c.lay in cc.SLICED and has(c, "res") and has(c, "mask") and c.Cin % 4 and c.Cout % 8)
    g = cc.gauss_inputs(c, 5)
    for k in ("x", "w", "res", "mask"):
        assert torch.equal(g[k].to(torch.bfloat16).float(), g[k]) and g[k].std() > 0.1 / (c.Cin * c.ks * c.ks) ** 0.5
    assert not torch.equal(g["bias"].to(torch.bfloat16).float(), g["bias"]) if "bias" in g else True
    for dt, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        co, cs = cc.strides(c._replace(dtype=name))["x"]
        t, check = cc.device_slice(g["x"], co, cs, dt, device="cpu")
        v = cc.vec_of(name)
        assert (t.co, t.cs, t.C) == (co, cs, c.Cin) and torch.equal(t.view().float(), g["x"])
        pad = t.buf[..., t.co + t.C:t.co + cc.rup(t.C, v)]
        assert pad.numel() and bool((pad == 0).all())
        rest = torch.cat([t.buf[..., :t.co], t.buf[..., t.co + cc.rup(t.C, v):]], dim=-1)
        canary = cc.canary(dt)
        assert rest.numel() and bool((rest == canary).all()) and abs(canary) > 1e7 and canary == guard.CANARY[torch.float32] or dt == torch.bfloat16
        assert torch.isfinite(torch.tensor(canary))
        check("x")
