"""Forward and input-gradient ("dgrad") conv test cases (plain Python and torch on the CPU, no GPU): the table of tests/test_conv_gpu.py,
the builders of its operands and its fp64 reference.  What the table covers is asserted by tests/test_conv_cases_cpu.py.

  CASES            small stand-alone launches of unet_conv2d.  A case STATES what the library plans for it -- the variant id, the split-K
                   workspace floats and the column-sum rows (unet_conv2d_variant, unet_conv2d_splitk_workspace, unet_conv2d_colsum_rows
                   plan without a GPU; the CPU test holds every case against them) -- there is no Python copy of the planner here.
  kernels(c)       the kernel instantiation(s) that follow from the stated variant and the shape by the arithmetic of launch_t256
                   (conv_bf16.hip) and launch_bn (conv_common.h): the test id names them, the coverage assertions count them.
  exact_inputs     integer-valued operands.  conv(|x|, |w|) + |bias| + |res| stays below 2^24 at every output element (exact_bound: computed
                   from the operands actually built; the builder draws smaller and sparser values until it holds), so every product, every
                   partial sum in any order and in any split and the result are exact in fp32: the kernels are compared bit for bit.
                   fp32 storage: about one value in sixteen of x and of res is +-(2^12 + 1), thirteen significant bits -- a multiply that took
                   a detour through bf16, fp16 or a 10-bit mantissa changes the result.  bf16 storage: integers up to 256, weights up to 4.
  gauss_inputs     the generators of test_conv_fwd / test_conv_forward_dgrad_wgrad_bf16, compared at those tests' tolerances.
  reference        plain torch in fp64.
  strides, device_slice    an operand as training passes it: a channel slice of a wider buffer, pad lanes zero, every other channel and both
                   guard bands of the allocation (tests/guard.py) a loud finite canary.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

# ------------------------------------------------------------------------------------------------------------------------ cases

Case = namedtuple("Case", "dtype kind ks stride N H W Cin Cout begin count lay ep tuning ws variant ws_floats rows")
# dtype    "f32" | "bf16": the storage type of the activations and of the packed filters
# kind     "fwd" | "dgrad"
# H, W     the larger spatial side of the launch: the forward INPUT's (fwd: x is H x W; dgrad: the produced gradient is H x W and the
#          incoming one out_hw(H, W)); a pixel-shuffle case reads H x W and stores 2H x 2W
# Cin      channels of the launch's input operand (the reduction), Cout: produced channels (pixel-shuffle: 4 nf)
# begin, count   unet_conv_desc.cout_begin / cout_count (0, 0: the whole range)
# lay      index into LAYOUTS
# ep       epilogue and descriptor options, a tuple of names out of EP_NAMES
# tuning   unet_tuning fields as a sorted tuple of pairs
# ws       the split-K workspace the launch brings: "exact" (what the library asks for, to the float) | "short" (one float less) | "none"
# variant, ws_floats, rows   what the library answers for the case (the variant UNDER the case's workspace mode)

EP_NAMES = ("bias", "res", "relu", "mask", "colsum", "colsumsq", "y_f32", "wimg", "ps", "tail3", "tail4")

# (co, tail) of x, y, res and mask in units of one 16-byte channel vector (4 fp32 / 8 bf16 channels; y of a y_f32 launch: 4): the slice starts
# at channel co * vec of a buffer of co * vec + rup(C, vec) + tail * vec channels.  Layouts 1, 3 and 4: all four are true slices (co > 0 and
# neighbours behind the pad lanes)
LAYOUTS = [
    ((0, 0), (0, 0), (0, 0), (0, 0)),
    ((1, 1), (2, 1), (1, 2), (3, 1)),
    ((0, 1), (0, 2), (0, 0), (0, 1)),
    ((2, 2), (1, 1), (2, 1), (1, 1)),
    ((3, 1), (1, 2), (1, 1), (2, 2)),
]
SLICED = (1, 3, 4)


def cdiv(a, b):
    return -(-a // b)


def rup(a, b):
    return cdiv(a, b) * b


def vec_of(dtype):
    return 8 if dtype == "bf16" else 4


def has(c, name):
    return name in c.ep


def out_hw(c):
    pad = (c.ks - 1) // 2
    return (c.H + 2 * pad - c.ks) // c.stride + 1, (c.W + 2 * pad - c.ks) // c.stride + 1


def dims(c):
    """(IH, IW, OH, OW) of the descriptor: the launch's input and output sides"""
    oh, ow = out_hw(c)
    return (oh, ow, c.H, c.W) if c.kind == "dgrad" else (c.H, c.W, oh, ow)


def y_vec(c):
    return 4 if c.dtype == "f32" or has(c, "y_f32") else 8


def y_channels(c):
    return c.Cout // 4 if has(c, "ps") else c.Cout


def tail_channels(c):
    return 3 if has(c, "tail3") else (4 if has(c, "tail4") else 0)


def strides(c):
    """{operand: (co, cs)} in channels for x, y, res, mask"""
    v = vec_of(c.dtype)
    (xo, xt), (yo, yt), (ro, rt), (mo, mt) = LAYOUTS[c.lay]
    yv = y_vec(c)
    if tail_channels(c):
        yt = max(yt, 2)           # the tail lands directly behind the shuffled channels, and a neighbour stays behind it
    return dict(x=(xo * v, xo * v + rup(c.Cin, v) + xt * v), y=(yo * yv, yo * yv + rup(y_channels(c), yv) + yt * yv),
                res=(ro * v, ro * v + rup(c.Cout, v) + rt * v), mask=(mo * v, mo * v + rup(c.Cout, v) + mt * v))


def produced(c):
    """(first, count) of the channels the launch produces"""
    return (c.begin, c.count) if c.count else (0, c.Cout)


def tail_at(c):
    co, _ = strides(c)["y"]
    return co + rup(y_channels(c), y_vec(c))


# ------------------------------------------------------------------------------------------------------------------------ the library's plan

X, WP, Y, RES, MASK, WS, COLSUM, COLSUMSQ, TAIL, BIAS = (0x1000000 * (i + 1) for i in range(10))      # fake, aligned, never dereferenced


def query_desc(L, c, tuning=None):
    """(unet_conv_desc over fake addresses, the unet_tuning it points to): enough for the three planning entry points"""
    import ctypes as C
    d = L.ConvDesc()
    s = strides(c)
    d.x, d.wp, d.y = X, WP, Y
    (d.x_co, d.x_cs), (d.y_co, d.y_cs) = s["x"], s["y"]
    d.N, d.Cin, d.Cout = c.N, c.Cin, c.Cout
    d.IH, d.IW, d.OH, d.OW = dims(c)
    d.ks, d.stride, d.kind = c.ks, c.stride, L.CONV_DGRAD if c.kind == "dgrad" else L.CONV_FWD
    d.dtype, d.y_f32 = (L.BF16 if c.dtype == "bf16" else L.F32), int(has(c, "y_f32"))
    d.flags = (L.CONV_RELU if has(c, "relu") else 0) | (L.CONV_MASK if has(c, "mask") else 0)
    if has(c, "bias"):
        d.bias = BIAS
    if has(c, "res"):
        d.res, (d.res_co, d.res_cs) = RES, s["res"]
    if has(c, "mask"):
        d.mask, (d.mask_co, d.mask_cs) = MASK, s["mask"]
    if has(c, "colsum"):
        d.colsum = COLSUM
    if has(c, "colsumsq"):
        d.colsumsq = COLSUMSQ
    d.cout_begin, d.cout_count = c.begin, c.count
    if has(c, "wimg"):
        d.wp_img_stride = 1 << 20
    if has(c, "ps"):
        d.pixel_shuffle = 1
        if tail_channels(c):
            d.ps_tail, d.ps_tail_cs, d.ps_tail_co, d.ps_tail_c, d.ps_tail_at = TAIL, 8, 0, tail_channels(c), tail_at(c)
    t = L.Tuning.default(**dict(c.tuning if tuning is None else tuning))
    d.tuning = C.pointer(t)
    return d, t


def query(L, c, ws=None):
    """[variant, workspace floats, column-sum rows] as the library plans the case, the variant under workspace mode `ws` (default: the case's)"""
    import ctypes as C
    d, _t = query_desc(L, c)
    need = int(L.lib.unet_conv2d_splitk_workspace(C.byref(d)))
    ws = c.ws if ws is None else ws
    if ws != "none" and need > 0:
        d.splitk_ws, d.splitk_ws_floats = WS, need - (1 if ws == "short" else 0)
    return [int(L.lib.unet_conv2d_variant(C.byref(d))), need, int(L.lib.unet_conv2d_colsum_rows(C.byref(d)))]


# ------------------------------------------------------------------------------------------------------------------------ from the variant to the kernel

FAMILY = {8: "gemm1x1", 9: "smallk", 10: "smallcin", 11: "head1x1"}


def splits_of(c):
    return c.variant // 1000000


def family(c):
    """the kernel family of the stated variant: gemm1x1 | smallk | smallcin | head1x1 | t256 | generic"""
    v = c.variant % 1000000
    return FAMILY[v] if v < 100 else ("t256" if _t256(c) else "generic")


def _t256(c):
    """last digit 7, or 6 on a stride-1 launch: the 256-pixel tile (6 on a stride-2 forward launch = 1 + 5: ten halo items on the 64-pixel tile)"""
    return c.variant % 10 == 7 or (c.variant % 10 == 6 and c.stride == 1)


def kernels(c):
    """the instantiation(s) the launch runs, from the stated variant and the shape: [names], two for a 256-pixel launch whose last channel
    block is narrower than the others.  The arithmetic of launch_t256 (tiles of a block, the fp32 sliver) and of launch_bn / launch_tw
    (<TW, MT, NT, WM, WN, HIT>); the special families name their storage type and form."""
    v = c.variant % 1000000
    t = dict(c.tuning)
    ty = "bf16" if c.dtype == "bf16" else "float"
    if v < 100:
        name = FAMILY[v]
        if name == "gemm1x1":
            mode = t.get("conv1x1_gemm", 0)
            form = "staged" if has(c, "ps") and mode != 1 else ("direct" if mode == 1 else "staged")
            return [f"conv1x1_gemm<{ty},{form}>" + ("+ps" if has(c, "ps") else "")]
        if name == "head1x1":
            mt = 4 if (c.dtype == "bf16") != (t.get("conv_head1x1", 1) == 2) else 2
            return [f"conv1x1_head<{ty},{mt}>"]
        if name == "smallcin":
            return [f"conv3x3_smallcin<{ty},{1 if c.Cin <= vec_of(c.dtype) else 8 // vec_of(c.dtype)}>"]
        return [f"conv1x1_smallk<{ty}>"]
    tw, bn, last = v // 10000, v % 10000 // 10, v % 10
    _, cols = produced(c)
    if _t256(c):
        nblk, full = cdiv(cols, bn), bn // 16
        last_tiles = cdiv(cols - (nblk - 1) * bn, 16)

        def one(tiles, width):
            last_w = width - (tiles - 1) * 16
            if c.dtype == "f32" and t.get("t256_sliver", 1) and tiles == 7 and tw == 32 and 1 <= last_w <= 4:
                return f"t256<7,32,{ty},sliver>"
            return f"t256<{tiles},{tw},{ty}>"
        if nblk == 1 or last_tiles == full:
            return [one(last_tiles if nblk == 1 else full, cols - (nblk - 1) * bn)]
        return [one(full, bn), one(last_tiles, cols - (nblk - 1) * bn)]
    hit = 10 if last in (1, 6) else 4
    if last in (5, 6):
        shape = (1, 1, 2, 2) if bn == 64 else (1, 2, 2, 2)
    else:
        shape = {32: (1, 1, 4, 1), 64: (2, 1, 2, 2), 128: (2, 2, 2, 2)}[bn]
    kern = "conv_bf16" if c.dtype == "bf16" else ("conv_igemm" if t.get("mfma_shape", 16) == 32 else "conv_igemm16")
    return [f"{kern}<{tw},{','.join(str(s) for s in shape)},{hit}>"]


# ------------------------------------------------------------------------------------------------------------------------ case table

def _mk(dtype, kind, ks, stride, N, H, W, Cin, Cout, v, wsf, rows, ep="", lay=0, ws="exact", begin=0, count=0, **tuning):
    ep = tuple(e for e in ep.split("+") if e)
    assert all(e in EP_NAMES for e in ep), ep
    return Case(dtype, kind, ks, stride, N, H, W, Cin, Cout, begin, count, lay, ep, tuple(sorted(tuning.items())), ws, v, wsf, rows)


F32, BF16, FWD, DGRAD = "f32", "bf16", "fwd", "dgrad"

# Every line: _mk(dtype, kind, ks, stride, N, H, W, Cin, Cout, variant, workspace floats, column-sum rows, ...).  The three numbers are what
# the library answered when the line was written; tests/test_conv_cases_cpu.py asks it again.
CASES = [
    # ---- one case per (dtype, kind, variant % 1000000, split) class of the recorded sweep of conv_plan_cases.py, at the cheapest small shape that reaches it
    # ---- (stride-2 forward launches on 32-wide tiles need 63 input columns: the images of 2 x 64, 3 x 65 and 5 x 63 are the table's only sides beyond 40; the
    # ---- 512-tile id ...7 takes 18 channel blocks on 30 pixel tiles)
    _mk(F32, FWD, 1, 1, 1, 7, 9, 4, 16, 9, 0, 8, ep="bias+res+relu+mask"),
    _mk(F32, FWD, 3, 1, 1, 7, 9, 4, 16, 10, 0, 8, ep="bias+relu", lay=1),
    _mk(F32, FWD, 1, 1, 1, 7, 9, 16, 4, 11, 0, 8, ep="bias", lay=2),
    _mk(F32, FWD, 1, 1, 1, 7, 9, 4, 4, 80320, 0, 8, ep="bias+res+relu+mask", lay=3),
    _mk(F32, FWD, 3, 2, 1, 7, 9, 4, 4, 80321, 0, 4, ep="bias", lay=4),
    _mk(F32, FWD, 1, 1, 1, 7, 9, 16, 36, 80645, 0, 4, ep="res", lay=1),
    _mk(F32, FWD, 1, 1, 1, 7, 9, 128, 36, 4080645, 9072, 4, ep="relu", lay=2),
    _mk(F32, FWD, 3, 2, 1, 7, 9, 4, 36, 80646, 0, 2, ep="mask", lay=3),
    _mk(F32, FWD, 3, 2, 1, 7, 9, 128, 36, 4080646, 2880, 2, lay=4),
    _mk(F32, FWD, 1, 1, 1, 7, 9, 128, 100, 3081280, 18900, 4, ep="bias+relu", plan_batch=64),
    _mk(F32, FWD, 3, 2, 1, 7, 9, 128, 136, 3081281, 8160, 2, ep="bias+res+relu", lay=2, plan_batch=64),
    _mk(F32, FWD, 1, 1, 1, 16, 16, 4, 4, 160320, 0, 8, ep="res+mask", lay=3),
    _mk(F32, FWD, 3, 2, 1, 5, 37, 4, 4, 160321, 0, 8, ep="bias+res+relu+mask", lay=4),
    _mk(F32, FWD, 3, 1, 1, 16, 16, 4, 4, 160326, 0, 2, ep="bias", plan_batch=4096),
    _mk(F32, FWD, 1, 1, 1, 16, 16, 16, 36, 160645, 0, 8, ep="res", lay=1),
    _mk(F32, FWD, 1, 1, 1, 16, 16, 128, 36, 4160645, 36864, 8, ep="relu", lay=3),
    _mk(F32, FWD, 3, 2, 1, 5, 37, 4, 36, 160646, 0, 4, ep="mask", lay=4),
    _mk(F32, FWD, 3, 2, 1, 5, 37, 128, 36, 4160646, 8208, 4),
    _mk(F32, FWD, 1, 1, 1, 16, 16, 128, 100, 3161280, 76800, 8, ep="bias+relu", lay=1, plan_batch=64),
    _mk(F32, FWD, 3, 2, 1, 5, 37, 128, 100, 3161281, 17100, 4, ep="bias+res+relu", lay=2, plan_batch=64),
    _mk(F32, FWD, 1, 1, 3, 17, 19, 256, 136, 6161285, 790704, 60, ep="res+mask", lay=4),
    _mk(F32, FWD, 3, 2, 1, 9, 33, 128, 100, 3161286, 25500, 8, ep="bias+res+relu+mask", plan_batch=32),
    _mk(F32, FWD, 1, 1, 1, 5, 37, 4, 4, 320320, 0, 16, ep="bias", lay=1),
    _mk(F32, FWD, 3, 2, 1, 2, 64, 4, 4, 320321, 0, 4, ep="res", lay=2),
    _mk(F32, FWD, 3, 1, 1, 5, 37, 4, 4, 320326, 0, 4, ep="relu", lay=3, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 1, 5, 37, 16, 36, 320640, 0, 8, ep="mask", lay=1, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 3, 5, 37, 1024, 36, 32320640, 639360, 36, lay=2),
    _mk(F32, FWD, 3, 2, 1, 2, 64, 4, 36, 320641, 0, 2, ep="bias+relu", lay=3, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 1, 5, 37, 16, 36, 320645, 0, 12, ep="bias+res+relu", lay=4),
    _mk(F32, FWD, 1, 1, 1, 5, 37, 128, 36, 4320645, 26640, 12, ep="res+mask"),
    _mk(F32, FWD, 3, 1, 1, 5, 37, 4, 36, 320646, 0, 4, ep="bias+res+relu+mask", lay=2, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 1, 2, 64, 128, 36, 4320646, 4608, 2, ep="bias", lay=3),
    _mk(F32, FWD, 1, 1, 1, 5, 37, 16, 100, 321280, 0, 8, ep="res", lay=4, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 3, 5, 37, 512, 136, 16321280, 1207680, 36, ep="relu"),
    _mk(F32, FWD, 3, 2, 1, 2, 64, 4, 100, 321281, 0, 2, ep="mask", lay=1, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 1, 2, 64, 128, 136, 3321281, 13056, 2, lay=3, plan_batch=64),
    _mk(F32, FWD, 1, 1, 2, 33, 35, 4, 1024, 321285, 0, 136, ep="bias+relu", lay=4),
    _mk(F32, FWD, 1, 1, 1, 5, 37, 1024, 136, 32321285, 805120, 12, ep="bias+res+relu"),
    _mk(F32, FWD, 3, 1, 1, 5, 37, 4, 100, 321286, 0, 4, ep="res+mask", lay=1, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 1, 5, 63, 128, 100, 3321286, 28800, 4, ep="bias+res+relu+mask", lay=2, plan_batch=64),
    _mk(F32, FWD, 3, 1, 3, 33, 33, 4, 2192, 321287, 0, 60, ep="bias", lay=4),
    _mk(F32, DGRAD, 1, 1, 1, 7, 9, 4, 16, 9, 0, 8, ep="res+mask"),
    _mk(F32, DGRAD, 1, 1, 1, 7, 9, 16, 4, 11, 0, 8, ep="bias", lay=1),
    _mk(F32, DGRAD, 1, 1, 1, 7, 9, 4, 4, 80320, 0, 8, ep="res+mask", lay=2),
    _mk(F32, DGRAD, 1, 1, 1, 7, 9, 16, 36, 80645, 0, 4, lay=3),
    _mk(F32, DGRAD, 1, 1, 1, 7, 9, 128, 36, 4080645, 9072, 4, ep="res"),
    _mk(F32, DGRAD, 1, 1, 1, 7, 9, 128, 100, 3081280, 18900, 4, ep="mask", lay=1, plan_batch=64),
    _mk(F32, DGRAD, 1, 1, 1, 16, 16, 4, 4, 160320, 0, 8, ep="res+mask", lay=2),
    _mk(F32, DGRAD, 3, 1, 1, 16, 16, 4, 4, 160326, 0, 2, lay=3, plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 1, 16, 16, 16, 36, 160645, 0, 8, ep="res", lay=4),
    _mk(F32, DGRAD, 1, 1, 1, 16, 16, 128, 36, 4160645, 36864, 8, ep="mask", lay=2),
    _mk(F32, DGRAD, 1, 1, 1, 16, 16, 16, 100, 161280, 0, 4, ep="res+mask", lay=3, plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 1, 16, 16, 128, 100, 3161280, 76800, 8, lay=4, plan_batch=64),
    _mk(F32, DGRAD, 1, 1, 1, 17, 19, 16, 100, 161285, 0, 20, ep="res", plan_batch=64),
    _mk(F32, DGRAD, 1, 1, 3, 17, 19, 256, 136, 6161285, 790704, 60, ep="mask", lay=1),
    _mk(F32, DGRAD, 1, 1, 1, 5, 37, 4, 4, 320320, 0, 16, ep="res+mask", lay=3),
    _mk(F32, DGRAD, 3, 1, 1, 5, 37, 4, 4, 320326, 0, 4, lay=4, plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 1, 5, 37, 16, 36, 320640, 0, 8, ep="res", plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 3, 5, 37, 1024, 36, 32320640, 639360, 36, ep="mask", lay=1),
    _mk(F32, DGRAD, 1, 1, 1, 5, 37, 16, 36, 320645, 0, 12, ep="res+mask", lay=2),
    _mk(F32, DGRAD, 1, 1, 1, 5, 37, 128, 36, 4320645, 26640, 12, lay=4),
    _mk(F32, DGRAD, 3, 1, 1, 5, 37, 4, 36, 320646, 0, 4, ep="res", plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 1, 5, 37, 16, 100, 321280, 0, 8, ep="mask", lay=1, plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 3, 5, 37, 512, 136, 16321280, 1207680, 36, ep="res+mask", lay=2),
    _mk(F32, DGRAD, 1, 1, 2, 33, 35, 4, 1024, 321285, 0, 136, lay=3),
    _mk(F32, DGRAD, 1, 1, 1, 5, 37, 1024, 136, 32321285, 805120, 12, ep="res"),
    _mk(F32, DGRAD, 3, 1, 1, 5, 37, 4, 100, 321286, 0, 4, ep="mask", lay=1, plan_batch=4096),
    _mk(F32, DGRAD, 3, 1, 3, 33, 33, 4, 2192, 321287, 0, 60, ep="res+mask", lay=2),
    _mk(BF16, FWD, 1, 1, 1, 7, 9, 32, 32, 8, 0, 8, ep="res", lay=3, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 1, 7, 9, 4, 16, 9, 0, 8, ep="bias+res+relu+mask", lay=4),
    _mk(BF16, FWD, 3, 1, 1, 8, 8, 4, 16, 10, 0, 4, ep="bias+relu", lay=1, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 1, 7, 9, 16, 4, 11, 0, 8, ep="bias", lay=2),
    _mk(BF16, FWD, 1, 1, 1, 7, 9, 4, 4, 80320, 0, 8, ep="relu", lay=3),
    _mk(BF16, FWD, 3, 2, 1, 7, 9, 4, 4, 80321, 0, 4, ep="mask", lay=4),
    _mk(BF16, FWD, 1, 1, 1, 7, 9, 16, 36, 80645, 0, 4),
    _mk(BF16, FWD, 1, 1, 1, 7, 9, 256, 36, 4080645, 9072, 4, ep="bias+relu", lay=3),
    _mk(BF16, FWD, 3, 2, 1, 7, 9, 4, 36, 80646, 0, 2, ep="bias+res+relu", lay=4),
    _mk(BF16, FWD, 3, 2, 1, 7, 9, 256, 36, 4080646, 2880, 2, ep="res+mask"),
    _mk(BF16, FWD, 1, 1, 1, 7, 9, 256, 100, 3081280, 18900, 4, ep="bias+res+relu+mask", lay=1, plan_batch=64),
    _mk(BF16, FWD, 3, 2, 1, 7, 9, 256, 136, 3081281, 8160, 2, ep="bias", lay=2, plan_batch=64),
    _mk(BF16, FWD, 1, 1, 1, 16, 16, 4, 4, 160320, 0, 8, ep="res", lay=4),
    _mk(BF16, FWD, 3, 2, 1, 5, 37, 4, 4, 160321, 0, 8, ep="relu"),
    _mk(BF16, FWD, 1, 1, 1, 16, 16, 16, 36, 160645, 0, 8, ep="mask", lay=1),
    _mk(BF16, FWD, 1, 1, 1, 16, 16, 256, 36, 4160645, 36864, 8, lay=2),
    _mk(BF16, FWD, 3, 2, 1, 5, 37, 4, 36, 160646, 0, 4, ep="bias+relu", lay=3),
    _mk(BF16, FWD, 3, 2, 1, 5, 37, 256, 36, 4160646, 8208, 4, ep="bias+res+relu"),
    _mk(BF16, FWD, 1, 1, 1, 16, 16, 256, 100, 3161280, 76800, 8, ep="res+mask", lay=1, plan_batch=64),
    _mk(BF16, FWD, 3, 2, 1, 5, 37, 256, 100, 3161281, 17100, 4, ep="bias+res+relu+mask", lay=2, plan_batch=64),
    _mk(BF16, FWD, 1, 1, 3, 17, 19, 512, 136, 6161285, 790704, 60, ep="bias", lay=3),
    _mk(BF16, FWD, 3, 1, 1, 16, 16, 256, 100, 3161286, 76800, 2, ep="res", lay=4, plan_batch=64),
    _mk(BF16, FWD, 1, 1, 1, 5, 37, 4, 4, 320320, 0, 16, ep="relu", lay=1),
    _mk(BF16, FWD, 3, 2, 1, 2, 64, 4, 4, 320321, 0, 4, ep="mask", lay=2),
    _mk(BF16, FWD, 3, 1, 1, 5, 37, 4, 4, 320326, 0, 16, lay=3, plan_batch=64),
    _mk(BF16, FWD, 1, 1, 1, 5, 37, 16, 36, 320640, 0, 8, ep="bias+relu", lay=4, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 1, 5, 37, 256, 36, 2320640, 13320, 12, ep="bias+res+relu", plan_batch=64),
    _mk(BF16, FWD, 3, 2, 1, 2, 64, 4, 36, 320641, 0, 2, ep="res+mask", lay=2, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 1, 3, 65, 228, 36, 3320641, 7128, 4, ep="bias+res+relu+mask", lay=3, plan_batch=64),
    _mk(BF16, FWD, 1, 1, 1, 5, 37, 16, 36, 320645, 0, 12, ep="bias", lay=4),
    _mk(BF16, FWD, 1, 1, 1, 5, 37, 256, 36, 4320645, 26640, 12, ep="res"),
    _mk(BF16, FWD, 3, 1, 1, 5, 37, 4, 36, 320646, 0, 12, ep="relu", lay=1, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 5, 37, 256, 36, 2320646, 13320, 12, ep="mask", lay=4, plan_batch=64),
    _mk(BF16, FWD, 1, 1, 1, 5, 37, 16, 100, 321280, 0, 8, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 1, 5, 37, 256, 100, 2321280, 37000, 12, ep="bias+relu", lay=1, plan_batch=64),
    _mk(BF16, FWD, 3, 2, 1, 2, 64, 4, 100, 321281, 0, 2, ep="bias+res+relu", lay=2, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 1, 2, 64, 228, 136, 3321281, 13056, 2, ep="res+mask", lay=3, plan_batch=64),
    _mk(BF16, FWD, 1, 1, 2, 33, 35, 4, 1024, 321285, 0, 136, ep="bias+res+relu+mask"),
    _mk(BF16, FWD, 1, 1, 2, 5, 37, 1024, 136, 16321285, 805120, 24, ep="bias", lay=1),
    _mk(BF16, FWD, 3, 1, 1, 5, 37, 4, 100, 321286, 0, 4, ep="res", lay=2, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 5, 37, 256, 100, 2321286, 37000, 4, ep="relu", lay=3, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 3, 33, 33, 4, 2192, 321287, 0, 60, ep="mask", lay=4),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 9, 32, 32, 8, 0, 8, lay=1, plan_batch=4096),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 9, 4, 16, 9, 0, 8, ep="res+mask", lay=2),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 9, 16, 4, 11, 0, 8, ep="bias", lay=3),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 9, 4, 4, 80320, 0, 8, ep="res", lay=4),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 9, 16, 36, 80645, 0, 4, ep="mask"),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 9, 256, 36, 4080645, 9072, 4, ep="res+mask", lay=2),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 9, 256, 100, 3081280, 18900, 4, lay=3, plan_batch=64),
    _mk(BF16, DGRAD, 1, 1, 1, 16, 16, 4, 4, 160320, 0, 8, ep="res", lay=4),
    _mk(BF16, DGRAD, 1, 1, 1, 16, 16, 16, 36, 160645, 0, 8, ep="mask"),
    _mk(BF16, DGRAD, 1, 1, 1, 16, 16, 256, 36, 4160645, 36864, 8, ep="res+mask", lay=1),
    _mk(BF16, DGRAD, 1, 1, 1, 16, 16, 16, 100, 161280, 0, 4, lay=3, plan_batch=4096),
    _mk(BF16, DGRAD, 1, 1, 1, 16, 16, 256, 100, 3161280, 76800, 8, ep="res", lay=4, plan_batch=64),
    _mk(BF16, DGRAD, 1, 1, 1, 17, 19, 16, 100, 161285, 0, 20, ep="mask", plan_batch=64),
    _mk(BF16, DGRAD, 1, 1, 3, 17, 19, 512, 136, 6161285, 790704, 60, ep="res+mask", lay=1),
    _mk(BF16, DGRAD, 3, 1, 1, 16, 16, 256, 100, 3161286, 76800, 2, lay=2, plan_batch=64),
    _mk(BF16, DGRAD, 1, 1, 1, 5, 37, 4, 4, 320320, 0, 16, ep="res"),
    _mk(BF16, DGRAD, 3, 1, 1, 5, 37, 4, 4, 320326, 0, 16, ep="mask", lay=1, plan_batch=64),
    _mk(BF16, DGRAD, 1, 1, 1, 5, 37, 16, 36, 320640, 0, 8, ep="res+mask", lay=2, plan_batch=4096),
    _mk(BF16, DGRAD, 1, 1, 1, 5, 37, 256, 36, 2320640, 13320, 12, lay=3, plan_batch=64),
    _mk(BF16, DGRAD, 1, 1, 1, 5, 37, 16, 36, 320645, 0, 12, ep="res", lay=4),
    _mk(BF16, DGRAD, 1, 1, 1, 5, 37, 256, 36, 4320645, 26640, 12, ep="mask", lay=1),
    _mk(BF16, DGRAD, 3, 1, 1, 5, 37, 4, 36, 320646, 0, 12, ep="res+mask", lay=2, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 5, 37, 256, 36, 2320646, 13320, 12, lay=3, plan_batch=64),
    _mk(BF16, DGRAD, 1, 1, 1, 5, 37, 16, 100, 321280, 0, 8, ep="res", lay=4, plan_batch=4096),
    _mk(BF16, DGRAD, 1, 1, 1, 5, 37, 256, 100, 2321280, 37000, 12, ep="mask", plan_batch=64),
    _mk(BF16, DGRAD, 1, 1, 2, 33, 35, 4, 1024, 321285, 0, 136, ep="res+mask", lay=2),
    _mk(BF16, DGRAD, 1, 1, 2, 5, 37, 1024, 136, 16321285, 805120, 24, lay=3),
    _mk(BF16, DGRAD, 3, 1, 1, 5, 37, 4, 100, 321286, 0, 4, ep="res", lay=4, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 5, 37, 256, 100, 2321286, 37000, 4, ep="mask", plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 3, 33, 33, 4, 2192, 321287, 0, 60, ep="res+mask", lay=1),
    # ---- conv_bf16_t256_kernel in both storage forms: channel-tile counts 1..8 at patch widths 32 and 16, two-launch blocks, the fp32 sliver, reduction tails,
    # ---- several tiles per workgroup, ragged patches
    _mk(F32, FWD, 3, 1, 1, 32, 32, 32, 16, 320326, 0, 8, lay=3, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 32, 24, 320326, 0, 8, ep="bias+relu", lay=4, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 32, 48, 320646, 0, 8, ep="bias+res+relu", plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 32, 56, 320646, 0, 8, ep="res+mask", lay=1, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 32, 80, 321286, 0, 8, ep="bias+res+relu+mask", lay=2, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 32, 88, 321286, 0, 8, ep="bias", lay=4, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 32, 112, 321286, 0, 8, ep="res", plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 32, 128, 321286, 0, 8, ep="relu", lay=1, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 32, 16, 320326, 0, 8, lay=2, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 32, 24, 320326, 0, 8, ep="res", lay=3, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 32, 48, 320646, 0, 8, ep="mask", lay=1, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 32, 56, 320646, 0, 8, ep="res+mask", lay=2, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 32, 80, 321286, 0, 8, lay=3, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 32, 88, 321286, 0, 8, ep="res", lay=4, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 32, 112, 321286, 0, 8, ep="mask", plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 32, 128, 321286, 0, 8, ep="res+mask", lay=2, plan_batch=64),
    _mk(F32, FWD, 3, 1, 2, 20, 20, 64, 16, 160326, 0, 16, ep="mask", lay=3, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 2, 20, 20, 32, 32, 160326, 0, 16, lay=4, plan_batch=64),
    _mk(F32, FWD, 3, 1, 2, 20, 20, 64, 40, 160646, 0, 16, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 2, 20, 20, 32, 64, 160646, 0, 16, ep="res", lay=1, plan_batch=64),
    _mk(F32, FWD, 3, 1, 2, 20, 20, 64, 72, 161286, 0, 16, ep="bias+relu", lay=3, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 2, 20, 20, 32, 96, 161286, 0, 16, ep="mask", lay=4, plan_batch=64),
    _mk(F32, FWD, 3, 1, 2, 20, 20, 64, 100, 161286, 0, 16, ep="bias+res+relu", plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 2, 20, 20, 32, 128, 161286, 0, 16, ep="res+mask", lay=1, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 36, 232, 321286, 0, 8, ep="res+mask", lay=2, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 20, 232, 321286, 0, 8, lay=4, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 36, 228, 321286, 0, 8, ep="bias+res+relu+mask", plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 20, 228, 321286, 0, 8, ep="res", lay=1, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 32, 16, 320326, 0, 8, ep="bias", lay=2, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 32, 24, 320326, 0, 8, ep="res", lay=3, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 32, 48, 320646, 0, 8, ep="relu", plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 32, 56, 320646, 0, 8, ep="mask", lay=1, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 32, 80, 321286, 0, 8, lay=2, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 32, 88, 321286, 0, 8, ep="bias+relu", lay=3, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 32, 112, 321286, 0, 8, ep="bias+res+relu", lay=4, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 32, 128, 321286, 0, 8, ep="res+mask", lay=2, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 32, 16, 320326, 0, 8, ep="mask", lay=3, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 32, 24, 320326, 0, 8, ep="res+mask", lay=4, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 32, 48, 320646, 0, 8, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 32, 56, 320646, 0, 8, ep="res", lay=1, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 32, 80, 321286, 0, 8, ep="mask", lay=3, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 32, 88, 321286, 0, 8, ep="res+mask", lay=4, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 32, 112, 321286, 0, 8, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 32, 128, 321286, 0, 8, ep="res", lay=1, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 2, 20, 20, 64, 16, 160326, 0, 16, ep="bias+res+relu+mask", lay=2, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 2, 20, 20, 32, 32, 160326, 0, 16, ep="mask", lay=4, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 2, 20, 20, 64, 40, 160646, 0, 16, ep="bias", plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 2, 20, 20, 32, 64, 160646, 0, 16, ep="res+mask", lay=1, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 2, 20, 20, 64, 72, 161286, 0, 16, ep="res", lay=2, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 2, 20, 20, 32, 96, 161286, 0, 16, lay=3, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 2, 20, 20, 64, 100, 161286, 0, 16, ep="relu", plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 2, 20, 20, 32, 128, 161286, 0, 16, ep="res", lay=1, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 36, 232, 321286, 0, 8, ep="mask", lay=2, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 20, 232, 321286, 0, 8, ep="mask", lay=3, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 36, 228, 321286, 0, 8, lay=4, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 20, 228, 321286, 0, 8, ep="res+mask", lay=1, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 34, 34, 36, 100, 321286, 0, 20, ep="bias+relu", lay=2, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 34, 34, 36, 100, 321286, 0, 20, ep="bias+res+relu", lay=3, plan_batch=64, t256_sliver=0),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 52, 228, 321286, 0, 8, ep="res+mask", lay=4, begin=128, count=100, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 52, 228, 321286, 0, 8, ep="bias+res+relu+mask", begin=128, count=100, plan_batch=64, t256_sliver=0),
    _mk(F32, FWD, 3, 1, 2, 33, 35, 100, 97, 321286, 0, 40, ep="bias", lay=3, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 34, 34, 36, 100, 321286, 0, 20, ep="res", lay=4, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 34, 34, 36, 100, 321286, 0, 20, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 34, 34, 36, 100, 321286, 0, 20, ep="res", lay=1, plan_batch=64, t256_sliver=0),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 52, 228, 321286, 0, 8, ep="mask", lay=2, begin=128, count=100, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 52, 228, 321286, 0, 8, ep="res+mask", lay=4, begin=128, count=100, plan_batch=64, t256_sliver=0),
    _mk(F32, DGRAD, 3, 1, 2, 33, 35, 100, 97, 321286, 0, 40, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 34, 34, 36, 100, 321286, 0, 20, ep="res", lay=1, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 36, 64, 320646, 0, 8, ep="relu", lay=2, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 40, 48, 320646, 0, 8, ep="mask", lay=3, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 45, 64, 320646, 0, 8, ep="mask", plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 13, 48, 320646, 0, 8, ep="res+mask", lay=1, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 4, 64, 320646, 0, 8, lay=2, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 20, 48, 320646, 0, 8, lay=3, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 100, 64, 320646, 0, 8, ep="bias+relu", lay=4, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 33, 64, 320646, 0, 8, ep="bias+res+relu", lay=1, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 34, 40, 320646, 0, 8, ep="res", lay=2, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 35, 64, 320646, 0, 8, ep="res+mask", lay=3, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 36, 40, 320646, 0, 8, ep="mask", lay=4, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 37, 64, 320646, 0, 8, ep="bias+res+relu+mask", plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 38, 40, 320646, 0, 8, ep="res+mask", lay=2, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 39, 64, 320646, 0, 8, ep="bias", lay=3, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 40, 40, 320646, 0, 8, lay=4, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 68, 64, 320646, 0, 8, ep="res", plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 100, 40, 320646, 0, 8, ep="res", lay=1, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 8, 64, 320646, 0, 8, ep="relu", lay=4, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 1, 40, 320646, 0, 8, ep="mask", plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 41, 64, 320646, 0, 8, ep="mask", lay=1, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 45, 40, 320646, 0, 8, ep="res+mask", lay=2, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 63, 64, 320646, 0, 8, lay=3, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 9, 40, 320646, 0, 8, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 20, 64, 320646, 0, 8, ep="bias+relu", lay=1, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 31, 40, 320646, 0, 8, ep="res", lay=2, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 32, 32, 73, 64, 320646, 0, 8, ep="bias+res+relu", lay=3, plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 40, 32, 32, 64, 320646, 0, 10, ep="res+mask", lay=4, plan_batch=64, t256_tiles_per_wg=2),
    _mk(F32, DGRAD, 3, 1, 1, 32, 32, 36, 128, 321286, 0, 8, ep="mask", lay=1, plan_batch=64, t256_tiles_per_wg=3),
    _mk(F32, FWD, 3, 1, 1, 40, 34, 36, 232, 321286, 0, 20, ep="bias+res+relu+mask", lay=2, plan_batch=64, t256_tiles_per_wg=3),
    _mk(F32, FWD, 3, 1, 3, 20, 20, 32, 64, 160646, 0, 24, ep="bias", lay=3, plan_batch=64, t256_tiles_per_wg=2),
    _mk(F32, DGRAD, 3, 1, 1, 33, 17, 32, 100, 161286, 0, 12, ep="res+mask", lay=4, plan_batch=64, t256_tiles_per_wg=2),
    _mk(BF16, FWD, 3, 1, 1, 40, 32, 32, 64, 320646, 0, 10, ep="res", plan_batch=64, t256_tiles_per_wg=2),
    _mk(BF16, DGRAD, 3, 1, 1, 32, 32, 36, 128, 321286, 0, 8, lay=2, plan_batch=64, t256_tiles_per_wg=3),
    _mk(BF16, FWD, 3, 1, 1, 40, 34, 36, 232, 321286, 0, 20, ep="relu", lay=3, plan_batch=64, t256_tiles_per_wg=3),
    _mk(BF16, FWD, 3, 1, 3, 20, 20, 32, 64, 160646, 0, 24, ep="mask", lay=4, plan_batch=64, t256_tiles_per_wg=2),
    _mk(BF16, DGRAD, 3, 1, 1, 33, 17, 32, 100, 161286, 0, 12, ep="res", plan_batch=64, t256_tiles_per_wg=2),
    _mk(F32, FWD, 3, 1, 1, 34, 34, 36, 96, 321286, 0, 20, lay=1, plan_batch=64),
    _mk(F32, DGRAD, 3, 1, 2, 33, 35, 32, 128, 321286, 0, 40, ep="mask", lay=3, plan_batch=64),
    _mk(F32, FWD, 3, 1, 3, 17, 19, 32, 64, 160646, 0, 24, ep="bias+relu", lay=4, plan_batch=64),
    _mk(F32, FWD, 3, 1, 3, 16, 31, 48, 32, 160326, 0, 12, ep="bias+res+relu", plan_batch=128),
    _mk(BF16, FWD, 3, 1, 1, 34, 34, 36, 100, 321286, 0, 20, ep="res+mask", lay=1, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 2, 33, 35, 32, 128, 321286, 0, 40, ep="res+mask", lay=2, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 3, 17, 19, 32, 64, 160646, 0, 24, ep="bias+res+relu+mask", plan_batch=64),
    _mk(BF16, FWD, 3, 1, 3, 16, 31, 48, 32, 160326, 0, 12, ep="bias", lay=1, plan_batch=128),
    # ---- the generic kernels on the launch_bn ladder: tw 8 / 16 / 32 x five tile shapes x HIT 4 / 10 on conv_igemm16_kernel, conv_igemm_kernel (mfma_shape =
    # ---- 32) and conv_bf16_kernel; the conv_igemm16 sliver; column sums
    _mk(F32, FWD, 3, 1, 2, 7, 9, 36, 20, 80320, 0, 16, ep="res", lay=2, f32_big_tile=0),
    _mk(F32, FWD, 3, 2, 2, 13, 15, 36, 20, 80321, 0, 8, ep="relu", lay=3),
    _mk(F32, DGRAD, 3, 1, 2, 7, 9, 20, 64, 80640, 0, 8, lay=4, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 2, 13, 15, 20, 64, 80641, 0, 4, ep="mask", lay=1, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 7, 9, 45, 100, 81280, 0, 8, lay=2, conv1x1_gemm=-1, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 2, 13, 15, 45, 100, 81281, 0, 4, ep="bias+relu", lay=3, plan_batch=4096),
    _mk(F32, DGRAD, 3, 2, 2, 13, 15, 36, 64, 80645, 0, 16, ep="res", lay=4),
    _mk(F32, FWD, 3, 2, 2, 13, 15, 36, 64, 80646, 0, 4, ep="bias+res+relu"),
    _mk(F32, DGRAD, 1, 1, 2, 9, 9, 20, 100, 81285, 0, 16, ep="mask", lay=2, conv1x1_gemm=-1, plan_batch=150),
    _mk(F32, FWD, 3, 2, 1, 19, 15, 20, 100, 81286, 0, 4, ep="res+mask", lay=3, plan_batch=300),
    _mk(F32, FWD, 3, 1, 1, 17, 19, 45, 32, 160320, 0, 24, ep="bias+res+relu+mask", lay=4, f32_big_tile=0),
    _mk(F32, FWD, 3, 2, 1, 9, 33, 45, 32, 160321, 0, 8, ep="bias"),
    _mk(F32, DGRAD, 3, 1, 1, 17, 19, 36, 36, 160640, 0, 12, ep="res+mask", lay=1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 1, 9, 33, 36, 36, 160641, 0, 4, ep="res", lay=3, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 1, 17, 19, 20, 72, 161280, 0, 12, ep="relu", lay=4, conv1x1_gemm=-1, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 1, 9, 33, 20, 72, 161281, 0, 4, ep="mask", plan_batch=4096),
    _mk(F32, DGRAD, 3, 2, 1, 33, 35, 45, 36, 160645, 0, 80, lay=1),
    _mk(F32, FWD, 3, 2, 1, 9, 33, 45, 36, 160646, 0, 8, lay=2),
    _mk(F32, DGRAD, 1, 1, 1, 7, 19, 36, 72, 161285, 0, 8, ep="res", lay=4, conv1x1_gemm=-1, plan_batch=150),
    _mk(F32, FWD, 3, 2, 1, 13, 33, 36, 72, 161286, 0, 8, ep="bias+relu", plan_batch=150),
    _mk(F32, FWD, 3, 1, 1, 5, 37, 20, 20, 320320, 0, 16, ep="bias+res+relu", lay=1, f32_big_tile=0),
    _mk(F32, FWD, 3, 2, 1, 3, 65, 20, 20, 320321, 0, 8, ep="res+mask", lay=2),
    _mk(F32, DGRAD, 3, 1, 1, 5, 37, 45, 64, 320640, 0, 8, ep="mask", lay=3, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 1, 3, 65, 45, 64, 320641, 0, 4, ep="bias+res+relu+mask", lay=1, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 1, 5, 37, 36, 100, 321280, 0, 8, ep="bias", lay=2, conv1x1_gemm=-1, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 1, 3, 65, 36, 100, 321281, 0, 4, ep="res", lay=3, plan_batch=4096),
    _mk(F32, DGRAD, 3, 1, 1, 5, 37, 20, 64, 320645, 0, 12, ep="res+mask", lay=4, f32_big_tile=0),
    _mk(F32, FWD, 3, 2, 1, 3, 65, 20, 64, 320646, 0, 4, ep="relu"),
    _mk(F32, DGRAD, 1, 1, 1, 3, 37, 45, 100, 321285, 0, 8, lay=2, conv1x1_gemm=-1, plan_batch=150),
    _mk(F32, FWD, 3, 2, 1, 5, 65, 45, 100, 321286, 0, 8, ep="mask", lay=3, plan_batch=150),
    _mk(F32, FWD, 3, 1, 2, 7, 9, 36, 32, 80320, 0, 16, lay=4, mfma_shape=32),
    _mk(F32, FWD, 3, 2, 2, 13, 15, 36, 32, 80321, 0, 8, ep="bias+relu", mfma_shape=32),
    _mk(F32, DGRAD, 3, 1, 2, 7, 9, 20, 36, 80640, 0, 8, ep="res", lay=1, mfma_shape=32, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 2, 13, 15, 20, 36, 80641, 0, 4, ep="bias+res+relu", lay=3, mfma_shape=32, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 7, 9, 45, 72, 81280, 0, 8, ep="res+mask", lay=4, conv1x1_gemm=-1, mfma_shape=32, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 2, 13, 15, 45, 72, 81281, 0, 4, ep="bias+res+relu+mask", mfma_shape=32, plan_batch=4096),
    _mk(F32, DGRAD, 3, 2, 2, 13, 15, 36, 36, 80645, 0, 16, ep="mask", lay=1, mfma_shape=32),
    _mk(F32, FWD, 3, 2, 2, 13, 15, 36, 36, 80646, 0, 4, ep="bias", lay=2, mfma_shape=32),
    _mk(F32, DGRAD, 1, 1, 2, 9, 9, 20, 72, 81285, 0, 16, ep="res+mask", lay=4, conv1x1_gemm=-1, mfma_shape=32, plan_batch=150),
    _mk(F32, FWD, 3, 2, 1, 19, 15, 20, 72, 81286, 0, 4, ep="res", mfma_shape=32, plan_batch=300),
    _mk(F32, FWD, 3, 1, 1, 17, 19, 45, 20, 160320, 0, 24, ep="relu", lay=1, mfma_shape=32),
    _mk(F32, FWD, 3, 2, 1, 9, 33, 45, 20, 160321, 0, 8, ep="mask", lay=2, mfma_shape=32),
    _mk(F32, DGRAD, 3, 1, 1, 17, 19, 36, 64, 160640, 0, 12, lay=3, mfma_shape=32, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 1, 9, 33, 36, 64, 160641, 0, 4, mfma_shape=32, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 1, 17, 19, 20, 100, 161280, 0, 12, ep="bias+relu", lay=1, conv1x1_gemm=-1, mfma_shape=32, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 1, 9, 33, 20, 100, 161281, 0, 4, ep="bias+res+relu", lay=2, mfma_shape=32, plan_batch=4096),
    _mk(F32, DGRAD, 3, 2, 1, 33, 35, 45, 64, 160645, 0, 80, ep="res", lay=3, mfma_shape=32),
    _mk(F32, FWD, 3, 2, 1, 9, 33, 45, 64, 160646, 0, 8, ep="res+mask", lay=4, mfma_shape=32),
    _mk(F32, DGRAD, 1, 1, 1, 7, 19, 36, 100, 161285, 0, 8, ep="mask", lay=2, conv1x1_gemm=-1, mfma_shape=32, plan_batch=150),
    _mk(F32, FWD, 3, 2, 1, 13, 33, 36, 100, 161286, 0, 8, ep="bias+res+relu+mask", lay=3, mfma_shape=32, plan_batch=150),
    _mk(F32, FWD, 3, 1, 1, 5, 37, 20, 32, 320320, 0, 16, ep="bias", lay=4, mfma_shape=32),
    _mk(F32, FWD, 3, 2, 1, 3, 65, 20, 32, 320321, 0, 8, ep="res", mfma_shape=32),
    _mk(F32, DGRAD, 3, 1, 1, 5, 37, 45, 36, 320640, 0, 8, ep="res+mask", lay=1, mfma_shape=32, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 1, 3, 65, 45, 36, 320641, 0, 4, ep="relu", lay=3, mfma_shape=32, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 1, 5, 37, 36, 72, 321280, 0, 8, ep="mask", lay=4, conv1x1_gemm=-1, mfma_shape=32, plan_batch=4096),
    _mk(F32, FWD, 3, 2, 1, 3, 65, 36, 72, 321281, 0, 4, mfma_shape=32, plan_batch=4096),
    _mk(F32, DGRAD, 3, 1, 1, 5, 37, 20, 36, 320645, 0, 12, lay=1, mfma_shape=32),
    _mk(F32, FWD, 3, 2, 1, 3, 65, 20, 36, 320646, 0, 4, ep="bias+relu", lay=2, mfma_shape=32),
    _mk(F32, DGRAD, 1, 1, 1, 3, 37, 45, 72, 321285, 0, 8, ep="res", lay=4, conv1x1_gemm=-1, mfma_shape=32, plan_batch=150),
    _mk(F32, FWD, 3, 2, 1, 5, 65, 45, 72, 321286, 0, 8, ep="bias+res+relu", mfma_shape=32, plan_batch=150),
    _mk(BF16, FWD, 3, 1, 2, 7, 9, 36, 20, 80320, 0, 16, ep="res+mask", lay=1, bf16_big_tile=0),
    _mk(BF16, FWD, 3, 2, 2, 13, 15, 36, 20, 80321, 0, 8, ep="bias+res+relu+mask", lay=2),
    _mk(BF16, DGRAD, 3, 1, 2, 7, 9, 20, 64, 80640, 0, 8, ep="mask", lay=3, bf16_big_tile=0, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 2, 13, 15, 20, 64, 80641, 0, 4, ep="bias", plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 7, 9, 45, 100, 81280, 0, 8, ep="res", lay=1, conv1x1_gemm=-1, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 2, 13, 15, 45, 100, 81281, 0, 4, ep="relu", lay=2, plan_batch=4096),
    _mk(BF16, DGRAD, 3, 2, 2, 13, 15, 36, 64, 80645, 0, 16, ep="res+mask", lay=3),
    _mk(BF16, FWD, 3, 2, 2, 13, 15, 36, 64, 80646, 0, 4, ep="mask", lay=4),
    _mk(BF16, DGRAD, 1, 1, 2, 9, 9, 20, 100, 81285, 0, 16, lay=1, conv1x1_gemm=-1, plan_batch=150),
    _mk(BF16, FWD, 3, 2, 1, 19, 15, 20, 100, 81286, 0, 4, lay=2, plan_batch=300),
    _mk(BF16, FWD, 3, 1, 1, 17, 19, 45, 32, 160320, 0, 24, ep="bias+relu", lay=3, bf16_big_tile=0),
    _mk(BF16, FWD, 3, 2, 1, 9, 33, 45, 32, 160321, 0, 8, ep="bias+res+relu", lay=4),
    _mk(BF16, DGRAD, 3, 1, 1, 17, 19, 36, 36, 160640, 0, 8, ep="res", bf16_big_tile=0, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 1, 9, 33, 36, 36, 160641, 0, 4, ep="res+mask", lay=3, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 1, 17, 19, 20, 72, 161280, 0, 12, ep="bias+res+relu+mask", lay=4, conv1x1_gemm=-1, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 1, 9, 33, 20, 72, 161281, 0, 4, ep="bias", plan_batch=4096),
    _mk(BF16, DGRAD, 3, 2, 1, 33, 35, 45, 36, 160645, 0, 80, ep="mask", lay=1),
    _mk(BF16, FWD, 3, 2, 1, 9, 33, 45, 36, 160646, 0, 8, ep="res", lay=2),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 19, 36, 72, 161285, 0, 8, ep="res+mask", lay=4, conv1x1_gemm=-1, plan_batch=150),
    _mk(BF16, FWD, 3, 2, 1, 13, 33, 36, 72, 161286, 0, 8, ep="relu", plan_batch=150),
    _mk(BF16, FWD, 3, 1, 1, 5, 37, 20, 20, 320320, 0, 16, ep="mask", lay=1, bf16_big_tile=0),
    _mk(BF16, FWD, 3, 2, 1, 3, 65, 20, 20, 320321, 0, 8, lay=2),
    _mk(BF16, DGRAD, 3, 1, 1, 5, 37, 45, 64, 320640, 0, 4, lay=3, bf16_big_tile=0, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 1, 3, 65, 45, 64, 320641, 0, 4, ep="bias+relu", plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 1, 5, 37, 36, 100, 321280, 0, 8, ep="bias+res+relu", lay=1, conv1x1_gemm=-1, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 1, 3, 65, 36, 100, 321281, 0, 4, ep="res+mask", lay=2, plan_batch=4096),
    _mk(BF16, DGRAD, 3, 1, 1, 5, 37, 20, 64, 320645, 0, 12, ep="res", lay=3, bf16_big_tile=0),
    _mk(BF16, FWD, 3, 2, 1, 3, 65, 20, 64, 320646, 0, 4, ep="bias+res+relu+mask", lay=4),
    _mk(BF16, DGRAD, 1, 1, 1, 3, 37, 45, 100, 321285, 0, 8, ep="mask", lay=1, conv1x1_gemm=-1, plan_batch=150),
    _mk(BF16, FWD, 3, 2, 1, 5, 65, 45, 100, 321286, 0, 8, ep="bias", lay=2, plan_batch=150),
    _mk(F32, DGRAD, 3, 1, 1, 17, 19, 20, 65, 161280, 0, 12, ep="res+mask", lay=3, conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, DGRAD, 3, 1, 1, 17, 19, 20, 65, 161280, 0, 12, ep="res+mask+colsum", lay=4, conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 1, 17, 19, 20, 65, 161280, 0, 12, ep="res", conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 1, 17, 19, 20, 65, 161280, 0, 12, ep="bias+res+relu+colsum+colsumsq", lay=2, conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 3, 1, 1, 17, 19, 36, 66, 161280, 0, 12, ep="relu", lay=3, conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 3, 1, 1, 17, 19, 36, 66, 161280, 0, 12, ep="bias+res+relu+colsum+colsumsq", lay=4, conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 1, 17, 19, 36, 66, 161280, 0, 12, conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 1, 17, 19, 36, 66, 161280, 0, 12, ep="res+mask+colsum", lay=1, conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, DGRAD, 3, 1, 1, 17, 19, 20, 99, 161280, 0, 12, ep="res", lay=4, conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, DGRAD, 3, 1, 1, 17, 19, 20, 99, 161280, 0, 12, ep="res+mask+colsum", conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 1, 17, 19, 20, 99, 161280, 0, 12, ep="mask", lay=1, conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 1, 17, 19, 20, 99, 161280, 0, 12, ep="bias+res+relu+colsum+colsumsq", lay=2, conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 3, 1, 1, 17, 19, 36, 100, 161280, 0, 12, lay=3, conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 3, 1, 1, 17, 19, 36, 100, 161280, 0, 12, ep="bias+res+relu+colsum+colsumsq", conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 1, 17, 19, 36, 100, 161280, 0, 12, ep="mask", lay=1, conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 1, 17, 19, 36, 100, 161280, 0, 12, ep="res+mask+colsum", lay=2, conv1x1_gemm=-1, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 3, 1, 2, 5, 37, 20, 228, 321280, 0, 16, ep="bias+relu", lay=3, begin=128, count=100, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 3, 1, 2, 5, 37, 20, 228, 321280, 0, 16, ep="bias+res+relu", lay=4, begin=0, count=128, f32_big_tile=0, plan_batch=4096),
    _mk(F32, FWD, 3, 1, 2, 9, 11, 20, 24, 80320, 0, 16, ep="bias+relu+colsum+colsumsq", lay=1),
    _mk(F32, FWD, 3, 1, 2, 17, 19, 36, 100, 160645, 0, 40, ep="bias+res+relu+mask+colsum+colsumsq", lay=2),
    _mk(F32, FWD, 3, 2, 2, 13, 15, 20, 40, 80646, 0, 4, ep="bias+colsum", lay=3),
    _mk(F32, DGRAD, 3, 1, 1, 5, 37, 36, 64, 320640, 0, 8, ep="res+mask+colsum", lay=4, plan_batch=4096),
    _mk(F32, DGRAD, 3, 2, 2, 9, 10, 32, 36, 80645, 0, 16, ep="mask+colsum"),
    _mk(F32, FWD, 1, 1, 2, 7, 9, 36, 100, 80645, 0, 8, ep="bias+colsum+colsumsq", lay=2),
    _mk(F32, FWD, 3, 1, 2, 9, 11, 20, 24, 80320, 0, 16, ep="bias+relu+colsum+colsumsq", lay=3, mfma_shape=32),
    _mk(F32, FWD, 3, 1, 2, 17, 19, 36, 100, 160645, 0, 40, ep="bias+res+relu+mask+colsum+colsumsq", lay=4, mfma_shape=32),
    _mk(F32, FWD, 3, 2, 2, 13, 15, 20, 40, 80646, 0, 4, ep="bias+colsum", mfma_shape=32),
    _mk(F32, DGRAD, 3, 1, 1, 5, 37, 36, 64, 320640, 0, 8, ep="res+mask+colsum", lay=1, mfma_shape=32, plan_batch=4096),
    _mk(F32, DGRAD, 3, 2, 2, 9, 10, 32, 36, 80645, 0, 16, ep="mask+colsum", lay=3, mfma_shape=32),
    _mk(F32, FWD, 1, 1, 2, 7, 9, 36, 100, 80645, 0, 8, ep="bias+colsum+colsumsq", lay=4, mfma_shape=32),
    _mk(F32, FWD, 3, 1, 1, 32, 32, 32, 64, 320640, 0, 16, ep="bias+relu+colsum+colsumsq", plan_batch=64),
    _mk(F32, FWD, 3, 1, 1, 8, 8, 256, 64, 80645, 0, 2, ep="bias+colsum", lay=1),
    # ---- split-K: 2 / 3 / middle / 32 splits, ragged last splits, slab rows wider than the range, channel ranges, every epilogue operand, bf16 and fp32
    # ---- outputs, short and missing workspaces
    _mk(F32, FWD, 3, 1, 1, 8, 8, 256, 64, 8080645, 32768, 2, ep="res+mask", lay=2),
    _mk(F32, FWD, 3, 1, 1, 7, 7, 136, 36, 3080645, 5292, 2, ep="bias+res+relu+mask"),
    _mk(F32, FWD, 3, 1, 1, 8, 8, 128, 32, 4080320, 8192, 4, ep="bias", lay=1),
    _mk(F32, FWD, 1, 1, 1, 7, 9, 264, 200, 2081280, 25200, 4, ep="res", lay=2, conv1x1_gemm=-1, plan_batch=50),
    _mk(F32, FWD, 3, 1, 1, 7, 9, 264, 200, 2081280, 25200, 4, ep="relu", lay=3, plan_batch=50),
    _mk(F32, FWD, 1, 1, 1, 7, 7, 1024, 32, 32080320, 50176, 4, ep="mask", lay=4),
    _mk(F32, FWD, 3, 1, 1, 7, 7, 1024, 32, 32080320, 50176, 4, lay=1),
    _mk(F32, FWD, 1, 1, 1, 7, 7, 300, 37, 7080645, 13720, 2, ep="bias+relu", lay=2),
    _mk(F32, FWD, 3, 1, 1, 7, 7, 200, 33, 5080645, 8820, 2, ep="bias+res+relu", lay=3),
    _mk(F32, FWD, 3, 1, 2, 7, 9, 1024, 200, 22080645, 554400, 8, ep="res+mask", lay=4),
    _mk(F32, FWD, 3, 1, 1, 8, 8, 200, 200, 5080645, 23040, 2, ep="bias+res+relu+mask", begin=128, count=72),
    _mk(F32, FWD, 1, 1, 2, 7, 9, 520, 228, 11080645, 138600, 8, ep="bias", lay=2, begin=128, count=100, conv1x1_gemm=-1),
    _mk(BF16, FWD, 3, 1, 1, 8, 8, 256, 64, 4080645, 16384, 2, ep="res", lay=3),
    _mk(BF16, FWD, 3, 1, 1, 7, 9, 264, 200, 2081280, 25200, 4, ep="relu", lay=4, plan_batch=64),
    _mk(BF16, FWD, 1, 1, 1, 7, 9, 264, 200, 2081280, 25200, 4, ep="mask", conv1x1_gemm=-1, plan_batch=64),
    _mk(BF16, FWD, 3, 1, 1, 7, 9, 256, 32, 3080320, 6048, 8, lay=1, plan_batch=64),
    _mk(BF16, FWD, 1, 1, 1, 7, 7, 300, 37, 5080645, 9800, 2, ep="bias+relu", lay=3, conv1x1_gemm=-1),
    _mk(BF16, FWD, 3, 1, 1, 7, 7, 520, 33, 6080645, 10584, 2, ep="bias+res+relu", lay=4),
    _mk(BF16, FWD, 1, 1, 1, 7, 7, 2048, 32, 32080320, 50176, 4, ep="res+mask", conv1x1_gemm=-1),
    _mk(BF16, FWD, 3, 1, 1, 7, 7, 1024, 32, 16080320, 25088, 4, ep="bias+res+relu+mask", lay=1),
    _mk(BF16, FWD, 3, 1, 1, 8, 8, 520, 200, 6080645, 27648, 2, ep="bias", lay=2, begin=128, count=72),
    _mk(BF16, FWD, 3, 1, 1, 8, 8, 264, 100, 3080645, 19200, 2, ep="bias+relu+y_f32", lay=4),
    _mk(BF16, FWD, 1, 1, 1, 7, 7, 300, 37, 5080645, 9800, 2, ep="bias+y_f32", conv1x1_gemm=-1),
    _mk(F32, DGRAD, 3, 1, 1, 8, 8, 256, 64, 8080645, 32768, 2, ep="res+mask", lay=1),
    _mk(F32, DGRAD, 3, 1, 1, 7, 7, 136, 36, 3080645, 5292, 2, lay=2),
    _mk(F32, DGRAD, 3, 1, 1, 8, 8, 128, 32, 4080320, 8192, 4, ep="res", lay=3),
    _mk(F32, DGRAD, 1, 1, 1, 7, 9, 264, 200, 2081280, 25200, 4, ep="mask", lay=1, conv1x1_gemm=-1, plan_batch=50),
    _mk(F32, DGRAD, 3, 1, 1, 7, 9, 264, 200, 2081280, 25200, 4, ep="res+mask", lay=2, plan_batch=50),
    _mk(F32, DGRAD, 1, 1, 1, 7, 7, 1024, 32, 32080320, 50176, 4, lay=3),
    _mk(F32, DGRAD, 3, 1, 1, 7, 7, 1024, 32, 32080320, 50176, 4, ep="res", lay=4),
    _mk(F32, DGRAD, 1, 1, 1, 7, 7, 300, 37, 7080645, 13720, 2, ep="mask"),
    _mk(F32, DGRAD, 3, 1, 1, 7, 7, 200, 33, 5080645, 8820, 2, ep="res+mask", lay=2),
    _mk(F32, DGRAD, 3, 1, 2, 7, 9, 1024, 200, 22080645, 554400, 8, lay=3),
    _mk(F32, DGRAD, 3, 1, 1, 8, 8, 200, 200, 5080645, 23040, 2, ep="res", lay=4, begin=128, count=72),
    _mk(F32, DGRAD, 1, 1, 2, 7, 9, 520, 228, 11080645, 138600, 8, ep="mask", begin=128, count=100, conv1x1_gemm=-1),
    _mk(BF16, DGRAD, 3, 1, 1, 8, 8, 256, 64, 4080645, 16384, 2, ep="res+mask", lay=1),
    _mk(BF16, DGRAD, 3, 1, 1, 7, 9, 264, 200, 2081280, 25200, 4, lay=3, plan_batch=64),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 9, 264, 200, 2081280, 25200, 4, ep="res", lay=4, conv1x1_gemm=-1, plan_batch=64),
    _mk(BF16, DGRAD, 3, 1, 1, 7, 9, 256, 32, 3080320, 6048, 8, ep="mask", plan_batch=64),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 7, 300, 37, 5080645, 9800, 2, ep="res+mask", lay=1, conv1x1_gemm=-1),
    _mk(BF16, DGRAD, 3, 1, 1, 7, 7, 520, 33, 6080645, 10584, 2, lay=2),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 7, 2048, 32, 32080320, 50176, 4, ep="res", lay=4, conv1x1_gemm=-1),
    _mk(BF16, DGRAD, 3, 1, 1, 7, 7, 1024, 32, 16080320, 25088, 4, ep="mask"),
    _mk(BF16, DGRAD, 3, 1, 1, 8, 8, 520, 200, 6080645, 27648, 2, ep="res+mask", lay=1, begin=128, count=72),
    _mk(BF16, DGRAD, 3, 1, 1, 8, 8, 264, 100, 3080645, 19200, 2, ep="y_f32", lay=2),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 7, 300, 37, 5080645, 9800, 2, ep="y_f32", lay=3, conv1x1_gemm=-1),
    _mk(F32, FWD, 3, 1, 1, 7, 9, 256, 36, 8080645, 18144, 4),
    _mk(F32, FWD, 3, 1, 1, 7, 9, 256, 36, 8080645, 18144, 4, ep="bias", lay=1),
    _mk(F32, FWD, 3, 1, 1, 7, 9, 256, 36, 8080645, 18144, 4, ep="res", lay=2),
    _mk(F32, FWD, 3, 1, 1, 7, 9, 256, 36, 8080645, 18144, 4, ep="relu", lay=3),
    _mk(F32, FWD, 3, 1, 1, 7, 9, 256, 36, 8080645, 18144, 4, ep="mask", lay=4),
    _mk(F32, FWD, 3, 1, 1, 7, 9, 256, 36, 8080645, 18144, 4, ep="bias+res+relu+mask", lay=2),
    _mk(F32, DGRAD, 1, 1, 2, 7, 7, 264, 100, 6080645, 58800, 4, lay=3, conv1x1_gemm=-1),
    _mk(F32, DGRAD, 1, 1, 2, 7, 7, 264, 100, 6080645, 58800, 4, ep="res", lay=4, conv1x1_gemm=-1),
    _mk(F32, DGRAD, 1, 1, 2, 7, 7, 264, 100, 6080645, 58800, 4, ep="mask", conv1x1_gemm=-1),
    _mk(F32, DGRAD, 1, 1, 2, 7, 7, 264, 100, 6080645, 58800, 4, ep="res+mask", lay=1, conv1x1_gemm=-1),
    _mk(BF16, FWD, 3, 1, 1, 7, 9, 520, 36, 6080645, 13608, 4, lay=3),
    _mk(BF16, FWD, 3, 1, 1, 7, 9, 520, 36, 6080645, 13608, 4, ep="bias", lay=4),
    _mk(BF16, FWD, 3, 1, 1, 7, 9, 520, 36, 6080645, 13608, 4, ep="res"),
    _mk(BF16, FWD, 3, 1, 1, 7, 9, 520, 36, 6080645, 13608, 4, ep="relu", lay=1),
    _mk(BF16, FWD, 3, 1, 1, 7, 9, 520, 36, 6080645, 13608, 4, ep="mask", lay=2),
    _mk(BF16, FWD, 3, 1, 1, 7, 9, 520, 36, 6080645, 13608, 4, ep="bias+res+relu+mask", lay=4),
    _mk(BF16, DGRAD, 1, 1, 2, 7, 7, 520, 100, 6080645, 58800, 4, conv1x1_gemm=-1),
    _mk(BF16, DGRAD, 1, 1, 2, 7, 7, 520, 100, 6080645, 58800, 4, ep="res", lay=1, conv1x1_gemm=-1),
    _mk(BF16, DGRAD, 1, 1, 2, 7, 7, 520, 100, 6080645, 58800, 4, ep="mask", lay=2, conv1x1_gemm=-1),
    _mk(BF16, DGRAD, 1, 1, 2, 7, 7, 520, 100, 6080645, 58800, 4, ep="res+mask", lay=3, conv1x1_gemm=-1),
    _mk(F32, FWD, 3, 1, 1, 8, 8, 256, 64, 80645, 32768, 2, ep="bias+res+relu+mask", ws="short"),
    _mk(F32, DGRAD, 1, 1, 1, 7, 7, 300, 37, 80645, 13720, 2, ep="res+mask", lay=1, ws="short", conv1x1_gemm=-1),
    _mk(F32, FWD, 3, 1, 1, 8, 8, 520, 200, 80645, 50688, 2, ep="res", lay=2, ws="short", begin=128, count=72),
    _mk(F32, FWD, 3, 1, 1, 8, 8, 256, 64, 80645, 32768, 2, ep="bias+res+relu+mask", lay=3, ws="none"),
    _mk(F32, DGRAD, 1, 1, 1, 7, 7, 300, 37, 80645, 13720, 2, ep="res+mask", lay=4, ws="none", conv1x1_gemm=-1),
    _mk(F32, FWD, 3, 1, 1, 8, 8, 520, 200, 80645, 50688, 2, ep="relu", lay=1, ws="none", begin=128, count=72),
    _mk(BF16, FWD, 3, 1, 1, 8, 8, 256, 64, 80645, 16384, 2, ep="bias+res+relu+mask", lay=2, ws="short"),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 7, 300, 37, 80645, 9800, 2, ep="res+mask", lay=3, ws="short", conv1x1_gemm=-1),
    _mk(BF16, FWD, 3, 1, 1, 8, 8, 520, 200, 80645, 27648, 2, ep="mask", lay=4, ws="short", begin=128, count=72),
    _mk(BF16, FWD, 3, 1, 1, 8, 8, 256, 64, 80645, 16384, 2, ep="bias+res+relu+mask", ws="none"),
    _mk(BF16, DGRAD, 1, 1, 1, 7, 7, 300, 37, 80645, 9800, 2, ep="res+mask", lay=3, ws="none", conv1x1_gemm=-1),
    _mk(BF16, FWD, 3, 1, 1, 8, 8, 520, 200, 80645, 27648, 2, lay=4, ws="none", begin=128, count=72),
    # ---- stride-2 dgrad: odd and even sides independently, one-pixel-high gradients
    _mk(F32, DGRAD, 3, 2, 1, 9, 9, 32, 32, 80320, 0, 16),
    _mk(F32, DGRAD, 3, 2, 1, 9, 10, 32, 36, 80645, 0, 8, ep="res", lay=1),
    _mk(F32, DGRAD, 3, 2, 1, 10, 9, 32, 32, 80320, 0, 16, ep="mask", lay=2),
    _mk(F32, DGRAD, 3, 2, 1, 10, 10, 32, 36, 80645, 0, 8, ep="res+mask", lay=4),
    _mk(F32, DGRAD, 3, 2, 2, 1, 9, 32, 32, 80320, 0, 32),
    _mk(F32, DGRAD, 3, 2, 2, 2, 11, 32, 32, 80320, 0, 32, ep="res", lay=1),
    _mk(F32, DGRAD, 3, 2, 2, 7, 2, 32, 32, 80320, 0, 32, ep="mask", lay=2),
    _mk(F32, DGRAD, 3, 2, 1, 33, 34, 32, 32, 160320, 0, 96, ep="res+mask", lay=3),
    _mk(BF16, DGRAD, 3, 2, 1, 9, 9, 32, 32, 80320, 0, 16),
    _mk(BF16, DGRAD, 3, 2, 1, 9, 10, 32, 36, 80645, 0, 8, ep="res", lay=1),
    _mk(BF16, DGRAD, 3, 2, 1, 10, 9, 32, 32, 80320, 0, 16, ep="mask", lay=2),
    _mk(BF16, DGRAD, 3, 2, 1, 10, 10, 32, 36, 80645, 0, 8, ep="res+mask", lay=3),
    _mk(BF16, DGRAD, 3, 2, 2, 1, 9, 32, 32, 80320, 0, 32, lay=4),
    _mk(BF16, DGRAD, 3, 2, 2, 2, 11, 32, 32, 80320, 0, 32, ep="res", lay=1),
    _mk(BF16, DGRAD, 3, 2, 2, 7, 2, 32, 32, 80320, 0, 32, ep="mask", lay=2),
    _mk(BF16, DGRAD, 3, 2, 1, 33, 34, 32, 32, 160320, 0, 96, ep="res+mask", lay=3),
    _mk(F32, DGRAD, 3, 2, 1, 9, 9, 32, 32, 80320, 0, 16, ep="res+mask+colsum", lay=4),
    _mk(F32, DGRAD, 3, 2, 2, 1, 9, 32, 36, 80645, 0, 16, ep="colsum"),
    # ---- the 1x1 families: smallk, head, the flat-pixel GEMM direct and staged, pixel shuffle with and without a tail
    _mk(F32, FWD, 1, 1, 3, 9, 11, 1, 16, 9, 0, 24, ep="bias", lay=2),
    _mk(F32, DGRAD, 1, 1, 3, 9, 11, 1, 99, 9, 0, 24, ep="res", lay=3),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 1, 100, 9, 0, 24, ep="mask", lay=4),
    _mk(F32, DGRAD, 1, 1, 3, 9, 11, 5, 16, 9, 0, 24, ep="res+mask"),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 5, 99, 9, 0, 24, ep="bias", lay=1),
    _mk(F32, DGRAD, 1, 1, 3, 9, 11, 5, 100, 9, 0, 24, ep="res", lay=4),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 8, 16, 9, 0, 24, ep="mask"),
    _mk(F32, DGRAD, 1, 1, 3, 9, 11, 8, 99, 9, 0, 24, ep="res+mask", lay=1),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 8, 100, 9, 0, 24, ep="bias", lay=2),
    _mk(BF16, DGRAD, 1, 1, 3, 9, 11, 1, 16, 9, 0, 24, ep="res", lay=3),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 1, 99, 9, 0, 24, ep="mask"),
    _mk(BF16, DGRAD, 1, 1, 3, 9, 11, 1, 100, 9, 0, 24, ep="res+mask", lay=1),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 5, 16, 9, 0, 24, ep="bias", lay=2),
    _mk(BF16, DGRAD, 1, 1, 3, 9, 11, 5, 99, 9, 0, 24, ep="res", lay=3),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 5, 100, 9, 0, 24, ep="mask", lay=4),
    _mk(BF16, DGRAD, 1, 1, 3, 9, 11, 8, 16, 9, 0, 24, ep="res+mask", lay=1),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 8, 99, 9, 0, 24, ep="bias", lay=2),
    _mk(BF16, DGRAD, 1, 1, 3, 9, 11, 8, 100, 9, 0, 24, ep="res", lay=3),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 9, 1, 11, 0, 24, lay=4),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 100, 1, 11, 0, 24, ep="relu"),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 128, 1, 11, 4752, 24, ep="bias", lay=2),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 9, 2, 11, 0, 24, ep="bias+relu", lay=3),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 100, 2, 11, 0, 24, lay=4),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 128, 2, 11, 4752, 24, ep="relu"),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 9, 5, 11, 0, 24, ep="bias", lay=1),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 100, 5, 11, 0, 24, ep="bias+relu", lay=3),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 128, 5, 11, 9504, 24, lay=4),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 9, 16, 11, 0, 24, ep="relu"),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 100, 16, 11, 0, 24, ep="bias", lay=1),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 128, 16, 11, 19008, 24, ep="bias+relu", lay=2),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 9, 1, 11, 0, 24),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 100, 1, 11, 0, 24, ep="relu", lay=1),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 128, 1, 11, 0, 24, ep="bias", lay=2),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 9, 2, 11, 0, 24, ep="bias+relu", lay=3),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 100, 2, 11, 0, 24, lay=4),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 128, 2, 11, 0, 24, ep="relu", lay=1),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 9, 5, 11, 0, 24, ep="bias", lay=2),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 100, 5, 11, 0, 24, ep="bias+relu", lay=3),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 128, 5, 11, 0, 24, lay=4),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 9, 16, 11, 0, 24, ep="relu"),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 100, 16, 11, 0, 24, ep="bias", lay=2),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 128, 16, 11, 0, 24, ep="bias+relu", lay=3),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 9, 1, 11, 0, 24, ep="y_f32", lay=4),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 100, 1, 11, 0, 24, ep="relu+y_f32"),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 128, 1, 11, 0, 24, ep="bias+y_f32", lay=1),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 9, 2, 11, 0, 24, ep="bias+relu+y_f32", lay=3),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 100, 2, 11, 0, 24, ep="y_f32", lay=4),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 128, 2, 11, 0, 24, ep="relu+y_f32"),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 9, 5, 11, 0, 24, ep="bias+y_f32", lay=1),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 100, 5, 11, 0, 24, ep="bias+relu+y_f32", lay=2),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 128, 5, 11, 0, 24, ep="y_f32", lay=4),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 9, 16, 11, 0, 24, ep="relu+y_f32"),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 100, 16, 11, 0, 24, ep="bias+y_f32", lay=1),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 128, 16, 11, 0, 24, ep="bias+relu+y_f32", lay=2),
    _mk(F32, FWD, 1, 1, 3, 9, 11, 100, 5, 11, 0, 24, ep="bias", lay=3, conv_head1x1=2),
    _mk(F32, DGRAD, 1, 1, 2, 7, 9, 36, 3, 11, 0, 16, lay=1),
    _mk(BF16, FWD, 1, 1, 3, 9, 11, 100, 5, 11, 0, 24, ep="bias", lay=2, conv_head1x1=2),
    _mk(BF16, DGRAD, 1, 1, 2, 7, 9, 36, 3, 11, 0, 16, lay=3),
    _mk(F32, FWD, 1, 1, 3, 7, 9, 64, 132, 8, 0, 12, ep="bias+relu", lay=4, conv1x1_gemm=1, plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 3, 7, 9, 96, 96, 8, 0, 12, conv1x1_gemm=1, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 11, 13, 32, 200, 8, 0, 8, ep="bias+res+relu", lay=2, begin=128, count=72, conv1x1_gemm=1, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 11, 13, 32, 200, 8, 0, 8, ep="res+mask", lay=3, begin=0, count=128, conv1x1_gemm=1, plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 1, 17, 19, 160, 260, 8, 0, 12, ep="res", lay=4, conv1x1_gemm=1, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 3, 7, 9, 64, 132, 8, 0, 12, ep="bias+res+relu+mask", conv1x1_gemm=2, plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 3, 7, 9, 96, 96, 8, 0, 12, ep="mask", lay=1, conv1x1_gemm=2, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 11, 13, 32, 200, 8, 0, 8, ep="bias", lay=3, begin=128, count=72, conv1x1_gemm=2, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 11, 13, 32, 200, 8, 0, 8, ep="res", lay=4, begin=0, count=128, conv1x1_gemm=2, plan_batch=4096),
    _mk(F32, DGRAD, 1, 1, 1, 17, 19, 160, 260, 8, 0, 12, ep="res+mask", conv1x1_gemm=2, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 3, 7, 9, 64, 132, 8, 0, 12, ep="relu", lay=1, conv1x1_gemm=1, plan_batch=4096),
    _mk(BF16, DGRAD, 1, 1, 3, 7, 9, 96, 96, 8, 0, 12, lay=2, conv1x1_gemm=1, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 11, 13, 32, 200, 8, 0, 8, ep="mask", lay=4, begin=128, count=72, conv1x1_gemm=1, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 11, 13, 32, 200, 8, 0, 8, begin=0, count=128, conv1x1_gemm=1, plan_batch=4096),
    _mk(BF16, DGRAD, 1, 1, 1, 17, 19, 160, 260, 8, 0, 12, ep="res", lay=1, conv1x1_gemm=1, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 3, 7, 9, 64, 132, 8, 0, 12, ep="bias+relu", lay=2, conv1x1_gemm=2, plan_batch=4096),
    _mk(BF16, DGRAD, 1, 1, 3, 7, 9, 96, 96, 8, 0, 12, ep="mask", lay=3, conv1x1_gemm=2, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 11, 13, 32, 200, 8, 0, 8, ep="bias+res+relu", begin=128, count=72, conv1x1_gemm=2, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 11, 13, 32, 200, 8, 0, 8, ep="res+mask", lay=1, begin=0, count=128, conv1x1_gemm=2, plan_batch=4096),
    _mk(BF16, DGRAD, 1, 1, 1, 17, 19, 160, 260, 8, 0, 12, ep="res+mask", lay=2, conv1x1_gemm=2, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 3, 7, 9, 64, 132, 8, 0, 12, ep="bias+res+relu+mask", lay=3, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 3, 7, 9, 64, 132, 8, 0, 12, ep="bias+relu+y_f32", lay=4, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 5, 7, 64, 64, 8, 0, -1, ep="ps+bias+relu", lay=2, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 3, 5, 32, 64, 8, 0, -1, ep="ps+bias+tail3", lay=3, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 5, 7, 64, 128, 8, 0, -1, ep="ps+relu+tail4", lay=4, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 3, 5, 32, 192, 8, 0, -1, ep="ps+bias+relu", plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 5, 7, 64, 192, 8, 0, -1, ep="ps+bias+tail3", lay=1, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 3, 5, 32, 64, 8, 0, -1, ep="ps+relu+tail4", lay=3, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 5, 7, 64, 64, 8, 0, -1, ep="ps+bias+relu", lay=4, conv1x1_gemm=1, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 3, 5, 32, 64, 8, 0, -1, ep="ps+bias+tail3", conv1x1_gemm=1, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 5, 7, 64, 128, 8, 0, -1, ep="ps+relu+tail4", lay=1, conv1x1_gemm=1, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 3, 5, 32, 192, 8, 0, -1, ep="ps+bias+relu", lay=2, conv1x1_gemm=1, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 5, 7, 64, 192, 8, 0, -1, ep="ps+bias+tail3", lay=4, conv1x1_gemm=1, plan_batch=4096),
    _mk(F32, FWD, 1, 1, 2, 3, 5, 32, 64, 8, 0, -1, ep="ps+relu+tail4", conv1x1_gemm=1, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 5, 7, 64, 64, 8, 0, -1, ep="ps+bias+relu", lay=1, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 3, 5, 32, 64, 8, 0, -1, ep="ps+bias+tail3", lay=2, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 5, 7, 64, 128, 8, 0, -1, ep="ps+relu+tail4", lay=3, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 3, 5, 32, 192, 8, 0, -1, ep="ps+bias+relu", plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 5, 7, 64, 192, 8, 0, -1, ep="ps+bias+tail3", lay=1, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 3, 5, 32, 64, 8, 0, -1, ep="ps+relu+tail4", lay=2, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 5, 7, 64, 64, 8, 0, -1, ep="ps+bias+relu", lay=3, conv1x1_gemm=1, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 3, 5, 32, 64, 8, 0, -1, ep="ps+bias+tail3", lay=4, conv1x1_gemm=1, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 5, 7, 64, 128, 8, 0, -1, ep="ps+relu+tail4", lay=1, conv1x1_gemm=1, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 3, 5, 32, 192, 8, 0, -1, ep="ps+bias+relu", lay=2, conv1x1_gemm=1, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 5, 7, 64, 192, 8, 0, -1, ep="ps+bias+tail3", lay=3, conv1x1_gemm=1, plan_batch=4096),
    _mk(BF16, FWD, 1, 1, 2, 3, 5, 32, 64, 8, 0, -1, ep="ps+relu+tail4", lay=4, conv1x1_gemm=1, plan_batch=4096),
    # ---- conv3x3_smallcin_kernel
    _mk(F32, FWD, 3, 1, 2, 9, 11, 1, 16, 10, 0, 16, ep="bias"),
    _mk(F32, FWD, 3, 2, 2, 17, 21, 1, 24, 10, 0, 16, lay=3),
    _mk(F32, FWD, 3, 1, 2, 9, 11, 1, 32, 10, 0, 16, ep="relu", lay=4),
    _mk(F32, FWD, 3, 2, 2, 17, 21, 3, 16, 10, 0, 16, ep="bias+relu"),
    _mk(F32, FWD, 3, 1, 2, 9, 11, 3, 24, 10, 0, 16, ep="bias", lay=1),
    _mk(F32, FWD, 3, 2, 2, 17, 21, 3, 32, 10, 0, 16, lay=2),
    _mk(F32, FWD, 3, 1, 2, 9, 11, 4, 16, 10, 0, 16, ep="relu", lay=4),
    _mk(F32, FWD, 3, 2, 2, 17, 21, 4, 24, 10, 0, 16, ep="bias+relu"),
    _mk(F32, FWD, 3, 1, 2, 9, 11, 4, 32, 10, 0, 16, ep="bias", lay=1),
    _mk(F32, FWD, 3, 2, 2, 17, 21, 8, 16, 10, 0, 16, lay=2),
    _mk(F32, FWD, 3, 1, 2, 9, 11, 8, 24, 10, 0, 16, ep="relu", lay=3),
    _mk(F32, FWD, 3, 2, 2, 17, 21, 8, 32, 10, 0, 16, ep="bias+relu"),
    _mk(F32, FWD, 3, 2, 1, 17, 15, 4, 32, 10, 0, 4, ep="bias+relu", lay=1),
    _mk(F32, FWD, 3, 1, 1, 17, 15, 3, 16, 10, 0, 16, ep="bias+relu", lay=2),
    _mk(F32, FWD, 3, 2, 1, 17, 15, 8, 24, 10, 0, 4, ep="bias+relu", lay=3),
    _mk(F32, FWD, 3, 1, 1, 17, 15, 1, 32, 10, 0, 16, ep="bias+relu", lay=4),
    _mk(BF16, FWD, 3, 2, 2, 17, 21, 1, 16, 10, 0, 16, ep="bias", lay=1, plan_batch=4096),
    _mk(BF16, FWD, 3, 1, 2, 9, 11, 1, 24, 10, 0, 16, lay=2, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 2, 17, 21, 1, 32, 10, 0, 16, ep="relu", lay=3, plan_batch=4096),
    _mk(BF16, FWD, 3, 1, 2, 9, 11, 3, 16, 10, 0, 16, ep="bias+relu", lay=4, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 2, 17, 21, 3, 24, 10, 0, 16, ep="bias", plan_batch=4096),
    _mk(BF16, FWD, 3, 1, 2, 9, 11, 3, 32, 10, 0, 16, lay=2, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 2, 17, 21, 4, 16, 10, 0, 16, ep="relu", lay=3, plan_batch=4096),
    _mk(BF16, FWD, 3, 1, 2, 9, 11, 4, 24, 10, 0, 16, ep="bias+relu", lay=4, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 2, 17, 21, 4, 32, 10, 0, 16, ep="bias", plan_batch=4096),
    _mk(BF16, FWD, 3, 1, 2, 9, 11, 8, 16, 10, 0, 16, lay=1, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 2, 17, 21, 8, 24, 10, 0, 16, ep="relu", lay=4, plan_batch=4096),
    _mk(BF16, FWD, 3, 1, 2, 9, 11, 8, 32, 10, 0, 16, ep="bias+relu", plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 1, 17, 15, 4, 32, 10, 0, 4, ep="bias+relu", lay=1, plan_batch=4096),
    _mk(BF16, FWD, 3, 1, 1, 17, 15, 3, 16, 10, 0, 16, ep="bias+relu", lay=2, plan_batch=4096),
    _mk(BF16, FWD, 3, 2, 1, 17, 15, 8, 24, 10, 0, 4, ep="bias+relu", lay=3, plan_batch=4096),
    _mk(BF16, FWD, 3, 1, 1, 17, 15, 1, 32, 10, 0, 16, ep="bias+relu", plan_batch=4096),
    # ---- per-image filters (wp_img_stride), three different images
    _mk(F32, FWD, 3, 1, 3, 9, 11, 36, 100, 80645, 0, 24, ep="bias+res+relu+wimg", lay=1),
    _mk(F32, FWD, 3, 1, 3, 17, 33, 36, 100, 321286, 0, 36, ep="bias+relu+wimg", lay=2, plan_batch=64),
    _mk(F32, FWD, 1, 1, 3, 7, 9, 264, 36, 6080645, 40824, 12, ep="bias+wimg", lay=3, conv1x1_gemm=-1),
    _mk(BF16, FWD, 3, 1, 3, 9, 11, 36, 100, 80645, 0, 24, ep="bias+res+relu+wimg", lay=4),
    _mk(BF16, FWD, 3, 1, 3, 17, 33, 36, 100, 321286, 0, 36, ep="bias+relu+wimg", lay=1, plan_batch=64),
    _mk(BF16, FWD, 1, 1, 3, 7, 9, 264, 36, 3080645, 20412, 12, ep="bias+wimg", lay=2, conv1x1_gemm=-1),
]


def case_id(i, c=None):
    c = CASES[i] if c is None else c
    tune = ",".join(f"{k}={v}" for k, v in c.tuning)
    rng = f"-ch{c.begin}+{c.count}" if c.count else ""
    ep = "+".join(c.ep)
    return (f"{i:03d}-{'+'.join(kernels(c))}-v{c.variant}-{c.dtype}-{c.kind}-k{c.ks}s{c.stride}-{c.N}x{c.H}x{c.W}-{c.Cin}to{c.Cout}{rng}-L{c.lay}"
            + (f"-{ep}" if ep else "") + (f"-ws_{c.ws}" if c.ws != "exact" else "") + (f"-{tune}" if tune else ""))


# ------------------------------------------------------------------------------------------------------------------------ operands

BIG = 4097.0                # 2^12 + 1: thirteen significant bits
MASK_VALUES = (2.0, -1.0, 0.0, -0.0, 0.5, -3.0, 1.0)
# how exact_inputs draws at level L (it starts at 0 and goes down until exact_bound holds):
# (max |small x|, chance of a large x or res value, max |w|, share of the weights kept, max |bias|, max |res|)
LEVELS = [(3, 1 / 16, 2, 1.0, 8, 3), (3, 1 / 64, 2, 1.0, 8, 3), (2, 0.0, 2, 1.0, 4, 2), (1, 0.0, 1, 1.0, 2, 1), (1, 0.0, 1, 0.5, 1, 1),
          (1, 0.0, 1, 0.25, 1, 1), (1, 0.0, 1, 0.125, 1, 1), (1, 0.0, 1, 1 / 16, 1, 0), (1, 0.0, 1, 1 / 32, 0, 0), (1, 0.0, 1, 1 / 64, 0, 0),
          (1, 0.0, 1, 1 / 256, 0, 0)]
LIMIT = float(2 ** 24)


def torch_dtype(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def weight_shape(c):
    """the fp32 master parameter of the conv the launch belongs to: [Cout, Cin, ks, ks] forward, and for an input gradient the FORWARD
    conv's, whose outputs are this launch's reduction: [c.Cin, c.Cout, ks, ks]; per-image filters: N of them"""
    shape = (c.Cin, c.Cout, c.ks, c.ks) if c.kind == "dgrad" else (c.Cout, c.Cin, c.ks, c.ks)
    return (c.N,) + shape if has(c, "wimg") else shape


def _shapes(c):
    IH, IW, OH, OW = dims(c)
    return (c.N, IH, IW, c.Cin), (c.N, OH, OW, c.Cout)


def _draw(c, g, level):
    xs, ys = _shapes(c)
    xmax, pbig, wmax, keep, bmax, rmax = LEVELS[level]
    if c.dtype == "bf16":           # every operand an integer of at most 256, weights at most 4
        big, wmax = 256.0, min(2 * wmax, 4)
        pbig *= 2
    else:
        big = BIG

    def ints(shape, m):
        return torch.randint(-m, m + 1, shape, generator=g).float() if m > 0 else torch.zeros(shape)

    def with_big(t, p):
        if p <= 0:
            return t
        sel = torch.rand(t.shape, generator=g) < p
        sign = torch.randint(0, 2, t.shape, generator=g).float() * 2 - 1
        return torch.where(sel, sign * big, t)

    x = with_big(ints(xs, xmax), pbig)
    w = ints(weight_shape(c), wmax)
    if keep < 1.0:
        w = w * (torch.rand(w.shape, generator=g) < keep)
    out = dict(x=x, w=w)
    if has(c, "bias"):
        out["bias"] = ints((c.Cout,), bmax)
    if has(c, "res"):
        out["res"] = with_big(ints(ys, rmax), pbig)
    if has(c, "mask"):
        out["mask"] = torch.tensor(MASK_VALUES)[torch.randint(0, len(MASK_VALUES), ys, generator=g)]
    if tail_channels(c):
        out["tail"] = ints((c.N, 2 * c.H, 2 * c.W, tail_channels(c)), 100)
    return out


def _conv(c, x, w):
    """the launch's convolution in the dtype of its operands: NHWC x -> NHWC [N, OH, OW, Cout]; image n with filter n under wimg"""
    xn = x.permute(0, 3, 1, 2)
    pad = (c.ks - 1) // 2

    def one(xi, wi):
        if c.kind == "dgrad":
            return torch.nn.grad.conv2d_input((xi.shape[0], c.Cout, c.H, c.W), wi, xi, stride=c.stride, padding=pad)
        return F.conv2d(xi, wi, None, stride=c.stride, padding=pad)
    y = torch.cat([one(xn[n:n + 1], w[n]) for n in range(c.N)]) if has(c, "wimg") else one(xn, w)
    return y.permute(0, 2, 3, 1).contiguous()


def exact_bound(c, ops_):
    """(the largest value conv(|x|, |w|) + |bias| + |res| takes at an output element, and for a case with column sums the largest per-channel
    sum over all pixels of that bound and of its square; else 0): the magnitudes no partial sum of the launch can exceed"""
    b = _conv(c, ops_["x"].double().abs(), ops_["w"].double().abs())
    if "bias" in ops_:
        b = b + ops_["bias"].double().abs()
    if "res" in ops_:
        b = b + ops_["res"].double().abs()
    sums = max(b.sum((0, 1, 2)).max().item(), (b * b).sum((0, 1, 2)).max().item()) if has(c, "colsum") else 0.0
    return b.max().item(), sums


def exact_inputs(c, seed):
    """{x | dy, w, bias, res, mask, tail}: integer-valued fp32 host tensors (NHWC; w: weight_shape), representable in the case's storage type,
    whose exact_bound is below 2^24.  `level` (returned under that key) says how far the magnitudes had to come down."""
    for level in range(len(LEVELS)):
        g = torch.Generator().manual_seed(1000003 * level + seed)
        ops_ = _draw(c, g, level)
        bound, sums = exact_bound(c, ops_)
        if bound < LIMIT and sums < LIMIT:
            ops_["level"] = level
            return ops_
    raise AssertionError(f"no exact operands for {c}: bound {bound}, column sums {sums}")


def gauss_inputs(c, seed):
    """normal operands as test_conv_fwd draws them (weights scaled by the reduction length); bf16 storage: rounded to bf16 first, as
    test_bf16_gpu does (the bias stays fp32)"""
    g = torch.Generator().manual_seed(seed)
    xs, ys = _shapes(c)
    rnd = (lambda t: t.to(torch.bfloat16).float()) if c.dtype == "bf16" else (lambda t: t)
    out = dict(x=rnd(torch.randn(xs, generator=g)), w=rnd(torch.randn(weight_shape(c), generator=g) / (c.Cin * c.ks * c.ks) ** 0.5))
    if has(c, "bias"):
        out["bias"] = torch.randn(c.Cout, generator=g)
    if has(c, "res"):
        out["res"] = rnd(torch.randn(ys, generator=g))
    if has(c, "mask"):
        out["mask"] = rnd(torch.randn(ys, generator=g))
    if tail_channels(c):
        out["tail"] = rnd(torch.randn((c.N, 2 * c.H, 2 * c.W, tail_channels(c)), generator=g))
    return out


def reference(c, ops_):
    """fp64, NHWC: forward y = mask > 0 ? relu?(conv + bias + res) : 0; dgrad (conv_transpose + res) * (mask > 0); pixel-shuffle
    PixelShuffle(2)(relu?(conv1x1 + bias)) as [N, 2H, 2W, nf].  All Cout channels: a channel-range launch produces a part of them."""
    y = _conv(c, ops_["x"].double(), ops_["w"].double())
    if "bias" in ops_:
        y = y + ops_["bias"].double()
    if "res" in ops_:
        y = y + ops_["res"].double()
    if has(c, "relu"):
        y = y.clamp_min(0.0)
    if "mask" in ops_:
        y = torch.where(ops_["mask"] > 0, y, torch.zeros_like(y))
    if has(c, "ps"):
        y = F.pixel_shuffle(y.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
    return y


def stored(c, ref):
    """the fp64 reference as the launch stores it: fp32, or rounded ONCE to bf16 (round to nearest even: the kernels store (__bf16)v)"""
    if y_vec(c) == 4:
        return ref.float().double()
    return ref.float().to(torch.bfloat16).double()


def canary(dtype):
    """a loud FINITE value in every channel and band that does not belong to an operand (the kernels may fetch a whole reduction chunk and
    meet the surplus with zero filter columns: a NaN there would test a contract the library does not make)"""
    import guard
    return torch.tensor(guard.CANARY[torch.float32]).to(dtype).item()


def device_slice(a, co, cs, dtype, device="cuda"):
    """(ops.TS, check): the NHWC host tensor `a` as channels co .. co + C of a guard-banded [N, H, W, cs] buffer.  The pad lanes
    C .. rup(C, vec) behind the slice are zero (the slice owns them); every other channel and both bands hold the canary."""
    import guard
    from unet_amd import ops
    N, H, W, C = a.shape
    v = ops.vec_of(dtype)
    assert co % v == 0 and cs % v == 0 and cs >= co + rup(C, v)
    buf, check = guard.guarded((N, H, W, cs), dtype, device, fill=canary(dtype))
    buf[..., co:co + C] = a.to(device=device, dtype=dtype)
    buf[..., co + C:co + rup(C, v)] = 0
    return ops.TS(buf, co, C), check
