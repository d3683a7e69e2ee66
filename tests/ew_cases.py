"""Elementwise, BatchNorm, pooling, shuffle and resize test cases (plain Python and torch on the CPU, no GPU): the table of
tests/test_ew_gpu.py, the builders of its operands and its fp64 reference.  What the table covers is asserted by tests/test_ew_cases_cpu.py.

  CASES            one stand-alone launch, or a forward / adjoint pair, of one ops.* entry point of csrc/elementwise.hip per case.
  layout(c)        {operand: (co, cs)} in CHANNELS: a slice starts at channel co of a buffer of cs channels.  bf16 cases need offsets that are
                   multiples of 8 (oct / vec forms) and offsets that are 4 mod 8 (quad / scalar forms), so device_slice takes no vector width.
  form(c)          the kernel form the launch must take, a restatement of the dispatch conditions of elementwise.hip (the library has no
                   query for it).  It assumes 16-byte aligned base addresses; the GPU test asserts them.
  walk(c)          plain arithmetic from the launch geometry (ew_grid, stats_rows, pick_tc): which loops the case drives.
  exact_inputs     integer or dyadic operands.  exact_bound adds the magnitudes of every term of every sum the launch forms and divides by the
                   smallest power of two all terms are multiples of: below 2^24, every intermediate and every partial sum in any order is exact
                   in fp32, so results are compared exactly; a bf16 output is the exact value rounded once.  The builder draws smaller and
                   sparser values until the bound holds.  fp32 storage: about one value in sixteen is +-(2^12 + 1), thirteen significant bits;
                   operands that the launch multiplies with each other (bn_stats' x * x, dot) take +-(2^6 + 1) instead, so that the PRODUCT
                   has thirteen.  bf16 storage: integers up to 256, so that sums such as 256 + 1 are exact ties of the output rounding.
  gauss_inputs     the generators of test_ops_gpu.py / test_bf16_gpu.py.
  reference        fp64, NHWC, from the definition of each op with torch's own functions, autograd for every adjoint.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

Case = namedtuple("Case", "op dtype N H W C lay opts to")
# op       the entry point (pairs: "maxpool" = maxpool + maxpool_bwd, "avgpool", "shuffle" = shuffle_blur + shuffle_blur_bwd, "resize")
# dtype    "f32" | "bf16": the storage type of the tensor operands (cast_slice: of its output; its input is fp32)
# H, W     the image of the launch's (forward) INPUT; shuffle: the low-resolution h x w
# C        channels; shuffle: Cu, the shuffled (output) channels, the input has 4 Cu
# lay      a key of LAYOUTS
# opts     a sorted tuple of names out of OPT_NAMES
# to       resize: the output side (H x W -> to x to)

OPT_NAMES = ("relu", "x2", "scale2", "out", "gout", "g_acc", "accumulate", "blur", "idx")

QUADWALK_OPS = ("affine_act", "bn_bwd_apply", "copy_slice", "relu_mask", "cast_slice")
REDUCTION_OPS = ("bn_stats", "bn_bwd_reduce", "colsum", "dot")
FORMED_OPS = ("affine_act", "bn_bwd_reduce", "bn_bwd_apply", "shuffle")
ARITHMETIC_OPS = ("affine_act", "bn_bwd_apply", "maxpool", "avgpool", "shuffle", "copy_slice", "cast_slice")   # bf16 outputs that are rounded

# (co, tail) of operand i out of n, in channels: the slice starts at channel co of a buffer of co + rup(C, 4) + tail channels
LAYOUTS = {
    "c": lambda i, n: (0, 0),                                                       # every operand contiguous
    "s8": lambda i, n: [(8, 8), (16, 8), (8, 16), (24, 8), (16, 16)][i],            # true slices, every offset and stride a multiple of 8
    "s4": lambda i, n: [(4, 4), (12, 4), (4, 12), (20, 4), (12, 12)][i],            # true slices, every offset 4 mod 8
    "mix": lambda i, n: (4, 4) if i == n - 1 else (8, 8),                           # only the last operand (an output) at 4 mod 8
    "cs4": lambda i, n: (8, 4),                                                     # offsets 8-aligned, channel strides 4 mod 8
}
SLICED = ("s8", "s4", "mix", "cs4")


def cdiv(a, b):
    return -(-a // b)


def rup(a, b):
    return cdiv(a, b) * b


def has(c, name):
    return name in c.opts


def torch_dtype(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def pool_hw(c):
    """output side of the pair's forward launch"""
    if c.op == "maxpool":
        return (c.H + 2 - 3) // 2 + 1, (c.W + 2 - 3) // 2 + 1
    if c.op == "avgpool":
        return (c.H + 1) // 2, (c.W + 1) // 2
    if c.op == "shuffle":
        return 2 * c.H, 2 * c.W
    if c.op == "resize":
        return c.to, c.to
    return c.H, c.W


def operands(c):
    """[(name, role, NHWC shape, torch dtype)] of the tensor operands in layout order; role "in" | "out" | "acc" (an output the launch adds to)"""
    dt = torch_dtype(c)
    s = (c.N, c.H, c.W, c.C)
    oh, ow = pool_hw(c)
    so = (c.N, oh, ow, c.C)
    acc = "acc" if has(c, "accumulate") else "out"
    op = c.op
    if op == "affine_act":
        r = [("x", "in", s)] + ([("x2", "in", s)] if has(c, "x2") else []) + [("y", "out", s)]
    elif op == "bn_stats" or op == "colsum":
        r = [("x", "in", s)]
    elif op == "bn_bwd_reduce":
        r = [("dout", "in", s)] + ([("out", "in", s)] if has(c, "out") else []) + [("x", "in", s)]
    elif op == "bn_bwd_apply":
        r = [("dout", "in", s)] + ([("out", "in", s)] if has(c, "out") else []) + [("x", "in", s), ("dx", "out", s)]
        if has(c, "gout"):
            r.append(("gout", "acc" if has(c, "g_acc") else "out", s))
    elif op == "maxpool":
        r = [("x", "in", s), ("y", "out", so)] + ([("dy", "in", so), ("dx", acc, s)] if has(c, "idx") else [])
    elif op in ("avgpool", "resize"):
        r = [("x", "in", s), ("y", "out", so), ("dy", "in", so), ("dx", acc, s)]
    elif op == "shuffle":
        s4 = (c.N, c.H, c.W, 4 * c.C)
        r = [("yc", "in", s4), ("X", "out", so), ("dX", "in", so), ("dyc", "out", s4)]
    elif op == "copy_slice":
        r = [("x", "in", s), ("y", acc, s)]
    elif op == "relu_mask":
        r = [("g", "in", s), ("ref", "in", s), ("y", "out", s)]
    elif op == "cast_slice":
        return [("x", "in", s, torch.float32), ("y", "out", s, torch.bfloat16)]
    elif op == "dot":
        r = [("x", "in", s), ("y", "in", s)]
    else:
        raise KeyError(op)
    return [t + (dt,) for t in r]


def layout(c):
    """{operand: (co, cs)} in channels"""
    ops_ = operands(c)
    out = {}
    for i, (name, _role, shape, _dt) in enumerate(ops_):
        co, tail = LAYOUTS[c.lay](i, len(ops_))
        out[name] = (co, co + rup(shape[3], 4) + tail)
    return out


# ------------------------------------------------------------------------------------------------------------------------ form, walk

def form(c):
    """the kernel form the launch takes: "quad" | "oct"; shuffle: "<forward>+<adjoint>" out of "scalar" | "vec".  Base addresses are taken
    to be 16-byte aligned and UNET_EW_OCT unset (elementwise.hip use_oct)."""
    lay = layout(c)
    bf = c.dtype == "bf16"

    def mult(names, v):
        return all(lay[n][0] % v == 0 and lay[n][1] % v == 0 for n in names if n in lay)
    if c.op == "affine_act":          # affine_act_impl: `use_oct() && C % 8 == 0 && x_cs % 8 == 0 && x_co % 8 == 0 && y_cs % 8 == 0 && ...`
        return "oct" if bf and c.C % 8 == 0 and mult(("x", "x2", "y"), 8) else "quad"
    if c.op == "bn_bwd_reduce":       # bn_bwd_reduce_impl: `use_oct() && C % 8 == 0 && d_cs % 8 == 0 && d_co % 8 == 0 && x_cs % 8 == 0 && ...`
        return "oct" if bf and c.C % 8 == 0 and mult(("dout", "out", "x"), 8) else "quad"
    if c.op == "bn_bwd_apply":        # bn_bwd_apply_impl: `use_oct() && C % 8 == 0 && d_cs % 8 == 0 && ... && dx_cs % 8 == 0 && dx_co % 8 == 0 && ...`
        return "oct" if bf and c.C % 8 == 0 and mult(("dout", "out", "x", "dx", "gout"), 8) else "quad"
    if c.op == "shuffle":
        v = 8 if bf else 4
        # shuffle_blur_impl: `!do_blur && Cu % V == 0 && X_cs % V == 0 && X_co % V == 0 && yc_cs % V == 0 && yc_co % V == 0 && aligned16(..)`
        fwd = "vec" if not has(c, "blur") and c.C % v == 0 and mult(("X", "yc"), v) else "scalar"
        # shuffle_blur_bwd_impl: `Cu % V == 0 && dX_cs % V == 0 && dX_co % V == 0 && yc_cs % V == 0 && ... && dyc_cs % V == 0 && dyc_co % V == 0 && ..`
        bwd = "vec" if c.C % v == 0 and mult(("dX", "yc", "dyc"), v) else "scalar"
        return f"{fwd}+{bwd}"
    return "quad"


GRID_CAP, BLOCK = 2048, 256            # common.h ew_grid: at most 2048 workgroups of 256 threads = 2^19 threads


def ew_grid(items):
    return max(1, min(GRID_CAP, cdiv(items, BLOCK)))


def stats_rows(P):                     # elementwise.hip stats_rows: one partial row per 32 pixels, at most 512
    return max(1, min(512, cdiv(P, 32)))


def pick_tc(cq):                       # elementwise.hip pick_tc: channel lanes of a workgroup, a power of two up to 64
    tc = 1
    while tc < cq and tc < 64:
        tc *= 2
    return tc


def _trips(p0, step, P, unroll):
    """(trips of the unrolled loop, trips of the tail loop) of the thread that starts at pixel p0"""
    p, u, t = p0, 0, 0
    while p + (unroll - 1) * step < P:
        p, u = p + unroll * step, u + 1
    while p < P:
        p, t = p + step, t + 1
    return u, t


def walk(c):
    """which loops the case drives.  QuadWalk ops: {cq, strides, carry}; reductions: {rows, cq, tc, passes, idle, unrolled, tail,
    last_block}: passes of the cbase loop, idle channel lanes of the last pass, most trips any thread makes through the unrolled and
    through the tail loop, and the channels of the last finalize workgroup (32 per workgroup)."""
    P = c.N * c.H * c.W
    octs = form(c) == "oct"
    cq = c.C // 8 if octs else cdiv(c.C, 4)
    if c.op in QUADWALK_OPS:
        items = P * cq
        threads = ew_grid(items) * BLOCK
        strides = items > threads
        return dict(cq=cq, strides=strides, carry=strides and threads % cq != 0)
    if c.op in REDUCTION_OPS:
        rows, tc = stats_rows(P), pick_tc(cq)
        py = BLOCK // tc
        step = rows * py
        unroll = 2 if octs else 4
        first, last = _trips(0, step, P, unroll), _trips(step - 1, step, P, unroll)
        passes = cdiv(cq, tc)
        return dict(rows=rows, cq=cq, tc=tc, passes=passes, idle=passes * tc - cq, unrolled=max(first[0], last[0]), tail=max(first[1], last[1]),
                    last_block=c.C - 32 * (cdiv(c.C, 32) - 1))
    return {}


# ------------------------------------------------------------------------------------------------------------------------ case table

def _mk(op, dtype, N, H, W, C, lay="c", opts="", to=None):
    o = tuple(sorted(e for e in opts.split("+") if e))
    assert all(e in OPT_NAMES for e in o), o
    assert lay in LAYOUTS
    return Case(op, dtype, N, H, W, C, lay, o, to)


F32, BF16 = "f32", "bf16"
CARRY = (2, 104, 104, 100)            # P = 21 632, Cq = 25: P Cq > 2^19 and 2^19 mod 25 != 0
CARRY8 = (2, 148, 148, 96)            # oct form: C8 = 12, P = 43 808
POW2 = (2, 130, 130, 64)              # Cq = 16, P = 33 800: threads stride, 2^19 mod 16 == 0
POW2_8 = (1, 129, 255, 128)           # oct form: C8 = 16, P = 32 895
SMALL = (2, 5, 7, 100)                # P Cq <= 2^19: no thread strides


def _table():
    t = []
    # ---- affine_act: QuadWalk in quad and oct form; relu, x2, scale2 on and off
    t += [_mk("affine_act", F32, *CARRY, opts="relu+x2+scale2"), _mk("affine_act", F32, *CARRY, lay="s4", opts="x2"),
          _mk("affine_act", F32, *POW2, lay="s8", opts="relu"), _mk("affine_act", F32, *SMALL, opts="relu+x2"),
          _mk("affine_act", F32, *SMALL, lay="s4", opts="x2+scale2"), _mk("affine_act", F32, 1, 3, 5, 8, lay="s8"),
          _mk("affine_act", BF16, *CARRY, lay="s4", opts="relu+x2+scale2"), _mk("affine_act", BF16, *CARRY, opts="x2"),
          _mk("affine_act", BF16, *CARRY8, opts="relu+x2+scale2"), _mk("affine_act", BF16, *CARRY8, lay="s8", opts="x2"),
          _mk("affine_act", BF16, *POW2_8, opts="relu+x2"), _mk("affine_act", BF16, *POW2, lay="s4", opts="relu"),
          _mk("affine_act", BF16, 2, 5, 7, 96, lay="s8", opts="relu+x2+scale2"), _mk("affine_act", BF16, 2, 5, 7, 96, lay="s4", opts="relu+x2+scale2"),
          _mk("affine_act", BF16, 2, 5, 7, 96, lay="mix", opts="x2+scale2"), _mk("affine_act", BF16, 2, 5, 7, 96, lay="cs4", opts="relu"),
          _mk("affine_act", BF16, 2, 5, 7, 96), _mk("affine_act", BF16, 2, 5, 7, 100, lay="s8", opts="x2")]
    # ---- bn_bwd_apply: out, gout, g_acc on and off
    t += [_mk("bn_bwd_apply", F32, *CARRY, opts="out+gout+g_acc"), _mk("bn_bwd_apply", F32, *CARRY, lay="s4", opts="out+gout"),
          _mk("bn_bwd_apply", F32, *POW2, lay="s8", opts="out"), _mk("bn_bwd_apply", F32, *SMALL, opts="gout+g_acc"),
          _mk("bn_bwd_apply", F32, *SMALL, lay="s8"), _mk("bn_bwd_apply", F32, 1, 3, 5, 8, lay="s4", opts="out+gout+g_acc"),
          _mk("bn_bwd_apply", BF16, *CARRY, lay="s4", opts="out+gout+g_acc"), _mk("bn_bwd_apply", BF16, *CARRY, opts="out"),
          _mk("bn_bwd_apply", BF16, *CARRY8, opts="out+gout+g_acc"), _mk("bn_bwd_apply", BF16, *CARRY8, lay="s8", opts="gout"),
          _mk("bn_bwd_apply", BF16, *POW2_8, opts="out+gout"), _mk("bn_bwd_apply", BF16, 2, 5, 7, 96, lay="s8", opts="out+gout+g_acc"),
          _mk("bn_bwd_apply", BF16, 2, 5, 7, 96, lay="s4", opts="out+gout+g_acc"), _mk("bn_bwd_apply", BF16, 2, 5, 7, 96, lay="mix", opts="out+gout"),
          _mk("bn_bwd_apply", BF16, 2, 5, 7, 96, lay="cs4"), _mk("bn_bwd_apply", BF16, 2, 5, 7, 96, opts="gout+g_acc"),
          _mk("bn_bwd_apply", BF16, 2, 5, 7, 96, lay="s8", opts="out")]
    # ---- copy_slice, relu_mask, cast_slice
    for dt in (F32, BF16):
        t += [_mk("copy_slice", dt, *CARRY, lay="s4" if dt == BF16 else "c"), _mk("copy_slice", dt, *CARRY, lay="s8", opts="accumulate"),
              _mk("copy_slice", dt, *POW2, opts="accumulate"), _mk("copy_slice", dt, *SMALL, lay="s4"),
              _mk("copy_slice", dt, 2, 5, 5, 20, lay="s8", opts="accumulate"), _mk("copy_slice", dt, 2, 5, 5, 20),
              _mk("relu_mask", dt, *CARRY, lay="s4" if dt == BF16 else "c"), _mk("relu_mask", dt, *POW2, lay="s8"),
              _mk("relu_mask", dt, *SMALL, lay="s4"), _mk("relu_mask", dt, 2, 5, 5, 20)]
    t += [_mk("cast_slice", BF16, *CARRY), _mk("cast_slice", BF16, *POW2, lay="s8"), _mk("cast_slice", BF16, *SMALL, lay="s4"),
          _mk("cast_slice", BF16, 1, 3, 5, 8, lay="s8")]
    # ---- reductions.  Every (op, dtype): C = 100 at P = 21 632 (rows 512: the four-trip loop plus its tail, TC = 32 with 7 idle lanes, a last
    # ---- finalize workgroup of 4 channels), C = 400 (two cbase passes), C = 36 at P = 50 / 20 / 900 (rows 2 / 1 / 29: TC = 16, 7 idle lanes),
    # ---- C = 64 (no idle lane)
    for op, dt in (("bn_stats", F32), ("bn_stats", BF16), ("bn_bwd_reduce", F32), ("bn_bwd_reduce", BF16), ("colsum", F32), ("dot", F32),
                   ("dot", BF16)):
        o = "out" if op == "bn_bwd_reduce" else ""
        quad = "s4" if (op, dt) == ("bn_bwd_reduce", BF16) else "c"          # (C = 400 is a multiple of 8: contiguous bf16 operands take the oct form)
        t += [_mk(op, dt, *CARRY, lay="s4", opts=o), _mk(op, dt, 1, 5, 10, 400, lay=quad), _mk(op, dt, 1, 5, 10, 36, lay="s8", opts=o),
              _mk(op, dt, 1, 4, 5, 36, lay="s4"), _mk(op, dt, 1, 30, 30, 36, opts=o), _mk(op, dt, 2, 8, 8, 64, lay="cs4")]
    # the oct form of bn_bwd_reduce (channel_reduce8): the two-pixel loop plus its tail; the tail alone; two full cbase passes; a second pass
    # with idle lanes; rows 1 and 29
    t += [_mk("bn_bwd_reduce", BF16, *CARRY8, opts="out"), _mk("bn_bwd_reduce", BF16, *CARRY8, lay="s8"),
          _mk("bn_bwd_reduce", BF16, 2, 12, 20, 64, opts="out"), _mk("bn_bwd_reduce", BF16, 1, 5, 10, 1024, opts="out"),
          _mk("bn_bwd_reduce", BF16, 1, 5, 10, 776, lay="s8", opts="out"), _mk("bn_bwd_reduce", BF16, 1, 4, 5, 64, lay="s8"),
          _mk("bn_bwd_reduce", BF16, 1, 30, 30, 96, opts="out"), _mk("bn_bwd_reduce", BF16, 2, 12, 20, 64, lay="s4", opts="out"),
          _mk("bn_bwd_reduce", BF16, 2, 12, 20, 64, lay="s8", opts="out")]
    # pad lanes (C = 3: TC = 1) and every row count at the `r + 24 < rows` boundary of rows_reduce2
    t += [_mk("colsum", F32, 1, 4, 5, 3, lay="s4"), _mk("colsum", F32, 2, 7, 9, 3), _mk("dot", F32, 1, 4, 5, 3), _mk("dot", F32, 2, 7, 9, 3, lay="s8"),
          _mk("dot", BF16, 2, 7, 9, 3, lay="s8")]
    t += [_mk("bn_stats", F32, 1, r, 32, 8, lay="s8" if r % 2 else "c") for r in range(25, 32)]
    # ---- max pool 3x3 / 2 (+ adjoint by index code): windows partly in the padding, 1-wide and 1-high images
    t += [_mk("maxpool", F32, 2, 7, 7, 8, opts="idx"), _mk("maxpool", F32, 1, 8, 8, 12, lay="s4", opts="idx+accumulate"),
          _mk("maxpool", F32, 2, 1, 5, 8, lay="s8", opts="idx"), _mk("maxpool", F32, 2, 5, 1, 8, opts="idx+accumulate"),
          _mk("maxpool", F32, 3, 2, 2, 4, lay="s4", opts="idx"), _mk("maxpool", F32, 2, 7, 7, 8, lay="s8"),
          _mk("maxpool", BF16, 2, 7, 7, 8, lay="s8", opts="idx+accumulate"), _mk("maxpool", BF16, 1, 8, 8, 12, lay="s4", opts="idx"),
          _mk("maxpool", BF16, 2, 1, 5, 8, opts="idx"), _mk("maxpool", BF16, 2, 5, 1, 8, lay="s4", opts="idx+accumulate"),
          _mk("maxpool", BF16, 3, 2, 2, 4, opts="idx"), _mk("maxpool", BF16, 2, 7, 7, 8)]
    # ---- average pool 2x2 ceil (+ adjoint): odd sides (divisors 1 and 2), 1 x 1
    for dt in (F32, BF16):
        t += [_mk("avgpool", dt, 2, 5, 7, 8), _mk("avgpool", dt, 2, 5, 7, 12, lay="s4", opts="accumulate"), _mk("avgpool", dt, 3, 1, 1, 8, lay="s8"),
              _mk("avgpool", dt, 2, 6, 6, 8, lay="s8", opts="accumulate"), _mk("avgpool", dt, 1, 6, 6, 4)]
    # ---- pixel shuffle with and without blur (+ adjoint): h = 1, w = 1; Cu 24 (vec in both types), 20 (vec fp32, scalar bf16), 6 (scalar)
    lays = ("c", "s8", "s4")
    k = 0
    for dt in (F32, BF16):
        for (h, w) in ((1, 6), (6, 1), (5, 7)):
            for cu in (24, 20, 6):
                for blur in ("", "blur"):
                    t.append(_mk("shuffle", dt, 2, h, w, cu, lay=lays[(k + k // 6) % 3], opts=blur))          # every Cu meets every layout
                    k += 1
    # ---- nearest resize (+ adjoint)
    for dt in (F32, BF16):
        t += [_mk("resize", dt, 2, 26, 26, 8, lay="s8", to=25), _mk("resize", dt, 1, 50, 50, 8, to=52), _mk("resize", dt, 2, 1, 1, 12, lay="s4", to=3)]
    return t


CASES = _table()


def case_id(i, c=None):
    c = CASES[i] if c is None else c
    o = "+".join(c.opts)
    return (f"{i:03d}-{c.op}-{c.dtype}-{form(c)}-{c.N}x{c.H}x{c.W}x{c.C}" + (f"-to{c.to}" if c.to else "") + f"-L{c.lay}" + (f"-{o}" if o else ""))


# ------------------------------------------------------------------------------------------------------------------------ operands

BIG = 4097.0                    # 2^12 + 1: thirteen significant bits
BIG_FACTOR = 65.0               # 2^6 + 1: its square has thirteen
MASK_VALUES = (2.0, -1.0, 0.0, -0.0, 0.5, -3.0, 1.0)
# how exact_inputs draws at level L (it starts at 0 and goes down until exact_bound holds): (max |small value|, chance of a large value)
LEVELS = [(3, 1 / 16), (3, 1 / 64), (2, 1 / 256), (1, 1 / 2048), (1, 0.0)]
LIMIT = float(2 ** 24)
MOMENTUM, EPS = 0.1, 1e-5


def _ints(g, shape, m, pbig=0.0, bigs=(BIG,)):
    t = torch.randint(-m, m + 1, shape, generator=g).float()
    if pbig > 0:
        sel = torch.rand(shape, generator=g) < pbig
        sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
        big = torch.tensor(bigs)[torch.randint(0, len(bigs), shape, generator=g)]
        t = torch.where(sel, sign * big, t)
    return t


def _pvec(g, C, ms, es, signed=True):
    """per-channel vector of small integers times powers of two"""
    m = torch.tensor(ms, dtype=torch.float32)[torch.randint(0, len(ms), (C,), generator=g)]
    e = torch.tensor(es, dtype=torch.float32)[torch.randint(0, len(es), (C,), generator=g)]
    sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1 if signed else 1.0
    return sign * m * torch.pow(2.0, e)


def _gate(g, shape):
    return torch.tensor(MASK_VALUES)[torch.randint(0, len(MASK_VALUES), shape, generator=g)]


def _shape(c, name):
    return next(s for n, _r, s, _d in operands(c) if n == name)


def _draw(c, g, level):
    m, pbig = LEVELS[level]
    bf = c.dtype == "bf16"
    bigs = (256.0,) if bf else (BIG,)
    factor = (256.0,) if bf else (BIG_FACTOR,)          # for operands the launch multiplies with each other
    if bf:
        pbig *= 2
    C, op = c.C, c.op
    s = (c.N, c.H, c.W, C)

    def data(shape=s, b=bigs):
        return _ints(g, shape, m, pbig, b)

    def target(name):                                    # what an accumulating launch finds in its output
        return _ints(g, _shape(c, name), 100)
    d = {}
    if op == "affine_act":
        d.update(x=data(), scale=_pvec(g, C, (1, 2, 3), (-1, 0, 1)), shift=_ints(g, (C,), 4) * 0.5)
        if has(c, "x2"):
            d["x2"] = data()
        if has(c, "scale2"):
            d.update(scale2=_pvec(g, C, (1, 2, 3), (-1, 0, 1)), shift2=_ints(g, (C,), 4) * 0.5)
    elif op == "bn_stats":
        d["x"] = data(b=factor)
    elif op == "colsum":
        d["x"] = data()
    elif op == "dot":
        d.update(x=data(b=factor), y=data(b=factor))
    elif op in ("bn_bwd_reduce", "bn_bwd_apply"):
        d.update(dout=data(), x=_ints(g, s, m) if op == "bn_bwd_reduce" else data(), mean=_ints(g, (C,), 2),
                 invstd=_pvec(g, C, (1,), (0, -1, -2), signed=False))
        if has(c, "out"):
            d["out"] = _gate(g, s)
        if op == "bn_bwd_apply":
            d.update(gamma=_pvec(g, C, (1, 2, 3), (-1, 0, 1)), c1=_ints(g, (C,), 4) * 0.5, c2=_pvec(g, C, (0, 1, 2, 3), (-1, 0)))
            if has(c, "g_acc"):
                d["gout0"] = target("gout")
    elif op == "maxpool":
        x = -1.0 - torch.randint(0, 9, s, generator=g).float()          # all negative, nine distinct values: the padding must not win, ties everywhere
        if not bf:
            x[c.N - 1, c.H - 1, c.W - 1, 1] = float("nan")
            x[0, :2, :2, 2] = float("-inf")                             # the whole window of output (0, 0)
        d["x"] = x
        if has(c, "idx"):
            d["dy"] = data(_shape(c, "dy"))
    elif op in ("avgpool", "resize"):
        d.update(x=data(), dy=data(_shape(c, "dy")))
    elif op == "shuffle":
        d.update(yc=data(_shape(c, "yc")).clamp_min(0.0), dX=data(_shape(c, "dX")))
    elif op == "copy_slice":
        d["x"] = data()
    elif op == "relu_mask":
        d.update(g=data(), ref=_gate(g, s))
    elif op == "cast_slice":
        d["x"] = _ints(g, s, m, 0.25, (BIG, 257.0, 259.0, 1027.0, 383.0))
    if op in ("maxpool", "avgpool", "copy_slice") and has(c, "accumulate"):
        name = "y" if op == "copy_slice" else "dx"
        d[name + "0"] = target(name)
    return d


def quantum(*ts):
    """the largest power of two that every finite non-zero element of every tensor is an integer multiple of (1.0 for none)"""
    q = float("inf")
    for t in ts:
        t = t.double().flatten()
        t = t[(t != 0) & t.isfinite()]
        if t.numel() == 0:
            continue
        mant, e = torch.frexp(t)
        mi = (mant.abs() * 2.0 ** 53).to(torch.int64)
        low = (mi & -mi).double()
        q = min(q, (low * torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 53).double())).min().item())
    return 1.0 if q == float("inf") else q


def _units(*terms, sums=False):
    """magnitudes of the terms of a sum, added up, in units of the terms' common quantum; sums: added over all pixels per channel too"""
    terms = [torch.where(t.double().isfinite(), t.double(), torch.zeros_like(t.double())) for t in terms]
    tot = sum(t.abs() for t in terms)
    if sums:
        tot = tot.sum((0, 1, 2))
    return tot.max().item() / quantum(*terms)


def exact_bound(c, d):
    """the largest magnitude, in units of the quantum of its terms, that any intermediate or partial sum of the launch(es) can reach"""
    d = {k: v.double() for k, v in d.items() if torch.is_tensor(v)}
    op = c.op
    z = torch.zeros(())
    if op == "affine_act":
        a = d["x"] * d["scale"]
        b = d["x2"] * d["scale2"] if has(c, "scale2") else d.get("x2", z)
        return _units(a, d["shift"].expand_as(a), b, d.get("shift2", z).expand_as(a))
    if op in ("bn_stats", "colsum"):
        return max(_units(d["x"], sums=True), _units(d["x"] * d["x"], sums=True) if op == "bn_stats" else 0.0)
    if op == "dot":
        p = d["x"] * d["y"]
        return p.abs().sum().item() / quantum(p)
    if op in ("bn_bwd_reduce", "bn_bwd_apply"):
        g = d["dout"]
        xc = _units(d["x"], d["mean"].expand_as(d["x"]))
        xh = (d["x"] - d["mean"]) * d["invstd"]
        if op == "bn_bwd_reduce":
            return max(xc, _units(g, sums=True), _units(g * xh, sums=True))
        k = d["gamma"] * d["invstd"]
        terms = (g, d["c1"].expand_as(g), xh * d["c2"])
        b = max(xc, _units(xh), _units(*terms), _units(*(k * t for t in terms)))
        return max(b, _units(g, d["gout0"])) if has(c, "g_acc") else b
    if op == "maxpool":
        return 4 * _units(d["dy"]) + _units(d.get("dx0", z)) if has(c, "idx") else 1.0
    if op == "avgpool":                                  # forward: four values, then x 1/4; adjoint: dy x 1/4 (+ the target)
        return max(16 * _units(d["x"]), 4 * _units(d["dy"]) + 4 * _units(d.get("dx0", z)))
    if op == "shuffle":                                  # forward blur: four values x 1/4; adjoint: weights 4 + 2 + 2 + 1, x 1/4
        return max(16 * _units(d["yc"]), 36 * _units(d["dX"]))
    if op == "resize":                                   # adjoint: at most (ceil(to / H) + 1)^2 values land on one input pixel
        return (cdiv(c.to, c.H) + 1) ** 2 * _units(d["dy"])
    if op == "copy_slice":
        return _units(d["x"], d.get("y0", z).expand_as(d["x"]))
    return _units(*(v for v in d.values()))


def exact_inputs(c, seed):
    """host tensors (fp32 values representable in the case's storage type; NHWC, per-channel vectors [C]) whose exact_bound is below 2^24;
    `level` says how far the magnitudes had to come down"""
    for level in range(len(LEVELS)):
        g = torch.Generator().manual_seed(1000003 * level + seed)
        d = _draw(c, g, level)
        bound = exact_bound(c, d)
        if bound < LIMIT:
            d["level"] = level
            return d
    raise AssertionError(f"no exact operands for {c}: bound {bound}")


def gauss_inputs(c, seed):
    """normal operands as test_batchnorm_train_fwd_bwd, test_maxpool, test_avgpool_ceil, test_shuffle_blur, test_resize_nearest,
    test_layout_and_slices and test_elementwise_twins_bf16 draw them; bf16 storage: rounded to bf16 first (per-channel vectors stay fp32)"""
    g = torch.Generator().manual_seed(seed)
    bf = c.dtype == "bf16" and c.op != "cast_slice"
    rnd = (lambda t: t.to(torch.bfloat16).float()) if bf else (lambda t: t)
    C, op = c.C, c.op
    s = (c.N, c.H, c.W, C)

    def randn(shape=s):
        return rnd(torch.randn(shape, generator=g))
    d = {}
    if op == "affine_act":
        d.update(x=rnd(torch.randn(s, generator=g) * 2 + 0.5), scale=torch.rand(C, generator=g) + 0.5, shift=torch.randn(C, generator=g))
        if has(c, "x2"):
            d["x2"] = randn()
        if has(c, "scale2"):
            d.update(scale2=torch.rand(C, generator=g) + 0.5, shift2=torch.randn(C, generator=g))
    elif op in ("bn_stats", "colsum", "dot"):
        d["x"] = rnd(torch.randn(s, generator=g) * 2 + 0.5)
        if op == "dot":
            d["y"] = d["x"].clone()                      # sum of squares: the statistic bn_stats forms, at its tolerance
    elif op in ("bn_bwd_reduce", "bn_bwd_apply"):
        x = rnd(torch.randn(s, generator=g) * 2 + 0.5)
        d.update(dout=randn(), x=x, mean=x.mean((0, 1, 2)), invstd=1.0 / (x.var((0, 1, 2), unbiased=False) + 1e-5).sqrt())
        if has(c, "out"):
            d["out"] = randn()
        if op == "bn_bwd_apply":
            d.update(gamma=torch.rand(C, generator=g) + 0.5, c1=torch.randn(C, generator=g) * 0.1, c2=torch.randn(C, generator=g) * 0.1)
            if has(c, "g_acc"):
                d["gout0"] = randn()
    elif op == "maxpool":
        d["x"] = rnd(torch.relu(torch.randn(s, generator=g)))
        if has(c, "idx"):
            d["dy"] = randn(_shape(c, "dy"))
    elif op in ("avgpool", "resize"):
        d.update(x=randn(), dy=randn(_shape(c, "dy")))
    elif op == "shuffle":
        d.update(yc=rnd(torch.relu(torch.randn(_shape(c, "yc"), generator=g))), dX=randn(_shape(c, "dX")))
    elif op in ("copy_slice", "cast_slice"):
        d["x"] = randn()
    elif op == "relu_mask":
        d.update(g=randn(), ref=randn())
    if op in ("maxpool", "avgpool", "copy_slice") and has(c, "accumulate"):
        name = "y" if op == "copy_slice" else "dx"
        d[name + "0"] = randn(_shape(c, name))
    return d


# ------------------------------------------------------------------------------------------------------------------------ reference

def _n(t):
    return t.permute(0, 3, 1, 2)


def _h(t):
    return t.permute(0, 2, 3, 1).contiguous()


def maxpool_codes(ind, W):
    """torch's flat input index of every window's winner (NCHW, return_indices=True) -> the library's code 3 r + s inside the 3 x 3 window
    whose first tap is input (2 oy - 1, 2 ox - 1)"""
    OH, OW = ind.shape[2:]
    oy = torch.arange(OH).view(1, 1, OH, 1)
    ox = torch.arange(OW).view(1, 1, 1, OW)
    r = ind // W - (2 * oy - 1)
    s_ = ind % W - (2 * ox - 1)
    return (3 * r + s_).to(torch.uint8)


def scatter_by_code(dy, code, H, W):
    """NCHW: every dy[n, c, oy, ox] added to the input pixel its window's code names"""
    N, C, OH, OW = dy.shape
    oy = torch.arange(OH).view(1, 1, OH, 1)
    ox = torch.arange(OW).view(1, 1, 1, OW)
    iy = 2 * oy - 1 + code.long() // 3
    ix = 2 * ox - 1 + code.long() % 3
    dx = torch.zeros(N, C, H * W, dtype=dy.dtype)
    dx.scatter_add_(2, (iy * W + ix).reshape(N, C, -1), dy.reshape(N, C, -1))
    return dx.view(N, C, H, W)


def _adjoint(fn, x, dy):
    """autograd: the gradient of <fn(x), dy> with respect to x"""
    x = x.clone().requires_grad_(True)
    fn(x).backward(dy)
    return x.grad


def _shuffle_fwd(blur):
    def fn(yc_nchw):
        up = F.pixel_shuffle(yc_nchw, 2)
        return F.avg_pool2d(F.pad(up, (1, 0, 1, 0), mode="replicate"), 2, stride=1) if blur else up
    return fn


def bn_finalize_ref(s, q, count, gamma, beta, rmean, rvar, momentum=MOMENTUM, eps=EPS):
    """fp64 BatchNorm2d training statistics from per-channel sums: dict(mean, var, invstd, scale, shift, running_mean, running_var);
    momentum and eps are the fp32 values the C ABI receives"""
    m = torch.tensor(momentum, dtype=torch.float32).double().item()
    e = torch.tensor(eps, dtype=torch.float32).double().item()
    s, q, gamma, beta, rmean, rvar = (t.double() for t in (s, q, gamma, beta, rmean, rvar))
    mean = s / count
    var = (q / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / (var + e).sqrt()
    scale = gamma * invstd
    unbiased = var * count / (count - 1.0) if count > 1 else var
    return dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=beta - mean * scale, running_mean=(1.0 - m) * rmean + m * mean,
                running_var=(1.0 - m) * rvar + m * unbiased, unbiased=unbiased, m=m)


def reference(c, inp):
    """{output: fp64 tensor}: NHWC tensors under the names of operands(c); reductions: per-channel `sum0` (and `sum1`), dot also `total`;
    maxpool: `idx`, the uint8 index codes (NHWC).  An accumulating output includes what the launch found there (`<name>0`)."""
    d = {k: (v.double() if torch.is_tensor(v) else v) for k, v in inp.items()}
    op = c.op
    if op == "affine_act":
        y = d["x"] * d["scale"] + d["shift"]
        if has(c, "x2"):
            y = y + (d["x2"] * d["scale2"] + d["shift2"] if has(c, "scale2") else d["x2"])
        return dict(y=y.clamp_min(0.0) if has(c, "relu") else y)
    if op == "bn_stats":
        return dict(sum0=d["x"].sum((0, 1, 2)), sum1=(d["x"] * d["x"]).sum((0, 1, 2)))
    if op == "colsum":
        return dict(sum0=d["x"].sum((0, 1, 2)))
    if op == "dot":
        p = d["x"] * d["y"]
        return dict(sum0=p.sum((0, 1, 2)), total=p.sum())
    if op in ("bn_bwd_reduce", "bn_bwd_apply"):
        g = torch.where(d["out"] > 0, d["dout"], torch.zeros_like(d["dout"])) if has(c, "out") else d["dout"]      # the gate: the STORED activation
        xh = (d["x"] - d["mean"]) * d["invstd"]
        if op == "bn_bwd_reduce":
            return dict(sum0=g.sum((0, 1, 2)), sum1=(g * xh).sum((0, 1, 2)))
        out = dict(dx=d["gamma"] * d["invstd"] * (g - d["c1"] - xh * d["c2"]))
        if has(c, "gout"):
            out["gout"] = g + d["gout0"] if has(c, "g_acc") else g
        return out
    if op == "maxpool":
        x = _n(d["x"])
        y, ind = F.max_pool2d(x, 3, 2, 1, return_indices=True)
        out = dict(y=_h(y), idx=_h(maxpool_codes(ind, c.W)))
        if has(c, "idx"):
            out["dx"] = _h(_adjoint(lambda t: F.max_pool2d(t, 3, 2, 1), x, _n(d["dy"]))) + d.get("dx0", 0.0)
        return out
    if op in ("avgpool", "resize"):
        fn = (lambda t: F.avg_pool2d(t, 2, ceil_mode=True)) if op == "avgpool" else (lambda t: F.interpolate(t, (c.to, c.to), mode="nearest"))
        x = _n(d["x"])
        return dict(y=_h(fn(x)), dx=_h(_adjoint(fn, x, _n(d["dy"]))) + d.get("dx0", 0.0))
    if op == "shuffle":
        fn = _shuffle_fwd(has(c, "blur"))
        yc = _n(d["yc"])
        dyc = _adjoint(fn, yc, _n(d["dX"]))
        return dict(X=_h(fn(yc)), dyc=_h(torch.where(yc > 0, dyc, torch.zeros_like(dyc))))
    if op == "copy_slice":
        return dict(y=d["x"] + d.get("y0", 0.0))
    if op == "relu_mask":
        return dict(y=torch.where(d["ref"] > 0, d["g"], torch.zeros_like(d["g"])))
    if op == "cast_slice":
        return dict(y=d["x"])
    raise KeyError(op)


def stored(dt, ref):
    """the fp64 reference as a launch stores it: fp32, or rounded ONCE to bf16 (round to nearest even)"""
    return ref.float().double() if dt == torch.float32 else ref.float().to(torch.bfloat16).double()


def canary(dtype):
    """a loud FINITE value in every channel and band that does not belong to an operand (after conv_cases.canary)"""
    import guard
    return torch.tensor(guard.CANARY[torch.float32]).to(dtype).item()


def _guarded(shape, dtype, fill, device):
    """guard.guarded with bands of a whole number of 64 elements: the tensor's base address keeps the allocation's 16-byte alignment"""
    import guard
    return guard.guarded(shape, dtype, device, fill=fill, guard=rup(guard.default_guard(shape, dtype), 64))


def _raw_ts():
    from unet_amd import ops

    class RawTS(ops.TS):
        """ops.TS without its vector-width assertion: the C ABI takes bf16 slices at any multiple of 4 channels (common.h slice_ok)"""

        def __post_init__(self):
            assert self.buf.is_contiguous() and self.buf.dim() == 4 and self.co + self.C <= self.cs
    return RawTS


def device_slice(a, co, cs, dtype, device="cuda", quantum_=4):
    """(TS, check): the NHWC host tensor `a` as channels co .. co + C of a guard-banded [N, H, W, cs] buffer.  The pad lanes C .. rup(C, quantum_)
    behind the slice are zero (the slice owns them); every other channel and both bands hold the canary."""
    N, H, W, C = a.shape
    assert co % quantum_ == 0 and cs % quantum_ == 0 and cs >= co + rup(C, quantum_)
    buf, check = _guarded((N, H, W, cs), dtype, canary(dtype), device)
    buf[..., co:co + C] = a.to(device=device, dtype=dtype)
    buf[..., co + C:co + rup(C, quantum_)] = 0
    return _raw_ts()(buf, co, C), check


def output_slice(shape, co, cs, dtype, device="cuda", init=None):
    """(TS, check): an output slice of a guard-banded buffer that is NaN everywhere -- bands, neighbouring channels and the slice itself, unless
    `init` (what an accumulating launch finds there) is given"""
    N, H, W, C = shape
    assert co % 4 == 0 and cs % 4 == 0 and cs >= co + C
    buf, check = _guarded((N, H, W, cs), dtype, float("nan"), device)
    if init is not None:
        buf[..., co:co + C] = init.to(device=device, dtype=dtype)
    return _raw_ts()(buf, co, C), check
