"""Weight-gradient test cases (plain Python, no GPU): a restatement of the planner of unet_amd/csrc/conv_wgrad.hip (make_wplan and the
launch ladder of unet_conv2d_wgrad), the case table of tests/test_wgrad_gpu.py and the builders of its operands.

  plan(case)       which kernel family a case runs on, its pixel splits, partial images per workgroup, reduce kernel and grid height.
                   Nothing in the library reports this: tests/test_wgrad_cases_cpu.py keeps the mirror honest through the one number
                   the library does report, unet_conv2d_wgrad_workspace = splits * nsub * T * Cout * Cin + splits * Cout (a drifted
                   threshold changes the column count, hence the splits, hence that number), and asserts that CASES reaches every
                   family instantiation, reduce kernel and plan edge.
  exact_inputs     integer-valued operands: every product and every partial sum is an integer below 2^24, exact in fp32 in ANY
                   summation order, so the kernels are compared with torch.equal.  fp32 storage draws x in [-511, 511] and dy in
                   [-2, 2] (ten significant bits: a kernel that multiplies at bf16 precision fails), bf16 storage x in [-15, 15] and
                   dy in [-3, 3].
  gauss_inputs     the generators of test_conv_wgrad / test_conv_forward_dgrad_wgrad_bf16, compared at those tests' tolerances.
  device_slice     an operand as training passes it: a channel slice (co, C) of a wider buffer, pad lanes C .. rup(C, vec) zero, every
                   other channel and both guard bands of the allocation (tests/guard.py) a loud canary.
"""
from collections import namedtuple

import torch

# ------------------------------------------------------------------------------------------------------------------------ cases

Case = namedtuple("Case", "N H W Cin Cout ks stride dtype layout tuning")
# layout = (x_co, x_tail, dy_co, dy_tail) in units of one 16-byte channel vector (4 fp32 / 8 bf16 channels): the slice starts at
# channel co * vec of a buffer of co * vec + rup(C, vec) + tail * vec channels (tail >= 1: there is always a neighbour behind the pad lanes)
LAYOUTS = [(0, 1, 0, 1), (1, 1, 2, 1), (3, 2, 0, 3), (0, 2, 1, 1), (2, 1, 1, 2)]

# the wgrad switches of unet_tuning as unet_tuning_default() sets them
DEFAULTS = dict(wgrad_mfma_shape=32, wgrad_bf16_k4=1, wgrad_1x1=1, wgrad_narrow=1, wgrad_wgs=0)

PREFILL = 5.0               # what dw holds before the accumulate launch
EXACT_RANGE = {"f32": (511, 2), "bf16": (15, 3)}        # max |x|, max |dy|


def cdiv(a, b):
    return -(-a // b)


def rup(a, b):
    return cdiv(a, b) * b


def vec_of(dtype):
    return 8 if dtype == "bf16" else 4


def out_hw(c):
    pad = (c.ks - 1) // 2
    return (c.H + 2 * pad - c.ks) // c.stride + 1, (c.W + 2 * pad - c.ks) // c.stride + 1


def pixels(c):
    OH, OW = out_hw(c)
    return c.N * OH * OW


def strides(c):
    """(x_co, x_cs, dy_co, dy_cs) in channels"""
    v = vec_of(c.dtype)
    xo, xt, do, dt = c.layout
    return xo * v, xo * v + rup(c.Cin, v) + xt * v, do * v, do * v + rup(c.Cout, v) + dt * v


# ------------------------------------------------------------------------------------------------------------------------ planner mirror

def plan(c, tuning=None):
    """{family, ptw, splits, nsub, reduce, grid_y} of a case (+ what the coverage test looks at), under c.tuning or `tuning`"""
    t = dict(DEFAULTS)
    t.update(c.tuning if tuning is None else tuning)
    N, Cin, Cout, ks, stride = c.N, c.Cin, c.Cout, c.ks, c.stride
    bf16 = c.dtype == "bf16"
    vec = vec_of(c.dtype)
    OH, OW = out_hw(c)
    P = N * OH * OW
    Cin4 = rup(Cin, vec)
    T = ks * ks
    x_co, x_cs, dy_co, dy_cs = strides(c)
    out = dict(T=T, P=P, nsub=1)

    ptw = 32 if OW >= 32 else (16 if OW >= 16 else 8)
    pt = (128 if stride == 1 else 32) if bf16 else (64 if stride == 1 else 32)
    pth = pt // ptw
    tiles_y, tiles_x = cdiv(OH, pth), cdiv(OW, ptw)
    total = N * tiles_y * tiles_x
    cols = cdiv(Cout, 64) * cdiv(Cin, 64)
    narrow = (not bf16) and t["wgrad_narrow"] != 0 and ks == 3 and stride == 1 and 80 < Cout <= 112 and OW >= 32
    if narrow:
        ptw = 32
        tiles_y, tiles_x = OH, cdiv(OW, 32)
        total = N * tiles_y * tiles_x
        nch = cdiv(Cin, 112)
        cw = rup(cdiv(Cin, nch), 4)
        ntw = 5 if Cout > 96 else 7
        nnb = cdiv(cdiv(9 * cw, 16), 4 * ntw)
        cols = nch * nnb
        out.update(cw=cw, chunks=cdiv(Cin, cw), last_chunk=Cin - (cdiv(Cin, cw) - 1) * cw)

    if (not bf16) and ks == 1 and Cout <= 16 and Cin4 <= 512 and t["wgrad_1x1"] != 0:
        ps = 256 // (Cin4 // 4)
        kk = 4 * cdiv(Cout, 4)
        cap = 65536 // ((kk * Cin4 + kk) * 4)
        capped = ps >= cap                     # the pixel lanes fill the 64 KiB of LDS (or would overflow them)
        ps = max(1, min(ps, cap))
        blocks = max(1, min(1024, P // (ps * 64)))
        ppb = cdiv(P, blocks)
        splits = cdiv(P, ppb)
        out.update(family=f"small1x1<{kk // 4}>", ptw=ptw, splits=splits, reduce="rows", grid_y=splits, slices=splits, ps=ps, ppb=ppb,
                   lds_capped=capped, total_tiles=total, tpb=0)
        return out

    gemm = (not bf16) and ks == 1 and t["wgrad_1x1"] != 0
    if gemm and t["wgrad_1x1"] != 2 and (Cin <= 64 or Cout <= 64 or 2.0 * P * Cin * Cout < 3.0e9):
        gemm = False
    if gemm:
        total = cdiv(P, 64)
        cols = cdiv(Cout, 128) * cdiv(Cin, 128)

    if t["wgrad_wgs"] > 0:
        target = t["wgrad_wgs"]
    elif bf16 and ks == 3 and stride == 1 and total * cols <= 20000:
        target = 256
    else:
        target = 512
    want = target // cols
    if (narrow or bf16) and want >= 8:
        want &= ~7
    want = max(want, 1)
    tpb = min(max(cdiv(total, want), 4), total)
    splits = cdiv(total, tpb)
    nsub = 1
    if (not bf16) and (not narrow) and (not gemm) and t["wgrad_mfma_shape"] == 32 and t["wgrad_narrow"] != 3:
        nsub = (2 if Cin <= 32 else 1) * (2 if Cout <= 32 else 1)

    grid_y = splits
    if bf16:
        k4 = (ptw == 32 and stride == 1 and t["wgrad_bf16_k4"] != 0 and c.H * c.W * x_cs * 2 < (1 << 31) - 65536
              and OH * OW * dy_cs * 2 < (1 << 31) - 65536)
        if k4:
            tl = cdiv(Cout, 16)
            kv = tl if tl <= 2 else (3 if rup(tl, 3) < rup(tl, 4) else 4)
            family = f"bf16_k4<{kv},{ks}>"
        else:
            family = f"bf16<{ptw},{stride},{ks}>"
        if splits >= 8:
            grid_y = rup(splits, 8)
    elif gemm:
        family = "gemm1x1"
    elif narrow:
        if 96 < Cout <= 100 and t["wgrad_narrow"] != 2:
            family = "flat<6,5,sliver>"
        elif Cout > 96:
            family = "flat<7,5>"
        else:
            family = "flat<6,7>"
        grid_y = rup(splits, 8)
    else:
        family = f"{'wgrad16' if t['wgrad_mfma_shape'] == 16 else 'wgrad'}<{ptw},{stride},{ks}>"

    slices = splits * nsub
    small_image = Cout * Cin * T < (1 << 31) // 8
    reduce = "q8" if slices >= 32 and small_image else ("q4" if slices >= 8 and small_image else "plain")
    out.update(family=family, ptw=ptw, splits=splits, nsub=nsub, reduce=reduce, grid_y=grid_y, slices=slices, total_tiles=total, tpb=tpb,
               pth=pth)
    return out


def workspace_floats(c, p):
    """what unet_conv2d_wgrad_workspace reports for plan p: the partial filter images and the partial bias rows"""
    return p["splits"] * p["nsub"] * p["T"] * c.Cout * c.Cin + p["splits"] * c.Cout


# ------------------------------------------------------------------------------------------------------------------------ case table

def _build_cases():
    cases = []

    def add(N, H, W, Cin, Cout, ks, stride, dtype="f32", **tuning):
        i = len(cases)                  # (the layouts rotate, with a shift every 5 and 25 cases so that no family's stride misses one)
        cases.append(Case(N, H, W, Cin, Cout, ks, stride, dtype, LAYOUTS[(i + i // 5 + i // 25) % len(LAYOUTS)], tuple(sorted(tuning.items()))))

    # ---- the nine (PTW, S, KS) forms of wgrad_kernel, wgrad16_kernel and wgrad_bf16_kernel on ragged tiles: output widths 7 / 19 / 37 for
    # PTW 8 / 16 / 32, heights below the tile height or one row into the second tile row, odd (and one even) extents at stride 2.
    # Channel pairs on both sides of the 64-wide block and its 32-wide halves: nsub = 4, 2, 2, 1, 1 on wgrad_kernel.
    pairs = [(3, 32), (32, 100), (100, 32), (65, 63), (100, 100)]
    forms = [  # (N, H, W, ks, stride)
        (2, 5, 7, 3, 1), (2, 6, 19, 3, 1), (2, 3, 37, 3, 1),           # fp32 tile heights 8 / 4 / 2, bf16 16 / 8 / 4
        (2, 9, 7, 1, 1), (3, 5, 19, 1, 1), (2, 5, 37, 1, 1),
        (2, 9, 13, 3, 2), (2, 5, 37, 3, 2), (2, 4, 74, 3, 2),          # OH x OW = 5 x 7, 3 x 19, 2 x 37: tile heights 4 / 2 / 1
    ]
    for fi, (N, H, W, ks, stride) in enumerate(forms):
        for pi, (Cin, Cout) in enumerate(pairs):
            add(N, H, W, Cin, Cout, ks, stride, "f32", wgrad_narrow=0)
            add(N, H, W, Cin, Cout, ks, stride, "bf16", wgrad_bf16_k4=0)
            if (fi + pi) % 2 == 0:
                add(N, H, W, Cin, Cout, ks, stride, "f32", wgrad_mfma_shape=16, wgrad_narrow=0)

    # ---- wgrad_flat_kernel: images of 1 / 2 / 3 / 5 rows (its halo is a ring of three), widths 32 / 33 / 40 / 64, every output-tile form,
    # one / two / three input-channel chunks with a short last chunk (113 = 60 + 53, 230 = 80 + 80 + 70); at least 4 tiles per block and at most
    # 5 rows per strip, so every block's tile range crosses a column strip, and with several blocks an image
    for N, H, W, Cin, Cout, tune in [
        (2, 1, 32, 9, 81, {}),                                  # two tiles in all: one block, one split
        (3, 2, 33, 36, 96, dict(wgrad_wgs=12)),
        (2, 3, 40, 112, 97, dict(wgrad_wgs=64)),
        (2, 5, 64, 113, 100, dict(wgrad_wgs=128)),
        (2, 2, 64, 230, 100, dict(wgrad_narrow=2)),
        (2, 3, 33, 230, 101, dict(wgrad_wgs=96)),
        (3, 5, 40, 36, 112, dict(wgrad_wgs=21)),
        (5, 1, 64, 113, 96, {}),
        (2, 5, 32, 230, 81, {}),
        (2, 3, 32, 9, 100, {}),
        (3, 2, 33, 112, 112, dict(wgrad_wgs=40)),
        (6, 3, 64, 36, 100, {}),                                # 36 tiles, 4 a block: 9 splits on a grid padded to 16 rows of blocks
        (4, 5, 33, 9, 96, dict(wgrad_wgs=7)),                   # 7 splits on a grid of 8
        (4, 3, 40, 36, 101, dict(wgrad_wgs=24)),                # 6 splits of one strip and a third each
    ]:
        add(N, H, W, Cin, Cout, 3, 1, "f32", **tune)

    # ---- wgrad1x1_kernel (forced: wgrad_1x1 = 2): pixel counts that are no multiple of its flat 64-pixel tile, channel counts around 128
    for N, H, W, Cin, Cout in [(3, 5, 7, 127, 129), (3, 5, 7, 129, 127), (3, 5, 7, 130, 70), (3, 5, 7, 70, 130), (5, 9, 11, 129, 130),
                               (1, 3, 9, 127, 130)]:
        add(N, H, W, Cin, Cout, 1, 1, "f32", wgrad_1x1=2)

    # ---- wgrad1x1_small_kernel<1..4>: 3 input channels (256 pixel lanes, 204 at its LDS cap), 100 (10 lanes, 6 idle threads), 512 (2 lanes,
    # 1 at the cap); fewer pixels than one block's ps * 64 and pixel counts that leave a remainder; 516 input channels leave the family
    for N, H, W, Cin, Cout in [
        (2, 9, 11, 3, 1), (2, 31, 34, 100, 4), (1, 15, 7, 512, 5), (3, 5, 7, 3, 8), (1, 9, 11, 100, 9), (3, 9, 11, 512, 12),
        (2, 33, 37, 3, 13), (2, 31, 33, 100, 16), (1, 25, 8, 512, 16), (3, 70, 71, 3, 16), (1, 17, 19, 512, 1), (2, 5, 7, 100, 13),
        (1, 15, 7, 516, 5), (3, 5, 7, 516, 16),
    ]:
        add(N, H, W, Cin, Cout, 1, 1, "f32")

    # ---- wgrad_bf16_k4_kernel<KV, KS>: 16 / 24 / 40 / 64 / 80 / 100 / 112 output channels run on KV = 1 / 2 / 3 / 4 / 3 / 4 / 4 tiles a block
    geo = [(2, 5, 37), (2, 3, 64), (1, 9, 32), (3, 2, 33)]
    cins = [8, 36, 100, 104]
    i = 0
    for Cout in (16, 24, 40, 64, 80, 100, 112):
        for ks in (1, 3):
            N, H, W = geo[i % 4]
            add(N, H, W, cins[i % 4], Cout, ks, 1, "bf16")
            i += 1

    # ---- split counts 1 / 7 / 8 / 9 / 31 / 32 / 33 (SPLITS below: the coverage test asserts that the mirror gives exactly these).
    # fp32: 346 images of 2 x 9 are 692 tiles of 8 x 8 (one partial image per split at 36 -> 40 channels: the reduce kernels change at 8 and 32).
    for wgs, _ in SPLITS["f32"]:
        add(346, 2, 9, 36, 40, 3, 1, "f32", wgrad_wgs=wgs)
    # bf16: from 8 splits on the grid is padded to a multiple of 8 and renumbered.  The planner rounds the wanted split count of bf16 launches
    # down to a multiple of 8, so no single tile count gives all seven: images of 5 x 33 are four tiles of 4 x 32, and the batch size sets the
    # total -- 132 tiles for 1 / 7 / 8 / 33 splits, 36 for 9 (the floor of 4 tiles a block), 152 for 31, 156 for 32.
    for N, wgs, _ in SPLITS["bf16"]:
        add(N, 5, 33, 36, 40, 3, 1, "bf16", wgrad_wgs=wgs)
    for N, wgs, s in SPLITS["bf16"]:
        if s in (7, 8, 9):                                      # the same switch of the numbering in wgrad_bf16_kernel
            add(N, 5, 33, 36, 40, 3, 1, "bf16", wgrad_wgs=wgs, wgrad_bf16_k4=0)
    # four partial images per workgroup (8 -> 8 channels, 168 tiles): 4 / 8 / 28 / 32 / 36 slices
    for wgs in NSUB4_WGS:
        add(3, 56, 56, 8, 8, 3, 1, "f32", wgrad_wgs=wgs)
    return cases


# the split-count cases: (unet_tuning.wgrad_wgs, splits) and (batch size, wgrad_wgs, splits)
SPLITS = {"f32": [(1, 1), (7, 7), (8, 8), (9, 9), (31, 31), (32, 32), (33, 33)],
          "bf16": [(33, 1, 1), (33, 7, 7), (33, 8, 8), (9, 16, 9), (38, 32, 31), (39, 32, 32), (33, 40, 33)]}
NSUB4_WGS = (1, 2, 7, 8, 9)

CASES = _build_cases()


def case_id(i, c=None):
    c = CASES[i] if c is None else c
    tune = ",".join(f"{k.replace('wgrad_', '')}={v}" for k, v in c.tuning)
    return f"{i:03d}-{plan(c)['family']}-{c.N}x{c.H}x{c.W}-{c.Cin}to{c.Cout}-k{c.ks}s{c.stride}-{c.dtype}" + (f"-{tune}" if tune else "")


# ------------------------------------------------------------------------------------------------------------------------ operands

def torch_dtype(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def exact_bound(c):
    """the largest magnitude any partial sum, dw or dbias can reach with exact_inputs, prefill included: below 2^24 every one is exact"""
    mx, md = EXACT_RANGE[c.dtype]
    return mx * md * pixels(c) + PREFILL


def exact_inputs(c, seed):
    """(x [N, H, W, Cin], dy [N, OH, OW, Cout]) fp32 host tensors of uniform integers (representable in the case's storage type)"""
    g = torch.Generator().manual_seed(seed)
    OH, OW = out_hw(c)
    mx, md = EXACT_RANGE[c.dtype]
    x = torch.randint(-mx, mx + 1, (c.N, c.H, c.W, c.Cin), generator=g).float()
    dy = torch.randint(-md, md + 1, (c.N, OH, OW, c.Cout), generator=g).float()
    return x, dy


def gauss_inputs(c, seed):
    """standard normal operands as test_conv_wgrad draws them (bf16 storage: rounded to bf16, as test_bf16_gpu does), NHWC fp32 host tensors"""
    g = torch.Generator().manual_seed(seed)
    OH, OW = out_hw(c)
    x = torch.randn(c.N, c.Cin, c.H, c.W, generator=g)
    dy = torch.randn(c.N, c.Cout, OH, OW, generator=g)
    if c.dtype == "bf16":
        x, dy = x.to(torch.bfloat16).float(), dy.to(torch.bfloat16).float()
    return x.permute(0, 2, 3, 1).contiguous(), dy.permute(0, 2, 3, 1).contiguous()


def reference(c, x, dy):
    """(dw [Cout, Cin, ks, ks], dbias [Cout]) in fp64 from NHWC host operands"""
    x64, dy64 = x.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2)
    dw = torch.nn.grad.conv2d_weight(x64, (c.Cout, c.Cin, c.ks, c.ks), dy64, stride=c.stride, padding=(c.ks - 1) // 2)
    return dw, dy64.sum((0, 2, 3))


def device_slice(a, co, cs, dtype, device="cuda"):
    """(ops.TS, check): the NHWC host tensor `a` as channels co .. co + C of a guard-banded [N, H, W, cs] buffer.  The pad lanes
    C .. rup(C, vec) behind the slice are zero (the project's convention); every other channel and both bands hold the canary."""
    import guard
    from unet_amd import ops
    N, H, W, C = a.shape
    v = ops.vec_of(dtype)
    assert co % v == 0 and cs % v == 0 and cs > co + rup(C, v)
    buf, check = guard.guarded((N, H, W, cs), dtype, device, fill=guard.CANARY[torch.float32])
    buf[..., co:co + C] = a.to(device=device, dtype=dtype)
    buf[..., co + C:co + rup(C, v)] = 0
    return ops.TS(buf, co, C), check


def operands(c, x, dy, device="cuda"):
    """((x slice, check), (dy slice, check)) of a case on the device"""
    x_co, x_cs, dy_co, dy_cs = strides(c)
    dt = torch_dtype(c)
    return device_slice(x, x_co, x_cs, dt, device), device_slice(dy, dy_co, dy_cs, dt, device)
