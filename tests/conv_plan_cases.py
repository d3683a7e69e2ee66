"""The fixed descriptor sweep behind tests/golden/conv_plans.json: what the conv dispatcher of libunet_hip.so answers, without a GPU, for
every family, tile shape, split count and error class it knows.  A case is a plain dict (hashable as JSON: the fixture carries the hash
of the whole list); `query` turns it into a unet_conv_desc over fake, aligned, never dereferenced addresses and asks the three host-only
entry points.  The library module is a parameter: the fixture is recorded against another build than the one under test."""
import ctypes as C
import hashlib
import json

X, WP, Y, RES, MASK, WS, COLSUM, COLSUMSQ, TAIL = (0x1000000 * (i + 1) for i in range(9))

CHANNELS = [(3, 32), (4, 32), (8, 32), (32, 5), (100, 5), (5, 100), (64, 64), (96, 100), (128, 128), (196, 228), (256, 192), (512, 512),
            (1024, 512)]
KS_STRIDE = [(1, 1), (3, 1), (3, 2)]
SIDES = [8, 16, 32, 64, 256]
BATCHES = [1, 2, 16]
# produced-channel ranges (cout_begin, cout_count) next to the whole launch; 192 = 128 + 64 is what ops._launch_conv splits, 228 = 128 + 100 is
# the two-launch last block of the 256-pixel tile
RANGES = {228: [(0, 128), (128, 100)], 192: [(0, 128), (128, 64)]}


def _rup(a, b):
    return (a + b - 1) // b * b


def conv_case(dtype, kind, ks, stride, side, N, cin, cout, ws="ok", tuning=None, **over):
    """dtype 0 = fp32, 1 = bf16; kind 0 = forward, 1 = dgrad (I* = the gradient's dims, O* = the forward input's); `side` is the larger of
    the two spatial sides; ws: "ok" (ample split-K workspace) | "none" | "short" (one float less than the library asks for)"""
    vec = 8 if dtype else 4
    big, small = side, (side - 1) // stride + 1
    c = dict(dtype=dtype, kind=kind, ks=ks, stride=stride, N=N, Cin=cin, Cout=cout, x_cs=_rup(cin, vec), y_cs=_rup(cout, vec),
             IH=small if kind else big, IW=small if kind else big, OH=big if kind else small, OW=big if kind else small, ws=ws, tuning=tuning)
    c.update(over)
    return c


def ps_case(dtype, side, N, cin, cout, tail=0, **over):
    """unet_conv_desc.pixel_shuffle: a 1x1 conv of `cout` = 4 nf channels stored as nf channels of a [N, 2 side, 2 side] buffer, with `tail`
    further channels copied behind them"""
    vec = 8 if dtype else 4
    c = dict(dtype=dtype, kind=0, ks=1, stride=1, N=N, Cin=cin, Cout=cout, x_cs=_rup(cin, vec), y_cs=_rup(cout // 4, 8) + _rup(tail, 4),
             IH=side, IW=side, OH=side, OW=side, pixel_shuffle=1, ws="none", tuning=None)
    if tail:
        c.update(ps_tail=TAIL, ps_tail_cs=_rup(tail, 4), ps_tail_co=0, ps_tail_c=tail, ps_tail_at=_rup(cout // 4, 8))
    c.update(over)
    return c


def cases():
    out = []

    def geometry(dtypes=(0, 1), kinds=(0, 1), kss=KS_STRIDE, sides=SIDES, batches=BATCHES, channels=CHANNELS, **kw):
        for dtype in dtypes:
            for kind in kinds:
                for ks, stride in kss:
                    for side in sides:
                        for N in batches:
                            for cin, cout in channels:
                                out.append(conv_case(dtype, kind, ks, stride, side, N, cin, cout, **kw))

    # 1. every geometry under the default tuning with an ample workspace
    geometry()
    # 2. channel ranges of the 228- and 192-wide layers
    for dtype in (0, 1):
        for kind in (0, 1):
            for ks, stride in KS_STRIDE:
                for side, N in ((16, 2), (64, 2), (256, 2), (32, 16)):
                    for cin, cout in ((196, 228), (256, 192)):
                        for b, n in RANGES[cout]:
                            out.append(conv_case(dtype, kind, ks, stride, side, N, cin, cout, cout_begin=b, cout_count=n))
    # 3. the deep stages (where plans split) without a workspace and with one that is a float short
    for ws in ("none", "short"):
        geometry(kss=[(1, 1), (3, 1)], sides=[8, 16, 32], batches=[1, 2], channels=CHANNELS[6:], ws=ws)
    # 4. bf16 with an fp32 output; fp32 with column sums (forward, the whole channel range)
    geometry(dtypes=(1,), batches=[2], y_f32=1)
    geometry(dtypes=(0,), kinds=(0,), batches=[2], colsum=COLSUM, colsumsq=COLSUMSQ)
    geometry(dtypes=(1,), kinds=(0,), kss=[(3, 1)], sides=[16], batches=[2], channels=CHANNELS[6:8], colsum=COLSUM)      # bf16: refused
    # 5. epilogue operands (the small-reduction families look at them) and per-image filters
    geometry(kss=[(1, 1), (3, 1)], sides=[16], batches=[2], res=RES, flags=5, mask=MASK)
    geometry(kss=[(1, 1), (3, 1)], sides=[16], batches=[2], wp_img_stride=1 << 20)
    # 6. tunings, each over the launches it can change
    some = dict(sides=[16, 64, 256], batches=[2])
    geometry(dtypes=(0,), kss=[(3, 1)], tuning=dict(f32_big_tile=0), **some)
    for v in (0, 2, 3):
        geometry(dtypes=(1,), kss=[(3, 1)], tuning=dict(bf16_big_tile=v), **some)
    for v in (0, 2):
        geometry(sides=[8, 16, 64], batches=[2], channels=CHANNELS[6:], tuning=dict(conv_splitk=v))
    geometry(dtypes=(0,), tuning=dict(mfma_shape=32), **some)
    geometry(sides=[8, 16, 64], batches=[1, 16], tuning=dict(plan_batch=1), channels=CHANNELS[:3] + CHANNELS[6:])
    geometry(kinds=(0,), kss=[(3, 1), (3, 2)], channels=CHANNELS[:3], tuning=dict(conv_smallcin=0), **some)
    for v in (0, 2):
        geometry(kss=[(1, 1)], channels=CHANNELS[3:5], tuning=dict(conv_head1x1=v), **some)
    for v in (-1, 1, 2):
        geometry(kss=[(1, 1)], tuning=dict(conv1x1_gemm=v), **some)
    for dtype in (0, 1):
        out.append(conv_case(dtype, 0, 3, 1, 64, 2, 64, 64, tuning="zero"))
        out.append(conv_case(dtype, 0, 1, 1, 64, 2, 5, 100, tuning="zero"))
    # 7. pixel-shuffle descriptors: valid, with a tail, too small a grid (unsupported), invalid
    for dtype in (0, 1):
        for side, N in ((64, 2), (64, 16), (256, 2), (16, 2)):
            for cin, cout in ((64, 256), (128, 512), (96, 384), (512, 1024)):
                out.append(ps_case(dtype, side, N, cin, cout))
                out.append(ps_case(dtype, side, N, cin, cout, tail=4))
                out.append(ps_case(dtype, side, N, cin, cout, tail=3, y_f32=dtype))
        out.append(ps_case(dtype, 64, 16, 64, 200))                       # Cout not 4 x 16 n
        out.append(ps_case(dtype, 64, 16, 64, 256, ks=3))
        out.append(ps_case(dtype, 64, 16, 64, 256, res=RES))
        out.append(ps_case(dtype, 64, 16, 64, 256, tail=4, ps_tail_at=4))  # the tail inside the shuffled channels
        out.append(ps_case(dtype, 64, 16, 64, 256, tuning=dict(conv1x1_gemm=1)))
        out.append(ps_case(dtype, 64, 16, 64, 256, tuning="zero"))
    out.append(ps_case(7, 64, 16, 64, 256))                                # unknown storage type
    # 8. descriptors the planner refuses
    for dtype in (0, 1):
        ok = dict(dtype=dtype, kind=0, ks=3, stride=1, side=16, N=2, cin=64, cout=64)
        for bad in (dict(ks=5), dict(stride=3), dict(ks=1, stride=2), dict(N=0), dict(kind=2), dict(x_co=2), dict(y_cs=60), dict(OH=17),
                    dict(cout_begin=8, cout_count=8), dict(cout_begin=64, cout_count=64), dict(wp_img_stride=2), dict(x=0), dict(x=X + 4),
                    dict(y=Y + 8), dict(res=RES + 4), dict(flags=4), dict(IH=1 << 12, IW=1 << 12, OH=1 << 12, OW=1 << 12, x_cs=1 << 8),
                    dict(N=1 << 20, IH=4096, IW=4096, OH=4096, OW=4096), dict(cout=5, y_cs=5 if dtype == 0 else 6)):
            geo = {k: bad.pop(k) for k in list(bad) if k in ("ks", "stride", "N", "kind", "cout")}
            out.append(conv_case(**{**ok, **geo}, **bad))
    out.append(conv_case(7, 0, 3, 1, 16, 2, 64, 64))                       # unknown storage type
    out.append(None)                                                        # a null descriptor
    return out


def sweep_hash(cs):
    return hashlib.sha256(json.dumps(cs, sort_keys=True).encode()).hexdigest()


def describe(c):
    return "NULL descriptor" if c is None else ", ".join(f"{k}={v:#x}" if isinstance(v, int) and v >= 0x1000000 else f"{k}={v}"
                                                         for k, v in c.items() if v is not None)


def query(L, c):
    """(unet_conv2d_variant, unet_conv2d_splitk_workspace, unet_conv2d_colsum_rows) of one case"""
    lib = L.lib
    if c is None:
        return [lib.unet_conv2d_variant(None), lib.unet_conv2d_splitk_workspace(None), lib.unet_conv2d_colsum_rows(None)]
    d = L.ConvDesc()
    d.x, d.wp, d.y = X, WP, Y
    for k, v in c.items():
        if k not in ("ws", "tuning"):
            setattr(d, k, v)
    tuning = c["tuning"]
    if tuning is not None:
        t = L.Tuning() if tuning == "zero" else L.Tuning.default(**tuning)
        d.tuning = C.pointer(t)
    need = lib.unet_conv2d_splitk_workspace(C.byref(d))
    if c["ws"] != "none" and need > 0:
        d.splitk_ws, d.splitk_ws_floats = WS, need - (1 if c["ws"] == "short" else 0)
    return [lib.unet_conv2d_variant(C.byref(d)), need, lib.unet_conv2d_colsum_rows(C.byref(d))]


def run(L, cs):
    return [query(L, c) for c in cs]
