"""Thin Python wrappers over the C ABI: torch tensors in, HIP launches out.

PyTorch is used for device memory and streams only.  Activations are fp32 NHWC
buffers; ``TS`` names a channel slice ``buf[..., co:co+C]`` of a buffer with
physical channel stride ``cs`` (this is how ``torch.cat`` disappears).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib as L
from ._lib import ConvDesc, WgradDesc, check, lib


# ---- kernel-selection switches (unet_tuning).  The LIBRARY keeps no state: every descriptor carries a pointer to the struct that is current
# on this side when it is built -- None (the defaults) unless a `with ops.tuning(...)` block is active in this thread.
import contextlib
import threading

_TUNE = threading.local()


@contextlib.contextmanager
def tuning(**fields):
    """`with ops.tuning(mfma_shape=32, conv_splitk=0): ...` -- launches issued by this thread inside the block carry these switches
    (A/B measurements; the tests cross-check independently written kernel families this way).  Blocks nest: inner fields override outer."""
    prev = getattr(_TUNE, "cur", None)
    cur = L.Tuning.default() if prev is None else L.Tuning.from_buffer_copy(prev)
    for k, v in fields.items():
        if k not in dict(L.Tuning._fields_):
            raise KeyError(f"unet_tuning has no field {k!r}")
        setattr(cur, k, int(v))
    _TUNE.cur = cur
    try:
        yield cur
    finally:
        _TUNE.cur = prev


def set_tuning(**fields) -> None:
    """the switches of THIS thread's launches from now on (outside `with tuning(...)` blocks); no arguments: back to the defaults.
    Python-side convenience for scripts and try / finally style tests -- the library itself stays stateless."""
    if not fields:
        _TUNE.cur = None
        return
    cur = getattr(_TUNE, "cur", None)
    cur = L.Tuning.default() if cur is None else L.Tuning.from_buffer_copy(cur)
    for k, v in fields.items():
        if k not in dict(L.Tuning._fields_):
            raise KeyError(f"unet_tuning has no field {k!r}")
        setattr(cur, k, int(v))
    _TUNE.cur = cur


def set_knob(name: str, v: int) -> int:
    """the value conventions of the setters the ABI had up to version 5 (unet_set_<name>), mapped onto unet_tuning fields"""
    v = int(v)
    if name == "mfma_shape":
        set_tuning(**({"f32_big_tile": int(v == -2)} if v < 0 else {"mfma_shape": v}))
    elif name == "wgrad_mfma_shape":
        set_tuning(**({"wgrad_bf16_k4": int(v == -2)} if v < 0 else {"wgrad_mfma_shape": v}))
    elif name == "bf16_big_tile":
        set_tuning(t256_tiles_per_wg=v - 100 if v >= 100 else 0, bf16_big_tile=(v if 2 <= v < 100 else int(bool(v))))
    elif name in ("conv_splitk", "wgrad_narrow", "wgrad_1x1", "t256_sliver", "conv1x1_gemm"):
        set_tuning(**{name: max(v, 0)})
    else:
        raise KeyError(name)
    return 0


def _tuning_ptr():
    cur = getattr(_TUNE, "cur", None)
    return None if cur is None else C.pointer(cur)


def wgrad_tuning_key():
    """the values of the switches a weight-gradient plan depends on (None = the defaults): cache key of planned workspace sizes"""
    cur = getattr(_TUNE, "cur", None)
    return None if cur is None else (cur.wgrad_mfma_shape, cur.wgrad_bf16_k4, cur.wgrad_1x1, cur.wgrad_narrow, cur.plan_batch, cur.wgrad_wgs)


# The launch stream of this thread as a raw hipStream_t.  torch.cuda.current_stream() builds a Stream object through several Python layers
# (device-index parsing, is_available(), an os.environ lookup): 8 us of a ~16 us host budget per launch -- scripts/host_profile.py showed the
# cfg1 step HOST-bound (issue time 6.95 ms = wall time), 29 % of it in that call.  The C entry points below are what it ends in.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


# a raw stream that replaces THIS THREAD's current one for the launches it issues while it is set (the side stream of the weight gradients:
# entering torch.cuda.stream(...) costs four current_stream() round trips per weight gradient).  Thread-local like the tuning state: a launch
# from another thread (a second model, a loader) never lands on somebody else's side stream.
class _StreamOverride(threading.local):
    raw: Optional[int] = None


_OVERRIDE = _StreamOverride()


def set_stream_override(raw: Optional[int]) -> None:
    _OVERRIDE.raw = raw


def _stream() -> int:
    o = _OVERRIDE.raw
    if o is not None:
        return o
    if _raw_stream is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def _device_index() -> int:
    return _raw_device() if _raw_device is not None else torch.cuda.current_device()


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def rup4(c: int) -> int:
    return (c + 3) // 4 * 4


def vec_of(dtype) -> int:
    """channels per 16-byte access: channel strides / offsets of a tensor are multiples of this"""
    return 8 if dtype == torch.bfloat16 else 4


def rupv(c: int, dtype) -> int:
    v = vec_of(dtype)
    return (c + v - 1) // v * v


@dataclass
class TS:
    """Channel slice of an NHWC buffer: fp32 (the parity path) or bf16 storage (BASELINE configs[1] variant)."""
    buf: torch.Tensor   # [N, H, W, cs] contiguous fp32 | bf16
    co: int
    C: int

    def __post_init__(self):
        assert self.buf.dtype in (torch.float32, torch.bfloat16) and self.buf.is_contiguous() and self.buf.dim() == 4
        v = vec_of(self.buf.dtype)
        assert self.co % v == 0 and self.cs % v == 0 and self.co + self.C <= self.cs, (self.co, self.C, self.cs)

    @property
    def bf16(self) -> bool: return self.buf.dtype == torch.bfloat16

    @property
    def cs(self) -> int: return self.buf.shape[3]
    @property
    def N(self) -> int: return self.buf.shape[0]
    @property
    def H(self) -> int: return self.buf.shape[1]
    @property
    def W(self) -> int: return self.buf.shape[2]
    @property
    def P(self) -> int: return self.buf.shape[0] * self.buf.shape[1] * self.buf.shape[2]
    @property
    def ptr(self) -> int: return self.buf.data_ptr()

    def view(self) -> torch.Tensor:
        return self.buf[..., self.co:self.co + self.C]

    def sub(self, off: int, C: int) -> "TS":
        return TS(self.buf, self.co + off, C)


def new_act(N, H, W, C, device, zero=False, dtype=torch.float32) -> TS:
    cs = rupv(C, dtype)
    need_zero = zero or cs != C
    buf = (torch.zeros if need_zero else torch.empty)((N, H, W, cs), dtype=dtype, device=device)
    return TS(buf, 0, C)


def _fn(name: str, t: "TS"):
    """the entry point for t's storage type: unet_<name> (fp32) or unet_<name>_bf16"""
    return getattr(lib, f"unet_{name}_bf16" if t.bf16 else f"unet_{name}")


def _need_f32(what: str, *ts):
    for t in ts:
        if t is not None and t.bf16:
            raise L.UnetHipError(f"{what}: not available with bf16 storage (fp32 parity path only)")


def full(buf: torch.Tensor, C: Optional[int] = None) -> TS:
    return TS(buf, 0, buf.shape[3] if C is None else C)


# ------------------------------------------------------------------ conv

def conv_out_hw(H, W, ks, stride):
    pad = (ks - 1) // 2
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


def pack_weights(w: torch.Tensor, mode: int, out: Optional[torch.Tensor] = None, dtype=torch.float32) -> torch.Tensor:
    """w: [Cout, Cin, ks, ks] contiguous fp32 master parameter.  mode 0 = forward image, 1 = dgrad image; dtype = storage type of
    the packed image (bf16: rounded once here, products accumulate in fp32)."""
    Cout, Cin, ks, _ = w.shape
    assert w.is_contiguous() and w.dtype == torch.float32
    if dtype == torch.bfloat16:
        n = lib.unet_pack_weights_size_bf16(Cout, Cin, ks, mode)
        if out is None or out.dtype != dtype:
            out = torch.empty(n, dtype=dtype, device=w.device)
        assert out.numel() >= n
        check(lib.unet_pack_weights_bf16(w.data_ptr(), out.data_ptr(), Cout, Cin, ks, mode, _stream()), "pack_weights_bf16")
        return out
    n = lib.unet_pack_weights_size(Cout, Cin, ks, mode)
    if out is None or out.dtype != dtype:
        out = torch.empty(n, dtype=torch.float32, device=w.device)
    assert out.numel() >= n
    check(lib.unet_pack_weights(w.data_ptr(), out.data_ptr(), Cout, Cin, ks, mode, _stream()), "pack_weights")
    return out


def pack_jobs(jobs, bf16: bool, device, cache: Optional[dict] = None):
    """Packed filter images of several convs in ONE launch (unet_pack_batch_run).  jobs: [(w [Cout,Cin,ks,ks] fp32 master parameter, packed
    image tensor, mode 0 | 1, out_scale [Cout] fp32 or None)].  The device job table holds raw addresses: `cache` (a dict owned by the
    caller) keeps tables keyed by every address in them."""
    if not jobs:
        return
    key = tuple((w.data_ptr(), wp.data_ptr(), mode, 0 if sc is None else sc.data_ptr()) for w, wp, mode, sc in jobs) + (bf16,)
    ent = None if cache is None else cache.get(key)
    if ent is None:
        arr = (L.PackJob * len(jobs))()
        for j, (w, wp, mode, sc) in zip(arr, jobs):
            assert w.is_contiguous() and w.dtype == torch.float32 and (sc is None or (sc.dtype == torch.float32 and sc.numel() >= w.shape[0]))
            j.w, j.wp = w.data_ptr(), wp.data_ptr()
            j.Cout, j.Cin, j.ks, j.mode = w.shape[0], w.shape[1], w.shape[2], mode
            j.out_scale = None if sc is None else sc.data_ptr()
        dt = L.BF16 if bf16 else L.F32
        host = torch.zeros(int(lib.unet_pack_batch_table_bytes(len(jobs))), dtype=torch.uint8)
        blocks = C.c_uint(0)
        check(lib.unet_pack_batch_build(arr, len(jobs), dt, host.data_ptr(), C.byref(blocks)), "pack_batch_build")
        ent = (host.to(device), len(jobs), int(blocks.value), dt)
        if cache is not None:
            cache[key] = ent
    table, n, blocks, dt = ent
    check(lib.unet_pack_batch_run(table.data_ptr(), n, blocks, dt, _stream()), "pack_batch_run")


def pack_weights_strided(w_base_ptr: int, so: int, sr: int, O: int, R: int, out: torch.Tensor) -> torch.Tensor:
    """packed 1x1 filter image whose (out o, reduction r) element is the element at w_base_ptr + es * (o*so + r*sr) of an activation buffer
    of out's storage type (es = 4 fp32 / 2 bf16)"""
    if out.dtype == torch.bfloat16:
        assert out.numel() >= lib.unet_pack_weights_size_bf16(O, R, 1, 0)
        check(lib.unet_pack_weights_strided_bf16(w_base_ptr, so, sr, out.data_ptr(), O, R, _stream()), "pack_weights_strided_bf16")
        return out
    assert out.numel() >= lib.unet_pack_weights_size(O, R, 1, 0)
    check(lib.unet_pack_weights_strided(w_base_ptr, so, sr, out.data_ptr(), O, R, _stream()), "pack_weights_strided")
    return out


def pack_size(O: int, R: int, dtype) -> int:
    """elements of the packed 1x1 image of an [O, R] operand in storage type dtype"""
    return int((lib.unet_pack_weights_size_bf16 if dtype == torch.bfloat16 else lib.unet_pack_weights_size)(O, R, 1, 0))


def row_softmax(x: "TS", y: "TS"):
    """y = softmax over the C channels of every pixel of x; x (the logits) is fp32, y fp32 or bf16"""
    _need_f32("row_softmax (logits)", x)
    fn = lib.unet_row_softmax_bf16 if y.bf16 else lib.unet_row_softmax
    check(fn(x.ptr, x.cs, x.co, y.ptr, y.cs, y.co, x.P, x.C, _stream()), "row_softmax")


def row_softmax_bwd(y: "TS", dy: "TS", dx: "TS"):
    """dx = y * (dy - sum_c y dy); y and dx share a storage type (fp32 | bf16), dy is fp32"""
    _need_f32("row_softmax_bwd (dy)", dy)
    assert y.bf16 == dx.bf16
    fn = lib.unet_row_softmax_bwd_bf16 if y.bf16 else lib.unet_row_softmax_bwd
    check(fn(y.ptr, y.cs, y.co, dy.ptr, dy.cs, dy.co, dx.ptr, dx.cs, dx.co, y.P, y.C, _stream()), "row_softmax_bwd")


# ---- fused SelfAttention for bf16 storage (csrc/attention.hip): the N x N matrix stays in registers
def sa_fused_supported(dp: int, C: int) -> bool:
    return bool(lib.unet_sa_fused_supported(int(dp), int(C)))


def sa_pack_elems(N: int, cc: int) -> int:
    return int(lib.unet_sa_pack_elems(int(N), int(cc)))


def sa_pack(x: "TS", out: torch.Tensor):
    """positions-innermost image of the channel slice x (rows = the H * W positions of each image): the operand of a product that sums over
    positions"""
    assert x.bf16 and out.dtype == torch.bfloat16 and out.numel() >= x.N * sa_pack_elems(x.H * x.W, x.C)
    check(lib.unet_sa_pack_bf16(x.ptr, x.cs, x.co, x.C, x.N, x.H * x.W, out.data_ptr(), _stream()), "sa_pack")


def sa_rows(N: int) -> int:
    """row count per image of the lse / D vectors of the fused attention kernels (whole 64-position blocks)"""
    return (N + 63) // 64 * 64


def sa_fwd(qkv: "TS", dp: int, C: int, vpack: torch.Tensor, O: "TS", lse: torch.Tensor):
    """O_j = sum_i softmax_i(G_j . F_i) H_i and lse_j for every image of the fused QKV buffer (F at channel 0, G at dp, H at 2 dp)"""
    assert qkv.bf16 and O.bf16 and qkv.co == 0 and lse.dtype == torch.float32 and O.C == C and O.P == qkv.P
    assert lse.numel() >= qkv.N * sa_rows(qkv.H * qkv.W) and vpack.numel() >= qkv.N * sa_pack_elems(qkv.H * qkv.W, C)
    check(lib.unet_sa_fwd_bf16(qkv.ptr, qkv.cs, dp, C, qkv.N, qkv.H * qkv.W, vpack.data_ptr(), O.ptr, O.cs, O.co, lse.data_ptr(), _stream()), "sa_fwd")


def sa_rowdot(a: "TS", o: "TS", D: torch.Tensor):
    assert a.bf16 and o.bf16 and a.C == o.C and a.P == o.P and D.dtype == torch.float32 and D.numel() >= a.N * sa_rows(a.H * a.W)
    check(lib.unet_sa_rowdot_bf16(a.ptr, a.cs, a.co, o.ptr, o.cs, o.co, a.N, a.H * a.W, a.C, D.data_ptr(), _stream()), "sa_rowdot")


def sa_bwd(qkv: "TS", dp: int, C: int, dO: "TS", dopack: torch.Tensor, gpack: torch.Tensor, fpack: torch.Tensor, lse: torch.Tensor,
           D: torch.Tensor, dqkv: "TS"):
    """the gradient of the whole QKV buffer (dF | dG | dH slices) from dO = dL/dO, with the weights recomputed from lse"""
    assert qkv.bf16 and dO.bf16 and dqkv.bf16 and qkv.co == 0 and dqkv.co == 0 and dqkv.cs == qkv.cs and dO.C == C and dO.P == qkv.P
    rows, N = qkv.N * sa_rows(qkv.H * qkv.W), qkv.H * qkv.W
    assert lse.dtype == torch.float32 and D.dtype == torch.float32 and lse.numel() >= rows and D.numel() >= rows        # [B][64 ceil(N / 64)]
    assert dopack.numel() >= qkv.N * sa_pack_elems(N, C) and min(gpack.numel(), fpack.numel()) >= qkv.N * sa_pack_elems(N, dp)
    check(lib.unet_sa_bwd_bf16(qkv.ptr, qkv.cs, dp, C, qkv.N, qkv.H * qkv.W, dO.ptr, dO.cs, dO.co, dopack.data_ptr(), gpack.data_ptr(),
                               fpack.data_ptr(), lse.data_ptr(), D.data_ptr(), dqkv.ptr, _stream()), "sa_bwd")


def cast_slice(x: "TS", y: "TS"):
    """fp32 slice -> bf16 slice (same geometry)"""
    assert not x.bf16 and y.bf16 and x.P == y.P and x.C == y.C
    check(lib.unet_cast_slice_bf16(x.ptr, x.cs, x.co, y.ptr, y.cs, y.co, x.P, x.C, _stream()), "cast_slice")


def _conv_desc(x: TS, wp: torch.Tensor, y: TS, ks: int, stride: int, kind: int, bias=None, res: Optional[TS] = None,
               mask: Optional[TS] = None, relu=False, colsum=None, colsumsq=None) -> ConvDesc:
    d = ConvDesc()
    d.x, d.x_cs, d.x_co = x.ptr, x.cs, x.co
    d.wp = wp.data_ptr()
    d.bias = _p(bias)
    if res is not None:
        d.res, d.res_cs, d.res_co = res.ptr, res.cs, res.co
    flags = L.CONV_RELU if relu else 0
    if mask is not None:
        d.mask, d.mask_cs, d.mask_co = mask.ptr, mask.cs, mask.co
        flags |= L.CONV_MASK
    d.y, d.y_cs, d.y_co = y.ptr, y.cs, y.co
    d.N, d.IH, d.IW, d.Cin = x.N, x.H, x.W, x.C
    d.OH, d.OW, d.Cout = y.H, y.W, y.C
    d.ks, d.stride, d.kind, d.flags = ks, stride, kind, flags
    d.colsum, d.colsumsq = _p(colsum), _p(colsumsq)
    d.tuning = _tuning_ptr()
    if x.bf16:
        assert wp.dtype == torch.bfloat16 and (res is None or res.bf16) and (mask is None or mask.bf16)
        d.dtype, d.y_f32 = L.BF16, int(not y.bf16)
    else:
        assert wp.dtype == torch.float32 and not y.bf16
    return d


class ConvProbe:
    """bench.py: brackets every conv launch of one kernel instantiation with events on the launch stream and
    sums the ALGORITHMIC FLOPs (2 * pixels * Cin * Cout * k*k, no padding) of those launches."""

    def __init__(self, variant: int):
        self.variant = variant
        self.events = []
        self.flops = 0.0
        self.bytes = 0.0          # ALGORITHMIC bytes of the probed launches: every operand tensor once in, the result once out
        self.detail = []          # (what, N, H, W, Cin, Cout, ks, stride, flops) per probed launch
        # a stream whose work must not run next to a probed launch (the side stream of the weight gradients): the launch stream waits for
        # it in front of the first event, so that the events time THIS kernel alone, not this kernel sharing the chip with another one
        self.exclusive_of = None

    def summary(self):
        ms = [a.elapsed_time(b) for a, b in self.events]
        return {"launches": len(ms), "total_ms": sum(ms), "avg_ms": sum(ms) / max(1, len(ms)), "flops": self.flops, "bytes": self.bytes}


CONV_PROBE: Optional[ConvProbe] = None


# Scratch for split-K conv launches (unet_conv_desc.splitk_ws): one fp32 buffer per device, grown on demand, reused by every launch
# (stream ordered).  It reaches its final size during the eager warm-up steps, so a captured step sees a static address.
_SPLITK_WS = {}
_SPLITK_RETIRED = []      # outgrown buffers stay alive: a captured hipGraph may hold their address in its split launches


def _splitk_ws(d: ConvDesc):
    need = int(lib.unet_conv2d_splitk_workspace(C.byref(d)))
    if need == 0:
        d.splitk_ws, d.splitk_ws_floats = None, 0
        return
    dev = _device_index()
    buf = _SPLITK_WS.get(dev)
    if buf is None or buf.numel() < need:
        if torch.cuda.is_current_stream_capturing():
            raise L.UnetHipError("split-K workspace would have to grow inside a hipGraph capture: run the eager warm-up at this geometry first")
        if buf is not None:
            _SPLITK_RETIRED.append(buf)
        buf = _SPLITK_WS[dev] = torch.empty(max(need, 1 << 22), dtype=torch.float32, device=f"cuda:{dev}")
    d.splitk_ws, d.splitk_ws_floats = buf.data_ptr(), buf.numel()


def _launch_conv_part(d: ConvDesc, what: str, alg_flops: float):
    _splitk_ws(d)
    pr = CONV_PROBE
    if pr is not None and lib.unet_conv2d_variant(C.byref(d)) % 1000000 == pr.variant:      # (split-K launches of the instantiation included)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if pr.exclusive_of is not None:
            torch.cuda.current_stream().wait_stream(pr.exclusive_of)
        e0.record()
        check(lib.unet_conv2d(C.byref(d), _stream()), what)
        e1.record()
        pr.events.append((e0, e1))
        pr.flops += alg_flops
        # x + y (+ residual, + mask) once each at the storage width, the packed filter image once, the bias vector
        es = 2 if d.dtype == L.BF16 else 4
        co = d.cout_count or d.Cout
        pix_in, pix_out = d.N * d.IH * d.IW, d.N * d.OH * d.OW
        pr.bytes += (es * (pix_in * d.Cin + pix_out * co * (1 + (1 if d.res else 0) + (1 if d.mask else 0)))
                     + (4 - es) * pix_out * co * d.y_f32 + es * d.ks * d.ks * d.Cin * co)
        pr.detail.append((what, d.N, d.OH, d.OW, d.Cin, d.cout_count or d.Cout, d.ks, d.stride, alg_flops))
        return
    check(lib.unet_conv2d(C.byref(d), _stream()), what)


def _launch_conv(d: ConvDesc, what: str, alg_flops: float):
    """A produced-channel count of k*128 + r with 0 < r <= 64 would run its last 128-wide channel block at most half full
    (and re-stage the input tile for it): issue the k*128 part and the r-wide part as two launches, the second with a 64- or
    32-wide channel block.  Column sums (rows depend on the tile geometry of ONE launch) keep the single launch."""
    Co = d.Cout
    r = Co % 128
    if Co > 128 and 0 < r <= 64 and not d.colsum:
        for b, n in ((0, Co - r), (Co - r, r)):
            d.cout_begin, d.cout_count = b, n
            _launch_conv_part(d, what, alg_flops * n / Co)
        d.cout_begin = d.cout_count = 0
        return
    _launch_conv_part(d, what, alg_flops)


def conv2d(x: TS, wp: torch.Tensor, y: TS, ks: int, stride: int = 1, bias=None, res=None, mask=None, relu=False,
           colsum=None, colsumsq=None, wp_img_stride: int = 0):
    """wp_img_stride > 0: image n of the batch uses the packed filter image at wp + n * wp_img_stride floats"""
    d = _conv_desc(x, wp, y, ks, stride, L.CONV_FWD, bias, res, mask, relu, colsum, colsumsq)
    d.wp_img_stride = wp_img_stride
    _launch_conv(d, "conv2d", 2.0 * y.P * x.C * y.C * ks * ks)


def _ps_desc(x: TS, wp: torch.Tensor, X: TS, bias, relu: bool) -> ConvDesc:
    """1x1 conv of 4 * X.C channels whose epilogue stores PixelShuffle(2)(act(conv(x))) into the slice X of a [N, 2H, 2W] buffer"""
    assert X.H == 2 * x.H and X.W == 2 * x.W and X.N == x.N and x.bf16 == X.bf16
    d = ConvDesc()
    d.x, d.x_cs, d.x_co = x.ptr, x.cs, x.co
    d.wp, d.bias = wp.data_ptr(), _p(bias)
    d.y, d.y_cs, d.y_co = X.ptr, X.cs, X.co
    d.N, d.IH, d.IW, d.Cin = x.N, x.H, x.W, x.C
    d.OH, d.OW, d.Cout = x.H, x.W, 4 * X.C
    d.ks, d.stride, d.kind, d.flags = 1, 1, L.CONV_FWD, (L.CONV_RELU if relu else 0)
    d.dtype = L.BF16 if x.bf16 else L.F32
    d.tuning = _tuning_ptr()
    d.pixel_shuffle = 1
    return d


def conv1x1_shuffle_applies(x: TS, X: TS) -> bool:
    """does the library take conv1x1 -> act -> PixelShuffle(2) as ONE launch for this geometry (unet_conv2d_variant == 8)?"""
    d = _ps_desc(x, torch.empty(0), X, None, True)
    d.wp = 16          # (any aligned non-null address: the query only plans)
    return int(lib.unet_conv2d_variant(C.byref(d))) == 8


def conv1x1_shuffle_tail_ok(X: TS, tail: TS, at: int) -> bool:
    """can conv1x1_shuffle append `tail`'s channels at channel `at` of X's buffer (unet_conv_desc.ps_tail: whole quads at quad-aligned places)?"""
    return (tail.bf16 == X.bf16 and (tail.N, tail.H, tail.W) == (X.N, X.H, X.W) and tail.cs % 4 == 0 and tail.co % 4 == 0 and at % 4 == 0
            and tail.co + rup4(tail.C) <= tail.cs and at >= X.co + X.C and at + rup4(tail.C) <= X.cs)


def conv1x1_shuffle(x: TS, wp_ps: torch.Tensor, X: TS, bias=None, relu=True, tail: Optional[TS] = None, tail_at: int = 0):
    """X = PixelShuffle(2)(act(conv1x1(x) + bias)); wp_ps is the mode-2 packed image (columns in pixel-shuffle order).
    tail: an NHWC slice of X's geometry copied to channels [tail_at, tail_at + C) of X's BUFFER by the same launch (the network input behind
    the up-sampled channels of the final concat)"""
    d = _ps_desc(x, wp_ps, X, bias, relu)
    if tail is not None:
        assert conv1x1_shuffle_tail_ok(X, tail, tail_at)
        d.ps_tail, d.ps_tail_cs, d.ps_tail_co, d.ps_tail_c, d.ps_tail_at = tail.ptr, tail.cs, tail.co, tail.C, tail_at
    check(lib.unet_conv2d(C.byref(d), _stream()), "conv1x1_shuffle")


def shuffle_bwd_xmask(dX: TS, X: TS, dyc: TS):
    """dyc[h,w,4c+2i+j] = X[2h+i,2w+j,c] > 0 ? dX[2h+i,2w+j,c] : 0 (the adjoint of conv1x1_shuffle's store incl. its ReLU)"""
    assert dyc.C == 4 * dX.C and dX.H == 2 * dyc.H and dX.W == 2 * dyc.W and X.C == dX.C
    check(_fn("shuffle_bwd_xmask", dX)(dX.ptr, dX.cs, dX.co, X.ptr, X.cs, X.co, dyc.ptr, dyc.cs, dyc.co, dyc.N, dyc.H, dyc.W, dX.C, _stream()),
          "shuffle_bwd_xmask")


def conv2d_variant(x: TS, wp: torch.Tensor, y: TS, ks: int, stride: int = 1, kind: int = 0) -> int:
    """id of the kernel instantiation the planner picks for this launch (unet_conv2d_variant; scripts/layer_table.py, tests)"""
    d = _conv_desc(x, wp, y, ks, stride, kind)
    _splitk_ws(d)
    return int(lib.unet_conv2d_variant(C.byref(d)))


def conv2d_dgrad(dy: TS, wp_dgrad: torch.Tensor, dx: TS, ks: int, stride: int = 1, res=None, mask=None, colsum=None):
    """dx = conv^T(dy); optional residual add, ReLU-backward mask, column sums of the result."""
    d = _conv_desc(dy, wp_dgrad, dx, ks, stride, L.CONV_DGRAD, None, res, mask, False, colsum, None)
    _launch_conv(d, "conv2d_dgrad", 2.0 * dy.P * dy.C * dx.C * ks * ks)


def conv_colsum_rows(x: TS, wp, y: TS, ks, stride, kind) -> int:
    d = _conv_desc(x, wp, y, ks, stride, kind)
    r = lib.unet_conv2d_colsum_rows(C.byref(d))
    if r < 0:
        check(r, "conv2d_colsum_rows")
    return r


def _wgrad_desc(x: TS, dy: TS, dw, dbias, ks, stride, ws, accumulate) -> WgradDesc:
    d = WgradDesc()
    d.x, d.x_cs, d.x_co = x.ptr, x.cs, x.co
    d.dy, d.dy_cs, d.dy_co = dy.ptr, dy.cs, dy.co
    d.dw, d.dbias = _p(dw), _p(dbias)
    d.N, d.IH, d.IW, d.Cin = x.N, x.H, x.W, x.C
    d.OH, d.OW, d.Cout = dy.H, dy.W, dy.C
    d.ks, d.stride = ks, stride
    d.workspace = _p(ws)
    d.workspace_floats = 0 if ws is None else ws.numel()
    d.accumulate = int(accumulate)
    d.tuning = _tuning_ptr()
    assert x.bf16 == dy.bf16
    d.dtype = L.BF16 if x.bf16 else L.F32
    return d


def wgrad_workspace(x: TS, dy: TS, ks, stride, with_bias=False) -> int:
    d = _wgrad_desc(x, dy, torch.empty(0), None, ks, stride, None, 0)
    d.dw = 1  # non-null placeholder for validation
    return int(lib.unet_conv2d_wgrad_workspace(C.byref(d)))


def wgrad_uses_dma(x: TS, dy: TS, ks, stride) -> bool:
    """whether the planner sends this weight gradient to the LDS-DMA form of the narrow-output kernel (under the current tuning)"""
    d = _wgrad_desc(x, dy, None, None, ks, stride, None, 0)
    r = lib.unet_conv2d_wgrad_dma(C.byref(d))
    assert r >= 0, "wgrad_uses_dma: bad descriptor"
    return r == 1


def conv2d_wgrad(x: TS, dy: TS, dw: torch.Tensor, ks: int, stride: int, ws: torch.Tensor, dbias=None, accumulate=False):
    d = _wgrad_desc(x, dy, dw, dbias, ks, stride, ws, accumulate)
    check(lib.unet_conv2d_wgrad(C.byref(d), _stream()), "conv2d_wgrad")


# ------------------------------------------------------------------ batch norm

def bn_stats_rows(P: int) -> int:
    return lib.unet_bn_stats_rows(P)


def bn_stats(x: TS, partial: torch.Tensor):
    check(_fn("bn_stats", x)(x.ptr, x.cs, x.co, x.P, x.C, partial.data_ptr(), _stream()), "bn_stats")


def bn_finalize(psum, psumsq, rows, count, C_, gamma, beta, rmean, rvar, momentum, eps, scale, shift, smean, sinvstd, tracked=None):
    assert tracked is None or tracked.dtype == torch.int64
    check(lib.unet_bn_finalize(_p(psum), _p(psumsq), rows, count, C_, _p(gamma), _p(beta), _p(rmean), _p(rvar), momentum, eps,
                               _p(scale), _p(shift), _p(smean), _p(sinvstd), _p(tracked), _stream()), "bn_finalize")


def bn_eval_coeffs(gamma, beta, rmean, rvar, eps, scale, shift):
    check(lib.unet_bn_eval_coeffs(_p(gamma), _p(beta), _p(rmean), _p(rvar), eps, rmean.numel(), _p(scale), _p(shift), _stream()),
          "bn_eval_coeffs")


def affine_act(x: TS, y: TS, scale=None, shift=None, x2: Optional[TS] = None, scale2=None, shift2=None, relu=False):
    check(_fn("affine_act", x)(x.ptr, x.cs, x.co, _p(scale), _p(shift),
                              None if x2 is None else x2.ptr, 0 if x2 is None else x2.cs, 0 if x2 is None else x2.co,
                              _p(scale2), _p(shift2), y.ptr, y.cs, y.co, x.P, x.C, int(relu), _stream()), "affine_act")


def bn_bwd_reduce(dout: TS, out: Optional[TS], x: TS, mean, invstd, partial):
    check(_fn("bn_bwd_reduce", x)(dout.ptr, dout.cs, dout.co, None if out is None else out.ptr, 0 if out is None else out.cs,
                                 0 if out is None else out.co, x.ptr, x.cs, x.co, _p(mean), _p(invstd), x.P, x.C,
                                 partial.data_ptr(), _stream()), "bn_bwd_reduce")


def bn_bwd_finalize(partial, rows, count, C_, dgamma, dbeta, c1, c2):
    check(lib.unet_bn_bwd_finalize(_p(partial), rows, count, C_, _p(dgamma), _p(dbeta), _p(c1), _p(c2), _stream()), "bn_bwd_finalize")


def bn_bwd_apply(dout: TS, out: Optional[TS], x: TS, mean, invstd, gamma, c1, c2, dx: TS, gout: Optional[TS] = None,
                 g_accumulate=False):
    check(_fn("bn_bwd_apply", x)(dout.ptr, dout.cs, dout.co, None if out is None else out.ptr, 0 if out is None else out.cs,
                                0 if out is None else out.co, x.ptr, x.cs, x.co, _p(mean), _p(invstd), _p(gamma), _p(c1), _p(c2),
                                dx.ptr, dx.cs, dx.co, None if gout is None else gout.ptr, 0 if gout is None else gout.cs,
                                0 if gout is None else gout.co, int(g_accumulate), x.P, x.C, _stream()), "bn_bwd_apply")


# ------------------------------------------------------------------ pooling

def maxpool(x: TS, y: TS, idx: Optional[torch.Tensor]):
    check(_fn("maxpool3x3s2", x)(x.ptr, x.cs, x.co, y.ptr, y.cs, y.co, _p(idx), x.N, x.H, x.W, x.C, y.H, y.W, _stream()), "maxpool")


def maxpool_bwd(dy: TS, idx: torch.Tensor, dx: TS, accumulate=False):
    check(_fn("maxpool3x3s2_bwd", dy)(dy.ptr, dy.cs, dy.co, idx.data_ptr(), dx.ptr, dx.cs, dx.co, dx.N, dx.H, dx.W, dx.C, dy.H, dy.W,
                                    int(accumulate), _stream()), "maxpool_bwd")


def avgpool(x: TS, y: TS):
    check(_fn("avgpool2_ceil", x)(x.ptr, x.cs, x.co, y.ptr, y.cs, y.co, x.N, x.H, x.W, x.C, y.H, y.W, _stream()), "avgpool")


def avgpool_bwd(dy: TS, dx: TS, accumulate=False):
    check(_fn("avgpool2_ceil_bwd", dy)(dy.ptr, dy.cs, dy.co, dx.ptr, dx.cs, dx.co, dx.N, dx.H, dx.W, dx.C, dy.H, dy.W, int(accumulate),
                                     _stream()), "avgpool_bwd")


# ------------------------------------------------------------------ decoder data movement

def shuffle_blur(yc: TS, X: TS, blur: bool):
    assert yc.C == 4 * X.C and X.H == 2 * yc.H and X.W == 2 * yc.W
    check(_fn("shuffle_blur", yc)(yc.ptr, yc.cs, yc.co, X.ptr, X.cs, X.co, yc.N, yc.H, yc.W, X.C, int(blur), _stream()), "shuffle_blur")


def shuffle_blur_bwd(dX: TS, yc: TS, dyc: TS, blur: bool):
    assert yc.C == 4 * dX.C and dX.H == 2 * yc.H and dX.W == 2 * yc.W
    check(_fn("shuffle_blur_bwd", dX)(dX.ptr, dX.cs, dX.co, yc.ptr, yc.cs, yc.co, dyc.ptr, dyc.cs, dyc.co, yc.N, yc.H, yc.W, dX.C,
                                    int(blur), _stream()), "shuffle_blur_bwd")


def resize_nearest(x: TS, y: TS):
    assert x.bf16 == y.bf16
    check(_fn("resize_nearest", x)(x.ptr, x.cs, x.co, y.ptr, y.cs, y.co, x.N, x.H, x.W, y.H, y.W, x.C, _stream()), "resize_nearest")


def resize_nearest_bwd(dy: TS, dx: TS):
    assert dy.bf16 == dx.bf16
    check(_fn("resize_nearest_bwd", dy)(dy.ptr, dy.cs, dy.co, dx.ptr, dx.cs, dx.co, dx.N, dx.H, dx.W, dy.H, dy.W, dx.C, _stream()),
          "resize_nearest_bwd")


def nchw_to_nhwc(x: torch.Tensor, y: TS, at: Optional[int] = None):
    """NCHW fp32 -> the channels of the NHWC slice `y`; with `at`, into channels [at, at + C) of y's buffer instead -- the one writer
    that may start at ANY channel (scalar stores): the network-input half of the final concat sits behind an up-sampling path whose
    width need not be a multiple of the vector width (xresnet34_deep: 102)."""
    N, C_, H, W = x.shape
    if at is None:
        assert x.is_contiguous() and y.C == C_
        check(_fn("nchw_to_nhwc", y)(x.data_ptr(), y.ptr, y.cs, y.co, N, C_, H, W, _stream()), "nchw_to_nhwc")
    else:
        assert x.is_contiguous() and y.co == 0 and at + C_ <= y.cs
        check(_fn("nchw_to_nhwc", y)(x.data_ptr(), y.ptr, y.cs, at, N, C_, H, W, _stream()), "nchw_to_nhwc")


def nhwc_to_nchw(x: TS, y: torch.Tensor):
    _need_f32("nhwc_to_nchw", x)
    assert y.is_contiguous()
    check(lib.unet_nhwc_to_nchw(x.ptr, x.cs, x.co, y.data_ptr(), x.N, x.C, x.H, x.W, _stream()), "nhwc_to_nchw")


def copy_slice(x: TS, y: TS, accumulate=False):
    check(_fn("copy_slice", x)(x.ptr, x.cs, x.co, y.ptr, y.cs, y.co, x.P, x.C, int(accumulate), _stream()), "copy_slice")


def relu_mask(g: TS, ref: TS, y: TS):
    assert g.bf16 == ref.bf16 == y.bf16
    check(_fn("relu_mask", g)(g.ptr, g.cs, g.co, ref.ptr, ref.cs, ref.co, y.ptr, y.cs, y.co, g.P, g.C, _stream()), "relu_mask")


def colsum_workspace(P, C_) -> int:
    return int(lib.unet_colsum_workspace(P, C_))


def colsum(x: TS, out: torch.Tensor, ws: torch.Tensor):
    _need_f32("colsum", x)
    assert ws.numel() >= colsum_workspace(x.P, x.C)
    check(lib.unet_colsum(x.ptr, x.cs, x.co, x.P, x.C, out.data_ptr(), ws.data_ptr(), _stream()), "colsum")


def dot(x: TS, y: TS, out: torch.Tensor, ws: torch.Tensor):
    """out[0] = sum(x * y) over all pixels and channels (fp32 accumulation)"""
    assert x.bf16 == y.bf16
    assert ws.numel() >= colsum_workspace(x.P, x.C)
    check(_fn("dot", x)(x.ptr, x.cs, x.co, y.ptr, y.cs, y.co, x.P, x.C, out.data_ptr(), ws.data_ptr(), _stream()), "dot")


# ------------------------------------------------------------------ loss

CE_MAXC = 64        # most classes the classification-loss kernels take (elementwise.hip CE_MAXC)


def ce_workspace(P) -> int:
    return int(lib.unet_ce_workspace(P))


def ce_fwd(z: TS, target: torch.Tensor, weight, loss, denom, ws):
    _need_f32("ce_fwd", z)
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == z.P
    check(lib.unet_ce_fwd(z.ptr, z.cs, z.co, target.data_ptr(), _p(weight), z.P, z.C, loss.data_ptr(), denom.data_ptr(),
                          ws.data_ptr(), _stream()), "ce_fwd")


def ce_fwd_parts(z: TS, target: torch.Tensor, weight, numden: torch.Tensor, ws):
    """numden[0] = sum w[y] * nll, numden[1] = sum w[y] over this rank's pixels (tile-DDP: all-reduced before the division)"""
    _need_f32("ce_fwd_parts", z)
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == z.P and numden.numel() >= 2
    check(lib.unet_ce_fwd_parts(z.ptr, z.cs, z.co, target.data_ptr(), _p(weight), z.P, z.C, numden.data_ptr(), ws.data_ptr(), _stream()),
          "ce_fwd_parts")


def ce_bwd(z: TS, target, weight, denom, gscale: float, dz: TS):
    check(_fn("ce_bwd", dz)(z.ptr, z.cs, z.co, target.data_ptr(), _p(weight), z.P, z.C, denom.data_ptr(), gscale, dz.ptr, dz.cs,
                          dz.co, _stream()), "ce_bwd")


def _pw_args(what: str, z: TS, target: torch.Tensor, pixel_weight: torch.Tensor):
    """one weight per pixel: float32 [P], contiguous, on the logits' device (the kernels index it by the pixel, not by the class)"""
    if not isinstance(target, torch.Tensor) or target.dtype != torch.int64 or not target.is_contiguous() or target.numel() != z.P:
        raise ValueError(f"{what}: target must be a contiguous int64 tensor of {z.P} pixels")
    if not isinstance(pixel_weight, torch.Tensor) or pixel_weight.dtype != torch.float32:
        raise ValueError(f"{what}: pixel_weight must be a float32 tensor, got {getattr(pixel_weight, 'dtype', type(pixel_weight))}")
    if not pixel_weight.is_contiguous() or pixel_weight.numel() != z.P:
        raise ValueError(f"{what}: pixel_weight must be contiguous with one weight per pixel ({z.P}), got {pixel_weight.numel()}")
    if pixel_weight.device != z.buf.device or target.device != z.buf.device:
        raise ValueError(f"{what}: target and pixel_weight must live on the logits' device {z.buf.device}")
    if z.C > CE_MAXC:
        raise ValueError(f"{what}: at most {CE_MAXC} classes, got {z.C}")


def ce_fwd_pw(z: TS, target: torch.Tensor, pixel_weight: torch.Tensor, loss, denom, ws):
    """loss[0] = sum pw * nll / sum pw, denom[0] = sum pw over the pixels whose target is in [0, C)"""
    _need_f32("ce_fwd_pw", z)
    _pw_args("ce_fwd_pw", z, target, pixel_weight)
    if ws.numel() < ce_workspace(z.P):
        raise ValueError(f"ce_fwd_pw: the workspace holds {ws.numel()} floats, needs {ce_workspace(z.P)}")
    check(lib.unet_ce_fwd_pw(z.ptr, z.cs, z.co, target.data_ptr(), pixel_weight.data_ptr(), z.P, z.C, loss.data_ptr(), denom.data_ptr(),
                             ws.data_ptr(), _stream()), "ce_fwd_pw")


def ce_fwd_parts_pw(z: TS, target: torch.Tensor, pixel_weight: torch.Tensor, numden: torch.Tensor, ws):
    """numden[0] = sum pw * nll, numden[1] = sum pw over this rank's pixels (tile-DDP: all-reduced before the division)"""
    _need_f32("ce_fwd_parts_pw", z)
    _pw_args("ce_fwd_parts_pw", z, target, pixel_weight)
    if numden.numel() < 2 or ws.numel() < ce_workspace(z.P):
        raise ValueError(f"ce_fwd_parts_pw: numden needs 2 floats and the workspace {ce_workspace(z.P)}, got {numden.numel()} and {ws.numel()}")
    check(lib.unet_ce_fwd_parts_pw(z.ptr, z.cs, z.co, target.data_ptr(), pixel_weight.data_ptr(), z.P, z.C, numden.data_ptr(), ws.data_ptr(),
                                   _stream()), "ce_fwd_parts_pw")


def ce_bwd_pw(z: TS, target, pixel_weight: torch.Tensor, denom, gscale: float, dz: TS):
    """dz = gscale * pw * (softmax(z) - onehot(y)) / denom[0]; dz fp32 or bf16"""
    _pw_args("ce_bwd_pw", z, target, pixel_weight)
    if dz.P != z.P or dz.C != z.C:
        raise ValueError(f"ce_bwd_pw: dz is {dz.P} x {dz.C}, the logits are {z.P} x {z.C}")
    check(_fn("ce_bwd_pw", dz)(z.ptr, z.cs, z.co, target.data_ptr(), pixel_weight.data_ptr(), z.P, z.C, denom.data_ptr(), gscale, dz.ptr, dz.cs,
                               dz.co, _stream()), "ce_bwd_pw")


def focal_fwd(z: TS, target: torch.Tensor, weight, gamma: float, loss, ws):
    """loss[0] = mean over all pixels of (1 - exp(-ce))^gamma * ce, ce = w[y] * nll (fastai FocalLossFlat(gamma, axis=1))"""
    _need_f32("focal_fwd", z)
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == z.P
    check(lib.unet_focal_fwd(z.ptr, z.cs, z.co, target.data_ptr(), _p(weight), z.P, z.C, float(gamma), loss.data_ptr(), ws.data_ptr(), _stream()),
          "focal_fwd")


def focal_bwd(z: TS, target, weight, gamma: float, gscale: float, dz: TS):
    check(_fn("focal_bwd", dz)(z.ptr, z.cs, z.co, target.data_ptr(), _p(weight), z.P, z.C, float(gamma), gscale, dz.ptr, dz.cs, dz.co, _stream()),
          "focal_bwd")


def dice_workspace(B: int, HW: int, C: int) -> int:
    return int(lib.unet_dice_workspace(B, HW, C))


def dice_fwd(z: TS, target: torch.Tensor, smooth: float, square_in_union: bool, mean_div: int, loss, coef, ws):
    """fastai DiceLoss over the z.N samples of the slice: loss[0] = sum_{b,c} 1 - (2 I + smooth) / (U + smooth), divided by mean_div when
    mean_div > 0 ('mean'); coef [N*C*2] receives d loss / dI and d loss / dU per (sample, class) for dice_bwd"""
    _need_f32("dice_fwd", z)
    if z.C > CE_MAXC:
        raise ValueError(f"dice_fwd: at most {CE_MAXC} classes, got {z.C}")
    HW = z.H * z.W
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == z.P
    assert coef.dtype == torch.float32 and coef.numel() >= 2 * z.N * z.C and ws.numel() >= dice_workspace(z.N, HW, z.C)
    check(lib.unet_dice_fwd(z.ptr, z.cs, z.co, target.data_ptr(), z.N, HW, z.C, float(smooth), int(bool(square_in_union)), int(mean_div),
                            loss.data_ptr(), coef.data_ptr(), ws.data_ptr(), _stream()), "dice_fwd")


def dice_bwd(z: TS, target, square_in_union: bool, coef, gscale: float, dz: TS):
    assert dz.N == z.N and dz.H == z.H and dz.W == z.W and dz.C == z.C and coef.numel() >= 2 * z.N * z.C
    check(_fn("dice_bwd", dz)(z.ptr, z.cs, z.co, target.data_ptr(), z.N, z.H * z.W, z.C, int(bool(square_in_union)), coef.data_ptr(),
                              float(gscale), dz.ptr, dz.cs, dz.co, _stream()), "dice_bwd")


def combined_workspace(B: int, HW: int, C: int) -> int:
    return int(lib.unet_combined_workspace(B, HW, C))


def combined_fwd(z: TS, target: torch.Tensor, weight, gamma: float, smooth: float, square_in_union: bool, mean_div: int, terms, coef, ws):
    """CombinedLoss = focal + alpha * Dice in one pass over the logits: terms[0] = the FocalLossFlat(gamma, weight) mean over all pixels,
    terms[1] = the DiceLoss(smooth, square_in_union) sum over the z.N samples and the classes, divided by mean_div when mean_div > 0; coef
    [N*C*2] as dice_fwd writes it.  The caller combines the terms (alpha, tile-DDP normalisation)."""
    _need_f32("combined_fwd", z)
    if z.C > CE_MAXC:
        raise ValueError(f"combined_fwd: at most {CE_MAXC} classes, got {z.C}")
    HW = z.H * z.W
    assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == z.P and terms.numel() >= 2
    assert coef.dtype == torch.float32 and coef.numel() >= 2 * z.N * z.C and ws.numel() >= combined_workspace(z.N, HW, z.C)
    check(lib.unet_combined_fwd(z.ptr, z.cs, z.co, target.data_ptr(), _p(weight), z.N, HW, z.C, float(gamma), float(smooth),
                                int(bool(square_in_union)), int(mean_div), terms.data_ptr(), coef.data_ptr(), ws.data_ptr(), _stream()),
          "combined_fwd")


def combined_bwd(z: TS, target, weight, gamma: float, square_in_union: bool, coef, fscale: float, dscale: float, dz: TS):
    """dz = fscale * d focal / d z + dscale * d dice / d z (the terms of combined_fwd; dscale carries alpha)"""
    assert dz.N == z.N and dz.H == z.H and dz.W == z.W and dz.C == z.C and coef.numel() >= 2 * z.N * z.C
    check(_fn("combined_bwd", dz)(z.ptr, z.cs, z.co, target.data_ptr(), _p(weight), z.N, z.H * z.W, z.C, float(gamma),
                                  int(bool(square_in_union)), coef.data_ptr(), float(fscale), float(dscale), dz.ptr, dz.cs, dz.co, _stream()),
          "combined_bwd")


REG_KINDS = {"mse": 0, "l1": 1, "smoothl1": 2}


def regloss_fwd(z: TS, target: torch.Tensor, kind: str, beta: float, loss, ws):
    _need_f32("regloss_fwd", z)
    assert target.dtype == torch.float32 and target.is_contiguous() and target.numel() == z.P and z.C == 1
    check(lib.unet_regloss_fwd(z.ptr, z.cs, z.co, target.data_ptr(), z.P, REG_KINDS[kind], float(beta), loss.data_ptr(), ws.data_ptr(),
                               _stream()), "regloss_fwd")


def regloss_bwd(z: TS, target: torch.Tensor, kind: str, beta: float, gscale: float, dz: TS):
    _need_f32("regloss_bwd", z, dz)
    check(lib.unet_regloss_bwd(z.ptr, z.cs, z.co, target.data_ptr(), z.P, REG_KINDS[kind], float(beta), float(gscale), dz.ptr, dz.cs,
                               dz.co, _stream()), "regloss_bwd")


def softmax_argmax(z: TS, probs: Optional[torch.Tensor], amax: Optional[torch.Tensor]):
    _need_f32("softmax_argmax", z)
    check(lib.unet_softmax_argmax(z.ptr, z.cs, z.co, z.N, z.H, z.W, z.C, _p(probs), _p(amax), _stream()), "softmax_argmax")


# ------------------------------------------------------------------ optimiser

def adam_step(p, g, m, v, code, lrs, mom, sqr_mom, eps, wd, step, grad_scale=1.0):
    arr = (C.c_float * 4)(*([float(l) for l in lrs] + [0.0] * (4 - len(lrs))))
    check(lib.unet_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), code.data_ptr(), p.numel(), arr,
                             float(mom), float(sqr_mom), float(eps), float(wd), int(step), float(grad_scale), _stream()), "adam_step")


def mosaic_accumulate(probs: torch.Tensor, mosaic: torch.Tensor, count: torch.Tensor, y0: int, x0: int):
    Cc, th, tw = probs.shape
    _, MH, MW = mosaic.shape
    check(lib.unet_mosaic_accumulate(probs.data_ptr(), Cc, th, tw, mosaic.data_ptr(), count.data_ptr(), MH, MW, y0, x0, _stream()),
          "mosaic_accumulate")


def mosaic_finalize(mosaic: torch.Tensor, count: torch.Tensor, amax: Optional[torch.Tensor]):
    Cc, MH, MW = mosaic.shape
    check(lib.unet_mosaic_finalize(mosaic.data_ptr(), count.data_ptr(), Cc, MH, MW, _p(amax), _stream()), "mosaic_finalize")


def _blend_tables(what: str, wy: torch.Tensor, wx: torch.Tensor, th: int, tw: int):
    assert wy.dtype == torch.float32 and wx.dtype == torch.float32 and wy.is_contiguous() and wx.is_contiguous(), what
    assert wy.numel() >= th and wx.numel() >= tw, (what, wy.numel(), th, wx.numel(), tw)


def mosaic_accumulate_weighted(probs: torch.Tensor, wy: torch.Tensor, wx: torch.Tensor, mosaic: torch.Tensor, count: torch.Tensor,
                               wsum: torch.Tensor, y0: int, x0: int):
    """the Gaussian-blended slab add: probs [C, th, tw] added as fl(w * p), w = fl(wy[ty] * wx[tx]); w added to wsum"""
    Cc, th, tw = probs.shape
    _, MH, MW = mosaic.shape
    _blend_tables("mosaic_accumulate_weighted", wy, wx, th, tw)
    assert wsum.shape == (MH, MW) and wsum.dtype == torch.float32 and count.shape == (MH, MW)
    check(lib.unet_mosaic_accumulate_weighted(probs.data_ptr(), Cc, th, tw, wy.data_ptr(), wx.data_ptr(), mosaic.data_ptr(), count.data_ptr(),
                                              wsum.data_ptr(), MH, MW, y0, x0, _stream()), "mosaic_accumulate_weighted")


# ------------------------------------------------------------------ sliding-window predict over an integer raster (csrc/raster.hip)

RASTER_TYPES = {torch.uint8: 0, torch.uint16: 1, torch.int16: 2, torch.int32: 3, torch.float32: 4}


class WindowSource:
    """Band-sequential integer (or float) samples on the device that windows are cut from: ONE raster [C, H, W] (``src_stride`` 0) or a
    batch of staged tiles [n, C, h, w].  Sample (source s, band c, row y, column x) = data[s, c, y, x]."""

    def __init__(self, data: torch.Tensor, div255_twice: bool = False):
        assert data.is_cuda and data.is_contiguous() and data.dim() in (3, 4) and data.dtype in RASTER_TYPES, (data.shape, data.dtype)
        self.data, self.rtype, self.div2 = data, RASTER_TYPES[data.dtype], int(bool(div255_twice))
        self.C, self.H, self.W = data.shape[-3:]
        self.src_stride = 0 if data.dim() == 3 else self.C * self.H * self.W


def window_table(rows, device) -> torch.Tensor:
    """int32 [n, 4] device table of (y0, x0, source index, 0)"""
    t = torch.zeros((len(rows), 4), dtype=torch.int32)
    if len(rows):
        a = torch.as_tensor(rows, dtype=torch.int32)
        t[:, :a.shape[1]] = a
    return t.to(device)


@dataclass
class WindowBatch:
    """windows [first, first + n) of a device window table over a WindowSource: an input batch of the network that is never
    materialised as an NCHW fp32 tensor -- HipDynamicUnet writes it straight into its NHWC input buffers (window_gather)"""
    src: WindowSource
    table: torch.Tensor
    first: int
    n: int
    th: int
    tw: int

    def write(self, dst_buf: torch.Tensor, at: int, orient: Optional[int] = None):
        """orient None: the plain gather; a D4 code (unet_amd/tta.py): every window written as g(window), code 0 included"""
        if orient is None:
            window_gather(self.src, self.table, self.first, self.n, self.th, self.tw, dst_buf, at)
        else:
            window_gather_oriented(self.src, self.table, self.first, self.n, self.th, self.tw, dst_buf, at, orient)


def raster_nodata_zero(src: WindowSource, nodata: float):
    assert src.data.dim() == 3
    check(lib.unet_raster_nodata_zero(src.data.data_ptr(), src.rtype, src.C, src.H * src.W, float(nodata), _stream()), "raster_nodata_zero")


def window_nonzero(src: WindowSource, table: torch.Tensor, th: int, tw: int) -> torch.Tensor:
    """int64 [n]: non-zero samples of every window (all bands)"""
    n = table.shape[0]
    out = torch.empty(n, dtype=torch.int64, device=table.device)
    if n:
        check(lib.unet_window_nonzero(src.data.data_ptr(), src.rtype, src.C, src.H * src.W, src.W, table.data_ptr(), n, th, tw,
                                      out.data_ptr(), _stream()), "window_nonzero")
    return out


def window_gather(src: WindowSource, table: torch.Tensor, first: int, n: int, th: int, tw: int, dst_buf: torch.Tensor, at: int):
    """windows [first, first + n) of the table -> channels [at, at + C) of the NHWC buffer dst_buf [>= n, th, tw, cs], scaled"""
    assert dst_buf.dim() == 4 and dst_buf.shape[0] >= n and tuple(dst_buf.shape[1:3]) == (th, tw) and dst_buf.is_contiguous()
    assert 0 <= first and first + n <= table.shape[0]
    dt = L.BF16 if dst_buf.dtype == torch.bfloat16 else L.F32
    check(lib.unet_window_gather(src.data.data_ptr(), src.rtype, src.C, src.src_stride, src.H * src.W, src.W,
                                 table.data_ptr() + 16 * first, n, th, tw, src.div2, dst_buf.data_ptr(), dst_buf.shape[3], at, dt,
                                 _stream()), "window_gather")


def window_gather_oriented(src: WindowSource, table: torch.Tensor, first: int, n: int, th: int, tw: int, dst_buf: torch.Tensor, at: int,
                           orient: int):
    """window_gather with every window written as g(window), g the D4 code `orient` (codes 4..7 need th == tw)"""
    assert dst_buf.dim() == 4 and dst_buf.shape[0] >= n and tuple(dst_buf.shape[1:3]) == (th, tw) and dst_buf.is_contiguous()
    assert 0 <= first and first + n <= table.shape[0]
    dt = L.BF16 if dst_buf.dtype == torch.bfloat16 else L.F32
    check(lib.unet_window_gather_oriented(src.data.data_ptr(), src.rtype, src.C, src.src_stride, src.H * src.W, src.W,
                                          table.data_ptr() + 16 * first, n, th, tw, src.div2, dst_buf.data_ptr(), dst_buf.shape[3], at, dt,
                                          int(orient), _stream()), "window_gather_oriented")


def nchw_to_nhwc_oriented(x: torch.Tensor, dst_buf: torch.Tensor, at: int, orient: int):
    """fp32 NCHW x [N, C, H, W] -> channels [at, at + C) of the NHWC buffer dst_buf [>= N, H, W, cs] (fp32 or bf16), image n written
    as g(x[n]), g the D4 code `orient`"""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    N, C_, H, W = x.shape
    assert dst_buf.dim() == 4 and dst_buf.shape[0] >= N and tuple(dst_buf.shape[1:3]) == (H, W) and dst_buf.is_contiguous()
    assert at >= 0 and at + C_ <= dst_buf.shape[3]
    dt = L.BF16 if dst_buf.dtype == torch.bfloat16 else L.F32
    check(lib.unet_nchw_to_nhwc_oriented(x.data_ptr(), dst_buf.data_ptr(), dst_buf.shape[3], at, N, C_, H, W, dt, int(orient), _stream()),
          "nchw_to_nhwc_oriented")


def tta_accumulate(z: TS, n: int, orient: int, raw: bool, first: bool, acc: torch.Tensor, finalize_k: int = 0,
                   probs: Optional[torch.Tensor] = None, amax: Optional[torch.Tensor] = None):
    """acc [>= n, H, W, cs] fp32 (channels [0, C)) = (first ? 0 : acc) + g^-1(softmax(z)) -- raw=True: g^-1(z) -- for the fp32 NHWC logits
    z of n windows produced under code g = orient.  finalize_k > 0 (last code of a set of k): acc /= k in place; probs (NCHW fp32
    [n, C, H, W]) and amax (int64 [n, H, W]) are written when given."""
    _need_f32("tta_accumulate", z)
    assert z.N >= n > 0
    assert acc.dtype == torch.float32 and acc.is_contiguous() and acc.dim() == 4 and acc.shape[0] >= n
    assert tuple(acc.shape[1:3]) == (z.H, z.W) and acc.shape[3] >= z.C
    assert finalize_k > 0 or (probs is None and amax is None)
    assert probs is None or (probs.dtype == torch.float32 and probs.is_contiguous() and tuple(probs.shape) == (n, z.C, z.H, z.W))
    assert amax is None or (amax.dtype == torch.int64 and amax.is_contiguous() and tuple(amax.shape) == (n, z.H, z.W))
    check(lib.unet_tta_accumulate(z.ptr, z.cs, z.co, n, z.C, z.H, z.W, int(orient), int(bool(raw)), int(bool(first)), acc.data_ptr(),
                                  acc.shape[3], int(finalize_k), _p(probs), _p(amax), _stream()), "tta_accumulate")


# ------------------------------------------------------------------ training feed (csrc/raster.hip: unet_tiles_stage / unet_mask_stage)

def _flip_bits(flips, n: int, at: int):
    """(hflip, vflip) bit masks of images [at, at + n) from a sequence of (h, v) pairs (None: nothing flipped)"""
    h = v = 0
    if flips is not None:
        for j in range(n):
            fh, fv = flips[at + j]
            h |= int(bool(fh)) << j
            v |= int(bool(fv)) << j
    return h, v


def tiles_stage(src: torch.Tensor, div255_twice: bool, out: torch.Tensor, flips=None):
    """staged integer tiles [n, C, H, W] (device) -> fp32 NCHW batch `out`, scaled like learner.scale_input (bit-equal); flips[j] = (h, v)"""
    assert src.is_cuda and src.is_contiguous() and src.dim() == 4 and src.dtype in RASTER_TYPES, (src.shape, src.dtype)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == tuple(src.shape)
    n, Cb, H, W = src.shape
    per = Cb * H * W
    for at in range(0, n, 64):
        m = min(64, n - at)
        hb, vb = _flip_bits(flips, m, at)
        check(lib.unet_tiles_stage(src.data_ptr() + at * per * src.element_size(), RASTER_TYPES[src.dtype], m, Cb, H, W, int(bool(div255_twice)),
                                   hb, vb, out.data_ptr() + at * per * 4, _stream()), "tiles_stage")


def mask_stage(src: torch.Tensor, out: torch.Tensor, flips=None):
    """staged masks [n, H, W] (device, any raster sample type) -> `out` int64 (classification) or float32 (regression targets)"""
    assert src.is_cuda and src.is_contiguous() and src.dim() == 3 and src.dtype in RASTER_TYPES, (src.shape, src.dtype)
    assert out.is_cuda and out.is_contiguous() and out.dtype in (torch.int64, torch.float32) and tuple(out.shape) == tuple(src.shape)
    n, H, W = src.shape
    for at in range(0, n, 64):
        m = min(64, n - at)
        hb, vb = _flip_bits(flips, m, at)
        check(lib.unet_mask_stage(src.data_ptr() + at * H * W * src.element_size(), RASTER_TYPES[src.dtype], m, H, W, hb, vb,
                                  out.data_ptr() + at * H * W * out.element_size(), int(out.dtype == torch.float32), _stream()), "mask_stage")


def dice_counts(pred: torch.Tensor, targ: torch.Tensor, n_cls: int, counts: torch.Tensor):
    """counts int64 [3, n_cls] += (intersection, predicted, target) pixel counts per class of this batch (DiceMulti)"""
    assert pred.dtype == torch.int64 and targ.dtype == torch.int64 and pred.is_contiguous() and targ.is_contiguous()
    assert pred.numel() == targ.numel() and counts.dtype == torch.int64 and counts.numel() == 3 * n_cls and counts.is_contiguous()
    check(lib.unet_dice_counts(pred.data_ptr(), targ.data_ptr(), pred.numel(), n_cls, counts.data_ptr(), _stream()), "dice_counts")


# ------------------------------------------------------------------ geometric augmentation (csrc/warp.hip: unet_warp_affine[_mask])

WARP_MAX_IMAGES = 64       # warp.hip MAXMAPS


def _chunks(n: int, limit: int):
    """(at, m) for every call of a kernel that takes at most `limit` images: images [at, at + m) of n"""
    for at in range(0, n, limit):
        yield at, min(limit, n - at)


def _image_ptr(t: torch.Tensor, at: int) -> int:
    """the address of image `at` of the contiguous batch t"""
    return t.data_ptr() + at * math.prod(t.shape[1:]) * t.element_size()


def _struct_ptr(array, at: int):
    """a pointer to element `at` of a ctypes array"""
    return C.cast(C.byref(array, at * C.sizeof(array._type_)), C.POINTER(array._type_))


def _warp_args(what: str, src: torch.Tensor, dst: torch.Tensor, inv_maps, dims: int):
    """the checked maps, fp32 [n, 6], of a warp of images (dims 4: [n, C, H, W] fp32) or masks (dims 3: [n, H, W] int64 or fp32)"""
    if not (src.is_cuda and dst.is_cuda):
        raise RuntimeError(f"{what}: the warp runs on the device only (HIP, no CPU fallback); got {src.device} / {dst.device} tensors")
    assert src.dim() == dims and src.is_contiguous() and dst.is_contiguous() and src.shape == dst.shape and src.dtype == dst.dtype, \
        (what, src.shape, dst.shape, src.dtype, dst.dtype)
    import numpy as np
    maps = np.ascontiguousarray(inv_maps, dtype=np.float32).reshape(-1, 6)
    assert maps.shape[0] == src.shape[0], (what, maps.shape, src.shape)
    assert src.dtype in ((torch.float32,) if dims == 4 else (torch.int64, torch.float32)), src.dtype
    return maps


def warp_affine(src: torch.Tensor, dst: torch.Tensor, inv_maps, interp: int, border: int, fill: float = 0.0):
    """dst[j] = src[j] sampled at inv_maps[j] (2 x 3 per image, output -> source) with interp 0 nearest / 1 bilinear and a cv2 border
    code; src / dst [n, C, H, W] fp32 on the device, out of place"""
    maps = _warp_args("warp_affine", src, dst, inv_maps, 4)
    n, Cc, H, W = src.shape
    for at, m in _chunks(n, WARP_MAX_IMAGES):
        check(lib.unet_warp_affine(_image_ptr(src, at), _image_ptr(dst, at), m, Cc, H, W, maps[at:at + m].ctypes.data_as(L.c_float_p),
                                   int(interp), int(border), float(fill), _stream()), "warp_affine")


def warp_affine_mask(src: torch.Tensor, dst: torch.Tensor, inv_maps, border: int, fill: float = 0.0):
    """the nearest-neighbour warp of masks [n, H, W] int64 (classification) or fp32 (regression targets), same maps as warp_affine"""
    maps = _warp_args("warp_affine_mask", src, dst, inv_maps, 3)
    n, H, W = src.shape
    for at, m in _chunks(n, WARP_MAX_IMAGES):
        check(lib.unet_warp_affine_mask(_image_ptr(src, at), _image_ptr(dst, at), int(src.dtype == torch.float32), m, H, W,
                                        maps[at:at + m].ctypes.data_as(L.c_float_p), int(border), float(fill), _stream()), "warp_affine_mask")


# ------------------------------------------------------------------ non-rigid augmentation (csrc/warp_field.hip)

FIELD_KINDS = {"dense": L.FIELD_DENSE, "grid": L.FIELD_GRID, "optical": L.FIELD_OPTICAL}


def _field_args(what: str, src: torch.Tensor, dst: torch.Tensor, kind: str, params, fired, pre_maps, dims: int):
    """the checked arguments of a field warp, as a function of the first image of a call: at -> (kind code, descriptors, field or None,
    grid step x, grid step y), the run of arguments unet_warp_field and unet_warp_field_mask share"""
    import numpy as np
    if kind not in FIELD_KINDS:
        raise ValueError(f"{what}: unknown kind {kind!r} (dense, grid, optical)")
    n = src.shape[0]
    pre = np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (n, 1)) if pre_maps is None else pre_maps
    pre = _warp_args(what, src, dst, pre, dims)
    flags = [bool(v) for v in fired]
    assert len(flags) == n, (what, len(flags), n)
    H, W = src.shape[-2:]
    images = (L.FieldImage * n)()
    for j in range(n):
        images[j].fired = int(flags[j])
        images[j].pre[:] = pre[j].tolist()
    field, steps = None, (0, 0)
    if kind == "dense":
        field = params
        if not field.is_cuda:
            raise RuntimeError(f"{what}: the field lives on the device (HIP, no CPU fallback); got a {field.device} tensor")
        assert field.dtype == torch.float32 and field.is_contiguous() and tuple(field.shape) == (n, 2, H, W), (what, field.shape, field.dtype)
    elif kind == "grid":
        step_x, step_y, nodes = params
        nodes = np.ascontiguousarray(nodes, dtype=np.float32)
        steps = (int(step_x), int(step_y))
        assert nodes.shape == (n, 2, L.FIELD_MAX_CELLS + 1), (what, nodes.shape)
        if min(steps) < 1 or -(-W // steps[0]) > L.FIELD_MAX_CELLS or -(-H // steps[1]) > L.FIELD_MAX_CELLS:
            raise ValueError(f"{what}: grid steps {steps} on a {H} x {W} image (1..{L.FIELD_MAX_CELLS} cells per axis)")
        for j in range(n):
            for a in range(2):
                images[j].nodes[a][:] = nodes[j, a].tolist()
    else:
        opt = np.ascontiguousarray(params, dtype=np.float32)
        assert opt.shape == (n, 3), (what, opt.shape)
        for j in range(n):
            images[j].optical[:] = opt[j].tolist()
    return lambda at: (FIELD_KINDS[kind], _struct_ptr(images, at), None if field is None else _image_ptr(field, at), *steps)


def warp_field(src: torch.Tensor, dst: torch.Tensor, kind: str, params, fired, pre_maps=None, interp: int = 1, border: int = 4,
               fill: float = 0.0):
    """dst[j] = src[j] sampled at pre_maps[j] * (p + d_j(p)) (include/unet_hip.h): kind "dense" with params the field [n, 2, H, W] fp32
    on the device, "grid" with params (step_x, step_y, nodes [n, 2, 17]) or "optical" with params [n, 3] = (k, dx, dy); d_j = 0 where
    fired[j] is false; pre_maps [n, 6]: D4 maps of the grid as augment.inverse_map gives them (None: identities).  src / dst [n, C, H, W] fp32 on the device, out of place; batches above 16
    images run in chunks"""
    field_args = _field_args("warp_field", src, dst, kind, params, fired, pre_maps, 4)
    n, Cc, H, W = src.shape
    for at, m in _chunks(n, L.FIELD_MAX_IMAGES):
        check(lib.unet_warp_field(_image_ptr(src, at), _image_ptr(dst, at), m, Cc, H, W, *field_args(at), int(interp), int(border),
                                  float(fill), _stream()), "warp_field")


def warp_field_mask(src: torch.Tensor, dst: torch.Tensor, kind: str, params, fired, pre_maps=None, border: int = 4, fill: float = 0.0):
    """the nearest-neighbour field warp of masks [n, H, W] int64 or fp32, same arguments as warp_field"""
    field_args = _field_args("warp_field_mask", src, dst, kind, params, fired, pre_maps, 3)
    n, H, W = src.shape
    for at, m in _chunks(n, L.FIELD_MAX_IMAGES):
        check(lib.unet_warp_field_mask(_image_ptr(src, at), _image_ptr(dst, at), int(src.dtype == torch.float32), m, H, W, *field_args(at),
                                       int(border), float(fill), _stream()), "warp_field_mask")


def elastic_field(field: torch.Tensor, workspace: torch.Tensor, keys, alpha, fired, same_dxdy: bool, taps):
    """field [n, 2, H, W] fp32 on the device = the ElasticTransform displacements of n images (include/unet_hip.h): keys [n, 2] Philox
    key words, alpha a scalar or [n], fired [n] (false: zeros), taps an odd number (at most 401) of fp32 filter taps; workspace: a device
    tensor of the field's shape for the row-pass result.  Batches above 64 images run in chunks"""
    import numpy as np
    if not (field.is_cuda and workspace.is_cuda):
        raise RuntimeError(f"elastic_field: the field is made on the device only (HIP, no CPU fallback); got {field.device} / "
                           f"{workspace.device} tensors")
    assert field.dim() == 4 and field.shape[1] == 2 and field.is_contiguous() and field.dtype == torch.float32, (field.shape, field.dtype)
    assert workspace.shape == field.shape and workspace.is_contiguous() and workspace.dtype == torch.float32, (workspace.shape, workspace.dtype)
    n, _, H, W = field.shape
    taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    if len(taps) > L.ELASTIC_MAX_KSIZE or len(taps) % 2 == 0:
        raise ValueError(f"elastic_field: {len(taps)} taps (odd, at most {L.ELASTIC_MAX_KSIZE})")
    keys = np.asarray(keys, dtype=np.int64).reshape(n, 2)
    alphas = np.broadcast_to(np.asarray(alpha, dtype=np.float32), (n,))
    flags = [bool(v) for v in fired]
    assert len(flags) == n, (len(flags), n)
    images = (L.ElasticImage * n)()
    for j in range(n):
        images[j] = L.ElasticImage(int(keys[j, 0]) & 0xffffffff, int(keys[j, 1]) & 0xffffffff, float(alphas[j]), int(flags[j]), int(bool(same_dxdy)))
    for at, m in _chunks(n, L.ELASTIC_MAX_IMAGES):
        check(lib.unet_elastic_field(_image_ptr(field, at), _image_ptr(workspace, at), m, H, W, _struct_ptr(images, at),
                                     taps.ctypes.data_as(L.c_float_p), len(taps), _stream()), "elastic_field")


# ------------------------------------------------------------------ pixel-level augmentation (csrc/pixel_aug.hip)

def _pixel_pieces(what: str, ops_: list, Cc: int) -> list:
    """one image's op list as programs the kernel takes: [(PixelOp list, rectangle list)], each <= 8 ops and <= 32 rectangles"""
    flat = []
    for op in ops_:
        if op[0] == "rects":                                       # more than 32 rectangles: several FILL_RECTS ops
            rects = list(op[1])
            flat += [("rects", rects[k:k + L.PIXEL_MAX_RECTS], op[2]) for k in range(0, len(rects), L.PIXEL_MAX_RECTS)]
        else:
            flat.append(op)
    pieces, cur, rects = [], [], []
    for op in flat:
        kind = op[0]
        if len(cur) == L.PIXEL_MAX_OPS or (kind == "rects" and len(rects) + len(op[1]) > L.PIXEL_MAX_RECTS):
            pieces.append((cur, rects))
            cur, rects = [], []
        if kind == "bc":
            cur.append(L.PixelOp(L.PIXEL_BRIGHTNESS_CONTRAST, 0, 0, float(op[1]), float(op[2])))
        elif kind == "gamma":
            cur.append(L.PixelOp(L.PIXEL_GAMMA, 0, 0, float(op[1]), 0.0))
        elif kind == "noise":
            code = L.PIXEL_GAUSS_NOISE | (L.PIXEL_PER_CHANNEL if op[5] else 0)
            cur.append(L.PixelOp(code, int(op[1]) & 0xffffffff, int(op[2]) & 0xffffffff, float(op[3]), float(op[4])))
        elif kind == "rects":
            cur.append(L.PixelOp(L.PIXEL_FILL_RECTS, len(rects), len(op[1]), float(op[2]), 0.0))
            rects += [tuple(int(v) for v in r) for r in op[1]]
        elif kind == "drop":
            bits = 0
            for c in op[1]:
                if not 0 <= int(c) < Cc:
                    raise ValueError(f"{what}: channel {c} of a {Cc}-channel image")
                bits |= 1 << int(c)
            cur.append(L.PixelOp(L.PIXEL_CHANNEL_DROP, bits, 0, float(op[2]), 0.0))
        elif kind == "permute":
            perm = [int(c) for c in op[1]]
            if Cc > 16:
                raise ValueError(f"{what}: a channel permutation supports at most 16 channels, the image has {Cc}")
            if sorted(perm) != list(range(Cc)):
                raise ValueError(f"{what}: {perm} is not a permutation of {Cc} channels")
            bits = sum(c << (4 * k) for k, c in enumerate(perm))
            cur.append(L.PixelOp(L.PIXEL_CHANNEL_PERMUTE, bits & 0xffffffff, bits >> 32, 0.0, 0.0))
        else:
            raise ValueError(f"{what}: unknown op {kind!r}")
    if cur:
        pieces.append((cur, rects))
    return pieces


def _fill_rects(dst, rects):
    for k, r in enumerate(rects):
        for q in range(4):
            dst[k][q] = r[q]


def pixel_ops(x: torch.Tensor, programs: dict):
    """the pointwise programs {image index: [op, ...]} applied IN PLACE to the fp32 batch x [n, C, H, W] on the device, one launch per 8
    images that have a program; images without one are not touched.  An op is ("bc", alpha, beta), ("gamma", gamma),
    ("noise", key0, key1, mean, sigma, per_channel), ("rects", [(y0, x0, y1, x1), ...], fill), ("drop", [channel, ...], fill) or
    ("permute", [source channel of channel 0, ...]): include/unet_hip.h."""
    if not x.is_cuda:
        raise RuntimeError(f"pixel_ops: the pixel programs run on the device only (HIP, no CPU fallback); got a {x.device} tensor")
    assert x.dim() == 4 and x.is_contiguous() and x.dtype == torch.float32, (x.shape, x.dtype)
    n, Cc, H, W = x.shape
    pieces = {int(j): _pixel_pieces("pixel_ops", ops_, Cc) for j, ops_ in programs.items() if ops_}
    assert all(0 <= j < n for j in pieces), (sorted(pieces), n)
    for rnd in range(max((len(p) for p in pieces.values()), default=0)):        # (one round unless a program outgrows 8 ops / 32 rectangles)
        todo = sorted(j for j, p in pieces.items() if len(p) > rnd)
        for at in range(0, len(todo), L.PIXEL_MAX_PROGS):
            chunk = todo[at:at + L.PIXEL_MAX_PROGS]
            progs = (L.PixelProg * len(chunk))()
            for pr, j in zip(progs, chunk):
                ops_, rects = pieces[j][rnd]
                pr.image, pr.nops, pr.nrects = j, len(ops_), len(rects)
                for k, op in enumerate(ops_):
                    pr.ops[k] = op
                _fill_rects(pr.rects, rects)
            check(lib.unet_pixel_ops(x.data_ptr(), n, Cc, H, W, C.addressof(progs), len(chunk), _stream()), "pixel_ops")


def fill_rects_mask(mask: torch.Tensor, rects: dict, fill):
    """the rectangles {mask index: [(y0, x0, y1, x1), ...]} of the device masks [n, H, W] (int64 or fp32) set to fill, in place"""
    if not mask.is_cuda:
        raise RuntimeError(f"fill_rects_mask: runs on the device only (HIP, no CPU fallback); got a {mask.device} tensor")
    assert mask.dim() == 3 and mask.is_contiguous() and mask.dtype in (torch.int64, torch.float32), (mask.shape, mask.dtype)
    n, H, W = mask.shape
    todo = []                                                       # (mask index, at most 32 rectangles); an index may repeat
    for j in sorted(rects):
        assert 0 <= j < n, (j, n)
        rs = [tuple(int(v) for v in r) for r in rects[j]]
        todo += [(int(j), rs[k:k + L.PIXEL_MAX_RECTS]) for k in range(0, len(rs), L.PIXEL_MAX_RECTS)]
    while todo:
        chunk, rest, last = [], [], -1
        for j, rs in todo:                                          # strictly increasing indices per launch
            if len(chunk) < L.PIXEL_MAX_PROGS and j > last:
                chunk.append((j, rs))
                last = j
            else:
                rest.append((j, rs))
        sets = (L.RectSet * len(chunk))()
        for s, (j, rs) in zip(sets, chunk):
            s.image, s.nrects = j, len(rs)
            _fill_rects(s.rects, rs)
        check(lib.unet_fill_rects_mask(mask.data_ptr(), int(mask.dtype == torch.float32), n, H, W, C.addressof(sets), len(chunk), float(fill),
                                       _stream()), "fill_rects_mask")
        todo = rest


def blur_separable(src: torch.Tensor, dst: torch.Tensor, taps: list):
    """dst[j] = src[j] filtered along rows and columns with taps[j] (an odd number of fp32 taps, at most 31; [1.0] copies), border
    reflect-101; src / dst [n, C, H, W] fp32 on the device, out of place"""
    if not (src.is_cuda and dst.is_cuda):
        raise RuntimeError(f"blur_separable: the blur runs on the device only (HIP, no CPU fallback); got {src.device} / {dst.device} tensors")
    assert src.dim() == 4 and src.is_contiguous() and dst.is_contiguous() and src.shape == dst.shape, (src.shape, dst.shape)
    assert src.dtype == torch.float32 and dst.dtype == torch.float32, (src.dtype, dst.dtype)
    import numpy as np
    n, Cc, H, W = src.shape
    assert len(taps) == n, (len(taps), n)
    ks = np.array([len(t) for t in taps], dtype=np.int32)
    if ks.max() > L.BLUR_MAX_KSIZE or not (ks % 2 == 1).all():
        raise ValueError(f"blur_separable: kernel sizes {sorted(set(ks.tolist()))} (odd, at most {L.BLUR_MAX_KSIZE})")
    tab = np.zeros((n, L.BLUR_MAX_KSIZE), dtype=np.float32)
    for j, t in enumerate(taps):
        tab[j, :len(t)] = t
    for at, m in _chunks(n, L.BLUR_MAX_IMAGES):
        check(lib.unet_blur_separable(_image_ptr(src, at), _image_ptr(dst, at), m, Cc, H, W, ks[at:at + m].ctypes.data_as(C.POINTER(C.c_int)),
                                      tab[at:at + m].ctypes.data_as(L.c_float_p), _stream()), "blur_separable")


def mosaic_accumulate_windows(z: TS, table: torch.Tensor, first: int, n: int, origin, mosaic: torch.Tensor, count: torch.Tensor,
                              row_lo: int, row_hi: int, raw: bool = False):
    """softmax (or, raw=True, the values themselves) of the fp32 NHWC logits of windows [first, first + n) added into mosaic / count"""
    _need_f32("mosaic_accumulate_windows", z)
    Cc, MH, MW = mosaic.shape
    assert z.N >= n and Cc == z.C and count.shape == (MH, MW) and count.dtype == torch.int32 and mosaic.dtype == torch.float32
    check(lib.unet_mosaic_accumulate_windows(z.ptr, z.cs, z.co, z.C, z.H, z.W, table.data_ptr() + 16 * first, n, int(origin[0]),
                                             int(origin[1]), int(raw), mosaic.data_ptr(), count.data_ptr(), MH, MW, int(row_lo), int(row_hi),
                                             _stream()), "mosaic_accumulate_windows")


def mosaic_finalize_rows(mosaic: torch.Tensor, count: torch.Tensor, row0: int, nrows: int, amax: Optional[torch.Tensor], fill=None):
    Cc, MH, MW = mosaic.shape
    assert amax is None or (amax.dtype == torch.uint8 and amax.numel() >= nrows * MW)
    fp = None if fill is None else C.byref(C.c_float(float(fill)))
    check(lib.unet_mosaic_finalize_rows(mosaic.data_ptr(), count.data_ptr(), Cc, MH, MW, row0, nrows, _p(amax),
                                        None if fp is None else C.cast(fp, L.c_float_p), _stream()), "mosaic_finalize_rows")


def mosaic_accumulate_windows_weighted(z: TS, table: torch.Tensor, first: int, n: int, origin, mosaic: torch.Tensor, count: torch.Tensor,
                                       wsum: torch.Tensor, wy: torch.Tensor, wx: torch.Tensor, row_lo: int, row_hi: int, raw: bool = False):
    """mosaic_accumulate_windows with Gaussian blending: every value is added as fl(w * v), w = fl(wy[ty] * wx[tx]) of the window's
    profile tables (fp32, z.H / z.W entries), and w is added to wsum [MH, MW]"""
    _need_f32("mosaic_accumulate_windows_weighted", z)
    Cc, MH, MW = mosaic.shape
    assert z.N >= n and Cc == z.C and count.shape == (MH, MW) and count.dtype == torch.int32 and mosaic.dtype == torch.float32
    assert wsum.shape == (MH, MW) and wsum.dtype == torch.float32
    _blend_tables("mosaic_accumulate_windows_weighted", wy, wx, z.H, z.W)
    check(lib.unet_mosaic_accumulate_windows_weighted(z.ptr, z.cs, z.co, z.C, z.H, z.W, table.data_ptr() + 16 * first, n, int(origin[0]),
                                                      int(origin[1]), int(raw), mosaic.data_ptr(), count.data_ptr(), MH, MW, int(row_lo),
                                                      int(row_hi), wy.data_ptr(), wx.data_ptr(), wsum.data_ptr(), _stream()),
          "mosaic_accumulate_windows_weighted")


def mosaic_finalize_rows_weighted(mosaic: torch.Tensor, count: torch.Tensor, wsum: torch.Tensor, row0: int, nrows: int,
                                  amax: Optional[torch.Tensor], fill=None):
    """mosaic_finalize_rows with the weight sum as divisor (where the hit count is positive)"""
    Cc, MH, MW = mosaic.shape
    assert amax is None or (amax.dtype == torch.uint8 and amax.numel() >= nrows * MW)
    assert wsum.shape == (MH, MW) and wsum.dtype == torch.float32
    fp = None if fill is None else C.byref(C.c_float(float(fill)))
    check(lib.unet_mosaic_finalize_rows_weighted(mosaic.data_ptr(), count.data_ptr(), wsum.data_ptr(), Cc, MH, MW, row0, nrows, _p(amax),
                                                 None if fp is None else C.cast(fp, L.c_float_p), _stream()), "mosaic_finalize_rows_weighted")


# ---------------------------------------------------------------------------------------------- class-mask post-processing (csrc/postprocess.hip)

MASK_MAX_PIXELS = 2 ** 31 - 1


def cc_tile_shape():
    """(rows, columns) of the tile that the labelling kernel holds in LDS"""
    th, tw = C.c_int(0), C.c_int(0)
    lib.unet_cc_tile_shape(C.byref(th), C.byref(tw))
    return th.value, tw.value


def check_mask_shape(what: str, shape):
    """[H, W] with 1 <= H * W <= 2^31 - 1 (labels are int32 linear indices): refused from the shape alone"""
    if len(shape) != 2 or int(shape[0]) < 1 or int(shape[1]) < 1:
        raise ValueError(f"{what}: expected a non-empty [H, W] mask, got shape {tuple(shape)}")
    if int(shape[0]) * int(shape[1]) > MASK_MAX_PIXELS:
        raise ValueError(f"{what}: {int(shape[0])} x {int(shape[1])} px exceeds 2^31 - 1 pixels (labels are int32 linear indices)")


def _pp_tensor(what: str, name: str, t: torch.Tensor, dtype, shape=None, numel=None):
    if shape is not None:
        check_mask_shape(what, shape)
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise ValueError(f"{what}: {name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))}")
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} must live on the GPU, got device {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if numel is not None and t.numel() < numel:
        raise ValueError(f"{what}: {name} holds {t.numel()} elements, needs {numel}")


def _pp_frozen(what: str, frozen) -> int:
    if frozen is None:
        return -1
    if isinstance(frozen, bool) or not isinstance(frozen, int) or not 0 <= frozen <= 255:
        raise ValueError(f"{what}: frozen_class must be None or an int in 0..255, got {frozen!r}")
    return frozen


def _pp_conn(what: str, connectivity) -> int:
    if connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def cc_label(mask: torch.Tensor, connectivity: int, labels: torch.Tensor, counters: torch.Tensor):
    """labels [H, W] int32 = smallest linear index of every pixel's component; counters int32[4] is reset (read it with postprocess_counters)"""
    _pp_tensor("cc_label", "mask", mask, torch.uint8, mask.shape)
    _pp_tensor("cc_label", "labels", labels, torch.int32, mask.shape)
    _pp_tensor("cc_label", "counters", counters, torch.int32, numel=4)
    H, W = mask.shape
    check(lib.unet_cc_label(mask.data_ptr(), H, W, _pp_conn("cc_label", connectivity), labels.data_ptr(), counters.data_ptr(), _stream()), "cc_label")


def cc_sizes(labels: torch.Tensor, sizes: torch.Tensor):
    """sizes [H, W] int32: the pixel count of a component at its root label, 0 elsewhere"""
    _pp_tensor("cc_sizes", "labels", labels, torch.int32, labels.shape)
    _pp_tensor("cc_sizes", "sizes", sizes, torch.int32, labels.shape)
    H, W = labels.shape
    check(lib.unet_cc_sizes(labels.data_ptr(), H, W, sizes.data_ptr(), _stream()), "cc_sizes")


def sieve_round(src: torch.Tensor, dst: Optional[torch.Tensor], connectivity: int, min_pixels: int, frozen_class, labels: torch.Tensor,
                sizes: torch.Tensor, keys: Optional[torch.Tensor], counters: torch.Tensor):
    """one sieve round src -> dst (unet_hip.h); dst None: a counting pass (counters[1] = small components of src)"""
    _pp_tensor("sieve_round", "src", src, torch.uint8, src.shape)
    if dst is not None:
        _pp_tensor("sieve_round", "dst", dst, torch.uint8, src.shape)
        _pp_tensor("sieve_round", "keys", keys, torch.int64, src.shape)
        if dst.data_ptr() == src.data_ptr():
            raise ValueError("sieve_round: src and dst must be different buffers")
    _pp_tensor("sieve_round", "labels", labels, torch.int32, src.shape)
    _pp_tensor("sieve_round", "sizes", sizes, torch.int32, src.shape)
    _pp_tensor("sieve_round", "counters", counters, torch.int32, numel=4)
    if isinstance(min_pixels, bool) or not isinstance(min_pixels, int) or min_pixels < 2:
        raise ValueError(f"sieve_round: min_pixels must be an int >= 2, got {min_pixels!r}")
    H, W = src.shape
    check(lib.unet_sieve_round(src.data_ptr(), _p(dst), H, W, _pp_conn("sieve_round", connectivity), min(min_pixels, 2 ** 62),
                               _pp_frozen("sieve_round", frozen_class), labels.data_ptr(), sizes.data_ptr(), _p(keys if dst is not None else None),
                               counters.data_ptr(), _stream()), "sieve_round")


def majority_filter(src: torch.Tensor, dst: torch.Tensor, k: int, frozen_class=None):
    """dst = k x k majority vote of src (one Jacobi pass; unet_hip.h)"""
    _pp_tensor("majority_filter", "src", src, torch.uint8, src.shape)
    _pp_tensor("majority_filter", "dst", dst, torch.uint8, src.shape)
    if isinstance(k, bool) or not isinstance(k, int) or k < 3 or k > 15 or k % 2 == 0:
        raise ValueError(f"majority_filter: k must be an odd int in 3..15, got {k!r}")
    if dst.data_ptr() == src.data_ptr():
        raise ValueError("majority_filter: src and dst must be different buffers")
    H, W = src.shape
    check(lib.unet_majority_filter(src.data_ptr(), dst.data_ptr(), H, W, k, _pp_frozen("majority_filter", frozen_class), _stream()), "majority_filter")


def postprocess_counters(counters: torch.Tensor):
    """(merged, small not merged) of the last round: the one host read (and stream sync) of a round.  A give-up code of the labelling
    (a find / union loop that ran H * W steps) raises UnetHipError; it is never retried"""
    _pp_tensor("postprocess_counters", "counters", counters, torch.int32, numel=4)
    host = (C.c_int32 * 4)()
    check(lib.unet_postprocess_counters(counters.data_ptr(), host, _stream()), "postprocess_counters")
    return int(host[0]), int(host[1])


# ---------------------------------------------------------------------------------------------- polygon rings (csrc/vectorize.hip)

VEC_MAX_COUNT = 2 ** 31 - 1


def _vec_count(what: str, name: str, v) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= VEC_MAX_COUNT:
        raise ValueError(f"{what}: {name} must be an int in 1..2^31 - 1, got {v!r}")
    return v


def vec_exclude_words(exclude) -> list:
    """class ids 0..255 (an iterable of ints) -> the 256-bit set as 8 words"""
    words = [0] * 8
    for c in exclude:
        if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c <= 255:
            raise ValueError(f"exclude: class ids must be ints in 0..255, got {c!r}")
        words[c >> 5] |= 1 << (c & 31)
    return words


def vec_flags(mask: torch.Tensor, labels: torch.Tensor, exclude, flags: torch.Tensor):
    """flags [H, W] uint8: bit s = side s (N=0 W=1 S=2 E=3) of the pixel is a boundary edge; 0 for the classes in `exclude`"""
    _pp_tensor("vec_flags", "mask", mask, torch.uint8, mask.shape)
    _pp_tensor("vec_flags", "labels", labels, torch.int32, mask.shape)
    _pp_tensor("vec_flags", "flags", flags, torch.uint8, mask.shape)
    H, W = mask.shape
    words = (C.c_uint32 * 8)(*vec_exclude_words(exclude))
    check(lib.unet_vec_flags(mask.data_ptr(), labels.data_ptr(), H, W, words, flags.data_ptr(), _stream()), "vec_flags")


def vec_scan_words(n: int) -> int:
    """int64 words of the block-sum workspace of vec_scan over n bytes; the last one receives the total"""
    return int(lib.unet_vec_scan_words(int(n)))


def vec_scan(src: torch.Tensor, out: torch.Tensor, blocks: torch.Tensor):
    """out (int32, src.numel()) = exclusive scan of popcount(src & 15) over the bytes of src; blocks[vec_scan_words - 1] = the total"""
    n = src.numel() if isinstance(src, torch.Tensor) else 0
    _vec_count("vec_scan", "the element count", n)
    _pp_tensor("vec_scan", "src", src, torch.uint8)
    _pp_tensor("vec_scan", "out", out, torch.int32, numel=n)
    _pp_tensor("vec_scan", "blocks", blocks, torch.int64, numel=vec_scan_words(n))
    check(lib.unet_vec_scan(src.data_ptr(), n, out.data_ptr(), blocks.data_ptr(), _stream()), "vec_scan")


def vec_read(words: torch.Tensor, first: int = 0, count: int = 1) -> list:
    """`count` int64 words of a device tensor from `first` on, as Python ints: one copy and one stream sync"""
    _pp_tensor("vec_read", "words", words, torch.int64, numel=first + count)
    if first < 0 or not 1 <= count <= 64:
        raise ValueError(f"vec_read: first must be >= 0 and count in 1..64, got {first}, {count}")
    host = (C.c_longlong * count)()
    check(lib.unet_vec_read(words.data_ptr() + 8 * first, count, host, _stream()), "vec_read")
    return [int(v) for v in host]


def vec_succ(flags: torch.Tensor, offs: torch.Tensor, E: int, succ: torch.Tensor, corner: torch.Tensor):
    """succ[e] (compact edge indices) and corner[e] = 1 where the walk turns after e"""
    _pp_tensor("vec_succ", "flags", flags, torch.uint8, flags.shape)
    _pp_tensor("vec_succ", "offs", offs, torch.int32, flags.shape)
    _vec_count("vec_succ", "E", E)
    _pp_tensor("vec_succ", "succ", succ, torch.int32, numel=E)
    _pp_tensor("vec_succ", "corner", corner, torch.uint8, numel=E)
    H, W = flags.shape
    check(lib.unet_vec_succ(flags.data_ptr(), offs.data_ptr(), H, W, E, succ.data_ptr(), corner.data_ptr(), _stream()), "vec_succ")


def vec_min_rounds(succ: torch.Tensor, E: int, a, b, init: bool, rounds: int, changed: torch.Tensor):
    """`rounds` doubling rounds of the cycle minimum between the buffer sets a = (m, nxt) and b; the result is in b after an odd count"""
    _vec_count("vec_min_rounds", "E", E)
    _pp_tensor("vec_min_rounds", "succ", succ, torch.int32, numel=E)
    for t in (*a, *b):
        _pp_tensor("vec_min_rounds", "a / b", t, torch.int32, numel=E)
    if isinstance(rounds, bool) or not isinstance(rounds, int) or not 0 <= rounds <= 64:
        raise ValueError(f"vec_min_rounds: rounds must be an int in 0..64, got {rounds!r}")
    _pp_tensor("vec_min_rounds", "changed", changed, torch.int32, numel=max(rounds, 1))
    check(lib.unet_vec_min_rounds(succ.data_ptr(), E, a[0].data_ptr(), a[1].data_ptr(), b[0].data_ptr(), b[1].data_ptr(), int(bool(init)), rounds,
                                  changed.data_ptr(), _stream()), "vec_min_rounds")


def vec_swap(labels: torch.Tensor, flags: torch.Tensor, offs: torch.Tensor, ring: torch.Tensor, succ: torch.Tensor, E: int):
    """exchanges the successors of the two edges that end in a saddle vertex when both lie in one ring"""
    _pp_tensor("vec_swap", "labels", labels, torch.int32, labels.shape)
    _pp_tensor("vec_swap", "flags", flags, torch.uint8, labels.shape)
    _pp_tensor("vec_swap", "offs", offs, torch.int32, labels.shape)
    _vec_count("vec_swap", "E", E)
    _pp_tensor("vec_swap", "ring", ring, torch.int32, numel=E)
    _pp_tensor("vec_swap", "succ", succ, torch.int32, numel=E)
    H, W = labels.shape
    check(lib.unet_vec_swap(labels.data_ptr(), flags.data_ptr(), offs.data_ptr(), H, W, ring.data_ptr(), succ.data_ptr(), _stream()), "vec_swap")


def vec_rank_init(flags: torch.Tensor, offs: torch.Tensor, succ: torch.Tensor, ring: torch.Tensor, E: int, steps: torch.Tensor, nxt: torch.Tensor,
                  area: torch.Tensor, mark: torch.Tensor):
    """the lists of the ranking: every cycle cut at its leader; mark[e] = 1 at leaders"""
    _pp_tensor("vec_rank_init", "flags", flags, torch.uint8, flags.shape)
    _pp_tensor("vec_rank_init", "offs", offs, torch.int32, flags.shape)
    _vec_count("vec_rank_init", "E", E)
    for name, t in (("succ", succ), ("ring", ring), ("steps", steps), ("nxt", nxt)):
        _pp_tensor("vec_rank_init", name, t, torch.int32, numel=E)
    _pp_tensor("vec_rank_init", "area", area, torch.int64, numel=E)
    _pp_tensor("vec_rank_init", "mark", mark, torch.uint8, numel=E)
    H, W = flags.shape
    check(lib.unet_vec_rank_init(flags.data_ptr(), offs.data_ptr(), H, W, succ.data_ptr(), ring.data_ptr(), steps.data_ptr(), nxt.data_ptr(),
                                 area.data_ptr(), mark.data_ptr(), E, _stream()), "vec_rank_init")


def vec_rank_rounds(E: int, a, b, rounds: int, changed: torch.Tensor):
    """`rounds` doubling rounds of the list ranking between the buffer sets a = (steps, nxt, area) and b"""
    _vec_count("vec_rank_rounds", "E", E)
    for s in (a, b):
        _pp_tensor("vec_rank_rounds", "steps", s[0], torch.int32, numel=E)
        _pp_tensor("vec_rank_rounds", "nxt", s[1], torch.int32, numel=E)
        _pp_tensor("vec_rank_rounds", "area", s[2], torch.int64, numel=E)
    if isinstance(rounds, bool) or not isinstance(rounds, int) or not 0 <= rounds <= 64:
        raise ValueError(f"vec_rank_rounds: rounds must be an int in 0..64, got {rounds!r}")
    _pp_tensor("vec_rank_rounds", "changed", changed, torch.int32, numel=max(rounds, 1))
    check(lib.unet_vec_rank_rounds(E, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), rounds,
                                   changed.data_ptr(), _stream()), "vec_rank_rounds")


def vec_ring_info(flags: torch.Tensor, offs: torch.Tensor, labels: torch.Tensor, succ: torch.Tensor, ring: torch.Tensor, ridx: torch.Tensor,
                  steps: torch.Tensor, area: torch.Tensor, E: int, R: int, ring_label: torch.Tensor, ring_len: torch.Tensor, ring_area: torch.Tensor):
    """per ring (index ridx[leader]): label, edge count, signed area"""
    _pp_tensor("vec_ring_info", "flags", flags, torch.uint8, flags.shape)
    _pp_tensor("vec_ring_info", "offs", offs, torch.int32, flags.shape)
    _pp_tensor("vec_ring_info", "labels", labels, torch.int32, flags.shape)
    _vec_count("vec_ring_info", "E", E)
    _vec_count("vec_ring_info", "R", R)
    for name, t in (("succ", succ), ("ring", ring), ("ridx", ridx), ("steps", steps)):
        _pp_tensor("vec_ring_info", name, t, torch.int32, numel=E)
    _pp_tensor("vec_ring_info", "area", area, torch.int64, numel=E)
    _pp_tensor("vec_ring_info", "ring_label", ring_label, torch.int32, numel=R)
    _pp_tensor("vec_ring_info", "ring_len", ring_len, torch.int64, numel=R)
    _pp_tensor("vec_ring_info", "ring_area", ring_area, torch.int64, numel=R)
    H, W = flags.shape
    check(lib.unet_vec_ring_info(flags.data_ptr(), offs.data_ptr(), labels.data_ptr(), H, W, succ.data_ptr(), ring.data_ptr(), ridx.data_ptr(),
                                 steps.data_ptr(), area.data_ptr(), R, ring_label.data_ptr(), ring_len.data_ptr(), ring_area.data_ptr(), _stream()),
          "vec_ring_info")


def vec_place(ring: torch.Tensor, steps: torch.Tensor, ridx: torch.Tensor, ring_base: torch.Tensor, ring_len: torch.Tensor, corner: torch.Tensor,
              E: int, R: int, pos: torch.Tensor, corner_ord: torch.Tensor):
    """pos[e] = the place of edge e in ring order; corner_ord = the corner marks in that order"""
    _vec_count("vec_place", "E", E)
    _vec_count("vec_place", "R", R)
    for name, t in (("ring", ring), ("steps", steps), ("ridx", ridx), ("pos", pos)):
        _pp_tensor("vec_place", name, t, torch.int32, numel=E)
    _pp_tensor("vec_place", "ring_base", ring_base, torch.int64, numel=R)
    _pp_tensor("vec_place", "ring_len", ring_len, torch.int64, numel=R)
    _pp_tensor("vec_place", "corner", corner, torch.uint8, numel=E)
    _pp_tensor("vec_place", "corner_ord", corner_ord, torch.uint8, numel=E)
    check(lib.unet_vec_place(ring.data_ptr(), steps.data_ptr(), ridx.data_ptr(), ring_base.data_ptr(), ring_len.data_ptr(), corner.data_ptr(), E, R,
                             pos.data_ptr(), corner_ord.data_ptr(), _stream()), "vec_place")


def vec_emit(flags: torch.Tensor, offs: torch.Tensor, corner: torch.Tensor, pos: torch.Tensor, voff: torch.Tensor, E: int, V: int, xy: torch.Tensor):
    """xy [V, 2] int32: the end vertex of every corner edge at its vertex index"""
    _pp_tensor("vec_emit", "flags", flags, torch.uint8, flags.shape)
    _pp_tensor("vec_emit", "offs", offs, torch.int32, flags.shape)
    _vec_count("vec_emit", "E", E)
    _vec_count("vec_emit", "V", V)
    _pp_tensor("vec_emit", "corner", corner, torch.uint8, numel=E)
    _pp_tensor("vec_emit", "pos", pos, torch.int32, numel=E)
    _pp_tensor("vec_emit", "voff", voff, torch.int32, numel=E)
    _pp_tensor("vec_emit", "xy", xy, torch.int32, numel=2 * V)
    H, W = flags.shape
    check(lib.unet_vec_emit(flags.data_ptr(), offs.data_ptr(), H, W, corner.data_ptr(), pos.data_ptr(), voff.data_ptr(), E, V, xy.data_ptr(), _stream()),
          "vec_emit")


# ---------------------------------------------------------------------------------------------- ring simplification (csrc/simplify.hip)

SIMP_MAX_Q = 16 * 4096          # the tolerance in sixteenths of a pixel


def _simp_rounds(what: str, rounds, changed: torch.Tensor) -> int:
    if isinstance(rounds, bool) or not isinstance(rounds, int) or not 0 <= rounds <= 64:
        raise ValueError(f"{what}: rounds must be an int in 0..64, got {rounds!r}")
    _pp_tensor(what, "changed", changed, torch.int32, numel=max(rounds, 1))
    return rounds


def simp_marks(labels: torch.Tensor, flags: torch.Tensor, offs: torch.Tensor, corner: torch.Tensor, E: int, cand: torch.Tensor):
    """cand[e] (uint8): bit 0 = the end vertex of edge e is a corner or a node, bit 4 = it is a node (unet_hip.h)"""
    _pp_tensor("simp_marks", "labels", labels, torch.int32, labels.shape)
    _pp_tensor("simp_marks", "flags", flags, torch.uint8, labels.shape)
    _pp_tensor("simp_marks", "offs", offs, torch.int32, labels.shape)
    _vec_count("simp_marks", "E", E)
    _pp_tensor("simp_marks", "corner", corner, torch.uint8, numel=E)
    _pp_tensor("simp_marks", "cand", cand, torch.uint8, numel=E)
    H, W = labels.shape
    check(lib.unet_simp_marks(labels.data_ptr(), flags.data_ptr(), offs.data_ptr(), corner.data_ptr(), H, W, E, cand.data_ptr(), _stream()), "simp_marks")


def simp_gather(ring: torch.Tensor, ridx: torch.Tensor, pos: torch.Tensor, coff: torch.Tensor, cand: torch.Tensor, E: int, R: int, C_: int,
                cring: torch.Tensor, cnode: torch.Tensor):
    """cring[k] / cnode[k] = ring index / node mark of candidate k = coff[pos[e]]"""
    for name, v in (("E", E), ("R", R), ("C", C_)):
        _vec_count("simp_gather", name, v)
    for name, t in (("ring", ring), ("ridx", ridx), ("pos", pos), ("coff", coff)):
        _pp_tensor("simp_gather", name, t, torch.int32, numel=E)
    _pp_tensor("simp_gather", "cand", cand, torch.uint8, numel=E)
    _pp_tensor("simp_gather", "cring", cring, torch.int32, numel=C_)
    _pp_tensor("simp_gather", "cnode", cnode, torch.uint8, numel=C_)
    check(lib.unet_simp_gather(ring.data_ptr(), ridx.data_ptr(), pos.data_ptr(), coff.data_ptr(), cand.data_ptr(), E, R, C_, cring.data_ptr(),
                               cnode.data_ptr(), _stream()), "simp_gather")


def simp_closed(cxy: torch.Tensor, cring: torch.Tensor, cnode: torch.Tensor, cs: torch.Tensor, cn: torch.Tensor, C_: int, R: int, W: int,
                nnodes: torch.Tensor, keys: torch.Tensor, keep: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor):
    """anchors and far points of the rings with fewer than two nodes, then keep / lo / hi (unet_hip.h); keys: int64 [3, R] work words"""
    _vec_count("simp_closed", "C", C_)
    _vec_count("simp_closed", "R", R)
    _vec_count("simp_closed", "W", W)
    _pp_tensor("simp_closed", "cxy", cxy, torch.int32, numel=2 * C_)
    _pp_tensor("simp_closed", "cring", cring, torch.int32, numel=C_)
    _pp_tensor("simp_closed", "cnode", cnode, torch.uint8, numel=C_)
    for name, t in (("cs", cs), ("cn", cn), ("nnodes", nnodes)):
        _pp_tensor("simp_closed", name, t, torch.int32, numel=R)
    _pp_tensor("simp_closed", "keys", keys, torch.int64, numel=3 * R)
    if tuple(keys.shape) != (3, R):
        raise ValueError(f"simp_closed: keys has shape {tuple(keys.shape)}, expected {(3, R)}")
    _pp_tensor("simp_closed", "keep", keep, torch.uint8, numel=C_)
    _pp_tensor("simp_closed", "lo", lo, torch.int32, numel=C_)
    _pp_tensor("simp_closed", "hi", hi, torch.int32, numel=C_)
    check(lib.unet_simp_closed(cxy.data_ptr(), cring.data_ptr(), cnode.data_ptr(), cs.data_ptr(), cn.data_ptr(), C_, R, W, nnodes.data_ptr(),
                               keys[0].data_ptr(), keys[1].data_ptr(), keys[2].data_ptr(), keep.data_ptr(), lo.data_ptr(), hi.data_ptr(), _stream()),
          "simp_closed")


def simp_near_rounds(C_: int, a, b, rounds: int, changed: torch.Tensor):
    """`rounds` doubling rounds of the nearest-kept search between the sets a = (lo, hi) and b; changed[r] = 1 if round r changed a pointer"""
    _vec_count("simp_near_rounds", "C", C_)
    for t in (*a, *b):
        _pp_tensor("simp_near_rounds", "a / b", t, torch.int32, numel=C_)
    _simp_rounds("simp_near_rounds", rounds, changed)
    check(lib.unet_simp_near_rounds(C_, a[0].data_ptr(), a[1].data_ptr(), b[0].data_ptr(), b[1].data_ptr(), rounds, changed.data_ptr(), _stream()),
          "simp_near_rounds")


def simp_dp_rounds(cxy: torch.Tensor, cring: torch.Tensor, cn: torch.Tensor, C_: int, R: int, W: int, q: int, first: bool, rounds: int,
                   keep: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, key: torch.Tensor, slot: torch.Tensor, win: torch.Tensor,
                   changed: torch.Tensor):
    """`rounds` Douglas-Peucker rounds at tolerance q / 16 pixels (unet_hip.h); changed[r] = 1 if round r still had a live segment"""
    _vec_count("simp_dp_rounds", "C", C_)
    _vec_count("simp_dp_rounds", "R", R)
    _vec_count("simp_dp_rounds", "W", W)
    if isinstance(q, bool) or not isinstance(q, int) or not 0 <= q <= SIMP_MAX_Q:
        raise ValueError(f"simp_dp_rounds: q must be an int in 0..{SIMP_MAX_Q}, got {q!r}")
    _pp_tensor("simp_dp_rounds", "cxy", cxy, torch.int32, numel=2 * C_)
    _pp_tensor("simp_dp_rounds", "cn", cn, torch.int32, numel=R)
    _pp_tensor("simp_dp_rounds", "keep", keep, torch.uint8, numel=C_)
    for name, t in (("cring", cring), ("lo", lo), ("hi", hi), ("win", win)):
        _pp_tensor("simp_dp_rounds", name, t, torch.int32, numel=C_)
    for name, t in (("key", key), ("slot", slot)):
        _pp_tensor("simp_dp_rounds", name, t, torch.int64, numel=C_)
    _simp_rounds("simp_dp_rounds", rounds, changed)
    check(lib.unet_simp_dp_rounds(cxy.data_ptr(), cring.data_ptr(), cn.data_ptr(), C_, R, W, q, int(bool(first)), rounds, keep.data_ptr(), lo.data_ptr(),
                                  hi.data_ptr(), key.data_ptr(), slot.data_ptr(), win.data_ptr(), changed.data_ptr(), _stream()), "simp_dp_rounds")


def simp_emit(cxy: torch.Tensor, cring: torch.Tensor, keep: torch.Tensor, koff: torch.Tensor, kstart: torch.Tensor, vbase: torch.Tensor,
              newring: torch.Tensor, C_: int, R: int, V: int, xy: torch.Tensor, vring: torch.Tensor):
    """xy / vring: the kept candidates of the rings with newring[r] >= 0, at vbase[r] + koff[k] - kstart[r]"""
    for name, v in (("C", C_), ("R", R), ("V", V)):
        _vec_count("simp_emit", name, v)
    _pp_tensor("simp_emit", "cxy", cxy, torch.int32, numel=2 * C_)
    _pp_tensor("simp_emit", "keep", keep, torch.uint8, numel=C_)
    for name, t in (("cring", cring), ("koff", koff)):
        _pp_tensor("simp_emit", name, t, torch.int32, numel=C_)
    for name, t in (("kstart", kstart), ("newring", newring)):
        _pp_tensor("simp_emit", name, t, torch.int32, numel=R)
    _pp_tensor("simp_emit", "vbase", vbase, torch.int64, numel=R)
    _pp_tensor("simp_emit", "xy", xy, torch.int32, numel=2 * V)
    _pp_tensor("simp_emit", "vring", vring, torch.int32, numel=V)
    check(lib.unet_simp_emit(cxy.data_ptr(), cring.data_ptr(), keep.data_ptr(), koff.data_ptr(), kstart.data_ptr(), vbase.data_ptr(), newring.data_ptr(),
                             C_, R, V, xy.data_ptr(), vring.data_ptr(), _stream()), "simp_emit")


def simp_area(xy: torch.Tensor, vring: torch.Tensor, ring_start: torch.Tensor, V: int, R: int, area2: torch.Tensor):
    """area2[r] (int64) = twice the signed area of ring r of the result"""
    _vec_count("simp_area", "V", V)
    _vec_count("simp_area", "R", R)
    _pp_tensor("simp_area", "xy", xy, torch.int32, numel=2 * V)
    _pp_tensor("simp_area", "vring", vring, torch.int32, numel=V)
    _pp_tensor("simp_area", "ring_start", ring_start, torch.int64, numel=R + 1)
    _pp_tensor("simp_area", "area2", area2, torch.int64, numel=R)
    check(lib.unet_simp_area(xy.data_ptr(), vring.data_ptr(), ring_start.data_ptr(), V, R, area2.data_ptr(), _stream()), "simp_area")


# ---------------------------------------------------------------------------------------------- instance split (csrc/instances.hip)

INST_MAX_RADIUS = 255
INST_MAX_Q = 16 * 255          # the depth in sixteenths of a pixel


def inst_tile_shapes():
    """((rows, columns) of the row pass's tile, (rows, columns) of the column pass's tile) of inst_distance"""
    v = [C.c_int(0) for _ in range(4)]
    lib.unet_inst_tile_shapes(*(C.byref(x) for x in v))
    return (v[0].value, v[1].value), (v[2].value, v[3].value)


def inst_partials() -> int:
    """int64 words of the `partial` argument of the inst_* launchers: block sums of a count, zero where a block has nothing"""
    return int(lib.unet_inst_partials())


def _inst_int(what: str, name: str, v, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{what}: {name} must be an int in {lo}..{hi}, got {v!r}")
    return v


def cc_label_keys(keys: torch.Tensor, labels: torch.Tensor, counters: torch.Tensor):
    """cc_label at 4-adjacency of an int32 [H, W] key image (equal keys = one component): the flat zones of the instance split"""
    _pp_tensor("cc_label_keys", "keys", keys, torch.int32, keys.shape)
    _pp_tensor("cc_label_keys", "labels", labels, torch.int32, keys.shape)
    _pp_tensor("cc_label_keys", "counters", counters, torch.int32, numel=4)
    H, W = keys.shape
    check(lib.unet_cc_label_keys(keys.data_ptr(), H, W, labels.data_ptr(), counters.data_ptr(), _stream()), "cc_label_keys")


def inst_distance(mask: torch.Tensor, classes, radius: int, g: torch.Tensor, keys: torch.Tensor):
    """keys [H, W] int32 = class << 16 | h, h the capped squared distance to the nearest pixel of another value for the classes in
    `classes` and 0 for the others; g [H, W] uint8 is the workspace of the row pass"""
    _pp_tensor("inst_distance", "mask", mask, torch.uint8, mask.shape)
    _pp_tensor("inst_distance", "g", g, torch.uint8, mask.shape)
    _pp_tensor("inst_distance", "keys", keys, torch.int32, mask.shape)
    _inst_int("inst_distance", "radius", radius, 1, INST_MAX_RADIUS)
    H, W = mask.shape
    words = (C.c_uint32 * 8)(*vec_exclude_words(classes))
    check(lib.unet_inst_distance(mask.data_ptr(), H, W, words, radius, g.data_ptr(), keys.data_ptr(), _stream()), "inst_distance")


def inst_check_labels(mask: torch.Tensor, labels: torch.Tensor, bad: torch.Tensor):
    """bad[0] = 1 unless every labels[p] names a pixel at or before p that names itself and has p's class (read it with vec_read)"""
    _pp_tensor("inst_check_labels", "mask", mask, torch.uint8, mask.shape)
    _pp_tensor("inst_check_labels", "labels", labels, torch.int32, mask.shape)
    _pp_tensor("inst_check_labels", "bad", bad, torch.int64, numel=1)
    H, W = mask.shape
    check(lib.unet_inst_check_labels(mask.data_ptr(), labels.data_ptr(), H, W, bad.data_ptr(), _stream()), "inst_check_labels")


def inst_ascent(keys: torch.Tensor, zone: torch.Tensor, zkey: torch.Tensor, ptr: torch.Tensor, partial: torch.Tensor):
    """ptr[Z] at every zone root Z = the zone of the highest pixel above Z that touches it, or Z (a seed); partial sums to the seeds"""
    _pp_tensor("inst_ascent", "keys", keys, torch.int32, keys.shape)
    _pp_tensor("inst_ascent", "zone", zone, torch.int32, keys.shape)
    _pp_tensor("inst_ascent", "zkey", zkey, torch.int64, keys.shape)
    _pp_tensor("inst_ascent", "ptr", ptr, torch.int32, keys.shape)
    _pp_tensor("inst_ascent", "partial", partial, torch.int64, numel=inst_partials())
    H, W = keys.shape
    check(lib.unet_inst_ascent(keys.data_ptr(), zone.data_ptr(), H, W, zkey.data_ptr(), ptr.data_ptr(), partial.data_ptr(), _stream()), "inst_ascent")


def inst_ptr_rounds(root: torch.Tensor, a: torch.Tensor, b: torch.Tensor, rounds: int, changed: torch.Tensor):
    """`rounds` doubling rounds of the pointers at the roots of `root` between a and b; the result is in b after an odd count"""
    _pp_tensor("inst_ptr_rounds", "root", root, torch.int32, root.shape)
    _pp_tensor("inst_ptr_rounds", "a", a, torch.int32, root.shape)
    _pp_tensor("inst_ptr_rounds", "b", b, torch.int32, root.shape)
    _inst_int("inst_ptr_rounds", "rounds", rounds, 0, 64)
    _pp_tensor("inst_ptr_rounds", "changed", changed, torch.int32, numel=max(rounds, 1))
    check(lib.unet_inst_ptr_rounds(root.data_ptr(), root.numel(), a.data_ptr(), b.data_ptr(), rounds, changed.data_ptr(), _stream()), "inst_ptr_rounds")


def inst_gather(root: torch.Tensor, ptr: torch.Tensor, out: torch.Tensor):
    """out[p] = ptr[root[p]]; out may be root"""
    _pp_tensor("inst_gather", "root", root, torch.int32, root.shape)
    _pp_tensor("inst_gather", "ptr", ptr, torch.int32, root.shape)
    _pp_tensor("inst_gather", "out", out, torch.int32, root.shape)
    check(lib.unet_inst_gather(root.data_ptr(), ptr.data_ptr(), root.numel(), out.data_ptr(), _stream()), "inst_gather")


def inst_merge_round(keys: torch.Tensor, seg: torch.Tensor, q: int, doublings: int, peak: torch.Tensor, best: torch.Tensor, a: torch.Tensor,
                     b: torch.Tensor, changed: torch.Tensor, partial: torch.Tensor):
    """one merge round on seg, in place (unet_hip.h); partial sums to the segments that merged"""
    _pp_tensor("inst_merge_round", "keys", keys, torch.int32, keys.shape)
    for name, t in (("seg", seg), ("peak", peak), ("a", a), ("b", b)):
        _pp_tensor("inst_merge_round", name, t, torch.int32, keys.shape)
    _pp_tensor("inst_merge_round", "best", best, torch.int64, keys.shape)
    _pp_tensor("inst_merge_round", "partial", partial, torch.int64, numel=inst_partials())
    _pp_tensor("inst_merge_round", "changed", changed, torch.int32, numel=32)
    _inst_int("inst_merge_round", "q", q, 0, INST_MAX_Q)
    _inst_int("inst_merge_round", "doublings", doublings, 1, 32)
    H, W = keys.shape
    check(lib.unet_inst_merge_round(keys.data_ptr(), seg.data_ptr(), H, W, q, doublings, peak.data_ptr(), best.data_ptr(), a.data_ptr(), b.data_ptr(),
                                    changed.data_ptr(), partial.data_ptr(), _stream()), "inst_merge_round")


def inst_canonical(seg: torch.Tensor, lowest: torch.Tensor, labels: torch.Tensor, partial: torch.Tensor):
    """labels[p] = the smallest linear index of p's segment; partial sums to the segments"""
    _pp_tensor("inst_canonical", "seg", seg, torch.int32, seg.shape)
    _pp_tensor("inst_canonical", "lowest", lowest, torch.int32, seg.shape)
    _pp_tensor("inst_canonical", "labels", labels, torch.int32, seg.shape)
    _pp_tensor("inst_canonical", "partial", partial, torch.int64, numel=inst_partials())
    check(lib.unet_inst_canonical(seg.data_ptr(), seg.numel(), lowest.data_ptr(), labels.data_ptr(), partial.data_ptr(), _stream()), "inst_canonical")


def inst_marks(mask: torch.Tensor, labels: torch.Tensor, classes, mark: torch.Tensor):
    """mark [H, W] uint8 = 1 at the root pixel (labels[p] == p) of every segment of a class in `classes`"""
    _pp_tensor("inst_marks", "mask", mask, torch.uint8, mask.shape)
    _pp_tensor("inst_marks", "labels", labels, torch.int32, mask.shape)
    _pp_tensor("inst_marks", "mark", mark, torch.uint8, mask.shape)
    words = (C.c_uint32 * 8)(*vec_exclude_words(classes))
    check(lib.unet_inst_marks(mask.data_ptr(), labels.data_ptr(), mask.numel(), words, mark.data_ptr(), _stream()), "inst_marks")


def inst_ids(mask: torch.Tensor, labels: torch.Tensor, offs: torch.Tensor, classes, ids: torch.Tensor):
    """ids [H, W] int32 (read as uint32) = offs[labels[p]] + 1 for the classes in `classes`, 0 for the others"""
    _pp_tensor("inst_ids", "mask", mask, torch.uint8, mask.shape)
    _pp_tensor("inst_ids", "labels", labels, torch.int32, mask.shape)
    _pp_tensor("inst_ids", "offs", offs, torch.int32, mask.shape)
    _pp_tensor("inst_ids", "ids", ids, torch.int32, mask.shape)
    words = (C.c_uint32 * 8)(*vec_exclude_words(classes))
    check(lib.unet_inst_ids(mask.data_ptr(), labels.data_ptr(), offs.data_ptr(), mask.numel(), words, ids.data_ptr(), _stream()), "inst_ids")


# ---------------------------------------------------------------------------------------------- polygon burning (csrc/rasterize.hip)

RAS_MAX_SIDE = 2 ** 20           # H, W < 2^20: row and column fit the 20-bit fields of a crossing's key
RAS_MAX_COORD = 2 ** 29          # |x|, |y| <= 2^21 pixels in 1/256 pixel
RAS_MAX_FEATURES = 2 ** 23       # (feature + 1) << 8 fits the uint32 word of the priority plane
RAS_MAX_CROSSINGS = 2 ** 31


def check_raster_shape(what: str, shape) -> tuple:
    """(H, W) with 1 <= H, W < 2^20: refused from the shape alone"""
    if not isinstance(shape, (tuple, list, torch.Size)) or len(shape) != 2 or any(isinstance(s, bool) or not hasattr(s, "__index__") for s in shape):
        raise ValueError(f"{what}: expected a shape (H, W) of two ints, got {shape!r}")
    H, W = int(shape[0]), int(shape[1])
    if not (1 <= H < RAS_MAX_SIDE and 1 <= W < RAS_MAX_SIDE):
        raise ValueError(f"{what}: H and W must lie in 1..2^20 - 1, got {H} x {W}")
    return H, W


def _ras_tensor(what: str, name: str, t: torch.Tensor, dtype, shape=None, numel=None):
    _pp_tensor(what, name, t, dtype, numel=numel)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")


def _ras_rings(what: str, xy: torch.Tensor, ring_start: torch.Tensor, vring: torch.Tensor, V: int, R: int):
    _vec_count(what, "V", V)
    _vec_count(what, "R", R)
    _ras_tensor(what, "xy", xy, torch.int32, shape=(V, 2))
    _ras_tensor(what, "ring_start", ring_start, torch.int64, shape=(R + 1,))
    _ras_tensor(what, "vring", vring, torch.int32, shape=(V,))


def ras_count(xy: torch.Tensor, ring_start: torch.Tensor, vring: torch.Tensor, V: int, R: int, H: int, counts: torch.Tensor, info: torch.Tensor):
    """counts[i] = the row centres of 0 .. H - 1 that the edge from vertex i to the next vertex of its ring crosses; info (int64[2]) is reset
    and info[1] becomes non-zero if a coordinate lies outside +-2^29 (bit 0) or the ring arrays do not hold a vertex (bit 1)"""
    _ras_rings("ras_count", xy, ring_start, vring, V, R)
    check_raster_shape("ras_count", (H, 1))
    _ras_tensor("ras_count", "counts", counts, torch.int32, numel=V)
    _ras_tensor("ras_count", "info", info, torch.int64, numel=2)
    check(lib.unet_ras_count(xy.data_ptr(), ring_start.data_ptr(), vring.data_ptr(), V, R, H, counts.data_ptr(), info.data_ptr(), _stream()), "ras_count")


def ras_scan_words(n: int) -> int:
    """int64 words of the block-sum workspace of ras_scan over n counts"""
    return int(lib.unet_ras_scan_words(int(n)))


def ras_scan(counts: torch.Tensor, n: int, offs: torch.Tensor, blocks: torch.Tensor, info: torch.Tensor):
    """offs (int64, n) = the exclusive scan of counts (int32, n); info[0] = the total"""
    _vec_count("ras_scan", "n", n)
    _ras_tensor("ras_scan", "counts", counts, torch.int32, numel=n)
    _ras_tensor("ras_scan", "offs", offs, torch.int64, numel=n)
    _ras_tensor("ras_scan", "blocks", blocks, torch.int64, numel=ras_scan_words(n))
    _ras_tensor("ras_scan", "info", info, torch.int64, numel=2)
    check(lib.unet_ras_scan(counts.data_ptr(), n, offs.data_ptr(), blocks.data_ptr(), info.data_ptr(), _stream()), "ras_scan")


def ras_emit(xy: torch.Tensor, ring_start: torch.Tensor, vring: torch.Tensor, ring_feature: torch.Tensor, V: int, R: int, H: int, W: int,
             offs: torch.Tensor, M: int, keys: torch.Tensor):
    """keys[offs[i] + t] = feature << 40 | row << 20 | k of the t-th crossing of edge i (unet_hip.h)"""
    _ras_rings("ras_emit", xy, ring_start, vring, V, R)
    check_raster_shape("ras_emit", (H, W))
    _vec_count("ras_emit", "M", M)
    _ras_tensor("ras_emit", "ring_feature", ring_feature, torch.int32, shape=(R,))
    _ras_tensor("ras_emit", "offs", offs, torch.int64, numel=V)
    _ras_tensor("ras_emit", "keys", keys, torch.int64, shape=(M,))
    check(lib.unet_ras_emit(xy.data_ptr(), ring_start.data_ptr(), vring.data_ptr(), ring_feature.data_ptr(), V, R, H, W, offs.data_ptr(), M,
                            keys.data_ptr(), _stream()), "ras_emit")


def ras_spans(keys: Optional[torch.Tensor], M: int, values: Optional[torch.Tensor], F: int, plane: torch.Tensor, bad: torch.Tensor):
    """zeroes plane (int32 [H, W], read as uint32) and bad (int64[1]); then every pair of the M sorted keys burns (feature + 1) << 8 | value
    into its span by an atomic maximum, and bad counts the pairs that are not one (feature, row).  M = 0 (keys, values None): the resets only"""
    H, W = check_raster_shape("ras_spans", plane.shape if isinstance(plane, torch.Tensor) else ())
    if isinstance(M, bool) or not isinstance(M, int) or not 0 <= M < RAS_MAX_CROSSINGS or M % 2:
        raise ValueError(f"ras_spans: M must be an even int in 0..2^31 - 1, got {M!r}")
    if isinstance(F, bool) or not isinstance(F, int) or not 0 <= F < RAS_MAX_FEATURES or (M and not F):
        raise ValueError(f"ras_spans: F must be an int under 2^23, and at least 1 with crossings, got {F!r}")
    if M:
        _ras_tensor("ras_spans", "keys", keys, torch.int64, shape=(M,))
        _ras_tensor("ras_spans", "values", values, torch.uint8, shape=(F,))
    _ras_tensor("ras_spans", "plane", plane, torch.int32, shape=(H, W))
    _ras_tensor("ras_spans", "bad", bad, torch.int64, numel=1)
    check(lib.unet_ras_spans(_p(keys if M else None), M, _p(values if M else None), F, H, W, plane.data_ptr(), bad.data_ptr(), _stream()), "ras_spans")


def ras_resolve(plane: torch.Tensor, fill: int, keep: bool, out: torch.Tensor):
    """out [H, W] uint8 = plane & 255 where the plane is non-zero; elsewhere what out held (keep) or fill"""
    H, W = check_raster_shape("ras_resolve", plane.shape if isinstance(plane, torch.Tensor) else ())
    _ras_tensor("ras_resolve", "plane", plane, torch.int32, shape=(H, W))
    _ras_tensor("ras_resolve", "out", out, torch.uint8, shape=(H, W))
    if isinstance(fill, bool) or not isinstance(fill, int) or not 0 <= fill <= 255:
        raise ValueError(f"ras_resolve: fill must be an int in 0..255, got {fill!r}")
    check(lib.unet_ras_resolve(plane.data_ptr(), H, W, fill, int(bool(keep)), out.data_ptr(), _stream()), "ras_resolve")


def _table_tensor(what: str, name: str, t, dtype, shape):
    """type, shape and contiguity of one argument: refused for host tensors too (_on_one_device comes behind all of them)"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise ValueError(f"{what}: {name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous")


def _on_one_device(what: str, tensors):
    """every given tensor of [(name, tensor or None), ...] lives on the GPU, and on the first one's"""
    first_name, first = tensors[0]
    for name, t in tensors:
        if t is not None and not t.is_cuda:
            raise ValueError(f"{what}: {name} must live on the GPU, got device {t.device}")
        if t is not None and t.device != first.device:
            raise ValueError(f"{what}: {name} lives on {t.device}, {first_name} on {first.device}")


def ras_resolve_ids(plane: torch.Tensor, ids: torch.Tensor):
    """ids (int32 [H, W]) = the feature that owns each pixel of the priority plane of ras_spans, -1 where there is none"""
    H, W = check_raster_shape("ras_resolve_ids", plane.shape if isinstance(plane, torch.Tensor) else ())
    _table_tensor("ras_resolve_ids", "plane", plane, torch.int32, (H, W))
    _table_tensor("ras_resolve_ids", "ids", ids, torch.int32, (H, W))
    _on_one_device("ras_resolve_ids", [("plane", plane), ("ids", ids)])
    check(lib.unet_ras_resolve_ids(plane.data_ptr(), H, W, ids.data_ptr(), _stream()), "ras_resolve_ids")


# ---------------------------------------------------------------------------------------------- zonal statistics (csrc/zonal.hip)

ZONAL_MAX_CLASSES = 256
ZONAL_MAX_BINS = 2 ** 31         # Z * C < 2^31: a key zone * C + class fits an int32


def zonal_lds_bins() -> int:
    """the largest Z * C that zonal_counts takes in its LDS form (a table of uint32 bins per workgroup); anything larger adds to the
    global tables directly"""
    return int(lib.unet_zonal_lds_bins())


def check_zonal_sizes(what: str, Z, C) -> tuple:
    """(Z, C) with 1 <= Z < 2^23, 1 <= C <= 256 and Z * C < 2^31"""
    for name, v in (("the number of zones", Z), ("the number of classes", C)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{what}: {name} must be an int, got {v!r}")
    if not 1 <= C <= ZONAL_MAX_CLASSES:
        raise ValueError(f"{what}: the number of classes must lie in 1..256, got {C}")
    if Z * C >= ZONAL_MAX_BINS:
        raise ValueError(f"{what}: zones x classes must stay under 2^31, got {Z} x {C}")
    if not 1 <= Z < RAS_MAX_FEATURES:
        raise ValueError(f"{what}: the number of zones must lie in 1..2^23 - 1, got {Z}")
    return Z, C


def zonal_counts(zones: torch.Tensor, mask: torch.Tensor, labels: Optional[torch.Tensor], Z: int, C: int, counts: torch.Tensor,
                 objects: Optional[torch.Tensor], bad: torch.Tensor):
    """counts[z, c] += the pixels with zones == z and mask == c; with labels (int32, labels[p] = the smallest linear index of the object
    of p) objects[z, c] += the anchors labels[p] == p among them.  counts and objects (int64 [Z, C]) are zeroed BY THE CALLER; bad
    (int64[1]) is reset and gains bit 0 for a mask value >= C and bit 1 for a zone outside -1 .. Z - 1 (such pixels are counted nowhere)"""
    what = "zonal_counts"
    H, W = check_raster_shape(what, zones.shape if isinstance(zones, torch.Tensor) else ())
    check_zonal_sizes(what, Z, C)
    if (labels is None) != (objects is None):
        raise ValueError(f"{what}: labels and objects are given together or not at all")
    if labels is not None and H * W > VEC_MAX_COUNT:
        raise ValueError(f"{what}: int32 labels index at most 2^31 - 1 pixels, got {H} x {W}")
    _table_tensor(what, "zones", zones, torch.int32, (H, W))
    _table_tensor(what, "mask", mask, torch.uint8, (H, W))
    _table_tensor(what, "counts", counts, torch.int64, (Z, C))
    _table_tensor(what, "bad", bad, torch.int64, (1,))
    if labels is not None:
        _table_tensor(what, "labels", labels, torch.int32, (H, W))
        _table_tensor(what, "objects", objects, torch.int64, (Z, C))
    _on_one_device(what, [("zones", zones), ("mask", mask), ("labels", labels), ("counts", counts), ("objects", objects), ("bad", bad)])
    check(lib.unet_zonal_counts(zones.data_ptr(), mask.data_ptr(), _p(labels), H, W, Z, C, counts.data_ptr(), _p(objects), bad.data_ptr(),
                                _stream()), what)


# ---------------------------------------------------------------------------------------------- zonal statistics of float planes (csrc/zonal_values.hip)

ZONAL_MIN_SHIFT, ZONAL_MAX_SHIFT = -98, 178         # 30 - E over the frexp exponents E of float32


def check_zonal_values_sizes(what: str, shape, Z) -> tuple:
    """(H, W, Z) with H, W within check_raster_shape, H * W <= 2^31 - 1 (the bound of the sums) and 1 <= Z < 2^23"""
    H, W = check_raster_shape(what, shape)
    if H * W > VEC_MAX_COUNT:
        raise ValueError(f"{what}: the sums are bounded for at most 2^31 - 1 pixels, got {H} x {W}")
    if isinstance(Z, bool) or not isinstance(Z, int):
        raise ValueError(f"{what}: the number of zones must be an int, got {Z!r}")
    if not 1 <= Z < RAS_MAX_FEATURES:
        raise ValueError(f"{what}: the number of zones must lie in 1..2^23 - 1, got {Z}")
    return H, W, Z


def check_zonal_nodata(what: str, nodata) -> tuple:
    """(has_nodata, nodata as the float32 the kernels compare with) of None or a real number"""
    if nodata is None:
        return 0, 0.0
    if isinstance(nodata, bool) or not isinstance(nodata, (int, float)) or nodata != nodata:
        raise ValueError(f"{what}: nodata must be None or a number, got {nodata!r}")
    return 1, float(nodata)


def check_zonal_shift(what: str, shift) -> int:
    if isinstance(shift, bool) or not isinstance(shift, int) or not ZONAL_MIN_SHIFT <= shift <= ZONAL_MAX_SHIFT:
        raise ValueError(f"{what}: shift must be an int in -98..178, got {shift!r}")
    return shift


def zonal_absmax(zones: torch.Tensor, values: torch.Tensor, Z: int, nodata, absmax: torch.Tensor):
    """absmax (int64[1], reset) = the largest bit pattern of |values| over the valid pixels: zone in 0 .. Z - 1, value finite and not nodata"""
    what = "zonal_absmax"
    H, W, Z = check_zonal_values_sizes(what, zones.shape if isinstance(zones, torch.Tensor) else (), Z)
    has, nd = check_zonal_nodata(what, nodata)
    _table_tensor(what, "zones", zones, torch.int32, (H, W))
    _table_tensor(what, "values", values, torch.float32, (H, W))
    _table_tensor(what, "absmax", absmax, torch.int64, (1,))
    _on_one_device(what, [("zones", zones), ("values", values), ("absmax", absmax)])
    check(lib.unet_zonal_absmax(zones.data_ptr(), values.data_ptr(), H, W, Z, has, nd, absmax.data_ptr(), _stream()), what)


def zonal_values(zones: torch.Tensor, values: torch.Tensor, Z: int, nodata, shift: int, sums: torch.Tensor, minmax: torch.Tensor, bad: torch.Tensor):
    """sums (int64 [5, Z]: pixels, valid, sum_q, sq_lo, sq_hi) and minmax (float32 [2, Z]) of the zones under q = rint(double(v) * 2^shift),
    both initialised by the call; bad (int64[1]) is reset and gains bit 1 for a zone outside -1 .. Z - 1 and bit 2 for a valid pixel with
    |q| > 2^30 (unet_hip.h)"""
    what = "zonal_values"
    H, W, Z = check_zonal_values_sizes(what, zones.shape if isinstance(zones, torch.Tensor) else (), Z)
    has, nd = check_zonal_nodata(what, nodata)
    check_zonal_shift(what, shift)
    _table_tensor(what, "zones", zones, torch.int32, (H, W))
    _table_tensor(what, "values", values, torch.float32, (H, W))
    _table_tensor(what, "sums", sums, torch.int64, (5, Z))
    _table_tensor(what, "minmax", minmax, torch.float32, (2, Z))
    _table_tensor(what, "bad", bad, torch.int64, (1,))
    _on_one_device(what, [("zones", zones), ("values", values), ("sums", sums), ("minmax", minmax), ("bad", bad)])
    check(lib.unet_zonal_values(zones.data_ptr(), values.data_ptr(), H, W, Z, has, nd, shift, sums.data_ptr(), minmax.data_ptr(), bad.data_ptr(),
                                _stream()), what)


# ---------------------------------------------------------------------------------------------- object attributes (csrc/objects.hip)

def check_objects_shape(what: str, shape) -> tuple:
    """(H, W) within check_raster_shape and H * W <= 2^31 - 1 (int32 labels index the pixels)"""
    H, W = check_raster_shape(what, shape)
    if H * W > VEC_MAX_COUNT:
        raise ValueError(f"{what}: int32 labels index at most 2^31 - 1 pixels, got {H} x {W}")
    return H, W


def obj_point_packed(H: int, W: int) -> bool:
    """whether obj_point finds the representative pixels of an H x W raster in one pass: (H - 1)^2 + (W - 1)^2 < 2^33, so that the squared
    distance and the 31-bit index share one 64-bit key"""
    return bool(lib.unet_obj_point_packed(int(H), int(W)))


def _obj_planes(what: str, mask, labels, offs) -> tuple:
    H, W = check_objects_shape(what, mask.shape if isinstance(mask, torch.Tensor) else ())
    _table_tensor(what, "mask", mask, torch.uint8, (H, W))
    _table_tensor(what, "labels", labels, torch.int32, (H, W))
    _table_tensor(what, "offs", offs, torch.int32, (H, W))
    return H, W


def _obj_count(what: str, P, n: int, least: int) -> int:
    if isinstance(P, bool) or not isinstance(P, int) or not least <= P <= n:
        raise ValueError(f"{what}: P must be an int in {least}..H * W, got {P!r}")
    return P


def obj_compact(mask: torch.Tensor, mark: torch.Tensor, offs: torch.Tensor, P: int, label: torch.Tensor, cls: torch.Tensor):
    """label[offs[p]] = p and cls[offs[p]] = mask[p] at every p with mark[p] != 0 (mark uint8 [H, W], offs = vec_scan(mark), P its total)"""
    what = "obj_compact"
    H, W = check_objects_shape(what, mask.shape if isinstance(mask, torch.Tensor) else ())
    _obj_count(what, P, H * W, 1)
    _table_tensor(what, "mask", mask, torch.uint8, (H, W))
    _table_tensor(what, "mark", mark, torch.uint8, (H, W))
    _table_tensor(what, "offs", offs, torch.int32, (H, W))
    _table_tensor(what, "label", label, torch.int32, (P,))
    _table_tensor(what, "cls", cls, torch.uint8, (P,))
    _on_one_device(what, [("mask", mask), ("mark", mark), ("offs", offs), ("label", label), ("cls", cls)])
    check(lib.unet_obj_compact(mask.data_ptr(), mark.data_ptr(), offs.data_ptr(), H * W, P, label.data_ptr(), cls.data_ptr(), _stream()), what)


def obj_accumulate(mask: torch.Tensor, labels: torch.Tensor, offs: torch.Tensor, exclude, P: int, sums: Optional[torch.Tensor],
                   bbox: Optional[torch.Tensor], bad: torch.Tensor):
    """sums (int64 [P, 5]: pixels, sum_x, sum_y, edges_v, edges_h) and bbox (int32 [P, 4]: x0, y0, x1, y1 half open) of the P objects whose
    index is offs[anchor], both initialised by the call; bad (int64[1]) is reset and gains bit 0 for a label outside 0 .. H * W - 1, bit 1
    for labels[labels[p]] != labels[p], bit 2 for mask[labels[p]] != mask[p].  P = 0 (sums, bbox None): the check of the input alone"""
    what = "obj_accumulate"
    H, W = _obj_planes(what, mask, labels, offs)
    _obj_count(what, P, H * W, 0)
    _table_tensor(what, "bad", bad, torch.int64, (1,))
    if P:
        _table_tensor(what, "sums", sums, torch.int64, (P, 5))
        _table_tensor(what, "bbox", bbox, torch.int32, (P, 4))
    elif sums is not None or bbox is not None:
        raise ValueError(f"{what}: no tables without objects")
    _on_one_device(what, [("mask", mask), ("labels", labels), ("offs", offs), ("sums", sums), ("bbox", bbox), ("bad", bad)])
    words = (C.c_uint32 * 8)(*vec_exclude_words(exclude))
    check(lib.unet_obj_accumulate(mask.data_ptr(), labels.data_ptr(), offs.data_ptr(), H, W, words, P, _p(sums), _p(bbox), bad.data_ptr(),
                                  _stream()), what)


def obj_point(mask: torch.Tensor, labels: torch.Tensor, offs: torch.Tensor, exclude, P: int, sums: torch.Tensor, bad: torch.Tensor,
              key64: torch.Tensor, point: torch.Tensor):
    """point (int32 [P]) = the representative pixel of every object from the complete sums of obj_accumulate; bad: the word of that call on
    the same planes (it made the check of the input: with a bit set nothing is done); key64 (int64 [P]) is workspace"""
    what = "obj_point"
    H, W = _obj_planes(what, mask, labels, offs)
    _obj_count(what, P, H * W, 1)
    _table_tensor(what, "sums", sums, torch.int64, (P, 5))
    _table_tensor(what, "bad", bad, torch.int64, (1,))
    _table_tensor(what, "key64", key64, torch.int64, (P,))
    _table_tensor(what, "point", point, torch.int32, (P,))
    _on_one_device(what, [("mask", mask), ("labels", labels), ("offs", offs), ("sums", sums), ("bad", bad), ("key64", key64), ("point", point)])
    words = (C.c_uint32 * 8)(*vec_exclude_words(exclude))
    check(lib.unet_obj_point(mask.data_ptr(), labels.data_ptr(), offs.data_ptr(), H, W, words, P, sums.data_ptr(), bad.data_ptr(),
                             key64.data_ptr(), point.data_ptr(), _stream()), what)


# ---------------------------------------------------------------------------------------------- float statistics per object (csrc/object_values.hip)

def obj_absmax(mask: torch.Tensor, values: torch.Tensor, exclude, nodata, absmax: torch.Tensor):
    """absmax (int64[1], reset) = the largest bit pattern of |values| over the valid pixels: class not excluded, value finite and not nodata"""
    what = "obj_absmax"
    H, W = check_objects_shape(what, mask.shape if isinstance(mask, torch.Tensor) else ())
    has, nd = check_zonal_nodata(what, nodata)
    _table_tensor(what, "mask", mask, torch.uint8, (H, W))
    _table_tensor(what, "values", values, torch.float32, (H, W))
    _table_tensor(what, "absmax", absmax, torch.int64, (1,))
    _on_one_device(what, [("mask", mask), ("values", values), ("absmax", absmax)])
    words = (C.c_uint32 * 8)(*vec_exclude_words(exclude))
    check(lib.unet_obj_absmax(mask.data_ptr(), values.data_ptr(), H, W, words, has, nd, absmax.data_ptr(), _stream()), what)


def obj_values(mask: torch.Tensor, labels: torch.Tensor, values: torch.Tensor, offs: torch.Tensor, exclude, P: int, nodata, shift: int,
               table: Optional[torch.Tensor], bad: torch.Tensor):
    """table (int64 [6, P], initialised by the call): valid, sum_q, sq_lo, sq_hi of the P objects whose index is offs[anchor] under
    q = rint(double(v) * 2^shift), then min and max as one word each: the float32 bits in the low half, the int32 linear index of the first
    pixel that attains it in the high half (+inf / -inf and -1 without a valid pixel).  bad (int64[1]) is reset and gains the three bits of
    obj_accumulate and bit 3 for a valid pixel with |q| > 2^30 (unet_hip.h).  P = 0 (table None): the check of the input alone"""
    what = "obj_values"
    H, W = _obj_planes(what, mask, labels, offs)
    _obj_count(what, P, H * W, 0)
    has, nd = check_zonal_nodata(what, nodata)
    check_zonal_shift(what, shift)
    _table_tensor(what, "values", values, torch.float32, (H, W))
    _table_tensor(what, "bad", bad, torch.int64, (1,))
    if P:
        _table_tensor(what, "table", table, torch.int64, (6, P))
    elif table is not None:
        raise ValueError(f"{what}: no table without objects")
    _on_one_device(what, [("mask", mask), ("labels", labels), ("values", values), ("offs", offs), ("table", table), ("bad", bad)])
    words = (C.c_uint32 * 8)(*vec_exclude_words(exclude))
    check(lib.unet_obj_values(mask.data_ptr(), labels.data_ptr(), values.data_ptr(), offs.data_ptr(), H, W, words, P, has, nd, shift, _p(table),
                              bad.data_ptr(), _stream()), what)


# ---------------------------------------------------------------------------------------------- GeoTIFF strips on the device (csrc/tiff_encode.hip)

def tiff_lzw_cap(n: int) -> int:
    """bytes that always hold the LZW stream of an n-byte strip"""
    return int(lib.unet_tiff_lzw_cap(int(n)))


def tiff_slot_bytes(strip_bytes: int) -> int:
    """the slot of one strip in the scratch of tiff_encode_strips: its capacity rounded up to 16 bytes"""
    return -(-tiff_lzw_cap(strip_bytes) // 16) * 16


def tiff_encode_strips(img: torch.Tensor, rows_per_strip: int, predictor: int, first: int, count: int, scratch: torch.Tensor,
                       sizes: torch.Tensor):
    """LZW-encodes strips [first, first + count) of img [P, H, W] (1-, 2- or 4-byte samples; any row / plane stride, unit column stride)
    into scratch (uint8, count slots of tiff_slot_bytes) and their byte counts into sizes (int32 [count], read as unsigned)"""
    what = "tiff_encode_strips"
    if not isinstance(img, torch.Tensor) or not img.is_cuda or img.dim() != 3 or img.element_size() not in (1, 2, 4) or img.is_complex():
        raise ValueError(f"{what}: img must be a [P, H, W] GPU tensor of 1-, 2- or 4-byte samples")
    P, H, W = (int(v) for v in img.shape)
    if min(P, H, W) < 1 or img.stride(2) != 1 or img.stride(1) < W or (P > 1 and img.stride(0) < 1):
        raise ValueError(f"{what}: img {tuple(img.shape)} with strides {img.stride()} needs contiguous rows and positive strides")
    es = img.element_size()
    if isinstance(rows_per_strip, bool) or not isinstance(rows_per_strip, int) or not 1 <= rows_per_strip <= H or rows_per_strip * W * es > 2 ** 31 - 1:
        raise ValueError(f"{what}: rows_per_strip must be an int in 1..{H} with a strip below 2^31 bytes, got {rows_per_strip!r}")
    if predictor not in (1, 2) or (predictor == 2 and img.dtype.is_floating_point):
        raise ValueError(f"{what}: predictor must be 1, or 2 on integer samples (got {predictor!r} on {img.dtype})")
    total = P * -(-H // rows_per_strip)
    if not (0 <= first and 1 <= count and first + count <= total):
        raise ValueError(f"{what}: strips [{first}, {first + count}) of {total}")
    slot = tiff_slot_bytes(rows_per_strip * W * es)
    _pp_tensor(what, "scratch", scratch, torch.uint8)
    _pp_tensor(what, "sizes", sizes, torch.int32)
    if scratch.numel() < count * slot or sizes.numel() < count or scratch.device != img.device or sizes.device != img.device:
        raise ValueError(f"{what}: needs {count * slot} scratch bytes and {count} sizes on the image's device")
    check(lib.unet_tiff_encode_strips(img.data_ptr(), es, P, H, W, img.stride(1), img.stride(0) if P > 1 else H * img.stride(1), rows_per_strip,
                                      predictor, first, count, scratch.data_ptr(), slot, sizes.data_ptr(), _stream()), what)
    return slot


def tiff_compact_strips(scratch: torch.Tensor, slot: int, sizes: torch.Tensor, offsets: torch.Tensor, count: int, out: torch.Tensor):
    """out[offsets[j] : offsets[j] + sizes[j]] = slot j of scratch; offsets int64 [count] = exclusive prefix sum of sizes"""
    what = "tiff_compact_strips"
    _pp_tensor(what, "scratch", scratch, torch.uint8)
    _pp_tensor(what, "sizes", sizes, torch.int32)
    _pp_tensor(what, "offsets", offsets, torch.int64)
    _pp_tensor(what, "out", out, torch.uint8)
    if count < 1 or slot < 4 or scratch.numel() < count * slot or sizes.numel() < count or offsets.numel() < count:
        raise ValueError(f"{what}: {count} slots of {slot} bytes do not fit the buffers")
    if any(t.device != scratch.device for t in (sizes, offsets, out)):
        raise ValueError(f"{what}: all buffers must live on one device")
    check(lib.unet_tiff_compact_strips(scratch.data_ptr(), slot, sizes.data_ptr(), offsets.data_ptr(), count, out.data_ptr(), out.numel(),
                                       _stream()), what)


def tiff_encode_tiles(img, tile: int, predictor: int, first: int, count: int, scratch: torch.Tensor, sizes: torch.Tensor):
    """LZW-encodes tiles [first, first + count) of img [P, H, W] (as tiff_encode_strips takes it) in TIFF tile order -- plane-major, tile
    rows, tile columns; samples beyond the right / bottom edge are zero -- into scratch (uint8, count slots of
    tiff_slot_bytes(tile * tile * element size)) and their byte counts into sizes (int32 [count], read as unsigned).
    img may be a list of such images of one dtype and plane count (the levels of a pyramid): the tiles are then numbered through the
    list, one image after the other, and one launch encodes tiles of several images."""
    what = "tiff_encode_tiles"
    imgs = list(img) if isinstance(img, (list, tuple)) else [img]
    if not 1 <= len(imgs) <= L.TIFF_MAX_LEVELS:
        raise ValueError(f"{what}: 1..{L.TIFF_MAX_LEVELS} images, got {len(imgs)}")
    if isinstance(tile, bool) or not isinstance(tile, int) or not 16 <= tile <= 1024 or tile % 16:
        raise ValueError(f"{what}: tile must be a multiple of 16 in 16..1024, got {tile!r}")
    table, total = (L.TiffLevel * len(imgs))(), 0
    for k, t in enumerate(imgs):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 3 or t.element_size() not in (1, 2, 4) or t.is_complex():
            raise ValueError(f"{what}: img must be a [P, H, W] GPU tensor of 1-, 2- or 4-byte samples")
        P, H, W = (int(v) for v in t.shape)
        if min(P, H, W) < 1 or t.stride(2) != 1 or t.stride(1) < W or (P > 1 and t.stride(0) < 1):
            raise ValueError(f"{what}: img {tuple(t.shape)} with strides {t.stride()}: rows must be contiguous and the strides positive")
        if t.dtype != imgs[0].dtype or P != imgs[0].shape[0] or t.device != imgs[0].device:
            raise ValueError(f"{what}: the images must share dtype, plane count and device")
        table[k] = L.TiffLevel(t.data_ptr(), t.stride(1), t.stride(0) if P > 1 else H * t.stride(1), H, W)
        total += P * -(-H // tile) * -(-W // tile)
    t0 = imgs[0]
    es = t0.element_size()
    if predictor not in (1, 2) or (predictor == 2 and t0.dtype.is_floating_point):
        raise ValueError(f"{what}: predictor must be 1, or 2 on integer samples (got {predictor!r} on {t0.dtype})")
    if not (0 <= first and 1 <= count and first + count <= total):
        raise ValueError(f"{what}: tiles [{first}, {first + count}) of {total}")
    slot = tiff_slot_bytes(tile * tile * es)
    _pp_tensor(what, "scratch", scratch, torch.uint8)
    _pp_tensor(what, "sizes", sizes, torch.int32)
    if scratch.numel() < count * slot or sizes.numel() < count or scratch.device != t0.device or sizes.device != t0.device:
        raise ValueError(f"{what}: scratch needs {count * slot} bytes and sizes {count} entries on {t0.device}")
    check(lib.unet_tiff_encode_tile_levels(table, len(imgs), es, int(t0.shape[0]), tile, predictor, first, count, scratch.data_ptr(), slot,
                                           sizes.data_ptr(), _stream()), what)
    return slot


TIFF_RESAMPLINGS = {"nearest": 0, "mode": 1, "average": 2}


def tiff_reduce_level(img: torch.Tensor, resampling: str, nodata, out: torch.Tensor):
    """out [P, ceil(H / 2), ceil(W / 2)] (contiguous, img's dtype) = the next overview level of img [P, H, W] (as tiff_encode_strips takes
    it) by the pyramid rule of unet_amd/tiffenc.py.  nodata: None, or the value whose samples do not count (NaN for float samples: NaN
    samples); a value no sample of an integer type can equal leaves every sample valid."""
    what = "tiff_reduce_level"
    kinds = {torch.uint8: 0, torch.uint16: 0, torch.int8: 1, torch.int16: 1, torch.int32: 1, torch.float32: 2}
    if not isinstance(img, torch.Tensor) or not img.is_cuda or img.dim() != 3 or img.dtype not in kinds:
        raise ValueError(f"{what}: img must be a [P, H, W] GPU tensor of 8 / 16 / 32-bit integers or float32")
    P, H, W = (int(v) for v in img.shape)
    if min(P, H, W) < 1 or max(H, W) < 2 or img.stride(2) != 1 or img.stride(1) < W or (P > 1 and img.stride(0) < 1):
        raise ValueError(f"{what}: img {tuple(img.shape)} with strides {img.stride()}: larger than 1 x 1, rows contiguous, strides positive")
    if resampling not in TIFF_RESAMPLINGS or (resampling == "mode" and img.dtype.is_floating_point):
        raise ValueError(f"{what}: resampling must be 'nearest', 'average' or (integer samples) 'mode', got {resampling!r} on {img.dtype}")
    h, w = -(-H // 2), -(-W // 2)
    _pp_tensor(what, "out", out, img.dtype, numel=P * h * w)
    if tuple(out.shape) != (P, h, w) or out.device != img.device:
        raise ValueError(f"{what}: out must be [{P}, {h}, {w}] on {img.device}, got {tuple(out.shape)} on {out.device}")
    has, nd = 0, 0.0
    if nodata is not None:
        nd = float(nodata)
        if img.dtype.is_floating_point:
            has = 1
        else:
            info = torch.iinfo(img.dtype)
            has = int(nd == nd and nd == int(nd) and info.min <= int(nd) <= info.max)
    check(lib.unet_tiff_reduce_level(img.data_ptr(), img.element_size(), kinds[img.dtype], P, H, W, img.stride(1),
                                     img.stride(0) if P > 1 else H * img.stride(1), TIFF_RESAMPLINGS[resampling], has, nd if has else 0.0,
                                     out.data_ptr(), _stream()), what)
    return out


# ---------------------------------------------------------------------------------------------- border distance and weight map (csrc/edt.hip)

EDT_MAX_SIDE = 8192          # 2 * 8191^2 < 2^31: the squared distance fits int32
EDT_NO_BORDER = 2 ** 31 - 1  # the squared distance of every pixel of an image without a border


def check_edt_shape(what: str, shape):
    """[B, H, W] with B >= 1 and 1 <= H, W <= 8192: refused from the shape alone"""
    if len(shape) != 3 or any(int(v) < 1 for v in shape):
        raise ValueError(f"{what}: expected a non-empty [B, H, W] batch of masks, got shape {tuple(shape)}")
    if int(shape[1]) > EDT_MAX_SIDE or int(shape[2]) > EDT_MAX_SIDE:
        raise ValueError(f"{what}: {int(shape[1])} x {int(shape[2])} px exceeds {EDT_MAX_SIDE} px a side (the squared distance is int32)")
    if int(shape[0]) > 65535:
        raise ValueError(f"{what}: at most 65535 masks per call, got {int(shape[0])}")


def _edt_exclude(what: str, exclude) -> int:
    if exclude is None:
        return -1
    if isinstance(exclude, bool) or not isinstance(exclude, int) or not 0 <= exclude < 2 ** 31:
        raise ValueError(f"{what}: exclude must be None or a class id >= 0, got {exclude!r}")
    return exclude


def edt_workspace(B: int, H: int, W: int) -> int:
    """bytes of the intermediate of border_edt"""
    check_edt_shape("edt_workspace", (B, H, W))
    return int(lib.unet_edt_workspace(B, H, W))


def border_edt(mask: torch.Tensor, d2: torch.Tensor, ws: torch.Tensor, exclude=None):
    """d2 int32 [B, H, W] = squared Euclidean distance to the nearest border pixel of the same image (EDT_NO_BORDER where an image has
    none); mask uint8 or int64 [B, H, W]; ws: any tensor of at least edt_workspace(B, H, W) bytes (unet_hip.h has the rules)"""
    check_edt_shape("border_edt", getattr(mask, "shape", ()))
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"border_edt: mask must be a uint8 or int64 tensor, got {getattr(mask, 'dtype', type(mask))}")
    if not mask.is_cuda or not mask.is_contiguous():
        raise ValueError("border_edt: mask must be a contiguous tensor on the GPU")
    _pp_tensor("border_edt", "d2", d2, torch.int32)
    if tuple(d2.shape) != tuple(mask.shape) and d2.numel() != mask.numel():
        raise ValueError(f"border_edt: d2 holds {d2.numel()} elements, the masks {mask.numel()}")
    B, H, W = (int(v) for v in mask.shape)
    need = edt_workspace(B, H, W)
    if not isinstance(ws, torch.Tensor) or not ws.is_cuda or not ws.is_contiguous() or ws.numel() * ws.element_size() < need:
        raise ValueError(f"border_edt: the workspace must be a contiguous GPU tensor of at least {need} bytes")
    if d2.device != mask.device or ws.device != mask.device:
        raise ValueError("border_edt: mask, d2 and the workspace must live on one device")
    check(lib.unet_border_edt(mask.data_ptr(), int(mask.dtype == torch.int64), B, H, W, _edt_exclude("border_edt", exclude), d2.data_ptr(),
                              ws.data_ptr(), _stream()), "border_edt")


def border_weight(d2: torch.Tensor, target: torch.Tensor, class_w, n_classes: int, w0: float, sigma: float, pw: torch.Tensor):
    """pw float32 [P] = class_w[y] + w0 * exp(-d2 / (2 sigma^2)); class_w float32 [n_classes] or None (ones); a target outside
    [0, n_classes) gives 0, d2 == EDT_NO_BORDER a border term of exactly 0"""
    if not w0 >= 0 or not sigma > 0:
        raise ValueError(f"border_weight: needs w0 >= 0 and sigma > 0, got {w0!r} and {sigma!r}")
    if isinstance(n_classes, bool) or not isinstance(n_classes, int) or n_classes < 1:
        raise ValueError(f"border_weight: n_classes must be an int >= 1, got {n_classes!r}")
    _pp_tensor("border_weight", "d2", d2, torch.int32)
    P = d2.numel()
    _pp_tensor("border_weight", "target", target, torch.int64)
    _pp_tensor("border_weight", "pw", pw, torch.float32)
    if P < 1 or target.numel() != P or pw.numel() != P:
        raise ValueError(f"border_weight: d2, target and pw must hold the same number of pixels, got {P}, {target.numel()}, {pw.numel()}")
    if class_w is not None:
        _pp_tensor("border_weight", "class_w", class_w, torch.float32, numel=n_classes)
    if any(t is not None and t.device != d2.device for t in (target, pw, class_w)):
        raise ValueError("border_weight: every tensor must live on one device")
    check(lib.unet_border_weight(d2.data_ptr(), target.data_ptr(), _p(class_w), n_classes, float(w0), float(sigma), P, pw.data_ptr(), _stream()),
          "border_weight")


# ---------------------------------------------------------------------------------------------- two nearest objects (csrc/object_edt.hip)

OBJ_MAX_RADIUS = 255
OBJ_MAX_CLASSES = 256        # an object's value is one byte of its key
OBJ_NO_OBJECT = 2 ** 31 - 1  # D1 / D2 where no object lies within the radius, and off the background


def check_object_shape(what: str, shape):
    """check_edt_shape and B * H * W <= 2^31 - 1 (a label is a linear index of the stacked batch)"""
    check_edt_shape(what, shape)
    if int(shape[0]) * int(shape[1]) * int(shape[2]) > 2 ** 31 - 1:
        raise ValueError(f"{what}: {tuple(int(v) for v in shape)} holds more than 2^31 - 1 pixels")


def _obj_int(what: str, name: str, v, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{what}: {name} must be an int in {lo}..{hi}, got {v!r}")
    return v


def object_edt_workspace(B: int, H: int, W: int) -> int:
    """bytes of the workspace of object_edt / object_border_weight: keys, labels and two candidates per pixel, 18 bytes per pixel"""
    check_object_shape("object_edt_workspace", (B, H, W))
    return int(lib.unet_object_edt_workspace(B, H, W))


def _object_call(what: str, mask, ws, background, exclude, n_classes, radius, d1, d2, class_w, w0, sigma, pw):
    check_object_shape(what, getattr(mask, "shape", ()))
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"{what}: mask must be a uint8 or int64 tensor, got {getattr(mask, 'dtype', type(mask))}")
    if not mask.is_cuda or not mask.is_contiguous():
        raise ValueError(f"{what}: mask must be a contiguous tensor on the GPU")
    _obj_int(what, "n_classes", n_classes, 1, OBJ_MAX_CLASSES)
    _obj_int(what, "background", background, 0, 255)
    _obj_int(what, "radius", radius, 1, OBJ_MAX_RADIUS)
    excl = _edt_exclude(what, exclude)
    if excl == background:
        raise ValueError(f"{what}: exclude and background are both {background}")
    B, H, W = (int(v) for v in mask.shape)
    need = object_edt_workspace(B, H, W)
    if not isinstance(ws, torch.Tensor) or not ws.is_cuda or not ws.is_contiguous() or ws.numel() * ws.element_size() < need or ws.data_ptr() % 16:
        raise ValueError(f"{what}: the workspace must be a contiguous, 16-byte aligned GPU tensor of at least {need} bytes")
    for name, t, dt in (("d1", d1, torch.int32), ("d2", d2, torch.int32), ("pw", pw, torch.float32)):
        if t is not None:
            _pp_tensor(what, name, t, dt)
            if t.numel() != mask.numel():
                raise ValueError(f"{what}: {name} holds {t.numel()} elements, the masks {mask.numel()}")
    if class_w is not None:
        _pp_tensor(what, "class_w", class_w, torch.float32, numel=n_classes)
    if any(t is not None and t.device != mask.device for t in (ws, d1, d2, pw, class_w)):
        raise ValueError(f"{what}: every tensor must live on one device")
    check(lib.unet_object_edt(mask.data_ptr(), int(mask.dtype == torch.int64), B, H, W, background, excl, n_classes, radius, ws.data_ptr(),
                              _p(d1), _p(d2), _p(class_w), float(w0), float(sigma), _p(pw), _stream()), what)


def object_edt(mask: torch.Tensor, d1: torch.Tensor, d2: torch.Tensor, ws: torch.Tensor, background: int = 0, exclude=None,
               n_classes: int = OBJ_MAX_CLASSES, radius: int = 30):
    """d1, d2 int32 [B, H, W] = for a background pixel the squared Euclidean distances to the nearest and the second nearest distinct
    object of its image within `radius`, OBJ_NO_OBJECT where there is none and off the background; mask uint8 or int64 [B, H, W]; ws: a
    16-byte aligned tensor of at least object_edt_workspace(B, H, W) bytes (unet_hip.h has the rules).  No host sync."""
    if d1 is None or d2 is None:
        raise ValueError("object_edt: d1 and d2 must be int32 tensors")
    _object_call("object_edt", mask, ws, background, exclude, n_classes, radius, d1, d2, None, 0.0, 1.0, None)


def object_border_weight(mask: torch.Tensor, class_w, n_classes: int, w0: float, sigma: float, pw: torch.Tensor, ws: torch.Tensor,
                         background: int = 0, exclude=None, radius: int = 30):
    """pw float32 [B, H, W] = class_w[y] + w0 * exp(-(sqrt D1 + sqrt D2)^2 / (2 sigma^2)) with D1, D2 of object_edt; class_w float32 [n_classes]
    or None (ones); a value outside [0, n_classes) gives 0, D2 == OBJ_NO_OBJECT a second term of exactly 0.  The same launches as
    object_edt: the row pass writes the map instead of the distances.  No host sync."""
    if not w0 >= 0 or not sigma > 0:
        raise ValueError(f"object_border_weight: needs w0 >= 0 and sigma > 0, got {w0!r} and {sigma!r}")
    if pw is None:
        raise ValueError("object_border_weight: pw must be a float32 tensor")
    _object_call("object_border_weight", mask, ws, background, exclude, n_classes, radius, None, None, class_w, w0, sigma, pw)
