"""ctypes binding of libunet_hip.so (the C ABI declared in include/unet_hip.h).

The header is the one place where a signature or a constant is written: unet_amd/_abi.py reads the prototypes, the #defines and the
enums from it at import.  Only the struct mirrors are written here; tests/test_abi_cpu.py has the C compiler check their layout.

The product path has NO fallback: if the HIP library is missing or does not
export a declared symbol, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import torch  # noqa: F401  -- FIRST: torch ships its own libamdhip64; loading libunet_hip.so before it binds /opt/rocm's copy and the process ends
#                    up with two HIP runtimes (the second one reports "no ROCm-capable device": seen with build() + smoke() in one process)

from ._abi import constants, signatures

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "lib" / "libunet_hip.so"
HEADER = _HERE.parent / "include" / "unet_hip.h"

_K = constants(HEADER)
UNET_OK = _K["UNET_OK"]
globals().update((k[len("UNET_"):], v) for k, v in _K.items())          # F32, BF16, CONV_*, PIXEL_*, BLUR_*, FIELD_*, ELASTIC_*, TIFF_MAX_LEVELS, ...

c_float_p = C.POINTER(C.c_float)
vp = C.c_void_p


class Tuning(C.Structure):
    """unet_tuning: the kernel-selection switches of one launch (include/unet_hip.h).  Start from Tuning.default()."""
    _fields_ = [(n, C.c_int) for n in ("conv_splitk", "mfma_shape", "f32_big_tile", "bf16_big_tile", "t256_tiles_per_wg", "t256_sliver",
                                       "conv1x1_gemm", "wgrad_mfma_shape", "wgrad_bf16_k4", "wgrad_1x1", "wgrad_narrow", "plan_batch", "wgrad_wgs", "conv_smallcin", "conv_head1x1")]

    @classmethod
    def default(cls, **over) -> "Tuning":
        t = cls()
        lib.unet_tuning_default(C.byref(t))
        for k, v in over.items():
            if k not in dict(cls._fields_):
                raise KeyError(f"unet_tuning has no field {k!r}")
            setattr(t, k, int(v))
        return t


class ConvDesc(C.Structure):
    _fields_ = [
        ("x", vp), ("x_cs", C.c_int), ("x_co", C.c_int),
        ("wp", vp),
        ("bias", vp),
        ("res", vp), ("res_cs", C.c_int), ("res_co", C.c_int),
        ("mask", vp), ("mask_cs", C.c_int), ("mask_co", C.c_int),
        ("y", vp), ("y_cs", C.c_int), ("y_co", C.c_int),
        ("N", C.c_int), ("IH", C.c_int), ("IW", C.c_int), ("Cin", C.c_int),
        ("OH", C.c_int), ("OW", C.c_int), ("Cout", C.c_int),
        ("ks", C.c_int), ("stride", C.c_int),
        ("kind", C.c_int), ("flags", C.c_int),
        ("colsum", vp),
        ("colsumsq", vp),
        ("cout_begin", C.c_int), ("cout_count", C.c_int),
        ("wp_img_stride", C.c_longlong),
        ("dtype", C.c_int), ("y_f32", C.c_int),
        ("splitk_ws", vp), ("splitk_ws_floats", C.c_size_t),
        ("tuning", C.POINTER(Tuning)),
        ("pixel_shuffle", C.c_int),
        ("ps_tail", vp), ("ps_tail_cs", C.c_int), ("ps_tail_co", C.c_int), ("ps_tail_c", C.c_int), ("ps_tail_at", C.c_int),
    ]


class WgradDesc(C.Structure):
    _fields_ = [
        ("x", vp), ("x_cs", C.c_int), ("x_co", C.c_int),
        ("dy", vp), ("dy_cs", C.c_int), ("dy_co", C.c_int),
        ("dw", vp),
        ("dbias", vp),
        ("N", C.c_int), ("IH", C.c_int), ("IW", C.c_int), ("Cin", C.c_int),
        ("OH", C.c_int), ("OW", C.c_int), ("Cout", C.c_int), ("ks", C.c_int), ("stride", C.c_int),
        ("workspace", vp), ("workspace_floats", C.c_size_t),
        ("accumulate", C.c_int),
        ("dtype", C.c_int),
        ("tuning", C.POINTER(Tuning)),
    ]


class PixelOp(C.Structure):
    _fields_ = [("code", C.c_uint32), ("u0", C.c_uint32), ("u1", C.c_uint32), ("f0", C.c_float), ("f1", C.c_float)]


class PixelProg(C.Structure):
    """unet_pixel_prog: the pointwise program of one image (include/unet_hip.h)"""
    _fields_ = [("image", C.c_uint32), ("nops", C.c_uint32), ("nrects", C.c_uint32), ("reserved", C.c_uint32),
                ("ops", PixelOp * _K["UNET_PIXEL_MAX_OPS"]), ("rects", (C.c_uint16 * 4) * _K["UNET_PIXEL_MAX_RECTS"])]


class RectSet(C.Structure):
    _fields_ = [("image", C.c_uint32), ("nrects", C.c_uint32), ("rects", (C.c_uint16 * 4) * _K["UNET_PIXEL_MAX_RECTS"])]


class FieldImage(C.Structure):
    """unet_field_image: the descriptor of one image of a field warp (include/unet_hip.h)"""
    _fields_ = [("fired", C.c_int32), ("pre", C.c_float * 6), ("optical", C.c_float * 3), ("nodes", (C.c_float * (_K["UNET_FIELD_MAX_CELLS"] + 1)) * 2)]


class ElasticImage(C.Structure):
    _fields_ = [("key0", C.c_uint32), ("key1", C.c_uint32), ("alpha", C.c_float), ("fired", C.c_int32), ("same_dxdy", C.c_int32)]


class TiffLevel(C.Structure):
    """unet_tiff_level: one image of a launch over tiles (include/unet_hip.h)"""
    _fields_ = [("src", vp), ("row_stride", C.c_longlong), ("plane_stride", C.c_longlong), ("H", C.c_int), ("W", C.c_int)]


class PackJob(C.Structure):
    _fields_ = [("w", vp), ("wp", vp), ("Cout", C.c_int), ("Cin", C.c_int), ("ks", C.c_int), ("mode", C.c_int), ("out_scale", vp)]


# header struct -> mirror class: the reader refuses a struct typedef of the header that is missing here
STRUCTS = {"unet_tuning": Tuning, "unet_conv_desc": ConvDesc, "unet_wgrad_desc": WgradDesc, "unet_pack_job": PackJob,
           "unet_field_image": FieldImage, "unet_elastic_image": ElasticImage, "unet_pixel_op": PixelOp, "unet_pixel_prog": PixelProg,
           "unet_rect_set": RectSet, "unet_tiff_level": TiffLevel}
# name -> (restype, [argtypes]) of every prototype.  A declaration the reader cannot type raises there, so every declared symbol has a signature
_sig = signatures(HEADER, STRUCTS)
# two struct pointers stay untyped, as they always were: their callers pass ctypes.addressof(array), a bare integer
for _name, _at, _cls in (("unet_pixel_ops", 5, PixelProg), ("unet_fill_rects_mask", 5, RectSet)):
    assert _sig[_name][1][_at] is C.POINTER(_cls), _name
    _sig[_name][1][_at] = vp


def declared_symbols() -> list[str]:
    """Every function name include/unet_hip.h declares (used by the CPU-side ABI test)."""
    return sorted(_sig)


def _load() -> C.CDLL:
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -m unet_amd.build` (hipcc --offload-arch=gfx950). "
            "The MI355X path has no CPU fallback.")
    lib = C.CDLL(str(LIB_PATH))
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    if missing:
        raise ImportError(f"libunet_hip.so does not export: {missing}")
    return lib


lib = _load()

for _name, (_res, _args) in _sig.items():
    _fn = getattr(lib, _name)
    _fn.restype = _res
    _fn.argtypes = _args

if lib.unet_abi_version() != _K["UNET_ABI_VERSION"]:
    raise ImportError("libunet_hip.so ABI version mismatch; rebuild with `python -m unet_amd.build --force`")


class UnetHipError(RuntimeError):
    pass


def check(rc: int, what: str = "") -> None:
    if rc != UNET_OK:
        msg = lib.unet_last_error().decode(errors="replace")
        raise UnetHipError(f"{what}: rc={rc}: {msg}")

