"""ctypes binding of libunet_hip.so (the C ABI declared in include/unet_hip.h).

The product path has NO fallback: if the HIP library is missing or does not
export a declared symbol, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path

import torch  # noqa: F401  -- FIRST: torch ships its own libamdhip64; loading libunet_hip.so before it binds /opt/rocm's copy and the process ends
#                    up with two HIP runtimes (the second one reports "no ROCm-capable device": seen with build() + smoke() in one process)

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "lib" / "libunet_hip.so"
HEADER = _HERE.parent / "include" / "unet_hip.h"

UNET_OK = 0
CONV_RELU = 1
CONV_MASK = 4
CONV_FWD = 0
CONV_DGRAD = 1
F32 = 0
BF16 = 1

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


PIXEL_MAX_PROGS, PIXEL_MAX_OPS, PIXEL_MAX_RECTS, BLUR_MAX_IMAGES, BLUR_MAX_KSIZE = 8, 8, 32, 16, 31
PIXEL_BRIGHTNESS_CONTRAST, PIXEL_GAMMA, PIXEL_GAUSS_NOISE, PIXEL_FILL_RECTS, PIXEL_CHANNEL_DROP, PIXEL_CHANNEL_PERMUTE = 1, 2, 3, 4, 5, 6
PIXEL_PER_CHANNEL = 0x100


class PixelOp(C.Structure):
    _fields_ = [("code", C.c_uint32), ("u0", C.c_uint32), ("u1", C.c_uint32), ("f0", C.c_float), ("f1", C.c_float)]


class PixelProg(C.Structure):
    """unet_pixel_prog: the pointwise program of one image (include/unet_hip.h)"""
    _fields_ = [("image", C.c_uint32), ("nops", C.c_uint32), ("nrects", C.c_uint32), ("reserved", C.c_uint32),
                ("ops", PixelOp * PIXEL_MAX_OPS), ("rects", (C.c_uint16 * 4) * PIXEL_MAX_RECTS)]


class RectSet(C.Structure):
    _fields_ = [("image", C.c_uint32), ("nrects", C.c_uint32), ("rects", (C.c_uint16 * 4) * PIXEL_MAX_RECTS)]


FIELD_MAX_IMAGES, FIELD_MAX_CELLS, ELASTIC_MAX_IMAGES, ELASTIC_MAX_KSIZE = 16, 16, 64, 401
FIELD_DENSE, FIELD_GRID, FIELD_OPTICAL = 0, 1, 2


class FieldImage(C.Structure):
    """unet_field_image: the descriptor of one image of a field warp (include/unet_hip.h)"""
    _fields_ = [("fired", C.c_int32), ("pre", C.c_float * 6), ("optical", C.c_float * 3), ("nodes", (C.c_float * (FIELD_MAX_CELLS + 1)) * 2)]


class ElasticImage(C.Structure):
    _fields_ = [("key0", C.c_uint32), ("key1", C.c_uint32), ("alpha", C.c_float), ("fired", C.c_int32), ("same_dxdy", C.c_int32)]


class TiffLevel(C.Structure):
    """unet_tiff_level: one image of a launch over tiles (include/unet_hip.h)"""
    _fields_ = [("src", vp), ("row_stride", C.c_longlong), ("plane_stride", C.c_longlong), ("H", C.c_int), ("W", C.c_int)]


TIFF_MAX_LEVELS = 32


class PackJob(C.Structure):
    _fields_ = [("w", vp), ("wp", vp), ("Cout", C.c_int), ("Cin", C.c_int), ("ks", C.c_int), ("mode", C.c_int), ("out_scale", vp)]


def declared_symbols() -> list[str]:
    """Every function name include/unet_hip.h declares (used by the CPU-side ABI test)."""
    txt = HEADER.read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", txt)))


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

i, ll, f, sz = C.c_int, C.c_longlong, C.c_float, C.c_size_t
_sig = {
    "unet_abi_version": (i, []),
    "unet_last_error": (C.c_char_p, []),
    "unet_conv2d_colsum_rows": (i, [C.POINTER(ConvDesc)]),
    "unet_conv2d": (i, [C.POINTER(ConvDesc), vp]),
    "unet_conv2d_variant": (i, [C.POINTER(ConvDesc)]),
    "unet_conv2d_splitk_workspace": (sz, [C.POINTER(ConvDesc)]),
    "unet_tuning_default": (None, [C.POINTER(Tuning)]),
    "unet_pack_batch_table_bytes": (sz, [i]),
    "unet_pack_batch_build": (i, [C.POINTER(PackJob), i, i, vp, C.POINTER(C.c_uint)]),
    "unet_pack_batch_run": (i, [vp, i, C.c_uint, i, vp]),
    "unet_pack_weights_size": (sz, [i, i, i, i]),
    "unet_pack_weights": (i, [vp, vp, i, i, i, i, vp]),
    "unet_pack_weights_strided": (i, [vp, ll, ll, vp, i, i, vp]),
    "unet_row_softmax": (i, [vp, i, i, vp, i, i, ll, i, vp]),
    "unet_row_softmax_bwd": (i, [vp, i, i, vp, i, i, vp, i, i, ll, i, vp]),
    "unet_conv2d_wgrad_workspace": (sz, [C.POINTER(WgradDesc)]),
    "unet_conv2d_wgrad_dma": (i, [C.POINTER(WgradDesc)]),
    "unet_conv2d_wgrad": (i, [C.POINTER(WgradDesc), vp]),
    "unet_bn_stats_rows": (i, [ll]),
    "unet_bn_stats": (i, [vp, i, i, ll, i, vp, vp]),
    "unet_bn_finalize": (i, [vp, vp, i, ll, i, vp, vp, vp, vp, f, f, vp, vp, vp, vp, vp, vp]),
    "unet_bn_eval_coeffs": (i, [vp, vp, vp, vp, f, i, vp, vp, vp]),
    "unet_affine_act": (i, [vp, i, i, vp, vp, vp, i, i, vp, vp, vp, i, i, ll, i, i, vp]),
    "unet_bn_bwd_reduce": (i, [vp, i, i, vp, i, i, vp, i, i, vp, vp, ll, i, vp, vp]),
    "unet_bn_bwd_finalize": (i, [vp, i, ll, i, vp, vp, vp, vp, vp]),
    "unet_bn_bwd_apply": (i, [vp, i, i, vp, i, i, vp, i, i, vp, vp, vp, vp, vp, vp, i, i, vp, i, i, i, ll, i, vp]),
    "unet_maxpool3x3s2": (i, [vp, i, i, vp, i, i, vp, i, i, i, i, i, i, vp]),
    "unet_maxpool3x3s2_bwd": (i, [vp, i, i, vp, vp, i, i, i, i, i, i, i, i, i, vp]),
    "unet_avgpool2_ceil": (i, [vp, i, i, vp, i, i, i, i, i, i, i, i, vp]),
    "unet_avgpool2_ceil_bwd": (i, [vp, i, i, vp, i, i, i, i, i, i, i, i, i, vp]),
    "unet_shuffle_blur": (i, [vp, i, i, vp, i, i, i, i, i, i, i, vp]),
    "unet_shuffle_blur_bwd": (i, [vp, i, i, vp, i, i, vp, i, i, i, i, i, i, i, vp]),
    "unet_shuffle_bwd_xmask": (i, [vp, i, i, vp, i, i, vp, i, i, i, i, i, i, vp]),
    "unet_resize_nearest": (i, [vp, i, i, vp, i, i, i, i, i, i, i, i, vp]),
    "unet_resize_nearest_bwd": (i, [vp, i, i, vp, i, i, i, i, i, i, i, i, vp]),
    "unet_nchw_to_nhwc": (i, [vp, vp, i, i, i, i, i, i, vp]),
    "unet_nhwc_to_nchw": (i, [vp, i, i, vp, i, i, i, i, vp]),
    "unet_copy_slice": (i, [vp, i, i, vp, i, i, ll, i, i, vp]),
    "unet_relu_mask": (i, [vp, i, i, vp, i, i, vp, i, i, ll, i, vp]),
    "unet_colsum": (i, [vp, i, i, ll, i, vp, vp, vp]),
    "unet_colsum_workspace": (sz, [ll, i]),
    "unet_dot": (i, [vp, i, i, vp, i, i, ll, i, vp, vp, vp]),
    "unet_ce_workspace": (sz, [ll]),
    "unet_ce_fwd": (i, [vp, i, i, vp, vp, ll, i, vp, vp, vp, vp]),
    "unet_ce_fwd_parts": (i, [vp, i, i, vp, vp, ll, i, vp, vp, vp]),
    "unet_ce_bwd": (i, [vp, i, i, vp, vp, ll, i, vp, f, vp, i, i, vp]),
    "unet_ce_fwd_pw": (i, [vp, i, i, vp, vp, ll, i, vp, vp, vp, vp]),
    "unet_ce_fwd_parts_pw": (i, [vp, i, i, vp, vp, ll, i, vp, vp, vp]),
    "unet_ce_bwd_pw": (i, [vp, i, i, vp, vp, ll, i, vp, f, vp, i, i, vp]),
    "unet_focal_fwd": (i, [vp, i, i, vp, vp, ll, i, f, vp, vp, vp]),
    "unet_focal_bwd": (i, [vp, i, i, vp, vp, ll, i, f, f, vp, i, i, vp]),
    "unet_dice_workspace": (sz, [i, ll, i]),
    "unet_dice_fwd": (i, [vp, i, i, vp, i, ll, i, f, i, ll, vp, vp, vp, vp]),
    "unet_dice_bwd": (i, [vp, i, i, vp, i, ll, i, i, vp, f, vp, i, i, vp]),
    "unet_combined_workspace": (sz, [i, ll, i]),
    "unet_combined_fwd": (i, [vp, i, i, vp, vp, i, ll, i, f, f, i, ll, vp, vp, vp, vp]),
    "unet_combined_bwd": (i, [vp, i, i, vp, vp, i, ll, i, f, i, vp, f, f, vp, i, i, vp]),
    "unet_regloss_fwd": (i, [vp, i, i, vp, ll, i, f, vp, vp, vp]),
    "unet_regloss_bwd": (i, [vp, i, i, vp, ll, i, f, f, vp, i, i, vp]),
    "unet_softmax_argmax": (i, [vp, i, i, i, i, i, i, vp, vp, vp]),
    "unet_adam_step": (i, [vp, vp, vp, vp, vp, ll, c_float_p, f, f, f, f, i, f, vp]),
    "unet_adam_hyper_floats": (i, []),
    "unet_adam_fill_hyper": (i, [c_float_p, c_float_p, f, f, f, f, i, f]),
    "unet_adam_step_dev": (i, [vp, vp, vp, vp, vp, ll, vp, vp]),
    "unet_mosaic_accumulate": (i, [vp, i, i, i, vp, vp, i, i, i, i, vp]),
    "unet_mosaic_finalize": (i, [vp, vp, i, i, i, vp, vp]),
    "unet_raster_nodata_zero": (i, [vp, i, i, ll, C.c_double, vp]),
    "unet_window_nonzero": (i, [vp, i, i, ll, i, vp, i, i, i, vp, vp]),
    "unet_window_gather": (i, [vp, i, i, ll, ll, i, vp, i, i, i, i, vp, i, i, i, vp]),
    "unet_mosaic_accumulate_windows": (i, [vp, i, i, i, i, i, vp, i, i, i, i, vp, vp, i, i, i, i, vp]),
    "unet_tiff_lzw_decode": (ll, [vp, ll, vp, ll]),
    "unet_tiff_packbits_decode": (ll, [vp, ll, vp, ll]),
    "unet_tiff_lzw_cap": (ll, [ll]),
    "unet_tiff_lzw_encode": (ll, [vp, ll, vp, ll]),
    "unet_tiff_encode_strips": (i, [vp, i, i, i, i, ll, ll, i, i, ll, i, vp, ll, vp, vp]),
    "unet_tiff_compact_strips": (i, [vp, ll, vp, vp, i, vp, ll, vp]),
    "unet_tiff_encode_tiles": (i, [vp, i, i, i, i, ll, ll, i, i, ll, i, vp, ll, vp, vp]),
    "unet_tiff_encode_tile_levels": (i, [C.POINTER(TiffLevel), i, i, i, i, i, ll, i, vp, ll, vp, vp]),
    "unet_tiff_reduce_level": (i, [vp, i, i, i, i, i, ll, ll, i, i, C.c_double, vp, vp]),
    "unet_mosaic_finalize_rows": (i, [vp, vp, i, i, i, i, i, vp, c_float_p, vp]),
    "unet_tiles_stage": (i, [vp, i, i, i, i, i, i, C.c_ulonglong, C.c_ulonglong, vp, vp]),
    "unet_mask_stage": (i, [vp, i, i, i, i, C.c_ulonglong, C.c_ulonglong, vp, i, vp]),
    "unet_dice_counts": (i, [vp, vp, ll, i, vp, vp]),
    "unet_warp_affine": (i, [vp, vp, i, i, i, i, c_float_p, i, i, f, vp]),
    "unet_warp_affine_mask": (i, [vp, vp, i, i, i, i, c_float_p, i, C.c_double, vp]),
    "unet_warp_field": (i, [vp, vp, i, i, i, i, i, C.POINTER(FieldImage), vp, i, i, i, i, f, vp]),
    "unet_warp_field_mask": (i, [vp, vp, i, i, i, i, i, C.POINTER(FieldImage), vp, i, i, i, C.c_double, vp]),
    "unet_elastic_field": (i, [vp, vp, i, i, i, C.POINTER(ElasticImage), c_float_p, i, vp]),
    "unet_pixel_ops": (i, [vp, i, i, i, i, vp, i, vp]),
    "unet_fill_rects_mask": (i, [vp, i, i, i, i, vp, i, C.c_double, vp]),
    "unet_blur_separable": (i, [vp, vp, i, i, i, i, C.POINTER(C.c_int), c_float_p, vp]),
    "unet_window_gather_oriented": (i, [vp, i, i, ll, ll, i, vp, i, i, i, i, vp, i, i, i, i, vp]),
    "unet_nchw_to_nhwc_oriented": (i, [vp, vp, i, i, i, i, i, i, i, i, vp]),
    "unet_tta_accumulate": (i, [vp, i, i, i, i, i, i, i, i, i, vp, i, i, vp, vp, vp]),
    "unet_mosaic_accumulate_weighted": (i, [vp, i, i, i, vp, vp, vp, vp, vp, i, i, i, i, vp]),
    "unet_mosaic_accumulate_windows_weighted": (i, [vp, i, i, i, i, i, vp, i, i, i, i, vp, vp, i, i, i, i, vp, vp, vp, vp]),
    "unet_mosaic_finalize_rows_weighted": (i, [vp, vp, vp, i, i, i, i, i, vp, c_float_p, vp]),
    "unet_cc_tile_shape": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "unet_cc_label": (i, [vp, i, i, i, vp, vp, vp]),
    "unet_cc_label_keys": (i, [vp, i, i, vp, vp, vp]),
    "unet_cc_sizes": (i, [vp, i, i, vp, vp]),
    "unet_sieve_round": (i, [vp, vp, i, i, i, ll, i, vp, vp, vp, vp, vp]),
    "unet_majority_filter": (i, [vp, vp, i, i, i, i, vp]),
    "unet_postprocess_counters": (i, [vp, C.POINTER(C.c_int32), vp]),
    "unet_edt_workspace": (sz, [i, i, i]),
    "unet_border_edt": (i, [vp, i, i, i, i, i, vp, vp, vp]),
    "unet_border_weight": (i, [vp, vp, vp, i, f, C.c_double, ll, vp, vp]),
    "unet_object_edt_workspace": (sz, [i, i, i]),
    "unet_object_edt": (i, [vp, i, i, i, i, i, i, i, i, vp, vp, vp, vp, f, C.c_double, vp, vp]),
    "unet_vec_flags": (i, [vp, vp, i, i, C.POINTER(C.c_uint32), vp, vp]),
    "unet_vec_scan_words": (ll, [ll]),
    "unet_vec_scan": (i, [vp, ll, vp, vp, vp]),
    "unet_vec_read": (i, [vp, i, C.POINTER(C.c_longlong), vp]),
    "unet_vec_succ": (i, [vp, vp, i, i, ll, vp, vp, vp]),
    "unet_vec_min_rounds": (i, [vp, ll, vp, vp, vp, vp, i, i, vp, vp]),
    "unet_vec_swap": (i, [vp, vp, vp, i, i, vp, vp, vp]),
    "unet_vec_rank_init": (i, [vp, vp, i, i, vp, vp, vp, vp, vp, vp, ll, vp]),
    "unet_vec_rank_rounds": (i, [ll, vp, vp, vp, vp, vp, vp, i, vp, vp]),
    "unet_vec_ring_info": (i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp, ll, vp, vp, vp, vp]),
    "unet_vec_place": (i, [vp, vp, vp, vp, vp, vp, ll, ll, vp, vp, vp]),
    "unet_vec_emit": (i, [vp, vp, i, i, vp, vp, vp, ll, ll, vp, vp]),
    "unet_simp_marks": (i, [vp, vp, vp, vp, i, i, ll, vp, vp]),
    "unet_simp_gather": (i, [vp, vp, vp, vp, vp, ll, ll, ll, vp, vp, vp]),
    "unet_simp_closed": (i, [vp, vp, vp, vp, vp, ll, ll, i, vp, vp, vp, vp, vp, vp, vp, vp]),
    "unet_simp_near_rounds": (i, [ll, vp, vp, vp, vp, i, vp, vp]),
    "unet_simp_dp_rounds": (i, [vp, vp, vp, ll, ll, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp]),
    "unet_simp_emit": (i, [vp, vp, vp, vp, vp, vp, vp, ll, ll, ll, vp, vp, vp]),
    "unet_simp_area": (i, [vp, vp, vp, ll, ll, vp, vp]),
    "unet_inst_tile_shapes": (None, [C.POINTER(C.c_int)] * 4),
    "unet_inst_partials": (i, []),
    "unet_inst_distance": (i, [vp, i, i, C.POINTER(C.c_uint32), i, vp, vp, vp]),
    "unet_inst_check_labels": (i, [vp, vp, i, i, vp, vp]),
    "unet_inst_ascent": (i, [vp, vp, i, i, vp, vp, vp, vp]),
    "unet_inst_ptr_rounds": (i, [vp, ll, vp, vp, i, vp, vp]),
    "unet_inst_gather": (i, [vp, vp, ll, vp, vp]),
    "unet_inst_merge_round": (i, [vp, vp, i, i, i, i, vp, vp, vp, vp, vp, vp, vp]),
    "unet_inst_canonical": (i, [vp, ll, vp, vp, vp, vp]),
    "unet_inst_marks": (i, [vp, vp, ll, C.POINTER(C.c_uint32), vp, vp]),
    "unet_inst_ids": (i, [vp, vp, vp, ll, C.POINTER(C.c_uint32), vp, vp]),
    "unet_ras_count": (i, [vp, vp, vp, ll, ll, i, vp, vp, vp]),
    "unet_ras_scan_words": (ll, [ll]),
    "unet_ras_scan": (i, [vp, ll, vp, vp, vp, vp]),
    "unet_ras_emit": (i, [vp, vp, vp, vp, ll, ll, i, i, vp, ll, vp, vp]),
    "unet_ras_spans": (i, [vp, ll, vp, ll, i, i, vp, vp, vp]),
    "unet_ras_resolve": (i, [vp, i, i, i, i, vp, vp]),
    "unet_ras_resolve_ids": (i, [vp, i, i, vp, vp]),
    "unet_zonal_lds_bins": (i, []),
    "unet_zonal_counts": (i, [vp, vp, vp, i, i, i, i, vp, vp, vp, vp]),
    "unet_zonal_absmax": (i, [vp, vp, i, i, i, i, C.c_float, vp, vp]),
    "unet_zonal_values": (i, [vp, vp, i, i, i, i, C.c_float, i, vp, vp, vp, vp]),
    "unet_obj_point_packed": (i, [i, i]),
    "unet_obj_compact": (i, [vp, vp, vp, ll, ll, vp, vp, vp]),
    "unet_obj_accumulate": (i, [vp, vp, vp, i, i, C.POINTER(C.c_uint32), ll, vp, vp, vp, vp]),
    "unet_obj_point": (i, [vp, vp, vp, i, i, C.POINTER(C.c_uint32), ll, vp, vp, vp, vp, vp]),
}
# bf16-storage twins: same argument lists (every tensor is a void pointer on this side)
for _n in ("bn_stats", "affine_act", "bn_bwd_reduce", "bn_bwd_apply", "maxpool3x3s2", "maxpool3x3s2_bwd", "avgpool2_ceil",
           "avgpool2_ceil_bwd", "shuffle_blur", "shuffle_blur_bwd", "shuffle_bwd_xmask", "resize_nearest", "resize_nearest_bwd", "nchw_to_nhwc", "copy_slice", "ce_bwd", "ce_bwd_pw", "focal_bwd",
           "dice_bwd", "combined_bwd"):
    _sig[f"unet_{_n}_bf16"] = _sig[f"unet_{_n}"]
for _n in ("pack_weights_strided", "row_softmax", "row_softmax_bwd", "relu_mask", "dot"):
    _sig[f"unet_{_n}_bf16"] = _sig[f"unet_{_n}"]
_sig["unet_sa_fused_supported"] = (i, [i, i])
_sig["unet_sa_pack_elems"] = (sz, [i, i])
_sig["unet_sa_pack_bf16"] = (i, [vp, i, i, i, i, i, vp, vp])
_sig["unet_sa_fwd_bf16"] = (i, [vp, i, i, i, i, i, vp, vp, i, i, vp, vp])
_sig["unet_sa_rowdot_bf16"] = (i, [vp, i, i, vp, i, i, i, i, i, vp, vp])
_sig["unet_sa_bwd_bf16"] = (i, [vp, i, i, i, i, i, vp, i, i, vp, vp, vp, vp, vp, vp, vp])
_sig["unet_cast_slice_bf16"] = (i, [vp, i, i, vp, i, i, ll, i, vp])
_sig["unet_pack_weights_size_bf16"] = _sig["unet_pack_weights_size"]
_sig["unet_pack_weights_bf16"] = _sig["unet_pack_weights"]

for _name, (_res, _args) in _sig.items():
    _fn = getattr(lib, _name)
    _fn.restype = _res
    _fn.argtypes = _args

_undeclared = [s for s in declared_symbols() if s not in _sig]
if _undeclared:
    raise ImportError(f"ctypes signatures missing for: {_undeclared}")

if lib.unet_abi_version() != 8:
    raise ImportError("libunet_hip.so ABI version mismatch; rebuild with `python -m unet_amd.build --force`")


class UnetHipError(RuntimeError):
    pass


def check(rc: int, what: str = "") -> None:
    if rc != UNET_OK:
        msg = lib.unet_last_error().decode(errors="replace")
        raise UnetHipError(f"{what}: rc={rc}: {msg}")

