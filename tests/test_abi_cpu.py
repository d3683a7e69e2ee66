"""The binding is derived from the headers (unet_amd/_abi.py): the reader on header text written here, the table it derives from
include/unet_hip.h against the built library, the constants against the values they had as literals, and the hand-written struct mirrors
against the layout the C compiler gives the header's structs.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

from unet_amd import _abi

ROOT = Path(__file__).resolve().parent.parent

SYNTHETIC = """
/* int unet_commented_out(int a); */
// int unet_also_commented_out(void);
#ifndef UNET_X_H
#define UNET_X_H
#ifdef __cplusplus
extern "C" {
#endif
#define UNET_E_BAD (-3)      /* a comment behind a value */
#define UNET_MASK 0x1F0
#define UNET_PLAIN 7
enum { UNET_A = 1, UNET_B = 2, UNET_C, UNET_FLAG = 0x100 };
typedef unsigned short unet_half;
typedef struct unet_thing {
    int a, b;            /* unet_not_a_call(1) in a comment */
    float c[4];
} unet_thing;
typedef struct { long long n; } unet_other;
int unet_version(void);
const char* unet_text();
void unet_fill(unet_thing* t);
size_t unet_many(const float* x, int x_cs,
                 long long P, unsigned flags,
                 unsigned long long bits, double d, float f,   // a comment between parameters
                 const unet_other* o, unet_half* h, int dims[3], const unsigned char* src, void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def _header(tmp_path, text, name="x.h"):
    p = tmp_path / name
    p.write_text(text)
    return p


# ------------------------------------------------------------------------------------------------------------ the reader
def test_reader_reads_prototypes_constants_and_struct_names(tmp_path):
    h = _header(tmp_path, SYNTHETIC)
    decls = _abi.declarations(h)
    assert [d.name for d in decls] == ["unet_version", "unet_text", "unet_fill", "unet_many"]          # the commented-out ones are not there
    by = {d.name: d for d in decls}
    assert by["unet_version"] == ("unet_version", "int", ()) and by["unet_text"] == ("unet_text", "const char*", ())
    assert by["unet_fill"] == ("unet_fill", "void", ("unet_thing*",))
    assert by["unet_many"].ret == "size_t" and by["unet_many"].params == (
        "const float*", "int", "long long", "unsigned", "unsigned long long", "double", "float", "const unet_other*", "unet_half*", "int*",
        "const unsigned char*", "void*")
    assert _abi.constants(h) == {"UNET_E_BAD": -3, "UNET_MASK": 0x1F0, "UNET_PLAIN": 7, "UNET_A": 1, "UNET_B": 2, "UNET_C": 3, "UNET_FLAG": 256}
    assert _abi.struct_names(h) == ["unet_thing", "unet_other"]

    class Thing(C.Structure):
        _fields_ = [("a", C.c_int), ("b", C.c_int), ("c", C.c_float * 4)]

    class Other(C.Structure):
        _fields_ = [("n", C.c_longlong)]

    vp = C.c_void_p
    sig = _abi.signatures(h, {"unet_thing": Thing, "unet_other": Other})
    assert sig == {"unet_version": (C.c_int, []), "unet_text": (C.c_char_p, []), "unet_fill": (None, [C.POINTER(Thing)]),
                   "unet_many": (C.c_size_t, [vp, C.c_int, C.c_longlong, C.c_uint, C.c_ulonglong, C.c_double, C.c_float, C.POINTER(Other), vp, vp,
                                              vp, vp])}
    assert _abi.signatures(h, {"unet_thing": Thing}, only=("unet_fill",)) == {"unet_fill": (None, [C.POINTER(Thing)])}
    with pytest.raises(_abi.AbiError, match="unet_absent"):
        _abi.signatures(h, {}, only=("unet_absent",))


@pytest.mark.parametrize("text, where, match", [
    ("int unet_f(short x);", "signatures", r"unet_f.*`short`"),                                      # a type outside the vocabulary
    ("long unet_f(int x);", "signatures", r"unet_f.*`long`"),
    ("int unet_f(unet_bf x);", "signatures", r"unet_f.*`unet_bf`"),
    ("int unet_g(void (*cb)(int, int), int n);", "declarations", r"unet_g.*function-pointer"),       # a function-pointer parameter
    ("typedef struct { int a; } unet_s;\nint unet_h(int a);", "signatures", r"unet_s.*mirror"),      # a struct without a mirror class
    ("typedef struct { int a; } unet_s;\nint unet_h(const unet_s* s);", "only", r"unet_h.*unet_s.*mirror"),
    ("int unet_ok(int a);\n#define UNET_CALL(x) unet_hidden(x)", "declarations", r"unet_hidden"),   # `unet_x(` no prototype accounts for
    ("int unet_ok(int a);\ntypedef int unet_cb(int);", "declarations", r"unet_cb"),
    ("int unet_ok(int a);\nstatic inline int unet_inl(int a) { return a; }\nint unet_next(void);", "declarations", r"unet_inl"),
    ("extern int unet_count;", "declarations", r"unet_count"),
    ("#define UNET_SHIFTED (1 << 3)", "constants", r"UNET_SHIFTED"),
])
def test_reader_raises_on_what_it_cannot_read(tmp_path, text, where, match):
    h = _header(tmp_path, text + "\n")
    call = {"declarations": lambda: _abi.declarations(h), "constants": lambda: _abi.constants(h), "signatures": lambda: _abi.signatures(h, {}),
            "only": lambda: _abi.signatures(h, {}, only=("unet_h",))}[where]
    with pytest.raises(_abi.AbiError, match=match):
        call()


def test_reader_imports_nothing_heavy():
    code = "import sys, unet_amd._abi; assert not {'torch', 'numpy', 'unet_amd._lib'} & set(sys.modules), sorted(sys.modules)"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


# ------------------------------------------------------------------------------------------------------------ the real header
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import unet_amd._lib as L
    return L


def test_every_declared_function_is_exported_and_typed_as_the_table_says(L):
    assert len(L._sig) >= 188 and L.declared_symbols() == sorted(L._sig)
    assert sorted(L._sig) == sorted(d.name for d in _abi.declarations(L.HEADER))
    for name, (res, args) in L._sig.items():
        fn = getattr(L.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_signatures_at_the_places_where_a_slip_would_hurt(L):
    s, vp, i, ll = L._sig, C.c_void_p, C.c_int, C.c_longlong
    assert s["unet_raster_nodata_zero"] == (i, [vp, i, i, ll, C.c_double, vp])
    assert s["unet_tiles_stage"][1][7] is C.c_ulonglong and s["unet_tiles_stage"][1][8] is C.c_ulonglong and len(s["unet_tiles_stage"][1]) == 11
    assert s["unet_pack_batch_run"][1][2] is C.c_uint
    assert s["unet_conv2d_splitk_workspace"] == (C.c_size_t, [C.POINTER(L.ConvDesc)])
    assert s["unet_tiff_lzw_cap"] == (ll, [ll])
    assert s["unet_last_error"] == (C.c_char_p, [])
    assert s["unet_tuning_default"] == (None, [C.POINTER(L.Tuning)])
    assert s["unet_zonal_values"][1][6] is C.c_float and s["unet_zonal_values"][1][7] is i and len(s["unet_zonal_values"][1]) == 12
    assert s["unet_tiff_encode_tile_levels"][1][0] is C.POINTER(L.TiffLevel)
    assert s["unet_conv2d_wgrad"] == (i, [C.POINTER(L.WgradDesc), vp]) and s["unet_pack_batch_build"][1][0] is C.POINTER(L.PackJob)
    assert s["unet_warp_field"][1][7] is C.POINTER(L.FieldImage) and s["unet_elastic_field"][1][5] is C.POINTER(L.ElasticImage)
    # the two struct pointers whose callers pass ctypes.addressof(array), an integer: untyped as they were in the hand-written table
    assert s["unet_pixel_ops"][1][5] is vp and s["unet_fill_rects_mask"][1][5] is vp
    derived = _abi.signatures(L.HEADER, L.STRUCTS)
    assert derived["unet_pixel_ops"][1][5] is C.POINTER(L.PixelProg) and derived["unet_fill_rects_mask"][1][5] is C.POINTER(L.RectSet)
    derived["unet_pixel_ops"][1][5] = derived["unet_fill_rects_mask"][1][5] = vp
    assert derived == s          # nothing else departs from the header


def test_constants_keep_the_values_they_had_as_literals(L):
    want = dict(UNET_OK=0, F32=0, BF16=1, CONV_RELU=1, CONV_MASK=4, CONV_FWD=0, CONV_DGRAD=1,
                PIXEL_MAX_PROGS=8, PIXEL_MAX_OPS=8, PIXEL_MAX_RECTS=32, BLUR_MAX_IMAGES=16, BLUR_MAX_KSIZE=31,
                PIXEL_BRIGHTNESS_CONTRAST=1, PIXEL_GAMMA=2, PIXEL_GAUSS_NOISE=3, PIXEL_FILL_RECTS=4, PIXEL_CHANNEL_DROP=5, PIXEL_CHANNEL_PERMUTE=6,
                PIXEL_PER_CHANNEL=0x100, FIELD_MAX_IMAGES=16, FIELD_MAX_CELLS=16, ELASTIC_MAX_IMAGES=64, ELASTIC_MAX_KSIZE=401,
                FIELD_DENSE=0, FIELD_GRID=1, FIELD_OPTICAL=2, TIFF_MAX_LEVELS=32)
    assert {k: getattr(L, k) for k in want} == want
    k = _abi.constants(L.HEADER)
    assert k["UNET_ABI_VERSION"] == 8 == L.lib.unet_abi_version() and k["UNET_E_BADARG"] == -1 and k["UNET_E_HIP"] == -3
    assert len(L.PixelProg().ops) == 8 and len(L.PixelProg().rects) == 32 and len(L.RectSet().rects) == 32 and len(L.FieldImage().nodes[0]) == 17


def test_tiffio_types_its_codecs_from_the_headers(L):
    from unet_amd import tiffio
    lib = tiffio._codecs()
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    for name in ("unet_tiff_lzw_decode", "unet_tiff_packbits_decode", "unet_tiff_lzw_encode"):
        fn = getattr(lib, name)
        assert fn.restype is ll and list(fn.argtypes) == [vp, ll, vp, ll] == L._sig[name][1], name
    assert lib.has_jpeg and lib.unet_tiff_jpeg_decode.restype is ll
    assert list(lib.unet_tiff_jpeg_decode.argtypes) == [vp, ll, vp, ll, i, vp, ll, vp]
    # with the host-only library present the reader needs neither torch nor the HIP library
    code = ("import sys, unet_amd.tiffio as t; lib = t._codecs(); assert lib.has_jpeg; "
            "assert not {'torch', 'unet_amd._lib'} & set(sys.modules), sorted(sys.modules)")
    assert (ROOT / "unet_amd" / "lib" / "libunet_tiff.so").exists()
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


# ------------------------------------------------------------------------------------------------------------ struct layouts
def test_struct_mirrors_have_the_layout_the_compiler_gives_the_header(L, tmp_path):
    assert set(_abi.struct_names(L.HEADER)) == set(L.STRUCTS) and len(L.STRUCTS) == 10          # a new struct of the header cannot be forgotten
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    lines, want = [], []
    for cname, cls in L.STRUCTS.items():
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        want.append(f"{cname} {C.sizeof(cls)}")
        for fname, _ in cls._fields_:
            lines.append(f'    printf("{cname}.{fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname}*)0)->{fname}));')
            want.append(f"{cname}.{fname} {getattr(cls, fname).offset} {getattr(cls, fname).size}")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "unet_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    r = subprocess.run([cc, "-I", str(L.HEADER.parent), str(src), "-o", str(tmp_path / "layout")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr          # (a field ctypes has and the header lacks does not compile)
    got = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(want) == 10 + sum(len(c._fields_) for c in L.STRUCTS.values()) and len(want) > 100
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]
