"""GPU suite of tiled GeoTIFF output with overviews (csrc/tiff_pyramid.hip, unet_tiff_encode_tiles in csrc/tiff_encode.hip,
unet_amd/tiffenc.py, the tile= / overviews= seam of predict.py): the pyramid kernels equal the rule restated sample by sample
(tests/tiff_cog_ref.py) bit for bit, the device encoder's tiles equal the host encoder's byte for byte, the files equal write_tiff's
whatever the band size, and predict_raster writes the content of its uncompressed run with the reference pyramid behind it.  Every device
buffer of the module -- pyramid levels, scratch slots, sizes, offsets, compact bytes -- sits in a guard-banded allocation that is checked
after every launch; sources sit between canaries."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import predict as P  # noqa: E402

import tiff_cog_ref as R  # noqa: E402
from tiff_cog_ref import image  # noqa: E402
from guard import CANARY, guarded  # noqa: E402

from unet_amd import tiffio  # noqa: E402
from unet_amd.tiffio import read_tiff, read_tiff_level, tiff_levels, write_tiff  # noqa: E402

DTYPES = ("uint8", "int8", "uint16", "int16", "int32", "float32")
_FILL = {torch.uint8: 0xA5, torch.int8: -91, torch.uint16: 0xA5A5, torch.int16: -23131, torch.int32: -7, torch.int64: -7, torch.float32: -3.5e7}
_CANARY = {**CANARY, torch.int8: -113}          # (no sample of the images below)
_LAUNCHERS = ("tiff_encode_strips", "tiff_compact_strips", "tiff_encode_tiles", "tiff_reduce_level")
GT = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)


class Guards:
    def __init__(self):
        self.checks, self.launches = [], 0

    def alloc(self, shape, dtype, device="cuda"):
        t, c = guarded(shape, dtype, device, _FILL[dtype])
        self.checks.append(c)
        return t

    def upload(self, a: np.ndarray) -> torch.Tensor:
        h = torch.from_numpy(np.ascontiguousarray(a))
        t, c = guarded(h.shape, h.dtype, "cuda", _CANARY[h.dtype])
        t.copy_(h.cuda())
        self.checks.append(c)
        return t

    def check(self, what=""):
        for c in self.checks:
            c(what)

    def clear(self):
        self.check("end of case")
        self.checks.clear()


@pytest.fixture
def guards(monkeypatch):
    from unet_amd import ops, tiffenc
    g = Guards()
    monkeypatch.setattr(tiffenc, "_alloc", g.alloc)
    for name in _LAUNCHERS:
        def wrapped(*a, _fn=getattr(ops, name), _name=name, **k):
            r = _fn(*a, **k)
            g.launches += 1
            g.check(_name)
            return r
        monkeypatch.setattr(ops, name, wrapped)
    return g


def _nodata(dtype, how):
    if dtype == "float32":
        return float("nan") if how == "nearest" else -9999.0
    return {"uint8": 0, "int8": -128, "uint16": 65535, "int16": -3, "int32": 2}[dtype]


# ------------------------------------------------------------------------------------------------------------------ the pyramid kernels

# planes x H x W: the shapes of the host suite, 257 x 130 (odd height over several blocks, 16-byte groups that end inside a row for every
# sample size), and the single rows / columns whose blocks are clipped to 1 or 2 samples; tile 16, so that all of them have levels
PYRAMID_SHAPES = [(2, 1, 7), (2, 7, 1), (2, 33, 65), (2, 37, 53), (1, 257, 130), (1, 256, 256), (1, 300, 517), (2, 10, 10)]


@pytest.mark.parametrize("how", ["mode", "average", "nearest"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pyramid_levels_equal_the_rule_bit_for_bit(guards, dtype, how):
    from unet_amd.tiffenc import build_overviews
    if how == "mode" and dtype == "float32":
        with pytest.raises(ValueError, match="float"):
            build_overviews(torch.zeros(1, 40, 40, device="cuda"), "mode")
        return
    for n, shape in enumerate(PYRAMID_SHAPES):
        nodata = None if n % 3 == 2 else _nodata(dtype, how)
        a = image(dtype, shape, 10 + n, nodata)
        if dtype == "float32" and nodata is not None and nodata != nodata:
            a[..., ::3, 1::4] = np.nan
        want = R.pyramid(a, 16, how, nodata)
        got = build_overviews(guards.upload(a), how, nodata, tile=16)
        assert [tuple(l.shape) for l in got] == [l.shape for l in want] and len(want) == len(R.level_shapes(*shape[1:], 16))
        for k, (x, y) in enumerate(zip(got, want)):
            assert x.dtype == getattr(torch, dtype) and x.cpu().numpy().tobytes() == y.tobytes(), (dtype, how, shape, "level", k + 1)
        guards.clear()
    assert guards.launches > 0
    assert build_overviews(guards.upload(image(dtype, (1, 1, 1), 1)), how, tile=16) == []          # 1 x 1: nothing to reduce


def test_row_sliced_and_single_plane_views_are_reduced_in_place(guards):
    from unet_amd.tiffenc import build_overviews
    for dtype, how in (("uint8", "mode"), ("int16", "average"), ("float32", "average"), ("int32", "nearest")):
        nodata = _nodata(dtype, how)
        cube = image(dtype, (4, 50, 61), 20, nodata)
        t = guards.upload(cube)
        for what, view, ref in (("row slice", t[:, 3:40], cube[:, 3:40]), ("one plane, row slice", t[2, 7:44], cube[2, 7:44]),
                                ("two planes of four, rows cut", t[1:3, :33], cube[1:3, :33])):
            assert view.data_ptr() != t.data_ptr() or not view.is_contiguous()
            got = build_overviews(view, how, nodata, tile=16)
            want = R.pyramid(ref, 16, how, nodata)
            assert len(got) == len(want) == 2
            for x, y in zip(got, want):
                assert x.shape == y.shape and x.cpu().numpy().tobytes() == y.tobytes(), (dtype, what)
        guards.clear()


def test_reduce_level_refuses_bad_arguments():
    from unet_amd import ops
    from unet_amd._lib import lib
    t = torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, 4, 4, dtype=torch.uint8, device="cuda")
    for args in ((t[0], "mode", None, out), (t, "cubic", None, out), (t, "mode", None, out[:, :3]), (t, "mode", None, out.to(torch.int16)),
                 (t[:, :, ::2], "mode", None, out), (t.float(), "mode", None, out.float()), (t[:, :1, :1], "mode", None, out[:, :1, :1])):
        with pytest.raises(ValueError):
            ops.tiff_reduce_level(*args)
    ptr, o = t.data_ptr(), out.data_ptr()
    for bad in ((ptr, 3, 0, 1, 8, 8, 8, 64, 1, 0, 0.0, o), (ptr, 1, 2, 1, 8, 8, 8, 64, 2, 0, 0.0, o), (ptr, 4, 2, 1, 8, 2, 2, 16, 1, 0, 0.0, o),
                (ptr, 1, 0, 1, 8, 8, 7, 64, 1, 0, 0.0, o), (ptr, 1, 0, 1, 8, 8, 8, 64, 1, 1, 256.0, o), (ptr, 1, 0, 1, 8, 8, 8, 64, 1, 1, 0.5, o),
                (ptr, 1, 0, 1, 1, 1, 1, 1, 1, 0, 0.0, o), (ptr, 1, 0, 1, 8, 8, 8, 64, 1, 0, 0.0, ptr), (None, 1, 0, 1, 8, 8, 8, 64, 1, 0, 0.0, o)):
        assert lib.unet_tiff_reduce_level(*bad, None) == -1, bad
    s, z = torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    for bad in ((ptr, 1, 1, 8, 8, 8, 64, 8, 1, 0, 1, s.data_ptr(), 128, z.data_ptr()), (ptr, 1, 1, 8, 8, 8, 64, 24, 1, 0, 1, s.data_ptr(), 4096, z.data_ptr()),
                (ptr, 1, 1, 8, 8, 8, 64, 16, 1, 1, 1, s.data_ptr(), 4096, z.data_ptr()), (ptr, 1, 1, 8, 8, 8, 64, 16, 1, 0, 1, s.data_ptr(), 64, z.data_ptr())):
        assert lib.unet_tiff_encode_tiles(*bad, None) == -1, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------ tile streams

def _host_tiles(a: np.ndarray, tile: int, predictor: int):
    """the host encoder's stream of every tile of a [P, H, W] array, in TIFF tile order"""
    lib = tiffio._codecs()
    out = []
    for block in R.tile_blocks(a, tile):
        src = tiffio._predicted_le(block, predictor)
        dst = np.empty(tiffio.lzw_cap(src.size), dtype=np.uint8)
        got = lib.unet_tiff_lzw_encode(src.ctypes.data, src.size, dst.ctypes.data, dst.size)
        assert got > 0
        out.append(dst[:got].tobytes())
    return out


def _device_tiles(g: Guards, t: torch.Tensor, tile: int, predictor: int):
    from unet_amd import ops
    Pn, H, W = t.shape
    n = Pn * -(-H // tile) * -(-W // tile)
    slot = ops.tiff_slot_bytes(tile * tile * t.element_size())
    assert slot % 16 == 0 and slot >= tiffio.lzw_cap(tile * tile * t.element_size())
    scratch, sizes = g.alloc((n * slot,), torch.uint8), g.alloc((n,), torch.int32)
    assert ops.tiff_encode_tiles(t, tile, predictor, 0, n, scratch, sizes) == slot
    sz = sizes.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert (sz > 0).all() and (sz <= slot).all(), sz
    offs = g.alloc((n,), torch.int64)
    offs.copy_(torch.from_numpy(np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.int64)))
    compact = g.alloc((int(sz.sum()),), torch.uint8)
    ops.tiff_compact_strips(scratch, slot, sizes, offs, n, compact)
    raw = scratch.cpu().numpy()
    return [raw[j * slot:j * slot + int(sz[j])].tobytes() for j in range(n)], compact.cpu().numpy().tobytes()


def _same(g: Guards, a: np.ndarray, tile: int, predictor: int = 1, t: torch.Tensor = None, what=""):
    a3 = a[None] if a.ndim == 2 else a
    if t is None:
        t = g.upload(a3)
    want = _host_tiles(a3, tile, predictor)
    got, compact = _device_tiles(g, t, tile, predictor)
    assert [len(s) for s in got] == [len(s) for s in want], (what, tile, predictor)
    for j, (x, y) in enumerate(zip(got, want)):
        assert x == y, (what, "tile", j, tile, predictor)
    assert compact == b"".join(want), (what, "compact")
    g.clear()


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiles_of_three_ragged_planes(guards, dtype):
    a = image(dtype, (3, 150, 210), 30)                          # 3 x 4 tiles of 64 a plane, ragged on both edges
    for predictor in ((1,) if dtype == "float32" else (1, 2)):
        _same(guards, a, 64, predictor, what=dtype)
    assert guards.launches == (2 if dtype == "float32" else 4)


def test_large_tiles_of_random_samples_constant_planes_and_images_smaller_than_a_tile(guards):
    rng = np.random.default_rng(31)
    _same(guards, rng.integers(-2 ** 31, 2 ** 31, (300, 260), dtype=np.int64).astype(np.int32), 256, what="random int32: 256 KiB a tile")
    _same(guards, np.full((70, 130), 7, np.uint8), 64, what="constant")
    _same(guards, np.full((70, 130), 7, np.uint16), 64, 2, what="constant, differenced")
    for shape, tile in (((100, 10), 64), ((10, 100), 64), ((10, 10), 16), ((1, 1), 16), ((16, 16), 16), ((17, 33), 16)):
        for predictor in (1, 2):
            _same(guards, image("int16", shape, 32), tile, predictor, what=shape)
    cube = image("uint16", (4, 50, 61), 33)
    t = guards.upload(cube)
    _same(guards, cube[2, 7:44], 16, 2, t=t[2, 7:44][None], what="one plane, row slice")
    t = guards.upload(cube)
    _same(guards, cube[1:3, :33], 32, t=t[1:3, :33], what="two planes of four, rows cut")


# ------------------------------------------------------------------------------------------------------------------------ whole files

def test_the_file_equals_the_host_writers_whatever_the_band_size(guards, tmp_path):
    from unet_amd.tiffenc import write_tiff_device
    a = image("uint16", (3, 150, 210), 40, nodata=0)
    t = guards.upload(a)
    write_tiff(tmp_path / "host.tif", a, geotransform=GT, nodata=0, compress="lzw", predictor=2, tile=64, overviews="average")
    want = (tmp_path / "host.tif").read_bytes()
    for band in (1, 3, None):
        tm = {}
        size = write_tiff_device(tmp_path / "dev.tif", t, geotransform=GT, nodata=0, predictor=2, band_strips=band, timing=tm, tile=64,
                                 overviews="average")
        assert (tmp_path / "dev.tif").read_bytes() == want, band
        assert size == len(want) and tm["levels"] == [(150, 210), (75, 105), (38, 53)] and tm["reduce_seconds"] > 0
        assert {"encode_seconds", "copy_seconds", "file_seconds"} <= set(tm)
        guards.check(f"band {band}")
    assert [l["height"] for l in tiff_levels(tmp_path / "dev.tif")] == [150, 75, 38]
    assert np.array_equal(read_tiff(tmp_path / "dev.tif")[0], a)
    guards.clear()
    for dtype, how, view in (("uint8", "mode", False), ("float32", "average", False), ("int8", "nearest", True), ("int32", None, True)):
        nodata = None if how is None else _nodata(dtype, how)
        full = image(dtype, (3, 90, 140), 41, nodata)
        t = guards.upload(full)
        a, t = (full[1:, 5:83], t[1:, 5:83]) if view else (full, t)
        write_tiff(tmp_path / "h.tif", a, geotransform=GT, nodata=nodata, compress="lzw", tile=32, overviews=how)
        write_tiff_device(tmp_path / "d.tif", t, geotransform=GT, nodata=nodata, band_strips=5, tile=32, overviews=how)
        assert (tmp_path / "d.tif").read_bytes() == (tmp_path / "h.tif").read_bytes(), (dtype, how)
        guards.clear()
    with pytest.raises(ValueError, match="needs tile"):
        write_tiff_device(tmp_path / "bad.tif", t, overviews="mode")
    with pytest.raises(ValueError, match="tile must be"):
        write_tiff_device(tmp_path / "bad.tif", t, tile=100)
    with pytest.raises(ValueError, match="float"):
        write_tiff_device(tmp_path / "bad.tif", t.float(), tile=32, overviews="mode")


# ------------------------------------------------------------------------------------------------------------ the prediction entry point

SIZE = 64


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """the tiny model and the 300 x 420 raster of the end-to-end cases"""
    from unet_amd.model import HipDynamicUnet
    d = tmp_path_factory.mktemp("cog_scene")
    torch.manual_seed(11)
    model = HipDynamicUnet("xresnet18", 4, 3, (SIZE, SIZE))
    model.eval()
    img = np.random.default_rng(5).integers(1, 250, (4, 300, 420)).astype(np.uint8)
    write_tiff(d / "scene.tif", img, geotransform=GT)
    return model, d / "scene.tif"


@pytest.mark.parametrize("kw", [{}, {"class_zero": True}, {"all_classes": True}, {"regression": True}, {"large_file": True}],
                         ids=["mask", "class_zero", "all_classes", "regression", "large_file"])
def test_predict_raster_writes_tiles_and_overviews_of_the_uncompressed_run(guards, scene, tmp_path, kw):
    model, rpath = scene
    run = lambda **k: P.predict_raster(model, rpath, SIZE, 0.2, max_empty=0.9, batch_size=8, **kw, **k)
    run(out_path=tmp_path / "plain.tif", return_array=False)
    assert guards.launches == 0
    tm = {}
    assert run(out_path=tmp_path / "cog.tif", compress="lzw", tile=128, overviews="auto", return_array=False, timing=tm) is None
    assert (guards.launches > 0) == ("large_file" not in kw)          # the int8 merge is host numpy: the host writer, the same file
    level0, meta = read_tiff(tmp_path / "cog.tif")
    plain, pmeta = read_tiff(tmp_path / "plain.tif")
    assert level0.dtype == plain.dtype and np.array_equal(level0, plain) and level0.shape[-2:] == (tm["mosaic"][0], tm["mosaic"][1])
    assert meta["geotransform"] == pmeta["geotransform"] and meta.get("nodata") == pmeta.get("nodata") and meta["tags"] == pmeta["tags"]
    how = "mode" if kw in ({}, {"class_zero": True}, {"large_file": True}) else "average"          # what "auto" stands for
    nodata = -9999 if "regression" in kw else None
    want = R.pyramid(level0, 128, how, nodata)
    info = tiff_levels(tmp_path / "cog.tif")
    assert len(want) == 2 and [(l["height"], l["width"]) for l in info[1:]] == [w.shape[-2:] for w in want]
    assert [l["subfile_type"] for l in info] == [0, 1, 1]
    for k, w in enumerate(want):
        got = read_tiff_level(tmp_path / "cog.tif", k + 1)
        assert got.dtype == w.dtype and got.tobytes() == w.tobytes(), k + 1
    assert tm["write_seconds"] > 0 and tm["file_bytes"] == (tmp_path / "cog.tif").stat().st_size
    write_tiff(tmp_path / "host.tif", level0, geotransform=meta["geotransform"], nodata=nodata, compress="lzw", tile=128, overviews=how,
               tags=read_tiff(rpath)[1]["tags"])
    assert (tmp_path / "host.tif").read_bytes() == (tmp_path / "cog.tif").read_bytes()
    guards.clear()
