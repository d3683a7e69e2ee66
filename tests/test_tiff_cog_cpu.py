"""The host side of tiled GeoTIFF output with overviews (tiffio.write_tiff(compress="lzw", tile=, overviews=)): the pyramid rule
of tiffio.reduce_level against its restatement one sample at a time (tests/tiff_cog_ref.py), every level of the written files through
read_tiff_level and through libtiff (Pillow), the layout against the rules of a cloud-optimised GeoTIFF, the argument errors, and the
bounded walk along the IFD chain."""
import os
import struct
import sys

import numpy as np
import pytest
from PIL import Image          # (libtiff: its absence is an error, not a skip)

sys.path.insert(0, os.path.dirname(__file__))

import tiff_cog_ref as R  # noqa: E402
from tiff_cog_ref import image  # noqa: E402

from unet_amd import tiffio  # noqa: E402
from unet_amd.tiffio import read_tiff, read_tiff_level, tiff_info, tiff_levels, write_tiff  # noqa: E402

DTYPES = ("uint8", "int8", "uint16", "int16", "int32", "float32")
GT = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (33, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_level_equals_the_rule_sample_by_sample(dtype, shape):
    for nodata in (None, 0):
        a = image(dtype, (2, *shape), 1, nodata)
        for how in tiffio.RESAMPLINGS:
            if how == "mode" and dtype == "float32":
                continue
            got, want = tiffio.reduce_level(a, how, nodata), R.reduce_level(a, how, nodata)
            assert got.dtype == want.dtype == a.dtype and got.shape == (2, -(-shape[0] // 2), -(-shape[1] // 2))
            assert got.tobytes() == want.tobytes(), (dtype, shape, how, nodata)


def test_ties_three_way_splits_and_a_block_of_nodata_alone():
    a = np.array([[1, 2, 3, 3, 4, 5, 9, 9, 7],
                  [2, 1, 4, 5, 5, 4, 9, 9, 7],
                  [6, 6, 1, 2, 8, 9, 9, 3, 9],
                  [7, 8, 3, 4, 8, 7, 3, 9, 3]], np.uint8)[None]
    assert tiffio.reduce_level(a, "mode").tolist() == [[[1, 3, 4, 9, 7], [6, 1, 8, 9, 9]]]            # every tie goes to the first value
    assert tiffio.reduce_level(a, "mode", nodata=9).tolist() == [[[1, 3, 4, 9, 7], [6, 1, 8, 3, 3]]]  # an all-nodata block stays nodata
    assert tiffio.reduce_level(a, "average", nodata=9).tolist() == [[[2, 4, 5, 9, 7], [7, 3, 8, 3, 3]]]          # 6 / 4, 15 / 4, 18 / 4 round half up
    assert tiffio.reduce_level(a, "nearest", nodata=9).tolist() == [[[1, 3, 4, 9, 7], [6, 1, 8, 9, 9]]]
    for how in tiffio.RESAMPLINGS:
        for nd in (None, 9, 3, 300, 2.5):                 # 300 and 2.5 are no uint8 samples: every sample is valid
            assert np.array_equal(tiffio.reduce_level(a, how, nd), R.reduce_level(a, how, nd)), (how, nd)


def test_negative_int16_averages_round_half_up():
    a = np.array([[-3, -4, -1, 0, -32768, -32768, 32767, 32767, -5],
                  [-4, -4, 0, 0, -32768, -32767, 32767, 32766, -6]], np.int16)[None]
    got = tiffio.reduce_level(a, "average")
    assert got.tolist() == [[[-4, 0, -32768, 32767, -5]]]            # -15 / 4 -> -3.75 -> -4; -1 / 4 -> 0; -131071 / 4 -> -32767.75; -11 / 2 -> -5
    assert np.array_equal(got, R.reduce_level(a, "average"))
    assert tiffio.reduce_level(a, "average", nodata=-4).tolist() == [[[-3, 0, -32768, 32767, -5]]]
    assert np.array_equal(tiffio.reduce_level(a, "average", nodata=-4), R.reduce_level(a, "average", nodata=-4))


def test_nan_nodata_in_float32():
    g = np.random.default_rng(3)
    a = (g.random((2, 9, 11)) * 100).astype(np.float32)
    a[:, 2:5, 3:8] = np.nan
    a[0, 0, 0] = np.nan
    for how in ("average", "nearest"):
        got, want = tiffio.reduce_level(a, how, float("nan")), R.reduce_level(a, how, float("nan"))
        assert got.tobytes() == want.tobytes(), how
    avg = tiffio.reduce_level(a, "average", float("nan"))
    assert np.isnan(avg[0, 1, 2]) and np.isnan(avg[1, 1, 3]) and not np.isnan(avg[0, 0, 0])          # all-NaN blocks; (0, 0) has three valid samples
    assert avg[0, 0, 0] == np.float32(np.float32(np.float32(a[0, 0, 1] + a[0, 1, 0]) + a[0, 1, 1]) / np.float32(3))
    plain = tiffio.reduce_level(a, "average")              # without nodata a NaN is a sample like any other
    assert np.isnan(plain[0, 0, 0])
    assert plain.tobytes() == R.reduce_level(a, "average").tobytes()


def test_levels_are_computed_from_the_level_before():
    a = image("uint8", (1, 37, 53), 4)
    lv = tiffio.build_overviews(a, 16, "mode")
    assert [l.shape[1:] for l in lv] == R.level_shapes(37, 53, 16) == [(19, 27), (10, 14)]
    assert np.array_equal(lv[1], R.reduce_level(lv[0], "mode"))
    assert tiffio.build_overviews(a[:, :10, :10], 16, "mode") == [] and tiffio.overview_shapes(16, 16, 16) == []
    assert tiffio.overview_shapes(17, 3, 16) == [(9, 2)]


# ------------------------------------------------------------------------------------------------------------------------------ files

_HOW = {"uint8": "mode", "int8": "mode", "uint16": "average", "int16": "average", "int32": "nearest", "float32": "average"}
_PYRAMIDS = {}


def _case(dtype, C, shape, tile):
    """(array, nodata, resampling, reference pyramid), computed once per case"""
    key = (dtype, C, shape, tile)
    if key not in _PYRAMIDS:
        nodata = {"uint8": 0, "int16": -3, "float32": -9999.0}.get(dtype)
        a = image(dtype, (C, *shape), 5, nodata)
        _PYRAMIDS[key] = (a, nodata, _HOW[dtype], R.pyramid(a, tile, _HOW[dtype], nodata))
    return _PYRAMIDS[key]


def _ifds(path):
    """[(offset of the IFD, {tag: (type, count, offset of the values or None when inline)}, tags)] along the chain"""
    b = open(path, "rb").read()
    first, big, bo = tiffio._header(b, path)
    out = []
    for off in tiffio._ifd_offsets(b, path, first, big, bo):
        n = struct.unpack("<Q" if big else "<H", b[off:off + (8 if big else 2)])[0]
        base, esz, inl, fmt = (off + 8, 20, 8, "<HHQQ") if big else (off + 2, 12, 4, "<HHII")
        where = {}
        for k in range(n):
            tag, typ, cnt, val = struct.unpack(fmt, b[base + esz * k:base + esz * (k + 1)])
            size = tiffio._TYPES[typ][1] * cnt
            where[tag] = (typ, cnt, val if size > inl else None, size)
        out.append((off, where, tiffio._parse_ifd(b, path, off, big, bo), base + esz * n + inl))
    return out, big


def _check_layout(path, C, shapes, tile):
    """the COG rules: IFDs first and in decreasing size, overviews marked, data of a smaller level in front of a larger one's"""
    ifds, big = _ifds(path)
    assert len(ifds) == len(shapes) and ifds[0][0] == (16 if big else 8)
    first_tile = [t[324][0] for _, _, t, _ in ifds]
    data_start = min(min(t[324]) for _, _, t, _ in ifds)
    for k, (off, where, tags, end) in enumerate(ifds):
        assert (tags[257][0], tags[256][0]) == tuple(shapes[k])
        assert end <= data_start
        for tag, (typ, cnt, at, size) in where.items():
            assert at is None or at + size <= data_start, (k, tag)
        assert tags[322] == tags[323] == (tile,) and tile % 16 == 0
        ty, tx = -(-shapes[k][0] // tile), -(-shapes[k][1] // tile)
        assert len(tags[324]) == len(tags[325]) == C * ty * tx
        offs = np.array(tags[324])
        assert (np.diff(offs) > 0).all() and np.array_equal(offs[1:], offs[:-1] + np.array(tags[325])[:-1])          # tile order, back to back
        assert tags[259] == (5,) and tags[284] == (2 if C > 1 else 1,)
        if k == 0:
            assert 254 not in tags
        else:
            assert tags[254] == (1,) and 33550 not in tags and 33922 not in tags
            assert shapes[k][0] * shapes[k][1] < shapes[k - 1][0] * shapes[k - 1][1]
            assert first_tile[k] < first_tile[k - 1]                                 # the smaller level's data comes first
        assert tags.get(42113) == ifds[0][2].get(42113) and tags[258] == ifds[0][2][258] and tags[339] == ifds[0][2][339]
        assert tags.get(317) == ifds[0][2].get(317)
    last = ifds[0][2]
    assert last[324][-1] + last[325][-1] == os.path.getsize(path)                    # the full resolution ends the file


def _check_file(path, a, want_levels, tile, nodata):
    C = a.shape[0]
    levels = [a] + want_levels
    info = tiff_levels(path)
    assert info == [{"height": l.shape[1], "width": l.shape[2], "subfile_type": int(k > 0)} for k, l in enumerate(levels)]
    back, meta = read_tiff(path)
    assert back.dtype == a.dtype and back.tobytes() == (a[0] if C == 1 else a).tobytes()
    assert meta["geotransform"] == GT and tiff_info(path)["height"] == a.shape[1]
    for k, l in enumerate(levels):
        got = read_tiff_level(path, k)
        assert got.dtype == a.dtype and got.tobytes() == (l[0] if C == 1 else l).tobytes(), ("read_tiff_level", k)
    with pytest.raises(ValueError, match=os.path.basename(str(path))):
        read_tiff_level(path, len(levels))
    _check_layout(path, C, [l.shape[1:] for l in levels], tile)
    with Image.open(path) as im:
        assert im.n_frames == len(levels)
        for k, l in enumerate(levels):
            im.seek(k)
            got = np.array(im)
            # Pillow has no signed 8 / 16-bit modes (the bits come back as uint8 / widened to int32) and shows the first band of a
            # band-sequential image whose other bands are unspecified extra samples
            got = got.view(np.int8) if a.dtype == np.int8 else got.astype(a.dtype)
            assert got.shape == l.shape[1:] and got.tobytes() == l[0].tobytes(), ("libtiff", k)


@pytest.mark.parametrize("shape,tile", [((37, 53), 16), ((300, 517), 128), ((256, 256), 128), ((10, 10), 16)],
                         ids=["37x53-16", "300x517-128", "256x256-128", "10x10-16"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tiled_files_with_overviews_read_back_level_by_level(tmp_path, dtype, C, shape, tile):
    a, nodata, how, want = _case(dtype, C, shape, tile)
    assert len(want) == {(37, 53): 2, (300, 517): 3, (256, 256): 1, (10, 10): 0}[shape]
    for predictor in ((1,) if dtype == "float32" else (1, 2)):
        p = tmp_path / f"p{predictor}.tif"
        write_tiff(p, a, geotransform=GT, nodata=nodata, compress="lzw", predictor=predictor, tile=tile, overviews=how)
        _check_file(p, a, want, tile, nodata)
        q = tmp_path / f"q{predictor}.tif"                       # tile without overviews: the same layout with one IFD
        write_tiff(q, a, geotransform=GT, nodata=nodata, compress="lzw", predictor=predictor, tile=tile)
        _check_file(q, a, [], tile, nodata)


def test_predictor_2_runs_along_the_padded_tile_row(tmp_path):
    """the first padded sample of a row holds 0 - last: the tile's stream is that of the zero-padded block, differenced as a whole"""
    a = image("uint16", (1, 20, 21), 6)
    write_tiff(tmp_path / "a.tif", a, compress="lzw", predictor=2, tile=16)
    raw = (tmp_path / "a.tif").read_bytes()
    tags, _ = tiffio._parse_tags(raw, "a.tif")
    lib = tiffio._codecs()
    for k, block in enumerate(R.tile_blocks(a, 16)):
        d = block.copy()
        d[:, 1:] -= block[:, :-1]
        dst = np.zeros(16 * 16 * 2, np.uint8)
        enc = np.frombuffer(raw[tags[324][k]:tags[324][k] + tags[325][k]], np.uint8)
        assert lib.unet_tiff_lzw_decode(enc.ctypes.data, enc.size, dst.ctypes.data, dst.size) == dst.size
        assert dst.tobytes() == d.astype("<u2").tobytes(), k
    edge = R.tile_blocks(a, 16)[1]                               # columns 16..20 of the image, then 11 padded ones
    assert a[0, 0, 20] != 0 and edge[0, 4] == a[0, 0, 20] and not edge[:, 5:].any()


def test_bigtiff_round_trips(tmp_path):
    a, nodata, how, want = _case("int16", 3, (37, 53), 16)
    write_tiff(tmp_path / "big.tif", a, geotransform=GT, nodata=nodata, compress="lzw", predictor=2, tile=16, overviews=how, bigtiff=True)
    assert (tmp_path / "big.tif").read_bytes()[:4] == b"II+\0"
    _check_file(tmp_path / "big.tif", a, want, 16, nodata)


def test_the_file_does_not_depend_on_the_thread_count(tmp_path, monkeypatch):
    a = np.tile(image("uint16", (1, 128, 256), 7), (1, 9, 2))          # 1152 x 512 uint16: 4.5 MiB, 36 + 9 + 4 + 1 tiles
    monkeypatch.setenv("UNET_TIFF_THREADS", "1")
    write_tiff(tmp_path / "one.tif", a, compress="lzw", predictor=2, tile=128, overviews="average")
    monkeypatch.setenv("UNET_TIFF_THREADS", "4")
    write_tiff(tmp_path / "four.tif", a, compress="lzw", predictor=2, tile=128, overviews="average")
    assert (tmp_path / "one.tif").read_bytes() == (tmp_path / "four.tif").read_bytes()
    assert [l["height"] for l in tiff_levels(tmp_path / "one.tif")] == [1152, 576, 288, 144, 72]


def test_without_the_new_arguments_the_files_are_unchanged(tmp_path):
    a = image("uint8", (3, 37, 53), 8)
    write_tiff(tmp_path / "a.tif", a, geotransform=GT, nodata=0, compress="lzw", predictor=2)
    write_tiff(tmp_path / "b.tif", a, geotransform=GT, nodata=0, compress="lzw", predictor=2, tile=None, overviews=None)
    assert (tmp_path / "a.tif").read_bytes() == (tmp_path / "b.tif").read_bytes()
    assert tiff_levels(tmp_path / "a.tif") == [{"height": 37, "width": 53, "subfile_type": 0}]
    write_tiff(tmp_path / "c.tif", a)
    write_tiff(tmp_path / "d.tif", a, tile=None, overviews=None)
    assert (tmp_path / "c.tif").read_bytes() == (tmp_path / "d.tif").read_bytes()


def test_argument_errors(tmp_path):
    a, f = np.zeros((20, 20), np.uint8), np.zeros((20, 20), np.float32)
    with pytest.raises(ValueError, match="compress='lzw'"):
        write_tiff(tmp_path / "x.tif", a, tile=16)
    with pytest.raises(ValueError, match="needs tile"):
        write_tiff(tmp_path / "x.tif", a, compress="lzw", overviews="mode")
    for bad in (0, 8, 24, 100, 1040, 2048, 16.0, True, "256"):
        with pytest.raises(ValueError, match="tile must be"):
            write_tiff(tmp_path / "x.tif", a, compress="lzw", tile=bad)
    with pytest.raises(ValueError, match="float"):
        write_tiff(tmp_path / "x.tif", f, compress="lzw", tile=16, overviews="mode")
    for bad in ("cubic", "auto", 2, True):
        with pytest.raises(ValueError, match="overviews must be"):
            write_tiff(tmp_path / "x.tif", a, compress="lzw", tile=16, overviews=bad)
    with pytest.raises(ValueError, match="rows_per_strip"):
        write_tiff(tmp_path / "x.tif", a, compress="lzw", tile=16, rows_per_strip=4)
    assert tiffio.check_tiling("lzw", 256, "auto", auto=True) == (256, "auto")
    assert tiffio.resolve_overviews("auto", True) == "mode" and tiffio.resolve_overviews("auto", False) == "average"
    assert tiffio.resolve_overviews("nearest", True) == "nearest" and tiffio.resolve_overviews(None, True) is None


def test_prediction_entry_points_refuse_bad_arguments_before_the_model_is_loaded(tmp_path):
    """model=None / a model file that does not exist: anything that touched the model would raise something else than ValueError"""
    import predict as P
    raster = np.zeros((3, 64, 64), np.uint8)
    cases = [({"tile": 256}, "compress='lzw'"), ({"compress": "lzw", "overviews": "auto"}, "needs tile"),
             ({"compress": "lzw", "tile": 100}, "tile must be"), ({"compress": "lzw", "tile": 256, "overviews": "bilinear"}, "overviews must be"),
             ({"compress": "lzw", "tile": 256, "overviews": "mode", "all_classes": True}, "float"),
             ({"compress": "lzw", "tile": 256, "overviews": "mode", "regression": True}, "float")]
    for kw, match in cases:
        with pytest.raises(ValueError, match=match):
            P.predict_raster(None, raster, 64, out_path=tmp_path / "o.tif", **kw)
        kw = dict(kw)
        regression = kw.pop("regression", False)
        with pytest.raises(ValueError, match=match):
            P.save_predictions(tmp_path / "missing.pkl", tmp_path, regression, merge=True, **kw)

    def resolved(overviews, regression, all_classes, specific_class, large_file):
        return P.check_outputs(regression, all_classes, specific_class, large_file, compress="lzw", tile=256, overviews=overviews).overviews
    assert resolved("auto", False, False, None, False) == "mode" and resolved("auto", False, True, None, False) == "average"
    assert resolved("auto", True, False, None, False) == "average" and resolved("auto", False, True, None, True) == "average"
    assert resolved("auto", False, False, None, True) == "mode" and resolved("auto", False, False, 2, False) == "average"
    assert resolved("auto", False, False, 2, True) == "average"
    assert resolved("nearest", False, False, None, False) == "nearest" and resolved(None, False, False, None, False) is None


def test_tile_and_overviews_of_params_and_main_reach_save_predictions(monkeypatch):
    import params_and_main as M
    import predict
    seen = {}
    monkeypatch.setattr(predict, "save_predictions", lambda *a, **k: seen.update(k))
    for name, val in (("Create_tiles", False), ("Train", False), ("Predict", True), ("enable_extra_parameters", True),
                      ("COMPRESS", ("lzw", 2)), ("TILE", 256), ("OVERVIEWS", "auto")):
        monkeypatch.setattr(M, name, val, raising=False)
    M.main()
    assert seen["compress"] == "lzw" and seen["predictor"] == 2 and seen["tile"] == 256 and seen["overviews"] == "auto"
    seen.clear()
    monkeypatch.setattr(M, "TILE", None)
    monkeypatch.setattr(M, "OVERVIEWS", None)
    M.main()
    assert "tile" not in seen and "overviews" not in seen


# ------------------------------------------------------------------------------------------------------------------ damaged IFD chains

def _chain_file(tmp_path):
    a = image("uint8", (1, 37, 53), 9)
    p = tmp_path / "chain.tif"
    write_tiff(p, a, compress="lzw", tile=16, overviews="mode")
    ifds, big = _ifds(p)
    assert not big and len(ifds) == 3
    return p, bytearray(p.read_bytes()), ifds


def test_a_cyclic_ifd_chain_is_refused(tmp_path):
    p, raw, ifds = _chain_file(tmp_path)
    for target in (ifds[0][0], ifds[1][0], ifds[2][0]):          # the last IFD points back to IFD 0, to IFD 1, to itself
        bad = bytearray(raw)
        bad[ifds[2][3] - 4:ifds[2][3]] = struct.pack("<I", target)
        p.write_bytes(bad)
        for fn in (tiff_levels, lambda q: read_tiff_level(q, 3)):
            with pytest.raises(ValueError, match="chain.tif.*cycle"):
                fn(p)
        assert read_tiff(p)[0].shape == (37, 53) and read_tiff_level(p, 0).shape == (37, 53)          # IFD 0 itself is sound


def test_a_truncated_ifd_chain_is_refused(tmp_path):
    p, raw, ifds = _chain_file(tmp_path)
    for target in (len(raw) - 1, len(raw) + 1000, 0xFFFFFFF0):   # the next pointer of IFD 1 leaves the file
        bad = bytearray(raw)
        bad[ifds[1][3] - 4:ifds[1][3]] = struct.pack("<I", target)
        p.write_bytes(bad)
        for fn in (tiff_levels, lambda q: read_tiff_level(q, 2)):
            with pytest.raises(ValueError, match="chain.tif"):
                fn(p)
    bad = bytearray(raw)                                          # an entry count that runs past the end of the file
    bad[ifds[2][0]:ifds[2][0] + 2] = struct.pack("<H", 60000)
    p.write_bytes(bad)
    with pytest.raises(ValueError, match="chain.tif"):
        tiff_levels(p)
    p.write_bytes(raw[:ifds[1][0] + 5])                           # the file ends inside IFD 1
    with pytest.raises(ValueError, match="chain.tif"):
        tiff_levels(p)
