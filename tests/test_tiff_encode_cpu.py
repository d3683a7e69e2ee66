"""The host side of compressed GeoTIFF output: unet_tiff_lzw_encode (csrc/tiff_codecs.hip) against the rule in plain Python
(tests/tiff_lzw_ref.py) and against the decoder, tiffio.write_tiff(compress="lzw") through read_tiff and through libtiff (Pillow), the
encoder under AddressSanitizer / UBSan as a stand-alone program (tests/fuzz/tiff_encode_fuzz.cpp), and split_raster's pass-through."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import tiff_lzw_ref as R  # noqa: E402

from unet_amd import tiffio  # noqa: E402
from unet_amd.tiffio import read_tiff, write_tiff  # noqa: E402

REPO = Path(__file__).resolve().parent.parent
# strip lengths at which the table reaches 511, 1023, 2047 or 4094 entries at or near the end of a strip of random bytes
EDGE_LENGTHS = [*range(1, 40), *range(250, 262), *range(760, 775), *range(1785, 1800), *range(3830, 3850), *range(4085, 4100)]


def _encode(data: bytes, cap=None, slack=64):
    """(return value, bytes written, the `slack` bytes behind dst + cap) of the host encoder"""
    lib = tiffio._codecs()
    n = len(data)
    cap = R.cap(n) if cap is None else cap
    src = np.frombuffer(data, dtype=np.uint8) if n else np.zeros(1, np.uint8)
    dst = np.full(cap + slack, 0xA5, dtype=np.uint8)
    got = lib.unet_tiff_lzw_encode(src.ctypes.data, n, dst.ctypes.data, cap)
    return got, dst[:max(got, 0)].tobytes(), dst[cap:]


def _decode(enc: bytes, n: int) -> bytes:
    lib = tiffio._codecs()
    src = np.frombuffer(enc, dtype=np.uint8)
    dst = np.empty(max(n, 1), dtype=np.uint8)
    got = lib.unet_tiff_lzw_decode(src.ctypes.data, src.size, dst.ctypes.data, n)
    assert got == n, (got, n)
    return dst[:n].tobytes()


def _check(data: bytes, what):
    got, enc, behind = _encode(data)
    assert 0 < got <= R.cap(len(data)), (what, got, R.cap(len(data)))
    assert enc == R.encode(data), what
    assert _decode(enc, len(data)) == data, what
    assert (behind == 0xA5).all(), what
    return enc


def test_cap_is_the_stated_formula_in_all_three_places():
    lib = tiffio._codecs()
    lib.unet_tiff_lzw_cap.restype, lib.unet_tiff_lzw_cap.argtypes = __import__("ctypes").c_longlong, [__import__("ctypes").c_longlong]
    for n in (0, 1, 2, 3835, 3836, 3837, 65536, 80000, 2 ** 31 - 1):
        want = (3 * (n + n // 3836 + 4) + 1) // 2
        assert R.cap(n) == tiffio.lzw_cap(n) == lib.unet_tiff_lzw_cap(n) == want


def test_every_short_length_of_random_bytes():
    g = np.random.default_rng(1)
    for n in range(0, 601):
        _check(g.integers(0, 256, n, dtype=np.uint8).tobytes(), n)
    assert _encode(b"")[1] == bytes([0x80, 0x40, 0x40])          # Clear, EOI at 9 bits, zero padding


def test_lengths_at_which_the_table_fills_near_the_end():
    g = np.random.default_rng(2)
    for n in EDGE_LENGTHS:
        _check(g.integers(0, 256, n, dtype=np.uint8).tobytes(), n)


def test_planes_constant_alternating_random_and_masks():
    g = np.random.default_rng(3)
    const = _check(bytes([7]) * (64 * 4100), "constant")
    assert len(const) < 1200                                   # very long strings: 262400 bytes in under 1.2 KB
    alt = np.zeros((64, 300), np.uint8)
    alt[:, ::2] = 200
    _check(alt.tobytes(), "alternating")
    rand = g.integers(0, 256, 96 * 300, dtype=np.uint8).tobytes()
    enc = _check(rand, "random 96 x 300")
    assert len(rand) // 3836 >= 5 and len(enc) > len(rand)     # the table fills several times: Clear goes out mid-strip
    for noise in (0.0, 0.02):
        m = R.blob_mask(200, 333, noise=noise, seed=4)
        e = _check(m.tobytes(), ("blob", noise))
        assert len(e) * 4 < m.size


def test_a_destination_that_is_too_small_returns_minus_one_and_nothing_is_written_past_it():
    g = np.random.default_rng(5)
    for n in (1, 37, 5000):
        data = g.integers(0, 256, n, dtype=np.uint8).tobytes()          # incompressible
        need = len(R.encode(data))
        for cap in (need - 1, need // 2, 1, 0):
            got, _, behind = _encode(data, cap=cap)
            assert got == -1, (n, cap, got)
            assert (behind == 0xA5).all(), (n, cap)
        got, enc, behind = _encode(data, cap=need)               # exactly enough
        assert got == need and enc == R.encode(data) and (behind == 0xA5).all()


def _image(dtype, shape, seed):
    g = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (g.random(shape) * 3 - 1).astype(dt)
    info = np.iinfo(dt)
    a = g.integers(info.min, int(info.max) + 1, shape, dtype=np.int64)
    a[..., :2] = [info.min, info.max]                                   # full-range values: the differences of Predictor 2 wrap
    return a.astype(dt)


@pytest.mark.parametrize("dtype", ["uint8", "int8", "uint16", "int16", "int32", "float32"])
@pytest.mark.parametrize("shape", [(37, 53), (3, 37, 53)])
def test_write_tiff_lzw_round_trips(tmp_path, dtype, shape):
    a = _image(dtype, shape, 6)
    H = shape[-2]
    gt = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)
    geokeys = {34735: (1, 1, 0, 1, 3072, 0, 1, 32632), 34737: ("WGS 84 / UTM zone 32N|",)}
    predictors = (1,) if np.dtype(dtype).kind == "f" else (1, 2)
    for predictor in predictors:
        for rps in (1, 7, H, None):
            for big in (False, True):
                p = tmp_path / "t.tif"
                write_tiff(p, a, geotransform=gt, tags=geokeys, nodata=-9999, bigtiff=big, compress="lzw", predictor=predictor, rows_per_strip=rps)
                back, meta = read_tiff(p)
                assert back.dtype == a.dtype and np.array_equal(back, a), (predictor, rps, big)
                assert meta["geotransform"] == gt and meta["nodata"] == -9999.0
                assert meta["tags"][34735] == geokeys[34735] and meta["tags"][34737] == geokeys[34737]
                raw = p.read_bytes()
                assert raw[2] == (43 if big else 42)
                tags, _ = tiffio._parse_tags(raw, p)
                assert tags[259] == (5,) and tags.get(317, (1,)) == (predictor,) and tags[284] == ((2,) if a.ndim == 3 else (1,))
                want_rps = H if rps is None else rps                # 53 samples a row: the 64 KiB default holds the whole plane
                assert tags[278] == (want_rps,)
                spp = -(-H // want_rps)
                assert len(tags[273]) == len(tags[279]) == spp * (a.shape[0] if a.ndim == 3 else 1)


def test_default_rows_per_strip_is_the_largest_that_fits_64_kib(tmp_path):
    a = np.zeros((40, 5000), np.uint16)
    write_tiff(tmp_path / "a.tif", a, compress="lzw")
    tags, _ = tiffio._parse_tags((tmp_path / "a.tif").read_bytes(), "a")
    assert tags[278] == (6,)                                           # 6 * 10000 <= 65536 < 7 * 10000
    b = np.zeros((3, 20000), np.float32)                                # one row is 80 KB: a strip is still one row
    write_tiff(tmp_path / "b.tif", b, compress="lzw")
    tags, _ = tiffio._parse_tags((tmp_path / "b.tif").read_bytes(), "b")
    assert tags[278] == (1,) and np.array_equal(read_tiff(tmp_path / "b.tif")[0], b)


def test_libtiff_reads_the_files(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    for dtype, predictor in (("uint8", 1), ("uint8", 2), ("uint16", 1), ("uint16", 2), ("float32", 1)):
        a = _image(dtype, (61, 47), 7)
        if dtype == "uint8":
            a = R.blob_mask(61, 47, noise=0.05, seed=7)
            a[0, :2] = [0, 255]
        for rps in (None, 5):
            p = tmp_path / f"{dtype}_{predictor}.tif"
            write_tiff(p, a, compress="lzw", predictor=predictor, rows_per_strip=rps, geotransform=(1.0, 2.0, 0.0, 3.0, 0.0, -2.0))
            with Image.open(p) as im:
                got = np.array(im)
            assert got.dtype == a.dtype and np.array_equal(got, a), (dtype, predictor, rps)


def test_compress_none_is_byte_identical_to_the_old_call(tmp_path):
    a = _image("uint8", (3, 37, 53), 8)
    write_tiff(tmp_path / "old.tif", a, geotransform=(1.0, 2.0, 0.0, 3.0, 0.0, -2.0), nodata=0)
    write_tiff(tmp_path / "new.tif", a, geotransform=(1.0, 2.0, 0.0, 3.0, 0.0, -2.0), nodata=0, compress=None, predictor=1, rows_per_strip=None)
    assert (tmp_path / "old.tif").read_bytes() == (tmp_path / "new.tif").read_bytes()


def test_argument_errors():
    a = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError, match="compress"):
        write_tiff("x.tif", a, compress="deflate")
    with pytest.raises(ValueError, match="predictor"):
        write_tiff("x.tif", a, compress="lzw", predictor=2)               # floats
    with pytest.raises(ValueError, match="predictor"):
        write_tiff("x.tif", a.astype(np.uint8), compress="lzw", predictor=3)
    with pytest.raises(ValueError, match="predictor"):
        write_tiff("x.tif", a.astype(np.uint8), predictor=2)               # without compress
    with pytest.raises(ValueError, match="rows_per_strip"):
        write_tiff("x.tif", a.astype(np.uint8), compress="lzw", rows_per_strip=0)
    assert not Path("x.tif").exists()


def test_prediction_entry_points_refuse_bad_arguments_before_the_model_is_loaded(tmp_path):
    """model=None / a model file that does not exist: anything that touched the model would raise something else than ValueError"""
    import predict as P
    raster = np.ones((3, 64, 64), np.uint8)
    missing = tmp_path / "no_such_model.pkl"
    for kw, msg in (({"compress": "deflate"}, "compress"), ({"compress": "lzw", "predictor": 3}, "predictor"), ({"predictor": 2}, "predictor"),
                    ({"compress": "lzw", "predictor": 2, "all_classes": True}, "predictor"),
                    ({"compress": "lzw", "predictor": 2, "specific_class": 1}, "predictor")):
        with pytest.raises(ValueError, match=msg):
            P.predict_raster(None, raster, 32, out_path=tmp_path / "o.tif", **kw)
        with pytest.raises(ValueError, match=msg):
            P.save_predictions(missing, tmp_path, False, merge=True, **kw)
    with pytest.raises(ValueError, match="predictor"):
        P.predict_raster(None, raster, 32, out_path=tmp_path / "o.tif", regression=True, compress="lzw", predictor=2)
    with pytest.raises(ValueError, match="predictor"):
        P.save_predictions(missing, tmp_path, True, merge=False, compress="lzw", predictor=2)
    with pytest.raises(ValueError, match="return_array"):
        P.predict_raster(None, raster, 32, return_array=False)
    assert P.check_outputs(False, True, None, True).floats is False          # the int8 merge of large_file holds integers: Predictor 2 is fine


def test_compress_setting_of_params_and_main_reaches_save_predictions(monkeypatch):
    import params_and_main as M
    import predict
    assert M.COMPRESS is None
    calls = []
    monkeypatch.setattr(predict, "save_predictions", lambda *a, **k: calls.append(k))
    for name, v in (("Create_tiles", False), ("Train", False), ("Predict", True), ("enable_extra_parameters", True)):
        monkeypatch.setattr(M, name, v)
    M.main()
    monkeypatch.setattr(M, "COMPRESS", "lzw")
    M.main()
    monkeypatch.setattr(M, "COMPRESS", ("lzw", 2))
    M.main()
    assert "compress" not in calls[0] and calls[1]["compress"] == "lzw" and calls[1]["predictor"] == 1
    assert (calls[2]["compress"], calls[2]["predictor"]) == ("lzw", 2)


def test_threaded_and_single_threaded_paths_write_the_same_file(tmp_path, monkeypatch):
    a = np.tile(R.blob_mask(256, 1024, noise=0.02, seed=9), (5, 2)).astype(np.uint16)      # 1280 x 2048 uint16 = 5 MiB, 80 strips
    a[::7, ::5] += 300
    monkeypatch.setenv("UNET_TIFF_THREADS", "1")
    write_tiff(tmp_path / "one.tif", a, compress="lzw", predictor=2)
    monkeypatch.setenv("UNET_TIFF_THREADS", "6")
    write_tiff(tmp_path / "six.tif", a, compress="lzw", predictor=2)
    assert (tmp_path / "one.tif").read_bytes() == (tmp_path / "six.tif").read_bytes()
    assert np.array_equal(read_tiff(tmp_path / "six.tif")[0], a)
    assert (tmp_path / "six.tif").stat().st_size * 8 < a.nbytes


def test_the_encoder_stays_inside_its_buffers_under_the_sanitizers(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no host compiler")
    exe = tmp_path / "tiff_encode_fuzz"
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        str(REPO / "tests" / "fuzz" / "tiff_encode_fuzz.cpp"), "-x", "c++", str(REPO / "unet_amd" / "csrc" / "tiff_codecs.hip"),
                        "-I", str(REPO / "include"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout or r.returncode != 0 and "asan" in (r.stderr + r.stdout).lower():
        pytest.skip("this compiler has no sanitizer runtime: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for seed in (1, 2):
        r = subprocess.run([str(exe), "240", str(seed)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        words = r.stdout.split()
        got = dict(zip(words[0::2], map(int, words[1::2])))
        assert got["encoded"] == 240 and got["refused"] >= 3 * 240, r.stdout


def test_split_raster_writes_lzw_tiles_that_read_back_equal(tmp_path):
    import create_tiles_unet as T
    g = np.random.default_rng(10)
    img = g.integers(1, 250, (3, 300, 260)).astype(np.uint16)
    mask = R.blob_mask(300, 260, seed=10) + 1
    gt = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)
    write_tiff(tmp_path / "scene.tif", img, geotransform=gt)
    write_tiff(tmp_path / "mask.tif", mask, geotransform=gt)
    plain = T.split_raster(tmp_path / "scene.tif", tmp_path / "mask.tif", tmp_path / "plain", patch_size=128, patch_overlap=0.2, seed=1)
    packed = T.split_raster(tmp_path / "scene.tif", tmp_path / "mask.tif", tmp_path / "lzw", patch_size=128, patch_overlap=0.2, seed=1,
                            compress="lzw", predictor=2)
    assert plain == packed
    files = sorted(p.relative_to(tmp_path / "plain") for p in (tmp_path / "plain").rglob("*.tif"))
    assert len(files) >= 8 and files == sorted(p.relative_to(tmp_path / "lzw") for p in (tmp_path / "lzw").rglob("*.tif"))
    for rel in files:
        a, ma = read_tiff(tmp_path / "plain" / rel)
        b, mb = read_tiff(tmp_path / "lzw" / rel)
        assert a.dtype == b.dtype and np.array_equal(a, b) and ma["geotransform"] == mb["geotransform"], rel
        tags, _ = tiffio._parse_tags((tmp_path / "lzw" / rel).read_bytes(), rel)
        assert tags[259] == (5,) and tags[317] == (2,)
