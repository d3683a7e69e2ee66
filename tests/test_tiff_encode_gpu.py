"""GPU suite of compressed GeoTIFF output (csrc/tiff_encode.hip, unet_amd/tiffenc.py, the compress= seam of predict.py): the device
encoder's bytes equal the host encoder's strip by strip (which tests/test_tiff_encode_cpu.py ties to the rule in tests/tiff_lzw_ref.py),
the files equal write_tiff's byte for byte whatever the band size, and the prediction entry points write the content of their
uncompressed runs.  Every device buffer of the encoder -- scratch slots, sizes, offsets, compact bytes -- sits in a guard-banded
allocation that is checked after every launch; sources of sliced views sit between canaries."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import predict as P  # noqa: E402

import tiff_lzw_ref as R  # noqa: E402
from guard import canary_input, guarded  # noqa: E402

from unet_amd import tiffio  # noqa: E402
from unet_amd.tiffio import read_tiff, write_tiff  # noqa: E402

_FILL = {torch.uint8: 0xA5, torch.int32: -7, torch.int64: -7}
_LAUNCHERS = ("tiff_encode_strips", "tiff_compact_strips")


class Guards:
    def __init__(self):
        self.checks, self.launches = [], 0

    def alloc(self, shape, dtype, device="cuda"):
        t, c = guarded(shape, dtype, device, _FILL[dtype])
        self.checks.append(c)
        return t

    def upload(self, a: np.ndarray) -> torch.Tensor:
        t, c = canary_input(torch.from_numpy(np.ascontiguousarray(a)))
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


def _host_strips(a: np.ndarray, rps: int, predictor: int):
    """the host encoder's stream of every strip of a [P, H, W] array, in file order"""
    lib = tiffio._codecs()
    out = []
    for p in range(a.shape[0]):
        for r0 in range(0, a.shape[1], rps):
            src = tiffio._predicted_le(a[p, r0:r0 + rps], predictor)
            dst = np.empty(tiffio.lzw_cap(src.size), dtype=np.uint8)
            got = lib.unet_tiff_lzw_encode(src.ctypes.data, src.size, dst.ctypes.data, dst.size)
            assert got > 0
            out.append(dst[:got].tobytes())
    return out


def _device_strips(g: Guards, t: torch.Tensor, rps: int, predictor: int):
    """launch A + launch B on guard-banded buffers -> ([strip bytes], compact bytes).  The compact buffer has exactly the total size."""
    from unet_amd import ops
    Pn, H, W = t.shape
    n = Pn * -(-H // rps)
    slot = ops.tiff_slot_bytes(rps * W * t.element_size())
    assert slot % 16 == 0 and slot >= R.cap(rps * W * t.element_size())
    scratch, sizes = g.alloc((n * slot,), torch.uint8), g.alloc((n,), torch.int32)
    assert ops.tiff_encode_strips(t, rps, predictor, 0, n, scratch, sizes) == slot
    sz = sizes.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert (sz > 0).all() and (sz <= slot).all(), sz
    offs = g.alloc((n,), torch.int64)
    offs.copy_(torch.from_numpy(np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.int64)))
    compact = g.alloc((int(sz.sum()),), torch.uint8)
    ops.tiff_compact_strips(scratch, slot, sizes, offs, n, compact)
    raw = scratch.cpu().numpy()
    return [raw[j * slot:j * slot + int(sz[j])].tobytes() for j in range(n)], compact.cpu().numpy().tobytes()


def _same(g: Guards, a: np.ndarray, rps: int, predictor: int = 1, t: torch.Tensor = None, what=""):
    """device == host, strip by strip, sizes and content; compact == their concatenation"""
    a3 = a[None] if a.ndim == 2 else a
    if t is None:
        t = g.upload(a3)
    want = _host_strips(a3, rps, predictor)
    got, compact = _device_strips(g, t, rps, predictor)
    assert [len(s) for s in got] == [len(s) for s in want], (what, rps, predictor)
    for j, (x, y) in enumerate(zip(got, want)):
        assert x == y, (what, "strip", j, rps, predictor)
    assert compact == b"".join(want), (what, "compact")
    g.clear()


def test_smallest_planes_and_single_rows(guards):
    rng = np.random.default_rng(1)
    _same(guards, np.array([[9]], np.uint8), 1, what="1 x 1")
    for W in (2, 3, 63, 64, 65, 257):
        _same(guards, rng.integers(0, 256, (1, W), dtype=np.uint8), 1, what=W)
        _same(guards, rng.integers(0, 4, (1, W), dtype=np.uint8), 1, what=(W, "few values"))
    _same(guards, rng.integers(0, 7, (1, 23, 65), dtype=np.uint8), 7, what="short last strip")


def test_random_constant_and_alternating_planes_as_one_strip(guards):
    rng = np.random.default_rng(2)
    _same(guards, rng.integers(0, 256, (96, 300), dtype=np.uint8), 96, what="random: Clear mid-strip, all code widths")
    _same(guards, np.full((64, 4100), 7, np.uint8), 64, what="constant")
    alt = np.zeros((64, 300), np.uint8)
    alt[:, ::2] = 200
    _same(guards, alt, 64, what="alternating")


@pytest.mark.parametrize("rps", [1, 16, 200])
def test_blob_mask(guards, rps):
    _same(guards, R.blob_mask(200, 333, noise=0.0, seed=3), rps, what="blob")
    _same(guards, R.blob_mask(200, 333, noise=0.02, seed=3), rps, what="blob + salt")


@pytest.mark.parametrize("lengths", [range(250, 262), range(760, 775), range(1785, 1800), range(3830, 3850)], ids=["511", "1023", "2047", "4094"])
def test_strip_lengths_at_which_the_table_fills_near_the_end(guards, lengths):
    rng = np.random.default_rng(4)
    for n in lengths:
        _same(guards, rng.integers(0, 256, (1, n), dtype=np.uint8), 1, what=n)


def test_planes_are_independent_and_in_order(guards):
    rng = np.random.default_rng(5)
    _same(guards, rng.random((5, 37, 53)).astype(np.float32), 7, what="float32 planes")
    _same(guards, rng.random((5, 37, 53)).astype(np.float32), 37, what="float32 planes, one strip each")
    _same(guards, rng.integers(0, 5, (5, 37, 53), dtype=np.uint8), 7, what="uint8 planes")


def test_predictor_2_wraps_per_sample(guards):
    rng = np.random.default_rng(6)
    for dt in (np.uint8, np.uint16, np.int16, np.int32):
        info = np.iinfo(dt)
        a = rng.integers(info.min, int(info.max) + 1, (2, 21, 67), dtype=np.int64).astype(dt)
        a[..., :2] = [info.min, info.max]
        smooth = (np.add.outer(np.arange(21), np.arange(67)) * 3 + 250).astype(dt)[None]
        for rps in (1, 5):
            _same(guards, a, rps, 2, what=(dt.__name__, "random"))
            _same(guards, smooth, rps, 2, what=(dt.__name__, "ramp"))
    _same(guards, R.blob_mask(40, 130, noise=0.02, seed=6), 8, 2, what="uint8 mask")


def test_row_sliced_and_plane_views_are_read_in_place(guards):
    rng = np.random.default_rng(7)
    tall = rng.integers(0, 200, (50, 77), dtype=np.uint8)
    t = guards.upload(tall)
    _same(guards, tall[3:40], 5, t=t[3:40][None], what="row slice")
    cube = rng.integers(0, 30000, (4, 50, 61)).astype(np.uint16)
    t = guards.upload(cube)
    v = t[2, 7:44]
    assert not v.is_contiguous() or v.data_ptr() != t.data_ptr()
    _same(guards, cube[2, 7:44], 6, 2, t=v[None], what="one plane, row slice")
    t = guards.upload(cube)
    _same(guards, cube[1:3, :33], 33, t=t[1:3, :33], what="two planes of four, rows cut")


def test_the_file_does_not_depend_on_the_band_size_and_equals_the_host_writers(guards, tmp_path):
    from unet_amd.tiffenc import write_tiff_device
    gt = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)
    a = np.stack([R.blob_mask(45, 130, noise=0.02, seed=s) for s in range(3)]).astype(np.uint16) * 257
    t = guards.upload(a)
    write_tiff(tmp_path / "host.tif", a, geotransform=gt, nodata=0, compress="lzw", predictor=2, rows_per_strip=4)
    want = (tmp_path / "host.tif").read_bytes()
    for band in (1, 3, None):
        tm = {}
        size = write_tiff_device(tmp_path / "dev.tif", t, geotransform=gt, nodata=0, predictor=2, rows_per_strip=4, band_strips=band, timing=tm)
        assert (tmp_path / "dev.tif").read_bytes() == want, band
        assert size == len(want) and set(tm) == {"encode_seconds", "copy_seconds", "file_seconds"}
        guards.check(f"band {band}")
    back, meta = read_tiff(tmp_path / "dev.tif")
    assert np.array_equal(back, a) and meta["geotransform"] == gt and meta["nodata"] == 0.0
    f = torch.from_numpy(np.random.default_rng(8).random((2, 19, 300)).astype(np.float32)).cuda()
    write_tiff(tmp_path / "hf.tif", f.cpu().numpy(), compress="lzw")
    write_tiff_device(tmp_path / "df.tif", f, band_strips=1)
    assert (tmp_path / "df.tif").read_bytes() == (tmp_path / "hf.tif").read_bytes()
    with pytest.raises(ValueError, match="predictor"):
        write_tiff_device(tmp_path / "bad.tif", f, predictor=2)
    guards.clear()


# ------------------------------------------------------------------------------------------------------------ the prediction entry points

def _model(arch, n_in, n_out, size, seed=0):
    from unet_amd.model import HipDynamicUnet
    torch.manual_seed(seed)
    m = HipDynamicUnet(arch, n_in, n_out, (size, size))
    m.eval()
    return m


def _export(tmp_path, model, n_out, size):
    from unet_amd.learner import CrossEntropyLossFlat, DataLoaders, Learner, TileDataset
    dls = DataLoaders(TileDataset([np.zeros((4, size, size), np.uint8)], None, "int8"), None, 1, device="cuda",
                      vocab=[str(i) for i in range(n_out)])
    learn = Learner(dls, model, loss_func=CrossEntropyLossFlat(axis=1), path=tmp_path)
    pkl = tmp_path / "m.pkl"
    learn.export(pkl)
    return pkl


SIZE, GT = 64, (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """the tiny model and raster of the end-to-end cases: (model, raster path, exported learner, folder of its tiles)"""
    import create_tiles_unet as T
    d = tmp_path_factory.mktemp("lzw_scene")
    model = _model("xresnet18", 4, 3, SIZE, seed=11)
    img = np.random.default_rng(5).integers(1, 250, (4, 200, 170)).astype(np.uint8)
    write_tiff(d / "scene.tif", img, geotransform=GT)
    pkl = _export(d, model, 3, SIZE)
    T.split_raster(d / "scene.tif", None, d / "cut", patch_size=SIZE, patch_overlap=0.2, split=[1], max_empty=0.9)
    return model, d / "scene.tif", pkl, d / "cut" / "img_tiles"


def _same_content(lzw, plain):
    a, ma = read_tiff(lzw)
    b, mb = read_tiff(plain)
    assert a.dtype == b.dtype and np.array_equal(a, b)
    assert ma["geotransform"] == mb["geotransform"] and ma.get("nodata") == mb.get("nodata") and ma["tags"] == mb["tags"]
    tags, _ = tiffio._parse_tags(open(lzw, "rb").read(), lzw)
    assert tags[259] == (5,)
    return a


@pytest.mark.parametrize("kw", [{}, {"class_zero": True}, {"all_classes": True}, {"regression": True}, {"specific_class": 1},
                                {"postprocess": {"majority": 3, "sieve": 30}, "class_zero": True}, {"large_file": True}],
                         ids=["mask", "class_zero", "all_classes", "regression", "specific_class", "postprocess", "large_file"])
def test_predict_raster_lzw_writes_the_content_of_the_uncompressed_run(guards, scene, tmp_path, kw):
    model, rpath, _, _ = scene
    run = lambda **k: P.predict_raster(model, rpath, SIZE, 0.2, max_empty=0.9, batch_size=5, **kw, **k)
    plain = run(out_path=tmp_path / "plain.tif")
    tm = {}
    predictor = 1 if ("all_classes" in kw or "regression" in kw or "specific_class" in kw) else 2
    out = run(out_path=tmp_path / "lzw.tif", compress="lzw", predictor=predictor, timing=tm)
    assert out.dtype == plain.dtype and np.array_equal(out, plain)
    stored = _same_content(tmp_path / "lzw.tif", tmp_path / "plain.tif")
    if "class_zero" in kw:
        assert stored.dtype == np.int16 and np.array_equal(stored, out.astype(np.int16) - 1)          # shifted after the clean-up
    else:
        assert np.array_equal(stored, out)
    if "regression" in kw:
        assert read_tiff(tmp_path / "lzw.tif")[1]["nodata"] == -9999.0
    assert tm["write_seconds"] > 0 and tm["file_bytes"] == (tmp_path / "lzw.tif").stat().st_size
    # the device encoder took every path but the int8 merge, which is host numpy; both write the host writer's file
    assert (guards.launches > 0) == ("large_file" not in kw)
    write_tiff(tmp_path / "host.tif", stored, geotransform=GT, nodata=-9999 if "regression" in kw else None, compress="lzw", predictor=predictor,
               tags=read_tiff(rpath)[1]["tags"])
    assert (tmp_path / "host.tif").read_bytes() == (tmp_path / "lzw.tif").read_bytes()
    assert run(out_path=tmp_path / "none.tif", compress="lzw", predictor=predictor, return_array=False) is None
    assert (tmp_path / "none.tif").read_bytes() == (tmp_path / "lzw.tif").read_bytes()
    guards.clear()


def test_save_predictions_lzw_merged_and_per_tile(guards, scene, tmp_path):
    import shutil
    model, rpath, pkl, tiles = scene
    folders = {}
    for name in ("plain", "lzw"):                       # save_predictions writes next to the tile folder: one copy of it per run
        folders[name] = tmp_path / name / "img_tiles"
        shutil.copytree(tiles, folders[name])
    tm = {}
    f0 = P.save_predictions(pkl, folders["plain"], False, merge=True, AOI="a", validation_vision=False, batch_size=5)
    f1 = P.save_predictions(pkl, folders["lzw"], False, merge=True, AOI="a", validation_vision=False, batch_size=5, compress="lzw", predictor=2,
                            timing=tm)
    merged = _same_content(f1, f0)
    assert guards.launches > 0 and tm["file_bytes"] == os.path.getsize(f1) and tm["write_seconds"] > 0
    assert np.array_equal(merged, P.predict_raster(model, rpath, SIZE, 0.2, max_empty=0.9, batch_size=5))
    n = guards.launches
    d0 = P.save_predictions(pkl, folders["plain"], False, merge=False, validation_vision=False, batch_size=5)
    d1 = P.save_predictions(pkl, folders["lzw"], False, merge=False, validation_vision=False, batch_size=5, compress="lzw")
    names = sorted(p.name for p in d0.glob("*.tif"))
    assert len(names) == len(list(tiles.glob("*.tif"))) and names == sorted(p.name for p in d1.glob("*.tif"))
    for name in names:
        _same_content(d1 / name, d0 / name)
    assert guards.launches == n                         # per-tile outputs go through the host encoder
    guards.clear()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, state, rpath, out_path, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      UNET_DIST_BACKEND="gloo", UNET_FORCE_DEVICE="0")
    import torch.distributed as dist
    import predict as P
    from unet_amd.model import HipDynamicUnet
    model = HipDynamicUnet("xresnet18", 4, 3, (SIZE, SIZE), device="cuda:0")
    model.load_state_dict(torch.load(state))
    model.eval()
    tm = {}
    a = P.predict_raster(model, rpath, SIZE, 0.2, max_empty=0.9, batch_size=5, out_path=out_path, compress="lzw", predictor=2, class_zero=True,
                         timing=tm)
    assert (a is None) == (rank != 0)
    q.put((rank, tm["active_ranks"], tm["strip_rows"]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_write_the_one_rank_file(scene, tmp_path):
    import torch.multiprocessing as mp
    model, rpath, _, _ = scene
    P.predict_raster(model, rpath, SIZE, 0.2, max_empty=0.9, batch_size=5, out_path=tmp_path / "one.tif", compress="lzw", predictor=2,
                     class_zero=True, return_array=False)
    state = tmp_path / "w.pt"
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, state)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, str(state), str(rpath), str(tmp_path / "two.tif"), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=120)
    assert [r[:2] for r in res] == [(0, 2), (1, 2)] and res[0][2] + res[1][2] == 200, res
    assert (tmp_path / "two.tif").read_bytes() == (tmp_path / "one.tif").read_bytes()
