"""GPU suite of the class-mask post-processing (csrc/postprocess.hip, unet_amd/postprocess.py): labels, sizes, majority filter, sieve and
the prediction entry points, every result compared for exact integer equality with the NumPy restatement (tests/postprocess_ref.py).
Every device buffer -- inputs, outputs and the module's own workspace -- sits in a guard-banded allocation that is checked after every
launch group."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import predict as P  # noqa: E402

import postprocess_ref as R  # noqa: E402
from guard import canary_input, guarded, guarded_ts  # noqa: E402
from merge_schedule import FakeWorld, run_ranks  # noqa: E402

_FILL = {torch.uint8: 0xA5, torch.int32: -7, torch.int64: -7}
_LAUNCHERS = ("cc_label", "cc_sizes", "sieve_round", "majority_filter", "postprocess_counters")


def _pp():
    from unet_amd import postprocess as PP
    return PP


def _tile():
    from unet_amd import ops
    return ops.cc_tile_shape()


class Guards:
    def __init__(self):
        self.checks, self.launches = [], 0

    def alloc(self, shape, dtype, device):
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
    from unet_amd import ops
    g = Guards()
    monkeypatch.setattr(_pp(), "_alloc", g.alloc)
    for name in _LAUNCHERS:
        def wrapped(*a, _fn=getattr(ops, name), _name=name, **k):
            r = _fn(*a, **k)
            g.launches += 1
            g.check(_name)
            return r
        monkeypatch.setattr(ops, name, wrapped)
    return g


def _shapes():
    th, tw = _tile()
    return [(1, 1), (1, 197), (197, 1), (th, tw), (th + 1, tw - 1), (67, 131), (200, 136)]


_REF = {}


def _ref_labels(H, W, name, conn):
    key = (H, W, name, conn)
    if key not in _REF:
        lab = R.label_components(R.patterns(H, W)[name], conn)
        _REF[key] = (lab, R.component_sizes(lab))
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------ labels and sizes

@pytest.mark.parametrize("shape_i", range(7))
def test_labels_and_sizes_equal_the_reference(guards, shape_i):
    PP = _pp()
    H, W = _shapes()[shape_i]
    for name, m in R.patterns(H, W).items():
        for conn in (4, 8):
            ref_l, ref_s = _ref_labels(H, W, name, conn)
            d = guards.upload(m)
            lab = PP.label_components(d, conn)
            assert lab.dtype == torch.int32 and lab.shape == (H, W)
            sizes = PP.component_sizes(lab)
            assert np.array_equal(lab.cpu().numpy(), ref_l), (name, conn, H, W)
            assert np.array_equal(sizes.cpu().numpy(), ref_s), (name, conn, H, W)
            assert np.array_equal(d.cpu().numpy(), m)
            guards.clear()


def test_labels_of_host_input_come_back_as_the_same_kind(guards):
    PP = _pp()
    m = R.patterns(40, 70)["noise5"]
    ref = R.label_components(m, 8)
    a = PP.label_components(m, 8)
    b = PP.label_components(torch.from_numpy(m), 8)
    assert isinstance(a, np.ndarray) and np.array_equal(a, ref)
    assert isinstance(b, torch.Tensor) and not b.is_cuda and np.array_equal(b.numpy(), ref)
    s = PP.component_sizes(a)
    assert isinstance(s, np.ndarray) and np.array_equal(s, R.component_sizes(ref))


# ------------------------------------------------------------------------------------------------------------ majority filter

@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (67, 131), (70, 144), (33, 256), (200, 136)])
def test_majority_filter_equals_the_reference(guards, shape):
    PP = _pp()
    H, W = shape
    pats = R.patterns(H, W, seed=1)
    for name in ("noise2", "noise5", "noise256", "blocks"):
        m = pats[name]
        d = guards.upload(m)
        for k in (3, 5, 15):
            for frozen in (None, 0, 3):
                got = PP.majority_filter(d, k, frozen)
                ref = R.majority_filter(m, k, frozen)
                assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref), (name, k, frozen, shape)
                if frozen is not None:
                    assert np.array_equal(ref == frozen, m == frozen)
        assert np.array_equal(d.cpu().numpy(), m)
        guards.clear()


def test_majority_ties_and_frozen_by_hand(guards):
    PP = _pp()
    cases = [(np.array([[7, 7, 2, 4, 4]]), 5, None, [[7, 7, 4, 4, 4]]),          # centre not among the tied classes: the smallest id
             (np.array([[7, 2, 9]]), 3, None, [[7, 2, 9]]),                          # centre among the tied classes: it stays
             (np.array([[5, 5, 3, 3]]), 3, None, [[5, 5, 3, 3]]),
             (np.array([[0, 0, 0, 1, 0]]), 3, 0, [[0, 0, 0, 1, 0]]),                 # frozen pixels do not vote and do not change
             (np.array([[0, 0, 0, 1, 0]]), 3, None, [[0, 0, 0, 0, 0]]),
             (np.array([[255, 254, 255], [3, 3, 3]]), 15, None, None)]               # k larger than the raster: every window is all of it
    for m, k, frozen, want in cases:
        m = m.astype(np.uint8)
        ref = R.majority_filter(m, k, frozen)
        if want is not None:
            assert ref.tolist() == want
        got = PP.majority_filter(guards.upload(m), k, frozen)
        assert np.array_equal(got.cpu().numpy(), ref), (m.tolist(), k, frozen)
        guards.clear()


# ------------------------------------------------------------------------------------------------------------ sieve

def _min_pixels(H, W):
    return (1, 2, 8, 50, H * W + 1)


@pytest.mark.parametrize("frozen", [None, 0])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", ["noise5", "blocks"])
def test_sieve_equals_the_reference(guards, name, conn, frozen):
    PP = _pp()
    H, W = 67, 131
    m = R.patterns(H, W)[name]
    d = guards.upload(m)
    for mp in _min_pixels(H, W):
        ref, rinfo = R.sieve(m, mp, conn, 16, frozen)
        got, info = PP.sieve(d, mp, conn, 16, frozen)
        print(name, conn, frozen, mp, info)
        assert np.array_equal(got.cpu().numpy(), ref) and info == rinfo, (name, conn, frozen, mp, info, rinfo)
        assert rinfo["rounds"] <= 16 and (mp <= 1 or rinfo["merged"][-1] == 0)          # the reference settles inside the cap for this seed
        if frozen is None and mp <= 50:
            assert rinfo["small_left"] == 0 and info["small_left"] == 0
        if frozen is not None:
            assert np.array_equal(got.cpu().numpy() == frozen, m == frozen)
        again, info2 = PP.sieve(d, mp, conn, 16, frozen)
        assert torch.equal(again, got) and info2 == info                                 # two runs, equal bits
        assert np.array_equal(d.cpu().numpy(), m)                                        # the input is never written
    guards.clear()


@pytest.mark.parametrize("shape_i", [1, 2, 4, 6])
def test_sieve_on_partial_tiles_and_single_rows(guards, shape_i):
    PP = _pp()
    H, W = _shapes()[shape_i]
    for name in ("noise5", "blocks", "noise256"):
        m = R.patterns(H, W, seed=2)[name]
        d = guards.upload(m)
        for mp, conn in ((8, 4), (50, 8)):
            ref, rinfo = R.sieve(m, mp, conn)
            got, info = PP.sieve(d, mp, conn)
            assert np.array_equal(got.cpu().numpy(), ref) and info == rinfo, (name, mp, conn, info, rinfo)
        guards.clear()


def test_sieve_cap_and_single_round(guards):
    PP = _pp()
    H, W = 67, 131
    m = R.patterns(H, W)["noise5"]
    d = guards.upload(m)
    full = R.sieve(m, 50)[1]
    assert full["rounds"] > 3                                                            # so that a cap of 1 or 2 rounds ends the run
    one, merged, _ = R.sieve_round(m, 50)
    got, info = PP.sieve(d, 50, max_rounds=1)
    assert np.array_equal(got.cpu().numpy(), one)
    assert info == {"rounds": 1, "merged": [merged], "small_left": R.count_small(one, 50)} and info["small_left"] > 0
    for cap in (2, 3):
        ref, rinfo = R.sieve(m, 50, max_rounds=cap)
        got, info = PP.sieve(d, 50, max_rounds=cap)
        assert rinfo["rounds"] == cap and rinfo["merged"][-1] > 0
        assert np.array_equal(got.cpu().numpy(), ref) and info == rinfo
    hand, hinfo = PP.sieve(guards.upload(np.array([[1, 0, 2]], dtype=np.uint8)), 2)
    assert hand.cpu().numpy().tolist() == [[1, 1, 1]] and hinfo == {"rounds": 3, "merged": [2, 1, 0], "small_left": 0}
    guards.clear()


def test_pipeline_is_majority_then_sieve(guards):
    PP = _pp()
    m = R.patterns(200, 136, seed=3)["blocks"]
    for kw in (dict(majority=5, sieve=64), dict(majority=3), dict(sieve=20, connectivity=8, frozen_class=0), dict(),
               dict(majority=5, sieve=64, frozen_class=1, max_rounds=2)):
        pp = PP.PostProcess(**kw)
        ref, rinfo = R.postprocess(m, pp.majority, pp.sieve, pp.connectivity, pp.max_rounds, pp.frozen_class)
        got, info = pp.run(guards.upload(m))
        assert np.array_equal(got.cpu().numpy(), ref) and info == rinfo, kw
        host = pp(m)
        assert isinstance(host, np.ndarray) and np.array_equal(host, ref)
        guards.clear()


# ------------------------------------------------------------------------------------------------------------ prediction entry points

class GatherModel:
    """forward_windows = the real window gather into a guarded NHWC buffer; the gathered channels are the logits"""

    def __init__(self, bands, checks):
        self.n_out, self._device, self.checks = bands, torch.device("cuda"), checks

    def forward_windows(self, wb):
        z, check = guarded_ts(wb.n, wb.th, wb.tw, self.n_out, 8, 0)
        wb.write(z.buf, z.co)
        self.checks.append(check)
        return z


def _scene(H, W, bands, seed):
    """integer bands whose largest one follows a blocks-and-salt class map: the argmax of the merged prediction is a noisy class mask"""
    rng = np.random.default_rng(seed)
    target = R.patterns(H, W, seed)["blocks"] % bands
    raster = rng.integers(1, 120, (bands, H, W)).astype(np.uint8)
    for c in range(bands):
        raster[c][target == c] = 230
    return raster


def _run(monkeypatch, model, raster, world, guards, size=32, **kw):
    out, _ = run_ranks(world, lambda r: P.predict_raster(model, raster, size, 0.25, batch_size=3, **kw), monkeypatch, FakeWorld(world))
    guards.check(f"world {world}")
    checks = getattr(model, "checks", [])
    for c in checks:
        c(f"world {world}")
    checks.clear()
    return out


@pytest.mark.parametrize("kw", [{}, {"tta": "flips"}, {"blend": "gaussian"}, {"large_file": True}], ids=["plain", "tta", "gaussian", "large_file"])
def test_predict_raster_postprocess_equals_postprocess_of_predict_raster(monkeypatch, guards, kw):
    PP = _pp()
    bands, H, W = 4, 150, 105
    raster = _scene(H, W, bands, 5)
    model = GatherModel(bands, [])
    if "tta" in kw:          # test-time augmentation needs a model with forward_tta: a small xresnet18 on 64 px windows
        model, kw = _model("xresnet18", bands, bands, 64, seed=3), dict(kw, size=64)
    pp = PP.PostProcess(majority=3, sieve=300, connectivity=8)
    plain = _run(monkeypatch, model, raster, 1, guards, **kw)
    assert guards.launches == 0                                                          # postprocess=None: no launch of this family
    none = _run(monkeypatch, model, raster, 1, guards, postprocess=None, **kw)
    assert guards.launches == 0 and none.dtype == np.uint8 and np.array_equal(none, plain)
    ref, rinfo = R.postprocess(plain, 3, 300, 8)
    if "tta" not in kw:
        assert rinfo["merged"][0] > 0 and not np.array_equal(ref, plain)                 # the scene has something to clean
    timing = {}
    one = _run(monkeypatch, model, raster, 1, guards, postprocess=pp, timing=timing, **kw)
    assert one.dtype == np.uint8 and np.array_equal(one, ref) and np.array_equal(one, pp(plain))
    assert timing["postprocess"] == rinfo and timing["postprocess_seconds"] > 0
    as_dict = _run(monkeypatch, model, raster, 1, guards, postprocess={"majority": 3, "sieve": 300, "connectivity": 8}, **kw)
    assert np.array_equal(as_dict, one)
    for world in (2, 3):
        got = _run(monkeypatch, model, raster, world, guards, postprocess=pp, **kw)
        assert np.array_equal(got, one), world


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


def test_save_predictions_postprocess_on_tile_files_with_class_zero(tmp_path, guards):
    import create_tiles_unet as T
    from unet_amd.tiffio import read_tiff, write_tiff
    PP = _pp()
    size = 64
    model = _model("xresnet18", 4, 3, size, seed=11)
    img = np.random.default_rng(5).integers(1, 250, (4, 200, 170)).astype(np.uint8)
    rpath = tmp_path / "scene.tif"
    write_tiff(rpath, img, geotransform=(400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5))
    pkl = _export(tmp_path, model, 3, size)
    tiles = tmp_path / "cut"
    T.split_raster(rpath, None, tiles, patch_size=size, patch_overlap=0.2, split=[1], max_empty=0.9)
    pp = PP.PostProcess(majority=3, sieve=30, frozen_class=0)
    plain = P.predict_raster(model, rpath, size, 0.2, max_empty=0.9, batch_size=5)
    ref, rinfo = R.postprocess(plain, 3, 30, 4, 16, 0)
    direct = P.predict_raster(model, rpath, size, 0.2, max_empty=0.9, batch_size=5, postprocess=pp, class_zero=True, out_path=tmp_path / "direct.tif")
    assert np.array_equal(direct, ref) and np.array_equal(direct == 0, plain == 0)
    assert np.array_equal(read_tiff(tmp_path / "direct.tif")[0], ref.astype(np.int16) - 1)          # store_tif shifts AFTER the clean-up
    timing = {}
    f = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, AOI="b", validation_vision=False, batch_size=5, class_zero=True,
                           postprocess=pp, timing=timing)
    assert np.array_equal(read_tiff(f)[0], ref.astype(np.int16) - 1)
    assert timing["postprocess"] == rinfo
    f0 = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, AOI="c", validation_vision=False, batch_size=5)
    assert np.array_equal(read_tiff(f0)[0], plain)                                                   # postprocess=None: today's output
    guards.check("end")
