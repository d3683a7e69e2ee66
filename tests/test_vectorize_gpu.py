"""GPU suite of the polygonizer (csrc/vectorize.hip, unet_amd/vectorize.py): every array of Polygons compared for exact equality with the
plain-Python restatement of the rules (tests/vectorize_ref.py), checks that do not go through that reference, and the prediction entry
points.  Every device buffer of the module sits in a guard-banded allocation and the inputs between canaries; all of them are checked
after every launcher."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import predict as P  # noqa: E402

import postprocess_ref as R  # noqa: E402
import vectorize_ref as V  # noqa: E402
from guard import canary_input, guarded  # noqa: E402
from merge_schedule import FakeWorld, run_ranks  # noqa: E402

_FILL = {torch.uint8: 0xA5, torch.int32: -7, torch.int64: -7}
_LAUNCHERS = ("cc_label", "postprocess_counters", "vec_flags", "vec_scan", "vec_read", "vec_succ", "vec_min_rounds", "vec_swap", "vec_rank_init",
              "vec_rank_rounds", "vec_ring_info", "vec_place", "vec_emit")


def _vz():
    from unet_amd import vectorize
    return vectorize


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
    monkeypatch.setattr(_vz(), "_alloc", g.alloc)
    for name in _LAUNCHERS:
        def wrapped(*a, _fn=getattr(ops, name), _name=name, **k):
            r = _fn(*a, **k)
            g.launches += 1
            g.check(_name)
            return r
        monkeypatch.setattr(ops, name, wrapped)
    return g


_REF = {}


def _ref(key, mask, exclude=None):
    if key not in _REF:
        _REF[key] = V.polygonize(mask, exclude)
    return _REF[key]


def _equal(polys, ref, what):
    host = polys.cpu()
    for name in V.ARRAYS:
        got, want = getattr(host, name), ref[name]
        assert str(got.dtype).split(".")[-1] == str(want.dtype), (what, name, got.dtype)
        assert tuple(got.shape) == want.shape, (what, name, tuple(got.shape), want.shape)
        assert np.array_equal(got.numpy(), want), (what, name)
        assert getattr(polys, name).is_cuda


def _run(guards, mask, key, exclude=None):
    VZ = _vz()
    d = guards.upload(mask)
    polys = VZ.polygonize(d, exclude)
    _equal(polys, _ref(key, mask, exclude), key)
    assert np.array_equal(d.cpu().numpy(), mask), key          # the input is never written
    guards.clear()
    return polys


# ------------------------------------------------------------------------------------------------------------ against the reference

def test_all_16_masks_of_2x2(guards):
    for i in range(16):
        _run(guards, np.array([[i & 1, i >> 1 & 1], [i >> 2 & 1, i >> 3 & 1]], dtype=np.uint8), ("2x2", i))


@pytest.mark.parametrize("shape", [(1, 1), (1, 197), (197, 1)])
def test_single_rows_and_columns(guards, shape):
    for name, m in R.patterns(*shape).items():
        _run(guards, m, (shape, name))


@pytest.mark.parametrize("name", ["constant", "checker", "spiral", "comb", "diag", "antidiag", "noise2", "noise5", "noise256", "blocks"])
@pytest.mark.parametrize("shape", [(63, 64), (64, 65), (67, 131)])
def test_patterns_equal_the_reference(guards, shape, name):
    H, W = shape
    m = R.patterns(H, W)[name]
    polys = _run(guards, m, (shape, name))
    ref = _ref((shape, name), m)
    if name == "noise2":
        assert ref["swaps"] > 0                                      # the saddle swaps are exercised
    if name == "checker":
        assert polys.n_rings == H * W and polys.edges == 4 * H * W          # the maximum ring count
    if name in ("spiral", "comb"):
        assert int(np.diff(ref["ring_start"]).max()) >= 4 and polys.edges > 2000          # one ring of thousands of edges: many doubling rounds
    if name == "constant":
        assert polys.xy.cpu().tolist() == [[0, 0], [0, H], [W, H], [W, 0]] and polys.ring_area.cpu().tolist() == [H * W]


def test_nested_frames_give_holes_inside_islands(guards):
    m = np.zeros((11, 11), dtype=np.uint8)
    for k in range(5):
        m[k:11 - k, k:11 - k] = k % 2 + 1
    m[5, 5] = 9
    polys = _run(guards, m, "nested")
    host = polys.cpu()
    assert host.poly_label.tolist() == [0, 12, 24, 36, 48, 60]
    assert np.diff(host.poly_ring_start.numpy()).tolist() == [2, 2, 2, 2, 2, 1]          # every frame has one hole; the centre pixel none
    assert host.poly_pixels.tolist() == [40, 32, 24, 16, 8, 1]


def test_exclude_one_class_and_all_classes(guards):
    m = R.patterns(64, 65)["noise5"]
    one = _run(guards, m, ("noise5", "ex3"), 3)
    assert 3 not in one.poly_class.cpu().tolist() and one.n_polygons > 0
    _run(guards, m, ("noise5", "ex14"), [1, 4])
    none = _run(guards, m, ("noise5", "all"), range(5))
    assert none.n_polygons == 0 and none.n_rings == 0 and none.n_vertices == 0 and none.edges == 0
    assert none.ring_start.cpu().tolist() == [0] and none.poly_ring_start.cpu().tolist() == [0]


# ------------------------------------------------------------------------------------------------------------ independent of the reference

@pytest.mark.parametrize("name", ["noise2", "blocks", "spiral"])
def test_areas_fill_and_determinism_without_the_reference(guards, name):
    from unet_amd import postprocess as PP
    VZ = _vz()
    H, W = 67, 131
    m = R.patterns(H, W, seed=7)[name]
    d = guards.upload(m)
    a = VZ.polygonize(d)
    b = VZ.polygonize(d)
    guards.check("two runs")
    for name_ in V.ARRAYS:
        assert torch.equal(getattr(a, name_), getattr(b, name_)), name_          # two runs, equal bits
    assert np.array_equal(d.cpu().numpy(), m)
    lab = PP.label_components(d, 4)
    sizes = PP.component_sizes(lab).cpu().numpy().ravel()
    lab = lab.cpu().numpy()
    host = a.cpu()
    assert np.array_equal(host.poly_pixels.numpy(), sizes[host.poly_label.numpy()])
    assert np.array_equal(host.poly_label.numpy(), np.unique(lab))
    assert np.array_equal(host.poly_class.numpy(), m.ravel()[host.poly_label.numpy()])
    arrays = {k: getattr(host, k).numpy() for k in V.ARRAYS}
    back = np.full((H, W), -1, dtype=np.int64)
    for i, l in enumerate(host.poly_label.tolist()):
        inside = V.fill_even_odd(V.rings_of(arrays, i), H, W)
        assert (back[inside] == -1).all()
        back[inside] = l
    assert np.array_equal(back, lab)                                              # the even-odd fill of the device rings is the label image
    for kind in (m, torch.from_numpy(m)):                                         # host and NumPy inputs: the same arrays
        c = VZ.polygonize(kind)
        for name_ in V.ARRAYS:
            assert torch.equal(getattr(c, name_), getattr(a, name_)), name_
    guards.clear()


# ------------------------------------------------------------------------------------------------------------ prediction entry points

def _model(arch, n_in, n_out, size, seed=0):
    from unet_amd.model import HipDynamicUnet
    torch.manual_seed(seed)
    m = HipDynamicUnet(arch, n_in, n_out, (size, size))
    m.eval()
    return m


def _export(tmp_path, model, n_out, size):
    from unet_amd.learner import CrossEntropyLossFlat, DataLoaders, Learner, TileDataset
    dls = DataLoaders(TileDataset([np.zeros((4, size, size), np.uint8)], None, "int8"), None, 1, device="cuda",
                      vocab=[f"c{i}" for i in range(n_out)])
    learn = Learner(dls, model, loss_func=CrossEntropyLossFlat(axis=1), path=tmp_path)
    pkl = tmp_path / "m.pkl"
    learn.export(pkl)
    return pkl


def _raster_of(doc, H, W, gt, shift=0):
    out = np.full((H, W), 255, dtype=np.int64)
    for f in doc["features"]:
        rings = []
        for ring in f["geometry"]["coordinates"]:
            assert ring[0] == ring[-1]
            rings.append([(int(round((x - gt[0]) / gt[1])), int(round((y - gt[3]) / gt[5]))) for x, y in ring[:-1]])
        inside = V.fill_even_odd(rings, H, W)
        assert (out[inside] == 255).all()
        out[inside] = f["properties"]["class"] + shift
    return out


def test_entry_points_write_the_polygons_of_the_mask_they_return(tmp_path, monkeypatch, guards):
    import create_tiles_unet as T
    from unet_amd import postprocess as PP
    from unet_amd.tiffio import read_tiff, write_tiff
    size = 64
    model = _model("xresnet18", 4, 3, size, seed=11)
    img = np.random.default_rng(5).integers(1, 250, (4, 200, 170)).astype(np.uint8)
    rpath = tmp_path / "scene.tif"
    gt = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)
    write_tiff(rpath, img, geotransform=gt)
    kw = dict(max_empty=0.9, batch_size=5)
    plain = P.predict_raster(model, rpath, size, 0.2, **kw)
    assert guards.launches == 0 and not (tmp_path / "a.geojson").exists()          # vector_path=None: no launch of this family
    H, W = plain.shape
    timing = {}
    got = P.predict_raster(model, rpath, size, 0.2, vector_path=tmp_path / "a.geojson", timing=timing, **kw)
    doc = json.load(open(tmp_path / "a.geojson"))
    assert np.array_equal(got, plain) and np.array_equal(_raster_of(doc, H, W, gt), plain)
    assert timing["vector_seconds"] > 0 and timing["vector_polygons"] == len(doc["features"]) > 0 and timing["vector_vertices"] >= 4
    assert "crs" not in doc                                                         # the scene carries no GeoKeyDirectory
    # with postprocess and class_zero: the file holds the cleaned mask, class 0 has no feature and the ids are shifted; nothing is returned
    pp = PP.PostProcess(majority=3, sieve=30, frozen_class=0)
    clean = P.predict_raster(model, rpath, size, 0.2, postprocess=pp, **kw)
    none = P.predict_raster(model, rpath, size, 0.2, postprocess=pp, class_zero=True, vector_path=tmp_path / "b.geojson", vector_exclude=2,
                            return_array=False, out_path=tmp_path / "b.tif", compress="lzw", **kw)
    assert none is None and np.array_equal(read_tiff(tmp_path / "b.tif")[0], clean.astype(np.int16) - 1)
    back = _raster_of(json.load(open(tmp_path / "b.geojson")), H, W, gt, shift=1)
    keep = (clean != 0) & (clean != 2)
    assert np.array_equal(back == 255, ~keep) and np.array_equal(back[keep], clean[keep])
    # the tile-file entry point writes the same features beside the merged raster, with the vocab's names
    pkl = _export(tmp_path, model, 3, size)
    tiles = tmp_path / "cut"
    T.split_raster(rpath, None, tiles, patch_size=size, patch_overlap=0.2, split=[1], max_empty=0.9)
    timing = {}
    f = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, AOI="b", validation_vision=False, batch_size=5, vector=True, timing=timing)
    assert np.array_equal(read_tiff(f)[0], plain)
    doc2 = json.load(open(f.with_suffix(".geojson")))
    assert [x["geometry"] for x in doc2["features"]] == [x["geometry"] for x in doc["features"]]
    assert all(x["properties"]["name"] == f"c{x['properties']['class']}" for x in doc2["features"])
    assert [{k: v for k, v in x["properties"].items() if k != "name"} for x in doc2["features"]] == [x["properties"] for x in doc["features"]]
    assert timing["vector_polygons"] == len(doc["features"])
    # two ranks: the file of one rank
    arr = torch.from_numpy(img)
    one = P.predict_raster(model, arr, size, 0.2, vector_path=tmp_path / "w1.geojson", **kw)
    out, _ = run_ranks(2, lambda r: P.predict_raster(model, arr, size, 0.2, vector_path=tmp_path / "w2.geojson", **kw), monkeypatch, FakeWorld(2))
    assert np.array_equal(out, one)
    assert open(tmp_path / "w2.geojson").read() == open(tmp_path / "w1.geojson").read()
    guards.check("end")
