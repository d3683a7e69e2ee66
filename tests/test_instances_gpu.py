"""GPU suite of the instance split (csrc/instances.hip, unet_amd/instances.py): labels and counts compared for exact equality with the
sequential restatement of the rules (tests/instances_ref.py), polygonize_labels against the reference tracer run on the same labels, and
the prediction entry points.  Every device buffer of the modules sits in a guard-banded allocation and the inputs between canaries; all of
them are checked after every launcher."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import predict as P  # noqa: E402

import instances_ref as I  # noqa: E402
import simplify_ref as S  # noqa: E402
import vectorize_ref as V  # noqa: E402
from guard import canary_input, guarded  # noqa: E402

_FILL = {torch.uint8: 0xA5, torch.int32: -7, torch.int64: -7}
_LAUNCHERS = ("inst_distance", "cc_label_keys", "postprocess_counters", "inst_ascent", "inst_ptr_rounds", "inst_gather", "inst_merge_round",
              "inst_canonical", "inst_marks", "inst_ids", "inst_check_labels", "cc_label", "vec_flags", "vec_scan", "vec_read", "vec_succ",
              "vec_min_rounds", "vec_swap", "vec_rank_init", "vec_rank_rounds", "vec_ring_info", "vec_place", "vec_emit")


def _in():
    from unet_amd import instances
    return instances


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
    monkeypatch.setattr(_in(), "_alloc", g.alloc)
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


def _ref(key, mask, classes, R, depth, max_rounds=64):
    key = (key, tuple(np.atleast_1d(classes).tolist()), R, depth, max_rounds)
    if key not in _REF:
        _REF[key] = I.split(mask, classes, R, depth, max_rounds)
    return _REF[key]


def _run(guards, mask, key, classes, R=64, depth=2.0, max_rounds=64):
    d = guards.upload(mask)
    labels, info = _in().split_instances(d, classes, R, depth, max_rounds)
    want, winfo = _ref(key, mask, classes, R, depth, max_rounds)
    assert labels.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == mask.shape
    got = labels.cpu().numpy()
    assert np.array_equal(got, want), (key, R, depth, int((got != want).sum()))
    assert info == winfo, (key, R, depth, info, winfo)
    assert np.array_equal(d.cpu().numpy(), mask), key          # the input is never written
    guards.clear()
    return got, info


# ------------------------------------------------------------------------------------------------------------ against the restatement

def test_touching_discs(guards):
    two = I.discs(40, 48, [(20, 16), (20, 31)])
    for depth, n in ((0, 2), (1, 2), (2, 2), (3, 1), (4, 1), (8, 1)):
        labels, _ = _run(guards, two, "two", 1, 64, depth)
        assert len(np.unique(labels[two == 1])) == n, depth
    three = I.discs(40, 60, [(20, 14), (20, 29), (20, 44)])
    for depth, n in ((2, 3), (3, 1)):
        labels, _ = _run(guards, three, "three", [1], 64, depth)
        assert len(np.unique(labels[three == 1])) == n, depth
    square = np.zeros((30, 30), dtype=np.uint8)
    square[3:27, 3:27] = 1
    for R in (4, 64):
        labels, _ = _run(guards, square, "square", 1, R, 2.0)
        assert len(np.unique(labels[square == 1])) == 1, R


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (41, 1)])
def test_degenerate_shapes(guards, shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for k, m in enumerate((np.zeros(shape, np.uint8), rng.integers(0, 2, shape).astype(np.uint8), (rng.random(shape) < 0.15).astype(np.uint8) * 3)):
        for classes in (0, [0, 1, 3]):
            _run(guards, m, (shape, k), classes, 8, 1.0)


def test_one_class_masks_split_and_not_split(guards):
    m = np.full((37, 70), 2, dtype=np.uint8)
    labels, info = _run(guards, m, "const", 2, 16, 2.0)                # no pixel of another value: h = R^2 everywhere, one zone, one seed
    assert (labels == 0).all() and info == {"seeds": 1, "segments": 1, "rounds": 1, "merged": [0]}
    labels, info = _run(guards, m, "const", [0, 1], 16, 2.0)           # the mask's class is not split
    assert (labels == 0).all() and info["segments"] == 1


def test_discs_across_the_seams_of_every_tile(guards):
    from unet_amd import ops
    (rth, rtw), (cth, ctw), (lth, ltw) = *ops.inst_tile_shapes(), ops.cc_tile_shape()
    th, tw = max(rth, cth, lth), max(rtw, ctw, ltw)
    H, W = th + 3, 2 * tw + 5
    centres = [(th - 2, tw - 5), (th - 2, tw + 9), (th - 9, 2 * tw + 1), (lth, ltw + 3), (lth + 4, ltw + 16), (12, ctw), (14, 3 * ctw + 12),
               (cth - 1, 2 * rtw - 7), (th + 1, 20)]
    m = I.discs(H, W, centres, r2=81)
    m[I.discs(H, W, [(lth - 3, 5 * ctw)], r2=144, value=1) == 1] = 2
    assert m[:, tw - 1].any() and m[:, tw].any() and m[th - 1].any() and m[th].any()
    for R, depth in ((64, 2.0), (7, 0.0)):
        _, info = _run(guards, m, "seams", [1, 2], R, depth)
        assert info["seeds"] > 4


def test_large_radius_where_the_halo_exceeds_the_tiles(guards):
    m = I.discs(40, 300, [(20, 40), (20, 58), (20, 150), (18, 171), (20, 280)], r2=121)
    m[:, 200:230] = 2
    _, info = _run(guards, m, "r255", [0, 1], 255, 2.0)          # the background's distances reach far beyond one tile; 255 is never reached
    assert info["segments"] >= 5


def test_radius_one(guards):
    m = I.blobs(45, 77, seed=5)
    labels, info = _run(guards, m, "r1", [1, 2], 1, 2.0)          # h = 1 on every split pixel: the zones are the components
    assert np.array_equal(labels, I.components(m)) and info["merged"] == [0]


@pytest.mark.parametrize("R, depth", [(16, 0), (16, 1), (16, 2), (5, 4)])
def test_random_blobs(guards, R, depth):
    m = I.blobs(97, 131)
    labels, info = _run(guards, m, "blobs", [1, 2], R, depth)
    comp = I.components(m)
    assert np.array_equal(labels[m == 0], comp[m == 0])          # the class that is not split keeps its component labels
    if depth == 0:
        assert info["segments"] == info["seeds"] and info["rounds"] == 1
    if depth == 2:
        assert info["rounds"] >= 3 and info["segments"] < info["seeds"]          # several rounds: merges of merged segments


def test_round_cap(guards):
    m = I.blobs(97, 131)
    _, one = _run(guards, m, "blobs", [1, 2], 16, 2, max_rounds=1)
    _, two = _run(guards, m, "blobs", [1, 2], 16, 2, max_rounds=2)
    _, full = _ref("blobs", m, [1, 2], 16, 2)
    assert one["rounds"] == 1 and two["rounds"] == 2 and one["merged"] == full["merged"][:1] and two["merged"] == full["merged"][:2]
    _, five = _run(guards, m, "blobs", [1, 2], 5, 4, max_rounds=5)          # the cap falls inside the second group of rounds
    assert five["rounds"] == 5 and five["merged"][-1] > 0


def test_two_runs_and_every_kind_of_input_give_equal_labels(guards):
    IN = _in()
    m = I.blobs(97, 131, seed=11)
    d = guards.upload(m)
    a, ia = IN.split_instances(d, [1, 2], 16, 2.0)
    b, ib = IN.split_instances(d, [1, 2], 16, 2.0)
    assert torch.equal(a, b) and ia == ib
    host, ih = IN.split_instances(m, [1, 2], 16, 2.0)
    assert isinstance(host, np.ndarray) and host.dtype == np.int32 and np.array_equal(host, a.cpu().numpy()) and ih == ia
    t, _ = IN.split_instances(torch.from_numpy(m), [1, 2], 16, 2.0)
    assert isinstance(t, torch.Tensor) and not t.is_cuda and np.array_equal(t.numpy(), host)
    stages = {}
    c, _ = IN.split_instances(d, [1, 2], 16, 2.0, stages=stages)
    assert torch.equal(a, c) and sorted(stages) == ["ascent", "canonical", "distance", "merge", "zones"]
    ids, count = IN.instance_ids(d, a, [1, 2])
    assert np.array_equal(ids.cpu().numpy().view(np.uint32), I.dense_ids(m, host, [1, 2])) and count == int(ids.max())
    guards.clear()


# ------------------------------------------------------------------------------------------------------------ polygonize_labels

def _reference_polygons(monkeypatch, mask, labels, exclude=None):
    """the reference tracer on the given labels: it asks its module-level `R` for the labels of the mask"""
    with monkeypatch.context() as mp:
        mp.setattr(V, "R", types.SimpleNamespace(label_components=lambda m, connectivity: np.asarray(labels)))
        return V.polygonize(mask, exclude)


def _equal(polys, ref, what):
    host = polys.cpu()
    for name in V.ARRAYS:
        got, want = getattr(host, name), ref[name]
        assert str(got.dtype).split(".")[-1] == str(want.dtype), (what, name, got.dtype)
        assert tuple(got.shape) == want.shape, (what, name, tuple(got.shape), want.shape)
        assert np.array_equal(got.numpy(), want), (what, name)
    return host


def test_polygonize_with_component_labels_equals_polygonize(guards):
    from unet_amd import postprocess as PP
    VZ = _vz()
    m = I.blobs(67, 131, seed=2)
    d = guards.upload(m)
    plain = VZ.polygonize(d, exclude=0)
    given = VZ.polygonize_labels(d, PP.label_components(d, 4), exclude=0)
    for name in V.ARRAYS:
        assert torch.equal(getattr(plain, name), getattr(given, name)), name
    assert given.edges == plain.edges
    bad = PP.label_components(d, 4).clone()
    bad[5, 7] = 67 * 131 - 1                                                # a label behind its pixel
    with pytest.raises(ValueError):
        VZ.polygonize_labels(d, bad)
    bad = PP.label_components(d, 4).clone()
    bad[m.shape[0] - 1, m.shape[1] - 1] = 0 if m[-1, -1] != m[0, 0] else int(np.flatnonzero(m.ravel() != m[0, 0])[0])          # another class
    with pytest.raises(ValueError):
        VZ.polygonize_labels(d, bad)
    for wrong in (torch.zeros((67, 130), dtype=torch.int32, device="cuda"), torch.zeros((67, 131), dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError):
            VZ.polygonize_labels(d, wrong)
    guards.clear()


def test_polygons_of_instances(guards, monkeypatch):
    IN, VZ = _in(), _vz()
    m = I.blobs(97, 131)
    d = guards.upload(m)
    labels, info = IN.split_instances(d, [1, 2], 16, 2.0)
    host_labels = labels.cpu().numpy()
    assert np.array_equal(host_labels, _ref("blobs", m, [1, 2], 16, 2.0)[0])
    polys = VZ.polygonize_labels(d, labels)
    host = _equal(polys, _reference_polygons(monkeypatch, m, host_labels), "instances")
    assert polys.n_polygons == info["segments"] > len(np.unique(I.components(m)))
    roots, sizes = np.unique(host_labels, return_counts=True)
    assert np.array_equal(host.poly_label.numpy(), roots) and np.array_equal(host.poly_pixels.numpy(), sizes)
    assert np.array_equal(host.poly_class.numpy(), m.ravel()[roots])
    part = VZ.polygonize_labels(d, labels, exclude=0)
    _equal(part, _reference_polygons(monkeypatch, m, host_labels, 0), "instances without class 0")
    # simplified: every border between two segments, instances of one class included, is one vertex chain walked from both sides
    simple = VZ.polygonize_labels(d, labels, simplify=1.0).cpu()
    arrays = {k: getattr(simple, k).numpy() for k in S.ARRAYS}
    assert not S.unbalanced_segments(arrays, *m.shape)
    assert simple.n_vertices < polys.n_vertices and simple.n_polygons > len(np.unique(I.components(m)))
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


def test_entry_points_write_one_feature_and_one_id_per_instance(tmp_path, guards):
    import create_tiles_unet as T
    from unet_amd import postprocess as PP
    from unet_amd.tiffio import read_tiff, write_tiff
    size = 64
    model = _model("xresnet18", 4, 3, size, seed=11)
    img = np.random.default_rng(5).integers(1, 250, (4, 200, 170)).astype(np.uint8)
    rpath = tmp_path / "scene.tif"
    gt = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)
    write_tiff(rpath, img, geotransform=gt)
    pp = PP.PostProcess(majority=5, sieve=20)
    kw = dict(max_empty=0.9, batch_size=5, postprocess=pp)
    plain = P.predict_raster(model, rpath, size, 0.2, out_path=tmp_path / "a.tif", vector_path=tmp_path / "a.geojson", **kw)
    n = guards.launches
    same = P.predict_raster(model, rpath, size, 0.2, out_path=tmp_path / "b.tif", vector_path=tmp_path / "b.geojson", instances=None, **kw)
    assert np.array_equal(same, plain) and guards.launches - n == n          # instances=None: the launches of a call without the argument
    assert open(tmp_path / "a.tif", "rb").read() == open(tmp_path / "b.tif", "rb").read()
    assert open(tmp_path / "a.geojson").read() == open(tmp_path / "b.geojson").read()
    split = sorted(int(c) for c in np.unique(plain))[-2:]          # two classes the random model predicts
    other = [c for c in range(3) if c not in split]
    inst = {"classes": split, "radius": 16, "min_depth": 1.0}
    timing = {}
    got = P.predict_raster(model, rpath, size, 0.2, out_path=tmp_path / "c.tif", vector_path=tmp_path / "c.geojson", vector_exclude=other,
                           instances=inst, instances_path=tmp_path / "c_inst.tif", compress="lzw", predictor=2, tile=64, timing=timing, **kw)
    assert np.array_equal(got, plain) and np.array_equal(read_tiff(tmp_path / "c.tif")[0], plain)
    want, winfo = I.split(plain, split, 16, 1.0)
    ids, meta = read_tiff(tmp_path / "c_inst.tif")
    assert ids.dtype == np.uint32 and np.array_equal(ids, I.dense_ids(plain, want, split))          # 0 off the split classes, ids <-> labels
    assert tuple(meta["geotransform"]) == tuple(read_tiff(tmp_path / "c.tif")[1]["geotransform"])
    N = int(ids.max())
    assert timing["instances"]["instances"] == N and timing["instances"]["segments"] == winfo["segments"] and timing["instances_seconds"] > 0
    doc = json.load(open(tmp_path / "c.geojson"))
    assert [f["properties"]["instance"] for f in doc["features"]] == list(range(1, N + 1))          # one feature per instance
    on = np.isin(plain, split)
    sizes = np.bincount(ids[on].astype(np.int64), minlength=N + 1)[1:]
    assert [f["properties"]["pixels"] for f in doc["features"]] == sizes.tolist()
    assert N >= len(np.unique(I.components(plain)[on])) > 0              # the instances refine the components
    # all classes in the file: the components of the class that is not split carry instance 0
    P.predict_raster(model, rpath, size, 0.2, vector_path=tmp_path / "d.geojson", instances=inst, return_array=False, **kw)
    doc = json.load(open(tmp_path / "d.geojson"))
    zero = [f for f in doc["features"] if f["properties"]["instance"] == 0]
    assert all(f["properties"]["class"] in other for f in zero) and len(doc["features"]) - len(zero) == N
    # the tile-file entry point: the same ids beside the merged raster
    pkl = _export(tmp_path, model, 3, size)
    tiles = tmp_path / "cut"
    T.split_raster(rpath, None, tiles, patch_size=size, patch_overlap=0.2, split=[1], max_empty=0.9)
    f = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, AOI="b", validation_vision=False, batch_size=5, postprocess=pp,
                           instances=inst, instances_raster=True, vector=True, vector_exclude=other)
    assert np.array_equal(read_tiff(f)[0], plain)
    assert np.array_equal(read_tiff(f.with_name(f.stem + "_instances.tif"))[0], ids)
    doc2 = json.load(open(f.with_suffix(".geojson")))
    assert [x["properties"]["instance"] for x in doc2["features"]] == list(range(1, N + 1))
    guards.check("end")
