"""GPU suite of the ring simplification (csrc/simplify.hip, unet_amd/vectorize.py): every array of the simplified Polygons
compared for exact equality with the plain-Python restatement of the rules (tests/simplify_ref.py), the balance and area checks that do not
go through the tracer, and the prediction entry points.  As in test_vectorize_gpu.py every device buffer of the module sits in a
guard-banded allocation and the inputs between canaries; all of them are checked after every launcher."""
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
import simplify_ref as S  # noqa: E402
from guard import canary_input, guarded  # noqa: E402
from merge_schedule import FakeWorld, run_ranks  # noqa: E402

_FILL = {torch.uint8: 0xA5, torch.int32: -7, torch.int64: -7}
_OLD = ("cc_label", "postprocess_counters", "vec_flags", "vec_scan", "vec_read", "vec_succ", "vec_min_rounds", "vec_swap", "vec_rank_init",
        "vec_rank_rounds", "vec_ring_info", "vec_place", "vec_emit")
_NEW = ("simp_marks", "simp_gather", "simp_closed", "simp_near_rounds", "simp_dp_rounds", "simp_emit", "simp_area")


def _vz():
    from unet_amd import vectorize
    return vectorize


class Guards:
    def __init__(self):
        self.checks, self.launches, self.names = [], 0, []

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
    for name in _OLD + _NEW:
        def wrapped(*a, _fn=getattr(ops, name), _name=name, **k):
            r = _fn(*a, **k)
            g.launches += 1
            g.names.append(_name)
            g.check(_name)
            return r
        monkeypatch.setattr(ops, name, wrapped)
    return g


_PREP, _REF = {}, {}


def _ref(key, mask, tol, exclude=None):
    if key not in _PREP:
        _PREP[key] = S.prepare(mask, exclude)
    if (key, tol) not in _REF:
        _REF[key, tol] = S.simplify(mask, tol, exclude, _PREP[key])
    return _REF[key, tol]


def _equal(polys, ref, what):
    host = polys.cpu()
    for name in S.ARRAYS:
        got, want = getattr(host, name), ref[name]
        assert str(got.dtype).split(".")[-1] == str(want.dtype), (what, name, got.dtype)
        assert tuple(got.shape) == want.shape, (what, name, tuple(got.shape), want.shape)
        assert np.array_equal(got.numpy(), want), (what, name)
        assert getattr(polys, name).is_cuda
    assert polys.candidates == ref["raw_vertices"] and polys.rounds == ref["depth"], (what, polys.candidates, polys.rounds, ref["depth"])
    return host


def _independent(host, H, W, what, balanced=True):
    """the checks that do not go through the tracer, on a device result"""
    arrays = {k: getattr(host, k).numpy() for k in S.ARRAYS}
    if balanced:
        assert not S.unbalanced_segments(arrays, H, W), what
        assert S.doubled_area_sum(arrays) == 2 * H * W, what
    lists = S.ring_lists(arrays)
    assert all(len(r) >= 3 for r in lists), what
    assert [S.half(S.area2(r)) for r in lists] == arrays["ring_area"].tolist(), what


def _run(guards, mask, key, tol, exclude=None):
    VZ = _vz()
    d = guards.upload(mask)
    polys = VZ.polygonize(d, exclude, simplify=tol)
    ref = _ref(key, mask, tol, exclude)
    host = _equal(polys, ref, (key, tol))
    assert np.array_equal(d.cpu().numpy(), mask), key          # the input is never written
    _independent(host, *mask.shape, (key, tol), balanced=exclude is None and ref["orphans"] == 0)
    guards.clear()
    return polys, ref


def _special():
    nested = np.zeros((11, 11), dtype=np.uint8)
    for k in range(5):
        nested[k:11 - k, k:11 - k] = k % 2 + 1
    nested[5, 5] = 9
    pair = np.zeros((6, 7), dtype=np.uint8)
    pair[2, 2] = pair[3, 3] = 1
    tee = np.zeros((8, 9), dtype=np.uint8)
    tee[:4], tee[4:, :5], tee[4:, 5:] = 1, 2, 3
    return {"nested": nested, "pair": pair, "tee": tee}


# ------------------------------------------------------------------------------------------------------------ against the reference

def test_all_16_masks_of_2x2(guards):
    for i in range(16):
        for tol in (0, 1):
            _run(guards, np.array([[i & 1, i >> 1 & 1], [i >> 2 & 1, i >> 3 & 1]], dtype=np.uint8), ("2x2", i), tol)


@pytest.mark.parametrize("shape", [(1, 1), (1, 197), (197, 1)])
def test_single_rows_and_columns(guards, shape):
    for name, m in R.patterns(*shape).items():
        _run(guards, m, (shape, name), 1)


@pytest.mark.parametrize("name", ["constant", "checker", "spiral", "comb", "diag", "antidiag", "noise2", "noise5", "noise256", "blocks"])
@pytest.mark.parametrize("shape", [(63, 64), (64, 65), (67, 131)])
def test_patterns_equal_the_reference(guards, shape, name):
    VZ = _vz()
    H, W = shape
    m = R.patterns(H, W)[name]
    for tol in (0, 1, 8):
        polys, ref = _run(guards, m, (shape, name), tol)
        if name == "spiral":
            assert ref["depth"] > 2 * VZ._SIMPLIFY_GROUP          # one arc of hundreds of candidates: many rounds, several groups
        if name in ("spiral", "noise2", "blocks"):
            assert ref["wraps"] > 0                                # arcs that run past their ring's leader
        if name == "constant":
            assert polys.xy.cpu().tolist() == [[0, 0], [0, H], [W, H], [W, 0]] and polys.ring_area.cpu().tolist() == [H * W]
        if tol == 0:
            assert polys.n_vertices == polys.candidates >= polys.raw_vertices
        if name == "noise2" and tol == 8:
            assert ref["dropped_polygons"] > 0 and ref["dropped_rings"] > ref["dropped_polygons"]


@pytest.mark.parametrize("name", ["nested", "pair", "tee"])
def test_node_free_rings_one_node_rings_and_a_junction(guards, name):
    m = _special()[name]
    for tol in (0.5, 2.5):
        polys, ref = _run(guards, m, name, tol)
        nodes = [sum(1 for c in cand if c[2]) for cand in ref["cand"]]
        if name == "nested":
            assert nodes.count(0) >= 8                       # closed arcs without a node: anchor and far point
        if name == "pair":
            assert nodes.count(1) >= 2                       # the two pixels touch at one saddle vertex: rings with one node
        if name == "tee":
            assert [5, 4] in polys.xy.cpu().tolist()          # the T-junction is kept on every ring that passes it
            assert sum(1 for r in S.ring_lists(ref) if (5, 4) in r) == 3


def test_exclude_one_class(guards):
    m = R.patterns(64, 65)["noise5"]
    polys, ref = _run(guards, m, ("noise5", "ex0"), 1, 0)
    assert 0 not in polys.poly_class.cpu().tolist() and polys.n_polygons > 0


def test_noise_across_scan_blocks_in_one_row(guards):
    H, W = 130, 4100
    m = (np.random.default_rng(3).random((H, W)) < 0.04).astype(np.uint8)
    polys, ref = _run(guards, m, "wide", 1)
    assert polys.edges > 4096 * 4 and ref["dropped_polygons"] > 0


# ------------------------------------------------------------------------------------------------------------ determinism, the default path

def test_two_runs_give_equal_arrays(guards):
    VZ = _vz()
    m = R.patterns(67, 131, seed=7)["blocks"]
    d = guards.upload(m)
    a = VZ.polygonize(d, simplify=1.5)
    b = VZ.polygonize(d, simplify=1.5)
    for name in S.ARRAYS:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.n_vertices < a.raw_vertices
    guards.clear()


def test_simplify_none_is_the_old_path(guards):
    VZ = _vz()
    m = R.patterns(63, 64)["blocks"]
    d = guards.upload(m)
    a = VZ.polygonize(d)
    names = list(guards.names)
    b = VZ.polygonize(d, None, None)
    c = VZ.polygonize(d, simplify=None)
    for name in S.ARRAYS:
        assert torch.equal(getattr(a, name), getattr(b, name)) and torch.equal(getattr(a, name), getattr(c, name)), name
    assert guards.names == names * 3 and not set(names) & set(_NEW)          # launch for launch, none of the new launchers
    assert (a.raw_vertices, a.candidates, a.rounds) == (0, 0, 0)
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


def _is_subsequence(small, big):
    it = iter(big)
    return all(any(x == y for y in it) for x in small)


def test_entry_points_write_the_simplified_polygons(tmp_path, monkeypatch, guards):
    import create_tiles_unet as T
    from unet_amd.tiffio import read_tiff, write_tiff
    size = 64
    model = _model("xresnet18", 4, 3, size, seed=11)
    img = np.random.default_rng(5).integers(1, 250, (4, 200, 170)).astype(np.uint8)
    rpath = tmp_path / "scene.tif"
    gt = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)
    write_tiff(rpath, img, geotransform=gt)
    kw = dict(max_empty=0.9, batch_size=5)
    with pytest.raises(ValueError):
        P.predict_raster(model, rpath, size, 0.2, vector_simplify=1.0, **kw)          # a tolerance without a vector output
    assert guards.launches == 0
    plain = P.predict_raster(model, rpath, size, 0.2, vector_path=tmp_path / "a.geojson", **kw)
    timing = {}
    got = P.predict_raster(model, rpath, size, 0.2, vector_path=tmp_path / "s.geojson", vector_simplify=1.0, timing=timing, **kw)
    assert np.array_equal(got, plain)
    raw, doc = json.load(open(tmp_path / "a.geojson")), json.load(open(tmp_path / "s.geojson"))
    props = [f["properties"] for f in doc["features"]]
    assert 0 < len(props) <= len(raw["features"]) and _is_subsequence(props, [f["properties"] for f in raw["features"]])
    assert all(ring[0] == ring[-1] and len(ring) >= 4 for f in doc["features"] for ring in f["geometry"]["coordinates"])
    assert timing["vector_polygons"] == len(props) and 0 < timing["vector_vertices"] < timing["vector_vertices_raw"]
    assert timing["vector_vertices_raw"] == sum(len(r) - 1 for f in raw["features"] for r in f["geometry"]["coordinates"])
    # the file's rings are those of polygonize(simplify=1.0) on the returned mask
    ref = S.simplify(plain, 1.0)
    want = [[[gt[0] + x * gt[1], gt[3] + y * gt[5]] for x, y in ring + ring[:1]] for ring in S.ring_lists(ref)]
    order = ref["poly_rings"].tolist()
    assert [r for f in doc["features"] for r in f["geometry"]["coordinates"]] == [want[i] for i in order]
    # the tile-file entry point writes the same features beside the merged raster
    pkl = _export(tmp_path, model, 3, size)
    tiles = tmp_path / "cut"
    T.split_raster(rpath, None, tiles, patch_size=size, patch_overlap=0.2, split=[1], max_empty=0.9)
    timing = {}
    f = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, AOI="b", validation_vision=False, batch_size=5, vector=True,
                           vector_simplify=1.0, timing=timing)
    assert np.array_equal(read_tiff(f)[0], plain)
    doc2 = json.load(open(f.with_suffix(".geojson")))
    assert [x["geometry"] for x in doc2["features"]] == [x["geometry"] for x in doc["features"]]
    assert timing["vector_polygons"] == len(props) and timing["vector_vertices_raw"] > timing["vector_vertices"]
    # one and three ranks: the same bytes
    arr = torch.from_numpy(img)
    one = P.predict_raster(model, arr, size, 0.2, vector_path=tmp_path / "w1.geojson", vector_simplify=1.0, **kw)
    out, _ = run_ranks(3, lambda r: P.predict_raster(model, arr, size, 0.2, vector_path=tmp_path / "w3.geojson", vector_simplify=1.0, **kw),
                       monkeypatch, FakeWorld(3))
    assert np.array_equal(out, one)
    assert open(tmp_path / "w3.geojson").read() == open(tmp_path / "w1.geojson").read()
    guards.check("end")
