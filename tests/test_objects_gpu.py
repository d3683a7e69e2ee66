"""GPU suite of the object attributes (csrc/objects.hip, unet_amd/objects.py): every table against the sequential restatement
of the rules (tests/objects_ref.py) on the shapes, patterns and alignments where the kernel takes another path; sums beyond 2^32, more than
2^16 objects, the register carry, ties of the point, bad input, determinism, the vector stage, the two entry points.  Every comparison is
exact equality.  Every buffer a kernel writes sits in a guard-banded allocation and every input between canaries; all of them are checked
after every launcher, and the inputs are compared unchanged afterwards."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import objects_cases as OC  # noqa: E402
import objects_ref as OR  # noqa: E402
import postprocess_ref as R  # noqa: E402
import zonal_cases as ZC  # noqa: E402
from guard import canary_input, guarded  # noqa: E402

_FILL = {torch.uint8: 0xA5, torch.int32: -7, torch.int64: -7}
_LAUNCHERS = ("inst_marks", "vec_scan", "vec_read", "obj_compact", "obj_accumulate", "obj_point")


def _ob():
    from unet_amd import objects
    return objects


class Guards:
    def __init__(self):
        self.checks, self.by_name = [], {}

    def alloc(self, shape, dtype, device):
        t, c = guarded(shape, dtype, device, _FILL[dtype])
        self.checks.append(c)
        return t

    def upload(self, a) -> torch.Tensor:
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
    monkeypatch.setattr(_ob(), "_alloc", g.alloc)
    for name in _LAUNCHERS:
        def wrapped(*a, _fn=getattr(ops, name), _name=name, **k):
            r = _fn(*a, **k)
            g.by_name[_name] = g.by_name.get(_name, 0) + 1
            g.check(_name)
            return r
        monkeypatch.setattr(ops, name, wrapped)
    return g


def _measure(guards, m, lab, exclude=None):
    """measure_objects on guarded copies; the inputs come back unchanged; returns the host table as a dict of arrays"""
    dm, dl = guards.upload(m), guards.upload(lab)
    t = _ob().measure_objects(dm, dl, exclude)
    assert t.label.is_cuda and t.pixels.dtype == torch.int64 and t.bbox.dtype == torch.int32 and tuple(t.bbox.shape) == (t.n_objects, 4)
    assert np.array_equal(dm.cpu().numpy(), m) and np.array_equal(dl.cpu().numpy(), lab)
    host = OR.host(t)
    guards.clear()
    return host


def _check(guards, m, lab, exclude=None, what="", ref=OR.table):
    want, got = ref(m, lab, exclude), _measure(guards, m, lab, exclude)
    for f in OR.FIELDS:
        assert np.array_equal(got[f], want[f]) and got[f].dtype == want[f].dtype, (what, f)
    assert got["shape"] == want["shape"]
    return got


# ------------------------------------------------------------------------------------------------------------ shapes x patterns

@pytest.mark.parametrize("shape", OC.SHAPES)
def test_patterns_equal_the_restatement(guards, shape):
    H, W = shape
    pats = OC.patterns(H, W, seed=H * 1000 + W)
    assert set(pats) == {"one", "checker", "hstripes", "vstripes", "blocks", "noise", "split"}
    for name, (m, lab) in pats.items():
        for exclude in (None, 1, (0, 2)):
            got = _check(guards, m, lab, exclude, (shape, name, exclude))
        if name == "one":
            assert _check(guards, m, lab)["pixels"].tolist() == [H * W]
        if name == "checker":
            t = _check(guards, m, lab)
            assert len(t["label"]) == H * W and (t["edges_v"] + t["edges_h"] == 4).all() and np.array_equal(t["point"], t["label"])
        if name == "split" and H > 1 and W > 1:
            t = _check(guards, m, lab)          # one rectangle of one class, four objects: the cuts are edges of both sides
            assert len(t["label"]) == 4 and int((t["edges_v"] + t["edges_h"]).sum()) == 2 * (H + W) + 2 * (H + W)
    assert guards.by_name["obj_accumulate"] == guards.by_name["vec_scan"] >= 21 and got is not None


def test_ring_u_and_the_ties_of_the_point(guards):
    for shape, at in (((9, 11), (0, 0)), ((40, 56), (13, 30)), ((33, 300), (20, 250))):
        for small in (OC.ring(), OC.u_shape(), OC.cross(), np.ones((2, 2), dtype=np.uint8)):
            m = OC.placed(shape, small, at)
            lab = R.label_components(m, 4)
            t = _check(guards, m, lab, 0, (shape, small.shape))
            k = int(np.argmax(t["pixels"]))
            assert lab.ravel()[t["point"][k]] == t["label"][k]                              # inside the object ...
            cx, cy = int(t["sum_x"][k] // t["pixels"][k]), int(t["sum_y"][k] // t["pixels"][k])
            if small.shape in ((9, 11), (9, 10)):
                assert lab[cy, cx] != t["label"][k]                                         # ... where the centroid is not
            _check(guards, m, lab, None, (shape, small.shape, "with the background"))
    # four pixels around a missing centre as one object: all at distance 1 from the centroid
    m = np.zeros((3, 3), dtype=np.uint8)
    m[0, 1] = m[1, 0] = m[1, 2] = m[2, 1] = 1
    t = _check(guards, m, OC.own_labels(m.astype(np.int64)), 0)
    assert t["point"].tolist() == [1] and t["pixels"].tolist() == [4]


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_planes_at_addresses_that_are_only_element_aligned(guards, shift):
    OB = _ob()
    for H, W in ((3, 17), (33, 300), (1, 1), (40, 56)):
        m, lab = OC.patterns(H, W, seed=shift)["noise"]
        n = H * W
        bufs = []
        for a in (m, lab):
            flat = guards.upload(np.concatenate([np.full(shift, a.reshape(-1)[0], a.dtype), a.reshape(-1)]))
            bufs.append(flat[shift:shift + n].view(H, W))
        assert bufs[1].data_ptr() % 16 != 0 and bufs[1].is_contiguous()
        want = OR.table(m, lab, 1)
        for dm, dl in ((bufs[0], bufs[1]), (guards.upload(m), bufs[1]), (bufs[0], guards.upload(lab))):          # both, or one plane only
            got = OR.host(OB.measure_objects(dm, dl, 1))
            assert OR.same(got, want), (H, W, shift)
        guards.clear()


def test_an_excluded_class_around_a_kept_object_still_gives_it_edges(guards):
    m = OC.placed((12, 20), OC.ring(), (2, 4), background=3)
    m[6, 9] = 2                                                                             # an island in the ring's hole (class 0)
    lab = R.label_components(m, 4)
    everything = _check(guards, m, lab)
    kept = _check(guards, m, lab, (0, 3))
    assert kept["cls"].tolist() == [1, 2] and len(everything["label"]) == 5          # the background, the frame of class 0, the ring, its hole, the island
    pick = np.isin(everything["label"], kept["label"])
    for f in OR.FIELDS:
        assert np.array_equal(everything[f][pick], kept[f])                                 # the same rows, whoever else is measured
    assert kept["edges_v"].tolist() == [2 * 7 + 2 * 3, 2] and kept["edges_h"].tolist() == [2 * 9 + 2 * 5, 2]
    assert len(_check(guards, m, lab, (0, 1, 2, 3))["label"]) == 0                         # nothing kept: empty tables, the check still runs


def test_labels_none_are_the_components_and_host_inputs_are_uploaded(guards):
    OB = _ob()
    m = OC.noise_mask(40, 56, 3)
    want = OR.table(m, R.label_components(m, 4), 0)
    assert OR.same(OR.host(OB.measure_objects(m, exclude=0)), want)
    assert OR.same(OR.host(OB.measure_objects(torch.from_numpy(m).cuda(), None, [0])), want)
    stages = {}
    OB.measure_objects(m, exclude=0, stages=stages)
    assert set(stages) == {"index", "accumulate", "point"}
    guards.clear()


def test_more_objects_than_65536(guards):
    H = W = 300
    yy, xx = np.mgrid[0:H, 0:W]
    m, lab = ((yy + xx) % 2).astype(np.uint8), (yy * W + xx).astype(np.int32)
    t = _check(guards, m, lab, None, "checkerboard", OR.table_fast)
    assert len(t["label"]) == 90000 and (t["pixels"] == 1).all() and (t["edges_v"] + t["edges_h"] == 4).all()
    half = _check(guards, m, lab, 0, "one colour", OR.table_fast)
    assert len(half["label"]) == 45000 and (half["cls"] == 1).all()


@pytest.mark.parametrize("shape", [(1, 1000000), (70000, 30)])
def test_sums_beyond_32_bits(guards, shape):
    from unet_amd import ops
    H, W = shape
    m, lab = np.full(shape, 2, dtype=np.uint8), np.zeros(shape, dtype=np.int32)
    t = _check(guards, m, lab, None, shape, OR.table_fast)
    n = H * W
    assert t["pixels"].tolist() == [n] and t["sum_x"].tolist() == [H * (W * (W - 1) // 2)] and t["sum_y"].tolist() == [W * (H * (H - 1) // 2)]
    assert max(int(t["sum_x"][0]), int(t["sum_y"][0])) > 2 ** 32 and t["bbox"].tolist() == [[0, 0, W, H]]
    assert t["edges_v"].tolist() == [2 * H] and t["edges_h"].tolist() == [2 * W]
    assert t["point"].tolist() == [((H - 1) // 2) * W + (W - 1) // 2]
    assert ops.obj_point_packed(H, W) == (shape == (70000, 30))                             # both forms of the point pass are in this test
    # two objects whose nearest pixels lie far from their centroids: an L along the frame (the two-pass form measures 10^11 and more)
    m2 = np.zeros(shape, dtype=np.uint8)
    if H == 1:
        m2[0, :10] = 1
        m2[0, -10:] = 1
        lab2 = OC.own_labels(m2.astype(np.int64))
    else:
        m2[:10, :] = 1
        m2[-10:, :] = 1
        lab2 = OC.own_labels(m2.astype(np.int64))
    t = _check(guards, m2, lab2, None, (shape, "far"), OR.table_fast)
    assert len(t["label"]) == 2 and (m2.ravel()[t["point"]] == t["cls"]).all()


def test_steps_of_one_label_carried_in_registers_and_a_change_inside_the_span(guards):
    m, lab = OC.carry_case()
    H, W = m.shape
    assert (H * W + 3) // 4 > 1024 * 256                                                    # more groups than the largest grid has lanes
    t = _check(guards, m, lab, None, "carry", OR.table_fast)
    assert t["label"][0] == 0 and t["pixels"][0] > 390 * W and len(t["label"]) > 500
    _check(guards, m, lab, 4, "carry, the large object excluded", OR.table_fast)


def test_bad_labels_raise_and_store_nothing_outside_the_tables(guards):
    OB = _ob()
    for H, W in ((3, 17), (33, 300)):
        m, lab = OC.patterns(H, W, seed=5)["blocks"]
        n = H * W
        for what, plane, at, value, text in (("beyond the raster", "lab", n // 2, n, "outside 0"), ("far beyond", "lab", n - 1, 2 ** 31 - 1, "outside 0"),
                                             ("negative", "lab", 0, -5, "outside 0"), ("not canonical", "lab", n - 1, 1, "not canonical"),
                                             ("a chain", "lab", 3, 2 * W + 3, "not canonical"), ("class of the anchor", "m", 1, 9, "class differs")):
            mm, ll = m.copy(), lab.copy()
            (ll if plane == "lab" else mm).reshape(-1)[at] = value
            assert lab.reshape(-1)[1] == 0                                                  # pixel 1 is no anchor
            assert OR.bad_bits(mm, ll), what
            dm, dl = guards.upload(mm), guards.upload(ll)
            with pytest.raises(ValueError, match=text):
                OB.measure_objects(dm, dl)
            guards.check(what)
            with pytest.raises(ValueError, match=text):
                OB.measure_objects(dm, dl, exclude=(0, 1, 2, 3))                            # with no object kept the planes are still checked
            assert np.array_equal(dm.cpu().numpy(), mm) and np.array_equal(dl.cpu().numpy(), ll)
            guards.clear()
    assert guards.by_name["obj_accumulate"] == 24


def test_two_runs_give_identical_tables(guards):
    m, lab = OC.patterns(33, 300, seed=3)["noise"]
    first = _measure(guards, m, lab)
    for _ in range(2):
        assert OR.same(_measure(guards, m, lab), first)


# ------------------------------------------------------------------------------------------------------------ the vector stage

def _ring_lengths(polys):
    return OR.ring_lengths({k: getattr(polys, k).numpy() for k in ("xy", "ring_start", "poly_ring_start", "poly_rings")})


def test_the_objects_are_the_polygons_of_the_vector_stage(guards):
    from unet_amd import instances as I
    from unet_amd import postprocess as PP
    from unet_amd import vectorize as VZ
    OB = _ob()
    m = OC.noise_mask()
    d = torch.from_numpy(m).cuda()
    polys = VZ.polygonize(d, exclude=2).cpu()
    t = OR.host(OB.measure_objects(d, PP.label_components(d, 4), exclude=2))
    assert OR.same(t, OR.table(m, R.label_components(m, 4), 2)) and len(t["label"]) > 40
    assert np.array_equal(t["label"], polys.poly_label.numpy()) and np.array_equal(t["pixels"], polys.poly_pixels.numpy())
    assert np.array_equal(t["cls"], polys.poly_class.numpy()) and np.array_equal(t["edges_v"] + t["edges_h"], _ring_lengths(polys))
    # an instance split: one component of two discs, cut at its neck
    m = OC.two_blobs()
    d = torch.from_numpy(m).cuda()
    labels = I.split_instances(d, classes=[1], radius=16, min_depth=1.0)[0]
    polys = VZ.polygonize_labels(d, labels, exclude=0).cpu()
    t = OR.host(OB.measure_objects(d, labels, exclude=0))
    assert len(t["label"]) == 2 and OR.same(t, OR.table(m, labels.cpu().numpy(), 0))
    assert np.array_equal(t["label"], polys.poly_label.numpy()) and np.array_equal(t["pixels"], polys.poly_pixels.numpy())
    assert np.array_equal(t["cls"], polys.poly_class.numpy()) and np.array_equal(t["edges_v"] + t["edges_h"], _ring_lengths(polys))
    guards.clear()


# ------------------------------------------------------------------------------------------------------------ prediction entry points

_KEYS = ("perimeter", "centroid_x", "centroid_y", "diameter", "compactness", "on_edge", "point_x", "point_y")


def _features(path):
    return json.load(open(path))["features"]


def _same_file(path, want_rows, tmp_path, gt, epsg=None, class_zero=False):
    """the objects file equals write_objects of the restatement's rows"""
    ref = tmp_path / ("ref_" + os.path.basename(path))
    _ob().write_objects(ref, want_rows, gt, epsg, class_zero=class_zero)
    assert open(path, "rb").read() == ref.read_bytes(), path
    return _features(path)


def _stripped(path):
    """a vector file's features without the added attributes"""
    feats = _features(path)
    for f in feats:
        for k in _KEYS:
            f["properties"].pop(k, None)
    return feats


def test_entry_points_write_the_attributes_of_the_mask_they_return(tmp_path, guards):
    import create_tiles_unet as T
    import predict as P
    from unet_amd import instances as I
    from unet_amd.tiffio import read_tiff
    from test_instances_gpu import _export, _model
    size, gt = ZC.E2E_SIZE, ZC.E2E_GT
    model = _model("xresnet18", 4, 3, size, seed=11)
    pkl = _export(tmp_path, model, 3, size)
    rpath = ZC.e2e_scene(tmp_path)
    kw = dict(max_empty=0.9, batch_size=5)
    plain = P.predict_raster(model, rpath, size, 0.2, out_path=tmp_path / "p.tif", vector_path=tmp_path / "p.geojson", **kw)
    assert "obj_accumulate" not in guards.by_name and len(np.unique(plain)) > 1          # the defaults launch nothing of this family
    comp = R.label_components(plain, 4)
    # the objects file alone
    timing = {}
    got = P.predict_raster(model, rpath, size, 0.2, objects_path=tmp_path / "a.geojson", timing=timing, **kw)
    assert np.array_equal(got, plain)
    rows = OR.rows(OR.table(plain, comp), gt)
    feats = _same_file(tmp_path / "a.geojson", rows, tmp_path, gt)
    assert len(feats) == len(rows) == timing["objects"] > 3 and timing["objects_seconds"] > 0
    assert P.predict_raster(model, rpath, size, 0.2, objects_path=tmp_path / "a.csv", objects_exclude=0, return_array=False, **kw) is None
    assert len(open(tmp_path / "a.csv").read().splitlines()) == 1 + len(OR.table(plain, comp, 0)["label"])
    # with the raster and the vector file: their bytes are those of the call without, apart from the added properties
    got = P.predict_raster(model, rpath, size, 0.2, out_path=tmp_path / "b.tif", vector_path=tmp_path / "b.geojson", objects_path=tmp_path / "b.geojson.pts.geojson",
                           objects_exclude=[1], class_zero=False, **kw)
    assert np.array_equal(got, plain) and (tmp_path / "b.tif").read_bytes() == (tmp_path / "p.tif").read_bytes()
    t1 = OR.table(plain, comp, 1)
    rows1 = OR.rows(t1, gt)
    _same_file(tmp_path / "b.geojson.pts.geojson", rows1, tmp_path, gt)
    assert _stripped(tmp_path / "b.geojson") == _features(tmp_path / "p.geojson")
    by_label = dict(zip(t1["label"].tolist(), rows1))
    polys = _features(tmp_path / "b.geojson")
    all_labels = OR.table(plain, comp)["label"].tolist()                                  # one polygon per component, in label order
    assert len(polys) == len(all_labels)
    for label, f in zip(all_labels, polys):
        if label in by_label:
            assert all(f["properties"][k] == by_label[label][k] for k in _KEYS) and f["properties"]["pixels"] == by_label[label]["pixels"]
        else:
            assert f["properties"]["class"] == 1 and not any(k in f["properties"] for k in _KEYS)
    # with instances the objects are the instances, and carry their ids
    inst = dict(classes=[1, 2], radius=8, min_depth=0.5)
    got = P.predict_raster(model, rpath, size, 0.2, vector_path=tmp_path / "i.geojson", objects_path=tmp_path / "io.geojson", instances=inst,
                           class_zero=True, **kw)
    P.predict_raster(model, rpath, size, 0.2, vector_path=tmp_path / "i1.geojson", instances=inst, class_zero=True, **kw)
    assert np.array_equal(got, plain)
    labels, ids, _ = I.Instances(**inst).run(torch.from_numpy(plain).cuda())
    ti = OR.table(plain, labels.cpu().numpy(), 0)
    rows_i = OR.rows(ti, gt, None, True, ids.cpu().numpy().ravel()[ti["label"]])
    pts = _same_file(tmp_path / "io.geojson", rows_i, tmp_path, gt, class_zero=True)
    assert _stripped(tmp_path / "i.geojson") == _features(tmp_path / "i1.geojson")
    with_attrs = _features(tmp_path / "i.geojson")
    assert len(with_attrs) == len(pts) and max(p["properties"]["instance"] for p in pts) > 0
    for f, p in zip(with_attrs, pts):
        assert all(f["properties"][k] == p["properties"][k] for k in _KEYS + ("class", "pixels", "area", "instance"))
    # the tile-file entry point writes <merged raster stem>_objects.geojson with the vocab's names
    tiles = tmp_path / "cut2"
    T.split_raster(rpath, None, tiles, patch_size=size, patch_overlap=0.2, split=[1], max_empty=0.9)
    f0 = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, AOI="n", validation_vision=False, batch_size=5, vector=True)
    timing = {}
    f = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, AOI="o", validation_vision=False, batch_size=5, vector=True, objects=True,
                           objects_exclude=0, timing=timing)
    assert np.array_equal(read_tiff(f)[0], plain) and f.read_bytes() == f0.read_bytes()
    tags = read_tiff(f)[1]["tags"]
    from unet_amd.vectorize import epsg_of_tags
    named = OR.rows(OR.table(plain, comp, 0), gt, ["c0", "c1", "c2"])
    pts = _same_file(f.with_name(f.stem + "_objects.geojson"), named, tmp_path, gt, epsg_of_tags(tags))
    assert pts[0]["properties"]["name"] in ("c1", "c2") and timing["objects"] == len(named)
    assert _stripped(f.with_suffix(".geojson")) == _features(f0.with_suffix(".geojson"))
    assert not list(tmp_path.rglob("n_*_objects.geojson"))
    guards.check("end")
