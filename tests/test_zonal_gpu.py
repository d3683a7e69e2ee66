"""GPU suite of the zonal statistics (csrc/zonal.hip, unet_amd/zonal.py): the tables against the NumPy restatement of the rules
(tests/zonal_ref.py) on every tail length, alignment, pattern and on both sides of the boundary between the two forms of the kernel; the
objects; bad input; the zone plane of the rasterizer; the round trip through polygonize; the two entry points.  Every comparison is exact
equality.  Every buffer a kernel writes sits in a guard-banded allocation and every input between canaries; all of them are checked after
every launcher, and the inputs are compared unchanged afterwards."""
import csv
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import rasterize_cases as RC  # noqa: E402
import rasterize_ref as RR  # noqa: E402
import zonal_cases as ZC  # noqa: E402
import zonal_ref as ZR  # noqa: E402
from guard import canary_input, guarded  # noqa: E402

_FILL = {torch.uint8: 0xA5, torch.int32: -7, torch.int64: -7}
_LAUNCHERS = ("ras_count", "ras_scan", "ras_emit", "ras_spans", "ras_resolve", "ras_resolve_ids", "zonal_counts", "vec_read")
SHAPES = [(1, 1), (1, 3), (1, 4), (1, 5), (3, 15), (2, 16), (3, 17), (5, 63), (7, 257), (33, 300)]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "zonal_default_outputs.json")


def _zn():
    from unet_amd import zonal
    return zonal


def _rz():
    from unet_amd import rasterize
    return rasterize


class Guards:
    def __init__(self):
        self.checks, self.launches, self.by_name = [], 0, {}

    def alloc(self, shape, dtype, device):
        t, c = guarded(shape, dtype, device, _FILL[dtype])
        self.checks.append(c)
        return t

    def upload(self, a) -> torch.Tensor:
        """a host array or any tensor -> a device copy between canaries (int64 has no canary in tests/guard.py: a sentinel band instead)"""
        a = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.detach().cpu().contiguous()
        if a.dtype == torch.int64:
            t, c = guarded(a.shape, a.dtype, "cuda", -(2 ** 62))
            t.copy_(a)
        else:
            t, c = canary_input(a)
        self.checks.append(c)
        return t

    def rings(self, r):
        return _rz().Rings(self.upload(r.xy), self.upload(r.ring_start), self.upload(r.feature_ring_start), self.upload(r.values))

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
    monkeypatch.setattr(_rz(), "_alloc", g.alloc)
    monkeypatch.setattr(_zn(), "_alloc", g.alloc)
    for name in _LAUNCHERS:
        def wrapped(*a, _fn=getattr(ops, name), _name=name, **k):
            r = _fn(*a, **k)
            g.launches += 1
            g.by_name[_name] = g.by_name.get(_name, 0) + 1
            g.check(_name)
            return r
        monkeypatch.setattr(ops, name, wrapped)
    return g


def _tables(guards, z, m, Z, C, labels=None):
    """zonal_counts on guarded copies; the inputs come back unchanged; returns the host tables (counts, objects or None)"""
    dz, dm = guards.upload(z), guards.upload(m)
    dl = None if labels is None else guards.upload(labels)
    stats = _zn().zonal_counts(dz, dm, Z, C, dl)
    assert stats.counts.is_cuda and stats.counts.dtype == torch.int64 and tuple(stats.counts.shape) == (Z, C)
    assert (stats.objects is None) == (labels is None)
    assert np.array_equal(dz.cpu().numpy(), z) and np.array_equal(dm.cpu().numpy(), m) and (labels is None or np.array_equal(dl.cpu().numpy(), labels))
    host = stats.cpu()
    guards.clear()
    return host.counts.numpy(), None if labels is None else host.objects.numpy()


def _own_labels(z, m):
    """a label image in the module's convention without a connectivity rule: the pixels of one (zone, class) pair form one object"""
    key = z.astype(np.int64).ravel() * 256 + m.ravel()
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    return first[inverse].astype(np.int32).reshape(z.shape)


def _check(guards, z, m, Z, C, what, labels=None):
    want, bad = ZR.counts(z, m, Z, C)
    assert not bad
    got, obj = _tables(guards, z, m, Z, C, labels)
    assert np.array_equal(got, want), what
    assert int(got.sum()) == int((z >= 0).sum())
    if labels is not None:
        assert np.array_equal(obj, ZR.objects(z, m, labels, Z, C)), what
    return got


# ------------------------------------------------------------------------------------------------------------ shapes x patterns x sizes

@pytest.mark.parametrize("shape", SHAPES)
def test_patterns_equal_the_reference_on_every_tail_and_around_the_form_boundary(guards, shape):
    from unet_amd import ops
    bins = ops.zonal_lds_bins()
    H, W = shape
    sizes = [(7, 1), (7, 5), (7, 256),                                                    # the LDS form, C in {1, 5, 256}
             (bins - 1, 1), (bins, 1), (bins + 1, 1), (4 * bins, 1),                      # Z * C at bins - 1, bins, bins + 1, 4 bins
             (bins // 256, 256), (bins // 256 + 1, 256), (bins // 5, 5), (bins // 5 + 1, 5), (4 * bins // 5 + 1, 5)]
    assert bins % 256 == 0 and bins // 5 * 5 <= bins < (bins // 5 + 1) * 5
    launches = 0
    for Z, C in sizes:
        patterns = ZC.zone_patterns(H, W, Z, C, seed=H * 1000 + W)
        assert set(patterns) == {"none", "one", "blocks", "checker", "stripes", "random"}
        launches += len(patterns)
        for name, (z, m) in patterns.items():
            got = _check(guards, z, m, Z, C, (shape, Z, C, name), labels=_own_labels(z, m) if name in ("blocks", "stripes", "random") else None)
            if name == "none":
                assert not got.any()
            else:
                assert got[Z - 1, C - 1] >= 1                                             # the largest zone index and class are populated
            if name == "one":
                assert got[Z - 1, C - 1] == H * W and int(got.sum()) == H * W
    assert guards.by_name["zonal_counts"] == launches


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_planes_at_addresses_that_are_only_element_aligned(guards, shift):
    # views that start `shift` elements into guarded allocations: no 16-byte access is possible, and none may touch the bands
    ZN = _zn()
    for (H, W), Z, C in (((3, 17), 7, 5), ((33, 300), 2000, 5), ((1, 1), 1, 1)):
        z, m = ZC.zone_patterns(H, W, Z, C, seed=shift)["random"]
        lab = _own_labels(z, m)
        n = H * W
        bufs = []
        for a in (z, m, lab):
            flat = guards.upload(np.concatenate([np.full(shift, a.reshape(-1)[0], a.dtype), a.reshape(-1)]))
            bufs.append(flat[shift:shift + n].view(H, W))
        assert bufs[0].data_ptr() % 16 != 0 and bufs[0].is_contiguous()
        stats = ZN.zonal_counts(bufs[0], bufs[1], Z, C, bufs[2]).cpu()
        guards.clear()
        assert np.array_equal(stats.counts.numpy(), ZR.counts(z, m, Z, C)[0]) and np.array_equal(stats.objects.numpy(), ZR.objects(z, m, lab, Z, C))
        # one plane aligned, the others not
        stats = ZN.zonal_counts(guards.upload(z), bufs[1], Z, C).cpu()
        guards.clear()
        assert np.array_equal(stats.counts.numpy(), ZR.counts(z, m, Z, C)[0])


def test_both_forms_give_identical_tables_on_one_input(guards):
    from unet_amd import ops
    bins = ops.zonal_lds_bins()
    H, W, Z, C = 33, 300, 40, 5
    z, m = ZC.zone_patterns(H, W, Z, C, seed=77)["random"]
    z[10:20, 100:300] = 3                                                                 # wavefronts with one key among mixed ones
    lab = _own_labels(z, m)
    padded = bins // C + 1
    assert Z * C <= bins < padded * C
    lds, lds_obj = _tables(guards, z, m, Z, C, lab)
    direct, direct_obj = _tables(guards, z, m, padded, C, lab)
    assert np.array_equal(direct[:Z], lds) and not direct[Z:].any() and np.array_equal(direct_obj[:Z], lds_obj) and not direct_obj[Z:].any()
    assert np.array_equal(lds, ZR.counts(z, m, Z, C)[0]) and lds.sum() == (z >= 0).sum()


@pytest.mark.parametrize("Z", [12, 3000])
def test_spans_of_several_steps_per_wavefront(guards, Z):
    # 4.2 M pixels: more groups of 4 than the largest grid holds lanes, so every wavefront walks a span of several steps and carries its
    # pending key from step to step -- through zones wider than a span, zone changes inside a span, and rows that are no multiple of 4
    H, W, C = 2049, 2051, 5
    rng = np.random.default_rng(Z)
    yy, xx = np.mgrid[0:H, 0:W]
    z = ((yy // 700) * 4 + xx // 600).astype(np.int32) % Z
    z[:300] = Z - 1                                                                       # 600 k pixels of one key on end
    z[1000:1003] = -1
    m = ((yy // 90 + xx // 1100) % C).astype(np.uint8)
    m[:300] = C - 1
    noisy = rng.random((H, W)) < 0.001
    m[noisy] = rng.integers(0, C, int(noisy.sum()), dtype=np.uint8)
    lab = _own_labels(z, m)
    want = np.bincount((z.astype(np.int64) * C + m).ravel()[z.ravel() >= 0], minlength=Z * C).reshape(Z, C)
    assert np.array_equal(want, ZR.counts(z, m, Z, C)[0])
    got, obj = _tables(guards, z, m, Z, C, lab)
    assert np.array_equal(got, want) and np.array_equal(obj, ZR.objects(z, m, lab, Z, C))
    assert got[Z - 1, C - 1] >= 300 * W - int(noisy[:300].sum())


def test_determinism_over_runs(guards):
    z, m = ZC.zone_patterns(33, 300, 9, 5, seed=3)["random"]
    lab = _own_labels(z, m)
    first = _tables(guards, z, m, 9, 5, lab)
    for _ in range(3):
        again = _tables(guards, z, m, 9, 5, lab)
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])


# ------------------------------------------------------------------------------------------------------------ objects

def test_objects_of_components_and_of_instances(guards):
    from unet_amd import instances as I
    from unet_amd import postprocess as PP
    m = RC.mask(67, 93, seed=21, salt=0.01)
    H, W = m.shape
    yy, xx = np.mgrid[0:H, 0:W]
    z = ((yy // 20) * 3 + xx // 40).astype(np.int32)
    z[30:40, 50:70] = -1
    Z, C = int(z.max()) + 1, 5
    d = torch.from_numpy(m).cuda()
    comp = PP.label_components(d, 4).cpu().numpy()
    inst = I.split_instances(d, classes=[1, 2], radius=8, min_depth=0.5)[0].cpu().numpy()
    assert (inst != comp).any()
    for labels in (comp, inst):
        counts, objects = _tables(guards, z, m, Z, C, labels)
        assert np.array_equal(counts, ZR.counts(z, m, Z, C)[0]) and np.array_equal(objects, ZR.objects(z, m, labels, Z, C))
        anchors = labels.ravel() == np.arange(H * W)
        assert int(objects.sum()) == int((anchors & (z.ravel() >= 0)).sum()) > Z          # every object once, in the zone of its first pixel
        assert (objects <= counts).all()
    assert _tables(guards, z, m, Z, C)[1] is None                                          # labels=None leaves objects None


def test_anchors_at_the_first_pixel_the_last_pixel_and_in_the_scalar_tail(guards):
    H, W, Z, C = 3, 17, 4, 3                                                              # 51 pixels: 48, 49 and 50 are the tail
    z = np.full((H, W), 2, dtype=np.int32)
    m = np.ones((H, W), dtype=np.uint8)
    lab = np.zeros((H, W), dtype=np.int32)                                                # one object anchored at pixel 0 ...
    for p, zone, cls in ((49, 3, 2), (50, 0, 0)):                                         # ... and two one-pixel objects in the tail
        lab.reshape(-1)[p], z.reshape(-1)[p], m.reshape(-1)[p] = p, zone, cls
    counts, objects = _tables(guards, z, m, Z, C, lab)
    assert objects.tolist() == [[1, 0, 0], [0, 0, 0], [0, 1, 0], [0, 0, 1]] and np.array_equal(objects, ZR.objects(z, m, lab, Z, C))
    assert counts.tolist() == [[1, 0, 0], [0, 0, 0], [0, 49, 0], [0, 0, 1]]
    z.reshape(-1)[0] = -1                                                                 # an object whose first pixel lies in no zone is counted nowhere
    assert _tables(guards, z, m, Z, C, lab)[1].tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 1]]


# ------------------------------------------------------------------------------------------------------------ bad input

@pytest.mark.parametrize("shape", [(3, 17), (33, 300)])
@pytest.mark.parametrize("Z", [6, 4000])
def test_bad_pixels_are_counted_nowhere_and_raise(guards, shape, Z):
    from unet_amd import ops
    ZN = _zn()
    H, W = shape
    C = 5
    z0, m0 = ZC.zone_patterns(H, W, Z, C, seed=9)["random"]
    for what, plane, value, bit in (("mask = C", "m", C, 1), ("zone = Z", "z", Z, 2), ("zone = -2", "z", -2, 2)):
        z, m = z0.copy(), m0.copy()
        for p in (0, H * W // 2, H * W - 1):                                              # the first pixel, the middle, the tail
            (m if plane == "m" else z).reshape(-1)[p] = value
            if plane == "m":
                z.reshape(-1)[p] = 1                                                      # inside a zone, so that it would have counted
        want, bad = ZR.counts(z, m, Z, C)
        keep = np.ones(H * W, dtype=bool)
        keep[[0, H * W // 2, H * W - 1]] = False
        removed = ZR.counts(np.where(keep.reshape(H, W), z, -1), np.where(keep.reshape(H, W), m, 0), Z, C)[0]
        assert bad and np.array_equal(want, removed)
        lab = _own_labels(z, m)
        dz, dm, dl = guards.upload(z), guards.upload(m), guards.upload(lab)
        counts, objects, word = guards.alloc((Z, C), torch.int64, "cuda").zero_(), guards.alloc((Z, C), torch.int64, "cuda").zero_(), guards.alloc((1,), torch.int64, "cuda")
        ops.zonal_counts(dz, dm, dl, Z, C, counts, objects, word)
        assert int(word.cpu()[0]) == bit, what
        assert np.array_equal(counts.cpu().numpy(), want), what                           # the tables of all other pixels
        assert np.array_equal(objects.cpu().numpy(), ZR.objects(z, m, lab, Z, C)), what
        with pytest.raises(ValueError, match="value >= 5" if plane == "m" else "outside -1"):
            ZN.zonal_counts(dz, dm, Z, C)
        guards.clear()


def test_confusion_matrix_is_the_case_zones_equal_truth(guards):
    C = 5
    truth, pred = RC.mask(67, 93, seed=1, classes=C), RC.mask(67, 93, seed=2, classes=C)
    got, _ = _tables(guards, truth.astype(np.int32), pred, C, C)
    assert np.array_equal(got.ravel(), np.bincount(truth.astype(np.int64).ravel() * C + pred.ravel(), minlength=C * C))
    assert np.array_equal(np.diag(got), [int(((truth == c) & (pred == c)).sum()) for c in range(C)])


# ------------------------------------------------------------------------------------------------------------ rasterize_ids

_SETS = RC.feature_sets()


def _host_rings(features):
    RZ = _rz()
    xy, rs, frs, vals = RR.pack(features)
    return RZ.Rings(torch.from_numpy(xy), torch.from_numpy(rs), torch.from_numpy(frs), torch.from_numpy(vals))


def _ids(guards, rings, shape):
    d = guards.rings(rings)
    stages = {}
    got = _zn().rasterize_ids(d, shape, stages)
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == tuple(shape)
    assert stages["pair_mismatch"] == 0 and stages["features"] == rings.n_features and "resolve" in stages
    for k in ("xy", "ring_start", "feature_ring_start", "values"):
        assert torch.equal(getattr(d, k).cpu(), getattr(rings, k))
    host = got.cpu().numpy()
    guards.clear()
    return host


@pytest.mark.parametrize("name", sorted(_SETS))
def test_ids_equal_the_reference_and_agree_with_rasterize(guards, name):
    RZ = _rz()
    shape = ZC.SHAPE
    rings = _host_rings(_SETS[name])
    before = dict(guards.by_name)
    ids = _ids(guards, rings, shape)
    assert guards.by_name.get("ras_resolve_ids", 0) == before.get("ras_resolve_ids", 0) + 1 and "ras_resolve" not in guards.by_name
    xy, rs, frs, vals = RR.pack(_SETS[name])
    assert np.array_equal(ids, ZR.ids(xy, rs, frs, shape)), name
    assert ids.min() >= -1 and ids.max() < max(len(vals), 1)
    burnt = RZ.rasterize(guards.rings(rings), shape, fill=255).cpu().numpy()               # rasterize() launches what it launched: its own resolve
    guards.clear()
    assert guards.by_name["ras_resolve"] == 1 and guards.by_name["ras_resolve_ids"] == before.get("ras_resolve_ids", 0) + 1
    inside = ids >= 0
    assert np.array_equal(vals[ids[inside]], burnt[inside]), name
    if 255 not in vals.tolist():
        assert np.array_equal(~inside, burnt == 255), name                                 # -1 exactly where the fill was kept
    if name in ("none", "degenerate"):
        assert (name == "none") == (not inside.any())
    if name == "overlap50":
        assert 255 not in vals.tolist()
        # the painter's order: of all features whose fill holds a pixel the highest index wins
        top = np.full(shape, -1)
        for f, (_, feature_rings) in enumerate(_SETS[name]):
            top[RR.feature_mask(feature_rings, *shape)] = f
        assert np.array_equal(ids, top) and len(np.unique(ids)) > 20


def test_ids_of_300_features_do_not_fit_a_byte(guards):
    ONE = RC.ONE
    shape = (40, 56)
    feats = []
    for f in range(300):                                                                   # 2 x 3 boxes in rows of 28, each half over the next one
        y, x = (f // 28) * 3, (f % 28) * 2
        feats.append((f % 251, [[(x * ONE, y * ONE), (x * ONE, (y + 4) * ONE), ((x + 3) * ONE, (y + 4) * ONE), ((x + 3) * ONE, y * ONE)]]))
    ids = _ids(guards, _host_rings(feats), shape)
    xy, rs, frs, _ = RR.pack(feats)
    assert np.array_equal(ids, ZR.ids(xy, rs, frs, shape)) and ids.max() == 299 and (ids > 255).sum() > 50
    counts, _ = _tables(guards, ids, np.zeros(shape, dtype=np.uint8), 300, 1)
    assert np.array_equal(counts.ravel(), np.bincount(ids[ids >= 0], minlength=300)) and counts[299, 0] > 0


def test_round_trip_through_polygonize(guards):
    from unet_amd import vectorize as VZ
    m = RC.mask(67, 93, seed=8)
    d = torch.from_numpy(m).cuda()
    polys = VZ.polygonize(d)
    ids = _zn().rasterize_ids(polys, m.shape)
    stats = _zn().zonal_counts(ids, d, polys.n_polygons, 5).cpu()
    guards.clear()
    counts = stats.counts.numpy()
    assert (ids >= 0).all() and ((counts != 0).sum(axis=1) == 1).all()                     # exactly one non-zero column per zone ...
    host = polys.cpu()
    assert np.array_equal(counts.sum(axis=1), host.poly_pixels.numpy().astype(np.int64))   # ... equal to poly_pixels ...
    assert np.array_equal(counts.argmax(axis=1), host.poly_class.numpy().astype(np.int64))   # ... in the column of the polygon's class


# ------------------------------------------------------------------------------------------------------------ prediction entry points

def _zones_document(gt, H, W):
    """zones in map coordinates on a grid of H x W pixels: two that overlap, one partly and one wholly outside the raster, one feature
    without a geometry, a MultiPolygon of two parts, one with a hole"""
    def ring(x0, y0, x1, y1):
        return [[gt[0] + x * gt[1], gt[3] + y * gt[5]] for x, y in ((x0, y0), (x0, y1), (x1, y1), (x1, y0), (x0, y0))]
    polygon = lambda *r: {"type": "Polygon", "coordinates": list(r)}  # noqa: E731
    feats = [("north", polygon(ring(0, 0, W, 30.5))), ("nothing", None), ("over", polygon(ring(20.25, 10, 70, 60))),
             ("edge", polygon(ring(W - 20, H - 25.5, W + 40, H + 30))), ("far", polygon(ring(W + 5, 0, W + 50, 40))),
             ("holed", polygon(ring(2, 40, 40, H - 2), ring(10, 50, 30, H - 12))),
             ("parts", {"type": "MultiPolygon", "coordinates": [[ring(45, 62, 60, 80)], [ring(62, 62, 75.5, 70)]]})]
    return {"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {"parcel": n, "nr": i}, "geometry": g} for i, (n, g) in enumerate(feats)]}


def _reference_rows(zones_path, gt, mask, names, class_zero, labels=None):
    """the added properties per zone from the returned mask: read_zones' rings through the reference rasterizer and the reference tables"""
    rings, feats = _zn().read_zones(zones_path, gt)
    ids = ZR.ids(rings.xy.numpy(), rings.ring_start.numpy(), rings.feature_ring_start.numpy(), mask.shape)
    C = len(names) if names is not None else int(mask.max()) + 1
    counts, bad = ZR.counts(ids, mask, len(feats), C)
    assert not bad
    objects = None if labels is None else ZR.objects(ids, mask, labels, len(feats), C)
    return feats, ZR.rows(counts, objects, names, abs(gt[1] * gt[5]), class_zero), counts


def _same_table(path, feats, rows):
    doc = json.load(open(path))
    assert len(doc["features"]) == len(feats) == len(rows)
    for f, src, row in zip(doc["features"], feats, rows):
        assert f["geometry"] == src["geometry"] and f["properties"] == {**src["properties"], **row}, src["properties"]


def test_entry_points_write_the_table_of_the_mask_they_return(tmp_path, guards):
    import create_tiles_unet as T
    import predict as P
    import postprocess_ref as R
    from unet_amd import instances as I
    from unet_amd.tiffio import read_tiff
    from test_instances_gpu import _export, _model
    size, gt = ZC.E2E_SIZE, ZC.E2E_GT
    model = _model("xresnet18", 4, 3, size, seed=11)
    pkl = _export(tmp_path, model, 3, size)
    # the defaults: what the commit before this stage returned and wrote, by its recorded digests; no launch of this family
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert ZC.default_outputs(P, T, tmp_path, model, pkl) == golden
    assert not any(k in guards.by_name for k in ("zonal_counts", "ras_resolve_ids", "ras_count", "ras_spans"))
    assert not list(tmp_path.rglob("*_zonal.geojson")) and not list(tmp_path.rglob("*.csv"))
    rpath = tmp_path / "scene.tif"
    kw = dict(max_empty=0.9, batch_size=5)
    plain = P.predict_raster(model, rpath, size, 0.2, **kw)
    H, W = plain.shape
    assert len(np.unique(plain)) > 1
    zpath = tmp_path / "zones.geojson"
    zpath.write_text(json.dumps(_zones_document(gt, H, W)))
    # predict_raster: the GeoJSON table, then the CSV with objects (components) under class_zero
    timing = {}
    got = P.predict_raster(model, rpath, size, 0.2, zones_path=zpath, zonal_path=tmp_path / "t.geojson", out_path=tmp_path / "t.tif", timing=timing, **kw)
    assert np.array_equal(got, plain) and np.array_equal(read_tiff(tmp_path / "t.tif")[0], plain)
    feats, rows, counts = _reference_rows(zpath, gt, plain, None, False)
    _same_table(tmp_path / "t.geojson", feats, rows)
    assert [f["properties"]["parcel"] for f in feats] == ["north", "over", "edge", "far", "holed", "parts"]
    assert rows[3]["pixels"] == 0 and rows[3]["majority"] is None and rows[2]["pixels"] == 20 * 26 and rows[0]["pixels"] < 30 * W   # `over` wins its overlap with `north`
    assert timing["zonal_seconds"] > 0 and timing["zonal_zones"] == 6 and timing["zonal_pixels"] == int(counts.sum()) > 0
    none = P.predict_raster(model, rpath, size, 0.2, zones_path=zpath, zonal_path=tmp_path / "t.csv", zonal_objects=True, class_zero=True,
                            return_array=False, **kw)
    assert none is None
    comp = R.label_components(plain, 4)
    feats, rows, _ = _reference_rows(zpath, gt, plain, None, True, comp)
    with open(tmp_path / "t.csv", newline="") as f:
        table = list(csv.reader(f))
    added = list(rows[0])
    assert table[0] == ["parcel", "nr"] + added and "px_nodata" in added and any(k.startswith("n_") for k in added)
    for line, src, row in zip(table[1:], feats, rows):
        assert line == [src["properties"]["parcel"], str(src["properties"]["nr"])] + ["" if row[k] is None else str(row[k]) for k in added]
    # with instances the objects are the instances
    inst = dict(classes=[1, 2], radius=8, min_depth=0.5)
    P.predict_raster(model, rpath, size, 0.2, zones_path=zpath, zonal_path=tmp_path / "i.geojson", zonal_objects=True, instances=inst, **kw)
    labels = I.split_instances(torch.from_numpy(plain).cuda(), **inst)[0].cpu().numpy()
    feats, rows_inst, _ = _reference_rows(zpath, gt, plain, None, False, labels)
    _same_table(tmp_path / "i.geojson", feats, rows_inst)
    # the tile-file entry point writes <merged raster stem>_zonal.geojson with the vocab's names
    tiles = tmp_path / "cut2"
    T.split_raster(rpath, None, tiles, patch_size=size, patch_overlap=0.2, split=[1], max_empty=0.9)
    timing = {}
    f = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, AOI="z", validation_vision=False, batch_size=5, zones=zpath, zonal_objects=True,
                           timing=timing)
    assert np.array_equal(read_tiff(f)[0], plain)
    feats, rows_named, _ = _reference_rows(zpath, gt, plain, ["c0", "c1", "c2"], False, comp)
    _same_table(f.with_name(f.stem + "_zonal.geojson"), feats, rows_named)
    assert "px_c1" in rows_named[0] and "n_c2" in rows_named[0] and timing["zonal_zones"] == 6
    f = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, AOI="y", validation_vision=False, batch_size=5, zones=zpath, zonal_objects=True,
                           instances=inst)
    _same_table(f.with_name(f.stem + "_zonal.geojson"), feats, _reference_rows(zpath, gt, plain, ["c0", "c1", "c2"], False, labels)[1])
    guards.check("end")
