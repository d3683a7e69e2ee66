"""GPU suite of the rasterizer (csrc/rasterize.hip, unet_amd/rasterize.py): rasterize(polygonize(mask)) == mask without any
reference, the device mask against the plain-Python restatement of the rules (tests/rasterize_ref.py) on polygons that the tracer never
produces, the partition along a shared oblique border, long spans and tall edges, the bookkeeping words, and the file entry points.  Every
comparison is exact equality.  Every device buffer of the module sits in a guard-banded allocation and every input between canaries; all of
them are checked after every launcher."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import rasterize_cases as RC  # noqa: E402
import rasterize_ref as RR  # noqa: E402
from guard import canary_input, guarded  # noqa: E402

_FILL = {torch.uint8: 0xA5, torch.int32: -7, torch.int64: -7}
_LAUNCHERS = ("ras_count", "ras_scan", "ras_emit", "ras_spans", "ras_resolve", "vec_read")
GT = (500000.0, 0.25, 0.0, 5600000.0, 0.0, -0.25)          # exact in float64, as every coordinate it produces here


def _rz():
    from unet_amd import rasterize
    return rasterize


def _vz():
    from unet_amd import vectorize
    return vectorize


class Guards:
    def __init__(self):
        self.checks, self.launches, self.mismatch = [], 0, []

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
        RZ = _rz()
        return RZ.Rings(self.upload(r.xy), self.upload(r.ring_start), self.upload(r.feature_ring_start), self.upload(r.values))

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
    for name in _LAUNCHERS:
        def wrapped(*a, _fn=getattr(ops, name), _name=name, **k):
            r = _fn(*a, **k)
            g.launches += 1
            g.check(_name)
            if _name == "ras_spans":
                g.mismatch.append(int(a[5].cpu()[0]))          # the pair-mismatch word of every call
            return r
        monkeypatch.setattr(ops, name, wrapped)
    return g


def _same_inputs(dev, host):
    for k in ("xy", "ring_start", "feature_ring_start", "values"):
        assert torch.equal(getattr(dev, k).cpu(), getattr(host, k).cpu()), k          # the inputs are never written


def _burn(guards, rings, shape, fill=0, out=None):
    """rasterize on guarded copies of the rings; returns the host array"""
    RZ = _rz()
    d = guards.rings(rings)
    stages = {}
    got = RZ.rasterize(d, shape, fill, out, stages)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == tuple(shape)
    assert stages["pair_mismatch"] == 0 and stages["features"] == rings.n_features and stages["crossings"] % 2 == 0
    assert all(stages[k] >= 0 for k in ("spans", "resolve"))
    _same_inputs(d, rings)
    host = got.cpu().numpy()
    guards.clear()
    assert guards.mismatch and not any(guards.mismatch)
    return host


def _host_rings(features):
    RZ = _rz()
    xy, rs, frs, vals = RR.pack(features)
    return RZ.Rings(torch.from_numpy(xy), torch.from_numpy(rs), torch.from_numpy(frs), torch.from_numpy(vals))


# ------------------------------------------------------------------------------------------------------------ round trip, no reference

@pytest.mark.parametrize("shape", [(67, 93), (1, 1), (1, 64), (64, 1), (130, 257)])
def test_round_trip_of_polygonize(guards, shape):
    RZ, VZ = _rz(), _vz()
    m = RC.mask(*shape, seed=shape[0] + shape[1])
    d = torch.from_numpy(m).cuda()
    polys = VZ.polygonize(d)
    assert np.array_equal(_burn(guards, RZ.rings_from_polygons(polys), shape, fill=9), m)
    if shape == (67, 93):
        host = polys.cpu()
        assert (np.diff(host.poly_ring_start.numpy()) > 1).any() and len(np.unique(m)) == 5          # holes occur
        # Polygons go in directly, and excluded classes come back as the fill
        assert np.array_equal(RZ.rasterize(polys, shape).cpu().numpy(), m)
        want = m.copy()
        want[(m == 0) | (m == 3)] = 7
        assert np.array_equal(_burn(guards, RZ.rings_from_polygons(VZ.polygonize(d, exclude=(0, 3))), shape, fill=7), want)
        # simplified at tolerance 0 the rings still bound the same pixels
        assert np.array_equal(RZ.rasterize(VZ.polygonize(d, simplify=0), shape, fill=9).cpu().numpy(), m)


def test_round_trip_of_the_instances(guards):
    from unet_amd import instances as I
    RZ, VZ = _rz(), _vz()
    m = RC.mask(67, 93, seed=21, salt=0.01)
    d = torch.from_numpy(m).cuda()
    labels, info = I.split_instances(d, classes=[1, 2], radius=8, min_depth=0.5)
    polys = VZ.polygonize_labels(d, labels)
    assert polys.n_polygons >= VZ.polygonize(d).n_polygons
    assert np.array_equal(_burn(guards, RZ.rings_from_polygons(polys, values=polys.poly_class), m.shape, fill=9), m)


# ------------------------------------------------------------------------------------------------------------ against the reference

_SETS = RC.feature_sets()
_REF = {}


def _ref(name, shape, fill, out=None):
    key = (name, fill, out is not None)
    if key not in _REF:
        _REF[key] = RR.rasterize(*RR.pack(_SETS[name]), shape, fill, out)
    return _REF[key]


@pytest.mark.parametrize("name", sorted(_SETS))
def test_feature_sets_equal_the_reference(guards, name):
    shape = (40, 56)
    rings = _host_rings(_SETS[name])
    got = _burn(guards, rings, shape, fill=4)
    assert np.array_equal(got, _ref(name, shape, 4)), name
    if name not in ("none", "degenerate"):
        assert len(np.unique(got)) > 2
    if name == "none":
        assert (got == 4).all()
    # the same with out= prefilled with a random mask: burnt in place, uncovered pixels keep what it held
    pre = RC.mask(*shape, seed=5, classes=250, salt=0.5)
    out, check = guarded(shape, torch.uint8, "cuda", 0x5A)
    out.copy_(torch.from_numpy(pre))
    got = _rz().rasterize(guards.rings(rings), shape, fill=4, out=out)
    check(name)
    guards.clear()
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), _ref(name, shape, 4, pre)), name


def test_out_at_an_address_that_is_not_16_byte_aligned(guards):
    shape = (40, 56)
    rings = _host_rings(_SETS["overlap50"])
    pre = RC.mask(*shape, seed=6, classes=250, salt=0.5)
    want = RR.rasterize(*RR.pack(_SETS["overlap50"]), shape, 0, pre)
    flat, check = guarded((shape[0] * shape[1] + 16,), torch.uint8, "cuda", 0x5A)
    for shift in (1, 7):
        flat.fill_(0x5A)
        out = flat[shift:shift + shape[0] * shape[1]].view(shape)
        out.copy_(torch.from_numpy(pre))
        _rz().rasterize(guards.rings(rings), shape, out=out)
        check(f"shift {shift}")
        guards.clear()
        assert np.array_equal(out.cpu().numpy(), want)
        assert (flat[:shift] == 0x5A).all() and (flat[shift + shape[0] * shape[1]:] == 0x5A).all()


def test_scan_over_several_blocks_and_at_unaligned_addresses(guards):
    # 2048 counts per block and 1024 block sums per pass of the one-block scan: the last size takes a second pass; the sums pass 2^32
    from unet_amd import ops
    rng = np.random.default_rng(3)
    for n, shift in ((1, 0), (2047, 0), (2048, 0), (2049, 1), (70001, 3), (2048 * 1024 + 4097, 0)):
        c = rng.integers(0, 2 ** 20, n).astype(np.int32)
        src = guards.upload(np.concatenate([np.full(shift, 12345, np.int32), c]))[shift:]
        offs = guards.alloc((n + shift,), torch.int64, "cuda")[shift:]
        blocks, info = guards.alloc((ops.ras_scan_words(n),), torch.int64, "cuda"), guards.alloc((2,), torch.int64, "cuda")
        ops.ras_scan(src, n, offs, blocks, info)
        want = np.concatenate([[0], np.cumsum(c.astype(np.int64))])
        assert np.array_equal(offs.cpu().numpy(), want[:-1]) and int(info.cpu()[0]) == want[-1], (n, shift)
        guards.clear()


# ------------------------------------------------------------------------------------------------------------ partition

@pytest.mark.parametrize("s", [1, 3])
def test_two_features_that_share_an_oblique_border_partition_the_pixels(guards, s):
    a, b = RC.oblique_halves(s)
    ab = _burn(guards, _host_rings([(1, [a]), (2, [b])]), (64, 64), fill=0)
    ba = _burn(guards, _host_rings([(2, [b]), (1, [a])]), (64, 64), fill=0)
    only_a = _burn(guards, _host_rings([(1, [a])]), (64, 64), fill=0)
    only_b = _burn(guards, _host_rings([(2, [b])]), (64, 64), fill=0)
    assert np.isin(ab, (1, 2)).all()                                  # no pixel belongs to neither
    assert np.array_equal(ab, ba)                                     # nor to both: the order changes no pixel
    assert np.array_equal(only_a + only_b, ab) and (only_a == 1).any() and (only_b == 2).any()
    assert np.array_equal(ab, RR.rasterize(*RR.pack([(1, [a]), (2, [b])]), (64, 64)))
    # the centres on the line itself go to the feature right of it
    assert all(ab[i, s * i] == 2 for i in range(64) if s * i < 64)


# ------------------------------------------------------------------------------------------------------------ long spans, tall edges

@pytest.mark.parametrize("shape", [(3, 5000), (5000, 3)])
def test_long_spans_and_many_rows(guards, shape):
    H, W = shape
    cover = [(0, 0), (0, H * 256), (W * 256, H * 256), (W * 256, 0)]
    assert (_burn(guards, _host_rings([(201, [cover])]), shape, fill=4) == 201).all()
    # an oblique triangle over the whole raster on top: one edge crosses every row, and its spans run over many columns
    tri = [(-256, -256), (W * 256 + 300, H * 128), (-100, H * 256 + 256)]
    feats = [(201, [cover]), (17, [tri])]
    got = _burn(guards, _host_rings(feats), shape, fill=4)
    assert np.array_equal(got, RR.rasterize(*RR.pack(feats), shape, 4))
    assert (got == 17).sum() > H * W // 4 and (got == 201).any()


# ------------------------------------------------------------------------------------------------------------ determinism, bookkeeping

def test_two_runs_and_permuted_rings_are_equal(guards):
    RZ = _rz()
    shape = (40, 56)
    feats = _SETS["multi"] + _SETS["overlap50"]
    first = _burn(guards, _host_rings(feats), shape)
    assert np.array_equal(_burn(guards, _host_rings(feats), shape), first)
    permuted = [(v, rings[::-1]) for v, rings in feats]
    assert len(feats[0][1]) == 4 and np.array_equal(_burn(guards, _host_rings(permuted), shape), first)
    rotated = [(v, [r[2:] + r[:2] for r in rings]) for v, rings in feats]                  # another first vertex, the same rings
    assert np.array_equal(_burn(guards, _host_rings(rotated), shape), first)
    assert np.array_equal(first, RR.rasterize(*RR.pack(feats), shape))
    assert guards.launches > 0 and not any(guards.mismatch)
    stages = {}
    RZ.rasterize(_host_rings(feats), shape, stages=stages)                                 # host Rings are uploaded
    assert set(stages) == {"count", "scan", "emit", "sort", "spans", "resolve", "crossings", "features", "pair_mismatch"}
    assert stages["pair_mismatch"] == 0 and stages["crossings"] > 0 and stages["features"] == len(feats)


def test_coordinates_beyond_the_limit_are_refused_on_the_device(guards):
    RZ = _rz()
    far = 2 ** 29 + 1
    for ring in ([(0, 0), (0, 512), (far, 512)], [(0, -far), (0, 512), (512, 512)]):
        r = _host_rings([(1, [ring])])
        with pytest.raises(ValueError):
            RZ.rasterize(RZ.Rings(r.xy.cuda(), r.ring_start.cuda(), r.feature_ring_start.cuda(), r.values.cuda()), (4, 4))
    ok = _burn(guards, _host_rings([(1, [[(-2 ** 29, -2 ** 29), (-2 ** 29, 2 ** 29), (2 ** 29, 2 ** 29), (2 ** 29, -2 ** 29)]])]), (5, 7))
    assert (ok == 1).all()                                            # the limit itself burns, without overflow
    guards.checks.clear()


# ------------------------------------------------------------------------------------------------------------ files

@pytest.mark.parametrize("class_zero", [False, True])
def test_geojson_written_from_a_mask_burns_back_to_the_mask(tmp_path, class_zero):
    RZ, VZ = _rz(), _vz()
    m = RC.mask(67, 93, seed=8)
    polys = VZ.polygonize(torch.from_numpy(m).cuda())
    path = tmp_path / "m.geojson"
    n = VZ.write_geojson(path, polys, GT, class_zero=class_zero)
    assert n == polys.n_polygons - (int((polys.poly_class == 0).sum()) if class_zero else 0)
    got = RZ.rasterize_geojson(path, m.shape, GT, class_zero=class_zero, fill=0 if class_zero else 9)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), m)


def test_split_raster_cuts_the_same_tiles_from_a_tiff_mask_and_from_its_geojson(tmp_path):
    import create_tiles_unet as T
    from unet_amd.tiffio import write_tiff
    VZ = _vz()
    rng = np.random.default_rng(12)
    img = rng.integers(1, 250, (3, 96, 96)).astype(np.uint8)
    m = RC.mask(96, 96, seed=13, classes=4) + np.uint8(1)             # no class 0, no nodata: both paths see the same array
    write_tiff(tmp_path / "scene.tif", img, geotransform=GT)
    write_tiff(tmp_path / "labels.tif", m, geotransform=GT)
    VZ.write_geojson(tmp_path / "labels.geojson", VZ.polygonize(torch.from_numpy(m).cuda()), GT)
    counts = {}
    for kind in ("tif", "geojson"):
        counts[kind] = T.split_raster(tmp_path / "scene.tif", tmp_path / f"labels.{kind}", tmp_path / kind, patch_size=32, patch_overlap=0.2,
                                      split=[0.7, 0.2, 0.1], seed=4)
    assert counts["tif"] == counts["geojson"] and sum(counts["tif"].values()) == 16
    files = {kind: sorted(str(p.relative_to(tmp_path / kind)) for p in (tmp_path / kind).rglob("*.tif")) for kind in counts}
    assert files["tif"] == files["geojson"] and len(files["tif"]) == 32
    for f in files["tif"]:
        assert (tmp_path / "tif" / f).read_bytes() == (tmp_path / "geojson" / f).read_bytes(), f
