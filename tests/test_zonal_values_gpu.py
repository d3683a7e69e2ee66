"""GPU suite of the zonal statistics of float planes (csrc/zonal_values.hip, unet_amd/zonal.py): the tables against the
restatement of the rules in NumPy and Python integers (tests/zonal_values_ref.py) on every tail length, alignment, zone pattern and value
pattern; spans of several steps; the additivity under one shift; bad input; the two entry points.  Every comparison is exact equality, the
extremes as bit patterns and the derived shift included.  Every buffer a kernel writes sits in a guard-banded allocation and every input
between canaries (the float canary is a finite -3e7, so a read outside a plane shows in the sums and in min); all of them are checked after
every launcher, and the inputs are compared unchanged afterwards."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import zonal_cases as ZC  # noqa: E402
import zonal_ref as ZR  # noqa: E402
import zonal_values_ref as VR  # noqa: E402
from guard import canary_input, guarded  # noqa: E402

_FILL = {torch.uint8: 0xA5, torch.int32: -7, torch.int64: -7}
_LAUNCHERS = ("ras_count", "ras_scan", "ras_emit", "ras_spans", "ras_resolve", "ras_resolve_ids", "zonal_counts", "zonal_absmax", "zonal_values",
              "vec_read")
SHAPES = [(1, 1), (1, 3), (1, 4), (1, 5), (3, 15), (2, 16), (3, 17), (5, 63), (7, 257), (33, 300)]
SEQUENTIAL = 2000          # pixels up to which the sequential reference runs; beyond it its vectorised form (equal: test_zonal_values_cpu.py)
_INTS = ("pixels", "valid", "sum_q", "sq_lo", "sq_hi")


def _zn():
    from unet_amd import zonal
    return zonal


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
    from unet_amd import ops, rasterize
    g = Guards()
    monkeypatch.setattr(rasterize, "_alloc", g.alloc)
    monkeypatch.setattr(_zn(), "_alloc", g.alloc)
    for name in _LAUNCHERS:
        def wrapped(*a, _fn=getattr(ops, name), _name=name, **k):
            r = _fn(*a, **k)
            g.by_name[_name] = g.by_name.get(_name, 0) + 1
            g.check(_name)
            return r
        monkeypatch.setattr(ops, name, wrapped)
    return g


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _reference(z, v, Z, nodata=None, shift=None):
    return (VR.tables if z.size <= SEQUENTIAL else VR.tables_fast)(z, v, Z, nodata, shift)


def _same(host, want, what):
    for k in _INTS:
        assert getattr(host, k).dtype == torch.int64 and getattr(host, k).tolist() == list(want[k]), (what, k)
    assert host.min.dtype == torch.float32 and np.array_equal(_bits(host.min.numpy()), _bits(want["min"])), (what, "min")
    assert np.array_equal(_bits(host.max.numpy()), _bits(want["max"])), (what, "max")
    assert host.shift == want["shift"], (what, "shift")


def _run(guards, z, v, Z, nodata=None, shift=None, planes=None):
    """zonal_values on guarded copies (or on the given device planes); the inputs come back unchanged; returns the host tables"""
    dz, dv = planes if planes is not None else (guards.upload(z), guards.upload(v))
    before = dict(guards.by_name)
    stats = _zn().zonal_values(dz, dv, Z, nodata, shift)
    assert guards.by_name.get("zonal_absmax", 0) - before.get("zonal_absmax", 0) == (1 if shift is None else 0)
    assert guards.by_name["zonal_values"] - before.get("zonal_values", 0) == 1
    for name in _INTS + ("min", "max"):
        t = getattr(stats, name)
        assert t.is_cuda and tuple(t.shape) == (Z,), name
    assert np.array_equal(dz.cpu().numpy(), z) and np.array_equal(_bits(dv.cpu().numpy()), _bits(v))
    host = stats.cpu()
    guards.clear()
    return host


def _check(guards, z, v, Z, what, nodata=None, shift=None, planes=None):
    want = _reference(z, v, Z, nodata, shift)
    assert not want["bad_zone"] and not want["overflow"], what
    host = _run(guards, z, v, Z, nodata, shift, planes)
    _same(host, want, what)
    assert sum(want["pixels"]) == int(((z >= 0) & (z < Z)).sum())
    return host


# ------------------------------------------------------------------------------------------------------------ patterns

def zone_patterns(H, W, Z, seed):
    """{name: int32 [H, W]} over zones 0 .. Z - 1; zone Z - 1 is populated in every pattern but "none" and "hole" (where no pixel has it)"""
    rng = np.random.default_rng(seed)
    n = H * W
    flat = np.arange(n).reshape(H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    p = {"one": np.full((H, W), Z - 1), "none": np.full((H, W), -1), "columns": xx % Z}          # columns: stripes one pixel wide, every lane a head
    for w in (4, 8, 256):
        p[f"runs{w}"] = (flat // w) % Z                         # runs that start and end at lane (4, 8) and wavefront (256) boundaries
    cross = np.zeros((H, W), dtype=np.int64)                    # a run of another zone across the wavefront boundary at pixel 256, off the lane grid
    cross.reshape(-1)[min(250, n - 1):270] = Z - 1
    p["cross"] = cross
    p["blocks"] = ((yy // 3) * ((W + 4) // 5) + xx // 5 + rng.integers(0, Z)) % Z
    p["blocks"][rng.random((H, W)) < 0.2] = -1
    p["hole"] = rng.integers(0, max(Z - 1, 1), (H, W)) if Z > 1 else np.full((H, W), -1)          # zone Z - 1 has no pixel
    out = {}
    for name, z in p.items():
        z = np.ascontiguousarray(z, dtype=np.int32)
        if name not in ("none", "hole"):
            z[-1, -1] = Z - 1
        out[name] = z
    return out


def value_patterns(H, W, seed):
    """{name: (float32 [H, W], nodata, shift)}"""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    noise = lambda s: (rng.standard_normal((H, W)) * s).astype(f32)  # noqa: E731
    p = {"constant": (np.full((H, W), 0.75, dtype=f32), None, None), "zeros": (np.zeros((H, W), dtype=f32), None, None)}
    for s in (1e-3, 1.0, 1e6):
        p[f"noise{s:g}"] = (noise(s), None, None)
    prob = rng.random((H, W)).astype(f32)
    prob[rng.random((H, W)) < 0.1] = 0.0
    prob[rng.random((H, W)) < 0.1] = 1.0
    p["prob"] = (prob, None, None)
    p["negzero"] = (np.where(rng.random((H, W)) < 0.5, f32(0.0), f32(-0.0)).astype(f32), None, None)          # A = 0
    below = np.clip(noise(2.0), -7.5, 7.5)
    exact = below.copy()
    exact[H // 2, W // 2] = -8.0                                # A = 2^3 exactly: E = 4
    below[H // 2, W // 2] = np.nextafter(f32(8.0), f32(0.0))    # the float just below it: E = 3
    p["pow2"], p["below_pow2"] = (exact, None, None), (below, None, None)
    p["denormal"] = ((rng.integers(-2 ** 20, 2 ** 20, (H, W)).astype(np.int64) * 2.0 ** -149).astype(f32), None, None)
    special = noise(50.0)
    for value in (np.nan, np.inf, -np.inf, -9999.0):
        special[rng.random((H, W)) < 0.08] = value
    special.reshape(-1)[:4] = np.array([np.nan, np.inf, -np.inf, -9999.0], dtype=f32)[:H * W]          # each of them at least once
    p["special"], p["special_nodata"] = (special, None, None), (special, -9999, None)
    half = rng.choice(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5, 0.0, 7.0], dtype=f32), (H, W))
    p["half"] = (half, None, 0)                                 # round half to even under an explicit shift
    return p


@pytest.mark.parametrize("shape", SHAPES)
def test_patterns_equal_the_reference_on_every_tail(guards, shape):
    H, W = shape
    values = value_patterns(H, W, seed=H * 1000 + W)
    assert np.isnan(values["special"][0]).any() and values["denormal"][0].dtype == np.float32
    names = sorted(values)
    launches = 0
    for Z in (1, 7, 70000):
        zones = zone_patterns(H, W, Z, seed=Z + W)
        assert set(zones) == {"one", "none", "columns", "runs4", "runs8", "runs256", "cross", "blocks", "hole"}
        for i, (zname, z) in enumerate(sorted(zones.items())):
            # every zone pattern with the noise, the specials under nodata and three more value patterns in rotation: all pairs over the shapes
            # (70000 zones: the two alone, the tables are long)
            rotation = [] if Z == 70000 else [names[i % len(names)], names[(i + 5) % len(names)], names[(i + 9) % len(names)]]
            for vname in sorted({"noise1", "special_nodata", *rotation}):
                v, nodata, shift = values[vname]
                host = _check(guards, z, v, Z, (shape, Z, zname, vname), nodata, shift)
                launches += 1
                if zname == "none":
                    assert not host.pixels.any() and bool(torch.isposinf(host.min).all()) and bool(torch.isneginf(host.max).all())
                if zname == "one":
                    assert int(host.pixels[Z - 1]) == H * W
                if zname == "hole" and Z > 1:
                    assert int(host.pixels[Z - 1]) == 0 and float(host.min[Z - 1]) == np.inf and float(host.max[Z - 1]) == -np.inf
                if vname == "half" and zname == "one":
                    assert int(host.sum_q[Z - 1]) == int(np.rint(v.astype(np.float64)).sum())
    assert guards.by_name["zonal_values"] == launches


def test_shifts_of_zero_powers_of_two_and_denormals(guards):
    z = zone_patterns(7, 257, 7, seed=1)["blocks"]
    z[3, 128] = 0                                               # the pixel that holds the largest magnitude of pow2 and below_pow2 is in a zone
    values = value_patterns(7, 257, seed=2)
    want = {"zeros": 30, "negzero": 30, "pow2": 26, "below_pow2": 27, "constant": 30, "half": 0}
    for name, s in want.items():
        v, nodata, shift = values[name]
        assert _check(guards, z, v, 7, name, nodata, shift).shift == s, name
    host = _check(guards, z, values["denormal"][0], 7, "denormal")
    assert host.shift >= 30 + 126 + 3 and int(host.sq_hi.max()) > 0                       # denormals are not flushed: E <= -129
    neg = _check(guards, z, values["negzero"][0], 7, "negzero")
    has = (neg.valid > 0).numpy()
    assert np.signbit(neg.min.numpy()[has]).all() and not np.signbit(neg.max.numpy()[has]).any()          # -0.0 below +0.0
    # a zone whose pixels are all nodata, and one whose pixels are all NaN: pixels without valid
    v = values["noise1"][0].copy()
    v[z == 2], v[z == 3] = -9999.0, np.nan
    host = _check(guards, z, v, 7, "all nodata", nodata=-9999)
    for zone in (2, 3):
        assert int(host.pixels[zone]) > 0 and int(host.valid[zone]) == 0 and float(host.min[zone]) == np.inf and int(host.sq_hi[zone]) == 0
    rows = _zn().zonal_value_rows(host, 0.25)
    assert rows == VR.rows(_reference(z, v, 7, -9999), 0.25) and rows[2]["mean"] is None and rows[1]["mean"] is not None


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_planes_at_addresses_that_are_only_element_aligned(guards, offset):
    # views that start `offset` elements into guarded allocations: no 16-byte access is possible, and none may touch the bands
    # the ten tail shapes, each with another zone pattern, value pattern and number of zones
    znames = ["blocks", "runs4", "columns", "cross", "runs8", "one", "hole", "runs256", "blocks", "blocks"]
    vnames = ["special_nodata", "noise1", "prob", "special", "half", "denormal", "noise1e+06", "negzero", "special_nodata", "special_nodata"]
    for i, (H, W) in enumerate(SHAPES):
        Z = (1, 7, 2000)[i % 3] if (H, W) != (33, 300) else 2000
        z = zone_patterns(H, W, Z, seed=offset)[znames[i]]
        v, nodata, shift = value_patterns(H, W, seed=offset)[vnames[i]]
        n = H * W
        bufs = []
        for a in (z, v):
            flat = guards.upload(np.concatenate([np.full(offset, a.reshape(-1)[0], a.dtype), a.reshape(-1)]))
            bufs.append(flat[offset:offset + n].view(H, W))
        assert bufs[0].data_ptr() % 16 != 0 and bufs[1].data_ptr() % 16 != 0 and bufs[0].is_contiguous()
        _check(guards, z, v, Z, (H, W, "both unaligned"), nodata, shift, planes=(bufs[0], bufs[1]))
        _check(guards, z, v, Z, (H, W, "values unaligned"), nodata, shift, planes=(guards.upload(z), bufs[1]))
        _check(guards, z, v, Z, (H, W, "zones unaligned"), nodata, shift, planes=(bufs[0], guards.upload(v)))


@pytest.mark.parametrize("Z", [12, 3000])
def test_spans_of_several_steps_per_wavefront(guards, Z):
    # The launcher keeps the span rule of zonal.hip (at most 1024 workgroups of 4 wavefronts, a span a multiple of 128 groups of 4 pixels):
    # 3.15 M pixels are 787 k groups over 4096 wavefronts, a span of 256 groups = four steps of 256 pixels per wavefront, so the pending
    # record is carried from step to step, flushed where the zone changes inside a span and at its end -- through zones wider than a span,
    # rows that are no multiple of 4, and values that are not valid
    H, W = 1537, 2049
    rng = np.random.default_rng(Z)
    yy, xx = np.mgrid[0:H, 0:W]
    z = (((yy // 500) * 4 + xx // 600) % Z).astype(np.int32)
    z[:300] = Z - 1                                             # 600 k pixels of one zone on end
    z[1000:1003] = -1
    z[1200:1210, ::7] = 5
    v = (rng.standard_normal((H, W)) * 3.0 + 20.0).astype(np.float32)
    v[rng.random((H, W)) < 0.001] = np.nan
    v[700:720] = -9999.0
    v[100:120] = 0.125                                          # a span of one constant
    host = _check(guards, z, v, Z, "large", nodata=-9999)
    assert int(host.pixels[Z - 1]) >= 300 * W and int(host.valid[Z - 1]) < int(host.pixels[Z - 1])
    # the mean against float64 within the derived bound: E = 6 here (A in 32 .. 64), so 2^-25, plus float64 rounding
    assert host.shift == 24
    ok = (z == Z - 1) & np.isfinite(v) & (v != -9999.0)
    mean = _zn().zonal_value_rows(host)[Z - 1]["mean"]
    assert abs(mean - v[ok].astype(np.float64).mean()) <= 2.0 ** -25 + 32 * np.spacing(64.0)


def test_tables_of_one_shift_add_up_and_runs_are_equal(guards):
    H, W, Z = 34, 300, 40
    z = zone_patterns(H, W, Z, seed=4)["blocks"]
    v = value_patterns(H, W, seed=4)["special"][0]
    v[:H // 2] *= 0.01                                          # the halves would derive different shifts
    whole = _check(guards, z, v, Z, "whole", nodata=-9999)
    s = whole.shift
    top = _check(guards, z[:H // 2], v[:H // 2], Z, "top", nodata=-9999, shift=s)
    bottom = _check(guards, z[H // 2:], v[H // 2:], Z, "bottom", nodata=-9999, shift=s)
    assert _run(guards, z[:H // 2], v[:H // 2], Z, -9999).shift > s
    for k in _INTS:
        assert torch.equal(getattr(top, k) + getattr(bottom, k), getattr(whole, k)), k
    assert np.array_equal(_bits(torch.minimum(top.min, bottom.min).numpy()), _bits(whole.min.numpy()))
    assert np.array_equal(_bits(torch.maximum(top.max, bottom.max).numpy()), _bits(whole.max.numpy()))
    for _ in range(3):                                          # two runs of one input are equal
        again = _run(guards, z, v, Z, -9999)
        assert torch.equal(again.table, whole.table) and again.shift == s


# ------------------------------------------------------------------------------------------------------------ bad input

@pytest.mark.parametrize("shape", [(3, 17), (33, 300)])
@pytest.mark.parametrize("Z", [6, 70000])
def test_bad_zones_are_counted_nowhere_index_nothing_and_raise(guards, shape, Z):
    from unet_amd import ops
    H, W = shape
    z0 = zone_patterns(H, W, Z, seed=9)["blocks"]
    v = value_patterns(H, W, seed=9)["noise1"][0]
    for what, value in (("zone = Z", Z), ("zone = -2", -2), ("zone = 2^31 - 1", 2 ** 31 - 1), ("zone = -2^31", -2 ** 31)):
        z = z0.copy()
        z.reshape(-1)[[0, H * W // 2, H * W - 1]] = value       # the first pixel, the middle, the tail
        want = VR.tables(z, v, Z, shift=20)
        assert want["bad_zone"] and want["pixels"] == VR.tables(np.where((z < 0) | (z >= Z), -1, z).astype(np.int32), v, Z, shift=20)["pixels"]
        dz, dv = guards.upload(z), guards.upload(v)
        table, word = guards.alloc((6, Z), torch.int64, "cuda"), guards.alloc((1,), torch.int64, "cuda")
        ops.zonal_values(dz, dv, Z, None, 20, table[:5], table[5].view(torch.float32).view(2, Z), word)
        assert int(word.cpu()[0]) == 2, what
        _same(_zn().ZonalValues.of_table(table, 20).cpu(), want, what)          # the tables of all other pixels
        with pytest.raises(ValueError, match="outside -1"):
            _zn().zonal_values(dz, dv, Z)
        guards.clear()


def test_a_shift_too_large_for_the_data_raises(guards):
    from unet_amd import ops
    H, W, Z = 7, 257, 7
    z = zone_patterns(H, W, Z, seed=3)["blocks"]
    v = value_patterns(H, W, seed=3)["noise1"][0]
    v[3, 100] = 5.0                                              # E = 3: the derived shift is 27
    z[3, 100] = 1
    assert _check(guards, z, v, Z, "derived").shift == 27
    _check(guards, z, v, Z, "smaller", shift=20)
    dz, dv = guards.upload(z), guards.upload(v)
    with pytest.raises(ValueError, match="shift=28 is too large"):
        _zn().zonal_values(dz, dv, Z, shift=28)
    table, word = guards.alloc((6, Z), torch.int64, "cuda"), guards.alloc((1,), torch.int64, "cuda")
    ops.zonal_values(dz, dv, Z, None, 28, table[:5], table[5].view(torch.float32).view(2, Z), word)
    want = VR.tables(z, v, Z, shift=28)
    assert int(word.cpu()[0]) == 4 and want["overflow"]
    _same(_zn().ZonalValues.of_table(table, 28).cpu(), want, "overflow")          # such a pixel is left out of the sums
    # an exact power of two at |q| = 2^30 is no overflow
    v[3, 100] = 4.0
    v[np.abs(v) > 4.0] = 1.0
    assert int(_check(guards, z, v, Z, "2^30", shift=28).sq_hi[1]) >= 2 ** 30               # q^2 = 2^60 = 2^30 * 2^30 + 0
    guards.clear()


# ------------------------------------------------------------------------------------------------------------ prediction entry points

def _reference_rows(zones_path, gt, plane, nodata):
    rings, feats = _zn().read_zones(zones_path, gt)
    ids = ZR.ids(rings.xy.numpy(), rings.ring_start.numpy(), rings.feature_ring_start.numpy(), plane.shape)
    t = VR.tables(ids.astype(np.int32), plane, len(feats), nodata)
    assert not t["bad_zone"]
    return feats, VR.rows(t, abs(gt[1] * gt[5])), t


def _same_table(path, feats, rows):
    doc = json.load(open(path))
    assert len(doc["features"]) == len(feats) == len(rows)
    for f, src, row in zip(doc["features"], feats, rows):
        assert f["geometry"] == src["geometry"] and f["properties"] == {**src["properties"], **row}, src["properties"]


def test_entry_points_write_the_table_of_the_plane_they_return(tmp_path, guards):
    import create_tiles_unet as T
    import predict as P
    from test_instances_gpu import _export, _model
    from test_zonal_gpu import _zones_document
    size, gt = ZC.E2E_SIZE, ZC.E2E_GT
    rpath = ZC.e2e_scene(tmp_path)
    kw = dict(max_empty=0.9, batch_size=5)
    reg = _model("xresnet18", 4, 1, size, seed=12)
    plain = P.predict_raster(reg, rpath, size, 0.2, regression=True, **kw)
    H, W = plain.shape
    assert plain.dtype == np.float32 and np.isfinite(plain).all() and plain.std() > 0
    zpath = tmp_path / "zones.geojson"
    zpath.write_text(json.dumps(_zones_document(gt, H, W)))
    # zonal_values=False: the class table, and neither new op is launched
    cls = _model("xresnet18", 4, 3, size, seed=11)
    P.predict_raster(cls, rpath, size, 0.2, zones_path=zpath, zonal_path=tmp_path / "c.geojson", zonal_values=False, **kw)
    assert guards.by_name["zonal_counts"] == 1 and "zonal_absmax" not in guards.by_name and "zonal_values" not in guards.by_name
    assert "px_0" in json.load(open(tmp_path / "c.geojson"))["features"][0]["properties"]
    # regression: the table of the returned plane, nodata -9999
    timing = {}
    got = P.predict_raster(reg, rpath, size, 0.2, regression=True, zones_path=zpath, zonal_path=tmp_path / "r.geojson", zonal_values=True, timing=timing,
                           **kw)
    assert np.array_equal(got, plain)
    feats, rows, t = _reference_rows(zpath, gt, plain, -9999)
    _same_table(tmp_path / "r.geojson", feats, rows)
    assert [f["properties"]["parcel"] for f in feats] == ["north", "over", "edge", "far", "holed", "parts"]
    assert rows[3]["pixels"] == 0 and rows[3]["mean"] is None and rows[2]["pixels"] == 20 * 26 and rows[0]["valid"] == rows[0]["pixels"] > 0
    assert timing["zonal_seconds"] > 0 and timing["zonal_zones"] == 6 and timing["zonal_pixels"] == sum(t["pixels"]) > 0
    assert guards.by_name["zonal_absmax"] == 1 and guards.by_name["zonal_values"] == 1 and guards.by_name["zonal_counts"] == 1
    # the probability of one class, as a CSV
    prob = P.predict_raster(cls, rpath, size, 0.2, specific_class=1, **kw)
    none = P.predict_raster(cls, rpath, size, 0.2, specific_class=1, zones_path=zpath, zonal_path=tmp_path / "p.csv", zonal_values=True, return_array=False,
                            **kw)
    assert none is None and prob.dtype == np.float32 and 0.0 <= prob.min() < prob.max() <= 1.0
    feats, rows, _ = _reference_rows(zpath, gt, prob, None)
    import csv
    with open(tmp_path / "p.csv", newline="") as f:
        table = list(csv.reader(f))
    added = list(rows[0])
    assert table[0] == ["parcel", "nr"] + added
    for line, src, row in zip(table[1:], feats, rows):
        assert line == [src["properties"]["parcel"], str(src["properties"]["nr"])] + ["" if row[k] is None else str(row[k]) for k in added]
    # the tile-file entry point writes <merged raster stem>_zonal.geojson
    pkl = _export(tmp_path, reg, 1, size)
    tiles = tmp_path / "cut"
    T.split_raster(rpath, None, tiles, patch_size=size, patch_overlap=0.2, split=[1], max_empty=0.9)
    folder = P.save_predictions(pkl, tiles / "img_tiles", True, merge=True, AOI="r", validation_vision=False, batch_size=5, zones=zpath, zonal_values=True)
    from unet_amd.tiffio import read_tiff
    merged = read_tiff(folder / "r_m_prediction.tif")[0]
    assert merged.shape == plain.shape and merged.dtype == np.float32
    _same_table(folder / "r_m_prediction_zonal.geojson", *_reference_rows(zpath, gt, merged, -9999)[:2])
    guards.check("end")
