"""CPU suite of the zonal statistics of float planes (unet_amd/zonal.py, csrc/zonal_values.hip): the reference against float64
statistics within the derived fixed-point bound, the rows and both file formats, every argument error of the two new ops and of
zonal_values -- raised with no GPU present --, the C ABI, and the planner's rules for zonal_values=.  The two tests of the reference
(test_reference_*, five cases) exercise tests/zonal_values_ref.py alone and so do not depend on the feature; every other test here needs it."""
import csv
import inspect
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import output_check_cases as OC  # noqa: E402
import zonal_values_ref as VR  # noqa: E402

NEW_SYMBOLS = ("unet_zonal_absmax", "unet_zonal_values")


def _zn():
    from unet_amd import zonal
    return zonal


# ------------------------------------------------------------------------------------------------------------ the reference

def _planes(scale, seed, H=37, W=53, Z=6):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    z = ((yy // 13) * 2 + xx // 27).astype(np.int32)
    z[rng.random((H, W)) < 0.1] = -1
    v = rng.random((H, W)).astype(np.float32) if scale == "prob" else (rng.standard_normal((H, W)) * scale).astype(np.float32)
    return z, v, Z


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e6, "prob"])
def test_reference_lies_within_the_fixed_point_bound_of_float64_statistics(scale):
    z, v, Z = _planes(scale, seed=3)
    if scale == "prob":
        v[0, 0], v[0, 1] = 0.0, 1.0
    t = VR.tables(z, v, Z)
    fast = VR.tables_fast(z, v, Z)
    assert all(np.array_equal(np.asarray(t[k]), np.asarray(fast[k])) for k in t), "the two forms of the reference"
    A = float(np.abs(v[z >= 0]).max())
    E = math.frexp(A)[1]
    assert t["shift"] == 30 - E and 2.0 ** (E - 1) <= A < 2.0 ** E
    # every q is the NumPy expression of the rules, |q| <= 2^30 and within 2^(E - 31) of the value
    q = np.rint(np.ldexp(v.astype(np.float64), t["shift"])).astype(np.int64)
    assert np.abs(q[z >= 0]).max() <= 2 ** 30
    assert np.abs(np.ldexp(q.astype(np.float64), -t["shift"]) - v.astype(np.float64)).max() <= 2.0 ** (E - 31)
    rows = VR.rows(t)
    bound = 2.0 ** (E - 31)
    ulp = np.spacing(A)                                        # float64 rounding of sums of |v| <= A: a few ulps of A
    for zone, row in enumerate(rows):
        x = v[z == zone].astype(np.float64)
        assert row["pixels"] == row["valid"] == x.size > 0
        few = math.ceil(math.log2(x.size)) + 4                 # pairwise float64 summation of n terms <= A: log2 n roundings of <= ulp(n A)
        assert abs(row["mean"] - x.mean()) <= bound + few * ulp, (zone, row["mean"], x.mean())
        assert abs(row["sum"] - x.sum()) <= x.size * (bound + few * ulp)
        # |std_q - std| <= the rms of the per-pixel errors <= bound (the triangle inequality in l2)
        assert abs(row["std"] - x.std()) <= bound + 64 * ulp
        assert row["min"] == float(x.min()) and row["max"] == float(x.max())
        mine = q[z == zone].tolist()                           # Python integers: an int64 sum of squares of 2^60 each would wrap
        assert t["sum_q"][zone] == sum(mine) and (t["sq_hi"][zone] << 30) + t["sq_lo"][zone] == sum(a * a for a in mine)


def test_reference_on_a_hand_made_case():
    z = np.array([[0, 0, 1, -1], [1, 1, 2, 2]], dtype=np.int32)
    v = np.array([[0.5, 1.5, np.nan, 7.0], [-9999.0, 2.5, np.inf, -np.inf]], dtype=np.float32)
    t = VR.tables(z, v, 4, nodata=-9999, shift=0)
    assert t["pixels"] == [2, 3, 2, 0] and t["valid"] == [2, 1, 0, 0]
    assert t["sum_q"] == [2, 2, 0, 0]                           # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2: half to even
    assert t["sq_lo"] == [4, 4, 0, 0] and t["sq_hi"] == [0, 0, 0, 0] and not t["bad_zone"] and not t["overflow"]
    assert t["min"].tolist() == [0.5, 2.5, np.inf, np.inf] and t["max"].tolist() == [1.5, 2.5, -np.inf, -np.inf]
    rows = VR.rows(t, 0.25)
    assert rows[0] == {"pixels": 2, "area": 0.5, "valid": 2, "mean": 1.0, "std": 1.0, "min": 0.5, "max": 1.5, "sum": 2.0}
    assert rows[2] == {"pixels": 2, "area": 0.5, "valid": 0, "mean": None, "std": None, "min": None, "max": None, "sum": None}
    t = VR.tables(z, v, 4)                                      # nodata=None: -9999 is a value, A = 9999, E = 14
    assert t["shift"] == 16 and t["valid"] == [2, 2, 0, 0] and t["min"][1] == -9999.0
    assert VR.tables(z, v, 4, shift=28)["overflow"] and VR.tables(np.array([[4]], dtype=np.int32), v[:1, :1], 4)["bad_zone"]
    assert VR.tables(np.array([[-2]], dtype=np.int32), v[:1, :1], 4)["bad_zone"]
    zero = VR.tables(z, np.zeros_like(v), 4)
    assert zero["shift"] == 30 and zero["sum_q"] == [0, 0, 0, 0]
    m = VR.tables(np.zeros((1, 2), dtype=np.int32), np.array([[0.0, -0.0]], dtype=np.float32), 1)
    assert np.signbit(m["min"][0]) and not np.signbit(m["max"][0])          # -0.0 lies below +0.0
    for a, E in ((1.0, 1), (np.nextafter(np.float32(1.0), np.float32(0.0)), 0), (2.0 ** -140, -139)):
        assert VR.tables(np.zeros((1, 1), dtype=np.int32), np.array([[a]], dtype=np.float32), 1)["shift"] == 30 - E


# ------------------------------------------------------------------------------------------------------------ rows and files

def _stats(t):
    ZN = _zn()
    i64 = lambda k: torch.tensor(t[k], dtype=torch.int64)  # noqa: E731
    return ZN.ZonalValues(i64("pixels"), i64("valid"), i64("sum_q"), i64("sq_lo"), i64("sq_hi"), torch.from_numpy(t["min"].copy()),
                          torch.from_numpy(t["max"].copy()), t["shift"])


def test_rows_equal_the_reference_rows_and_shift_of_absmax():
    ZN = _zn()
    for scale in (1e-3, 1.0, 1e6, "prob"):
        z, v, Z = _planes(scale, seed=8, Z=7)                   # zone 6 has no pixel
        v[z == 1] = -9999.0                                     # all of zone 1 is nodata
        t = VR.tables(z, v, Z, nodata=-9999)
        rows = ZN.zonal_value_rows(_stats(t), 0.25)
        assert rows == VR.rows(t, 0.25) and list(rows[0]) == ["pixels", "area", "valid", "mean", "std", "min", "max", "sum"]
        assert rows[6]["pixels"] == 0 and rows[6]["mean"] is None and rows[1]["pixels"] > 0 and rows[1]["valid"] == 0 and rows[1]["sum"] is None
        assert ZN.shift_of_absmax(VR.absmax_bits(z, v, Z, -9999)) == t["shift"]
    assert ZN.shift_of_absmax(0) == 30 and ZN.shift_of_absmax(0x3F800000) == 29 and ZN.shift_of_absmax(0x3F7FFFFF) == 30
    assert ZN.shift_of_absmax(1) == 178 and ZN.shift_of_absmax(0x7F7FFFFF) == -98
    with pytest.raises(ValueError, match="not finite"):
        ZN.shift_of_absmax(0x7F800000)
    # a host copy of tables that are no views of one allocation
    again = _stats(t).cpu()
    assert again.table is None and torch.equal(again.sum_q, _stats(t).sum_q) and again.shift == t["shift"]
    table = torch.arange(18, dtype=torch.int64).reshape(6, 3)
    views = ZN.ZonalValues.of_table(table, 5)
    assert views.sq_hi.tolist() == [12, 13, 14] and views.min.dtype == torch.float32 and tuple(views.max.shape) == (3,)
    assert views.min.data_ptr() == table[5].data_ptr() and views.max.data_ptr() == table[5].data_ptr() + 12 and views.cpu().table is not None


_SQUARE = {"type": "Polygon", "coordinates": [[[0, 0], [0, 4], [4, 4], [4, 0], [0, 0]]]}
_CRS = {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::25832"}}


def _zones_file(path, n):
    feats = [{"type": "Feature", "properties": {"parcel": f"P-{i}", "valid": "own"} if i else {"parcel": "P-0"}, "geometry": _SQUARE} for i in range(n)]
    path.write_text(json.dumps({"type": "FeatureCollection", "crs": _CRS, "features": feats}))


def test_write_zonal_writes_the_value_rows_alone_and_beside_the_class_rows(tmp_path):
    ZN = _zn()
    z, v, Z = _planes(1.0, seed=5, Z=7)
    v[z == 1] = np.nan
    t = VR.tables(z, v, Z)
    stats, want = _stats(t), VR.rows(t, 4.0)
    _zones_file(tmp_path / "z.geojson", Z)
    _, feats = ZN.read_zones(tmp_path / "z.geojson")
    assert ZN.write_zonal(tmp_path / "v.geojson", feats, None, pixel_area=4.0, values=stats) == Z
    doc = json.loads((tmp_path / "v.geojson").read_text())
    assert doc["crs"] == _CRS and len(doc["features"]) == Z
    for f, src, row in zip(doc["features"], feats, want):
        assert f["geometry"] == src["geometry"] and f["properties"] == {**src["properties"], **row}
        assert list(f["properties"])[-len(row):] == list(row)
    assert doc["features"][1]["properties"]["mean"] is None and doc["features"][2]["properties"]["valid"] == want[2]["valid"]          # replaces the own one
    ZN.write_zonal(tmp_path / "v.csv", feats, None, pixel_area=4.0, values=stats)
    with open(tmp_path / "v.csv", newline="") as f:
        table = list(csv.reader(f))
    added = list(want[0])
    assert table[0] == ["parcel"] + added and len(table) == Z + 1
    for line, row in zip(table[1:], want):
        assert line[1:] == ["" if row[k] is None else str(row[k]) for k in added]
    # beside the class rows: the class rows first, the value rows behind them, pixels and area once
    counts = np.stack([np.bincount(z[(z >= 0) & (v > 0)], minlength=Z), np.bincount(z[(z >= 0) & ~(v > 0)], minlength=Z)], axis=1).astype(np.int64)
    cls = ZN.ZonalStats(torch.from_numpy(counts))
    ZN.write_zonal(tmp_path / "b.geojson", feats, cls, pixel_area=4.0, values=stats)
    p = json.loads((tmp_path / "b.geojson").read_text())["features"][0]["properties"]
    own = ZN.zonal_rows(cls, None, 4.0)[0]
    assert p == {"parcel": "P-0", **own, **want[0]} and list(p)[1:] == list(own) + [k for k in want[0] if k not in own]
    with pytest.raises(ValueError, match="not of the same zones"):
        ZN.write_zonal(tmp_path / "b.geojson", feats, ZN.ZonalStats(torch.from_numpy(counts + 1)), values=stats)
    with pytest.raises(ValueError, match="7 zones, the features 6"):
        ZN.write_zonal(tmp_path / "b.geojson", feats[:6], None, values=stats)
    # without values= the call writes the bytes it wrote: the class rows alone
    ZN.write_zonal(tmp_path / "c1.geojson", feats, cls, None, 4.0, False, None)
    ZN.write_zonal(tmp_path / "c2.geojson", feats, cls, pixel_area=4.0, values=None)
    rows = ZN.zonal_rows(cls, None, 4.0)
    body = ",\n".join(json.dumps({"type": "Feature", "properties": {**{k: x for k, x in f["properties"].items() if k not in r}, **r}, "geometry": f["geometry"]})
                      for f, r in zip(feats, rows))
    assert (tmp_path / "c1.geojson").read_text() == '{"type":"FeatureCollection","crs":' + json.dumps(_CRS) + ',"features":[\n' + body + "\n]}\n"
    assert (tmp_path / "c1.geojson").read_bytes() == (tmp_path / "c2.geojson").read_bytes()
    assert list(inspect.signature(ZN.write_zonal).parameters) == ["path", "features", "stats", "codes", "pixel_area", "class_zero", "crs", "values"]


# ------------------------------------------------------------------------------------------------------------ C ABI

def test_header_declares_and_library_exports_the_new_symbols():
    from unet_amd import _lib as L
    declared = L.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L.lib, s) and s in L._sig, s
    assert "#define UNET_ABI_VERSION 8" in L.HEADER.read_text() and L.lib.unet_abi_version() == 8          # additions only


def test_bad_arguments_return_minus_one_without_a_launch():
    from unet_amd import _lib as L
    lib = L.lib
    p = 4096          # a non-null, aligned address that is never dereferenced: every call below fails its host check
    side = 2 ** 20
    calls = [
        lambda: lib.unet_zonal_absmax(None, p, 4, 4, 1, 0, 0.0, p, None),
        lambda: lib.unet_zonal_absmax(p, None, 4, 4, 1, 0, 0.0, p, None),
        lambda: lib.unet_zonal_absmax(p, p, 4, 4, 1, 0, 0.0, None, None),
        lambda: lib.unet_zonal_absmax(p, p, 0, 4, 1, 0, 0.0, p, None),
        lambda: lib.unet_zonal_absmax(p, p, 4, side, 1, 0, 0.0, p, None),
        lambda: lib.unet_zonal_absmax(p, p, 65536, 32768, 1, 0, 0.0, p, None),             # 2^31 pixels
        lambda: lib.unet_zonal_absmax(p, p, 4, 4, 0, 0, 0.0, p, None),
        lambda: lib.unet_zonal_absmax(p, p, 4, 4, 2 ** 23, 0, 0.0, p, None),
        lambda: lib.unet_zonal_absmax(p, p, 4, 4, 1, 2, 0.0, p, None),
        lambda: lib.unet_zonal_values(None, p, 4, 4, 1, 0, 0.0, 0, p, p, p, None),
        lambda: lib.unet_zonal_values(p, None, 4, 4, 1, 0, 0.0, 0, p, p, p, None),
        lambda: lib.unet_zonal_values(p, p, 4, 4, 1, 0, 0.0, 0, None, p, p, None),
        lambda: lib.unet_zonal_values(p, p, 4, 4, 1, 0, 0.0, 0, p, None, p, None),
        lambda: lib.unet_zonal_values(p, p, 4, 4, 1, 0, 0.0, 0, p, p, None, None),
        lambda: lib.unet_zonal_values(p, p, 0, 4, 1, 0, 0.0, 0, p, p, p, None),
        lambda: lib.unet_zonal_values(p, p, 4, side, 1, 0, 0.0, 0, p, p, p, None),
        lambda: lib.unet_zonal_values(p, p, 65536, 32768, 1, 0, 0.0, 0, p, p, p, None),    # 2^31 pixels
        lambda: lib.unet_zonal_values(p, p, 4, 4, 0, 0, 0.0, 0, p, p, p, None),
        lambda: lib.unet_zonal_values(p, p, 4, 4, 2 ** 23, 0, 0.0, 0, p, p, p, None),
        lambda: lib.unet_zonal_values(p, p, 4, 4, 1, -1, 0.0, 0, p, p, p, None),
        lambda: lib.unet_zonal_values(p, p, 4, 4, 1, 0, 0.0, -99, p, p, p, None),
        lambda: lib.unet_zonal_values(p, p, 4, 4, 1, 0, 0.0, 179, p, p, p, None),
    ]
    for i, c in enumerate(calls):
        assert c() == -1, i
        assert lib.unet_last_error(), i


def test_hipcc_builds_the_kernels_for_gfx950_without_a_device(tmp_path):
    from unet_amd import build as B
    src = B.CSRC / "zonal_values.hip"
    assert src in B._sources()
    r = subprocess.run([B.HIPCC, *B.FLAGS, "-c", str(src), "-o", str(tmp_path / "zonal_values.o")], capture_output=True, text=True)
    assert r.returncode == 0 and (tmp_path / "zonal_values.o").stat().st_size > 0, r.stderr[-4000:]
    text = src.read_text()
    assert "asm" not in text and "2^61" in text                  # plain C++ and vector atomics; the bound of the sums is stated


# ------------------------------------------------------------------------------------------------------------ ops

def _args(H=4, W=6, Z=3):
    return dict(zones=torch.zeros((H, W), dtype=torch.int32), values=torch.zeros((H, W), dtype=torch.float32), Z=Z, nodata=None, shift=0,
                sums=torch.zeros((5, Z), dtype=torch.int64), minmax=torch.zeros((2, Z), dtype=torch.float32), bad=torch.zeros(1, dtype=torch.int64))


def _raises(text, both=True, **change):
    from unet_amd import ops
    a = _args()
    a.update(change)
    with pytest.raises(ValueError, match=text):
        ops.zonal_values(**a)
    if both:
        b = dict(zones=a["zones"], values=a["values"], Z=a["Z"], nodata=a["nodata"], absmax=torch.zeros(1, dtype=torch.int64))
        with pytest.raises(ValueError, match=text.replace("zonal_values", "zonal_absmax")):
            ops.zonal_absmax(**b)


def test_the_two_ops_refuse_every_bad_argument_before_a_launch():
    i32, i64, f32 = torch.int32, torch.int64, torch.float32
    _raises("zones must be a torch.int32", zones=torch.zeros((4, 6), dtype=i64))
    _raises("values must be a torch.float32", values=torch.zeros((4, 6), dtype=torch.float64))
    _raises("values must be a torch.float32", values=torch.zeros((4, 6), dtype=i32))
    _raises("values must be a", values=np.zeros((4, 6), dtype=np.float32))
    _raises("expected a shape", zones=np.zeros((4, 6), dtype=np.int32))
    _raises("expected a shape", zones=torch.zeros((24,), dtype=i32))
    _raises("values has shape", values=torch.zeros((6, 4), dtype=f32))
    _raises("zones must be contiguous", zones=torch.zeros((6, 4), dtype=i32).t())
    _raises("values must be contiguous", values=torch.zeros((4, 12), dtype=f32)[:, ::2])
    _raises("must be an int", Z=3.0)
    _raises("must be an int", Z=True)
    _raises("zones must lie in", Z=0)
    _raises("zones must lie in", Z=2 ** 23)
    _raises("at most 2\\^31 - 1 pixels", zones=torch.zeros((1, 1), dtype=i32).expand(65536, 32768))          # H * W = 2^31, no memory behind it
    _raises("H and W must lie in", zones=torch.zeros((0, 6), dtype=i32))
    _raises("H and W must lie in", zones=torch.zeros((1, 1), dtype=i32).expand(1, 2 ** 20))
    _raises("nodata must be None or a number", nodata="x")
    _raises("nodata must be None or a number", nodata=float("nan"))
    from unet_amd import ops
    for absmax, text in ((torch.zeros(1, dtype=i32), "absmax must be a torch.int64"), (torch.zeros(2, dtype=i64), "absmax has shape")):
        with pytest.raises(ValueError, match=text):
            ops.zonal_absmax(torch.zeros((4, 6), dtype=i32), torch.zeros((4, 6), dtype=f32), 3, None, absmax)
    _raises("sums must be a torch.int64", both=False, sums=torch.zeros((5, 3), dtype=i32))
    _raises("sums has shape", both=False, sums=torch.zeros((3, 5), dtype=i64))
    _raises("sums must be contiguous", both=False, sums=torch.zeros((3, 5), dtype=i64).t())
    _raises("minmax must be a torch.float32", both=False, minmax=torch.zeros((2, 3), dtype=i32))
    _raises("minmax has shape", both=False, minmax=torch.zeros((3, 2), dtype=f32))
    _raises("bad must be a torch.int64", both=False, bad=torch.zeros(1, dtype=i32))
    _raises("bad has shape", both=False, bad=torch.zeros(2, dtype=i64))
    for shift in (-99, 179, 1.0, True, None):
        _raises("shift must be an int in -98..178", both=False, shift=shift)
    _raises("must live on the GPU")                               # every tensor is right but on the host: the device is checked last


def test_zonal_values_refuses_limits_types_and_a_missing_device(tmp_path):
    ZN = _zn()
    z, v = np.zeros((4, 6), dtype=np.int32), np.zeros((4, 6), dtype=np.float32)
    for kw, text in ((dict(n_zones=0), "zones must lie in"), (dict(n_zones=2 ** 23), "zones must lie in"), (dict(n_zones=3.0), "must be an int"),
                     (dict(n_zones=3, shift=179), "shift must be an int"), (dict(n_zones=3, shift=-99), "shift must be an int"),
                     (dict(n_zones=3, shift=0.0), "shift must be an int"), (dict(n_zones=3, nodata="x"), "nodata must be")):
        with pytest.raises(ValueError, match=text):
            ZN.zonal_values(z, v, **kw)
    with pytest.raises(ValueError, match="values has shape"):
        ZN.zonal_values(z, v[:3], 3)
    with pytest.raises(ValueError, match="expected a shape"):
        ZN.zonal_values(z.reshape(-1), v.reshape(-1), 3)
    with pytest.raises(ValueError, match="at most 2\\^31 - 1 pixels"):
        ZN.zonal_values(torch.zeros((1, 1), dtype=torch.int32).expand(65536, 32768), torch.zeros((1, 1)).expand(65536, 32768), 3)
    with pytest.raises(ValueError, match="zonal_values: values must be a torch.float32"):
        ZN.zonal_values(z, v.astype(np.float64), 3)
    with pytest.raises(ValueError, match="zonal_values: values must be a torch.float32"):
        ZN.zonal_values(torch.from_numpy(z), torch.from_numpy(z), 3)
    with pytest.raises(ValueError, match="zonal_values: zones must be a torch.int32"):
        ZN.zonal_values(z.astype(np.int64), v, 3)
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="no device"):
            ZN.zonal_values(z, v, 3)                              # no host fallback
        (tmp_path / "z.geojson").write_text(json.dumps({"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {}, "geometry": _SQUARE}]}))
        with pytest.raises(ValueError, match="no device"):
            ZN.zonal_plane(v, tmp_path / "z.geojson", tmp_path / "out.geojson")
        assert not (tmp_path / "out.geojson").exists()
    # the messages of zonal_counts are the ones they were
    with pytest.raises(ValueError, match="zonal_counts: mask must be a torch.uint8"):
        ZN._plane(v, torch.uint8, "mask")
    assert inspect.signature(ZN._plane).parameters["what"].default == "zonal_counts"
    doc = ZN.__doc__
    for word in ("half to even", "2^61", "frexp", "2^(E-31)", "order-preserving", "percentiles", "fractional pixel coverage", "all_classes", "float64"):
        assert word in doc, word
    assert "Out of scope: statistics of float planes" not in doc


def test_zonal_plane_refuses_another_epsg_before_anything_runs(tmp_path, monkeypatch):
    ZN = _zn()
    _zones_file(tmp_path / "z.geojson", 2)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)          # the check under test comes before the first device call
    with pytest.raises(ValueError, match="EPSG:25832, the raster in EPSG:31467"):
        ZN.zonal_plane(np.zeros((8, 8), dtype=np.float32), tmp_path / "z.geojson", tmp_path / "t.geojson", None, {34735: [1, 1, 0, 1, 3072, 0, 1, 31467]})
    assert not (tmp_path / "t.geojson").exists()
    assert list(inspect.signature(ZN.zonal_plane).parameters) == ["out", "zones_path", "out_path", "geotransform", "tags", "nodata", "timing"]


# ------------------------------------------------------------------------------------------------------------ the planner

def test_check_outputs_rules_for_zonal_values():
    import predict as P
    for kw in (dict(regression=True), dict(specific_class=1)):
        plan = P.check_outputs(**kw, zones="z.geojson", zonal_values=True)
        assert plan.zones and plan.zonal_values and plan.keep and not plan.zonal_objects and not plan.mask
        assert P.check_outputs(**kw, zones="z.geojson", zonal_values=True, raster=False, return_array=False).zonal_values
    assert P.check_outputs(regression=True, zones="z.geojson", zonal_values=True).nodata == -9999
    assert P.check_outputs(specific_class=1, zones="z.geojson", zonal_values=True).nodata is None
    z = dict(zones="z.geojson", zonal_values=True)
    for kw, text in ((dict(**z), "zonal_values needs a float plane, regression or specific_class: the class mask has none \\(its table is zones without"),
                     (dict(all_classes=True, **z), "zonal_values needs one float plane: not with all_classes"),
                     (dict(regression=True, large_file=True, **z), "zonal_values needs the float plane on one device: not with large_file"),
                     (dict(specific_class=1, large_file=True, **z), "not with large_file"),
                     (dict(regression=True, merge=False, **z), "zonal_values needs merge=True: per-tile outputs are not summarised"),
                     (dict(regression=True, zonal_values=True), "zonal_values without zones"),
                     (dict(regression=True, zonal_objects=True, **z), "zonal_values with zonal_objects"),
                     (dict(regression=True, zonal_objects=True, zonal_values=True), "zonal_objects without zones")):
        with pytest.raises(ValueError, match=text):
            P.check_outputs(**kw)
    # without it: the refusals of before, word for word
    with pytest.raises(ValueError, match="zonal statistics needs the class mask: not with regression, all_classes or specific_class"):
        P.check_outputs(regression=True, zones="z.geojson")
    assert repr(P.check_outputs()).endswith(", zonal_objects=False, objects=None)") and P.check_outputs().zonal_values is False
    assert list(inspect.signature(P.check_outputs).parameters)[-4:] == ["objects", "objects_exclude", "zones", "zonal_objects"]
    assert inspect.signature(P.check_outputs).parameters["zonal_values"].default is False
    assert inspect.signature(P.check_outputs).parameters["zonal_values"].kind is inspect.Parameter.KEYWORD_ONLY          # it can shift no positional argument
    with pytest.raises(TypeError):
        P.check_outputs(*([False] * 4 + [True, False, "mean"] + [None] * 2 + [1] + [None] * 6 + [False, True, True, "instances_raster", True]))


def _kw_of_case(form, c):
    c = dict(c)
    if form == "save":
        c["vector"] = c["vector"] or None
        return c
    c["vector"], c["instances_raster"] = c.pop("vector_path"), c.pop("instances_path") is not None
    c["raster"], c["raster_arg"] = c.pop("out_path") is not None, "instances_path"
    return c


@pytest.mark.parametrize("form", ["save", "raster"])
def test_the_default_takes_the_branches_and_raises_the_messages_of_before(form):
    import predict as P

    def outcome(**kw):
        try:
            return repr(P.check_outputs(**kw))
        except ValueError as e:
            return "ValueError: " + str(e)

    n = 0
    for c in OC.cases(form):
        kw = _kw_of_case(form, c)
        for zones in ((None, "z.geojson") if n % 16 == 0 else (None,)):          # with zones on every 16th case, to keep the test quick
            assert outcome(**kw, zones=zones) == outcome(**kw, zones=zones, zonal_values=False), kw
        n += 1
    assert n == sum(1 for _ in OC.cases(form)) > 1000


def test_entry_points_take_the_argument_and_refuse_before_the_model_is_loaded(tmp_path):
    import predict as P
    assert inspect.signature(P.predict_raster).parameters["zonal_values"].default is False
    assert inspect.signature(P.save_predictions).parameters["zonal_values"].default is False
    with pytest.raises(ValueError, match="zonal_values needs a float plane"):
        P.predict_raster(None, None, zones_path="z.geojson", zonal_path="t.csv", zonal_values=True)
    with pytest.raises(ValueError, match="zonal_values without zones"):
        P.predict_raster(None, None, regression=True, zonal_values=True)
    with pytest.raises(ValueError, match="zonal_values needs merge=True"):
        P.save_predictions(tmp_path / "no_model.pkl", tmp_path, True, merge=False, zones="z.geojson", zonal_values=True)
    with pytest.raises(ValueError, match="not with all_classes"):
        P.save_predictions(tmp_path / "no_model.pkl", tmp_path, False, merge=True, all_classes=True, zones="z.geojson", zonal_values=True)


def test_params_and_main_passes_zonal_values(monkeypatch):
    import params_and_main as M
    import predict
    assert M.ZONAL_VALUES is False
    calls = {}
    monkeypatch.setattr(predict, "save_predictions", lambda *a, **kw: calls.update(kw))
    monkeypatch.setattr(M, "Create_tiles", False); monkeypatch.setattr(M, "Train", False); monkeypatch.setattr(M, "Predict", True)
    monkeypatch.setattr(M, "enable_extra_parameters", True)
    M.main()
    assert "zonal_values" not in calls                            # the default passes nothing new
    monkeypatch.setattr(M, "ZONES", "parcels.geojson"); monkeypatch.setattr(M, "ZONAL_VALUES", True)
    M.main()
    assert calls["zones"] == "parcels.geojson" and calls["zonal_values"] is True
