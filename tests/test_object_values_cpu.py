"""CPU suite of the float statistics per object (unet_amd/objects.py): the sequential restatement of the rules against its
vectorised form on the patterns of the GPU suite, object_value_rows against exact fractions, the rows joined by object_rows, the C ABI, the
planner's rules and the refusals of both entry points before a model is loaded, params_and_main, the checks of the value raster, and the
ValueErrors that need no device."""
import dataclasses
import inspect
import json
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import object_values_ref as VR  # noqa: E402
import objects_cases as OC  # noqa: E402
import objects_ref as OR  # noqa: E402
from test_object_values_gpu import SHAPES, object_patterns, value_patterns  # noqa: E402  (plain NumPy)

GT = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)


def _ob():
    from unet_amd import objects
    return objects


def _ex(exclude):
    return () if exclude is None else ((exclude,) if isinstance(exclude, int) else tuple(exclude))


def _equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if k in ("min", "max"):
            assert a[k].dtype == np.float32 and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)
        else:
            assert a[k] == b[k], (what, k)


def _stats(t: dict):
    """the ObjectValues (host tensors) that holds a reference table"""
    OB = _ob()
    i64 = lambda k: torch.tensor(t[k], dtype=torch.int64)  # noqa: E731
    i32 = lambda k: torch.tensor(t[k], dtype=torch.int32)  # noqa: E731
    return OB.ObjectValues(i32("label"), i64("valid"), i64("sum_q"), i64("sq_lo"), i64("sq_hi"), torch.from_numpy(t["min"].copy()),
                           torch.from_numpy(t["max"].copy()), i32("argmin"), i32("argmax"), t["shift"], t["shape"])


# ------------------------------------------------------------------------------------------------------------ the two references

@pytest.mark.parametrize("shape", SHAPES)
def test_the_sequential_reference_equals_its_vectorised_form(shape):
    H, W = shape
    values = value_patterns(H, W, seed=H * 1000 + W)
    n = 0
    for oname, (m, lab, ex) in object_patterns(H, W, seed=W).items():
        for vname, (v, nodata, shift) in values.items():
            a, b = VR.tables(m, lab, v, _ex(ex), nodata, shift), VR.tables_fast(m, lab, v, _ex(ex), nodata, shift)
            _equal(a, b, (shape, oname, vname))
            assert a["label"] == OR.table(m, lab, ex)["label"].tolist() and not a["bad"]          # the objects of measure_objects
            n += 1
    assert n == 11 * 11


def test_the_references_agree_on_bad_labels_and_overflow():
    m, lab = OC.patterns(33, 300, seed=5)["blocks"]
    v = value_patterns(33, 300, seed=5)["mixed"][0]
    n = m.size
    for plane, at, value, bit in (("lab", n // 2, n, 1), ("lab", 0, -5, 1), ("lab", n - 1, 1, 2), ("lab", 3, 2 * 300 + 3, 2), ("m", 1, 9, 4)):
        mm, ll = m.copy(), lab.copy()
        (ll if plane == "lab" else mm).reshape(-1)[at] = value
        a, b = VR.tables(mm, ll, v, shift=20), VR.tables_fast(mm, ll, v, shift=20)
        _equal(a, b, (plane, at))
        assert a["bad"] & bit
    a, b = VR.tables(m, lab, v, shift=28), VR.tables_fast(m, lab, v, shift=28)
    _equal(a, b, "overflow")
    assert a["overflow"] and sum(a["valid"]) < n


def test_the_reference_on_a_case_worked_by_hand():
    m = np.array([[1, 1, 0, 2], [1, 0, 0, 2]], dtype=np.uint8)
    lab = np.array([[0, 0, 2, 3], [0, 2, 2, 3]], dtype=np.int32)
    v = np.array([[1.5, -2.0, 9.0, 0.5], [1.5, 9.0, 9.0, np.nan]], dtype=np.float32)
    t = VR.tables(m, lab, v, exclude=(0,))
    assert t["label"] == [0, 3] and t["shift"] == 30 - 2 and t["valid"] == [3, 1]          # A = 2.0 = 0.5 * 2^2; the 9.0 lie in the excluded class
    assert t["sum_q"] == [2 ** 28, 2 ** 27] and t["argmax"] == [0, 3] and t["argmin"] == [1, 3]          # 1.5 twice: the first has the maximum
    assert t["max"].tolist() == [1.5, 0.5] and t["min"].tolist() == [-2.0, 0.5]
    q2 = (3 * 2 ** 27) ** 2 * 2 + (2 ** 29) ** 2
    assert t["sq_hi"][0] * 2 ** 30 + t["sq_lo"][0] == q2
    t = VR.tables(m, lab, v, exclude=(0, 2), nodata=-2.0)
    assert t["label"] == [0] and t["valid"] == [2] and t["argmin"] == [0] and t["shift"] == 30 - 1
    t = VR.tables(m, lab, np.full((2, 4), np.inf, dtype=np.float32))
    assert t["valid"] == [0, 0, 0] and t["argmax"] == [-1] * 3 and np.isposinf(t["min"]).all() and np.isneginf(t["max"]).all() and t["shift"] == 30


# ------------------------------------------------------------------------------------------------------------ rows

def test_object_value_rows_equal_exact_arithmetic_on_the_integers():
    OB = _ob()
    H, W = 33, 300
    m, lab, ex = object_patterns(H, W, seed=2)["noise_excluded"]
    v = (np.random.default_rng(3).standard_normal((H, W)) * 6.0 + 17.0).astype(np.float32)
    v[m == 2] = np.nan                                          # the objects of class 2 have no valid pixel
    v[5, 7] = -9999.0
    t = VR.tables_fast(m, lab, v, _ex(ex), nodata=-9999)
    rows = OB.object_value_rows(_stats(t), GT, "height")
    assert rows == VR.rows(t, GT, "height") and len(rows) == len(t["label"]) > 20
    keys = ["height_" + k for k in ("valid", "mean", "std", "sum", "min", "max", "peak_x", "peak_y")]
    s = t["shift"]
    E = 30 - s
    assert E == math.frexp(float(np.abs(v[np.isfinite(v) & (v != -9999.0) & (m != 1)]).max()))[1]
    seen_none = seen = 0
    for k, row in enumerate(rows):
        assert list(row) == keys
        L = t["label"][k]
        if m.ravel()[L] == 2:
            assert set(row.values()) == {None} and t["valid"][k] == 0
            seen_none += 1
            continue
        seen += 1
        n = t["valid"][k]
        mean = Fraction(t["sum_q"][k], n) / Fraction(2) ** s
        var = (Fraction((t["sq_hi"][k] << 30) + t["sq_lo"][k], n) - Fraction(t["sum_q"][k], n) ** 2) / Fraction(4) ** s
        assert row["height_valid"] == n and abs(Fraction(row["height_mean"]) - mean) <= abs(mean) * Fraction(1, 2 ** 50)
        assert abs(row["height_std"] - math.sqrt(var)) <= 1e-9 * max(1.0, math.sqrt(var))
        assert Fraction(row["height_sum"]) == Fraction(t["sum_q"][k]) / Fraction(2) ** s          # exact: the sum fits a double here
        # the bound derived in DESIGN 3.25: the mean lies within 2^(E - 31) of the float64 mean of the raw floats, plus float64 rounding
        own = (lab == L) & np.isfinite(v) & (v != -9999.0)
        assert own.sum() == n
        assert abs(row["height_mean"] - v[own].astype(np.float64).mean()) <= 2.0 ** (E - 31) + 8 * np.spacing(2.0 ** E)
        assert row["height_min"] == float(v[own].min()) and row["height_max"] == float(v[own].max())
        # the peak: the first pixel that attains the maximum, its centre in map units under a negative gt[5]
        p = int(np.flatnonzero(own.ravel() & (v.ravel() == v[own].max()))[0])
        assert t["argmax"][k] == p
        assert row["height_peak_x"] == GT[0] + (p % W + 0.5) * GT[1] and row["height_peak_y"] == GT[3] + (p // W + 0.5) * GT[5]
        assert row["height_peak_y"] < GT[3]
    assert seen_none > 3 and seen > 10
    # without a geotransform the units are pixels
    plain = OB.object_value_rows(_stats(t))
    k = next(i for i, r in enumerate(plain) if r["value_valid"])
    assert plain[k]["value_peak_x"] == t["argmax"][k] % W + 0.5 and plain[k]["value_peak_y"] == t["argmax"][k] // W + 0.5
    with pytest.raises(ValueError, match="name must be"):
        OB.object_value_rows(_stats(t), GT, "")


def test_object_rows_append_the_value_keys_after_instance(tmp_path):
    OB = _ob()
    m = OC.noise_mask(20, 31, 2)
    lab = OC.R.label_components(m, 4)
    t = OR.table(m, lab, 0)
    P = len(t["label"])
    v = np.random.default_rng(1).random((20, 31)).astype(np.float32)
    v[m == 3] = np.nan
    h, c = _stats(VR.tables(m, lab, v * 30, (0,))), _stats(VR.tables(m, lab, v, (0,)))
    base = ["class", "name", "pixels", "area", "perimeter", "centroid_x", "centroid_y", "bbox", "diameter", "compactness", "point_x", "point_y",
            "on_edge", "instance"]
    kw = dict(geotransform=GT, codes=list("abcde"), instance=np.arange(P))
    plain = OB.object_rows(t, **kw)
    assert [list(r) for r in plain] == [base] * P and OB.object_rows(t, **kw, values=None) == plain == OB.object_rows(t, **kw, values={})
    rows = OB.object_rows(t, **kw, values={"height": h, "confidence": c})
    added = [f"{n}_{k}" for n in ("height", "confidence") for k in ("valid", "mean", "std", "sum", "min", "max", "peak_x", "peak_y")]
    assert [list(r) for r in rows] == [base + added] * P
    hr, cr = OB.object_value_rows(h, GT, "height"), OB.object_value_rows(c, GT, "confidence")
    for row, p, a, b in zip(rows, plain, hr, cr):
        assert row == {**p, **a, **b}
    assert any(r["height_mean"] is None for r in rows) and any(r["height_mean"] is not None for r in rows)
    # a table of other objects is refused
    other = _stats(VR.tables(m, lab, v, (1,)))
    with pytest.raises(ValueError, match="not a table of the same objects"):
        OB.object_rows(t, **kw, values={"height": other})
    with pytest.raises(ValueError, match="not a table of the same objects"):
        OB.object_rows(t, **kw, values={"height": dataclasses.replace(h, shape=(31, 20))})
    # both writers carry the columns; None is null in GeoJSON and an empty field in the CSV
    assert OB.write_objects(tmp_path / "o.geojson", t, GT, 25832, list("abcde"), values={"height": h}) == P
    feats = json.load(open(tmp_path / "o.geojson"))["features"]
    assert [f["properties"] for f in feats] == OB.object_rows(t, GT, list("abcde"), values={"height": h})
    OB.write_objects(tmp_path / "o.csv", t, GT, values={"height": h})
    import csv
    with open(tmp_path / "o.csv", newline="") as f:
        table = list(csv.reader(f))
    assert table[0][-8:] == added[:8] and len(table) == 1 + P
    for line, row in zip(table[1:], OB.object_rows(t, GT, values={"height": h})):
        assert line[-8:] == ["" if row[k] is None else repr(row[k]) if isinstance(row[k], float) else str(row[k]) for k in added[:8]]
    # without values the files are what they were
    OB.write_objects(tmp_path / "p.geojson", t, GT, 25832, list("abcde"))
    OB.write_objects(tmp_path / "q.geojson", t, GT, 25832, list("abcde"), values=None)
    assert (tmp_path / "p.geojson").read_bytes() == (tmp_path / "q.geojson").read_bytes()


# ------------------------------------------------------------------------------------------------------------ the library

def test_the_header_declares_the_symbols_and_the_library_exports_them():
    import ctypes as C
    from unet_amd import _abi, _lib
    names = ("unet_obj_absmax", "unet_obj_values")
    assert set(names) <= set(_lib.declared_symbols()) and set(names) <= {d.name for d in _abi.declarations(_lib.HEADER)}
    for n in names:
        assert hasattr(_lib.lib, n) and n in _lib._sig
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    assert _lib._sig["unet_obj_absmax"] == (i, [vp, vp, i, i, vp, i, C.c_float, vp, vp])
    assert _lib._sig["unet_obj_values"] == (i, [vp, vp, vp, vp, i, i, vp, ll, i, C.c_float, i, vp, vp, vp])
    assert _abi.constants(_lib.HEADER)["UNET_ABI_VERSION"] == 8 == _lib.lib.unet_abi_version()          # additions only


def test_argument_and_limit_errors_need_no_device():
    OB = _ob()
    m, lab, v = np.zeros((4, 6), dtype=np.uint8), np.zeros((4, 6), dtype=np.int32), np.zeros((4, 6), dtype=np.float32)
    for bad in (None, m.astype(np.int32), m[0], [[0]], torch.zeros(4, 6)):
        with pytest.raises(ValueError, match="mask must be"):
            OB.object_values(bad, v)
    for bad in (None, v.astype(np.float64), v[0], m, torch.zeros(4, 6, dtype=torch.float64)):
        with pytest.raises(ValueError, match="values must be"):
            OB.object_values(m, bad)
    for bad in (lab.astype(np.int64), lab[0], "labels"):
        with pytest.raises(ValueError, match="labels must be"):
            OB.object_values(m, v, bad)
    with pytest.raises(ValueError, match="labels has shape"):
        OB.object_values(m, v, lab[:3])
    with pytest.raises(ValueError, match="values has shape"):
        OB.object_values(m, v[:, :5], lab)
    for bad in (-1, 256, 1.5, "a", [0, 300]):
        with pytest.raises(ValueError, match="exclude"):
            OB.object_values(m, v, lab, bad)
    for bad in ("x", float("nan"), True, [1]):
        with pytest.raises(ValueError, match="nodata must be None or a number"):
            OB.object_values(m, v, lab, nodata=bad)
    for bad in (179, -99, 1.0, True):
        with pytest.raises(ValueError, match="shift must be an int in -98..178"):
            OB.object_values(m, v, lab, shift=bad)
    for shape, text in (((2 ** 20, 4), "2\\^20 - 1"), ((2 ** 16, 2 ** 15), "2\\^31 - 1 pixels")):
        big = np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.uint8), shape=shape, strides=(0, 0))
        with pytest.raises(ValueError, match=text):          # from the shape alone, before anything is uploaded
            OB.object_values(big, np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.float32), shape=shape, strides=(0, 0)))
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="no device"):
            OB.object_values(m, v, lab)                                  # no host fallback
        with pytest.raises(ValueError, match="no device"):
            OB.object_values(m, v)
    doc = " ".join(OB.__doc__.lower().split())
    for word in ("key(v) << 32 | (0xffffffff - p)", "smallest linear index that attains it", "median and percentiles", "float64 planes",
                 "resampling a value raster", "the peak as the feature's geometry", "argmin = argmax = -1"):
        assert word in doc, word
    assert "statistics of float planes per object, the pole" not in doc          # no longer out of scope
    assert [f.name for f in dataclasses.fields(OB.ObjectValues)] == ["label", "valid", "sum_q", "sq_lo", "sq_hi", "min", "max", "argmin", "argmax",
                                                                     "shift", "shape"]
    assert [f.name for f in dataclasses.fields(OB.ObjectTable)][-1] == "shape" and len(OB._TABLE_ARRAYS) == 9          # as they were
    assert list(inspect.signature(OB.object_values).parameters) == ["mask", "values", "labels", "exclude", "nodata", "shift", "stages"]


# ------------------------------------------------------------------------------------------------------------ the planner

def test_check_outputs_rules_for_the_new_arguments():
    import predict as P
    base = P.check_outputs()
    assert base.objects_values is None and base.objects_confidence is False
    params = inspect.signature(P.check_outputs).parameters
    names = list(params)
    at = names.index("zonal_values")
    assert names[at + 1:at + 4] == ["objects_values", "objects_values_name", "objects_confidence"]          # directly after zonal_values
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names[at:])
    assert names[-4:] == ["objects", "objects_exclude", "zones", "zonal_objects"]
    fields = [f.name for f in dataclasses.fields(P.OutputPlan)]
    assert fields[-1] == "objects" and {"objects_values", "objects_confidence"} <= set(fields[:-1])
    plan = P.check_outputs(objects="o.geojson", objects_values="chm.tif", objects_values_name="height", objects_confidence=True)
    assert plan.objects_values == "height" and plan.objects_confidence is True and plan.objects == () and plan.keep
    assert P.check_outputs(objects=True, objects_values="chm.tif").objects_values == "value"
    assert P.check_outputs(objects=True, objects_values_name="height").objects_values is None          # a name alone asks for nothing
    # the defaults change no plan
    for kw in (dict(), dict(objects="o.csv"), dict(vector="v.geojson", objects=True, class_zero=True), dict(regression=True), dict(large_file=True)):
        a = P.check_outputs(**kw)
        b = P.check_outputs(**kw, objects_values=None, objects_values_name="value", objects_confidence=False)
        assert a == b and a.objects_values is None and not a.objects_confidence, kw
    for kw, text in ((dict(objects_values="chm.tif"), "objects_values without an objects output"),
                     (dict(objects_confidence=True), "objects_confidence without an objects output"),
                     (dict(objects_values="chm.tif", objects=False), "objects_values without an objects output"),
                     (dict(objects_values="chm.tif", vector="v.geojson"), "objects_values without an objects output"),
                     (dict(objects=True, objects_values=3), "objects_values must be None or the path"),
                     (dict(objects=True, objects_values="chm.tif", objects_values_name=""), "objects_values_name must be a non-empty string"),
                     (dict(objects=True, objects_values="chm.tif", objects_values_name=7), "objects_values_name must be a non-empty string"),
                     (dict(objects=True, objects_values="chm.tif", objects_values_name="confidence", objects_confidence=True), "is taken by"),
                     (dict(objects=True, objects_confidence=True, regression=True), "object attributes needs the class mask"),
                     (dict(objects=True, objects_confidence=True, large_file=True), "not with large_file"),
                     (dict(objects=True, objects_values="chm.tif", merge=False), "object attributes needs merge=True")):
        with pytest.raises(ValueError, match=text):
            P.check_outputs(**kw)
    with pytest.raises(TypeError):
        P.check_outputs(False, False, None, False, True, False, "mean", None, None, 1, None, None, None, None, None, None, False, True, True,
                        "instances_raster", False, "chm.tif")          # nothing behind raster_arg is positional


def test_entry_points_take_the_arguments_and_refuse_before_the_model_is_loaded(tmp_path):
    import predict as P
    sig = inspect.signature(P.predict_raster).parameters
    assert sig["objects_values_path"].default is None and sig["objects_values_name"].default == "value" and sig["objects_confidence"].default is False
    sig = inspect.signature(P.save_predictions).parameters
    assert sig["objects_values"].default is None and sig["objects_values_name"].default == "value" and sig["objects_confidence"].default is False
    with pytest.raises(ValueError, match="objects_values without an objects output"):
        P.predict_raster(None, None, objects_values_path="chm.tif")
    with pytest.raises(ValueError, match="objects_confidence without an objects output"):
        P.predict_raster(None, None, objects_confidence=True, vector_path="v.geojson")
    with pytest.raises(ValueError, match="object attributes needs the class mask"):
        P.predict_raster(None, None, objects_path="o.geojson", objects_confidence=True, specific_class=1)
    with pytest.raises(ValueError, match="objects_values_name must be"):
        P.predict_raster(None, None, objects_path="o.geojson", objects_values_path="chm.tif", objects_values_name=None)
    with pytest.raises(ValueError, match="objects_values without an objects output"):
        P.save_predictions(tmp_path / "no_model.pkl", tmp_path, False, merge=True, objects_values=tmp_path / "chm.tif")
    with pytest.raises(ValueError, match="objects_confidence without an objects output"):
        P.save_predictions(tmp_path / "no_model.pkl", tmp_path, False, merge=True, objects_confidence=True)
    with pytest.raises(ValueError, match="object attributes needs merge=True"):
        P.save_predictions(tmp_path / "no_model.pkl", tmp_path, False, merge=False, objects=True, objects_confidence=True)


def test_params_and_main_passes_the_settings(monkeypatch):
    import params_and_main as M
    import predict
    assert M.OBJECTS_VALUES is None and M.OBJECTS_VALUES_NAME == "value" and M.OBJECTS_CONFIDENCE is False
    calls = {}
    monkeypatch.setattr(predict, "save_predictions", lambda *a, **kw: calls.update(kw))
    monkeypatch.setattr(M, "Create_tiles", False); monkeypatch.setattr(M, "Train", False); monkeypatch.setattr(M, "Predict", True)
    monkeypatch.setattr(M, "enable_extra_parameters", True)
    M.main()
    assert not {"objects_values", "objects_values_name", "objects_confidence"} & set(calls)          # the defaults pass nothing new
    monkeypatch.setattr(M, "OBJECTS", True); monkeypatch.setattr(M, "OBJECTS_VALUES", "chm.tif"); monkeypatch.setattr(M, "OBJECTS_VALUES_NAME", "height")
    monkeypatch.setattr(M, "OBJECTS_CONFIDENCE", True)
    M.main()
    assert calls["objects"] is True and calls["objects_values"] == "chm.tif" and calls["objects_values_name"] == "height"
    assert calls["objects_confidence"] is True
    calls.clear()
    monkeypatch.setattr(M, "enable_extra_parameters", False)                  # the non-expert branch resets them
    M.main()
    assert not {"objects", "objects_values", "objects_confidence"} & set(calls)
    assert M.OBJECTS_VALUES is None and M.OBJECTS_VALUES_NAME == "value" and M.OBJECTS_CONFIDENCE is False


# ------------------------------------------------------------------------------------------------------------ the value raster

def _write_float64_tiff(path, a: np.ndarray, gt):
    """a one-strip little-endian GeoTIFF of float64 samples (the project's writer stores floats as float32)"""
    import struct
    H, W = a.shape
    data = np.ascontiguousarray(a, dtype="<f8").tobytes()
    scale, tie = struct.pack("<3d", gt[1], -gt[5], 0.0), struct.pack("<6d", 0.0, 0.0, 0.0, gt[0], gt[3], 0.0)
    entries = [(256, 3, 1, W), (257, 3, 1, H), (258, 3, 1, 64), (259, 3, 1, 1), (262, 3, 1, 1), (273, 4, 1, 8), (277, 3, 1, 1), (278, 3, 1, H),
               (279, 4, 1, len(data)), (339, 3, 1, 3)]
    ifd_at = 8 + len(data)
    extra_at = ifd_at + 2 + 12 * (len(entries) + 2) + 4
    entries += [(33550, 12, 3, extra_at), (33922, 12, 6, extra_at + len(scale))]
    body = struct.pack("<H", len(entries)) + b"".join(struct.pack("<HHII", *e) for e in entries) + struct.pack("<I", 0)
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HI", 42, ifd_at) + data + body + scale + tie)


def test_the_value_raster_must_lie_on_the_output_grid(tmp_path):
    from unet_amd.tiffio import write_tiff
    OB = _ob()
    rng = np.random.default_rng(0)
    v = (rng.random((20, 31)) * 30).astype(np.float32)
    write_tiff(tmp_path / "chm.tif", v, geotransform=GT, nodata=-9999)
    a, nodata = OB.read_value_raster(tmp_path / "chm.tif", (20, 31), GT)
    assert a.dtype == np.float32 and a.flags.c_contiguous and np.array_equal(a.view(np.uint32), v.view(np.uint32)) and nodata == -9999
    assert OB.read_value_raster(tmp_path / "chm.tif", (20, 31), list(GT))[1] == -9999
    assert OB.read_value_raster(tmp_path / "chm.tif", (20, 31), None)[0].shape == (20, 31)          # an output without a georeference: the shape alone
    for dtype in (np.uint8, np.uint16, np.int16):               # converted exactly
        ints = rng.integers(np.iinfo(dtype).min, np.iinfo(dtype).max, (20, 31), endpoint=True).astype(dtype)
        write_tiff(tmp_path / "i.tif", ints, geotransform=GT)
        a, nodata = OB.read_value_raster(tmp_path / "i.tif", (20, 31), GT)
        assert a.dtype == np.float32 and np.array_equal(a.astype(np.int64), ints.astype(np.int64)) and nodata is None
    with pytest.raises(ValueError, match=r"20 x 31 px.*the output 20 x 30 px.*no resampling"):
        OB.read_value_raster(tmp_path / "chm.tif", (20, 30), GT)
    shifted = (GT[0] + 0.5, *GT[1:])
    with pytest.raises(ValueError, match=r"400000\.0.*400000\.5.*no resampling"):
        OB.read_value_raster(tmp_path / "chm.tif", (20, 31), shifted)
    with pytest.raises(ValueError, match="no resampling"):
        OB.read_value_raster(tmp_path / "chm.tif", (20, 31), (GT[0], 1.0, 0.0, GT[3], 0.0, -1.0))
    write_tiff(tmp_path / "plain.tif", v)                       # no georeference where the output has one
    with pytest.raises(ValueError, match="geotransform None"):
        OB.read_value_raster(tmp_path / "plain.tif", (20, 31), GT)
    write_tiff(tmp_path / "two.tif", np.stack([v, v]), geotransform=GT)
    with pytest.raises(ValueError, match="must have one band, got 2"):
        OB.read_value_raster(tmp_path / "two.tif", (20, 31), GT)
    for dtype in (np.int32, np.uint32):
        write_tiff(tmp_path / "d.tif", v.astype(dtype), geotransform=GT)
        with pytest.raises(ValueError, match=f"holds {np.dtype(dtype).name} samples"):
            OB.read_value_raster(tmp_path / "d.tif", (20, 31), GT)
    from unet_amd.tiffio import read_tiff
    _write_float64_tiff(tmp_path / "f64.tif", v.astype(np.float64), GT)
    back, meta = read_tiff(tmp_path / "f64.tif")
    assert back.dtype == np.float64 and np.array_equal(back, v.astype(np.float64)) and tuple(meta["geotransform"]) == GT
    with pytest.raises(ValueError, match="holds float64 samples"):
        OB.read_value_raster(tmp_path / "f64.tif", (20, 31), GT)
