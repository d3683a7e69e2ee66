"""CPU suite of the object attributes (unet_amd/objects.py): the sequential restatement (tests/objects_ref.py) against
independent facts -- hand-computed tables, the ring lengths of the reference tracer, scipy where it is there --, the planner's rules, the
entry points' refusals before a model is loaded, params_and_main, the two writers, the unchanged bytes of write_geojson, the C ABI and the
ValueErrors that need no device."""
import csv
import dataclasses
import inspect
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import objects_cases as OC  # noqa: E402
import objects_ref as OR  # noqa: E402
import postprocess_ref as R  # noqa: E402
import vectorize_ref as VR  # noqa: E402


def _ob():
    from unet_amd import objects
    return objects


def _table(m, exclude=None, labels=None):
    lab = R.label_components(m, 4) if labels is None else labels
    assert OR.bad_bits(m, lab) == 0
    return OR.table(m, lab, exclude)


def _one(t, k=0):
    return {f: t[f][k].tolist() for f in OR.FIELDS}


# ------------------------------------------------------------------------------------------------------------ the restatement

def test_hand_computed_tables():
    # a 2 x 2 square of class 1 at (1, 1) in a 4 x 5 raster of class 0
    m = OC.placed((4, 5), np.ones((2, 2), dtype=np.uint8), (1, 1))
    t = _table(m, exclude=0)
    assert _one(t) == dict(label=6, cls=1, pixels=4, sum_x=6, sum_y=6, bbox=[1, 1, 3, 3], edges_v=4, edges_h=4, point=6) and len(t["label"]) == 1
    # with the background: 20 - 4 pixels, the frame (2 x 4 + 2 x 5) plus the square's border, centroid floor(34 / 16), floor(24 / 16) = (2, 1),
    # which is a pixel of the square; the background pixels at distance 1 are (2, 0) and (3, 1), and the smaller index wins: (2, 0)
    t = _table(m)
    assert _one(t, 0) == dict(label=0, cls=0, pixels=16, sum_x=34, sum_y=24, bbox=[0, 0, 5, 4], edges_v=8 + 4, edges_h=10 + 4, point=2)
    assert _one(t, 1)["label"] == 6
    # a one-pixel island in the last pixel of a 3 x 3 raster
    m = np.zeros((3, 3), dtype=np.uint8)
    m[2, 2] = 7
    assert _one(_table(m, exclude=0)) == dict(label=8, cls=7, pixels=1, sum_x=2, sum_y=2, bbox=[2, 2, 3, 3], edges_v=2, edges_h=2, point=8)
    # the ring: 9 x 11, the frame rows 1..7 x columns 1..9, two thick, around the hole rows 3..5 x columns 3..7
    t = _table(OC.ring(), exclude=0)
    px = 7 * 9 - 3 * 5
    assert _one(t) == dict(label=12, cls=1, pixels=px, sum_x=5 * px, sum_y=4 * px, bbox=[1, 1, 10, 8], edges_v=2 * 7 + 2 * 3, edges_h=2 * 9 + 2 * 5,
                           point=2 * 11 + 5)          # the centre (5, 4) is in the hole; (5, 2) and (5, 6) are 2 away, (2, 4) 3
    assert OC.ring()[4, 5] == 0 and OC.ring()[2, 5] == 1
    # the U: 9 x 10, arms columns 1..2 and 7..8 over rows 1..7, the floor rows 6..7
    t = _table(OC.u_shape(), exclude=0)
    px = 2 * 7 * 2 + 2 * 4
    sy = 2 * 2 * sum(range(1, 8)) + 4 * (6 + 7)
    assert _one(t)["pixels"] == px and _one(t)["sum_x"] == px * 9 // 2 and _one(t)["sum_y"] == sy and _one(t)["bbox"] == [1, 1, 9, 8]
    cx, cy = (px * 9 // 2) // px, sy // px
    assert (cx, cy) == (4, 4) and OC.u_shape()[cy, cx] == 0                              # between the arms
    assert _one(t)["point"] == 4 * 10 + 2                                                # (2, 4) is 2 away, (7, 4) 3
    assert _one(t)["edges_v"] == 2 * 7 + 2 * 5 and _one(t)["edges_h"] == 2 + 2 + 4 + 8
    # the hollow cross: four pixels around a missing centre, one object by a hand-made label image: all at distance 1, the smallest index wins
    m = np.zeros((3, 3), dtype=np.uint8)
    m[0, 1] = m[1, 0] = m[1, 2] = m[2, 1] = 1
    lab = OC.own_labels(m.astype(np.int64))
    t = OR.table(m, lab, exclude=0)
    assert _one(t) == dict(label=1, cls=1, pixels=4, sum_x=4, sum_y=4, bbox=[0, 0, 3, 3], edges_v=8, edges_h=8, point=1)


def test_the_point_lies_in_the_object_and_the_centroid_need_not():
    outside = 0
    for m in (OC.ring(), OC.u_shape(), OC.cross(), OC.noise_mask(40, 56, 3)):
        lab = R.label_components(m, 4)
        t = OR.table(m, lab)
        W = m.shape[1]
        assert (lab.ravel()[t["point"]] == t["label"]).all()
        cx, cy = t["sum_x"] // t["pixels"], t["sum_y"] // t["pixels"]
        inside = lab[cy, cx] == t["label"]
        d2 = (t["point"] % W - cx) ** 2 + (t["point"] // W - cy) ** 2
        assert ((d2 == 0) == inside).all()
        outside += int((~inside).sum())
    assert outside >= 2          # the ring and the U at least


@pytest.mark.parametrize("shape", OC.SHAPES)
def test_edges_equal_the_ring_lengths_of_the_reference_tracer_and_the_fast_form_equals_the_loop(shape):
    H, W = shape
    for name, (m, lab) in OC.patterns(H, W, seed=H * 1000 + W).items():
        for exclude in (None, 1, (0, 2)):
            slow, fast = OR.table(m, lab, exclude), OR.table_fast(m, lab, exclude)
            assert OR.same(slow, fast), (shape, name, exclude)
            assert OR.bad_bits(m, lab) == 0
        if name in ("split", "blocks", "hstripes", "vstripes", "checker") or H * W > 3000:
            continue          # the tracer labels components itself: only where the labels ARE the components, and on small rasters
        polys = VR.polygonize(m, exclude=1)
        t = OR.table(m, lab, 1)
        assert np.array_equal(t["label"], polys["poly_label"]) and np.array_equal(t["pixels"], polys["poly_pixels"])
        assert np.array_equal(t["cls"], polys["poly_class"])
        assert np.array_equal(t["edges_v"] + t["edges_h"], OR.ring_lengths(polys)), (shape, name)


def test_edges_of_the_noise_mask_equal_the_ring_lengths():
    m = OC.noise_mask(40, 56, 8)
    polys, t = VR.polygonize(m), _table(m)
    assert np.array_equal(t["label"], polys["poly_label"]) and len(t["label"]) > 30
    assert np.array_equal(t["edges_v"] + t["edges_h"], OR.ring_lengths(polys))
    assert int(t["pixels"].sum()) == m.size and (t["edges_v"] >= 2).all() and (t["edges_h"] >= 2).all()


def test_against_scipy_where_it_is_there():
    try:
        from scipy import ndimage
    except ImportError:
        pytest.skip("scipy is not installed")
    m = OC.noise_mask(40, 56, 5)
    lab = R.label_components(m, 4)
    t = OR.table(m, lab)
    ids = t["label"] + 1
    assert np.array_equal(ndimage.sum(np.ones_like(lab), lab + 1, ids).astype(np.int64), t["pixels"])
    com = np.array(ndimage.center_of_mass(np.ones_like(lab), lab + 1, ids))
    assert np.allclose(com[:, 0], t["sum_y"] / t["pixels"], rtol=0, atol=1e-9) and np.allclose(com[:, 1], t["sum_x"] / t["pixels"], rtol=0, atol=1e-9)
    index = np.zeros(lab.size + 1, dtype=np.int64)
    index[ids] = np.arange(len(ids)) + 1
    for k, sl in enumerate(ndimage.find_objects(index[lab + 1])):
        assert [sl[1].start, sl[0].start, sl[1].stop, sl[0].stop] == t["bbox"][k].tolist()


def test_bad_labels_set_their_bits():
    m, lab = OC.patterns(5, 7, 1)["blocks"]
    for value, at, bit in ((35, 3, OR.BAD_RANGE), (-1, 0, OR.BAD_RANGE), (1, 9, OR.BAD_CANONICAL)):
        bad = lab.copy()
        bad.reshape(-1)[at] = value
        assert OR.bad_bits(m, bad) & bit, (value, at)
    wrong = m.copy()
    wrong[0, 1] = 9
    assert OR.bad_bits(wrong, lab) == OR.BAD_CLASS


def test_rows_derive_what_the_docstring_says():
    OB = _ob()
    gt = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.25)
    m = OC.placed((9, 12), OC.ring(7, 9), (2, 3))
    t = _table(m, exclude=0)
    row, = OR.rows(t, gt, codes=["bg", "crown"], class_zero=True, instance=[5])
    px = 5 * 7 - 1 * 3
    assert list(row) == ["class", "name", "pixels", "area", "perimeter", "centroid_x", "centroid_y", "bbox", "diameter", "compactness", "point_x",
                         "point_y", "on_edge", "instance"]
    assert row["class"] == 0 and row["name"] == "crown" and row["pixels"] == px and row["area"] == px * 0.125 and row["instance"] == 5
    assert row["perimeter"] == (2 * 7 + 2 * 3) * 0.5 + (2 * 5 + 2 * 1) * 0.25
    assert row["centroid_x"] == 400000.0 + (7 + 0.5) * 0.5 and row["centroid_y"] == 5700000.0 - (5 + 0.5) * 0.25
    assert row["bbox"] == [400000.0 + 4 * 0.5, 5700000.0 - 8 * 0.25, 400000.0 + 11 * 0.5, 5700000.0 - 3 * 0.25] and row["on_edge"] is False
    assert row["diameter"] == 2 * math.sqrt(row["area"] / math.pi) and row["compactness"] == 4 * math.pi * row["area"] / row["perimeter"] ** 2
    # the centre (7, 5) is the middle of the hole (row 5, columns 6..8); (7, 4) above it is the first pixel of the ring at distance 1
    assert (row["point_x"], row["point_y"]) == (400000.0 + 7.5 * 0.5, 5700000.0 - 4.5 * 0.25)
    # the module derives the same rows from the same table, with and without a geotransform
    table = OB.ObjectTable(**{f: torch.from_numpy(t[f]) for f in OR.FIELDS}, shape=t["shape"])
    assert OB.object_rows(table, gt, ["bg", "crown"], True, [5]) == [row]
    full = _table(m)
    assert OB.object_rows(full) == OR.rows(full) and OR.rows(full)[0]["on_edge"] is True and OR.rows(full)[0]["class"] == 0
    assert OB.object_rows(full, class_zero=True)[0]["class"] == -1
    assert "name" not in OR.rows(full)[0] and "instance" not in OR.rows(full)[0]
    for kw in (dict(codes=["only"]), dict(instance=[1]), dict(geotransform=(0, 1, 0.5, 0, 0, 1))):
        with pytest.raises(ValueError):
            OB.object_rows(full, **kw)


# ------------------------------------------------------------------------------------------------------------ the writers

def test_write_objects_geojson_and_csv(tmp_path):
    OB = _ob()
    gt = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)
    t = _table(OC.noise_mask(20, 31, 2))
    table = OB.ObjectTable(**{f: torch.from_numpy(t[f]) for f in OR.FIELDS}, shape=t["shape"])
    want = OR.rows(t, gt, class_zero=True)
    n = OB.write_objects(tmp_path / "o.geojson", table, gt, epsg=25832, class_zero=True)
    kept = [r for r in want if r["class"] >= 0]
    assert n == len(kept) < len(want)                                                   # under class_zero class 0 gets no feature
    doc = json.load(open(tmp_path / "o.geojson"))
    assert doc["crs"] == {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::25832"}} and doc["type"] == "FeatureCollection"
    assert [f["properties"] for f in doc["features"]] == kept
    assert all(f["geometry"] == {"type": "Point", "coordinates": [r["point_x"], r["point_y"]]} for f, r in zip(doc["features"], kept))
    assert OB.write_objects(tmp_path / "rows.geojson", want, gt, epsg=25832, class_zero=True) == n          # rows in the table's place
    assert (tmp_path / "rows.geojson").read_bytes() == (tmp_path / "o.geojson").read_bytes()
    assert "crs" not in json.load(open(OB.write_objects(tmp_path / "p.geojson", table) and tmp_path / "p.geojson"))
    assert OB.write_objects(tmp_path / "o.csv", table, gt) == len(want)
    with open(tmp_path / "o.csv", newline="") as f:
        lines = list(csv.reader(f))
    plain = OR.rows(t, gt)
    names = [k for k in plain[0] if k != "bbox"]
    assert lines[0] == ["class", "pixels", "area", "perimeter", "centroid_x", "centroid_y", "xmin", "ymin", "xmax", "ymax", "diameter", "compactness",
                        "point_x", "point_y", "on_edge"] and len(lines) == len(plain) + 1
    for line, row in zip(lines[1:], plain):
        got = dict(zip(lines[0], line))
        assert [float(got[k]) for k in ("xmin", "ymin", "xmax", "ymax")] == row["bbox"]
        assert all(got[k] == str(row[k]) if not isinstance(row[k], float) else float(got[k]) == row[k] for k in names)
    with pytest.raises(ValueError, match="geojson or .csv"):
        OB.write_objects(tmp_path / "o.shp", table)
    empty = OB.ObjectTable(**{f: torch.from_numpy(t[f][:0]) for f in OR.FIELDS}, shape=t["shape"])
    assert OB.write_objects(tmp_path / "e.geojson", empty) == 0 and json.load(open(tmp_path / "e.geojson"))["features"] == []
    assert OB.write_objects(tmp_path / "e.csv", empty) == 0


def test_write_geojson_without_attributes_writes_the_bytes_it_wrote_and_with_them_joins_by_label(tmp_path):
    from unet_amd import vectorize as VZ
    OB = _ob()
    gt = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)
    m = OC.noise_mask(20, 31, 2)
    polys = VR.polygonize(m, exclude=0)
    assert list(inspect.signature(VZ.write_geojson).parameters)[-1] == "attributes"
    assert inspect.signature(VZ.write_geojson).parameters["attributes"].default is None
    kw = dict(geotransform=gt, epsg=25832, codes=list("abcde"), class_zero=True, instance=np.arange(len(polys["poly_label"])))
    VZ.write_geojson(tmp_path / "a.geojson", polys, **kw)
    VZ.write_geojson(tmp_path / "b.geojson", polys, **kw, attributes=None)
    assert (tmp_path / "a.geojson").read_bytes() == (tmp_path / "b.geojson").read_bytes()
    t = _table(m, exclude=(0, 3))                                                       # class 3 has polygons and no rows
    rows = OR.rows(t, gt, list("abcde"), True)
    by_label = OB.rows_by_label(t, rows)
    assert list(by_label) == t["label"].tolist()
    VZ.write_geojson(tmp_path / "c.geojson", polys, **kw, attributes=by_label)
    plain, joined = (json.load(open(tmp_path / f))["features"] for f in ("a.geojson", "c.geojson"))
    assert len(plain) == len(joined) and VZ.ATTRIBUTE_KEYS == ("perimeter", "centroid_x", "centroid_y", "diameter", "compactness", "on_edge", "point_x", "point_y")
    seen = 0
    for label, a, c in zip(polys["poly_label"].tolist(), plain, joined):
        assert a["geometry"] == c["geometry"]
        if label in by_label:
            seen += 1
            assert list(c["properties"]) == list(a["properties"]) + list(VZ.ATTRIBUTE_KEYS)
            assert all(c["properties"][k] == by_label[label][k] for k in VZ.ATTRIBUTE_KEYS)
            assert c["properties"]["pixels"] == by_label[label]["pixels"] and c["properties"]["area"] == by_label[label]["area"]
        else:
            assert c["properties"] == a["properties"] and a["properties"]["class"] == 2
    assert 0 < seen < len(plain)


# ------------------------------------------------------------------------------------------------------------ the planner

def test_check_outputs_rules_for_the_new_arguments():
    import predict as P
    base = P.check_outputs()
    assert base.objects is None and base.keep is False and base.encode_in_place is False
    assert repr(base).endswith(", zonal_objects=False, objects=None)")
    plan = P.check_outputs(objects="o.geojson")
    assert plan.objects == () and plan.keep and not plan.encode_in_place
    assert P.check_outputs(objects=True, objects_exclude=3).objects == (3,)
    assert P.check_outputs(objects=True, objects_exclude=[4, 2], class_zero=True).objects == (0, 2, 4)          # class 0 is always excluded there
    assert P.check_outputs(objects=True, class_zero=True).objects == (0,)
    for kw in (dict(), dict(compress="lzw"), dict(vector="v.geojson"), dict(raster=False), dict(large_file=True), dict(merge=False), dict(regression=True),
               dict(instances={"classes": [1]}, instances_raster=True), dict(zones="z.geojson", zonal_objects=True)):
        a, b = P.check_outputs(**kw), P.check_outputs(**kw, objects=None, objects_exclude=None)
        assert repr(a) == repr(b) and a.keep == b.keep and a.encode_in_place == b.encode_in_place and a.objects is None, kw
        assert repr(P.check_outputs(**kw, objects=False)) == repr(a)
        if not (kw.get("large_file") or kw.get("merge") is False or kw.get("regression")):
            c = P.check_outputs(**kw, objects="o.geojson")
            assert c.keep and c.encode_in_place == a.encode_in_place and c.objects == (), kw
            assert repr(dataclasses.replace(c, objects=None)) == repr(a), kw
    for kw, text in ((dict(regression=True), "object attributes needs the class mask: not with regression, all_classes or specific_class"),
                     (dict(all_classes=True), "object attributes needs the class mask"),
                     (dict(specific_class=1), "object attributes needs the class mask"),
                     (dict(large_file=True), "object attributes needs the class mask on one device: not with large_file"),
                     (dict(merge=False), "object attributes needs merge=True: per-tile outputs are not measured")):
        with pytest.raises(ValueError, match=text):
            P.check_outputs(**kw, objects="o.geojson")
    with pytest.raises(ValueError, match="objects_exclude without an objects output"):
        P.check_outputs(objects_exclude=1)
    with pytest.raises(ValueError, match="objects must be None, a bool or the path"):
        P.check_outputs(objects=3)
    with pytest.raises(ValueError, match="class ids must be ints in 0..255"):
        P.check_outputs(objects=True, objects_exclude=[256])
    # an objects file is an output: of instances, and for return_array=False
    with pytest.raises(ValueError, match="return_array=False needs out_path"):
        P.check_outputs(raster=False, return_array=False)
    assert P.check_outputs(raster=False, return_array=False, objects="o.csv").objects == ()
    with pytest.raises(ValueError, match="instances without an output"):
        P.check_outputs(instances={"classes": [1]})
    assert P.check_outputs(instances={"classes": [1]}, objects="o.geojson").instances is not None
    # in front of the zonal arguments, which stay last
    assert list(inspect.signature(P.check_outputs).parameters)[-4:] == ["objects", "objects_exclude", "zones", "zonal_objects"]
    assert [f.name for f in dataclasses.fields(P.OutputPlan)][-1] == "objects"


def test_entry_points_take_the_arguments_and_refuse_before_the_model_is_loaded(tmp_path):
    import predict as P
    sig = inspect.signature(P.predict_raster).parameters
    assert sig["objects_path"].default is None and sig["objects_exclude"].default is None
    sig = inspect.signature(P.save_predictions).parameters
    assert sig["objects"].default is False and sig["objects_exclude"].default is None
    with pytest.raises(ValueError, match="object attributes needs the class mask"):
        P.predict_raster(None, None, objects_path="o.geojson", regression=True)
    with pytest.raises(ValueError, match="not with large_file"):
        P.predict_raster(None, None, objects_path="o.geojson", large_file=True)
    with pytest.raises(ValueError, match="objects_exclude without an objects output"):
        P.predict_raster(None, None, objects_exclude=[1])
    with pytest.raises(ValueError, match="object attributes needs merge=True"):
        P.save_predictions(tmp_path / "no_model.pkl", tmp_path, False, merge=False, objects=True)
    with pytest.raises(ValueError, match="objects_exclude without an objects output"):
        P.save_predictions(tmp_path / "no_model.pkl", tmp_path, False, merge=True, objects_exclude=2)


def test_params_and_main_passes_the_objects(monkeypatch):
    import params_and_main as M
    import predict
    assert M.OBJECTS is False and M.OBJECTS_EXCLUDE is None
    calls = {}
    monkeypatch.setattr(predict, "save_predictions", lambda *a, **kw: calls.update(kw))
    monkeypatch.setattr(M, "Create_tiles", False); monkeypatch.setattr(M, "Train", False); monkeypatch.setattr(M, "Predict", True)
    monkeypatch.setattr(M, "enable_extra_parameters", True)
    M.main()
    assert "objects" not in calls and "objects_exclude" not in calls          # the defaults pass nothing new
    monkeypatch.setattr(M, "OBJECTS", True); monkeypatch.setattr(M, "OBJECTS_EXCLUDE", [0])
    M.main()
    assert calls["objects"] is True and calls["objects_exclude"] == [0]
    calls.clear()
    monkeypatch.setattr(M, "enable_extra_parameters", False)                  # the non-expert branch resets them
    M.main()
    assert "objects" not in calls and M.OBJECTS is False and M.OBJECTS_EXCLUDE is None


# ------------------------------------------------------------------------------------------------------------ the library and the limits

def test_the_c_abi_symbols_are_in_the_built_library():
    from unet_amd import _lib
    names = ("unet_obj_point_packed", "unet_obj_compact", "unet_obj_accumulate", "unet_obj_point")
    assert set(names) <= set(_lib.declared_symbols())
    for n in names:
        assert hasattr(_lib.lib, n) and n in _lib._sig
    from unet_amd import ops
    assert ops.obj_point_packed(20000, 20000) and ops.obj_point_packed(65536, 65536) and ops.obj_point_packed(1, 92682)
    assert not ops.obj_point_packed(1, 1000000) and not ops.obj_point_packed(92683, 2) and not ops.obj_point_packed(65537, 65537)


def test_argument_and_limit_errors_need_no_device():
    OB = _ob()
    m, lab = np.zeros((4, 6), dtype=np.uint8), np.zeros((4, 6), dtype=np.int32)
    for bad in (None, m.astype(np.int32), m[0], [[0]], torch.zeros(4, 6)):
        with pytest.raises(ValueError, match="mask must be"):
            OB.measure_objects(bad)
    for bad in (lab.astype(np.int64), lab[0], "labels"):
        with pytest.raises(ValueError, match="labels must be"):
            OB.measure_objects(m, bad)
    with pytest.raises(ValueError, match="labels has shape"):
        OB.measure_objects(m, lab[:3])
    for bad in (-1, 256, 1.5, "a", [0, 300]):
        with pytest.raises(ValueError, match="exclude"):
            OB.measure_objects(m, lab, bad)

    for shape, text in (((2 ** 20, 4), "2\\^20 - 1"), ((4, 2 ** 20), "2\\^20 - 1"), ((2 ** 16, 2 ** 15), "2\\^31 - 1 pixels")):
        big = np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.uint8), shape=shape, strides=(0, 0))
        with pytest.raises(ValueError, match=text):          # from the shape alone, before anything is uploaded
            OB.measure_objects(big)
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="no device"):
            OB.measure_objects(m, lab)                                   # no host fallback
        with pytest.raises(ValueError, match="no device"):
            OB.measure_objects(m)
    for word in ("smallest linear index", "half open", "lexicographically", "another label or lies outside", "host fallback", "second moments",
                 "8-connectivity", "labels[labels[p]] != labels[p]", "2^31 - 1"):
        assert word.lower() in " ".join(OB.__doc__.lower().split()), word
    assert OB.check_objects(None) is None and OB.check_objects(False) is None and OB.check_objects(True, 2, True) == (0, 2)
