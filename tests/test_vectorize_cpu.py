"""CPU suite of the polygonizer (unet_amd/vectorize.py): the plain-Python restatement of the ring rules (tests/vectorize_ref.py) against
rings written out by hand and against the four properties the rules promise, write_geojson on the reference's output, and every argument
error of the module and of the prediction entry points -- all raised with no GPU present."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import postprocess_ref as R  # noqa: E402
import vectorize_ref as V  # noqa: E402

GT = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)


def _vec():
    from unet_amd import vectorize
    return vectorize


def _rings(mask, exclude=None):
    return [(r["label"], r["xy"], r["area"]) for r in V.trace(np.array(mask, dtype=np.uint8), exclude)[0]]


# ------------------------------------------------------------------------------------------------------------ literal rings

def test_single_pixel():
    assert _rings([[1]]) == [(0, [(0, 0), (0, 1), (1, 1), (1, 0)], 1)]


def test_frame_with_one_hole():
    assert _rings([[1, 1, 1], [1, 0, 1], [1, 1, 1]]) == [
        (0, [(0, 0), (0, 3), (3, 3), (3, 0)], 9),
        (0, [(2, 1), (2, 2), (1, 2), (1, 1)], -1),          # the hole: clockwise on screen, leader = the S side of pixel (0, 1)
        (4, [(1, 1), (1, 2), (2, 2), (2, 1)], 1)]


def test_frame_whose_hole_pixels_touch_diagonally_has_two_holes_not_a_figure_8():
    m = np.ones((4, 4), dtype=np.uint8)
    m[1, 1] = m[2, 2] = 0
    rings, info = V.trace(m)
    assert info["swaps"] == 1
    assert [(r["label"], r["xy"], r["area"]) for r in rings] == [
        (0, [(0, 0), (0, 4), (4, 4), (4, 0)], 16),
        (0, [(2, 1), (2, 2), (1, 2), (1, 1)], -1),
        (5, [(1, 1), (1, 2), (2, 2), (2, 1)], 1),
        (0, [(3, 2), (3, 3), (2, 3), (2, 2)], -1),
        (10, [(2, 2), (2, 3), (3, 3), (3, 2)], 1)]
    p = V.polygonize(m)
    assert p["poly_label"].tolist() == [0, 5, 10] and p["poly_pixels"].tolist() == [14, 1, 1]
    assert p["poly_ring_start"].tolist() == [0, 3, 4, 5] and p["poly_rings"].tolist() == [0, 1, 3, 2, 4]          # exterior, then holes by leader


def test_two_diagonal_pixels_of_one_class_inside_another_class():
    m = np.zeros((4, 4), dtype=np.uint8)
    m[1, 1] = m[2, 2] = 7
    got = _rings(m)
    assert got == [
        (0, [(0, 0), (0, 4), (4, 4), (4, 0)], 16),
        (0, [(2, 1), (2, 2), (1, 2), (1, 1)], -1),
        (5, [(1, 1), (1, 2), (2, 2), (2, 1)], 1),
        (0, [(3, 2), (3, 3), (2, 3), (2, 2)], -1),
        (10, [(2, 2), (2, 3), (3, 3), (3, 2)], 1)]          # 4-connectivity: the two pixels are two polygons


def test_l_shape():
    got = _rings([[1, 0], [1, 1]])
    assert got == [
        (0, [(0, 0), (0, 2), (2, 2), (2, 1), (1, 1), (1, 0)], 3),
        (1, [(1, 0), (1, 1), (2, 1), (2, 0)], 1)]


# ------------------------------------------------------------------------------------------------------------ properties (a)-(d)

def _check_properties(m, exclude=None):
    H, W = m.shape
    rings, info = V.trace(m, exclude)
    lab = R.label_components(m, 4)
    sizes = R.component_sizes(lab).ravel()
    leaders = [r["leader"] for r in rings]
    assert leaders == sorted(leaders) and len(set(leaders)) == len(leaders)
    by = {}
    for r in rings:
        assert r["leader"] == min(r["edges"]) and len(r["xy"]) >= 4
        assert V.vertex_visits_once(r["edges"], W)                                                                  # (a)
        by.setdefault(r["label"], []).append(r)
    excl = V.exclude_set(exclude)
    assert set(by) == {int(l) for l in np.unique(lab) if int(m.ravel()[l]) not in excl}
    for l, rs in by.items():
        positive = [r for r in rs if r["area"] > 0]
        assert len(positive) == 1 and positive[0]["leader"] == 4 * l and all(r["area"] < 0 for r in rs if r is not positive[0])          # (b)
        assert sum(r["area"] for r in rs) == sizes[l]                                                               # (c)
        assert np.array_equal(V.fill_even_odd([r["xy"] for r in rs], H, W), lab == l)                                # (d)
    return info["swaps"]


@pytest.mark.parametrize("shape", [(17, 23), (40, 33)])
def test_properties_on_the_patterns(shape):
    swaps = {name: _check_properties(m) for name, m in R.patterns(*shape).items()}
    assert swaps["noise2"] > 0 and swaps["constant"] == 0


def test_properties_on_all_16_binary_2x2_masks_and_with_exclude():
    for i in range(16):
        _check_properties(np.array([[i & 1, i >> 1 & 1], [i >> 2 & 1, i >> 3 & 1]], dtype=np.uint8))
    m = R.patterns(17, 23)["noise5"]
    _check_properties(m, 0)
    _check_properties(m, [1, 4])
    assert V.polygonize(m, range(5))["xy"].shape == (0, 2)


# ------------------------------------------------------------------------------------------------------------ write_geojson

def _mask():
    m = R.patterns(24, 31, seed=4)["blocks"].copy()
    m[3:12, 4:15] = 2
    m[5:9, 6:11] = 0          # a hole ...
    m[6, 8] = 3               # ... with an island
    return m


def _raster_of(doc, H, W, gt=None, shift=0):
    """even-odd fill of every feature's rings, mapped back through the inverse geotransform; 255 where no feature covers a pixel"""
    out = np.full((H, W), 255, dtype=np.int64)
    for f in doc["features"]:
        rings = []
        for ring in f["geometry"]["coordinates"]:
            assert ring[0] == ring[-1] and len(ring) >= 5
            pts = ring[:-1]
            if gt is not None:
                pts = [((x - gt[0]) / gt[1], (y - gt[3]) / gt[5]) for x, y in pts]
                assert all(float(x).is_integer() and float(y).is_integer() for x, y in pts)
            rings.append([(int(x), int(y)) for x, y in pts])
        inside = V.fill_even_odd(rings, H, W)
        assert (out[inside] == 255).all()          # features do not overlap
        out[inside] = f["properties"]["class"] + shift
    return out


def _area2(ring):
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring[:-1], ring[1:]))


def test_geojson_round_trip_orientation_and_properties(tmp_path):
    VZ = _vec()
    m = _mask()
    H, W = m.shape
    p = V.polygonize(m)
    n = VZ.write_geojson(tmp_path / "a.geojson", p, GT, 32632, codes=["water", "wood", "field", "town"])
    doc = json.load(open(tmp_path / "a.geojson"))
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == n == len(p["poly_label"])
    assert doc["crs"] == {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::32632"}}
    holes = 0
    for f, cls, px in zip(doc["features"], p["poly_class"].tolist(), p["poly_pixels"].tolist()):
        assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon"
        assert f["properties"] == {"class": cls, "name": ["water", "wood", "field", "town"][cls], "pixels": px, "area": px * 0.25}
        rings = f["geometry"]["coordinates"]
        assert _area2(rings[0]) > 0 and all(_area2(r) < 0 for r in rings[1:])          # y up in map coordinates: CCW exterior, CW holes
        assert (_area2(rings[0]) + sum(_area2(r) for r in rings[1:])) / 2 == px * 0.25
        holes += len(rings) - 1
    assert holes >= 2
    assert np.array_equal(_raster_of(doc, H, W, GT), m)
    # the text holds repr of the float64 coordinates
    x0 = GT[0] + float(p["xy"][0, 0]) * GT[1]
    assert repr(x0) in open(tmp_path / "a.geojson").read()


def test_geojson_without_geotransform_holds_integer_pixel_coordinates(tmp_path):
    VZ = _vec()
    m = _mask()
    p = V.polygonize(m)
    VZ.write_geojson(tmp_path / "b.geojson", p)
    doc = json.load(open(tmp_path / "b.geojson"))
    assert "crs" not in doc
    assert all(isinstance(c, int) for f in doc["features"] for r in f["geometry"]["coordinates"] for pt in r for c in pt)
    assert all("name" not in f["properties"] and f["properties"]["area"] == f["properties"]["pixels"] for f in doc["features"])
    assert np.array_equal(_raster_of(doc, *m.shape), m)


def test_geojson_class_zero_and_exclude(tmp_path):
    VZ = _vec()
    m = _mask()
    H, W = m.shape
    VZ.write_geojson(tmp_path / "c.geojson", V.polygonize(m), GT, class_zero=True, codes=["NO_Data", "a", "b", "c"])
    doc = json.load(open(tmp_path / "c.geojson"))
    back = _raster_of(doc, H, W, GT, shift=1)
    assert np.array_equal(back == 255, m == 0) and np.array_equal(back[m != 0], m[m != 0])          # class 0 has no feature, ids are shifted
    assert {f["properties"]["class"] for f in doc["features"]} == {0, 1, 2}
    assert all(f["properties"]["name"] == "abc"[f["properties"]["class"]] for f in doc["features"])
    VZ.write_geojson(tmp_path / "d.geojson", V.polygonize(m, [1, 3]), GT)
    back = _raster_of(json.load(open(tmp_path / "d.geojson")), H, W, GT)
    keep = (m != 1) & (m != 3)
    assert np.array_equal(back == 255, ~keep) and np.array_equal(back[keep], m[keep])
    assert VZ.write_geojson(tmp_path / "e.geojson", V.polygonize(m, range(4))) == 0
    assert json.load(open(tmp_path / "e.geojson")) == {"type": "FeatureCollection", "features": []}


def test_epsg_of_tags():
    VZ = _vec()
    head = (1, 1, 0, 3)
    assert VZ.epsg_of_tags({34735: head + (1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32632)}) == 32632
    assert VZ.epsg_of_tags({34735: head + (1024, 0, 1, 2, 2048, 0, 1, 4326, 3072, 0, 1, 32767)}) == 4326
    assert VZ.epsg_of_tags({34735: (1, 1, 0, 1, 3072, 0, 1, 32767)}) is None
    assert VZ.epsg_of_tags({34735: (1, 1, 0, 1, 3072, 34736, 1, 0)}) is None          # the value lives in another tag
    assert VZ.epsg_of_tags({}) is None and VZ.epsg_of_tags(None) is None and VZ.epsg_of_tags({34735: (1, 1)}) is None


# ------------------------------------------------------------------------------------------------------------ argument errors

def test_polygonize_refuses_bad_arguments_before_the_gpu():
    VZ = _vec()
    m = np.zeros((4, 4), dtype=np.uint8)
    for bad in (np.zeros((4, 4), dtype=np.int32), np.zeros((2, 4, 4), dtype=np.uint8), np.zeros((0, 4), dtype=np.uint8), [[0]],
                torch.zeros((4, 4), dtype=torch.int64), np.broadcast_to(np.uint8(0), (65536, 32768))):
        with pytest.raises(ValueError):
            VZ.polygonize(bad)
    for bad in (-1, 256, 1.5, [0, 300], "ab", True, [None]):
        with pytest.raises(ValueError):
            VZ.polygonize(m, exclude=bad)
    with pytest.raises(TypeError):
        VZ.polygonize(m, connectivity=8)          # 4-connected only: there is no such argument
    assert "Connectivity 8" in VZ.__doc__ and "Connectivity 8" in VZ.polygonize.__doc__
    for kw in (dict(geotransform=(0, 1, 0, 0, 0)), dict(geotransform=(0, 0, 0, 0, 0, -1)), dict(geotransform=(0, 1, 0.1, 0, 0, -1)), dict(epsg=0),
               dict(epsg="4326"), dict(codes=[])):
        with pytest.raises(ValueError):
            VZ.write_geojson(os.devnull, V.polygonize(m), **kw)


def test_entry_points_refuse_combinations_before_the_model_loads(tmp_path):
    import predict as P
    raster = np.zeros((3, 64, 64), dtype=np.uint8)
    out = tmp_path / "v.geojson"
    for kw in (dict(regression=True), dict(all_classes=True), dict(specific_class=1), dict(large_file=True), dict(vector_exclude=256),
               dict(vector_exclude="x")):
        with pytest.raises(ValueError):
            P.predict_raster(None, raster, 32, vector_path=out, **kw)          # model None: nothing but the checks can run
    with pytest.raises(ValueError):
        P.predict_raster(None, raster, 32, vector_exclude=1)                   # exclude without a vector output
    missing = tmp_path / "no_such_model.pkl"
    for kw in (dict(regression=True), dict(all_classes=True), dict(specific_class=1), dict(large_file=True), dict(merge=False),
               dict(vector_exclude=[1, -2])):
        kw = dict(dict(regression=False, merge=True), **kw)
        regression = kw.pop("regression")
        with pytest.raises(ValueError):
            P.save_predictions(missing, tmp_path, regression, vector=True, **kw)
    with pytest.raises(ValueError):
        P.save_predictions(missing, tmp_path, False, merge=True, vector_exclude=1)
    assert not out.exists()


def test_params_and_main_passes_vector_only_when_set(monkeypatch):
    import create_tiles_unet
    import params_and_main as M
    import predict
    import train
    assert M.VECTOR is False and M.VECTOR_EXCLUDE is None
    calls = {}
    monkeypatch.setattr(create_tiles_unet, "split_raster", lambda **kw: None)
    monkeypatch.setattr(train, "train_func", lambda *a: None)
    monkeypatch.setattr(predict, "save_predictions", lambda *a, **k: calls.setdefault("predict", (a, k)))
    monkeypatch.setattr(M, "Create_tiles", False); monkeypatch.setattr(M, "Train", False); monkeypatch.setattr(M, "Predict", True)
    monkeypatch.setattr(M, "enable_extra_parameters", True)
    M.main()
    assert calls.pop("predict")[1] == {"tta": None}
    monkeypatch.setattr(M, "VECTOR", True); monkeypatch.setattr(M, "VECTOR_EXCLUDE", [0])
    M.main()
    assert calls.pop("predict")[1] == {"tta": None, "vector": True, "vector_exclude": [0]}
    monkeypatch.setattr(M, "enable_extra_parameters", False)
    M.main()
    assert calls.pop("predict")[1] == {"tta": None} and M.VECTOR is False and M.VECTOR_EXCLUDE is None


# ------------------------------------------------------------------------------------------------------------ C ABI

NEW_SYMBOLS = ("unet_vec_flags", "unet_vec_scan_words", "unet_vec_scan", "unet_vec_read", "unet_vec_succ", "unet_vec_min_rounds", "unet_vec_swap",
               "unet_vec_rank_init", "unet_vec_rank_rounds", "unet_vec_ring_info", "unet_vec_place", "unet_vec_emit")


def test_header_declares_and_library_exports_the_new_symbols():
    from unet_amd import _lib as L
    declared = L.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L.lib, s) and s in L._sig, s


def test_bad_arguments_return_minus_one_without_a_launch():
    from unet_amd import _lib as L
    lib = L.lib
    p, q = 4096, 8192          # non-null, aligned addresses that are never dereferenced: every call below fails its host check
    big = 2 ** 31
    calls = [
        lambda: lib.unet_vec_flags(None, p, 4, 4, None, p, None),
        lambda: lib.unet_vec_flags(p, p, 65536, 32768, None, p, None),
        lambda: lib.unet_vec_scan(p, 0, p, p, None),
        lambda: lib.unet_vec_scan(p, big, p, p, None),
        lambda: lib.unet_vec_scan(p, 16, p + 2, p, None),
        lambda: lib.unet_vec_read(None, 1, None, None),
        lambda: lib.unet_vec_succ(p, p, 4, 4, 0, p, p, None),
        lambda: lib.unet_vec_succ(p, p, 4, 4, big, p, p, None),
        lambda: lib.unet_vec_min_rounds(p, 16, p, q, p, q, 1, 1, p, None),          # the buffer sets must differ
        lambda: lib.unet_vec_min_rounds(p, 16, p, q, p + 64, q + 64, 1, 65, p, None),
        lambda: lib.unet_vec_swap(p, p, p, 0, 4, p, p, None),
        lambda: lib.unet_vec_rank_init(p, p, 4, 4, p, p, p, p, None, p, 16, None),
        lambda: lib.unet_vec_rank_rounds(16, p, q, p, p, q + 64, q, 1, p, None),
        lambda: lib.unet_vec_ring_info(p, p, p, 4, 4, p, p, p, p, p, 0, p, p, p, None),
        lambda: lib.unet_vec_place(p, p, p, p, p, p, 16, 17, p, p, None),           # more rings than edges
        lambda: lib.unet_vec_emit(p, p, 4, 4, p, p, p, 16, 4, p + 4, None),             # xy not 8-byte aligned
    ]
    for i, c in enumerate(calls):
        assert c() == -1, i
        assert lib.unet_last_error(), i
    assert lib.unet_vec_scan_words(1) == 2 and lib.unet_vec_scan_words(4096) == 2 and lib.unet_vec_scan_words(4097) == 3
