"""CPU suite of the zonal statistics (unet_amd/zonal.py, csrc/zonal.hip): the C ABI, every argument error of the two new ops -- raised with
no GPU present --, the planner's rules for the new arguments, the host reader and writers on hand-made tables, and read_geojson against
what the commit before the parser was shared returned (tests/golden/zonal_read_geojson.json: recorded by calling that commit's
read_geojson on the files of zonal_cases.write_set_files, pixel and map coordinates, with and without class_zero)."""
import csv
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import zonal_cases as ZC  # noqa: E402
import zonal_ref as ZR  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "zonal_read_geojson.json")
NEW_SYMBOLS = ("unet_ras_resolve_ids", "unet_zonal_lds_bins", "unet_zonal_counts")


def _zn():
    from unet_amd import zonal
    return zonal


# ------------------------------------------------------------------------------------------------------------ C ABI

def test_header_declares_and_library_exports_the_new_symbols():
    from unet_amd import _lib as L
    declared = L.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L.lib, s) and s in L._sig, s
    assert "#define UNET_ABI_VERSION 8" in L.HEADER.read_text() and L.lib.unet_abi_version() == 8          # additions only
    bins = L.lib.unet_zonal_lds_bins()
    assert 256 <= bins and bins * 4 <= 64 * 1024          # at least one zone of 256 classes; uint32 bins within a workgroup's static LDS


def test_bad_arguments_return_minus_one_without_a_launch():
    from unet_amd import _lib as L
    lib = L.lib
    p = 4096          # a non-null, aligned address that is never dereferenced: every call below fails its host check
    side = 2 ** 20
    calls = [
        lambda: lib.unet_ras_resolve_ids(None, 4, 4, p, None),
        lambda: lib.unet_ras_resolve_ids(p, 4, 4, None, None),
        lambda: lib.unet_ras_resolve_ids(p, 0, 4, p, None),
        lambda: lib.unet_ras_resolve_ids(p, 4, side, p, None),
        lambda: lib.unet_zonal_counts(None, p, None, 4, 4, 1, 1, p, None, p, None),
        lambda: lib.unet_zonal_counts(p, None, None, 4, 4, 1, 1, p, None, p, None),
        lambda: lib.unet_zonal_counts(p, p, None, 4, 4, 1, 1, None, None, p, None),
        lambda: lib.unet_zonal_counts(p, p, None, 4, 4, 1, 1, p, None, None, None),
        lambda: lib.unet_zonal_counts(p, p, p, 4, 4, 1, 1, p, None, p, None),             # labels without objects
        lambda: lib.unet_zonal_counts(p, p, None, 4, 4, 1, 1, p, p, p, None),             # objects without labels
        lambda: lib.unet_zonal_counts(p, p, None, 0, 4, 1, 1, p, None, p, None),
        lambda: lib.unet_zonal_counts(p, p, None, 4, side, 1, 1, p, None, p, None),
        lambda: lib.unet_zonal_counts(p, p, None, 4, 4, 0, 1, p, None, p, None),
        lambda: lib.unet_zonal_counts(p, p, None, 4, 4, 2 ** 23, 1, p, None, p, None),
        lambda: lib.unet_zonal_counts(p, p, None, 4, 4, 1, 0, p, None, p, None),
        lambda: lib.unet_zonal_counts(p, p, None, 4, 4, 1, 257, p, None, p, None),
        lambda: lib.unet_zonal_counts(p, p, p, 65536, 32768, 1, 1, p, p, p, None),        # 2^31 pixels with int32 labels
    ]
    for i, c in enumerate(calls):
        assert c() == -1, i
        assert lib.unet_last_error(), i


# ------------------------------------------------------------------------------------------------------------ ops

def _args(H=4, W=6, Z=3, C=5, labels=False):
    z, m = torch.zeros((H, W), dtype=torch.int32), torch.zeros((H, W), dtype=torch.uint8)
    lab = torch.zeros((H, W), dtype=torch.int32) if labels else None
    return dict(zones=z, mask=m, labels=lab, Z=Z, C=C, counts=torch.zeros((Z, C), dtype=torch.int64),
                objects=torch.zeros((Z, C), dtype=torch.int64) if labels else None, bad=torch.zeros(1, dtype=torch.int64))


def _raises(text, **change):
    from unet_amd import ops
    a = _args(labels=change.pop("with_labels", False))
    a.update(change)
    with pytest.raises(ValueError, match=text):
        ops.zonal_counts(**a)


def test_zonal_counts_refuses_every_bad_argument_before_a_launch():
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    _raises("zones must be a torch.int32", zones=torch.zeros((4, 6), dtype=i64))
    _raises("mask must be a torch.uint8", mask=torch.zeros((4, 6), dtype=i32))
    _raises("counts must be a torch.int64", counts=torch.zeros((3, 5), dtype=i32))
    _raises("bad must be a torch.int64", bad=torch.zeros(1, dtype=i32))
    _raises("labels must be a torch.int32", with_labels=True, labels=torch.zeros((4, 6), dtype=i64))
    _raises("objects must be a torch.int64", with_labels=True, objects=torch.zeros((3, 5), dtype=i32))
    _raises("expected a shape", zones=np.zeros((4, 6), dtype=np.int32))
    _raises("mask must be a", mask=np.zeros((4, 6), dtype=np.uint8))
    _raises("expected a shape", zones=torch.zeros((24,), dtype=i32))
    _raises("mask has shape", mask=torch.zeros((6, 4), dtype=u8))
    _raises("counts has shape", counts=torch.zeros((5, 3), dtype=i64))
    _raises("counts has shape", counts=torch.zeros((15,), dtype=i64))
    _raises("bad has shape", bad=torch.zeros(2, dtype=i64))
    _raises("labels has shape", with_labels=True, labels=torch.zeros((4, 7), dtype=i32))
    _raises("objects has shape", with_labels=True, objects=torch.zeros((3, 4), dtype=i64))
    _raises("zones must be contiguous", zones=torch.zeros((6, 4), dtype=i32).t())
    _raises("mask must be contiguous", mask=torch.zeros((4, 12), dtype=u8)[:, ::2])
    _raises("counts must be contiguous", counts=torch.zeros((5, 3), dtype=i64).t())
    _raises("labels must be contiguous", with_labels=True, labels=torch.zeros((6, 4), dtype=i32).t())
    _raises("together or not at all", labels=torch.zeros((4, 6), dtype=i32))
    _raises("together or not at all", objects=torch.zeros((3, 5), dtype=i64))
    for C in (0, 257, -1):
        _raises("classes must lie in 1..256", C=C, counts=torch.zeros((3, max(C, 1)), dtype=i64))
    _raises("must be an int", C=5.0)
    _raises("must be an int", Z=True)
    _raises("zones must lie in", Z=0)
    _raises("zones must lie in", Z=2 ** 23, C=1)                  # the rasterizer's limit
    _raises("under 2\\^31", Z=2 ** 23, C=256)                     # Z * C = 2^31
    _raises("under 2\\^31", Z=2 ** 31, C=1)
    _raises("H and W must lie in", zones=torch.zeros((0, 6), dtype=i32))
    _raises("H and W must lie in", zones=torch.zeros((1, 2 ** 20), dtype=i32))
    _raises("must live on the GPU")                               # every tensor is right but on the host: the device is checked last


def test_ras_resolve_ids_refuses_every_bad_argument_before_a_launch():
    from unet_amd import ops
    i32 = torch.int32
    ok = torch.zeros((4, 6), dtype=i32)
    for text, plane, ids in (("plane must be a torch.int32", ok.to(torch.int64), ok), ("ids must be a torch.int32", ok, ok.to(torch.uint8)),
                             ("expected a shape", ok.reshape(-1), ok), ("ids has shape", ok, torch.zeros((6, 4), dtype=i32)),
                             ("plane must be contiguous", torch.zeros((6, 4), dtype=i32).t(), ok), ("ids must be contiguous", ok, torch.zeros((6, 4), dtype=i32).t()),
                             ("expected a shape", None, ok), ("ids must be a", ok, None), ("must live on the GPU", ok, ok.clone())):
        with pytest.raises(ValueError, match=text):
            ops.ras_resolve_ids(plane, ids)


def test_module_entry_points_refuse_limits_and_a_missing_device(tmp_path):
    ZN = _zn()
    z, m = np.zeros((4, 6), dtype=np.int32), np.zeros((4, 6), dtype=np.uint8)
    for kw in (dict(n_zones=0, n_classes=5), dict(n_zones=2 ** 23, n_classes=1), dict(n_zones=2 ** 23, n_classes=256), dict(n_zones=3, n_classes=257),
               dict(n_zones=3, n_classes=0), dict(n_zones=3.0, n_classes=5)):
        with pytest.raises(ValueError):
            ZN.zonal_counts(z, m, **kw)
    with pytest.raises(ValueError, match="mask has shape"):
        ZN.zonal_counts(z, m[:3], 3, 5)
    with pytest.raises(ValueError, match="labels has shape"):
        ZN.zonal_counts(z, m, 3, 5, labels=np.zeros((4, 5), dtype=np.int32))
    with pytest.raises(ValueError):
        ZN.zonal_counts(z.reshape(-1), m.reshape(-1), 3, 5)
    for shape in ((0, 4), (4, 2 ** 20), (4,), "ab"):
        with pytest.raises(ValueError):
            ZN.rasterize_ids(None, shape)
    with pytest.raises(ValueError):
        ZN.rasterize_ids("rings", (4, 4))
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="no device"):
            ZN.zonal_counts(z, m, 3, 5)                           # no host fallback
        with pytest.raises(ValueError, match="no device"):
            ZN.zonal_counts(z.astype(np.int64), m, 3, 5)          # ... and it is said before the types are looked at on the device
        (tmp_path / "z.geojson").write_text(json.dumps(_doc([_feat(_SQUARE, id=1)])))
        with pytest.raises(ValueError, match="no device"):
            ZN.rasterize_ids(ZN.read_zones(tmp_path / "z.geojson")[0], (4, 4))
        with pytest.raises(ValueError, match="no device"):
            ZN.zonal_mask(m, tmp_path / "z.geojson", tmp_path / "out.geojson")
        assert not (tmp_path / "out.geojson").exists()
    for word in ("first pixel in row-major order", "centroid", "ALL_TOUCHED", "reprojection", "Shapefile", "host fallback", "last feature", "2^23"):
        assert word.lower() in ZN.__doc__.lower(), word


# ------------------------------------------------------------------------------------------------------------ the planner

def test_check_outputs_rules_for_the_new_arguments():
    import predict as P
    base = P.check_outputs()
    assert base.zones is False and base.zonal_objects is False and base.keep is False and base.encode_in_place is False
    plan = P.check_outputs(zones="z.geojson")
    assert plan.zones and not plan.zonal_objects and plan.keep and not plan.encode_in_place
    assert P.check_outputs(zones="z.geojson", zonal_objects=True).zonal_objects
    # the defaults leave every other field, keep and encode as they were, whatever else is asked for
    for kw in (dict(), dict(compress="lzw"), dict(vector="v.geojson"), dict(raster=False), dict(large_file=True), dict(merge=False), dict(regression=True),
               dict(instances={"classes": [1]}, instances_raster=True)):
        a, b = P.check_outputs(**kw), P.check_outputs(**kw, zones=None, zonal_objects=False)
        assert repr(a) == repr(b) and a.keep == b.keep and a.encode_in_place == b.encode_in_place and not a.zones, kw
        if not (kw.get("large_file") or kw.get("merge") is False or kw.get("regression")):
            c = P.check_outputs(**kw, zones="z.geojson")
            assert c.keep and c.encode_in_place == a.encode_in_place and c.zones, kw
            assert repr(dataclasses.replace(c, zones=False)) == repr(a), kw
    for kw, text in ((dict(regression=True), "zonal statistics needs the class mask: not with regression, all_classes or specific_class"),
                     (dict(all_classes=True), "zonal statistics needs the class mask"),
                     (dict(specific_class=1), "zonal statistics needs the class mask"),
                     (dict(large_file=True), "zonal statistics needs the class mask on one device: not with large_file"),
                     (dict(merge=False), "zonal statistics needs merge=True: per-tile outputs are not summarised")):
        with pytest.raises(ValueError, match=text):
            P.check_outputs(**kw, zones="z.geojson")
    with pytest.raises(ValueError, match="zonal_objects without zones"):
        P.check_outputs(zonal_objects=True)
    with pytest.raises(ValueError, match="zones must be None or the path"):
        P.check_outputs(zones=True)
    # return_array=False is satisfied by a zonal output as by a vector output; instances may feed the table alone
    with pytest.raises(ValueError, match="return_array=False needs out_path"):
        P.check_outputs(raster=False, return_array=False)
    assert P.check_outputs(raster=False, return_array=False, zones="z.geojson").zones
    with pytest.raises(ValueError, match="instances without an output"):
        P.check_outputs(instances={"classes": [1]})
    assert P.check_outputs(instances={"classes": [1]}, zones="z.geojson", zonal_objects=True).instances is not None
    # the new arguments stand at the end of the signature
    import inspect
    assert list(inspect.signature(P.check_outputs).parameters)[-2:] == ["zones", "zonal_objects"]


def test_entry_points_take_the_arguments_and_refuse_before_the_model_is_loaded(tmp_path):
    import inspect

    import predict as P
    sig = inspect.signature(P.predict_raster).parameters
    assert sig["zones_path"].default is None and sig["zonal_path"].default is None and sig["zonal_objects"].default is False
    sig = inspect.signature(P.save_predictions).parameters
    assert sig["zones"].default is None and sig["zonal_objects"].default is False
    for kw in (dict(zones_path="z.geojson"), dict(zonal_path="t.csv")):
        with pytest.raises(ValueError, match="go together"):
            P.predict_raster(None, None, **kw)
    with pytest.raises(ValueError, match="zonal statistics needs the class mask"):
        P.predict_raster(None, None, zones_path="z.geojson", zonal_path="t.csv", regression=True)
    with pytest.raises(ValueError, match="zonal statistics needs merge=True"):
        P.save_predictions(tmp_path / "no_model.pkl", tmp_path, False, merge=False, zones="z.geojson")
    with pytest.raises(ValueError, match="zonal_objects without zones"):
        P.save_predictions(tmp_path / "no_model.pkl", tmp_path, False, merge=True, zonal_objects=True)


def test_params_and_main_passes_the_zones(monkeypatch):
    import params_and_main as M
    import predict
    assert M.ZONES is None and M.ZONAL_OBJECTS is False
    calls = {}
    monkeypatch.setattr(predict, "save_predictions", lambda *a, **kw: calls.update(kw))
    monkeypatch.setattr(M, "Create_tiles", False); monkeypatch.setattr(M, "Train", False); monkeypatch.setattr(M, "Predict", True)
    monkeypatch.setattr(M, "enable_extra_parameters", True)
    M.main()
    assert "zones" not in calls and "zonal_objects" not in calls          # the defaults pass nothing new
    monkeypatch.setattr(M, "ZONES", "parcels.geojson"); monkeypatch.setattr(M, "ZONAL_OBJECTS", True)
    M.main()
    assert calls["zones"] == "parcels.geojson" and calls["zonal_objects"] is True


# ------------------------------------------------------------------------------------------------------------ files

_SQUARE = {"type": "Polygon", "coordinates": [[[0, 0], [0, 4], [4, 4], [4, 0], [0, 0]]]}
_PARTS = {"type": "MultiPolygon", "coordinates": [[[[5, 0], [5, 2], [7, 2]]], [[[0, 5], [3, 5], [3, 8], [0, 8]], [[1, 6], [2, 6], [2, 7]]]]}
_CRS = {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::25832"}}


def _feat(geometry, **props):
    return {"type": "Feature", "properties": props, "geometry": geometry}


def _doc(features, crs=None):
    d = {"type": "FeatureCollection", "features": features}
    if crs is not None:
        d["crs"] = crs
    return d


def _zones_file(path):
    feats = [_feat(_SQUARE, parcel="A-1", owner={"name": "x"}), _feat(None, parcel="gone"), _feat(_PARTS, parcel="B-2", pixels="own", ha=1.5),
             {"type": "Feature", "properties": None, "geometry": _SQUARE}, _feat(_SQUARE, parcel="D-4")]
    path.write_text(json.dumps(_doc(feats, _CRS)))
    return feats


# hand-made tables of the 4 read zones, C = 4: a plain zone, a tie between classes 1 and 3 (and, under class_zero, one between 1 and 2 once
# class 0 is set aside), a zone whose only pixels are class 0, a zone without pixels
_COUNTS = np.array([[5, 1, 2, 0], [9, 4, 3, 4], [7, 0, 0, 0], [0, 0, 0, 0]], dtype=np.int64)
_OBJECTS = np.array([[1, 1, 2, 0], [2, 1, 1, 3], [1, 0, 0, 0], [0, 0, 0, 0]], dtype=np.int64)


def test_read_zones_keeps_properties_geometry_and_the_crs(tmp_path):
    ZN = _zn()
    from unet_amd import rasterize as RZ
    written = _zones_file(tmp_path / "z.geojson")
    rings, feats = ZN.read_zones(tmp_path / "z.geojson")
    assert len(feats) == 4 and rings.n_features == 4 and rings.values.tolist() == [0, 0, 0, 0]          # the null geometry is skipped
    assert [f["properties"] for f in feats] == [written[0]["properties"], written[2]["properties"], {}, written[4]["properties"]]
    assert [f["geometry"] for f in feats] == [_SQUARE, _PARTS, _SQUARE, _SQUARE]
    assert feats.crs == _CRS and ZN.epsg_of_crs(feats.crs) == 25832
    assert rings.feature_ring_start.tolist() == [0, 1, 4, 5, 6] and rings.ring_start.tolist() == [0, 4, 7, 11, 14, 18, 22]
    # the same rings as read_geojson on the same file with a burn attribute on every feature
    for f in written:
        f["properties"] = {"class": 0}
    (tmp_path / "b.geojson").write_text(json.dumps(_doc(written)))
    burn = RZ.read_geojson(tmp_path / "b.geojson")
    for k in ("xy", "ring_start", "feature_ring_start", "values"):
        assert torch.equal(getattr(rings, k), getattr(burn, k)), k
    # map coordinates
    moved = ZN.read_zones(tmp_path / "z.geojson", (100.0, 0.5, 0.0, 50.0, 0.0, -0.5))[0]
    assert moved.xy[:4].tolist() == [[-200 * 256, 100 * 256], [-200 * 256, 92 * 256], [-192 * 256, 92 * 256], [-192 * 256, 100 * 256]]
    for name, crs, want in (("short", {"type": "name", "properties": {"name": "EPSG:4326"}}, 4326), ("crs84", {"type": "name", "properties": {"name": "urn:ogc:def:crs:OGC:1.3:CRS84"}}, None),
                            ("none", None, None), ("odd", {"type": "link"}, None)):
        assert ZN.epsg_of_crs(crs) == want, name
    (tmp_path / "line.geojson").write_text(json.dumps(_doc([_feat({"type": "LineString", "coordinates": [[0, 0], [1, 1]]})])))
    with pytest.raises(ValueError, match="feature 0: geometry type 'LineString' is not supported"):
        ZN.read_zones(tmp_path / "line.geojson")
    (tmp_path / "n.geojson").write_text(json.dumps({"type": "Feature"}))
    with pytest.raises(ValueError, match="expected a GeoJSON FeatureCollection"):
        ZN.read_zones(tmp_path / "n.geojson")
    with pytest.raises(ValueError, match="rotation"):
        ZN.read_zones(tmp_path / "z.geojson", (0, 1, 0.1, 0, 0, -1))


@pytest.mark.parametrize("class_zero", [False, True])
@pytest.mark.parametrize("objects", [False, True])
def test_write_zonal_geojson(tmp_path, class_zero, objects):
    ZN = _zn()
    _zones_file(tmp_path / "z.geojson")
    _, feats = ZN.read_zones(tmp_path / "z.geojson")
    stats = ZN.ZonalStats(torch.from_numpy(_COUNTS), torch.from_numpy(_OBJECTS) if objects else None)
    assert ZN.write_zonal(tmp_path / "t.geojson", feats, stats, pixel_area=0.25, class_zero=class_zero) == 4
    doc = json.loads((tmp_path / "t.geojson").read_text())
    assert doc["type"] == "FeatureCollection" and doc["crs"] == _CRS and len(doc["features"]) == 4
    want = ZR.rows(_COUNTS, _OBJECTS if objects else None, None, 0.25, class_zero)
    for f, src, row in zip(doc["features"], feats, want):
        assert f["type"] == "Feature" and f["geometry"] == src["geometry"]
        assert f["properties"] == {**src["properties"], **row}
        assert list(f["properties"])[-len(row):] == list(row)                     # the added properties come behind the zone's own
    p = [f["properties"] for f in doc["features"]]
    assert p[0]["parcel"] == "A-1" and p[0]["owner"] == {"name": "x"} and p[1]["ha"] == 1.5 and "parcel" not in p[2]
    assert p[1]["pixels"] == 20                                                    # an added name replaces the zone's own property
    if class_zero:
        # ids shift by -1, class 0 is px_nodata, outside the denominators and the majority
        assert [q["majority"] for q in p] == [1, 0, None, None]                    # zone 1: classes 1 and 3 tie at 4 pixels -> the smaller, 1 - 1
        assert p[0]["px_nodata"] == 5 and p[0]["px_0"] == 1 and p[0]["frac_0"] == 1 / 3 and p[0]["frac_1"] == 2 / 3 and "frac_nodata" not in p[0]
        assert p[2]["pixels"] == 7 and p[2]["area"] == 1.75 and p[2]["frac_0"] is None and p[2]["px_nodata"] == 7
        assert ("n_nodata" not in p[0]) and (("n_0" in p[0]) == objects)
    else:
        assert [q["majority"] for q in p] == [0, 0, 0, None]
        assert p[1]["frac_1"] == 0.2 and p[1]["frac_3"] == 0.2 and p[2]["frac_0"] == 1.0 and p[0]["area"] == 2.0
        assert p[3]["pixels"] == 0 and p[3]["majority"] is None and all(p[3][f"frac_{c}"] is None for c in range(4)) and p[3]["px_2"] == 0
        if objects:
            assert [p[1][f"n_{c}"] for c in range(4)] == [2, 1, 1, 3]
    assert ("n_1" in p[0]) == objects


def test_write_zonal_names_classes_by_codes_and_takes_a_crs(tmp_path):
    ZN = _zn()
    _zones_file(tmp_path / "z.geojson")
    _, feats = ZN.read_zones(tmp_path / "z.geojson")
    stats = ZN.ZonalStats(torch.from_numpy(_COUNTS), torch.from_numpy(_OBJECTS))
    codes = ["NO_Data", "forest", "water", "sealed"]
    other = {"type": "name", "properties": {"name": "EPSG:31467"}}
    ZN.write_zonal(tmp_path / "t.geojson", feats, stats, codes=codes, class_zero=True, crs=other)
    doc = json.loads((tmp_path / "t.geojson").read_text())
    assert doc["crs"] == other
    p = doc["features"][0]["properties"]
    assert p["px_nodata"] == 5 and p["px_forest"] == 1 and p["frac_water"] == 2 / 3 and p["n_water"] == 2 and p["majority"] == 1
    assert [f["properties"] for f in doc["features"]] == [{**f["properties"], **r} for f, r in zip(feats, ZR.rows(_COUNTS, _OBJECTS, codes, 1.0, True))]
    with pytest.raises(ValueError, match="codes names 3 classes"):
        ZN.write_zonal(tmp_path / "t.geojson", feats, stats, codes=codes[:3])
    with pytest.raises(ValueError, match="4 zones, the features 3"):
        ZN.write_zonal(tmp_path / "t.geojson", feats[:3], stats)
    with pytest.raises(ValueError, match="geojson or .csv"):
        ZN.write_zonal(tmp_path / "t.shp", feats, stats)
    plain = ZN.ZoneFeatures(feats)
    ZN.write_zonal(tmp_path / "nocrs.geojson", plain, stats)
    assert "crs" not in json.loads((tmp_path / "nocrs.geojson").read_text())


@pytest.mark.parametrize("class_zero", [False, True])
def test_write_zonal_csv(tmp_path, class_zero):
    ZN = _zn()
    _zones_file(tmp_path / "z.geojson")
    _, feats = ZN.read_zones(tmp_path / "z.geojson")
    stats = ZN.ZonalStats(torch.from_numpy(_COUNTS), torch.from_numpy(_OBJECTS))
    assert ZN.write_zonal(tmp_path / "t.csv", feats, stats, pixel_area=4.0, class_zero=class_zero) == 4
    with open(tmp_path / "t.csv", newline="") as f:
        table = list(csv.reader(f))
    want = ZR.rows(_COUNTS, _OBJECTS, None, 4.0, class_zero)
    added = list(want[0])
    assert table[0] == ["parcel", "owner", "ha"] + added and len(table) == 5          # the zones' own properties first ("pixels" is an added name)
    assert [r[0] for r in table[1:]] == ["A-1", "B-2", "", "D-4"] and table[1][1] == '{"name": "x"}' and table[2][2] == "1.5" and table[1][2] == ""
    for line, row in zip(table[1:], want):
        assert line[3:] == ["" if row[k] is None else str(row[k]) for k in added]
    assert table[4][3:5] == ["0", "0.0"] and table[4][table[0].index("majority")] == ""          # the zone without pixels


def test_zonal_mask_refuses_another_epsg_before_anything_runs(tmp_path, monkeypatch):
    ZN = _zn()
    _zones_file(tmp_path / "z.geojson")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)          # the check under test comes before the first device call
    tags_31467 = {34735: [1, 1, 0, 1, 3072, 0, 1, 31467]}
    m = np.zeros((8, 8), dtype=np.uint8)
    with pytest.raises(ValueError, match="EPSG:25832, the raster in EPSG:31467"):
        ZN.zonal_mask(m, tmp_path / "z.geojson", tmp_path / "t.geojson", None, tags_31467)
    assert not (tmp_path / "t.geojson").exists()
    (tmp_path / "empty.geojson").write_text(json.dumps(_doc([_feat(None, a=1)])))
    with pytest.raises(ValueError, match="no Polygon or MultiPolygon zone"):
        ZN.zonal_mask(m, tmp_path / "empty.geojson", tmp_path / "t.geojson")


# ------------------------------------------------------------------------------------------------------------ the shared parser

def test_read_geojson_returns_what_it_returned_before_the_parser_was_shared(tmp_path):
    from unet_amd import rasterize as RZ
    with open(GOLDEN) as f:
        golden = json.load(f)
    seen = 0
    for tag, gt in (("pixel", None), ("map", ZC.GT)):
        for name, path in ZC.write_set_files(tmp_path, gt).items():
            for cz in (False, True):
                want = golden[f"{name}/{tag}/{'class_zero' if cz else 'plain'}"]
                assert "error" not in want
                got = RZ.read_geojson(path, gt, "class", cz)
                assert ZC.rings_as_lists(got) == want, (name, tag, cz)
                assert got.xy.dtype == torch.int32 and got.ring_start.dtype == torch.int64 and got.values.dtype == torch.uint8
                seen += 1
            # read_zones parses the same rings
            zones = _zn().read_zones(path, gt)[0]
            plain = golden[f"{name}/{tag}/plain"]
            assert ZC.rings_as_lists(zones) == {**plain, "values": [0] * len(plain["values"])}, (name, tag)
    assert seen == len(golden) == 32
    # and its error texts
    (tmp_path / "bad.geojson").write_text(json.dumps(_doc([_feat(_SQUARE, **{"class": 1}), _feat(_SQUARE, **{"class": 1.5})])))
    with pytest.raises(ValueError, match="feature 1: the attribute 'class' must be an integer, got 1.5"):
        RZ.read_geojson(tmp_path / "bad.geojson")
    (tmp_path / "ring.geojson").write_text(json.dumps(_doc([_feat({"type": "Polygon", "coordinates": [[[0, 0], [1], [2, 2]]]}, **{"class": 1})])))
    with pytest.raises(ValueError, match="feature 0: a ring is not a list of \\[x, y\\] positions"):
        RZ.read_geojson(tmp_path / "ring.geojson")
    (tmp_path / "pt.geojson").write_text(json.dumps(_doc([_feat({"type": "Point", "coordinates": [0, 0]}, **{"class": "x"})])))
    with pytest.raises(ValueError, match="feature 0: geometry type 'Point' is not supported"):          # the geometry is judged before the attribute
        RZ.read_geojson(tmp_path / "pt.geojson")


def test_reference_tables_on_a_hand_made_case():
    z = np.array([[0, 0, 1, -1], [1, 1, 1, 2], [-1, 2, 2, 2]], dtype=np.int32)
    m = np.array([[1, 1, 0, 1], [0, 0, 2, 2], [2, 2, 2, 1]], dtype=np.uint8)
    lab = np.array([[0, 0, 2, 3], [4, 4, 6, 6], [6, 6, 6, 11]], dtype=np.int32)
    c, bad = ZR.counts(z, m, 3, 3)
    assert c.tolist() == [[0, 2, 0], [3, 0, 1], [0, 1, 3]] and not bad
    assert ZR.objects(z, m, lab, 3, 3).tolist() == [[0, 1, 0], [2, 0, 1], [0, 1, 0]]          # the object of label 6 counts in zone 1, where its first pixel lies
    m[0, 0], z[2, 3] = 3, 3
    c, bad = ZR.counts(z, m, 3, 3)
    assert bad and c.tolist() == [[0, 1, 0], [3, 0, 1], [0, 0, 3]]
    assert ZR.counts(np.array([[-2]]), np.array([[0]]), 1, 1)[1]
