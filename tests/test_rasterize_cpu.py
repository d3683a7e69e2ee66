"""CPU suite of the rasterizer (unet_amd/rasterize.py): the plain-Python restatement of the burning rules (tests/rasterize_ref.py) held
against the sequential tracer (tests/vectorize_ref.py) as its inverse, the GeoJSON reader against write_geojson and against files written by
hand, and every limit and argument error -- all raised with no GPU present."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import rasterize_cases as RC  # noqa: E402
import rasterize_ref as RR  # noqa: E402
import vectorize_ref as V  # noqa: E402

GT = (500000.0, 0.25, 0.0, 5600000.0, 0.0, -0.25)          # every product and quotient below is exact in float64


def _rz():
    from unet_amd import rasterize
    return rasterize


def _vz():
    from unet_amd import vectorize
    return vectorize


def _host_polygons(p: dict):
    VZ = _vz()
    return VZ.Polygons(**{k: torch.from_numpy(np.ascontiguousarray(p[k])) for k in V.ARRAYS})


def _round_trip(m, exclude=None, fill=0):
    p = V.polygonize(m, exclude)
    return RR.rasterize(*RR.rings_of_polygons(p), m.shape, fill)


# ------------------------------------------------------------------------------------------------------------ the reference round trip

@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_reference_round_trip_on_random_masks(seed):
    m = RC.mask(23, 31, seed)
    assert len(np.unique(m)) == 5
    assert np.array_equal(_round_trip(m), m)


def test_reference_round_trip_on_saddles_and_holes():
    frame = np.ones((3, 3), dtype=np.uint8)
    frame[1, 1] = 0                                                   # a frame with one hole
    two_holes = np.ones((4, 4), dtype=np.uint8)
    two_holes[1, 1] = two_holes[2, 2] = 0                             # hole pixels that touch diagonally: a saddle, two holes
    diagonal = np.zeros((4, 4), dtype=np.uint8)
    diagonal[1, 1] = diagonal[2, 2] = 7                               # two diagonal pixels of one class inside another
    l_shape = np.array([[1, 0], [1, 1]], dtype=np.uint8)
    nested = np.zeros((11, 11), dtype=np.uint8)
    for k in range(5):
        nested[k:11 - k, k:11 - k] = k % 2 + 1                        # holes inside islands inside holes
    nested[5, 5] = 9
    for m in (frame, two_holes, diagonal, l_shape, nested, np.array([[3]], dtype=np.uint8)):
        assert np.array_equal(_round_trip(m), m)
    assert V.trace(two_holes)[1]["swaps"] == 1
    for i in range(16):
        m = np.array([[i & 1, i >> 1 & 1], [i >> 2 & 1, i >> 3 & 1]], dtype=np.uint8)
        assert np.array_equal(_round_trip(m), m)


def test_reference_round_trip_with_excluded_classes_leaves_the_fill():
    m = RC.mask(23, 31, 5)
    want = m.copy()
    want[(m == 0) | (m == 3)] = 7
    assert np.array_equal(_round_trip(m, (0, 3), fill=7), want)


def test_reference_tie_rules_and_partition():
    # a centre exactly on the left or top border is inside, exactly on the right or bottom border outside
    box = [(2 * 256 + 128, 1 * 256 + 128), (2 * 256 + 128, 4 * 256 + 128), (5 * 256 + 128, 4 * 256 + 128), (5 * 256 + 128, 1 * 256 + 128)]
    got = RR.feature_mask([box], 6, 8)
    want = np.zeros((6, 8), dtype=bool)
    want[1:4, 2:5] = True
    assert np.array_equal(got, want)
    for s in (1, 3):
        a, b = RC.oblique_halves(s)
        A, B = RR.feature_mask([a], 64, 64), RR.feature_mask([b], 64, 64)
        assert (A ^ B).all() and A.any() and B.any()


def test_rings_from_polygons_equals_the_reference_packing():
    RZ = _rz()
    m = RC.mask(23, 31, 2)
    p = V.polygonize(m)
    r = RZ.rings_from_polygons(_host_polygons(p))
    xy, rs, frs, vals = RR.rings_of_polygons(p)
    assert r.xy.dtype == torch.int32 and r.ring_start.dtype == torch.int64 and r.feature_ring_start.dtype == torch.int64 and r.values.dtype == torch.uint8
    assert np.array_equal(r.xy.numpy(), xy) and np.array_equal(r.ring_start.numpy(), rs)
    assert np.array_equal(r.feature_ring_start.numpy(), frs) and np.array_equal(r.values.numpy(), vals)
    assert (np.diff(p["poly_rings"]) != 1).any()                      # the indirection is not the identity here
    other = np.arange(len(vals), dtype=np.uint8)[::-1].copy()
    assert np.array_equal(RZ.rings_from_polygons(_host_polygons(p), other).values.numpy(), other)
    with pytest.raises(ValueError):
        RZ.rings_from_polygons(_host_polygons(p), other[:-1])
    with pytest.raises(ValueError):
        RZ.rings_from_polygons(_host_polygons(p), other.astype(np.int32))
    RZ.check_rings(r)


# ------------------------------------------------------------------------------------------------------------ read_geojson

def _same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("xy", "ring_start", "feature_ring_start", "values"))


@pytest.mark.parametrize("gt", [None, GT])
def test_a_file_of_write_geojson_reads_back_to_the_same_rings(tmp_path, gt):
    RZ, VZ = _rz(), _vz()
    m = RC.mask(23, 31, 1)
    p = V.polygonize(m)
    VZ.write_geojson(tmp_path / "a.geojson", p, gt)
    want = RZ.rings_from_polygons(_host_polygons(p))
    got = RZ.read_geojson(tmp_path / "a.geojson", gt)
    assert _same(got, want)
    assert not got.xy.is_cuda
    assert np.array_equal(RR.rasterize(got.xy.numpy(), got.ring_start.numpy(), got.feature_ring_start.numpy(), got.values.numpy(), m.shape), m)


def test_class_zero_is_the_inverse_of_write_geojson(tmp_path):
    RZ, VZ = _rz(), _vz()
    m = RC.mask(23, 31, 3)
    p = V.polygonize(m)
    VZ.write_geojson(tmp_path / "z.geojson", p, GT, class_zero=True)
    got = RZ.read_geojson(tmp_path / "z.geojson", GT, class_zero=True)
    back = RR.rasterize(got.xy.numpy(), got.ring_start.numpy(), got.feature_ring_start.numpy(), got.values.numpy(), m.shape, fill=0)
    assert np.array_equal(back, m)                                   # class 0 has no feature: it comes back as the fill
    assert 0 not in got.values.tolist() and (m == 0).any()
    plain = RZ.read_geojson(tmp_path / "z.geojson", GT)
    assert torch.equal(plain.values + 1, got.values)


def _write(path, features):
    path.write_text(json.dumps({"type": "FeatureCollection", "features": features}))
    return path


def _feat(geometry, **props):
    return {"type": "Feature", "properties": props, "geometry": geometry}


def test_multipolygon_null_geometry_and_the_closing_point(tmp_path):
    RZ = _rz()
    sq = lambda x, y, s: [[x, y], [x, y + s], [x + s, y + s], [x + s, y], [x, y]]          # noqa: E731
    open_ring = [[20, 1], [20, 5.5], [24.25, 5.5]]                                       # not closed: closed implicitly
    f = [_feat({"type": "Polygon", "coordinates": [sq(1, 1, 8), sq(3, 3, 2)]}, **{"class": 4}),
         _feat(None, **{"class": 9}),
         _feat({"type": "MultiPolygon", "coordinates": [[sq(10, 1, 4)], [sq(10, 8, 5), sq(11, 9, 1)], [open_ring]]}, **{"class": 200.0}),
         {"type": "Feature", "properties": {"class": 1}}]
    r = RZ.read_geojson(_write(tmp_path / "m.geojson", f))
    assert r.values.tolist() == [4, 200]
    assert r.feature_ring_start.tolist() == [0, 2, 6]
    assert r.ring_start.tolist() == [0, 4, 8, 12, 16, 20, 23]                            # every closing point dropped, the open ring kept whole
    assert r.xy[:4].tolist() == [[256, 256], [256, 9 * 256], [9 * 256, 9 * 256], [9 * 256, 256]]
    assert r.xy[20:].tolist() == [[20 * 256, 256], [20 * 256, 5 * 256 + 128], [24 * 256 + 64, 5 * 256 + 128]]
    got = RR.rasterize(r.xy.numpy(), r.ring_start.numpy(), r.feature_ring_start.numpy(), r.values.numpy(), (16, 30))
    assert got[2, 2] == 4 and got[3, 3] == 0 and got[9, 9] == 0 and got[2, 11] == 200 and got[9, 11] == 0 and got[12, 14] == 200
    # quantisation: floor(256 x + 0.5)
    r = RZ.read_geojson(_write(tmp_path / "q.geojson", [_feat({"type": "Polygon", "coordinates": [[[0.001, -0.002], [3.998, 0.0], [1.0, 2.5]]]}, **{"class": 1})]))
    assert r.xy.tolist() == [[0, -1], [1023, 0], [256, 640]]
    # with a geotransform the map coordinates become pixel coordinates first
    ring = [[GT[0] + x * GT[1], GT[3] + y * GT[5]] for x, y in ((1, 1), (1, 3), (2.5, 3))]
    r = RZ.read_geojson(_write(tmp_path / "g.geojson", [_feat({"type": "Polygon", "coordinates": [ring]}, k=7)]), GT, attribute="k")
    assert r.xy.tolist() == [[256, 256], [256, 768], [640, 768]] and r.values.tolist() == [7]
    empty = RZ.read_geojson(_write(tmp_path / "e.geojson", []))
    assert empty.n_features == 0 and empty.n_rings == 0 and empty.n_vertices == 0 and empty.xy.shape == (0, 2)


def test_read_geojson_raises_value_errors(tmp_path):
    RZ = _rz()
    tri = {"type": "Polygon", "coordinates": [[[0, 0], [0, 4], [4, 4]]]}
    bad = {
        "line": [_feat(tri, **{"class": 1}), _feat({"type": "LineString", "coordinates": [[0, 0], [1, 1]]}, **{"class": 1})],
        "point": [_feat({"type": "Point", "coordinates": [0, 0]}, **{"class": 1})],
        "missing": [_feat(tri, other=1)],
        "no_props": [{"type": "Feature", "properties": None, "geometry": tri}],
        "text": [_feat(tri, **{"class": "1"})],
        "fraction": [_feat(tri, **{"class": 1.5})],
        "bool": [_feat(tri, **{"class": True})],
        "negative": [_feat(tri, **{"class": -1})],
        "big": [_feat(tri, **{"class": 256})],
        "far": [_feat({"type": "Polygon", "coordinates": [[[0, 0], [0, 4], [2 ** 21 + 1, 4]]]}, **{"class": 1})],
        "position": [_feat({"type": "Polygon", "coordinates": [[[0, 0], [0], [4, 4]]]}, **{"class": 1})],
    }
    for name, feats in bad.items():
        with pytest.raises(ValueError) as e:
            RZ.read_geojson(_write(tmp_path / f"{name}.geojson", feats))
        if name == "line":
            assert "feature 1" in str(e.value) and "LineString" in str(e.value)
    with pytest.raises(ValueError):
        RZ.read_geojson(_write(tmp_path / "z.geojson", [_feat(tri, **{"class": 255})]), class_zero=True)          # 0..254 under class_zero
    assert RZ.read_geojson(_write(tmp_path / "z.geojson", [_feat(tri, **{"class": 254})]), class_zero=True).values.tolist() == [255]
    assert RZ.read_geojson(_write(tmp_path / "ok.geojson", [_feat({"type": "Polygon", "coordinates": [[[0, 0], [0, 4], [2 ** 21, -2 ** 21]]]}, **{"class": 0})])
                           ).xy[2].tolist() == [2 ** 29, -2 ** 29]
    (tmp_path / "n.geojson").write_text(json.dumps({"type": "Feature"}))
    with pytest.raises(ValueError):
        RZ.read_geojson(tmp_path / "n.geojson")
    for gt in ((0, 1, 0.5, 0, 0, -1), (0, 1, 0, 0, 0.5, -1), (0, 0, 0, 0, 0, -1), (0, 1, 0, 0, 0)):          # rotation, zero pixel size, five numbers
        with pytest.raises(ValueError):
            RZ.read_geojson(tmp_path / "ok.geojson", gt)


# ------------------------------------------------------------------------------------------------------------ limits and arguments

def _rings(xy, rs, frs, vals):
    RZ = _rz()
    return RZ.Rings(torch.tensor(xy, dtype=torch.int32).reshape(-1, 2), torch.tensor(rs, dtype=torch.int64), torch.tensor(frs, dtype=torch.int64),
                    torch.tensor(vals, dtype=torch.uint8))


def test_limits_and_arguments_are_refused_before_the_gpu():
    RZ = _rz()
    ok = _rings([[0, 0], [0, 512], [512, 512]], [0, 3], [0, 1], [5])
    for shape in ((0, 4), (4, 0), (2 ** 20, 4), (4, 2 ** 20), (4,), (4, 4, 4), (4.0, 4), "ab", 16, (True, 4)):
        with pytest.raises(ValueError):
            RZ.rasterize(ok, shape)
    for fill in (-1, 256, 1.5, True, None):
        with pytest.raises(ValueError):
            RZ.rasterize(ok, (4, 4), fill=fill)
    far = 2 ** 29 + 1
    bad = [
        _rings([[0, 0], [0, 512], [far, 512]], [0, 3], [0, 1], [5]),            # |x| > 2^21 pixels
        _rings([[0, -far], [0, 512], [512, 512]], [0, 3], [0, 1], [5]),
        _rings([[0, 0], [0, 512], [512, 512]], [0, 4], [0, 1], [5]),            # ring_start beyond the vertices
        _rings([[0, 0], [0, 512], [512, 512]], [1, 3], [0, 1], [5]),
        _rings([[0, 0], [0, 512], [512, 512]], [0, 3, 2, 3], [0, 3], [5]),      # falling
        _rings([[0, 0], [0, 512], [512, 512]], [0, 3], [0, 2], [5]),            # feature_ring_start beyond the rings
        _rings([[0, 0], [0, 512], [512, 512]], [0, 3], [0, 1, 1], [5]),         # one value for two features
    ]
    bad.append(RZ.Rings(ok.xy.to(torch.int64), ok.ring_start, ok.feature_ring_start, ok.values))
    bad.append(RZ.Rings(ok.xy, ok.ring_start.to(torch.int32), ok.feature_ring_start, ok.values))
    bad.append(RZ.Rings(ok.xy, ok.ring_start, ok.feature_ring_start, ok.values.to(torch.int32)))
    bad.append(RZ.Rings(ok.xy.reshape(-1), ok.ring_start, ok.feature_ring_start, ok.values))
    F = 2 ** 23
    bad.append(RZ.Rings(ok.xy, ok.ring_start, torch.ones(F + 1, dtype=torch.int64), torch.zeros(F, dtype=torch.uint8)))          # 2^23 features
    for r in bad + [None, "rings", {"xy": ok.xy}]:
        with pytest.raises(ValueError):
            RZ.rasterize(r, (4, 4))
    RZ.check_rings(_rings([[2 ** 29, -2 ** 29], [0, 512], [512, 512]], [0, 3], [0, 1], [5]))          # the limit itself is allowed
    with pytest.raises(ValueError):
        RZ.quantise(np.array([2.0 ** 21 + 0.01]))
    with pytest.raises(ValueError):
        RZ.quantise(np.array([np.nan]))
    assert RZ.quantise(np.array([-0.5 / 256, 0.49 / 256, 0.5 / 256, 2.0 ** 21])).tolist() == [0, 0, 1, 2 ** 29]
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="no device"):
            RZ.rasterize(ok, (4, 4))                                             # no host fallback
    for word in ("ALL_TOUCHED", "Lines and points".lower(), "non-zero winding", "regression masks", "Shapefile", "reprojection", "host fallback"):
        assert word in RZ.__doc__, word


def test_split_raster_refuses_a_vector_mask_without_a_device(tmp_path, monkeypatch):
    import create_tiles_unet as T
    from unet_amd.tiffio import write_tiff
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    write_tiff(tmp_path / "img.tif", np.ones((3, 64, 64), dtype=np.uint8), geotransform=GT)
    _write(tmp_path / "labels.geojson", [])
    with pytest.raises(ValueError, match="GPU"):
        T.split_raster(tmp_path / "img.tif", tmp_path / "labels.geojson", tmp_path / "cut", patch_size=32, patch_overlap=0, split=[1])
    assert not (tmp_path / "cut").exists()


def test_params_and_main_passes_the_mask_attribute(monkeypatch):
    import create_tiles_unet
    import params_and_main as M
    assert M.MASK_ATTRIBUTE == "class"
    calls = {}
    monkeypatch.setattr(create_tiles_unet, "split_raster", lambda **kw: calls.update(kw))
    monkeypatch.setattr(M, "Create_tiles", True); monkeypatch.setattr(M, "Train", False); monkeypatch.setattr(M, "Predict", False)
    monkeypatch.setattr(M, "MASK_ATTRIBUTE", "landuse")
    M.main()
    assert calls["mask_attribute"] == "landuse"


# ------------------------------------------------------------------------------------------------------------ C ABI

NEW_SYMBOLS = ("unet_ras_count", "unet_ras_scan_words", "unet_ras_scan", "unet_ras_emit", "unet_ras_spans", "unet_ras_resolve")


def test_header_declares_and_library_exports_the_new_symbols():
    from unet_amd import _lib as L
    declared = L.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L.lib, s) and s in L._sig, s
    assert "#define UNET_ABI_VERSION 8" in L.HEADER.read_text()
    assert L.lib.unet_ras_scan_words(1) == 1 and L.lib.unet_ras_scan_words(2048) == 1 and L.lib.unet_ras_scan_words(2049) == 2


def test_bad_arguments_return_minus_one_without_a_launch():
    from unet_amd import _lib as L
    lib = L.lib
    p = 4096          # a non-null, aligned address that is never dereferenced: every call below fails its host check
    big = 2 ** 31
    side = 2 ** 20
    calls = [
        lambda: lib.unet_ras_count(None, p, p, 4, 1, 4, p, p, None),
        lambda: lib.unet_ras_count(p, p, p, 0, 1, 4, p, p, None),
        lambda: lib.unet_ras_count(p, p, p, big, 1, 4, p, p, None),
        lambda: lib.unet_ras_count(p, p, p, 4, 0, 4, p, p, None),
        lambda: lib.unet_ras_count(p, p, p, 4, 1, side, p, p, None),
        lambda: lib.unet_ras_count(p + 4, p, p, 4, 1, 4, p, p, None),          # xy not 8-byte aligned
        lambda: lib.unet_ras_scan(p, 0, p, p, p, None),
        lambda: lib.unet_ras_scan(p, big, p, p, p, None),
        lambda: lib.unet_ras_scan(p, 4, p, None, p, None),
        lambda: lib.unet_ras_emit(p, p, p, p, 4, 1, 4, side, p, 2, p, None),
        lambda: lib.unet_ras_emit(p, p, p, p, 4, 1, 4, 4, p, 0, p, None),
        lambda: lib.unet_ras_emit(p, p, p, None, 4, 1, 4, 4, p, 2, p, None),
        lambda: lib.unet_ras_spans(p, 3, p, 1, 4, 4, p, p, None),                # an odd number of crossings
        lambda: lib.unet_ras_spans(p, big, p, 1, 4, 4, p, p, None),
        lambda: lib.unet_ras_spans(p, 2, p, 2 ** 23, 4, 4, p, p, None),
        lambda: lib.unet_ras_spans(p, 2, p, 0, 4, 4, p, p, None),
        lambda: lib.unet_ras_spans(p + 8, 2, p, 1, 4, 4, p, p, None),            # keys not 16-byte aligned
        lambda: lib.unet_ras_spans(None, 2, p, 1, 4, 4, p, p, None),
        lambda: lib.unet_ras_spans(p, 2, p, 1, 0, 4, p, p, None),
        lambda: lib.unet_ras_resolve(p, 4, side, 0, 0, p, None),
        lambda: lib.unet_ras_resolve(p, 4, 4, 256, 0, p, None),
        lambda: lib.unet_ras_resolve(p, 4, 4, 0, 0, None, None),
    ]
    for i, c in enumerate(calls):
        assert c() == -1, i
        assert lib.unet_last_error(), i
