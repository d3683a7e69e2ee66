"""CPU suite of the ring simplification (unet_amd/vectorize.py): the plain-Python restatement of the rules
(tests/simplify_ref.py) against properties that do not go through it -- at tolerance 0 the rings of the tracer come back, at every tolerance
shared borders stay shared, the areas add up to the raster, every dropped candidate lies within the tolerance and every node stays -- and
the host-side entry points: quantisation, argument checks, the GeoJSON file of a simplified result."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import postprocess_ref as R  # noqa: E402
import simplify_ref as S  # noqa: E402
import vectorize_ref as V  # noqa: E402

TOLERANCES = (0, 0.5, 1, 2.5, 8)
# the (case, tolerance) pairs in which a hole outlives its exterior ring, computed with the reference: none among these cases.  Only
# pairs listed here may skip the balance check.
ORPHANS = []


def _vz():
    from unet_amd import vectorize
    return vectorize


def _special():
    nested = np.zeros((11, 11), dtype=np.uint8)
    for k in range(5):
        nested[k:11 - k, k:11 - k] = k % 2 + 1
    nested[5, 5] = 9
    pair = np.zeros((6, 7), dtype=np.uint8)
    pair[2, 2] = pair[3, 3] = 1
    tee = np.zeros((8, 9), dtype=np.uint8)
    tee[:4], tee[4:, :5], tee[4:, 5:] = 1, 2, 3
    return {"nested": nested, "pair": pair, "tee": tee}


def _cases():
    out = {}
    for shape in ((63, 64), (67, 131)):
        for name, m in R.patterns(*shape).items():
            out[f"{name}-{shape[0]}x{shape[1]}"] = m
    for i in range(16):
        out[f"2x2-{i}"] = np.array([[i & 1, i >> 1 & 1], [i >> 2 & 1, i >> 3 & 1]], dtype=np.uint8)
    out.update(_special())
    return out


CASES = _cases()
_PREP = {}


def _simplified(case, tol):
    if case not in _PREP:
        _PREP[case] = S.prepare(CASES[case])
    return S.simplify(CASES[case], tol, None, _PREP[case])


def _drop_collinear(ring):
    n = len(ring)
    keep = []
    for i, (x, y) in enumerate(ring):
        (ax, ay), (bx, by) = ring[i - 1], ring[(i + 1) % n]
        if (x - ax) * (by - y) - (y - ay) * (bx - x) != 0:
            keep.append((x, y))
    return keep


def test_the_orphan_list_is_a_minority():
    assert len(ORPHANS) * 2 < len(CASES) * len(TOLERANCES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_tolerance_zero_keeps_every_candidate_and_gives_back_the_traced_rings(case):
    m = CASES[case]
    H, W = m.shape
    s = _simplified(case, 0)
    plain = V.polygonize(m)
    assert s["dropped_rings"] == 0 and s["dropped_polygons"] == 0 and s["orphans"] == 0
    lists, traced = S.ring_lists(s), S.ring_lists(plain)
    assert lists == [[c[:2] for c in cand] for cand in s["cand"]]                       # every ring equals its candidate list
    is_node = S.node_map(R.label_components(m, 4).tolist(), H, W)
    for ring, old in zip(lists, traced):
        assert all(is_node(*v) for v in set(ring) - set(old))                           # what polygonize does not list is a node
        assert _drop_collinear(ring) == old                                             # and lies straight between its neighbours
    for name in ("ring_label", "ring_area", "poly_label", "poly_class", "poly_pixels", "poly_ring_start", "poly_rings"):
        assert np.array_equal(s[name], plain[name]) and s[name].dtype == plain[name].dtype, name
    assert s["raw_vertices"] == len(s["xy"]) >= len(plain["xy"])


@pytest.mark.parametrize("tol", TOLERANCES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_borders_stay_shared_areas_add_up_and_nothing_moves_further_than_the_tolerance(case, tol):
    m = CASES[case]
    H, W = m.shape
    s = _simplified(case, tol)
    q = S.quantise(tol)
    assert (s["orphans"] > 0) == ((case, tol) in ORPHANS)
    if (case, tol) not in ORPHANS:
        assert not S.unbalanced_segments(s, H, W)                # every segment off the frame occurs reversed exactly as often
        assert S.doubled_area_sum(s) == 2 * H * W                # so the signed areas of the rings sum to the raster
    lists = S.ring_lists(s)
    assert len(lists) == len(s["final"]) and all(len(r) >= 3 for r in lists)
    for j, (ring, i) in enumerate(zip(lists, s["final"])):
        cand = s["cand"][i]
        assert S.within_tolerance(cand, ring, q)                 # every candidate within the tolerance of the line that replaced it
        assert all(c[:2] in ring for c in cand if c[2])          # nodes are never removed
        assert S.half(S.area2(ring)) == int(s["ring_area"][j])
    # orders: rings by leader, polygons by label, the exterior first; the pixel counts are the true ones
    leaders = [s["leader"][i] for i in s["final"]]
    assert leaders == sorted(leaders) and s["poly_label"].tolist() == sorted(set(s["ring_label"].tolist()))
    plain = dict(zip(*np.unique(R.label_components(m, 4), return_counts=True)))
    assert s["poly_pixels"].tolist() == [plain[l] for l in s["poly_label"].tolist()]
    for p, l in enumerate(s["poly_label"].tolist()):
        rings = s["poly_rings"][s["poly_ring_start"][p]:s["poly_ring_start"][p + 1]].tolist()
        assert [s["ring_label"][r] for r in rings] == [l] * len(rings) and rings == sorted(rings) and leaders[rings[0]] == 4 * l


def test_a_larger_tolerance_keeps_fewer_vertices_on_the_long_arcs():
    for case in ("spiral-67x131", "noise2-67x131", "blocks-63x64"):
        counts = [len(_simplified(case, tol)["xy"]) for tol in TOLERANCES]
        assert counts[0] > counts[-1] and counts == sorted(counts, reverse=True), (case, counts)
    assert _simplified("spiral-67x131", 0)["depth"] > 100 and _simplified("spiral-67x131", 0)["wraps"] > 0


def test_quantisation_at_the_boundaries_of_q():
    VZ = _vz()
    for tol, q in ((0, 0), (0.03, 0), (0.04, 1), (0.71, 11), (0.72, 12), (0.75, 12), (1, 16), (2.5, 40), (4096, 65536)):
        assert S.quantise(tol) == q and VZ.check_simplify(tol) == q, tol
    island = np.zeros((3, 3), dtype=np.uint8)
    island[1, 1] = 1
    a, b = S.simplify(island, 0.71), S.simplify(island, 0.75)
    assert len(a["poly_label"]) == 2 and a["dropped_rings"] == 0                   # q = 11: 256 * 1 > 121 * 2
    assert len(b["poly_label"]) == 1 and b["dropped_rings"] == 2                   # q = 12: 256 * 1 <= 144 * 2, the island and its hole go together
    assert b["xy"].tolist() == [[0, 0], [0, 3], [3, 3], [3, 0]] and b["poly_pixels"].tolist() == [8] and b["ring_area"].tolist() == [9]
    assert S.kept(1, 2, 11) and not S.kept(1, 2, 12) and S.kept(2 ** 31 - 1, 2 ** 62, 65535) is (256 * (2 ** 31 - 1) ** 2 > 65535 ** 2 * 2 ** 62)


def test_check_vector_and_polygonize_refuse_bad_tolerances():
    VZ = _vz()
    assert VZ.check_vector("a.geojson", None, simplify=1.5) == () and VZ.check_vector(None) is None
    assert VZ.check_vector("a.geojson", 3, simplify=0) == (3,) and VZ.check_vector(True, None, class_zero=True, simplify=4096) == (0,)
    with pytest.raises(ValueError, match="without a vector output"):
        VZ.check_vector(None, None, simplify=1.0)
    with pytest.raises(ValueError, match="without a vector output"):
        VZ.check_vector(False, None, simplify=0)
    for bad in (float("nan"), float("inf"), "1", [1], True, -0.5, 4096.5, -1):
        with pytest.raises(ValueError, match="simplify"):
            VZ.check_vector("a.geojson", None, simplify=bad)
        with pytest.raises(ValueError, match="simplify"):
            VZ.polygonize(np.zeros((2, 2), dtype=np.uint8), simplify=bad)          # before anything touches the GPU
    import inspect

    import predict as P
    import params_and_main as M
    assert inspect.signature(P.predict_raster).parameters["vector_simplify"].default is None
    assert inspect.signature(P.save_predictions).parameters["vector_simplify"].default is None
    assert M.VECTOR_SIMPLIFY is None
    assert list(inspect.signature(VZ.polygonize).parameters) == ["mask", "exclude", "simplify", "stages"]


def test_geojson_of_a_simplified_result(tmp_path):
    VZ = _vz()
    s = _simplified("blocks-63x64", 1)
    gt = (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)
    n = VZ.write_geojson(tmp_path / "s.geojson", s, gt, 32632)
    doc = json.load(open(tmp_path / "s.geojson"))
    assert n == len(doc["features"]) == len(s["poly_label"]) < len(_simplified("blocks-63x64", 0)["poly_label"])
    lists = S.ring_lists(s)
    for p, f in enumerate(doc["features"]):
        rings = s["poly_rings"][s["poly_ring_start"][p]:s["poly_ring_start"][p + 1]].tolist()
        coords = f["geometry"]["coordinates"]
        assert len(coords) == len(rings) and f["properties"]["pixels"] == int(s["poly_pixels"][p])
        for ring, r in zip(coords, rings):
            assert ring[0] == ring[-1] and len(ring) == len(lists[r]) + 1 >= 4
            assert [[int(round((x - gt[0]) / gt[1])), int(round((y - gt[3]) / gt[5]))] for x, y in ring[:-1]] == [list(v) for v in lists[r]]
