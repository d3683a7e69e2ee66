"""CPU suite of the instance split (unet_amd/instances.py): the sequential restatement of the rules (tests/instances_ref.py) against a
brute-force distance and the properties the rules promise, the facts pinned while the rules were written, the integer form of the
shallow test against exact rational arithmetic, and every argument error of the module and of the prediction entry points -- all with
no GPU present."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import instances_ref as I  # noqa: E402


def _inst():
    from unet_amd import instances
    return instances


def _connected(sel: np.ndarray) -> bool:
    return len(np.unique(I.flood(sel.astype(np.int64))[sel])) == 1


# ------------------------------------------------------------------------------------------------------------ restatement against brute force

@pytest.mark.parametrize("seed, shape, classes, R, depth", [(0, (24, 31), [1, 2], 5, 1.0), (1, (17, 23), [0], 3, 0.0), (2, (9, 30), [2], 64, 2.0),
                                                            (3, (24, 31), [0, 1, 2], 2, 0.5), (4, (1, 19), [1], 4, 1.0), (5, (21, 1), [0, 1], 4, 0.0)])
def test_restatement_has_the_promised_properties(seed, shape, classes, R, depth):
    rng = np.random.default_rng(seed)
    m = I.blobs(*shape, seed=seed, sigma=1.5) if min(shape) > 1 else rng.integers(0, 3, shape).astype(np.uint8)
    h = I.heights(m, classes, R)
    assert np.array_equal(h, I.heights_brute(m, classes, R))                      # the distance is the O(n^2) minimum over all pixels
    assert h.max() <= R * R and (h[~np.isin(m, classes)] == 0).all() and (h[np.isin(m, classes)] >= 1).all()
    labels, info = I.split(m, classes, R, depth)
    comp = I.components(m)
    index = np.arange(m.size).reshape(m.shape)
    for l in np.unique(labels):
        sel = labels == l
        assert _connected(sel) and len(np.unique(m[sel])) == 1 and index[sel].min() == l          # 4-connected, one class, smallest index
        assert len(np.unique(comp[sel])) == 1                                     # the partition refines the components
    off = ~np.isin(m, classes)
    assert np.array_equal(labels[off], comp[off])                                 # classes not split: exactly the component labels
    assert info["segments"] == len(np.unique(labels)) and info["rounds"] == len(info["merged"]) >= 1
    assert info["seeds"] - sum(info["merged"]) == info["segments"]
    plain, pinfo = I.split(m, classes, R, 0.0)
    assert pinfo["segments"] == pinfo["seeds"] == info["seeds"] and pinfo["merged"] == [0]          # q = 0: the plain watershed
    capped, cinfo = I.split(m, classes, R, depth, max_rounds=1)
    assert cinfo["rounds"] == 1 and cinfo["segments"] == info["seeds"] - info["merged"][0]


# ------------------------------------------------------------------------------------------------------------ pinned facts

def _instances_of(m, R, depth):
    labels, _ = I.split(m, 1, R, depth)
    return len(np.unique(labels[m == 1]))


def test_two_and_three_touching_discs():
    two = I.discs(40, 48, [(20, 16), (20, 31)])
    assert [_instances_of(two, 64, d) for d in (0, 1, 2, 3, 4, 8)] == [2, 2, 2, 1, 1, 1]
    three = I.discs(40, 60, [(20, 14), (20, 29), (20, 44)])
    assert _instances_of(three, 64, 2) == 3 and _instances_of(three, 64, 3) == 1


def test_a_square_is_one_instance_with_and_without_a_capped_plateau():
    m = np.zeros((30, 30), dtype=np.uint8)
    m[3:27, 3:27] = 1
    assert _instances_of(m, 4, 2.0) == 1 and _instances_of(m, 64, 2.0) == 1
    assert I.heights(m, [1], 4).max() == 16 and (I.heights(m, [1], 4) == 16).sum() == 18 * 18          # the plateau of the cap


# ------------------------------------------------------------------------------------------------------------ the shallow test

def _sqrt_less(peak: int, pas: int, q: int) -> bool:
    """sqrt(peak) - sqrt(pas) < q / 16 in exact rationals: both sides of sqrt(peak) < q / 16 + sqrt(pas) are >= 0, so squaring twice keeps
    the order as long as the sign of what is squared is looked at"""
    a = Fraction(peak) - Fraction(q * q, 256) - pas          # sqrt(peak) < t + sqrt(pas)  <=>  peak - t^2 - pas < 2 t sqrt(pas)
    t = Fraction(q, 16)
    if a < 0:
        return True
    return a * a < 4 * t * t * pas


def test_shallow_equals_the_square_roots_exactly():
    import math
    for q in (0, 1, 32, 33, 4080):
        assert q == I.quantise(q / 16)
        for peak in range(0, 401):
            for pas in range(0, peak + 1):
                want = _sqrt_less(peak, pas, q)
                assert I.shallow(peak, pas, q) == want, (peak, pas, q)
                gap = math.sqrt(peak) - math.sqrt(pas) - q / 16          # float square roots agree wherever they are not at a tie
                if abs(gap) > 1e-9:
                    assert want == (gap < 0), (peak, pas, q)
        assert not I.shallow(7, 7, 0) and (q == 0 or I.shallow(7, 7, q))
    assert I.quantise(2.0) == 32 and I.quantise(0.03) == 0 and I.quantise(0.04) == 1 and I.quantise(255) == 4080


# ------------------------------------------------------------------------------------------------------------ argument errors and seams

def test_split_instances_refuses_bad_arguments_before_the_gpu():
    IN = _inst()
    m = np.zeros((4, 4), dtype=np.uint8)
    for bad in (np.zeros((4, 4), dtype=np.int32), np.zeros((2, 4, 4), dtype=np.uint8), np.zeros((0, 4), dtype=np.uint8), [[0]],
                torch.zeros((4, 4), dtype=torch.int64), np.broadcast_to(np.uint8(0), (65536, 32768))):
        with pytest.raises(ValueError):
            IN.split_instances(bad, 1)
    for bad in (None, -1, 256, 1.5, [0, 300], "ab", True, [None], []):
        with pytest.raises(ValueError):
            IN.split_instances(m, bad)
    for kw in (dict(radius=0), dict(radius=256), dict(radius=2.0), dict(radius=True), dict(min_depth=-1), dict(min_depth=256), dict(min_depth="2"),
               dict(min_depth=float("nan")), dict(min_depth=True), dict(max_rounds=0), dict(max_rounds=1.5)):
        with pytest.raises(ValueError):
            IN.split_instances(m, 1, **kw)
        with pytest.raises(ValueError):
            IN.Instances(1, **kw)
    assert IN.check_split(64, 2.0, 64) == (64, 32, 64) and IN.check_classes([3, 1, 3]) == (1, 3) and IN.check_classes(np.int64(2)) == (2,)
    for word in ("markers", "8-connected", "smoothing", "skimage.segmentation.watershed"):
        assert word in IN.__doc__, word


def test_check_instances():
    IN = _inst()
    from predict import check_outputs
    assert check_outputs(instances=None, regression=True, merge=False).instances is None          # None is never refused
    assert IN.check_instances(None) is None
    got = IN.check_instances({"classes": [2, 1], "radius": 16})
    assert isinstance(got, IN.Instances) and (got.classes, got.radius, got.min_depth, got.max_rounds) == ((1, 2), 16, 2.0, 64)
    same = IN.Instances(2)
    assert IN.check_instances(same) is same
    for bad in ({"classes": 1, "depth": 2}, {}, {"classes": 300}, [1], 1, "trees"):
        with pytest.raises(ValueError):
            IN.check_instances(bad)
    assert check_outputs(instances=same, instances_raster=True).instances is same
    for kw in (dict(regression=True), dict(all_classes=True), dict(specific_class=0), dict(large_file=True), dict(merge=False),
               dict(instances_raster=False)):          # the last: no output
        with pytest.raises(ValueError):
            check_outputs(**dict(dict(instances=same, instances_raster=True), **kw))


def test_polygonize_refuses_bad_labels_before_the_gpu():
    from unet_amd import vectorize as VZ
    m = torch.zeros((4, 4), dtype=torch.uint8)
    for bad in (np.zeros((4, 4), dtype=np.int32), torch.zeros((4, 4), dtype=torch.int32), torch.zeros((4, 4), dtype=torch.int64), "x"):
        with pytest.raises(ValueError):
            VZ.check_labels(bad, m)          # not an int32 tensor on the GPU
    with pytest.raises(ValueError):
        VZ.check_labels(None, m)
    for bad in (-1, 256, 1.5, "ab", True):
        with pytest.raises(ValueError):
            VZ.polygonize_labels(m, torch.zeros((4, 4), dtype=torch.int32), exclude=bad)          # before anything touches the GPU
    with pytest.raises(ValueError, match="simplify"):
        VZ.polygonize_labels(m, torch.zeros((4, 4), dtype=torch.int32), simplify=-1)
    import inspect
    assert list(inspect.signature(VZ.polygonize_labels).parameters) == ["mask", "labels", "exclude", "simplify", "stages"]
    assert "smallest linear index" in " ".join(VZ.polygonize_labels.__doc__.split())


def test_entry_points_refuse_combinations_before_the_model_loads(tmp_path):
    import predict as P
    raster = np.zeros((3, 64, 64), dtype=np.uint8)
    out, ras = tmp_path / "v.geojson", tmp_path / "i.tif"
    inst = {"classes": 1}
    for kw in (dict(regression=True), dict(all_classes=True), dict(specific_class=1), dict(large_file=True)):
        with pytest.raises(ValueError):
            P.predict_raster(None, raster, 32, instances=inst, instances_path=ras, **kw)          # model None: nothing but the checks can run
    for kw in (dict(instances=inst), dict(instances_path=ras), dict(instances={"classes": 1, "radius": 0}, vector_path=out),
               dict(instances={"class": 1}, instances_path=ras), dict(instances=[1], instances_path=ras)):
        with pytest.raises(ValueError):
            P.predict_raster(None, raster, 32, **kw)          # no output; a raster without the split; bad arguments
    missing = tmp_path / "no_such_model.pkl"
    for kw in (dict(regression=True), dict(all_classes=True), dict(specific_class=1), dict(large_file=True), dict(merge=False)):
        kw = dict(dict(regression=False, merge=True), **kw)
        regression = kw.pop("regression")
        with pytest.raises(ValueError):
            P.save_predictions(missing, tmp_path, regression, instances=inst, instances_raster=True, **kw)
    for kw in (dict(instances=inst), dict(instances_raster=True), dict(instances={"classes": 1, "min_depth": -2}, vector=True)):
        with pytest.raises(ValueError):
            P.save_predictions(missing, tmp_path, False, merge=True, **kw)
    assert not out.exists() and not ras.exists()


def test_params_and_main_passes_instances_only_when_set(monkeypatch):
    import create_tiles_unet
    import params_and_main as M
    import predict
    import train
    assert M.INSTANCES is None and M.INSTANCES_RASTER is False
    calls = {}
    monkeypatch.setattr(create_tiles_unet, "split_raster", lambda **kw: None)
    monkeypatch.setattr(train, "train_func", lambda *a: None)
    monkeypatch.setattr(predict, "save_predictions", lambda *a, **k: calls.setdefault("predict", (a, k)))
    monkeypatch.setattr(M, "Create_tiles", False); monkeypatch.setattr(M, "Train", False); monkeypatch.setattr(M, "Predict", True)
    monkeypatch.setattr(M, "enable_extra_parameters", True)
    M.main()
    assert calls.pop("predict")[1] == {"tta": None}
    monkeypatch.setattr(M, "INSTANCES", {"classes": [2]}); monkeypatch.setattr(M, "INSTANCES_RASTER", True)
    M.main()
    assert calls.pop("predict")[1] == {"tta": None, "instances": {"classes": [2]}, "instances_raster": True}
    monkeypatch.setattr(M, "enable_extra_parameters", False)
    M.main()
    assert calls.pop("predict")[1] == {"tta": None} and M.INSTANCES is None and M.INSTANCES_RASTER is False


def test_geojson_instance_property(tmp_path):
    import json
    import vectorize_ref as V
    from unet_amd import vectorize as VZ
    m = np.array([[1, 1, 0], [1, 2, 2]], dtype=np.uint8)
    polys = V.polygonize(m)
    VZ.write_geojson(tmp_path / "a.json", polys)
    VZ.write_geojson(tmp_path / "b.json", polys, instance=np.array([1, 0, 2]))
    a, b = json.load(open(tmp_path / "a.json")), json.load(open(tmp_path / "b.json"))
    assert all("instance" not in f["properties"] for f in a["features"])
    assert [f["properties"]["instance"] for f in b["features"]] == [1, 0, 2]
    assert [list(f["properties"])[-1] for f in b["features"]] == ["instance"] * 3          # behind the other properties
    for f in b["features"]:
        del f["properties"]["instance"]
    assert a == b
    with pytest.raises(ValueError):
        VZ.write_geojson(tmp_path / "c.json", polys, instance=[1, 2])


# ------------------------------------------------------------------------------------------------------------ C ABI

NEW_SYMBOLS = ("unet_cc_label_keys", "unet_inst_tile_shapes", "unet_inst_partials", "unet_inst_distance", "unet_inst_check_labels", "unet_inst_ascent",
               "unet_inst_ptr_rounds", "unet_inst_gather", "unet_inst_merge_round", "unet_inst_canonical", "unet_inst_marks", "unet_inst_ids")


def test_header_declares_and_library_exports_the_new_symbols():
    from unet_amd import _lib as L
    from unet_amd import ops
    declared = L.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L.lib, s) and s in L._sig, s
    assert ops.inst_tile_shapes() == ((4, 256), (64, 32)) and ops.inst_partials() == 2048


def test_bad_arguments_return_minus_one_without_a_launch():
    import ctypes as C
    from unet_amd import _lib as L
    lib = L.lib
    p, q, r, s = 4096, 8192, 12288, 16384          # non-null, aligned addresses that are never dereferenced: every call below fails its host check
    words = (C.c_uint32 * 8)()
    big = 2 ** 31
    calls = [
        lambda: lib.unet_cc_label_keys(None, 4, 4, p, p, None),
        lambda: lib.unet_cc_label_keys(p, 65536, 32768, p, p, None),
        lambda: lib.unet_cc_label_keys(p, 4, 4, p + 4, p, None),                       # labels not 16-byte aligned
        lambda: lib.unet_inst_distance(p, 4, 4, words, 0, p, p, None),
        lambda: lib.unet_inst_distance(p, 4, 4, words, 256, p, p, None),
        lambda: lib.unet_inst_distance(p, 0, 4, words, 8, p, p, None),
        lambda: lib.unet_inst_distance(p, 4, 4, None, 8, p, p, None),
        lambda: lib.unet_inst_check_labels(p, p, 65536, 32768, p, None),
        lambda: lib.unet_inst_ascent(p, p, 4, 4, p, None, p, None),
        lambda: lib.unet_inst_ptr_rounds(p, 16, q, q, 1, p, None),                     # the buffers must differ
        lambda: lib.unet_inst_ptr_rounds(p, 16, q, r, 65, p, None),
        lambda: lib.unet_inst_ptr_rounds(p, big, q, r, 1, p, None),
        lambda: lib.unet_inst_gather(p, p, 16, q, None),                               # ptr must not be root
        lambda: lib.unet_inst_merge_round(p, q, 4, 4, 4081, 1, r, p, s, s + 64, p, p, None),
        lambda: lib.unet_inst_merge_round(p, q, 4, 4, 32, 0, r, p, s, s + 64, p, p, None),
        lambda: lib.unet_inst_merge_round(p, q, 4, 4, 32, 33, r, p, s, s + 64, p, p, None),
        lambda: lib.unet_inst_merge_round(p, q, 4, 4, 32, 1, r, p, s, s, p, p, None),
        lambda: lib.unet_inst_merge_round(p, q, 4, 4, 32, 1, r, p, s, s + 64, None, p, None),
        lambda: lib.unet_inst_canonical(p, 16, q, q, p, None),
        lambda: lib.unet_inst_canonical(p, 0, q, r, p, None),
        lambda: lib.unet_inst_marks(p, p, big, words, p, None),
        lambda: lib.unet_inst_ids(p, p, None, 16, words, p, None),
    ]
    for i, c in enumerate(calls):
        assert c() == -1, i
        assert lib.unet_last_error(), i
