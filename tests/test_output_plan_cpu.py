"""CPU suite of the output side of the prediction entry points (predict.check_outputs / OutputPlan / _write_outputs).

* the argument checks: every case of the grids of tests/output_check_cases.py goes through the REAL entry points, which are stopped right
  behind check_outputs, and the outcomes -- the error text, or the resolved values of the plan -- are compared with
  tests/golden/output_checks.json, recorded from the checks as they stood before check_outputs existed (tests/golden/make_output_checks.py);
* the output stage: recording fakes in place of Instances.run, vectorize_mask, write_tiff and store_tif; what is expected of the order, of the
  arguments and of where the merged array lives is what the two entry points did when each carried its own copy of the stage."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import predict as P
from unet_amd import tiffio

import output_check_cases as G
from merge_schedule import CheckedOps, FakeSource, FakeWorld, StubModel, fake_window_nonzero, run_ranks

GOLDEN = json.loads((Path(__file__).parent / "golden" / "output_checks.json").read_text())


class _Stop(Exception):
    """raised by the first statement behind check_outputs in both entry points"""


@pytest.fixture
def plans(monkeypatch):
    """the entry points stop behind their checks; -> the list that receives every plan check_outputs returned"""
    seen, real = [], P.check_outputs

    def check_outputs(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]

    def stop():
        raise _Stop

    monkeypatch.setattr(P, "check_outputs", check_outputs)
    monkeypatch.setattr(P, "_dist_ctx", stop)
    return seen


def _resolved(plan: P.OutputPlan) -> str:
    return G.accepted(plan.want, plan.floats, plan.int8_merge, plan.tile, plan.overviews, plan.vector, plan.postprocess is not None,
                      plan.instances is not None, plan.keep, plan.encode_in_place)


@pytest.mark.parametrize("form", ["save", "raster"])
def test_argument_checks_equal_the_record_over_the_whole_grid(plans, form):
    def decide(c):
        c = dict(c)
        del plans[:]
        try:                                # a ValueError of the checks passes through to G.record
            if form == "save":
                P.save_predictions("model.pkl", "tiles", c.pop("regression"), **c)
            else:
                P.predict_raster(None, None, **c)
        except _Stop:
            assert len(plans) == 1
        else:
            raise AssertionError("the entry point went on behind its checks")
        return _resolved(plans[0])

    got, want = G.record(form, decide), GOLDEN[form]
    assert got["cases"] == want["cases"] == {"save": 196608, "raster": 393216}[form]          # neither side skipped a case
    assert got["outcomes"] == want["outcomes"]
    assert got["sha256"] == want["sha256"]


def test_the_record_is_the_one_of_the_issue():
    save = GOLDEN["save"]["outcomes"]
    assert sum(n for s, n in save.items() if s.startswith("ok ")) == 1420 and sum(not s.startswith("ok ") for s in save) == 20

    def count(start):
        return sum(n for s, n in save.items() if s.startswith(start))
    assert count("postprocess needs the class mask") == 53760 and count("blend='gaussian' with large_file") == 49152
    assert count("blend='gaussian' needs merge=True") == 24576 and count("instances without an output") == 72
    assert count("instances needs merge=True") == 36
    raster = GOLDEN["raster"]["outcomes"]
    assert any(s.startswith("return_array=False needs out_path") for s in raster) and "instances_path without instances" in raster


def test_the_plan_states_each_derived_value_once():
    p = P.check_outputs()
    assert (p.want, p.floats, p.int8_merge, p.nodata, p.keep, p.encode_in_place) == ("argmax", False, False, None, False, False)
    p = P.check_outputs(regression=True, large_file=True)
    assert (p.want, p.floats, p.int8_merge, p.nodata) == (0, True, False, -9999)
    p = P.check_outputs(specific_class=2, large_file=True, compress="lzw", predictor=2)
    assert (p.want, p.floats, p.int8_merge, p.keep, p.encode_in_place) == (2, False, True, True, True)
    p = P.check_outputs(compress="lzw", raster=False)                  # predict_raster without out_path: nothing to encode
    assert not p.keep and not p.encode_in_place
    p = P.check_outputs(vector="v.geojson", class_zero=True, vector_exclude=3, raster=False, return_array=False)
    assert p.vector == (0, 3) and p.keep and not p.encode_in_place
    with pytest.raises(Exception):
        p.blend = "gaussian"                                           # frozen
    for name in ("_float_output", "_overviews", "_check_tiling", "_want", "_run_instances"):
        assert not hasattr(P, name), name


# ------------------------------------------------------------------------------------------------------------ the output stage

class _Recorder:
    """recording fakes of the four things the output stage calls"""

    def __init__(self, monkeypatch):
        self.calls = []
        self.labels, self.ids = object(), None
        rec = self

        def run(self, mask, timing=None):
            assert isinstance(mask, torch.Tensor) and mask.dtype == torch.uint8 and mask.is_contiguous()
            rec.ids = torch.arange(mask.numel(), dtype=torch.int32).reshape(mask.shape)
            rec.calls.append(("instances", dict(mask=mask)))
            return rec.labels, rec.ids, {}

        def vectorize_mask(mask, path, exclude=(), geotransform=None, epsg=None, codes=None, class_zero=False, timing=None, simplify=None,
                           labels=None, ids=None):
            rec.calls.append(("vector", dict(mask=mask, path=path, exclude=exclude, codes=codes, simplify=simplify, labels=labels, ids=ids)))

        def write_tiff(path, arr, geotransform=None, tags=None, **kw):
            rec.calls.append(("instance_raster", dict(path=path, arr=arr, **kw)))

        def store_tif(output_file, data, geotrans=None, tags=None, nodata=None, class_zero=False, compress=None, predictor=1, timing=None,
                      tile=None, overviews=None):
            rec.calls.append(("raster", dict(path=output_file, data=data, nodata=nodata, compress=compress, predictor=predictor, tile=tile,
                                             overviews=overviews)))

        monkeypatch.setattr(P.Instances, "run", run)
        for name, fn in (("vectorize_mask", vectorize_mask), ("write_tiff", write_tiff), ("store_tif", store_tif)):
            monkeypatch.setattr(P, name, fn)

    def check(self, compress, vector, instances, raster=True):
        """the parent's stage: instances (and their raster), then the vector file, then the raster"""
        want = (["instances", "instance_raster"] if instances else []) + (["vector"] if vector else []) + (["raster"] if raster else [])
        assert [w for w, _ in self.calls] == want
        got = dict(self.calls)
        if instances:
            a = got["instance_raster"]
            assert a["arr"].dtype == np.uint32 and np.array_equal(a["arr"], self.ids.numpy().view(np.uint32))
            assert (a["compress"], a["predictor"], a["tile"]) == (compress, 2 if compress else 1, 32 if compress else None)
        if vector:
            v = got["vector"]
            assert isinstance(v["mask"], torch.Tensor)                                    # kept where the merge assembled it
            assert (v["labels"] is self.labels and v["ids"] is self.ids) if instances else (v["labels"] is None and v["ids"] is None)
            assert v["exclude"] == (2,) and v["simplify"] == 1.5
        if instances and vector:
            assert v["mask"] is got["instances"]["mask"]
        if raster:
            r = got["raster"]
            assert isinstance(r["data"], torch.Tensor if compress else np.ndarray), type(r["data"])
            assert r["data"].dtype == (torch.uint8 if compress else np.uint8) and r["nodata"] is None
            assert (r["compress"], r["predictor"], r["tile"], r["overviews"]) == (compress, 2 if compress else 1, 32 if compress else None,
                                                                                   "mode" if compress else None)
        return got


def _options(tmp_path, compress, vector, instances):
    kw = dict(compress="lzw", predictor=2, tile=32, overviews="auto") if compress else {}
    if instances:
        kw.update(instances={"classes": 1}, instances_path=tmp_path / "i.tif")
    if vector:
        kw.update(vector_path=tmp_path / "v.geojson", vector_exclude=2, vector_simplify=1.5)
    return kw


COMBOS = [(c, v, i) for c in (None, "lzw") for v in (False, True) for i in (False, True)]


def _raster_run(monkeypatch, raster, world, **kw):
    fw = FakeWorld(world)
    CheckedOps(fw, numeric=True).install(monkeypatch)
    monkeypatch.setattr(P.ops, "WindowSource", FakeSource)
    monkeypatch.setattr(P.ops, "window_nonzero", fake_window_nonzero)
    return run_ranks(world, lambda r: P.predict_raster(StubModel(3, fw), raster, 16, 0.25, batch_size=3, **kw), monkeypatch, fw)[0]


@pytest.fixture(scope="module")
def scene():
    raster = np.random.default_rng(11).integers(1, 250, (2, 45, 38)).astype(np.uint8)
    return raster, {}


def _plain(monkeypatch, scene):
    """the mask of the plain call, computed once and left unchanged"""
    raster, cache = scene
    if "mask" not in cache:
        cache["mask"] = _raster_run(monkeypatch, raster, 1)
        cache["mask"].setflags(write=False)
    return cache["mask"]


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("compress,vector,instances", COMBOS)
def test_predict_raster_output_stage(monkeypatch, tmp_path, scene, compress, vector, instances, world):
    mask = _plain(monkeypatch, scene)
    rec = _Recorder(monkeypatch)
    out = _raster_run(monkeypatch, scene[0], world, out_path=tmp_path / "o.tif", **_options(tmp_path, compress, vector, instances))
    got = rec.check(compress, vector, instances)
    assert isinstance(out, np.ndarray) and np.array_equal(out, mask)
    assert np.array_equal(np.asarray(got["raster"]["data"]), mask) and got["raster"]["path"] == tmp_path / "o.tif"
    if vector:
        assert got["vector"]["path"] == tmp_path / "v.geojson" and got["vector"]["codes"] is None and np.array_equal(got["vector"]["mask"], mask)


@pytest.mark.parametrize("compress", [None, "lzw"])
@pytest.mark.parametrize("return_array", [True, False])
def test_predict_raster_without_out_path_but_with_a_vector_path(monkeypatch, tmp_path, scene, compress, return_array):
    mask = _plain(monkeypatch, scene)
    rec = _Recorder(monkeypatch)
    kw = dict(compress="lzw", predictor=2) if compress else {}
    out = _raster_run(monkeypatch, scene[0], 1, vector_path=tmp_path / "v.geojson", vector_exclude=2, vector_simplify=1.5, return_array=return_array,
                      **kw)
    got = rec.check(compress, True, False, raster=False)
    assert np.array_equal(got["vector"]["mask"], mask)
    assert (isinstance(out, np.ndarray) and np.array_equal(out, mask)) if return_array else out is None      # no raster: nothing to encode, so
    rec.calls.clear()                                                                                      # the array goes to the host
    out = _raster_run(monkeypatch, scene[0], 1, out_path=tmp_path / "o.tif", return_array=False, **kw)
    assert out is None and [w for w, _ in rec.calls] == ["raster"]
    assert isinstance(rec.calls[0][1]["data"], torch.Tensor if compress else np.ndarray)


@pytest.mark.parametrize("compress,vector,instances", COMBOS)
def test_save_predictions_output_stage(monkeypatch, tmp_path, compress, vector, instances):
    """save_predictions behind its merge: _save_merged is replaced by one that hands back a mask the way _Merge.finish does -- as a tensor
    exactly when compress, a vector file or instances are asked for"""
    import types
    tiles = tmp_path / "tiles"
    tiles.mkdir()
    tiffio.write_tiff(tiles / "t0.tif", np.ones((3, 8, 8), np.uint8), geotransform=[10.0, 1.0, 0.0, 50.0, 0.0, -1.0])
    mask = np.random.default_rng(2).integers(0, 3, (8, 8)).astype(np.uint8)
    keep = compress is not None or vector or instances
    learn = types.SimpleNamespace(model=types.SimpleNamespace(_device=torch.device("cpu"), n_out=3),
                                  dls=types.SimpleNamespace(vocab=["a", "b", "c"], train_ds=types.SimpleNamespace(dtype="int8")))
    monkeypatch.setattr(P, "load_learner", lambda *a, **k: learn)
    monkeypatch.setattr(P, "_dist_ctx", lambda: (0, 0, 1))
    monkeypatch.setattr(P, "_tile_windows", lambda *a: None)

    def save_merged(model, tiles_, geos, windows, rank, world, plan, *rest):
        assert plan.keep == keep
        return (torch.from_numpy(mask) if keep else mask), [10.0, 1.0, 0.0, 50.0, 0.0, -1.0]

    monkeypatch.setattr(P, "_save_merged", save_merged)
    rec = _Recorder(monkeypatch)
    kw = _options(tmp_path, compress, vector, instances)
    if "vector_path" in kw:
        kw["vector"] = bool(kw.pop("vector_path"))
    if "instances_path" in kw:
        kw["instances_raster"] = bool(kw.pop("instances_path"))
    out = P.save_predictions(tmp_path / "net.pkl", tiles, False, merge=True, AOI="aoi", **kw)
    assert out == tmp_path / "aoi_net_prediction.tif"
    got = rec.check(compress, vector, instances)
    assert got["raster"]["path"] == out and np.array_equal(np.asarray(got["raster"]["data"]), mask)
    if vector:
        assert got["vector"]["path"] == tmp_path / "aoi_net_prediction.geojson" and got["vector"]["codes"] == ["a", "b", "c"]
    if instances:
        assert got["instance_raster"]["path"] == tmp_path / "aoi_net_prediction_instances.tif"
