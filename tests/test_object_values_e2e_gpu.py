"""GPU suite of the float statistics per object at the prediction entry points (predict.py): the height_* and confidence_*
columns that predict_raster and save_predictions write equal the restatement of the rules (tests/object_values_ref.py) applied to the
returned mask, to its labels and to the plane -- exactly, as the files' bytes.  The confidence plane is recomputed on the host from a second
call with all_classes=True: both calls run the same merge (the same placements, batches and finalisation; `want` only selects what
_Merge.finish hands out), so the maximum over the returned class planes has the bits of the plane that the objects stage summarised; the test
asserts that the argmax of those planes is the returned mask.  The buffers of the objects stage sit in guard bands as in
tests/test_object_values_gpu.py.  N ranks: every rank of a 2-rank run in one process (tests/merge_schedule.py), with a fake world that
queues the two strips -- mask and confidence -- that a rank sends; its reference plane comes from a 2-rank all_classes run.  A world-2 run
over a real process group (the style of tests/test_ddp_gpu.py) is not part of this suite."""
import json
import os
import sys
from dataclasses import dataclass

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import object_values_ref as VR  # noqa: E402
import objects_ref as OR  # noqa: E402
import postprocess_ref as R  # noqa: E402
import zonal_cases as ZC  # noqa: E402
from merge_schedule import FakeWorld, run_ranks  # noqa: E402
from test_object_values_gpu import guards  # noqa: E402,F401  (the fixture)

_VALUE_KEYS = tuple(f"{n}_{k}" for n in ("height", "confidence") for k in ("valid", "mean", "std", "sum", "min", "max", "peak_x", "peak_y"))
KW = dict(max_empty=0.9, batch_size=5)


def _ob():
    from unet_amd import objects
    return objects


@dataclass
class QueueWorld(FakeWorld):
    """FakeWorld whose ranks may send more than one strip to rank 0: they are received in the order they were sent, as over a real backend"""

    def send(self, t, dst):
        assert dst == 0 and self.rank != 0, (self.rank, dst)
        self.parts.setdefault(self.rank, []).append(t.clone())

    def recv(self, buf, src):
        assert self.rank == 0 and self.parts.get(src), (self.rank, src, sorted(self.parts))
        got = self.parts[src].pop(0)
        if not self.parts[src]:
            del self.parts[src]
        assert got.shape == buf.shape and got.dtype == buf.dtype, (src, got.shape, buf.shape)
        buf.copy_(got)


def _height(shape, tmp_path, gt):
    """a synthetic canopy height model on the output grid, with nodata, NaN and a plateau; returns (path, array)"""
    from unet_amd.tiffio import write_tiff
    H, W = shape
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:H, 0:W]
    v = (12.0 + 9.0 * np.sin(yy / 7.0) * np.cos(xx / 5.0) + rng.random((H, W))).astype(np.float32)
    v[rng.random((H, W)) < 0.03] = -9999.0
    v[rng.random((H, W)) < 0.02] = np.nan
    v[10:14, 20:30] = 31.5                                      # equal maxima: the peak is the first of them
    path = tmp_path / "chm.tif"
    write_tiff(path, v, geotransform=gt, nodata=-9999)
    return path, v


def _want_rows(mask, labels, exclude, gt, height, conf, codes=None, class_zero=False, instance=None):
    ex = () if exclude is None else ((exclude,) if isinstance(exclude, int) else tuple(exclude))
    t = OR.table(mask, labels, exclude)
    rows = OR.rows(t, gt, codes, class_zero, instance)
    h = VR.rows(VR.tables(mask, labels, height, ex, -9999), gt, "height")
    c = VR.rows(VR.tables(mask, labels, conf, ex), gt, "confidence")
    assert len(rows) == len(h) == len(c)
    return t, [{**a, **b, **d} for a, b, d in zip(rows, h, c)]


def _same_file(path, rows, tmp_path, gt, epsg=None, class_zero=False):
    ref = tmp_path / ("ref_" + os.path.basename(path))
    _ob().write_objects(ref, rows, gt, epsg, class_zero=class_zero)
    assert open(path, "rb").read() == ref.read_bytes(), path
    return json.load(open(path))["features"]


def test_entry_points_write_the_statistics_of_the_planes(tmp_path, guards, monkeypatch):  # noqa: F811
    import create_tiles_unet as T
    import predict as P
    from unet_amd import instances as I
    from unet_amd.tiffio import read_tiff
    from unet_amd.vectorize import epsg_of_tags
    from test_instances_gpu import _export, _model
    size, gt = ZC.E2E_SIZE, ZC.E2E_GT
    model = _model("xresnet18", 4, 3, size, seed=11)
    rpath = ZC.e2e_scene(tmp_path)
    # the defaults: the objects file as it was, and neither new launcher runs
    plain = P.predict_raster(model, rpath, size, 0.2, objects_path=tmp_path / "plain.geojson", vector_path=tmp_path / "plain_v.geojson", **KW)
    assert guards.by_name["obj_accumulate"] == 1 and "obj_absmax" not in guards.by_name and "obj_values" not in guards.by_name
    comp = R.label_components(plain, 4)
    _same_file(tmp_path / "plain.geojson", OR.rows(OR.table(plain, comp), gt), tmp_path, gt)
    probs = P.predict_raster(model, rpath, size, 0.2, all_classes=True, **KW)
    assert probs.dtype == np.float32 and probs.shape == (3,) + plain.shape and np.array_equal(probs.argmax(axis=0).astype(np.uint8), plain)
    conf = np.ascontiguousarray(probs.max(axis=0))
    assert 0.33 < conf.min() < conf.max() <= 1.0
    hpath, height = _height(plain.shape, tmp_path, gt)
    # the objects file with both planes
    timing = {}
    got = P.predict_raster(model, rpath, size, 0.2, objects_path=tmp_path / "a.geojson", objects_values_path=hpath, objects_values_name="height",
                           objects_confidence=True, timing=timing, **KW)
    assert np.array_equal(got, plain)
    assert guards.by_name["obj_absmax"] == 2 and guards.by_name["obj_values"] == 2 and guards.by_name["obj_accumulate"] == 2
    _, rows = _want_rows(plain, comp, None, gt, height, conf)
    feats = _same_file(tmp_path / "a.geojson", rows, tmp_path, gt)
    assert len(feats) == timing["objects"] > 3 and 0 < timing["objects_values_seconds"] <= timing["objects_seconds"]
    assert all(list(f["properties"])[-16:] == list(_VALUE_KEYS) for f in feats)
    assert any(f["properties"]["height_max"] == 31.5 for f in feats) and all(f["properties"]["confidence_valid"] == f["properties"]["pixels"] for f in feats)
    # a CSV, one plane, an excluded class
    assert P.predict_raster(model, rpath, size, 0.2, objects_path=tmp_path / "a.csv", objects_exclude=0, objects_confidence=True, return_array=False,
                            **KW) is None
    import csv
    with open(tmp_path / "a.csv", newline="") as f:
        table = list(csv.reader(f))
    t0, rows0 = _want_rows(plain, comp, 0, gt, height, conf)
    assert table[0][-8:] == list(_VALUE_KEYS[8:]) and "height_mean" not in table[0] and len(table) == 1 + len(rows0)
    assert [line[-8:] for line in table[1:]] == [[repr(r[k]) if isinstance(r[k], float) else str(r[k]) for k in _VALUE_KEYS[8:]] for r in rows0]
    # with the vector file and instances: the objects are the instances, and the polygons carry the same columns
    inst = dict(classes=[1, 2], radius=8, min_depth=0.5)
    got = P.predict_raster(model, rpath, size, 0.2, vector_path=tmp_path / "i.geojson", objects_path=tmp_path / "io.geojson", instances=inst,
                           class_zero=True, objects_values_path=hpath, objects_values_name="height", objects_confidence=True, **KW)
    P.predict_raster(model, rpath, size, 0.2, vector_path=tmp_path / "i1.geojson", objects_path=tmp_path / "io1.geojson", instances=inst, class_zero=True,
                     **KW)
    assert np.array_equal(got, plain)
    labels, ids, _ = I.Instances(**inst).run(torch.from_numpy(plain).cuda())
    labels = labels.cpu().numpy()
    ti = OR.table(plain, labels, 0)
    _, rows_i = _want_rows(plain, labels, 0, gt, height, conf, None, True, ids.cpu().numpy().ravel()[ti["label"]])
    pts = _same_file(tmp_path / "io.geojson", rows_i, tmp_path, gt, class_zero=True)
    polys, polys1 = (json.load(open(tmp_path / f))["features"] for f in ("i.geojson", "i1.geojson"))
    assert len(polys) == len(polys1) == len(pts) and max(p["properties"]["instance"] for p in pts) > 0
    for f, f1, p in zip(polys, polys1, pts):
        assert f["geometry"] == f1["geometry"] and list(f["properties"]) == list(f1["properties"]) + list(_VALUE_KEYS)
        assert all(f["properties"][k] == p["properties"][k] for k in _VALUE_KEYS)
        assert {k: v for k, v in f["properties"].items() if k not in _VALUE_KEYS} == f1["properties"]
    # a value raster off the grid is refused before the merge runs
    from unet_amd.tiffio import write_tiff
    write_tiff(tmp_path / "off.tif", height, geotransform=(gt[0] + 0.5, *gt[1:]))
    launches = dict(guards.by_name)
    with pytest.raises(ValueError, match="no resampling"):
        P.predict_raster(model, rpath, size, 0.2, objects_path=tmp_path / "x.geojson", objects_values_path=tmp_path / "off.tif", **KW)
    assert guards.by_name == launches and not (tmp_path / "x.geojson").exists()
    # the tile-file entry point: <merged raster stem>_objects.geojson with the vocab's names, and the polygons of vector=True
    pkl = _export(tmp_path, model, 3, size)
    tiles = tmp_path / "cut"
    T.split_raster(rpath, None, tiles, patch_size=size, patch_overlap=0.2, split=[1], max_empty=0.9)
    f0 = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, AOI="n", validation_vision=False, batch_size=5, vector=True, objects=True)
    timing = {}
    f = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, AOI="o", validation_vision=False, batch_size=5, vector=True, objects=True,
                           objects_exclude=0, objects_values=hpath, objects_values_name="height", objects_confidence=True, timing=timing)
    merged = read_tiff(f)[0]
    assert np.array_equal(merged, plain) and f.read_bytes() == f0.read_bytes()
    fp = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, all_classes=True, AOI="p", validation_vision=False, batch_size=5)
    conf2 = np.ascontiguousarray(read_tiff(fp)[0].max(axis=0))
    _, named = _want_rows(plain, comp, 0, gt, height, conf2, ["c0", "c1", "c2"])
    pts = _same_file(f.with_name(f.stem + "_objects.geojson"), named, tmp_path, gt, epsg_of_tags(read_tiff(f)[1]["tags"]))
    assert timing["objects"] == len(named) and timing["objects_values_seconds"] > 0
    with_cols = json.load(open(f.with_suffix(".geojson")))["features"]
    by_point = {(p["properties"]["point_x"], p["properties"]["point_y"]): p["properties"] for p in pts}
    seen = 0
    for feat in with_cols:
        props = feat["properties"]
        if "point_x" in props:
            seen += 1
            assert all(props[k] == by_point[(props["point_x"], props["point_y"])][k] for k in _VALUE_KEYS)
        else:
            assert props["class"] == 0 and not any(k in props for k in _VALUE_KEYS)
    assert seen == len(pts)
    # two ranks, last (the fake world stays patched in until the test ends): each rank takes the plane of its own rows and rank 0
    # assembles it behind the mask.  Two ranks run other batches than one (two windows each instead of four), so their probabilities may
    # differ from one rank's in the last bits, as a specific_class plane's do: the reference plane is that of a 2-rank all_classes run
    probs2, _ = run_ranks(2, lambda r: P.predict_raster(model, rpath, size, 0.2, all_classes=True, **KW), monkeypatch, FakeWorld(2))
    assert np.array_equal(probs2.argmax(axis=0).astype(np.uint8), plain) and np.abs(probs2 - probs).max() < 1e-3
    out, _ = run_ranks(2, lambda r: P.predict_raster(model, rpath, size, 0.2, objects_path=tmp_path / "w2.geojson", objects_values_path=hpath,
                                                     objects_values_name="height", objects_confidence=True, **KW), monkeypatch, QueueWorld(2))
    assert np.array_equal(out, plain)
    _same_file(tmp_path / "w2.geojson", _want_rows(plain, comp, None, gt, height, np.ascontiguousarray(probs2.max(axis=0)))[1], tmp_path, gt)
    guards.check("end")
