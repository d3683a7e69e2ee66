"""GPU suite of the output side of the prediction entry points: every output option at once -- postprocess, instances with their raster, a
simplified vector file, a tiled LZW raster with Predictor 2 and overviews -- through predict_raster and through save_predictions, which share
one checked OutputPlan and one output stage (predict._write_outputs) and so must write the same rasters and the same features."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import predict as P  # noqa: E402

from test_instances_gpu import _export, _model  # noqa: E402

TIMING_KEYS = {"write_seconds", "file_bytes", "vector_seconds", "vector_polygons", "vector_vertices", "vector_vertices_raw", "instances_seconds",
               "instances", "instances_write_seconds", "instances_file_bytes", "postprocess_seconds"}


def test_every_output_option_at_once_through_both_entry_points(tmp_path):
    import create_tiles_unet as T
    from unet_amd.tiffio import read_tiff, tiff_info, write_tiff
    size = 64
    model = _model("xresnet18", 4, 3, size, seed=11)
    img = np.random.default_rng(5).integers(1, 250, (4, 200, 170)).astype(np.uint8)
    rpath = tmp_path / "scene.tif"
    write_tiff(rpath, img, geotransform=(400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5))
    kw = dict(batch_size=5, postprocess={"majority": 5, "sieve": 20}, instances={"classes": [1, 2], "radius": 16, "min_depth": 1.0},
              vector_simplify=1.0, compress="lzw", predictor=2, tile=64, overviews="auto")
    t1, t2 = {}, {}
    got = P.predict_raster(model, rpath, size, 0.2, max_empty=0.9, out_path=tmp_path / "a.tif", vector_path=tmp_path / "a.geojson",
                           instances_path=tmp_path / "a_inst.tif", timing=t1, **kw)
    tiles = tmp_path / "cut"
    T.split_raster(rpath, None, tiles, patch_size=size, patch_overlap=0.2, split=[1], max_empty=0.9)
    f = P.save_predictions(_export(tmp_path, model, 3, size), tiles / "img_tiles", False, merge=True, AOI="b", validation_vision=False,
                           vector=True, instances_raster=True, timing=t2, **kw)
    mask, meta = read_tiff(tmp_path / "a.tif")
    assert mask.dtype == np.uint8 and np.array_equal(mask, got) and len(np.unique(mask)) > 1
    mask2, meta2 = read_tiff(f)
    assert np.array_equal(mask2, mask) and tuple(meta2["geotransform"]) == tuple(meta["geotransform"])
    ids, ids2 = read_tiff(tmp_path / "a_inst.tif")[0], read_tiff(f.with_name(f.stem + "_instances.tif"))[0]
    assert ids.dtype == np.uint32 and np.array_equal(ids2, ids) and np.array_equal(ids > 0, np.isin(mask, [1, 2])) and ids.max() > 0
    a, b = tiff_info(tmp_path / "a.tif"), tiff_info(f)
    assert os.path.getsize(tmp_path / "a.tif") == t1["file_bytes"] and os.path.getsize(f) == t2["file_bytes"]
    assert (a["height"], a["width"]) == (b["height"], b["width"]) == mask.shape
    feats, feats2 = (json.load(open(p))["features"] for p in (tmp_path / "a.geojson", f.with_suffix(".geojson")))
    assert len(feats) == len(feats2) == t1["vector_polygons"] == t2["vector_polygons"] > 0
    for x, y in zip(feats, feats2):
        assert x["geometry"] == y["geometry"]
        assert (x["properties"]["pixels"], x["properties"]["instance"]) == (y["properties"]["pixels"], y["properties"]["instance"])
    assert {x["properties"]["instance"] for x in feats} <= set(range(int(ids.max()) + 1))          # (a ring simplified away has no feature)
    for t in (t1, t2):
        assert TIMING_KEYS <= set(t), TIMING_KEYS - set(t)
        assert t["instances"]["instances"] == int(ids.max()) and t["vector_vertices"] <= t["vector_vertices_raw"]
