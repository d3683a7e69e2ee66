"""Inputs of the zonal tests (plain NumPy, seeded): the feature sets of tests/rasterize_cases.py written as GeoJSON files, zone planes and
label images for the histogram kernel."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))

import rasterize_cases as RC  # noqa: E402

GT = (500000.0, 0.25, 0.0, 5600000.0, 0.0, -0.25)          # exact in float64, as every coordinate it produces here
SHAPE = (40, 56)                                           # the raster of RC.feature_sets()


def _position(X, Y, gt):
    x, y = X / 256.0, Y / 256.0
    return [x, y] if gt is None else [gt[0] + x * gt[1], gt[3] + y * gt[5]]


def set_document(name: str, features, gt=None) -> dict:
    """one feature set as a FeatureCollection: a Polygon per feature ("multi": a MultiPolygon with one part per ring), every second ring
    closed by repeating its first point, the burn value as the property `class` and a `name`; "stars" also holds a feature with a null
    geometry in second place"""
    out = []
    for i, (value, rings) in enumerate(features):
        coords = [[_position(X, Y, gt) for X, Y in ring] + ([_position(*ring[0], gt)] if ring and j % 2 else []) for j, ring in enumerate(rings)]
        geom = {"type": "MultiPolygon", "coordinates": [[c] for c in coords]} if name == "multi" else {"type": "Polygon", "coordinates": coords}
        out.append({"type": "Feature", "properties": {"class": int(value), "name": f"{name}-{i}"}, "geometry": geom})
    if name == "stars":
        out.insert(1, {"type": "Feature", "properties": {"class": 3, "name": "nothing"}, "geometry": None})
    return {"type": "FeatureCollection", "features": out}


def write_set_files(folder, gt=None) -> dict:
    """{set name: path} of the files of every feature set of RC.feature_sets()"""
    paths = {}
    for name, features in sorted(RC.feature_sets().items()):
        paths[name] = os.path.join(os.fspath(folder), f"{name}.geojson")
        with open(paths[name], "w") as f:
            json.dump(set_document(name, features, gt), f)
    return paths


def rings_as_lists(r) -> dict:
    """a Rings as JSON-ready lists"""
    return {"xy": r.xy.tolist(), "ring_start": r.ring_start.tolist(), "feature_ring_start": r.feature_ring_start.tolist(), "values": r.values.tolist()}


# ------------------------------------------------------------------------------------------------------------ planes

def zone_patterns(H: int, W: int, Z: int, C: int, seed: int) -> dict:
    """{name: (zones int32 [H, W], mask uint8 [H, W])}; in every pattern but "none" the zone Z - 1 and the class C - 1 occur together on the
    last pixel"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    p = {}
    p["none"] = (np.full((H, W), -1), rng.integers(0, C, (H, W)))
    p["one"] = (np.full((H, W), Z - 1), np.full((H, W), C - 1))
    p["blocks"] = (((yy // 2) * ((W + 1) // 2) + xx // 2) % Z, ((yy // 2 + xx // 2) % C))
    p["checker"] = ((yy * W + xx) % Z, (yy + xx) % C)
    p["stripes"] = (((yy * W + xx) // 24) % Z, ((yy * W + xx) // 40) % C)          # runs of 6 and 10 lanes' worth of one key, across the rows
    z = rng.integers(0, Z, (H, W))
    z[rng.random((H, W)) < 0.3] = -1
    p["random"] = (z, rng.integers(0, C, (H, W)))
    out = {}
    for name, (z, m) in p.items():
        z, m = np.ascontiguousarray(z, dtype=np.int32), np.ascontiguousarray(m, dtype=np.uint8)
        if name != "none":
            z[-1, -1], m[-1, -1] = Z - 1, C - 1
        out[name] = (z, m)
    return out


# ------------------------------------------------------------------------------------------------------------ the entry points

E2E_SIZE, E2E_GT = 64, (400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5)


def e2e_scene(folder):
    """the 96 x 96 scene of the end-to-end tests, written as <folder>/scene.tif; returns its path"""
    from unet_amd.tiffio import write_tiff
    img = np.random.default_rng(5).integers(1, 250, (4, 96, 96)).astype(np.uint8)
    path = os.path.join(os.fspath(folder), "scene.tif")
    write_tiff(path, img, geotransform=E2E_GT)
    return path


def default_outputs(P, T, folder, model, pkl) -> dict:
    """{name: sha256} of what both entry points return and write with no zonal argument given: the mask, the LZW raster and the vector file
    of predict_raster, the merged raster and the vector file of save_predictions.  tests/golden/zonal_default_outputs.json holds these
    digests as the commit before the zonal statistics produced them."""
    import hashlib
    from pathlib import Path
    folder = Path(folder)
    digest = lambda b: hashlib.sha256(b).hexdigest()  # noqa: E731
    rpath = e2e_scene(folder)
    mask = P.predict_raster(model, rpath, E2E_SIZE, 0.2, max_empty=0.9, batch_size=5, out_path=folder / "d.tif", vector_path=folder / "d.geojson",
                            compress="lzw", postprocess={"majority": 3, "sieve": 10})
    out = {"mask_shape": list(mask.shape), "mask": digest(np.ascontiguousarray(mask).tobytes()), "raster": digest((folder / "d.tif").read_bytes()),
           "vector": digest((folder / "d.geojson").read_bytes())}
    T.split_raster(rpath, None, folder / "cut", patch_size=E2E_SIZE, patch_overlap=0.2, split=[1], max_empty=0.9)
    f = P.save_predictions(pkl, folder / "cut" / "img_tiles", False, merge=True, AOI="d", validation_vision=False, batch_size=5, vector=True,
                           postprocess={"majority": 3, "sieve": 10})
    out["merged_raster"] = digest(Path(f).read_bytes())
    out["merged_vector"] = digest(Path(f).with_suffix(".geojson").read_bytes())
    return out
