"""The grid of output arguments that tests/golden/output_checks.json records and tests/test_output_plan_cpu.py replays: every combination
of the values below, in this order (the last name varies fastest), in the two forms the entry points hand them to the checks.

    "save"    save_predictions: merge, vector=True | False, instances_raster=True | False
    "raster"  predict_raster: merge is always True, the vector output follows from vector_path, the instance raster from instances_path,
              and out_path / return_array decide whether the prediction goes anywhere

One outcome string per case: the text of the ValueError, or for an accepted case the resolved values (`accepted`).  A record is the case
count, the count per distinct outcome and a SHA-256 over the outcome strings joined by newlines."""
import hashlib
import itertools

_BOOL = (False, True)
_COMMON = (("blend", ("mean", "gaussian")), ("postprocess", (None, {"sieve": 8})), ("compress", (None, "lzw")), ("predictor", (1, 2)),
           ("tile", (None, 256)), ("overviews", (None, "auto", "mode")), ("vector_exclude", (None, 1)), ("vector_simplify", (None, 1.0)),
           ("instances", (None, {"classes": 1})))
GRIDS = {
    "save": (("regression", _BOOL), ("all_classes", _BOOL), ("large_file", _BOOL), ("class_zero", _BOOL), ("vector", _BOOL),
             ("instances_raster", _BOOL), ("specific_class", (None, 1)), ("merge", (True, False))) + _COMMON,
    "raster": (("regression", _BOOL), ("all_classes", _BOOL), ("large_file", _BOOL), ("class_zero", _BOOL), ("vector_path", (None, "v.geojson")),
               ("instances_path", (None, "i.tif")), ("specific_class", (None, 1)), ("out_path", (None, "o.tif")), ("return_array", (True, False)))
    + _COMMON,
}


def cases(form: str):
    names = [n for n, _ in GRIDS[form]]
    for values in itertools.product(*(v for _, v in GRIDS[form])):
        yield dict(zip(names, values))


def accepted(want, floats, int8_merge, tile, overviews, exclude, post, inst, keep, encode) -> str:
    """the outcome string of an accepted case; post / inst: whether a PostProcess / an Instances came out of the checks"""
    return (f"ok want={want!r} floats={bool(floats)} int8_merge={bool(int8_merge)} tile={tile!r} overviews={overviews!r} exclude={exclude!r} "
            f"post={bool(post)} inst={bool(inst)} keep={bool(keep)} encode={bool(encode)}")


def record(form: str, decide) -> dict:
    """decide(case) -> the accepted string, or raises the ValueError of the checks"""
    counts, sha, n = {}, hashlib.sha256(), 0
    for c in cases(form):
        try:
            s = decide(c)
        except ValueError as e:
            s = str(e)
        counts[s] = counts.get(s, 0) + 1
        sha.update((("\n" if n else "") + s).encode())
        n += 1
    return {"cases": n, "outcomes": dict(sorted(counts.items())), "sha256": sha.hexdigest()}
