"""Record tests/golden/output_checks.json: what the argument checks of the two prediction entry points answered BEFORE they became
predict.check_outputs, over the grids of tests/output_check_cases.py.

    python tests/golden/make_output_checks.py <root of the tree to record>

The tree to record is the parent of the change that introduced check_outputs (a checkout of it outside this one), never the tree under
test: below stand the opening blocks of its save_predictions and predict_raster, statement by statement, on the functions that tree has.
tests/test_output_plan_cpu.py replays the same grids through check_outputs and compares.  No GPU is needed: nothing here launches."""
import importlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import output_check_cases as G  # noqa: E402


def old_save(P, regression, all_classes, large_file, class_zero, vector, instances_raster, specific_class, merge, blend, postprocess, compress,
             predictor, tile, overviews, vector_exclude, vector_simplify, instances):
    P.check_blend(blend, large_file, merge)
    post = P.check_postprocess(postprocess, regression, all_classes, specific_class, merge)
    P.check_compress(compress, predictor, P._float_output(regression, all_classes, specific_class, large_file))
    tile, overviews = P._check_tiling(compress, tile, overviews, regression, all_classes, specific_class, large_file)
    vec = P.check_vector(vector or None, vector_exclude, regression, all_classes, specific_class, large_file, merge, class_zero, vector_simplify)
    if instances is None and instances_raster:
        raise ValueError("instances_raster without instances")
    inst = P.check_instances(instances, regression, all_classes, specific_class, large_file, merge, vec is not None or bool(instances_raster))
    keep = compress is not None or vec is not None or inst is not None          # what save_predictions hands to _save_merged
    return G.accepted(P._want(regression, all_classes, specific_class), P._float_output(regression, all_classes, specific_class, large_file),
                      large_file and not regression, tile, overviews, vec, post, inst, keep, compress is not None)


def old_raster(P, regression, all_classes, large_file, class_zero, vector_path, instances_path, specific_class, out_path, return_array, blend,
               postprocess, compress, predictor, tile, overviews, vector_exclude, vector_simplify, instances):
    P.check_blend(blend, large_file)
    post = P.check_postprocess(postprocess, regression, all_classes, specific_class)
    P.check_compress(compress, predictor, P._float_output(regression, all_classes, specific_class, large_file))
    tile, overviews = P._check_tiling(compress, tile, overviews, regression, all_classes, specific_class, large_file)
    vec = P.check_vector(vector_path, vector_exclude, regression, all_classes, specific_class, large_file, True, class_zero, vector_simplify)
    if instances is None and instances_path is not None:
        raise ValueError("instances_path without instances")
    inst = P.check_instances(instances, regression, all_classes, specific_class, large_file, True, vec is not None or instances_path is not None)
    if not return_array and out_path is None and vec is None:
        raise ValueError("return_array=False needs out_path: the prediction would go nowhere")
    keep_out = compress is not None and out_path is not None
    return G.accepted(P._want(regression, all_classes, specific_class), P._float_output(regression, all_classes, specific_class, large_file),
                      large_file and not regression, tile, overviews, vec, post, inst, keep_out or vec is not None or inst is not None, keep_out)


def main():
    tree = Path(sys.argv[1]).resolve()
    sys.path.insert(0, str(tree))
    P = importlib.import_module("predict")
    assert Path(P.__file__).resolve().is_relative_to(tree), f"predict came from {P.__file__}, not from {tree}"
    doc = {"save": G.record("save", lambda c: old_save(P, **c)), "raster": G.record("raster", lambda c: old_raster(P, **c))}
    (HERE / "output_checks.json").write_text(json.dumps(doc, indent=1) + "\n")
    for form, r in doc.items():
        ok = sum(n for s, n in r["outcomes"].items() if s.startswith("ok "))
        print(f"{form}: {r['cases']} cases, {ok} accepted, {len(r['outcomes'])} distinct outcomes, sha256 {r['sha256'][:16]}")


if __name__ == "__main__":
    main()
