"""Record tests/golden/conv_plans.json: what a BUILT tree answers for the sweep of tests/conv_plan_cases.py.

    python tests/golden/make_conv_plans.py <root of the built tree to record>

The tree to record is the parent of a change to the conv dispatcher (a copy of it outside this checkout, built with
`python -m unet_amd.build`), never the tree under test: tests/test_conv_dispatch_cpu.py compares the new code against these numbers.
No GPU is needed: the three entry points only plan."""
import importlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import conv_plan_cases as P  # noqa: E402


def main():
    tree = Path(sys.argv[1]).resolve()
    sys.path.insert(0, str(tree))
    L = importlib.import_module("unet_amd._lib")
    assert Path(L.__file__).resolve().is_relative_to(tree), f"unet_amd came from {L.__file__}, not from {tree}"
    cs = P.cases()
    doc = {"sweep_sha256": P.sweep_hash(cs), "abi": L.lib.unet_abi_version(), "results": P.run(L, cs)}
    text = json.dumps(doc, separators=(",", ":")).replace("],[", "],\n[")
    (HERE / "conv_plans.json").write_text(text + "\n")
    print(len(cs), "cases,", len(text), "bytes")


if __name__ == "__main__":
    main()
