"""The conv dispatcher against a recorded table (no GPU: unet_conv2d_variant, unet_conv2d_splitk_workspace and unet_conv2d_colsum_rows only
plan).  tests/golden/conv_plans.json was recorded from the build BEFORE the four per-file ladders became csrc/conv_dispatch.hip
(tests/golden/make_conv_plans.py), over the sweep of tests/conv_plan_cases.py: a family threaded into one place and not another, a changed
validation order or a split-K redirect applied twice shows up as a differing entry."""
import json
from pathlib import Path

import pytest

import conv_plan_cases as P

GOLDEN = Path(__file__).resolve().parent / "golden" / "conv_plans.json"


@pytest.fixture(scope="module")
def table():
    doc = json.loads(GOLDEN.read_text())
    cs = P.cases()
    assert doc["sweep_sha256"] == P.sweep_hash(cs), "tests/conv_plan_cases.py changed: record the fixture again FROM THE PARENT BUILD"
    assert len(doc["results"]) == len(cs)
    return cs, doc["results"]


def test_the_recorded_table_covers_every_family_and_error_class(table):
    cs, res = table
    ids = [r[0] for r in res]
    tiled = [(c, v) for c, v in zip(cs, ids) if v >= 100]
    for special in (8, 9, 10, 11):
        for dtype in (0, 1):
            assert any(v == special and c["dtype"] == dtype for c, v in zip(cs, ids) if c), (special, dtype)
    for last in (0, 1, 5, 6, 7):
        for dtype in (0, 1):
            assert any(v % 10 == last and c["dtype"] == dtype for c, v in tiled), (last, dtype)
    for dtype in (0, 1):
        assert any(v // 1000000 >= 2 and c["dtype"] == dtype for c, v in tiled), dtype
        # stride-2 dgrad: four parity classes, each with its own tap set (column-sum rows count them)
        assert any(c["kind"] == 1 and c["stride"] == 2 and c["dtype"] == dtype for c, v in tiled), dtype
    assert any(c and c.get("pixel_shuffle") and v == 8 and c.get("ps_tail") for c, v in zip(cs, ids))
    assert any(c and c.get("pixel_shuffle") and v == -2 for c, v in zip(cs, ids))          # UNET_E_UNSUPPORTED: too small a grid
    assert any(c and c.get("pixel_shuffle") and v == -1 for c, v in zip(cs, ids))
    assert any(c and c["tuning"] == "zero" and v == -1 for c, v in zip(cs, ids))
    assert any(c and c.get("colsum") and c["dtype"] == 1 and v == -1 for c, v in zip(cs, ids))
    assert any(c and not c.get("pixel_shuffle") and c["tuning"] is None and v == -1 and r[2] == -1 for c, v, r in zip(cs, ids, res))
    assert cs[-1] is None and res[-1] == [-1, 0, -1]
    # a workspace one float short (or none) falls back to the unsplit plan of the same launch
    short = {json.dumps({**c, "ws": "ok"}, sort_keys=True): r for c, r in zip(cs, res) if c and c["ws"] == "short"}
    full = {json.dumps(c, sort_keys=True): r for c, r in zip(cs, res) if c and c["ws"] == "ok"}
    pairs = [(full[k], r) for k, r in short.items() if k in full and full[k][0] >= 2000000]
    assert pairs and all(r[0] < 1000000 and r[1] == f[1] for f, r in pairs)


def test_the_dispatcher_answers_what_the_parent_build_answered(table):
    import unet_amd._lib as L
    cs, res = table
    bad = []
    for i, (c, want) in enumerate(zip(cs, res)):
        got = P.query(L, c)
        if got != want:
            bad.append(f"case {i}: (variant, workspace floats, colsum rows) = {got}, recorded {want}: {P.describe(c)}")
    assert not bad, f"{len(bad)} of {len(cs)} entries differ\n" + "\n".join(bad[:20])
