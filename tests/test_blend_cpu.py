"""CPU suite of Gaussian window blending (blend="gaussian"): the profile, the refusals, the C ABI surface, the params_and_main keyword,
and the N-rank merge schedule of the blended path with bounds-checking fakes (tests/blend_schedule.py) -- the cfg5 plan on the meta
device for bounds, small plans with numpy float32 arithmetic for numbers (N ranks == 1 rank == the numpy restatement)."""
import numpy as np
import pytest
import torch

import predict as P
from unet_amd.mosaic import MergePlan, blend_profile, check_blend, merge_order, sliding_windows

import blend_ref as B
from blend_schedule import BlendCheckedOps
from merge_schedule import FakeSource, FakeWorld, StubModel, check_schedule, fake_window_nonzero, run_ranks

C5 = 5


# ------------------------------------------------------------------------------------------------------------ profile

@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 400, 512, 1024])
def test_profile_is_the_closed_form(n):
    g = blend_profile(n)
    t = np.arange(n, dtype=np.float64)
    ref = np.exp(-((t - (n - 1) / 2) ** 2) / (2 * (n / 8) ** 2))
    ref = (ref / ref.max()).astype(np.float32)
    assert g.dtype == np.float32 and g.shape == (n,)
    assert np.array_equal(g.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(g, g[::-1]) and g.max() == np.float32(1.0) and (g > 0).all()
    if n > 2:
        assert abs(float(g.min()) - np.exp(-8 * (n - 1) ** 2 / n ** 2)) <= 1e-6 and g.min() >= 3.3e-4


# ------------------------------------------------------------------------------------------------------------ refusals

def test_blend_argument_is_checked_on_the_host():
    assert check_blend("mean") == "mean" and check_blend("gaussian") == "gaussian"
    assert check_blend("mean", large_file=True, merge=False) == "mean"          # the default path is never refused
    with pytest.raises(ValueError, match="blend"):
        check_blend("gauss")
    with pytest.raises(ValueError, match="large_file"):
        check_blend("gaussian", large_file=True)
    with pytest.raises(ValueError, match="merge=True"):
        check_blend("gaussian", merge=False)


def test_entry_points_refuse_before_any_upload(monkeypatch, tmp_path):
    calls = []
    monkeypatch.setattr(P, "_dist_ctx", lambda: calls.append("dist") or (0, 0, 1))
    monkeypatch.setattr(P, "load_learner", lambda *a, **k: calls.append("load"))
    raster = np.ones((1, 40, 40), np.uint8)
    for kw in ({"blend": "median"}, {"blend": "gaussian", "large_file": True}):
        with pytest.raises(ValueError):
            P.predict_raster(object(), raster, 16, 0.2, **kw)
    for kw in ({"merge": True, "blend": "median"}, {"merge": True, "blend": "gaussian", "large_file": True},
               {"merge": False, "blend": "gaussian"}):
        with pytest.raises(ValueError):
            P.save_predictions(tmp_path / "m.pkl", tmp_path, False, **kw)
    assert not calls


# ------------------------------------------------------------------------------------------------------------ ABI

def test_header_declares_and_library_exports_the_blend_entry_points():
    from unet_amd import _lib as L
    syms = L.declared_symbols()
    for s in ("unet_mosaic_accumulate_windows_weighted", "unet_mosaic_accumulate_weighted", "unet_mosaic_finalize_rows_weighted"):
        assert s in syms, s
        assert hasattr(L.lib, s), s
    assert L.lib.unet_abi_version() == 8
    assert "#define UNET_ABI_VERSION 8" in L.HEADER.read_text()


# ------------------------------------------------------------------------------------------------------------ params_and_main

def test_params_and_main_passes_blend_only_when_set(monkeypatch):
    import params_and_main as M
    import predict
    import train
    import create_tiles_unet
    assert M.BLEND == "mean"
    calls = {}
    monkeypatch.setattr(create_tiles_unet, "split_raster", lambda **kw: None)
    monkeypatch.setattr(train, "train_func", lambda *a: None)
    monkeypatch.setattr(predict, "save_predictions", lambda *a, **k: calls.setdefault("predict", (a, k)))
    monkeypatch.setattr(M, "Create_tiles", False); monkeypatch.setattr(M, "Train", False); monkeypatch.setattr(M, "Predict", True)
    monkeypatch.setattr(M, "enable_extra_parameters", True)
    M.main()
    a, k = calls.pop("predict")
    assert len(a) == 11 and k == {"tta": None}                                  # the default call, exactly as before
    monkeypatch.setattr(M, "BLEND", "gaussian")
    M.main()
    a, k = calls.pop("predict")
    assert len(a) == 11 and k == {"tta": None, "blend": "gaussian"}
    monkeypatch.setattr(M, "enable_extra_parameters", False)                    # reset with the other extra parameters
    M.main()
    a, k = calls.pop("predict")
    assert len(a) == 11 and k == {"tta": None} and M.BLEND == "mean"


# ------------------------------------------------------------------------------------------------------------ N-rank schedule: bounds

def _holes(wins: np.ndarray) -> np.ndarray:
    i = np.arange(len(wins))
    drop = ((i * 7919) % 13 == 0) | ((i >= 380) & (i < 430)) | ((wins[:, 0] == wins[-1, 0]) & (wins[:, 1] < 5000))
    return wins[~drop]


def _bounds_run(monkeypatch, wins, H, W, size, world, batch, C=C5):
    fw = FakeWorld(world)
    ck = BlendCheckedOps(fw, numeric=False)
    ck.install(monkeypatch)
    ck.forbid_mean(monkeypatch)
    table = P.ops.window_table
    monkeypatch.setattr(P.ops, "window_table", lambda rows, device: table(rows, "cpu"))
    model = StubModel(C, fw, device="meta", numeric=False)
    src = FakeSource(torch.empty((4, 1, 1), dtype=torch.uint8))
    src.H, src.W = H, W
    places, MH, MW, oy, ox, rows = P._raster_plan(wins, size, H, W, batch)
    gtab = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)
    gtab = torch.cat([gtab, torch.zeros_like(gtab)], 1)

    def make_input(first, n, n_pad):
        P._check_batch(first, n, n_pad, len(rows))
        return P.ops.WindowBatch(src, gtab, first, n_pad, size, size)

    def rank(r):
        return P._run_merge(model, places, MH, MW, False, False, r, world, batch, make_input, "argmax", blend="gaussian")

    with monkeypatch.context() as m:
        def gather(self, part, planes):
            assert tuple(part.shape) == (self.hi - self.lo, MW), (part.shape, self.lo, self.hi)
            return None if self.rank else "rank0"
        m.setattr(P._Merge, "_gather_rows", gather)
        _, fw = run_ranks(world, rank, monkeypatch, fw)
    plan = MergePlan(places, MH, MW, world)
    check_schedule(fw, C)
    for r in range(world):
        mg = fw.merges[r]
        lo, hi = plan.own[r]
        assert mg.wsum is not None and tuple(mg.wsum.shape) == (max(hi - lo, 1), MW)
        assert set(mg._profiles) <= {size}                                      # one table per side length, uploaded once
        acc = fw.launches(r, "accumulate")
        assert all(x["weighted"] and x["wy"] == size and x["wx"] == size and x["row_hi"] == hi - lo for x in acc)
        assert sum(x["n"] for x in acc) == (plan.ranges[r][1] - plan.ranges[r][0] if hi > lo else 0)
        adds = fw.launches(r, "slab_add")
        want = plan.slabs(r + 1) if r + 1 < plan.active else []
        assert [(x["rows"], x["wy"], x["wx"]) for x in adds] == [(rr, size, size) for _, rr in want]
        fin = fw.launches(r, "finalize")
        assert len(fin) == (1 if hi > lo else 0) and all(x["weighted"] for x in fin)
    return plan


@pytest.mark.parametrize("kept", ["all", "holes"])
@pytest.mark.parametrize("world", [1, 2, 3, 4, 5, 6, 7, 8])
def test_cfg5_blended_plan_launches_in_bounds(monkeypatch, world, kept):
    """every launch of the blended cfg5 merge (20000 x 20000, 512 px, overlap 0.2, 2401 windows) stays inside its tensors"""
    H = W = 20000
    wins = sliding_windows(H, W, 512, 0.2)
    assert len(wins) == 2401
    if kept == "holes":
        wins = _holes(wins)
    for batch in (2, 16):
        _bounds_run(monkeypatch, wins, H, W, 512, world, batch)


# ------------------------------------------------------------------------------------------------------------ N-rank schedule: numbers

def _fakes(monkeypatch, fw, numeric=True):
    ck = BlendCheckedOps(fw, numeric=numeric)
    ck.install(monkeypatch)
    monkeypatch.setattr(P.ops, "WindowSource", FakeSource)
    monkeypatch.setattr(P.ops, "window_nonzero", fake_window_nonzero)
    return ck


def _predict_all_ranks(monkeypatch, raster, world, batch, C, size, overlap, blend, **kw):
    fw = FakeWorld(world)
    _fakes(monkeypatch, fw)
    model = StubModel(C, fw)
    out, fw = run_ranks(world, lambda r: P.predict_raster(model, raster, size, overlap, batch_size=batch, blend=blend, **kw), monkeypatch, fw)
    check_schedule(fw, C)
    return out


def _restated(raster, C, size, overlap, max_empty, regression, all_classes):
    """the blended merge of predict_raster in plain numpy float32: the stub's logits window by window, in merge order"""
    fw = FakeWorld(1)
    model = StubModel(C, fw)
    Cb, H, W = raster.shape
    wins = sliding_windows(H, W, size, overlap)
    nz = np.array([np.count_nonzero(raster[:, y:y + size, x:x + size]) for y, x in wins])
    wins = wins[~(nz < size * size * Cb * (1 - max_empty))]
    oy, ox = wins[:, 0].min(), wins[:, 1].min()
    MH, MW = wins[:, 0].max() + size - oy, wins[:, 1].max() + size - ox
    src = FakeSource(torch.from_numpy(raster))
    g = blend_profile(size)
    acc, cnt, ws = np.zeros((C, MH, MW), np.float32), np.zeros((MH, MW), np.int32), np.zeros((MH, MW), np.float32)
    for y, x in wins[merge_order(wins)]:
        tab = torch.tensor([[y, x, 0, 0]])
        z = model.forward_windows(P.ops.WindowBatch(src, tab, 0, 1, size, size)).view()[0].numpy()
        v = z if regression else BlendCheckedOps.softmax_f32(z)
        B.accumulate_weighted_f32(acc, cnt, ws, [np.moveaxis(v, 2, 0)], [(y - oy, x - ox)], [(g, g)])
    m, am = B.finalize_weighted(acc, cnt, ws, 0, MH, -9999.0 if regression else None)
    return m[0] if regression else (m if all_classes else am)


@pytest.mark.parametrize("geom", [
    # (bands, H, W, size, overlap, C, worlds, batches)
    (3, 157, 131, 32, 0.3, 5, (2, 3, 6), (1, 4)),
    (1, 97, 203, 24, 0.5, 2, (3, 5), (2, 7)),
    (4, 70, 66, 16, 0.2, 7, (6, 8), (16,)),
])
def test_blended_n_ranks_equal_one_rank_and_numpy(monkeypatch, geom):
    bands, H, W, size, overlap, C, worlds, batches = geom
    g = np.random.default_rng(H * W + 1)
    raster = g.integers(1, 250, (bands, H, W)).astype(np.uint8)
    raster[:, H // 3:H // 3 + size + 3, : W // 2] = 0                          # windows that max_empty drops
    kinds = (("argmax", {}), ("all", {"all_classes": True}), ("reg", {"regression": True}))
    want = {k: _restated(raster, C, size, overlap, 0.9, bool(kw.get("regression")), bool(kw.get("all_classes"))) for k, kw in kinds}
    mean = _predict_all_ranks(monkeypatch, raster, 1, batches[0], C, size, overlap, "mean", all_classes=True)
    assert not np.array_equal(mean, want["all"])                               # the weights matter
    for batch in batches:
        for k, kw in kinds:
            one = _predict_all_ranks(monkeypatch, raster, 1, batch, C, size, overlap, "gaussian", **kw)
            assert np.array_equal(one.view(np.uint8), want[k].view(np.uint8)), (batch, k)
            for world in worlds:
                got = _predict_all_ranks(monkeypatch, raster, world, batch, C, size, overlap, "gaussian", **kw)
                assert got.dtype == one.dtype and np.array_equal(got.view(np.uint8), one.view(np.uint8)), (world, batch, k)


def test_two_tile_sizes_through_run_merge(monkeypatch):
    """save_predictions' case: tiles of two sizes in one merge (one profile table per side length), N ranks == 1 rank == numpy"""
    C, MH, MW = 4, 75, 64
    g = np.random.default_rng(3)
    places = [(y, x, 16, 16) for y in range(0, MH - 16 + 1, 11) for x in range(0, MW - 16 + 1, 12)]
    places += [(y + 3, x + 2, 12, 20) for y in range(0, MH - 16, 17) for x in range(0, MW - 22, 19)]
    places = np.array(places, dtype=np.int64)
    places = places[merge_order(places)]
    raster = g.integers(1, 250, (3, MH + 8, MW + 24)).astype(np.uint8)
    rows = [[int(y), int(x), 0, 0] for y, x, _, _ in places] + [[0, 0, 0, 0]] * 16

    def run(world, batch, want):
        fw = FakeWorld(world)
        _fakes(monkeypatch, fw)
        model = StubModel(C, fw)
        src = FakeSource(torch.from_numpy(raster))
        tab = torch.tensor(rows)

        def make_input(first, n, n_pad):
            P._check_batch(first, n, n_pad, len(rows))
            h, w = (int(v) for v in places[first, 2:])
            return P.ops.WindowBatch(src, tab, first, n_pad, h, w)

        out, fw = run_ranks(world, lambda r: P._run_merge(model, places, MH, MW, False, False, r, world, batch, make_input, want,
                                                          blend="gaussian"), monkeypatch, fw)
        check_schedule(fw, C)
        assert all(set(mg._profiles) <= {12, 16, 20} for mg in fw.merges.values())
        return out

    # numpy restatement
    fw = FakeWorld(1)
    model = StubModel(C, fw)
    src = FakeSource(torch.from_numpy(raster))
    acc, cnt, ws = np.zeros((C, MH, MW), np.float32), np.zeros((MH, MW), np.int32), np.zeros((MH, MW), np.float32)
    for y, x, h, w in places:
        z = model.forward_windows(P.ops.WindowBatch(src, torch.tensor([[y, x, 0, 0]]), 0, 1, int(h), int(w))).view()[0].numpy()
        B.accumulate_weighted_f32(acc, cnt, ws, [np.moveaxis(BlendCheckedOps.softmax_f32(z), 2, 0)], [(y, x)],
                                  [(blend_profile(h), blend_profile(w))])
    ref, ref_am = B.finalize_weighted(acc, cnt, ws, 0, MH)
    for batch in (1, 3, 16):
        one = run(1, batch, "all")
        assert np.array_equal(one.view(np.uint32), ref.view(np.uint32)), batch
        for world in (2, 3, 5):
            got = run(world, batch, "all")
            assert np.array_equal(got.view(np.uint32), one.view(np.uint32)), (world, batch)
            assert np.array_equal(run(world, batch, "argmax"), ref_am), (world, batch)
