"""CPU suite: the N-rank merge schedule of predict_raster as the product code runs it (predict._run_merge / _Merge and predict_raster's
own window tables), every rank of a world in one process (tests/merge_schedule.py), with bounds-checking fakes over the device launches.

* bounds: the cfg5 geometry (20000 x 20000, windows of 512, overlap 0.2 -- the plan of the round-5 six-rank abort) for several worlds and
  batch sizes, all windows and a kept subset with holes; tensors live on the meta device, nothing is allocated or computed;
* numbers: small odd rasters through predict_raster end to end with numpy arithmetic in the fakes -- N ranks == 1 rank bit for bit;
* the host checks of the window tables: a window outside the source or a batch outside the table raises ValueError before any launch."""
import numpy as np
import pytest
import torch

import predict as P
from unet_amd.mosaic import MergePlan, sliding_windows

from merge_schedule import CheckedOps, FakeSource, FakeWorld, StubModel, check_schedule, fake_window_nonzero, run_ranks

C5 = 5      # cfg5: xresnet34 4 -> 5 classes


def _holes(wins: np.ndarray) -> np.ndarray:
    """a deterministic max_empty-style drop: whole runs of windows (some at a rank boundary of world 6) and a scatter"""
    i = np.arange(len(wins))
    drop = ((i * 7919) % 13 == 0) | ((i >= 380) & (i < 430)) | ((wins[:, 0] == wins[-1, 0]) & (wins[:, 1] < 5000))
    return wins[~drop]


def _bounds_run(monkeypatch, wins, H, W, size, world, batch, C=C5):
    """the launches of every rank of predict_raster's merge for these kept windows, on the meta device"""
    fw = FakeWorld(world)
    CheckedOps(fw, numeric=False).install(monkeypatch)
    table = P.ops.window_table
    monkeypatch.setattr(P.ops, "window_table", lambda rows, device: table(rows, "cpu"))      # tables stay readable for the checks
    model = StubModel(C, fw, device="meta", numeric=False)
    src = FakeSource(torch.empty((4, 1, 1), dtype=torch.uint8))
    src.H, src.W = H, W
    places, MH, MW, oy, ox, rows = P._raster_plan(wins, size, H, W, batch)
    gtab = torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)
    gtab = torch.cat([gtab, torch.zeros_like(gtab)], 1)     # (y0, x0, source 0, 0), kept on the host to be checked

    def make_input(first, n, n_pad):
        P._check_batch(first, n, n_pad, len(rows))
        return P.ops.WindowBatch(src, gtab, first, n_pad, size, size)

    def rank(r):
        return P._run_merge(model, places, MH, MW, False, False, r, world, batch, make_input, "argmax")

    with monkeypatch.context() as m:
        # the real _gather_rows copies the strips to the host: on the meta device only their extents are checked
        def gather(self, part, planes):
            assert tuple(part.shape) == (self.hi - self.lo, MW), (part.shape, self.lo, self.hi)
            fw.record("strip", rows=self.hi - self.lo)
            return None if self.rank else "rank0"
        m.setattr(P._Merge, "_gather_rows", gather)
        _, fw = run_ranks(world, rank, monkeypatch, fw)
    plan = MergePlan(places, MH, MW, world)
    check_schedule(fw, C)
    gathered = []
    for r in range(world):
        g = fw.launches(r, "gather")
        a, b = plan.ranges[r]
        assert [x["first"] for x in g] == [f for f, _ in plan.batches(r, batch)]
        n_pad = max((n for _, n in plan.batches(r, batch)), default=0)
        assert all(x["n_pad"] == n_pad and x["first"] + n_pad <= len(rows) for x in g)
        gathered += list(range(a, b))
        ex = fw.launches(r, "exchange")
        if r < plan.active and plan.active > 1:
            assert len(ex) == 1 and ex[0]["recv"] == (plan.slab_floats(r + 1, C) if r + 1 < plan.active else 0)
        else:
            assert not ex
        acc = fw.launches(r, "accumulate")
        lo, hi = plan.own[r]
        assert all(x["row_lo"] == 0 and x["row_hi"] == hi - lo for x in acc)
        assert sum(x["n"] for x in acc) == (b - a if hi > lo else 0)
        assert len(fw.launches(r, "slab_add")) == len(plan.slabs(r + 1) if r + 1 < plan.active else [])
    assert gathered == list(range(len(places)))       # every window predicted once, by one rank
    return plan, fw


@pytest.mark.parametrize("kept", ["all", "holes"])
@pytest.mark.parametrize("world", [1, 2, 3, 5, 6, 8])
def test_cfg5_plan_launches_in_bounds(monkeypatch, world, kept):
    """every launch of the cfg5 merge stays inside its tensors, for every rank, at batch 1, 2, 3 and 16"""
    H = W = 20000
    wins = sliding_windows(H, W, 512, 0.2)
    if kept == "holes":
        wins = _holes(wins)
    for batch in (1, 2, 3, 16):
        _bounds_run(monkeypatch, wins, H, W, 512, world, batch)


def test_cfg5_world6_batch2_is_the_plan_of_the_round5_abort(monkeypatch):
    """the run that aborted once: every rank owns 400 windows (the last 401); its last batch is n = 1 padded to 2; ranks 1-5 hold
    90 / 82 / 74 / 66 / 58 slabs and rank 1 sends 266 MB, among them the 41 full 512-row slabs of window row 8"""
    wins = sliding_windows(20000, 20000, 512, 0.2)
    plan, fw = _bounds_run(monkeypatch, wins, 20000, 20000, 512, 6, 2)
    assert [b - a for a, b in plan.ranges] == [400] * 5 + [401]
    assert plan.batches(5, 2)[-1] == (2400, 1)
    assert [len(plan.slabs(r)) for r in range(1, 6)] == [90, 82, 74, 66, 58]
    assert plan.slab_floats(1, C5) * 4 == pytest.approx(266e6, rel=0.01)
    assert sum(rows == 512 for _, rows in plan.slabs(1)) == 41
    assert fw.launches(5, "gather")[-1] == {"first": 2400, "n_pad": 2}


def _predict_all_ranks(monkeypatch, raster, world, batch, C, size, overlap, max_empty=0.9, regression=False, all_classes=False,
                       cs=None, co=0):
    fw = FakeWorld(world)
    CheckedOps(fw, numeric=True).install(monkeypatch)
    monkeypatch.setattr(P.ops, "WindowSource", FakeSource)
    monkeypatch.setattr(P.ops, "window_nonzero", fake_window_nonzero)
    model = StubModel(C, fw, cs=cs, co=co)
    out, fw = run_ranks(world, lambda r: P.predict_raster(model, raster, size, overlap, max_empty=max_empty, batch_size=batch,
                                                          regression=regression, all_classes=all_classes), monkeypatch, fw)
    check_schedule(fw, C)
    return out


@pytest.mark.parametrize("geom", [
    # (bands, H, W, size, overlap, C, world list, batch list)
    (3, 157, 131, 32, 0.3, 5, (2, 3, 6, 8), (1, 3, 4)),
    (1, 97, 203, 24, 0.5, 2, (3, 5), (2, 7)),
    (4, 70, 66, 16, 0.2, 7, (6, 8, 40), (2, 16)),
])
def test_n_ranks_equal_one_rank_bit_for_bit(monkeypatch, geom):
    """predict_raster end to end with numpy arithmetic in the fakes: the mosaic assembled from N ranks' strips and slabs equals one
    rank's, for the argmax, all class planes and regression; a raster with empty (dropped) windows included"""
    bands, H, W, size, overlap, C, worlds, batches = geom
    g = np.random.default_rng(H * W)
    raster = g.integers(1, 250, (bands, H, W)).astype(np.uint8)
    raster[:, H // 3:H // 3 + size + 3, : W // 2] = 0                          # windows that max_empty drops: holes in the plan
    for batch in batches:
        ref = {k: _predict_all_ranks(monkeypatch, raster, 1, batch, C, size, overlap, **kw)
               for k, kw in (("argmax", {}), ("all", {"all_classes": True}), ("reg", {"regression": True}))}
        assert ref["argmax"].shape == ref["all"].shape[1:] and 0 < ref["argmax"].max() < C
        for world in worlds:
            for k, kw in (("argmax", {}), ("all", {"all_classes": True}), ("reg", {"regression": True})):
                got = _predict_all_ranks(monkeypatch, raster, world, batch, C, size, overlap, **kw)
                assert got.dtype == ref[k].dtype and np.array_equal(got.view(np.uint8), ref[k].view(np.uint8)), (world, batch, k)


def test_n_ranks_with_channel_offset_logits(monkeypatch):
    """the logits slice of the network output starts at a channel offset inside a wider buffer (z.co > 0, z.cs > C)"""
    g = np.random.default_rng(5)
    raster = g.integers(0, 200, (2, 90, 77)).astype(np.uint8)
    ref = _predict_all_ranks(monkeypatch, raster, 1, 3, 3, 20, 0.25, all_classes=True, cs=12, co=4)
    got = _predict_all_ranks(monkeypatch, raster, 5, 3, 3, 20, 0.25, all_classes=True, cs=12, co=4)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_window_tables_are_checked_on_the_host():
    """a window outside the source, or a batch outside its table, raises ValueError before anything is uploaded"""
    wins = np.array([[0, 0], [10, 20], [36, 0]])
    P._check_windows(wins, 64, 64, 100, 84)
    with pytest.raises(ValueError, match="window 2"):
        P._raster_plan(wins, 64, 99, 84, 4)                                   # 36 + 64 > 99: one row past the last
    with pytest.raises(ValueError, match="window 1"):
        P._check_windows(np.array([[0, 0], [0, 21]]), 64, 64, 100, 84)       # 21 + 64 > 84
    with pytest.raises(ValueError):
        P._check_windows(np.array([[-1, 0]]), 8, 8, 100, 84)
    with pytest.raises(ValueError, match="source"):
        P._check_windows([[0, 0, 3, 0]], 8, 8, 8, 8, sources=3)              # the staged-tile table: source index past the batch
    P._check_windows([[0, 0, 2, 0]], 8, 8, 8, 8, sources=3)
    P._check_batch(12, 1, 4, 16)
    with pytest.raises(ValueError):
        P._check_batch(13, 1, 4, 16)
    with pytest.raises(ValueError):
        P._check_batch(0, 5, 4, 16)


def test_predict_raster_rejects_a_bad_table_before_any_launch(monkeypatch):
    """predict_raster's own tables go through the check: a sliding-window rule that returned a window past the raster is refused"""
    fw = FakeWorld(1)
    CheckedOps(fw, numeric=True).install(monkeypatch)
    monkeypatch.setattr(P.ops, "WindowSource", FakeSource)
    calls = []
    monkeypatch.setattr(P.ops, "window_nonzero", lambda *a: calls.append(a))
    monkeypatch.setattr(P, "_dist_ctx", lambda: (0, 0, 1))
    monkeypatch.setattr(P, "sliding_windows", lambda H, W, size, overlap: np.array([[0, 0], [H - size + 1, 0]]))
    with pytest.raises(ValueError, match="window 1"):
        P.predict_raster(StubModel(2, fw), np.ones((1, 40, 40), np.uint8), 16, 0.2)
    assert not calls and not fw.log
