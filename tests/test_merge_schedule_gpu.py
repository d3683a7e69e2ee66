"""The N-rank merge schedule of predict_raster on the device: every rank of a world in one process (tests/merge_schedule.py) with the real
ops launches, each rank's mosaic, hit counter and sendbuf inside guard-banded allocations (tests/guard.py) that are checked after the run.

* a stub model whose forward gathers its windows with the real unet_window_gather into a guarded NHWC buffer and uses the gathered
  channels as logits: worlds 6 and 8 at batch 2 and 3 on rasters where every rank has slabs and a ragged last batch -- equal to the fp64
  merge, and N ranks == 1 rank bit for bit;
* the real xresnet18 network, world 6 at batch 2 with batch_invariant=True (the form of the round-5 six-rank run): == 1 rank bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import predict as P  # noqa: E402
from unet_amd.mosaic import MergePlan, sliding_windows  # noqa: E402

import merge_ref as R  # noqa: E402
from guard import guarded, guarded_ts  # noqa: E402
from merge_schedule import FakeWorld, run_ranks  # noqa: E402


class GatherModel:
    """forward_windows = the real window gather into a guarded NHWC buffer; the gathered channels are the logits"""

    def __init__(self, bands, checks):
        self.n_out, self._device, self.checks = bands, torch.device("cuda"), checks

    def forward_windows(self, wb):
        z, check = guarded_ts(wb.n, wb.th, wb.tw, self.n_out, 8, 4)
        wb.write(z.buf, z.co)
        self.checks.append(check)
        return z


def _guard_merge(checks):
    def on(mg):
        mg.mosaic, c1 = guarded(mg.mosaic.shape, mg.mosaic.dtype, fill=0)
        mg.count, c2 = guarded(mg.count.shape, mg.count.dtype, fill=0)
        checks.extend([c1, c2])
        if mg.sendbuf is not None:
            mg.sendbuf, c3 = guarded(mg.sendbuf.shape, torch.float32, fill=float("nan"))
            checks.extend([c3, lambda what="", s=mg.sendbuf: _all_written(s, what)])
    return on


def _all_written(sendbuf, what):
    assert not bool(sendbuf.isnan().any()), f"{what}: sendbuf not fully written"


def _run(monkeypatch, model, raster, world, batch, size, overlap, checks, **kw):
    fw = FakeWorld(world, on_merge=_guard_merge(checks))
    out, fw = run_ranks(world, lambda r: P.predict_raster(model, raster, size, overlap, batch_size=batch, **kw), monkeypatch, fw)
    for c in checks:
        c(f"world {world} batch {batch}")
    checks.clear()
    return out, fw


@pytest.mark.parametrize("world,H,W", [(6, 136, 105), (8, 184, 105)])
def test_stub_merge_over_n_ranks(monkeypatch, world, H, W):
    size, overlap, bands = 32, 0.25, 3
    g = np.random.default_rng(world)
    raster = g.integers(1, 250, (bands, H, W)).astype(np.uint8)
    wins = sliding_windows(H, W, size, overlap)
    places = np.concatenate([wins, np.full((len(wins), 2), size)], 1)
    plan = MergePlan(places, H, W, world)
    checks = []
    model = GatherModel(bands, checks)
    # fp64 reference: mean of the windows' softmax probabilities
    ref = np.zeros((bands, H, W))
    cnt = np.zeros((H, W))
    for y, x in wins:
        ref[:, y:y + size, x:x + size] += R.softmax64(R.scale(R.cut(raster, y, x, size, size)), axis=0)
        cnt[y:y + size, x:x + size] += 1
    ref /= cnt
    for batch in (2, 3):
        assert all(plan.batches(r, batch)[-1][1] < batch for r in range(world)) and all(plan.slabs(r) for r in range(1, world))
        one, _ = _run(monkeypatch, model, raster, 1, batch, size, overlap, checks, all_classes=True)
        assert np.abs(one - ref).max() <= 2e-6
        got, _ = _run(monkeypatch, model, raster, world, batch, size, overlap, checks, all_classes=True)
        assert np.array_equal(got.view(np.uint32), one.view(np.uint32)), (world, batch)
        am1, _ = _run(monkeypatch, model, raster, 1, batch, size, overlap, checks)
        amN, _ = _run(monkeypatch, model, raster, world, batch, size, overlap, checks)
        assert np.array_equal(amN, am1) and np.array_equal(am1, one.argmax(0).astype(np.uint8))


@pytest.mark.parametrize("H,W,active", [(1300, 1100, 4), (1140, 600, 6)])
def test_xresnet18_world6_batch2_equals_one_rank(monkeypatch, H, W, active):
    """1300 x 1100: six windows per row, seven per rank -- the plan falls back to four active ranks and two idle ones;
    1140 x 600: six active ranks, each with slabs and a last batch of one window padded to two"""
    from unet_amd.model import HipDynamicUnet
    torch.manual_seed(0)
    model = HipDynamicUnet("xresnet18", 4, 5, (256, 256))
    model.eval()
    g = np.random.default_rng(6)
    raster = g.integers(1, 256, (4, H, W)).astype(np.uint8)
    checks = []
    one, _ = _run(monkeypatch, model, raster, 1, 2, 256, 0.2, checks, batch_invariant=True)
    six, fw = _run(monkeypatch, model, raster, 6, 2, 256, 0.2, checks, batch_invariant=True)
    assert fw.merges[5].plan.active == active and all(fw.merges[r].sendbuf is not None for r in range(1, active))
    assert one.shape == (H, W) and len(np.unique(one)) > 1
    assert np.array_equal(six, one)
