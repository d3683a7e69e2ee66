"""Gaussian window blending (blend="gaussian") on the device:

  6-8  the weighted kernels against the numpy float32 restatement (tests/blend_ref.py), bit for bit, every tensor inside a guard-banded
       allocation (tests/guard.py) checked after every launch: the batched accumulate in raw and softmax mode (overlaps inside one launch,
       63 / 64 / 65 / 129 windows across the 64-window chunks, strip clipping, non-square windows), the slab add, the finalisation;
  9    a profile of ones makes blend="gaussian" the mean path bit for bit (argmax, all classes, regression, tta="flips"; 1 and 3 ranks);
  10   xresnet18 in fp32 and bf16 storage against a float64 weighted mean of the device's own per-window logits;
  11   N ranks == 1 rank bit for bit on the real kernels (every rank in one process, tests/merge_schedule.py);
  12   save_predictions(merge=True) over split_raster's tiles == predict_raster, with and without tta;
  13   regression: the weighted mean of the raw values, -9999 where no window was kept;
  14   predict_raster without blend= is blend="mean"."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import predict as P  # noqa: E402
from unet_amd.mosaic import blend_profile, sliding_windows  # noqa: E402

import blend_ref as B  # noqa: E402
import merge_ref as R  # noqa: E402
from guard import guarded, guarded_ts  # noqa: E402
from merge_schedule import FakeWorld, run_ranks  # noqa: E402


def _ops():
    from unet_amd import ops
    return ops


def _table(rows):
    return _ops().window_table([list(r) + [0] * (4 - len(r)) for r in rows], "cuda")


def _logits(g, N, th, tw, C, cs, co, scale=3.0):
    z, check = guarded_ts(N, th, tw, C, cs, co, fill=7.25)
    v = (g.standard_normal((N, th, tw, C)) * scale).astype(np.float32)
    z.view().copy_(torch.from_numpy(v))
    return z, v, check


def _prof(n, fill=float("nan")):
    """profile table of n entries inside a guarded allocation whose bands hold NaN: a read past it would poison the sums"""
    t, check = guarded((n,), torch.float32, fill=fill)
    t.copy_(torch.from_numpy(blend_profile(n)))
    return t, check


def _acc_w(z, wins, first, n, origin, MH, MW, row_lo, row_hi, raw, C, th, tw):
    ops = _ops()
    mosaic, cm = guarded((C, MH, MW), torch.float32, fill=0.0)
    count, cc = guarded((MH, MW), torch.int32, fill=0)
    wsum, cw = guarded((MH, MW), torch.float32, fill=0.0)
    wy, cy = _prof(th)
    wx, cx = _prof(tw)
    ops.mosaic_accumulate_windows_weighted(z, _table(wins), first, n, origin, mosaic, count, wsum, wy, wx, row_lo, row_hi, raw=raw)
    for c, what in ((cm, "mosaic"), (cc, "count"), (cw, "wsum"), (cy, "wy"), (cx, "wx")):
        c(what)
    return mosaic.cpu().numpy(), count.cpu().numpy(), wsum.cpu().numpy()


def _ref_w(vals, wins, th, tw, C, MH, MW, origin=(0, 0), row_lo=0, row_hi=None):
    """vals [n, C, th, tw] float32"""
    g = (blend_profile(th), blend_profile(tw))
    return B.accumulate_weighted_f32(np.zeros((C, MH, MW), np.float32), np.zeros((MH, MW), np.int32), np.zeros((MH, MW), np.float32),
                                     list(vals), wins, [g] * len(vals), origin, row_lo, row_hi)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.itemsize == 4 else a,
                                                                        b.view(np.uint32) if b.itemsize == 4 else b)


# ------------------------------------------------------------------------------------------------------------ 6. raw mode

@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("th,tw", [(7, 5), (12, 12)])
def test_weighted_accumulate_raw_is_the_sequential_f32_sum(n, th, tw):
    """windows overlap inside one launch and across the 64-window chunks: every pixel adds fl(w * v) in placement order"""
    g = np.random.default_rng(n * 100 + th)
    C, MH, MW = 3, 30, 41
    z, v, zc = _logits(g, n + 2, th, tw, C, 8, 4)
    wins = [(int(g.integers(0, MH - th + 1)), int(g.integers(0, MW - tw + 1))) for _ in range(n)]
    wins[n // 2:n // 2 + 2] = [wins[0]] * len(wins[n // 2:n // 2 + 2])       # repeats
    wins = sorted(wins)
    got = _acc_w(z, wins, 0, n, (0, 0), MH, MW, 0, MH, True, C, th, tw)
    ref = _ref_w(v[:n].transpose(0, 3, 1, 2), wins, th, tw, C, MH, MW)
    assert n == 1 or ref[1].max() >= 3
    assert np.array_equal(got[1], ref[1]) and _same(got[2], ref[2]) and _same(got[0], ref[0])
    zc("z")


def test_weighted_accumulate_strip_clipping():
    """a strip [lo, lo + rows) of the mosaic with origin (lo, 0): windows above, across, inside, below the strip; a launch that starts
    in the middle of the table and a row range narrower than the strip"""
    g = np.random.default_rng(2)
    C, th, tw, MW, lo, rows = 5, 10, 8, 29, 23, 17
    wins = [(0, 0), (5, 21), (18, 3), (18, 3), (25, 10), (33, 0), (35, 21), (40, 12)]
    n = len(wins)
    z, v, zc = _logits(g, n, th, tw, C, 12, 4)
    vals = v.transpose(0, 3, 1, 2)
    got = _acc_w(z, wins, 0, n, (lo, 0), rows, MW, 0, rows, True, C, th, tw)
    ref = _ref_w(vals, wins, th, tw, C, rows, MW, (lo, 0), 0, rows)
    assert all(_same(a, b) if a.dtype != np.int32 else np.array_equal(a, b) for a, b in zip(got, ref))
    got = _acc_w(z, [(0, 0)] * 3 + wins, 3, n, (lo, 0), rows, MW, 2, rows - 3, True, C, th, tw)
    ref = _ref_w(vals, wins, th, tw, C, rows, MW, (lo, 0), 2, rows - 3)
    assert all(_same(a, b) if a.dtype != np.int32 else np.array_equal(a, b) for a, b in zip(got, ref))
    zc("z")


def test_weighted_accumulate_rejects_65_classes_without_launching():
    from unet_amd import _lib as L
    ops = _ops()
    z, _, zc = _logits(np.random.default_rng(0), 2, 4, 4, 65, 68, 0)
    mosaic, cm = guarded((65, 8, 8), torch.float32, fill=0.0)
    count, cc = guarded((8, 8), torch.int32, fill=0)
    wsum, cw = guarded((8, 8), torch.float32, fill=0.0)
    wy, cy = _prof(4)
    with pytest.raises(L.UnetHipError):
        ops.mosaic_accumulate_windows_weighted(z, _table([(0, 0), (4, 4)]), 0, 2, (0, 0), mosaic, count, wsum, wy, wy, 0, 8)
    torch.cuda.synchronize()
    assert not bool(mosaic.any()) and not bool(count.any()) and not bool(wsum.any())
    cm(), cc(), cw(), cy(), zc()


# ------------------------------------------------------------------------------------------------------------ 7. softmax mode

@pytest.mark.parametrize("C", [1, 2, 5, 64])
def test_weighted_accumulate_softmax_weights_softmax_argmax(C):
    ops = _ops()
    g = np.random.default_rng(C)
    n, th, tw, MH, MW = 70, 9, 6, 24, 31
    cs = ops.rup4(C) + 8
    z, v, zc = _logits(g, n, th, tw, C, cs, 4)
    wins = sorted((int(g.integers(0, MH - th + 1)), int(g.integers(0, MW - tw + 1))) for _ in range(n))
    got = _acc_w(z, wins, 0, n, (0, 0), MH, MW, 0, MH, False, C, th, tw)
    probs = torch.empty((n, C, th, tw), dtype=torch.float32, device="cuda")
    ops.softmax_argmax(z, probs, None)
    ref = _ref_w(probs.cpu().numpy(), wins, th, tw, C, MH, MW)
    assert np.array_equal(got[1], ref[1]) and _same(got[2], ref[2]) and _same(got[0], ref[0])
    zc("z")


# ------------------------------------------------------------------------------------------------------------ 8. slab add, finalize

def test_weighted_slab_add():
    """the receiver's add of a slab: the top rr rows of a window of height h take rows [0, rr) of g_h; clipped at the strip edges"""
    ops = _ops()
    g = np.random.default_rng(8)
    C, h, w, MH, MW = 5, 12, 9, 14, 30
    slabs = [(4, 0, 0), (12, 2, 21), (1, 13, 5), (7, 7, 3), (7, 7, 3)]         # (rows, y0, x0); the last two repeat, one is clipped
    mosaic, cm = guarded((C, MH, MW), torch.float32, fill=0.0)
    count, cc = guarded((MH, MW), torch.int32, fill=0)
    wsum, cw = guarded((MH, MW), torch.float32, fill=0.0)
    wy, cy = _prof(h)
    wx, cx = _prof(w)
    init = (g.random((C, MH, MW)) * 2).astype(np.float32)
    mosaic.copy_(torch.from_numpy(init))
    ref = (init.copy(), np.zeros((MH, MW), np.int32), np.zeros((MH, MW), np.float32))
    for rr, y0, x0 in slabs:
        p = g.random((C, rr, w)).astype(np.float32)
        pd, cp = guarded((C, rr, w), torch.float32, fill=float("nan"))
        pd.copy_(torch.from_numpy(p))
        ops.mosaic_accumulate_weighted(pd, wy, wx, mosaic, count, wsum, y0, x0)
        for c, what in ((cm, "mosaic"), (cc, "count"), (cw, "wsum"), (cy, "wy"), (cx, "wx"), (cp, "slab")):
            c(what)
        B.accumulate_weighted_f32(*ref, [p], [(y0, x0)], [(blend_profile(h), blend_profile(w))])
    assert _same(mosaic.cpu().numpy(), ref[0]) and np.array_equal(count.cpu().numpy(), ref[1]) and _same(wsum.cpu().numpy(), ref[2])


@pytest.mark.parametrize("fill", [None, -9999.0])
def test_weighted_finalize_rows(fill):
    ops = _ops()
    g = np.random.default_rng(4)
    C, MH, MW, row0, nrows = 4, 20, 33, 5, 9
    m = (g.random((C, MH, MW)) * 3).astype(np.float32)
    cnt = g.integers(0, 4, (MH, MW)).astype(np.int32)
    ws = (g.random((MH, MW)) * 2 + 1e-3).astype(np.float32)
    cnt[row0 + 2, :7] = 0
    m[:, row0, :5] = np.array([0.25, 0.75, 0.5, 0.75], np.float32)[:, None]        # exact ties -> the first maximum
    m[:, row0 + 1, :5] = 0.0
    m[:, row0 + 3, :5] = np.array([0.1, 0.6, 0.6, 0.6], np.float32)[:, None] * 3
    cnt[row0, :5], cnt[row0 + 1, :5], cnt[row0 + 3, :5] = 1, 2, 3
    mosaic, cm = guarded((C, MH, MW), torch.float32, fill=0.0)
    count, cc = guarded((MH, MW), torch.int32, fill=0)
    wsum, cw = guarded((MH, MW), torch.float32, fill=0.0)
    mosaic.copy_(torch.from_numpy(m))
    count.copy_(torch.from_numpy(cnt))
    wsum.copy_(torch.from_numpy(ws))
    am, ca = guarded((nrows * MW,), torch.uint8, fill=0xAB)
    ops.mosaic_finalize_rows_weighted(mosaic, count, wsum, row0, nrows, am, fill=fill)
    cm("mosaic"), cc("count"), cw("wsum"), ca("argmax")
    ref_m, ref_am = B.finalize_weighted(m, cnt, ws, row0, nrows, fill)
    assert _same(mosaic.cpu().numpy(), ref_m)                                   # rows outside [row0, row0 + nrows) untouched
    got = am.cpu().numpy().reshape(nrows, MW)
    assert np.array_equal(got, ref_am)
    assert got[0, :5].tolist() == [1] * 5 and got[1, :5].tolist() == [0] * 5 and got[3, :5].tolist() == [1] * 5
    assert np.array_equal(wsum.cpu().numpy(), ws) and np.array_equal(count.cpu().numpy(), cnt)


# ------------------------------------------------------------------------------------------------------------ merges on real kernels

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
        if mg.wsum is not None:
            mg.wsum, c3 = guarded(mg.wsum.shape, torch.float32, fill=0.0)
            checks.append(c3)
        if mg.sendbuf is not None:
            mg.sendbuf, c4 = guarded(mg.sendbuf.shape, torch.float32, fill=float("nan"))
            checks.append(c4)
    return on


def _run(monkeypatch, model, raster, world, size, overlap, checks, **kw):
    fw = FakeWorld(world, on_merge=_guard_merge(checks))
    out, fw = run_ranks(world, lambda r: P.predict_raster(model, raster, size, overlap, **kw), monkeypatch, fw)
    for c in checks:
        c(f"world {world} {kw}")
    checks.clear()
    return out


def _model(arch, n_in, n_out, size, act_dtype="f32", seed=0):
    from unet_amd.model import HipDynamicUnet
    torch.manual_seed(seed)
    m = HipDynamicUnet(arch, n_in, n_out, (size, size), act_dtype=act_dtype)
    m.eval()
    return m


def test_profile_of_ones_is_the_mean_path(monkeypatch):
    """with every weight 1 the blended path adds the same numbers in the same order and divides by the same count: bit for bit"""
    model = _model("xresnet18", 4, 3, 64)
    raster = np.random.default_rng(9).integers(1, 256, (4, 190, 171)).astype(np.uint8)
    checks = []
    monkeypatch.setattr(P, "blend_profile", lambda n: np.ones(n, np.float32))
    for kw in ({}, {"all_classes": True}, {"tta": "flips"}, {"all_classes": True, "tta": "flips"}):
        for world in (1, 3):
            mean = _run(monkeypatch, model, raster, world, 64, 0.3, checks, batch_size=4, **kw)
            gauss = _run(monkeypatch, model, raster, world, 64, 0.3, checks, batch_size=4, blend="gaussian", **kw)
            assert _same(gauss, mean), (kw, world)
    reg = _model("xresnet18", 4, 1, 64, seed=1)
    for tta in (None, "flips"):
        for world in (1, 3):
            mean = _run(monkeypatch, reg, raster, world, 64, 0.3, checks, batch_size=4, regression=True, tta=tta)
            gauss = _run(monkeypatch, reg, raster, world, 64, 0.3, checks, batch_size=4, regression=True, tta=tta, blend="gaussian")
            assert _same(gauss, mean), (tta, world)


@pytest.mark.parametrize("act_dtype", ["f32", "bf16"])
def test_xresnet18_against_fp64_weighted_mean_of_its_own_logits(act_dtype):
    ops = _ops()
    size, bs = 128, 4
    model = _model("xresnet18", 4, 5, size, act_dtype)
    H, W = 330, 300
    raster = np.random.default_rng(3).integers(1, 256, (4, H, W)).astype(np.uint8)
    got = P.predict_raster(model, raster, size, 0.2, batch_size=bs, blend="gaussian", all_classes=True)
    am = P.predict_raster(model, raster, size, 0.2, batch_size=bs, blend="gaussian")
    mean = P.predict_raster(model, raster, size, 0.2, batch_size=bs, all_classes=True)
    # the device's own per-window logits, in the batches (and padding) predict_raster runs
    wins = sliding_windows(H, W, size, 0.2)
    src = ops.WindowSource(torch.from_numpy(raster).cuda())
    tab = ops.window_table(wins.tolist() + [wins[-1].tolist()] * bs, "cuda")
    g = blend_profile(size).astype(np.float64)
    w64 = g[:, None] * g[None, :]
    acc, ws = np.zeros((5, H, W)), np.zeros((H, W))
    for first in range(0, len(wins), bs):
        z = model.forward_windows(ops.WindowBatch(src, tab, first, bs, size, size)).view().cpu().numpy()
        for j in range(min(bs, len(wins) - first)):
            y, x = wins[first + j]
            acc[:, y:y + size, x:x + size] += w64 * R.softmax64(z[j]).transpose(2, 0, 1)
            ws[y:y + size, x:x + size] += w64
    ref = acc / ws
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 2e-6, np.abs(got - ref).max()
    top2 = np.sort(ref, axis=0)[-2:]
    sure = top2[1] - top2[0] > 1e-5
    assert sure.mean() > 0.9 and np.array_equal(am[sure], ref.argmax(0).astype(np.uint8)[sure])
    assert np.abs(mean - ref).max() > 1e-4                                      # the weights matter


@pytest.mark.parametrize("world", [2, 3, 6])
def test_n_ranks_equal_one_rank_on_the_device(monkeypatch, world):
    size, overlap, bands = 32, 0.25, 3
    H, W = 184, 105
    raster = np.random.default_rng(world).integers(1, 250, (bands, H, W)).astype(np.uint8)
    checks = []
    model = GatherModel(bands, checks)
    for batch in (2, 3):
        for kw in ({}, {"all_classes": True}):
            one = _run(monkeypatch, model, raster, 1, size, overlap, checks, batch_size=batch, blend="gaussian", **kw)
            got = _run(monkeypatch, model, raster, world, size, overlap, checks, batch_size=batch, blend="gaussian", **kw)
            assert _same(got, one), (world, batch, kw)
    # 1 rank against the numpy float32 restatement: the gathered channels' softmax weighted in placement order
    wins = sliding_windows(H, W, size, overlap)
    vals = [torch.softmax(torch.from_numpy(R.scale(R.cut(raster, y, x, size, size))), 0).numpy() for y, x in wins]
    ref = _ref_w(np.array(vals), wins.tolist(), size, size, bands, H, W)
    m, _ = B.finalize_weighted(*ref, 0, H)
    assert np.abs(one - m).max() <= 1e-6                                        # (torch's softmax is not the kernel's: close, not equal)


def test_regression_weighted_mean_with_fill(monkeypatch):
    """raw values (one band) weighted in placement order, bit for bit; -9999 where every window over a pixel was dropped"""
    size, overlap = 32, 0.25
    H, W = 120, 130
    raster = np.random.default_rng(13).integers(1, 250, (1, H, W)).astype(np.uint8)
    raster[:, :60, :60] = 0                                                     # windows (0, 0), (0, 24), (24, 0), (24, 24) dropped
    checks = []
    model = GatherModel(1, checks)
    got = _run(monkeypatch, model, raster, 1, size, overlap, checks, batch_size=3, regression=True, blend="gaussian", max_empty=0.5)
    wins = sliding_windows(H, W, size, overlap)
    keep = [(y, x) for y, x in wins if np.sum(raster[:, y:y + size, x:x + size] != 0) >= size * size * 0.5]
    assert (0, 0) not in keep and min(k[0] for k in keep) == 0 and min(k[1] for k in keep) == 0
    ref = _ref_w(np.array([R.scale(R.cut(raster, y, x, size, size)) for y, x in keep]), keep, size, size, 1, H, W)
    m, _ = B.finalize_weighted(*ref, 0, H, fill=-9999.0)
    assert got.dtype == np.float32 and _same(got, m[0])
    assert (got[:24, :24] == -9999.0).all() and (got[60:] != -9999.0).all()
    got3 = _run(monkeypatch, model, raster, 3, size, overlap, checks, batch_size=3, regression=True, blend="gaussian", max_empty=0.5)
    assert _same(got3, got)


def test_default_is_mean(monkeypatch):
    size, overlap, bands = 32, 0.25, 3
    raster = np.random.default_rng(1).integers(1, 250, (bands, 100, 90)).astype(np.uint8)
    checks = []
    model = GatherModel(bands, checks)
    for kw in ({}, {"all_classes": True}):
        a = _run(monkeypatch, model, raster, 1, size, overlap, checks, batch_size=4, **kw)
        b = _run(monkeypatch, model, raster, 1, size, overlap, checks, batch_size=4, blend="mean", **kw)
        assert _same(a, b), kw
    c = _run(monkeypatch, model, raster, 1, size, overlap, checks, batch_size=4, blend="gaussian", all_classes=True)
    assert not _same(a, c)


# ------------------------------------------------------------------------------------------------------------ 12. files == raster

def _export(tmp_path, model, n_out, size):
    from unet_amd.learner import CrossEntropyLossFlat, DataLoaders, Learner, TileDataset
    dls = DataLoaders(TileDataset([np.zeros((4, size, size), np.uint8)], None, "int8"), None, 1, device="cuda",
                      vocab=[str(i) for i in range(n_out)])
    learn = Learner(dls, model, loss_func=CrossEntropyLossFlat(axis=1), path=tmp_path)
    pkl = tmp_path / "m.pkl"
    learn.export(pkl)
    return pkl


def test_save_predictions_blended_equals_predict_raster(tmp_path):
    import create_tiles_unet as T
    from unet_amd.tiffio import read_tiff, write_tiff
    size = 128
    model = _model("xresnet18", 4, 3, size, seed=11)
    img = np.random.default_rng(5).integers(1, 250, (4, 400, 350)).astype(np.uint8)
    img[:, :130, :130] = 0
    rpath = tmp_path / "scene.tif"
    write_tiff(rpath, img, geotransform=(400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5))
    pkl = _export(tmp_path, model, 3, size)
    tiles = tmp_path / "cut"
    T.split_raster(rpath, None, tiles, patch_size=size, patch_overlap=0.2, split=[1], max_empty=0.9)
    for kw in ({}, {"all_classes": True}, {"tta": "flips"}):
        direct = P.predict_raster(model, rpath, size, 0.2, max_empty=0.9, batch_size=5, blend="gaussian", **kw)
        f = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, AOI="b", validation_vision=False, batch_size=5,
                               blend="gaussian", **kw)
        assert _same(read_tiff(f)[0], direct), kw
