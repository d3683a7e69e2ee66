"""The merge-path kernels against a plain numpy / fp64 restatement (tests/merge_ref.py), every output inside a guard-banded allocation
(tests/guard.py) that is checked after every launch, every input raster inside canary bands.

  window_nonzero / window_gather   every raster type; windows flush with each edge, non-square, as wide as the raster, repeated; both
                                   destination types at a channel offset; the padded table of predict_raster; the batched staged
                                   source of save_predictions; the `slices` clamp of window_nonzero
  mosaic_accumulate_windows        raw mode bit-equal to the sequential float32 sum in placement order (overlaps inside one launch,
                                   63 / 64 / 65 / 129 windows across the MAXWIN chunks); softmax mode bit-equal to softmax_argmax's
                                   probabilities accumulated raw and close to fp64; the strip clipping _Merge uses; channel offsets
  mosaic_finalize_rows             a row range inside the mosaic, zero-count pixels with and without fill, exact ties
  slab writers                     softmax_argmax / nhwc_to_nchw into adjacent slabs of one sendbuf, as _Merge.add_batch cuts them
  nchw_to_nhwc(at=...)             the scalar-store writer at an unaligned channel, fp32 and bf16
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import merge_ref as R  # noqa: E402
from guard import canary_input, guarded, guarded_ts  # noqa: E402

RASTERS = [  # (torch type, numpy type, low, high): samples drawn in [low, high), never the canary
    (torch.uint8, np.uint8, 0, 250), (torch.uint16, np.uint16, 0, 65000), (torch.int16, np.int16, -30000, 30000),
    (torch.int32, np.int32, -1000000000, 1000000000), (torch.float32, np.float32, 0, 300),
]


def _ops():
    from unet_amd import ops
    return ops


def _raster(g, npdt, lo, hi, shape, zero_frac=0.3):
    a = (g.random(shape) * (hi - lo) + lo).astype(npdt) if npdt == np.float32 else g.integers(lo, hi, shape).astype(npdt)
    a[g.random(shape) < zero_frac] = 0
    return a


def _host(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(a.view(np.int16)).view(torch.uint16) if a.dtype == np.uint16 else torch.from_numpy(a)


def _table(rows):
    return _ops().window_table([list(r) + [0] * (4 - len(r)) for r in rows], "cuda")


# ------------------------------------------------------------------------------------------------------------ window_nonzero / gather

@pytest.mark.parametrize("tdt,npdt,lo,hi", RASTERS, ids=[str(r[1].__name__) for r in RASTERS])
def test_window_nonzero_and_gather_at_the_edges(tdt, npdt, lo, hi):
    ops = _ops()
    g = np.random.default_rng(11)
    C, H, W = 3, 90, 70
    a = _raster(g, npdt, lo, hi, (C, H, W))
    data, check_in = canary_input(_host(a))
    div2 = npdt == np.uint16
    src = ops.WindowSource(data, div255_twice=div2)
    for th, tw, wins in (
            (61, 37, [(0, 0), (H - 61, W - 37), (0, W - 37), (H - 61, 0), (13, 17), (H - 61, W - 37)]),   # flush with every edge, repeats
            (20, W, [(H - 20, 0), (0, 0), (35, 0)]),                                                        # as wide as the raster
            (H, 1, [(0, W - 1), (0, 0)])):
        tab = _table(wins)
        nz = ops.window_nonzero(src, tab, th, tw).cpu().numpy()
        assert nz.tolist() == [int(np.count_nonzero(R.cut(a, y, x, th, tw))) for y, x in wins], (th, tw)
        # the padded table of predict_raster: n real windows, then repeats of the last one up to n_pad
        n = len(wins)
        ptab = _table(wins + [wins[-1]] * 3)
        for adt, cs, co in ((torch.float32, 12, 4), (torch.bfloat16, 16, 8)):
            buf, check = guarded((n + 2, th, tw, cs), adt, fill=7.0)
            ops.window_gather(src, ptab, n - 1, 3, th, tw, buf, co)          # last real window + 2 repeats
            ops.window_gather(src, ptab, 0, n - 1, th, tw, buf[3:], co)
            check(f"gather {npdt.__name__} {adt}")
            got = buf.cpu()
            order = [wins[-1]] * 3 + wins[:n - 1]
            for j, (y, x) in enumerate(order[:n + 2]):
                want = torch.from_numpy(R.scale(R.cut(a, y, x, th, tw), div2)).permute(1, 2, 0).to(adt)
                assert torch.equal(got[j, :, :, co:co + C], want), (npdt, adt, j)
            rest = torch.cat([got[..., :co], got[..., co + C:]], -1)
            assert bool((rest == 7.0).all()), "lanes outside the gathered slice were written"
    check_in("raster")


def test_gather_from_the_batched_staged_source():
    """save_predictions' form: staged tiles [n, C, h, w] (src_stride != 0), table (0, 0, j)"""
    ops = _ops()
    g = np.random.default_rng(5)
    for tdt, npdt, lo, hi in RASTERS:
        a = _raster(g, npdt, lo, hi, (5, 4, 40, 36))
        data, check_in = canary_input(_host(a))
        src = ops.WindowSource(data, div255_twice=npdt == np.uint16)
        assert src.src_stride == 4 * 40 * 36
        tab = _table([(0, 0, j) for j in range(5)])
        buf, check = guarded((5, 40, 36, 8), torch.float32, fill=7.0)
        ops.window_gather(src, tab, 0, 5, 40, 36, buf, 4)
        check("staged gather")
        nz = ops.window_nonzero(ops.WindowSource(data[4]), _table([(0, 0)]), 40, 36).cpu().item()
        assert nz == int(np.count_nonzero(a[4]))
        for j in range(5):
            want = torch.from_numpy(R.scale(a[j], npdt == np.uint16)).permute(1, 2, 0)
            assert torch.equal(buf[j, :, :, 4:].cpu(), want), (npdt, j)
        assert bool((buf[..., :4] == 7.0).all())
        check_in("staged source")


@pytest.mark.parametrize("bands,th,tw", [(1, 1024, 1023), (1, 1024, 1024), (1, 1024, 1025), (4, 512, 512), (5, 512, 512), (2, 3, 5)])
def test_window_nonzero_slices(bands, th, tw):
    """bands * th * tw below, at and above 64 * 16384 samples, where the per-window slice count is clamped to 64"""
    ops = _ops()
    g = np.random.default_rng(th + tw)
    H, W = th + 9, tw + 6
    a = _raster(g, np.uint8, 0, 250, (bands, H, W), zero_frac=0.5)
    data, check_in = canary_input(_host(a))
    wins = [(0, 0), (H - th, W - tw), (9, 0), (0, 6)]
    nz = ops.window_nonzero(ops.WindowSource(data), _table(wins), th, tw).cpu().numpy()
    assert nz.tolist() == [int(np.count_nonzero(R.cut(a, y, x, th, tw))) for y, x in wins]
    check_in()


# ------------------------------------------------------------------------------------------------------------ mosaic_accumulate_windows

def _logits(g, N, th, tw, C, cs, co, scale=3.0):
    z, check = guarded_ts(N, th, tw, C, cs, co, fill=7.25)
    v = (g.standard_normal((N, th, tw, C)) * scale).astype(np.float32)
    z.view().copy_(torch.from_numpy(v))
    return z, v, check


def _acc(z, wins, first, n, origin, MH, MW, row_lo, row_hi, raw, C):
    ops = _ops()
    mosaic, cm = guarded((C, MH, MW), torch.float32, fill=0.0)
    count, cc = guarded((MH, MW), torch.int32, fill=0)
    ops.mosaic_accumulate_windows(z, _table(wins), first, n, origin, mosaic, count, row_lo, row_hi, raw=raw)
    cm("mosaic")
    cc("count")
    return mosaic.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_accumulate_raw_is_the_sequential_f32_sum(n):
    """windows overlap inside one launch (and across the 64-window chunks): every pixel sums in placement order"""
    g = np.random.default_rng(n)
    C, th, tw, MH, MW = 3, 7, 5, 30, 41
    z, v, zc = _logits(g, n + 2, th, tw, C, 8, 4)
    wins = [(int(g.integers(0, MH - th + 1)), int(g.integers(0, MW - tw + 1))) for _ in range(n)]
    wins[n // 2:n // 2 + 2] = [wins[0]] * len(wins[n // 2:n // 2 + 2])       # repeats
    wins = sorted(wins)
    got_m, got_c = _acc(z, wins, 0, n, (0, 0), MH, MW, 0, MH, True, C)
    ref_m, ref_c = R.accumulate_f32(np.zeros((C, MH, MW), np.float32), np.zeros((MH, MW), np.int32),
                                    [v[k].transpose(2, 0, 1) for k in range(n)], wins)
    assert n == 1 or ref_c.max() >= 3
    assert np.array_equal(got_c, ref_c)
    assert np.array_equal(got_m.view(np.uint32), ref_m.view(np.uint32))
    zc("z")


@pytest.mark.parametrize("C", [1, 2, 5, 64])
def test_accumulate_softmax_matches_softmax_argmax_and_fp64(C):
    ops = _ops()
    g = np.random.default_rng(C)
    n, th, tw, MH, MW = 70, 9, 6, 24, 31
    cs = ops.rup4(C) + 8
    z, v, zc = _logits(g, n, th, tw, C, cs, 4)
    wins = sorted((int(g.integers(0, MH - th + 1)), int(g.integers(0, MW - tw + 1))) for _ in range(n))
    got_m, got_c = _acc(z, wins, 0, n, (0, 0), MH, MW, 0, MH, False, C)
    # the kernel's promise: softmax mode == softmax_argmax's probabilities accumulated in raw mode
    probs = torch.empty((n, C, th, tw), dtype=torch.float32, device="cuda")
    ops.softmax_argmax(z, probs, None)
    pz, pc = guarded_ts(n, th, tw, C, cs, 0)
    pz.view().copy_(probs.permute(0, 2, 3, 1))
    raw_m, raw_c = _acc(pz, wins, 0, n, (0, 0), MH, MW, 0, MH, True, C)
    pc("probs TS")
    assert np.array_equal(got_c, raw_c) and np.array_equal(got_m.view(np.uint32), raw_m.view(np.uint32))
    p64 = R.softmax64(v)
    ref = np.zeros((C, MH, MW))
    for k, (y, x) in enumerate(wins):
        ref[:, y:y + th, x:x + tw] += p64[k].transpose(2, 0, 1)
    assert np.abs(got_m - ref).max() <= 2e-6 * max(1, got_c.max()), np.abs(got_m - ref).max()
    zc("z")


def test_accumulate_strip_clipping_as_merge_uses_it():
    """a strip of rows [lo, lo + rows) of the full mosaic with origin (lo, 0), row_lo = 0, row_hi = rows: windows entirely above,
    partly above, inside, partly below the strip and partly past MW"""
    g = np.random.default_rng(2)
    C, th, tw, MW, lo, rows = 5, 10, 8, 29, 23, 17
    wins = [(0, 0), (5, 21), (18, 3), (18, 3), (25, 10), (33, 0), (35, 25), (40, 12)]        # sorted by row, like a plan
    n = len(wins)
    z, v, zc = _logits(g, n, th, tw, C, 12, 4)
    for raw in (True, False):
        got_m, got_c = _acc(z, wins, 0, n, (lo, 0), rows, MW, 0, rows, raw, C)
        vals = v if raw else R.softmax64(v).astype(np.float32)
        ref_m, ref_c = R.accumulate_f32(np.zeros((C, rows, MW), np.float32), np.zeros((rows, MW), np.int32),
                                        [vals[k].transpose(2, 0, 1) for k in range(n)], wins, (lo, 0), 0, rows)
        assert np.array_equal(got_c, ref_c)
        if raw:
            assert np.array_equal(got_m.view(np.uint32), ref_m.view(np.uint32))
        else:
            assert np.abs(got_m - ref_m).max() <= 4e-6
    # a launch that starts in the middle of the table (first > 0) and a row range narrower than the strip
    got_m, got_c = _acc(z, [(0, 0)] * 3 + wins, 3, n, (lo, 0), rows, MW, 2, rows - 3, True, C)
    ref_m, ref_c = R.accumulate_f32(np.zeros((C, rows, MW), np.float32), np.zeros((rows, MW), np.int32),
                                    [v[k].transpose(2, 0, 1) for k in range(n)], wins, (lo, 0), 2, rows - 3)
    assert np.array_equal(got_c, ref_c) and np.array_equal(got_m.view(np.uint32), ref_m.view(np.uint32))
    zc("z")


def test_accumulate_rejects_65_classes_without_launching():
    from unet_amd import _lib as L
    ops = _ops()
    g = np.random.default_rng(0)
    z, _, zc = _logits(g, 2, 4, 4, 65, 68, 0)
    mosaic, cm = guarded((65, 8, 8), torch.float32, fill=0.0)
    count, cc = guarded((8, 8), torch.int32, fill=0)
    with pytest.raises(L.UnetHipError):
        ops.mosaic_accumulate_windows(z, _table([(0, 0), (4, 4)]), 0, 2, (0, 0), mosaic, count, 0, 8)
    torch.cuda.synchronize()
    assert not bool(mosaic.any()) and not bool(count.any())
    cm(), cc(), zc()


# ------------------------------------------------------------------------------------------------------------ mosaic_finalize_rows

@pytest.mark.parametrize("fill", [None, -9999.0])
def test_finalize_rows(fill):
    ops = _ops()
    g = np.random.default_rng(4)
    C, MH, MW, row0, nrows = 4, 20, 33, 5, 9
    m = (g.random((C, MH, MW)) * 3).astype(np.float32)
    cnt = g.integers(0, 4, (MH, MW)).astype(np.int32)
    cnt[row0 + 2, :7] = 0
    # exact ties: two classes share the maximum -> the first one, as np.argmax
    m[:, row0, :5] = np.array([0.25, 0.75, 0.5, 0.75], np.float32)[:, None]
    m[:, row0 + 1, :5] = np.array([0.0, 0.0, 0.0, 0.0], np.float32)[:, None]
    m[:, row0 + 3, :5] = np.array([0.1, 0.6, 0.6, 0.6], np.float32)[:, None] * 3
    cnt[row0, :5], cnt[row0 + 1, :5], cnt[row0 + 3, :5] = 1, 2, 3
    mosaic, cm = guarded((C, MH, MW), torch.float32, fill=0.0)
    count, cc = guarded((MH, MW), torch.int32, fill=0)
    mosaic.copy_(torch.from_numpy(m))
    count.copy_(torch.from_numpy(cnt))
    am, ca = guarded((nrows * MW,), torch.uint8, fill=0xAB)
    ops.mosaic_finalize_rows(mosaic, count, row0, nrows, am, fill=fill)
    cm("mosaic"), cc("count"), ca("argmax")
    ref_m, ref_am = R.finalize(m, cnt, row0, nrows, fill)
    assert np.array_equal(mosaic.cpu().numpy().view(np.uint32), ref_m.view(np.uint32))      # rows outside [row0, row0 + nrows) untouched
    got = am.cpu().numpy().reshape(nrows, MW)
    assert np.array_equal(got, ref_am)
    assert got[0, :5].tolist() == [1] * 5 and got[1, :5].tolist() == [0] * 5 and got[3, :5].tolist() == [1] * 5


# ------------------------------------------------------------------------------------------------------------ slab writers

def test_slab_writers_into_one_sendbuf():
    """_Merge.add_batch: rows [0, r) of window j -> sendbuf[off:off + C*r*w].view(1, C, r, w), several adjacent slabs"""
    ops = _ops()
    g = np.random.default_rng(8)
    C, th, tw = 5, 12, 9
    slabs = [(0, 4), (1, 12), (2, 1), (1, 7)]
    z, v, zc = _logits(g, 3, th, tw, C, 12, 4)
    total = sum(C * r * tw for _, r in slabs)
    for raw in (False, True):
        send, sc = guarded((total,), torch.float32, fill=float("nan"))
        off = 0
        for j, r in slabs:
            out = send[off:off + C * r * tw].view(1, C, r, tw)
            zs = ops.TS(z.buf[j:j + 1, :r], z.co, z.C)
            ops.nhwc_to_nchw(zs, out) if raw else ops.softmax_argmax(zs, out, None)
            sc(f"sendbuf after slab {off}")
            off += C * r * tw
        got = send.cpu().numpy()
        assert not np.isnan(got).any()
        off = 0
        for j, r in slabs:
            s = got[off:off + C * r * tw].reshape(C, r, tw)
            want = v[j, :r].transpose(2, 0, 1)
            if raw:
                assert np.array_equal(s, want)
            else:
                assert np.abs(s - R.softmax64(v[j, :r]).transpose(2, 0, 1)).max() <= 1e-6
            off += C * r * tw
    zc("z")


# ------------------------------------------------------------------------------------------------------------ nchw_to_nhwc(at=...)

@pytest.mark.parametrize("dt,cs", [(torch.float32, 108), (torch.bfloat16, 112)])
def test_nchw_to_nhwc_at_unaligned_channel(dt, cs):
    ops = _ops()
    g = torch.Generator().manual_seed(1)
    N, C, H, W, at = 2, 6, 9, 11, 102
    x = torch.randn((N, C, H, W), generator=g).cuda()
    y, check = guarded_ts(N, H, W, cs, cs, 0, dtype=dt, fill=7.25)
    ops.nchw_to_nhwc(x, y, at=at)
    check("nchw_to_nhwc at")
    got = y.buf.cpu()
    assert torch.equal(got[..., at:at + C], x.cpu().permute(0, 2, 3, 1).to(dt))
    assert bool((got[..., :at] == 7.25).all()) and bool((got[..., at + C:] == 7.25).all())
