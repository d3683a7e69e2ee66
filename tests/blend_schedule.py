"""Bounds-checking fakes of the three blended merge launches (ops.mosaic_accumulate_windows_weighted, ops.mosaic_accumulate_weighted,
ops.mosaic_finalize_rows_weighted) on top of merge_schedule.CheckedOps: each records the launch under the name of its unweighted
twin, asserts that everything it would touch -- profile tables included -- lies inside its tensor, and with numeric=True does the
float32 arithmetic of tests/blend_ref.py."""
import numpy as np
import torch

from unet_amd import ops

import blend_ref as B
from merge_schedule import CheckedOps


def _table_ok(t: torch.Tensor, n: int, what: str):
    assert t.dtype == torch.float32 and t.dim() == 1 and t.is_contiguous(), (what, t.dtype, t.shape)
    assert t.numel() >= n, f"{what}: a profile of {t.numel()} entries for {n} rows / columns"


class BlendCheckedOps(CheckedOps):
    def install(self, monkeypatch):
        super().install(monkeypatch)
        for name in ("mosaic_accumulate_windows_weighted", "mosaic_accumulate_weighted", "mosaic_finalize_rows_weighted"):
            monkeypatch.setattr(ops, name, getattr(self, name))

    @staticmethod
    def _wsum_ok(wsum, mosaic):
        _, MH, MW = mosaic.shape
        assert tuple(wsum.shape) == (MH, MW) and wsum.dtype == torch.float32, (wsum.shape, MH, MW)

    def mosaic_accumulate_windows_weighted(self, z, table, first, n, origin, mosaic, count, wsum, wy, wx, row_lo, row_hi, raw=False):
        Cc, MH, MW = mosaic.shape
        assert Cc == z.C and tuple(count.shape) == (MH, MW) and z.N >= n >= 1
        assert 0 <= first and first + n <= table.shape[0], (first, n, table.shape)
        assert 0 <= row_lo < row_hi <= MH, (row_lo, row_hi, MH)
        self._wsum_ok(wsum, mosaic)
        _table_ok(wy, z.H, "wy")
        _table_ok(wx, z.W, "wx")
        self.fw.record("accumulate", first=first, n=n, row_lo=row_lo, row_hi=row_hi, weighted=True, wy=wy.numel(), wx=wx.numel())
        if table.device.type == "meta":
            return
        wins = table[first:first + n, :2].cpu().numpy().astype(np.int64)
        X = wins[:, 1] - int(origin[1])
        assert (X >= 0).all() and (X + z.W <= MW).all(), ("window outside the mosaic's columns", X, z.W, MW)
        if self.numeric:
            zz = z.view()[:n].numpy()
            v = zz if raw else self.softmax_f32(zz)
            gy, gx = wy.numpy(), wx.numpy()
            B.accumulate_weighted_f32(mosaic.numpy(), count.numpy(), wsum.numpy(), list(np.moveaxis(v, 3, 1)), wins.tolist(),
                                      [(gy, gx)] * n, tuple(origin), row_lo, row_hi)

    def mosaic_accumulate_weighted(self, probs, wy, wx, mosaic, count, wsum, y0, x0):
        Cc, th, tw = probs.shape
        _, MH, MW = mosaic.shape
        assert Cc == mosaic.shape[0] and 0 <= y0 and y0 + th <= MH and 0 <= x0 and x0 + tw <= MW, \
            f"slab [{y0}, {y0 + th}) x [{x0}, {x0 + tw}) outside the strip of {MH} x {MW}"
        self._wsum_ok(wsum, mosaic)
        _table_ok(wy, th, "wy")
        _table_ok(wx, tw, "wx")
        self.fw.record("slab_add", y0=y0, rows=th, weighted=True, wy=wy.numel(), wx=wx.numel())
        if self.numeric:
            B.accumulate_weighted_f32(mosaic.numpy(), count.numpy(), wsum.numpy(), [probs.numpy()], [(y0, x0)], [(wy.numpy(), wx.numpy())])

    def mosaic_finalize_rows_weighted(self, mosaic, count, wsum, row0, nrows, amax, fill=None):
        _, MH, MW = mosaic.shape
        assert 0 <= row0 and 0 < nrows and row0 + nrows <= MH
        assert amax is None or (amax.numel() == nrows * MW and amax.dtype == torch.uint8), (amax.shape, nrows, MW)
        self._wsum_ok(wsum, mosaic)
        self.fw.record("finalize", row0=row0, nrows=nrows, weighted=True)
        if self.numeric:
            m, am = B.finalize_weighted(mosaic.numpy(), count.numpy(), wsum.numpy(), row0, nrows, fill)
            mosaic.copy_(torch.from_numpy(m))
            if amax is not None:
                amax.view(nrows, MW).copy_(torch.from_numpy(am))

    # the unweighted launches must not run in a blended merge
    def forbid_mean(self, monkeypatch):
        def no(name):
            def f(*a, **k):
                raise AssertionError(f"{name} launched in a blended merge")
            return f
        for name in ("mosaic_accumulate_windows", "mosaic_accumulate", "mosaic_finalize_rows"):
            monkeypatch.setattr(ops, name, no(name))
