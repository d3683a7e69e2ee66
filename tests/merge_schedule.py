"""Every rank of an N-rank merged prediction in ONE process, on the product code (predict._run_merge / _Merge, predict_raster).

The ranks run in descending order with predict._dist / predict._exchange replaced by an in-process fake: the sendbuf of rank r is recorded
and served to rank r - 1 (which must ask for exactly its size), the strips sent to rank 0 are recorded and served to it the same way.
The _Merge of every rank is recorded (and may be modified through `on_merge`, e.g. to put its buffers into guard-banded allocations).

CheckedOps: bounds-checking stand-ins for the ops launches of the merge.  Each one records the launch and asserts that everything it
would touch lies inside its tensor; with numeric=True it also does the arithmetic in numpy (float32, fixed order), so an N-rank run can
be compared with the 1-rank run bit for bit on a machine without a GPU."""
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

import predict as P
from unet_amd import ops

import merge_ref as R


@dataclass
class FakeWorld:
    world: int
    backend: str = "gloo"
    on_merge: Optional[Callable] = None
    rank: int = 0
    merges: Dict[int, object] = field(default_factory=dict)
    log: Dict[int, List[tuple]] = field(default_factory=dict)
    slabs: Dict[int, torch.Tensor] = field(default_factory=dict)
    parts: Dict[int, torch.Tensor] = field(default_factory=dict)

    # -- torch.distributed, as far as _Merge._gather_rows uses it
    def get_backend(self):
        return self.backend

    def send(self, t, dst):
        assert dst == 0 and self.rank != 0 and self.rank not in self.parts, (self.rank, dst)
        self.parts[self.rank] = t.clone()

    def recv(self, buf, src):
        assert self.rank == 0 and src in self.parts, (self.rank, src, sorted(self.parts))
        got = self.parts.pop(src)
        assert got.shape == buf.shape and got.dtype == buf.dtype, (src, got.shape, buf.shape)
        buf.copy_(got)

    # -- predict._exchange
    def exchange(self, send, dst, recv_numel, src, dtype, device):
        r = self.rank
        self.record("exchange", send=None if send is None else send.numel(), recv=recv_numel)
        if send is not None and send.numel():
            assert dst == r - 1 and r not in self.slabs
            self.slabs[r] = send.clone()
        sent = self.slabs.pop(src, None)
        want = 0 if sent is None else sent.numel()
        assert recv_numel == want, f"rank {r} expects {recv_numel} floats from rank {src}, which sent {want}"
        return None if not recv_numel else sent.to(device)

    def record(self, what, **kw):
        self.log.setdefault(self.rank, []).append((what, kw))

    def launches(self, rank, what=None):
        return [kw for w, kw in self.log.get(rank, []) if what is None or w == what]


def run_ranks(world: int, fn: Callable[[int], object], monkeypatch, fw: Optional[FakeWorld] = None):
    """fn(rank) for rank = world - 1 .. 0 under the fake world; returns (rank 0's result, the FakeWorld)"""
    fw = fw or FakeWorld(world)
    base = P._Merge

    class RecordingMerge(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            fw.merges[self.rank] = self
            if fw.on_merge is not None:
                fw.on_merge(self)

    monkeypatch.setattr(P, "_Merge", RecordingMerge)
    monkeypatch.setattr(P, "_dist", lambda: fw)
    monkeypatch.setattr(P, "_exchange", fw.exchange)
    out = None
    for r in reversed(range(world)):
        fw.rank = r
        monkeypatch.setattr(P, "_dist_ctx", lambda r=r: (r, 0, world))
        res = fn(r)
        if r == 0:
            out = res
        else:
            assert res is None, f"rank {r} returned a result"
    assert not fw.slabs and not fw.parts, ("sent but never received", sorted(fw.slabs), sorted(fw.parts))
    monkeypatch.setattr(P, "_Merge", base)
    return out, fw


def check_schedule(fw: FakeWorld, C: int):
    """what every rank did agrees with its plan: slab writes tile its sendbuf exactly, inactive ranks issued nothing"""
    for r, mg in fw.merges.items():
        plan = mg.plan
        if r >= plan.active:
            assert not fw.log.get(r), f"inactive rank {r} issued {fw.log[r]}"
            continue
        lo = plan.own[r][0]
        want = []
        off = 0
        for i, rows in plan.slabs(r):
            y0, _, h, w = (int(v) for v in plan.places[i])
            assert 1 <= rows <= h and y0 + rows == min(y0 + h, lo), (r, i, y0, h, rows, lo)
            want.append((off, C * rows * w, rows))
            off += C * rows * w
        n = 0 if mg.sendbuf is None else mg.sendbuf.numel()
        assert n == off == plan.slab_floats(r, C)
        got = sorted((kw["off"], kw["numel"], kw["rows"]) for kw in fw.launches(r, "slab"))
        assert got == want, f"rank {r}: slab writes {got[:4]}... != plan {want[:4]}..."


def _in_storage(t: torch.Tensor, what: str):
    end = t.storage_offset() + t.numel()
    cap = t.untyped_storage().nbytes() // t.element_size()
    assert t.storage_offset() >= 0 and end <= cap, f"{what}: elements [{t.storage_offset()}, {end}) of a storage of {cap}"


class CheckedOps:
    """bounds-checking fakes of the ops the merge launches (install with monkeypatch)"""

    def __init__(self, fw: FakeWorld, numeric: bool):
        self.fw, self.numeric = fw, numeric

    def install(self, monkeypatch):
        for name in ("mosaic_accumulate_windows", "softmax_argmax", "nhwc_to_nchw", "mosaic_accumulate", "mosaic_finalize_rows"):
            monkeypatch.setattr(ops, name, getattr(self, name))

    def _slab(self, z: ops.TS, out: torch.Tensor):
        mg = self.fw.merges.get(self.fw.rank)
        if mg is not None and mg.sendbuf is not None and out._base is mg.sendbuf:
            assert z.N == 1 and out.shape == (1, z.C, z.H, z.W), (z.N, out.shape)
            self.fw.record("slab", off=out.storage_offset(), numel=out.numel(), rows=z.H)

    @staticmethod
    def softmax_f32(z: np.ndarray) -> np.ndarray:
        """[..., C] float32 logits -> float32 probabilities, one fixed order of operations"""
        e = np.exp(z - z.max(axis=-1, keepdims=True))
        return (e / e.sum(axis=-1, keepdims=True, dtype=np.float32)).astype(np.float32)

    def mosaic_accumulate_windows(self, z, table, first, n, origin, mosaic, count, row_lo, row_hi, raw=False):
        Cc, MH, MW = mosaic.shape
        assert Cc == z.C and tuple(count.shape) == (MH, MW) and z.N >= n >= 1
        assert 0 <= first and first + n <= table.shape[0], (first, n, table.shape)
        assert 0 <= row_lo < row_hi <= MH, (row_lo, row_hi, MH)
        wins = table[first:first + n, :2].cpu().numpy().astype(np.int64) if table.device.type != "meta" else None
        self.fw.record("accumulate", first=first, n=n, row_lo=row_lo, row_hi=row_hi)
        if wins is None:
            return
        X = wins[:, 1] - int(origin[1])
        assert (X >= 0).all() and (X + z.W <= MW).all(), ("window outside the mosaic's columns", X, z.W, MW)
        if self.numeric:
            zz = z.view()[:n].numpy()
            v = zz if raw else self.softmax_f32(zz)
            R.accumulate_f32(mosaic.numpy(), count.numpy(), list(np.moveaxis(v, 3, 1)), wins.tolist(), tuple(origin), row_lo, row_hi)

    def softmax_argmax(self, z, probs, amax):
        assert probs is not None and amax is None
        assert probs.is_contiguous() and probs.numel() == z.N * z.C * z.H * z.W, (probs.shape, z.N, z.C, z.H, z.W)
        _in_storage(probs, "softmax_argmax probs")
        self._slab(z, probs)
        if self.numeric:
            probs.view(z.N, z.C, z.H, z.W).copy_(torch.from_numpy(np.moveaxis(self.softmax_f32(z.view().numpy()), 3, 1)))

    def nhwc_to_nchw(self, z, out):
        assert out.is_contiguous() and out.numel() == z.N * z.C * z.H * z.W
        _in_storage(out, "nhwc_to_nchw out")
        self._slab(z, out)
        if self.numeric:
            out.view(z.N, z.C, z.H, z.W).copy_(z.view().permute(0, 3, 1, 2))

    def mosaic_accumulate(self, probs, mosaic, count, y0, x0):
        Cc, th, tw = probs.shape
        _, MH, MW = mosaic.shape
        assert Cc == mosaic.shape[0] and 0 <= y0 and y0 + th <= MH and 0 <= x0 and x0 + tw <= MW, \
            f"slab [{y0}, {y0 + th}) x [{x0}, {x0 + tw}) outside the strip of {MH} x {MW}"
        self.fw.record("slab_add", y0=y0, rows=th)
        if self.numeric:
            R.accumulate_f32(mosaic.numpy(), count.numpy(), [probs.numpy()], [(y0, x0)])

    def mosaic_finalize_rows(self, mosaic, count, row0, nrows, amax, fill=None):
        _, MH, MW = mosaic.shape
        assert 0 <= row0 and 0 < nrows and row0 + nrows <= MH
        assert amax is None or (amax.numel() == nrows * MW and amax.dtype == torch.uint8), (amax.shape, nrows, MW)
        self.fw.record("finalize", row0=row0, nrows=nrows)
        if self.numeric:
            m, am = R.finalize(mosaic.numpy(), count.numpy(), row0, nrows, fill)
            mosaic.copy_(torch.from_numpy(m))
            if amax is not None:
                amax.view(nrows, MW).copy_(torch.from_numpy(am))


class FakeSource:
    """ops.WindowSource on a host tensor (the real one needs a device tensor)"""

    def __init__(self, data: torch.Tensor, div255_twice: bool = False):
        assert data.dim() in (3, 4) and data.dtype in ops.RASTER_TYPES
        self.data, self.rtype, self.div2 = data, ops.RASTER_TYPES[data.dtype], int(bool(div255_twice))
        self.C, self.H, self.W = data.shape[-3:]
        self.src_stride = 0 if data.dim() == 3 else self.C * self.H * self.W
        self.sources = 1 if data.dim() == 3 else data.shape[0]


def check_windows_inside(table: np.ndarray, th, tw, H, W, sources=1, what="window"):
    t = np.asarray(table).reshape(-1, 4)
    assert (t[:, 0] >= 0).all() and (t[:, 1] >= 0).all(), what
    assert (t[:, 0] + th <= H).all() and (t[:, 1] + tw <= W).all(), f"{what}: a window reaches past the {H} x {W} source"
    assert (t[:, 2] >= 0).all() and (t[:, 2] < sources).all(), what


def fake_window_nonzero(src, table, th, tw):
    t = table.cpu().numpy()
    check_windows_inside(t, th, tw, src.H, src.W, getattr(src, "sources", 1), "window_nonzero")
    a = src.data.numpy()
    return torch.tensor([int(np.count_nonzero(a[:, y:y + th, x:x + tw])) for y, x in t[:, :2]], dtype=torch.int64)


class StubModel:
    """a model whose forward_windows checks its WindowBatch and returns fp32 NHWC logits of n_pad windows.
    numeric: logits from the window's samples and its table row (a function of the window alone, so any batch cut gives the same)."""

    def __init__(self, C, fw: FakeWorld, device="cpu", numeric=True, cs=None, co=0):
        self.n_out, self._device, self.fw, self.numeric = C, torch.device(device), fw, numeric
        self.cs, self.co = (ops.rup4(C) if cs is None else cs), co
        self._buf = None

    def forward_windows(self, wb):
        src = wb.src
        assert 0 <= wb.first and wb.first + wb.n <= wb.table.shape[0], (wb.first, wb.n, wb.table.shape)
        self.fw.record("gather", first=wb.first, n_pad=wb.n)
        shape = (wb.n, wb.th, wb.tw, self.cs)
        if not self.numeric:
            if wb.table.device.type != "meta":
                check_windows_inside(wb.table[wb.first:wb.first + wb.n].cpu().numpy(), wb.th, wb.tw, src.H, src.W, src.sources, "gather")
            if self._buf is None or tuple(self._buf.shape) != shape:
                self._buf = torch.empty(shape, dtype=torch.float32, device=self._device)
            return ops.TS(self._buf, self.co, self.n_out)
        t = wb.table[wb.first:wb.first + wb.n].cpu().numpy()
        check_windows_inside(t, wb.th, wb.tw, src.H, src.W, src.sources, "gather")
        a = src.data.numpy()
        buf = np.full(shape, 7.25, dtype=np.float32)
        for j, (y, x, s, _) in enumerate(t):
            win = R.scale(R.cut(a if a.ndim == 3 else a[s], y, x, wb.th, wb.tw), bool(src.div2))
            for c in range(self.n_out):
                buf[j, :, :, self.co + c] = win[c % win.shape[0]] * np.float32(1 + c) + np.float32(0.125 * ((y // 7 + x // 5 + c) % 4))
        return ops.TS(torch.from_numpy(buf), self.co, self.n_out)
