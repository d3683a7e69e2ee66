"""Guard-banded device allocations: a tensor sits in the middle of one flat allocation whose two bands hold a sentinel, so a store
past either end of the tensor -- one row, one image or one window too far -- lands in a band instead of in a neighbouring
caching-allocator block, and check() sees it.  The bands are compared bitwise (viewed as integers), so a NaN sentinel works too.

For INPUTS the bands hold a loud canary instead (CANARY: a non-zero value of every raster type that the tests never use as a sample),
so that a read outside the tensor shows up in counts or gathered values."""
import math

import torch

from unet_amd import ops

MIN_GUARD_BYTES = 64 * 1024

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}

# canaries of the raster sample types: the tests draw samples below these (integers) or as small non-negative floats
CANARY = {torch.uint8: 251, torch.uint16: 65021, torch.int16: -31111, torch.int32: -1999999999, torch.float32: -3.0e7}


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(_INT_VIEW[t.element_size()])


def default_guard(shape, dtype) -> int:
    """elements per band: one full image / row-plane of the tensor (everything but its leading dimension), never under 64 KiB"""
    es = torch.empty((), dtype=dtype).element_size()
    plane = math.prod(shape[1:]) if len(shape) > 1 else math.prod(shape)
    return max(int(plane), -(-MIN_GUARD_BYTES // es))


def guarded(shape, dtype, device="cuda", fill=0, guard=None):
    """(contiguous tensor of `shape`, check) inside one flat allocation of numel + 2 * guard elements, all of it set to `fill`.
    check() asserts that both bands still hold the bits of `fill`."""
    shape = tuple(int(s) for s in shape)
    n = math.prod(shape)
    g = default_guard(shape, dtype) if guard is None else int(guard)
    flat = torch.empty(n + 2 * g, dtype=dtype, device=device)
    want = _bits(torch.full((1,), fill, dtype=dtype))
    _bits(flat).fill_(int(want.item()))
    t = flat[g:g + n].view(shape)

    def check(what=""):
        bits = _bits(flat)
        for name, band in (("leading", bits[:g]), ("trailing", bits[g + n:])):
            bad = (band != want.to(band.device)).nonzero()
            assert bad.numel() == 0, (f"{what}: {bad.numel()} element(s) of the {name} guard band overwritten, first at "
                                      f"{int(bad[0]) if name == 'trailing' else int(bad[0]) - g} relative to the tensor's "
                                      f"{'end' if name == 'trailing' else 'start'}")

    return t, check


def guarded_ts(N, H, W, C, cs=None, co=0, dtype=torch.float32, device="cuda", fill=7.25, guard=None):
    """(ops.TS [N, H, W, cs] slice (co, C), check) inside a guard-banded allocation; the whole buffer starts at `fill`"""
    cs = ops.rupv(C, dtype) if cs is None else cs
    buf, check = guarded((N, H, W, cs), dtype, device, fill, guard)
    return ops.TS(buf, co, C), check


def canary_input(a: torch.Tensor, device="cuda", guard=None):
    """device copy of the host tensor `a` inside an allocation whose bands hold CANARY[a.dtype]; returns (tensor, check)"""
    t, check = guarded(a.shape, a.dtype, device, CANARY[a.dtype], guard)
    t.copy_(a.to(device))
    return t, check
