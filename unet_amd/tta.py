"""Test-time augmentation (TTA) codes: the 8 symmetries of the square (the dihedral group D4) as they act on a [..., H, W] tensor.

A TTA set is an ordered tuple of distinct codes.  Its prediction for one window is the mean, in code order, of
g^-1(softmax(f(g(x)))) (regression: of the raw outputs), summed in fp32 and divided by k once; it replaces the window's softmax
probabilities everywhere (overlap merge, per-tile outputs, rank-to-rank slabs, the int8 large_file merge).  On the device the
orientation is an index permutation inside the window gather / input staging (unet_window_gather_oriented,
unet_nchw_to_nhwc_oriented) and inside the accumulate (unet_tta_accumulate); nothing is interpolated.

    code  g(x)                                   inverse
    0     x                                      0
    1     torch.flip(x, [-1])                    1
    2     torch.flip(x, [-2])                    2
    3     torch.flip(x, [-2, -1])                3
    4     x.transpose(-2, -1)                    4
    5     torch.rot90(x, 1, (-2, -1))            6
    6     torch.rot90(x, -1, (-2, -1))           5
    7     torch.flip(x.transpose(-2, -1), [-2, -1])  7
"""
from __future__ import annotations

from typing import Iterable, Optional, Tuple, Union

import torch

INVERSE = (0, 1, 2, 3, 4, 6, 5, 7)
FLIPS = (0, 1, 2, 3)
D4 = (0, 1, 2, 3, 4, 5, 6, 7)

TTASpec = Union[None, str, Iterable[int]]


def orient(x: torch.Tensor, code: int) -> torch.Tensor:
    """g(x) of the table (host / torch restatement; the device kernels implement the same permutations)"""
    if code == 0:
        return x
    if code == 1:
        return torch.flip(x, [-1])
    if code == 2:
        return torch.flip(x, [-2])
    if code == 3:
        return torch.flip(x, [-2, -1])
    if code == 4:
        return x.transpose(-2, -1)
    if code == 5:
        return torch.rot90(x, 1, (-2, -1))
    if code == 6:
        return torch.rot90(x, -1, (-2, -1))
    if code == 7:
        return torch.flip(x.transpose(-2, -1), [-2, -1])
    raise ValueError(f"TTA code {code!r} is not one of 0..7")


def unorient(x: torch.Tensor, code: int) -> torch.Tensor:
    """g^-1(x)"""
    return orient(x, INVERSE[code])


def parse(tta: TTASpec, shapes: Iterable[Tuple[int, int]] = ()) -> Optional[Tuple[int, ...]]:
    """None | "flips" | "d4" | a sequence of distinct codes -> tuple of codes (None stays None).  `shapes`: the (h, w) of every window
    or tile the set will be applied to -- codes 4..7 (transposes and quarter turns) need square ones."""
    if tta is None:
        return None
    if isinstance(tta, str):
        if tta == "flips":
            codes = FLIPS
        elif tta == "d4":
            codes = D4
        else:
            raise ValueError(f"tta={tta!r}: expected None, 'flips', 'd4' or a tuple of D4 codes 0..7")
    else:
        try:
            codes = tuple(int(c) for c in tta)
        except TypeError:
            raise ValueError(f"tta={tta!r}: expected None, 'flips', 'd4' or a tuple of D4 codes 0..7") from None
        if any(isinstance(c, bool) for c in tta) or any(not 0 <= c <= 7 for c in codes):
            raise ValueError(f"tta={tta!r}: codes must lie in 0..7")
        if len(set(codes)) != len(codes):
            raise ValueError(f"tta={tta!r}: codes must be distinct")
        if not codes:
            raise ValueError("tta=(): an empty TTA set predicts nothing; use tta=None")
    if any(c >= 4 for c in codes):
        bad = sorted({(int(h), int(w)) for h, w in shapes if int(h) != int(w)})
        if bad:
            raise ValueError(f"tta={tta!r}: codes 4..7 (transposes, quarter turns) need square windows, got {bad[0][0]} x {bad[0][1]}; "
                             f"use tta=\"flips\" for non-square tiles")
    return codes
