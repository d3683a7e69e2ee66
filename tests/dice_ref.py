"""fp64 restatement of fastai ``DiceLoss(axis=1, smooth, reduction, square_in_union)`` used by the Dice tests (the oracle package stays
as it is).  Written per class with explicit comparisons, independently of ``unet_amd.learner.DiceLoss``."""
import torch


def dice_loss_ref(pred: torch.Tensor, targ: torch.Tensor, smooth: float = 1e-6, reduction: str = "sum",
                  square_in_union: bool = False) -> torch.Tensor:
    """pred [B,C,H,W] (any float dtype; computed in fp64, autograd flows back to pred), targ [B,H,W] int.  A target outside [0, C) has an
    all-zero one-hot row."""
    B, C = pred.shape[:2]
    p = torch.softmax(pred.double(), dim=1)
    terms = []
    for c in range(C):
        t = (targ == c).double()                       # -100, C, ... never equal any class
        pc = p[:, c]
        inter = (pc * t).flatten(1).sum(1)
        union = ((pc * pc if square_in_union else pc) + t).flatten(1).sum(1)
        terms.append(1.0 - (2.0 * inter + smooth) / (union + smooth))
    loss = torch.stack(terms, dim=1)                   # [B, C]
    if reduction == "mean":
        return loss.sum() / (B * C)
    assert reduction == "sum"
    return loss.sum()
