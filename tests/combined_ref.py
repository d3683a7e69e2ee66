"""fp64 restatement of ``CombinedLoss(axis=1, smooth, alpha, gamma, reduction, square_in_union, weight)`` = focal + alpha * Dice, used by the
CombinedLoss tests (the oracle package stays as it is).  Written per class with explicit comparisons, independently of
``unet_amd.learner``:

    focal = 1 / P * sum over the pixels whose target is a class c of (1 - exp(-ce)) ** gamma * ce,   ce = w[c] * (logsumexp(z) - z_c)
            (P counts ALL pixels; a target outside [0, C) adds nothing to the sum),
    dice  = sum over (sample, class) of 1 - (2 I + smooth) / (U + smooth),  I = sum p t,  U = sum (p + t)  [sum (p^2 + t)], 'mean': / (B C),
            t = [target == c] (a target outside [0, C) equals no class)."""
import torch


def combined_terms_ref(pred: torch.Tensor, targ: torch.Tensor, smooth: float = 1.0, gamma: float = 2.0, reduction: str = "sum",
                       square_in_union: bool = False, weight=None, dtype=torch.float64):
    """(focal, dice) as scalars; pred [B,C,H,W] (autograd flows back to it), targ [B,H,W] int, weight [C] or None.  dtype = torch.float32
    evaluates the same expressions in fp32: the rounding floor a test may allow an fp32 kernel."""
    assert reduction in ("sum", "mean")
    B, C = pred.shape[:2]
    z = pred.to(dtype)
    lse = torch.logsumexp(z, dim=1)                     # [B,H,W]
    p = torch.exp(z - lse.unsqueeze(1))                 # softmax
    focal = z.new_zeros(())
    terms = []
    for c in range(C):
        hit = targ == c                                # -100, C, ... never equal any class
        t = hit.to(dtype)
        w = 1.0 if weight is None else float(weight[c])
        # the pixels of class c only, and of those the ones with 1 - exp(-ce) > 0: where it is 0 (one class; a logit margin beyond the exp
        # range) the value is 0 and so is the limit of its derivative, which autograd would return as 0 * inf for gamma < 1.  Elsewhere a
        # harmless 1 goes through the power and is multiplied by 0.
        ce = w * (lse - z[:, c])
        live = hit & ((1.0 - torch.exp(-ce.detach())) > 0)
        ce = torch.where(live, ce, torch.ones_like(lse))
        focal = focal + ((1.0 - torch.exp(-ce)) ** gamma * ce * live.to(dtype)).sum()
        pc = p[:, c]
        inter = (pc * t).flatten(1).sum(1)
        union = ((pc * pc if square_in_union else pc) + t).flatten(1).sum(1)
        terms.append(1.0 - (2.0 * inter + smooth) / (union + smooth))
    dice = torch.stack(terms, dim=1).sum()              # over [B, C]
    if reduction == "mean":
        dice = dice / (B * C)
    return focal / targ.numel(), dice


def combined_loss_ref(pred: torch.Tensor, targ: torch.Tensor, smooth: float = 1.0, alpha: float = 1.0, gamma: float = 2.0,
                      reduction: str = "sum", square_in_union: bool = False, weight=None, dtype=torch.float64) -> torch.Tensor:
    focal, dice = combined_terms_ref(pred, targ, smooth, gamma, reduction, square_in_union, weight, dtype)
    return focal + alpha * dice
