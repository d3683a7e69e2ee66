"""CombinedLoss (focal + alpha * Dice, the compound loss fastai's documentation of DiceLoss ends with) without a GPU: the generic path against
the fp64 restatement (tests/combined_ref.py) and against the two losses it is made of, the constructor, the C ABI of the fused kernels, the
export / load_learner metadata and the arguments the fused path refuses before any launch."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from combined_ref import combined_loss_ref

ROOT = Path(__file__).resolve().parent.parent


def _case(C, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(3, C, 9, 7, generator=g, dtype=torch.float64) * 2.5
    y = torch.randint(0, C, (3, 9, 7), generator=g)
    y[0, 0, :3] = -100                               # outside [0, C): 0 to the focal sum (still counted), all-zero one-hot rows for Dice
    y[1, 2, 1:4] = C
    w = (torch.rand(C, generator=g) + 0.3)           # fp32: the loss keeps its class weights in fp32
    return z, y, w


@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("square_in_union", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_generic_path_matches_the_restatement(gamma, reduction, square_in_union, weighted):
    """value and autograd gradient in fp64 within 1e-10 relative; gamma = 0.5 with ignored targets: no NaN from the power at ce = 0"""
    from unet_amd.learner import CombinedLoss
    z, y, w = _case(5, int(10 * gamma) + 2 * square_in_union + weighted)
    smooth, alpha = (1.0, 0.7) if reduction == "sum" else (1e-6, 2.5)
    loss_fn = CombinedLoss(1, smooth, alpha, gamma=gamma, reduction=reduction, square_in_union=square_in_union, weight=w if weighted else None)
    z1 = z.clone().requires_grad_(True)
    z2 = z.clone().requires_grad_(True)
    got = loss_fn(z1, y)
    want = combined_loss_ref(z2, y, smooth, alpha, gamma, reduction, square_in_union, w.double() if weighted else None)
    got.backward()
    want.backward()
    assert torch.isfinite(z1.grad).all() and torch.isfinite(z2.grad).all()
    assert abs(got.item() - want.item()) <= 1e-10 * abs(want.item())
    assert (z1.grad - z2.grad).abs().max().item() <= 1e-10 * z2.grad.abs().max().item()


@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_alpha_zero_is_the_focal_loss_bit_for_bit(gamma):
    from unet_amd.learner import CombinedLoss, FocalLossFlat
    g = torch.Generator().manual_seed(5)
    z = torch.randn(2, 4, 11, 6, generator=g) * 2.0
    y = torch.randint(0, 4, (2, 11, 6), generator=g)
    w = torch.rand(4, generator=g) + 0.3
    got = CombinedLoss(alpha=0.0, gamma=gamma, weight=w)(z, y)
    want = FocalLossFlat(gamma=gamma, axis=1, weight=w)(z, y)
    assert torch.equal(got, want)


def test_gamma_zero_is_dice_plus_cross_entropy():
    """gamma = 0, alpha = 1, no class weights: the Dice + CE of nnU-Net"""
    from unet_amd.learner import CombinedLoss, DiceLoss
    g = torch.Generator().manual_seed(6)
    z = torch.randn(2, 4, 11, 6, generator=g, dtype=torch.float64) * 2.0
    y = torch.randint(0, 4, (2, 11, 6), generator=g)
    for reduction in ("sum", "mean"):
        got = CombinedLoss(1, 0.5, 1.0, gamma=0.0, reduction=reduction)(z, y)
        want = torch.nn.functional.cross_entropy(z, y) + DiceLoss(1, 0.5, reduction)(z, y)
        assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item())


def test_constructor_defaults_errors_and_surface():
    from unet_amd.learner import CombinedLoss, CrossEntropyLossFlat, DiceLoss
    c = CombinedLoss()
    assert (c.axis, c.smooth, c.alpha, c.gamma, c.reduction, c.square_in_union) == (1, 1.0, 1.0, 2.0, "sum", False)
    assert c.func.weight is None
    c = CombinedLoss(1, 0.5, 2.0)                      # fastai's three positional arguments
    assert (c.smooth, c.alpha) == (0.5, 2.0)
    with pytest.raises(TypeError):
        CombinedLoss(1, 0.5, 2.0, 3.0)                 # the rest is keyword-only
    assert not isinstance(c, (CrossEntropyLossFlat, DiceLoss))      # _focal_gamma / _dice must not route it as one of its parts
    with pytest.raises(ValueError):
        CombinedLoss(reduction="none")
    with pytest.raises(ValueError):
        CombinedLoss(alpha=-0.1)
    with pytest.raises(ValueError):
        CombinedLoss(gamma=-1.0)
    x = torch.randn(2, 4, 3, 3)
    assert torch.allclose(c.activation(x), torch.softmax(x, 1))
    assert torch.equal(c.decodes(x), x.argmax(1))


def test_assigned_class_weights_feed_the_focal_term():
    """train.py:211 assigns loss_func.func.weight for every loss object"""
    from unet_amd.learner import CombinedLoss
    z, y, w = _case(5, 3)
    c = CombinedLoss(gamma=2.0)
    plain = c(z, y).item()
    c.func.weight = w
    assert abs(c(z, y).item() - combined_loss_ref(z, y, weight=w.double()).item()) <= 1e-10 * abs(plain)
    assert abs(c(z, y).item() - plain) > 1e-3 * abs(plain)
    import train as T
    assert T.CombinedLoss is CombinedLoss


def test_header_declares_and_library_exports_the_combined_entry_points():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    ge.build()
    import unet_amd._lib as L
    want = {"unet_combined_workspace", "unet_combined_fwd", "unet_combined_bwd", "unet_combined_bwd_bf16"}
    assert want <= set(L.declared_symbols())
    for s in want:
        assert hasattr(L.lib, s), s
    # host-side query: B x blocks-per-sample partial rows of 2 C + 1 floats (I, U per class and the block's focal sum)
    assert L.lib.unet_combined_workspace(3, 37 * 29, 5) == 3 * 5 * 11
    assert L.lib.unet_combined_workspace(16, 512 * 512, 5) == 16 * 64 * 11
    assert L.lib.unet_combined_workspace(0, 10, 5) == 0
    # arguments are checked on the host before any launch: 65 classes, a negative gamma, a bad slice
    buf = torch.zeros(16)
    p = buf.data_ptr()
    assert L.lib.unet_combined_fwd(p, 68, 0, p, None, 1, 1, 65, 2.0, 1.0, 0, 0, p, p, p, None) != 0 and b"combined_fwd" in L.lib.unet_last_error()
    assert L.lib.unet_combined_fwd(p, 4, 0, p, None, 1, 1, 3, -1.0, 1.0, 0, 0, p, p, p, None) != 0 and b"combined_fwd" in L.lib.unet_last_error()
    assert L.lib.unet_combined_bwd(p, 4, 2, p, None, 1, 1, 3, 2.0, 0, p, 1.0, 1.0, p, 4, 0, None) != 0 and b"combined_bwd" in L.lib.unet_last_error()
    assert L.lib.unet_combined_bwd_bf16(p, 4, 0, p, None, 1, 1, 3, 2.0, 0, p, 1.0, 1.0, p, 4, 2, None) != 0 and b"combined_bwd" in L.lib.unet_last_error()


def _cpu_learner(tmp_path, loss, n_out=3):
    from unet_amd.learner import DataLoaders, DiceMulti, Learner, TileDataset
    from unet_amd.model import HipDynamicUnet
    model = HipDynamicUnet("xresnet18", 4, n_out, (64, 64), device="cpu")     # structure only
    dls = DataLoaders(TileDataset([np.zeros((4, 64, 64), np.uint8)], [np.zeros((64, 64), np.uint8)]), None, 1, device="cpu",
                      vocab=list("abc")[:n_out])
    return Learner(dls, model, loss_func=loss, metrics=[DiceMulti()], path=tmp_path)


def test_export_meta_round_trip_keeps_the_combined_loss(tmp_path):
    from unet_amd.learner import CombinedLoss, CrossEntropyLossFlat, DiceLoss, FocalLossFlat, _loss_from_meta
    loss = CombinedLoss(1, 0.25, 0.5, gamma=0.5, reduction="mean", square_in_union=True)
    loss.func.weight = torch.tensor([0.25, 0.5, 2.0])
    learn = _cpu_learner(tmp_path, loss)
    assert learn._combined is loss and learn._dice is None and learn._focal_gamma is None and not learn.regression
    assert torch.equal(learn._weights(), torch.tensor([0.25, 0.5, 2.0]))
    learn.export(tmp_path / "combined.pkl")
    meta = torch.load(tmp_path / "combined.pkl", map_location="cpu")["meta"]
    assert meta["combined"] == {"smooth": 0.25, "alpha": 0.5, "gamma": 0.5, "reduction": "mean", "square_in_union": True,
                                "class_weights": [0.25, 0.5, 2.0]}
    assert "dice" not in meta and meta["focal_gamma"] is None and meta["regression"] is None
    c = _loss_from_meta(meta)
    assert isinstance(c, CombinedLoss)
    assert (c.smooth, c.alpha, c.gamma, c.reduction, c.square_in_union) == (0.25, 0.5, 0.5, "mean", True)
    assert torch.equal(c.func.weight, torch.tensor([0.25, 0.5, 2.0]))
    assert _loss_from_meta(dict(meta, combined=dict(meta["combined"], class_weights=None))).func.weight is None
    # old-style meta dicts (no "combined" key) give the losses they gave before
    old = {"class_weights": [1.0, 2.0, 3.0], "regression": None, "focal_gamma": None}
    ce = _loss_from_meta(old)
    assert type(ce) is CrossEntropyLossFlat and torch.equal(ce.func.weight, torch.tensor([1.0, 2.0, 3.0]))
    fl = _loss_from_meta(dict(old, focal_gamma=2.0))
    assert type(fl) is FocalLossFlat and fl.gamma == 2.0
    d = _loss_from_meta(dict(old, dice={"smooth": 0.5, "reduction": "mean", "square_in_union": False}))
    assert type(d) is DiceLoss and (d.smooth, d.reduction) == (0.5, "mean")
    assert type(_loss_from_meta({"regression": "l1"})).__name__ == "L1LossFlat"
    _cpu_learner(tmp_path, CrossEntropyLossFlat(axis=1)).export(tmp_path / "ce.pkl")
    assert "combined" not in torch.load(tmp_path / "ce.pkl", map_location="cpu")["meta"]


def test_fused_path_refuses_mixed_losses_and_too_many_classes(tmp_path):
    from unet_amd.learner import CombinedLoss, DiceLoss
    from unet_amd.model import HipDynamicUnet
    import train as T
    x, y = torch.zeros(1, 4, 64, 64), torch.zeros(1, 64, 64, dtype=torch.int64)
    m = HipDynamicUnet("xresnet18", 4, 3, (64, 64), device="cpu")
    for kw in ({"dice": DiceLoss()}, {"focal_gamma": 2.0}, {"reg_kind": "mse"}):
        with pytest.raises(ValueError, match="CombinedLoss"):
            m.forward_loss_backward(x, y, combined=CombinedLoss(), **kw)
    with pytest.raises(ValueError, match="64 classes"):
        HipDynamicUnet("xresnet18", 4, 65, (64, 64), device="cpu").forward_loss_backward(x, y, combined=CombinedLoss())

    class _Dls:
        device = "cpu"
    with pytest.raises(ValueError, match="regression"):
        T.train_unet([1.0], _Dls(), "xresnet18", 1, tmp_path / "m", 1e-3, 10, regression=True, loss_func=CombinedLoss())
