"""DiceLoss (fastai losses.DiceLoss, the fifth loss of the reference's configuration, params_and_main.py:16) without a GPU: the generic-path
restatement against the fp64 spec (values and autograd gradients), the C ABI of the fused kernels, the export / load_learner metadata and
the arguments the fused path refuses before any launch."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from dice_ref import dice_loss_ref

ROOT = Path(__file__).resolve().parent.parent


def _case(C, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(3, C, 9, 7, generator=g, dtype=torch.float64) * 2.5
    y = torch.randint(0, C, (3, 9, 7), generator=g)
    y[0, 0, :3] = -100                               # ignore-style targets: all-zero one-hot rows
    y[1, 2, 1:4] = C
    return z, y


@pytest.mark.parametrize("C", [1, 2, 5, 12])
@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("square_in_union", [False, True])
def test_generic_path_matches_the_spec(C, reduction, square_in_union):
    from unet_amd.learner import DiceLoss
    smooth = 1e-6 if not square_in_union else 0.5
    loss_fn = DiceLoss(axis=1, smooth=smooth, reduction=reduction, square_in_union=square_in_union)
    z, y = _case(C, 10 * C + square_in_union)
    z1 = z.clone().requires_grad_(True)
    z2 = z.clone().requires_grad_(True)
    got = loss_fn(z1, y)
    want = dice_loss_ref(z2, y, smooth, reduction, square_in_union)
    got.backward()
    want.backward()
    assert abs(got.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
    assert (z1.grad - z2.grad).abs().max().item() <= 1e-12 * max(1e-30, z2.grad.abs().max().item()) + 1e-15


def test_defaults_activation_and_decodes():
    from unet_amd.learner import CrossEntropyLossFlat, DiceLoss
    d = DiceLoss()
    assert (d.axis, d.smooth, d.reduction, d.square_in_union) == (1, 1e-6, "sum", False)
    assert not isinstance(d, CrossEntropyLossFlat)       # _weights / _focal_gamma must not route it as a cross-entropy
    d.func.weight = torch.tensor([1.0, 2.0])            # train.py:211 assigns it for every loss (quirk Q5); Dice ignores it
    x = torch.randn(2, 4, 3, 3)
    assert torch.allclose(d.activation(x), torch.softmax(x, 1))
    assert torch.equal(d.decodes(x), x.argmax(1))
    with pytest.raises(ValueError):
        DiceLoss(reduction="none")


def test_header_declares_and_library_exports_the_dice_entry_points():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    ge.build()
    import unet_amd._lib as L
    want = {"unet_dice_workspace", "unet_dice_fwd", "unet_dice_bwd", "unet_dice_bwd_bf16"}
    assert want <= set(L.declared_symbols())
    for s in want:
        assert hasattr(L.lib, s), s
    assert L.lib.unet_abi_version() == 8
    # host-side query: B x blocks-per-sample partial rows of 2 C floats
    assert L.lib.unet_dice_workspace(3, 37 * 29, 5) == 3 * 5 * 2 * 5
    assert L.lib.unet_dice_workspace(16, 512 * 512, 5) == 16 * 64 * 2 * 5
    assert L.lib.unet_dice_workspace(0, 10, 5) == 0
    # arguments are checked on the host before any launch: 65 classes, a bad slice
    buf = torch.zeros(16)
    rc = L.lib.unet_dice_fwd(buf.data_ptr(), 68, 0, buf.data_ptr(), 1, 1, 65, 1e-6, 0, 0, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None)
    assert rc != 0 and b"dice_fwd" in L.lib.unet_last_error()
    rc = L.lib.unet_dice_bwd(buf.data_ptr(), 4, 2, buf.data_ptr(), 1, 1, 3, 0, buf.data_ptr(), 1.0, buf.data_ptr(), 4, 0, None)
    assert rc != 0 and b"dice_bwd" in L.lib.unet_last_error()


def _cpu_learner(tmp_path, loss, n_out=3):
    from unet_amd.learner import DataLoaders, DiceMulti, Learner, TileDataset
    from unet_amd.model import HipDynamicUnet
    model = HipDynamicUnet("xresnet18", 4, n_out, (64, 64), device="cpu")     # structure only
    dls = DataLoaders(TileDataset([np.zeros((4, 64, 64), np.uint8)], [np.zeros((64, 64), np.uint8)]), None, 1, device="cpu",
                      vocab=list("abc")[:n_out])
    return Learner(dls, model, loss_func=loss, metrics=[DiceMulti()], path=tmp_path)


def test_export_meta_round_trip_keeps_the_dice_loss(tmp_path):
    """Learner.export writes a "dice" key; the loss load_learner rebuilds from it keeps the class and its arguments (the model itself needs
    a device to load: the GPU suite runs load_learner end to end)"""
    from unet_amd.learner import CrossEntropyLossFlat, DiceLoss, FocalLossFlat, _loss_from_meta
    loss = DiceLoss(axis=1, smooth=0.25, reduction="mean", square_in_union=True)
    loss.func.weight = torch.tensor([0.2, 0.3, 0.5])
    _cpu_learner(tmp_path, loss).export(tmp_path / "dice.pkl")
    meta = torch.load(tmp_path / "dice.pkl", map_location="cpu")["meta"]
    assert meta["dice"] == {"smooth": 0.25, "reduction": "mean", "square_in_union": True}
    assert meta["class_weights"] is None and meta["focal_gamma"] is None and meta["regression"] is None
    d = _loss_from_meta(meta)
    assert isinstance(d, DiceLoss) and (d.smooth, d.reduction, d.square_in_union) == (0.25, "mean", True)
    # files without the key load as before
    _cpu_learner(tmp_path, CrossEntropyLossFlat(axis=1, weight=torch.tensor([1.0, 2.0, 3.0]))).export(tmp_path / "ce.pkl")
    meta = torch.load(tmp_path / "ce.pkl", map_location="cpu")["meta"]
    assert "dice" not in meta
    ce = _loss_from_meta(meta)
    assert type(ce) is CrossEntropyLossFlat and torch.equal(ce.func.weight, torch.tensor([1.0, 2.0, 3.0]))
    assert type(_loss_from_meta(dict(meta, focal_gamma=2.0))) is FocalLossFlat


def test_fused_path_refuses_regression_and_too_many_classes(tmp_path):
    from unet_amd.learner import DiceLoss
    from unet_amd.model import HipDynamicUnet
    import train as T
    x, y = torch.zeros(1, 4, 64, 64), torch.zeros(1, 64, 64, dtype=torch.int64)
    with pytest.raises(ValueError, match="64 classes"):
        HipDynamicUnet("xresnet18", 4, 65, (64, 64), device="cpu").forward_loss_backward(x, y, dice=DiceLoss())
    with pytest.raises(ValueError, match="classification"):
        HipDynamicUnet("xresnet18", 4, 1, (64, 64), device="cpu").forward_loss_backward(x, y.float(), reg_kind="mse", dice=DiceLoss())

    class _Dls:
        device = "cpu"
    with pytest.raises(ValueError, match="regression"):
        T.train_unet([1.0], _Dls(), "xresnet18", 1, tmp_path / "m", 1e-3, 10, regression=True, loss_func=DiceLoss())
