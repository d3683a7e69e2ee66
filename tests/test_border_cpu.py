"""Host side of the border-weighted cross-entropy: the NumPy restatement against itself (tests/border_ref.py), the argument checks that
need no device, the export-meta round trip and the C ABI's new symbols."""
import numpy as np
import pytest
import torch

import border_ref as R
from unet_amd import border as BD  # the feature: without it this module does not import
from unet_amd.learner import BorderWeightedCrossEntropy, CrossEntropyLossFlat, _loss_from_meta


@pytest.mark.parametrize("shape", R.SHAPES)
def test_reference_distances_agree(shape):
    """the exhaustive minimum over the border set == rint(scipy's EDT squared), on blocky masks, salt noise and the corner mask, with and
    without exclude; at 512^2, where the exhaustive form is 2^28 terms per image, one batch of a blocky and a corner image"""
    rng = np.random.default_rng(sum(shape))
    B, H, W = shape
    if H * W > 1 << 17:
        cases = [(np.concatenate([R.blocky(rng, 1, H, W), R.corner(1, H, W)]), None)]
    else:
        cases = [(m, ex) for m in (R.blocky(rng, B, H, W), R.salt(rng, B, H, W), R.corner(B, H, W)) for ex in (None, 0)]
    for m, ex in cases:
        a, b = R.d2_brute(m, ex), R.d2_scipy(m, ex)
        assert a.dtype == np.int32 and b.dtype == np.int32 and np.array_equal(a, b)


def test_hand_cases():
    m = np.array([[[1, 0, 2]]], dtype=np.uint8)
    assert R.edge_set(m).all()
    assert not R.edge_set(m, exclude=0).any()                       # both pairs hold a 0: no border
    assert (R.d2_brute(m, 0) == R.SENTINEL).all() and (R.d2_scipy(m, 0) == R.SENTINEL).all()
    u = np.full((2, 5, 7), 3, dtype=np.int64)
    u[1, 2, 3] = 1
    d = R.d2_scipy(u)
    assert (d[0] == R.SENTINEL).all()                               # a uniform image beside a busy one
    assert d[1, 2, 3] == 0 and d[1, 2, 2] == 0 and d[1, 0, 0] == 4 + 4            # nearest: (2, 2)
    w = R.weight_map(u, d, [1.0, 2.0, 3.0, 4.0], 10.0, 5.0, 4)
    assert (w[0] == 4.0).all() and w[1, 2, 3] == 2.0 + 10.0
    u[0, 0, 0] = 9
    assert R.weight_map(u, R.d2_scipy(u), None, 10.0, 5.0, 4)[0, 0, 0] == 0.0
    assert BD.NO_BORDER == R.SENTINEL


def test_shape_limits_are_refused_before_any_launch():
    from unet_amd import ops
    for shape in [(1, 1, 8193), (1, 8193, 1), (0, 4, 4), (1, 0, 4), (4, 4, 4, 4), (4,)]:
        with pytest.raises(ValueError):
            BD.distance_to_border(np.zeros(shape, dtype=np.uint8))
        with pytest.raises(ValueError):
            BD.border_weight_map(np.zeros(shape, dtype=np.uint8), n_classes=2)
    with pytest.raises(ValueError):
        ops.edt_workspace(1, 8193, 8)
    assert ops.edt_workspace(2, 8192, 8192) == 2 * 8192 * 8192 * 2
    with pytest.raises(ValueError):
        BD.distance_to_border(np.zeros((1, 4, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        BD.distance_to_border(np.zeros((1, 4, 4), dtype=np.uint8), exclude=-1)
    with pytest.raises(ValueError):
        BD.border_weight_map(np.zeros((1, 4, 4), dtype=np.uint8))                    # neither class weights nor n_classes
    with pytest.raises(ValueError):
        BD.border_weight_map(np.zeros((1, 4, 4), dtype=np.uint8), [1.0, 2.0], n_classes=3)


@pytest.mark.parametrize("kw", [{"w0": -1.0}, {"w0": float("nan")}, {"sigma": 0.0}, {"sigma": -2.0}, {"sigma": float("nan")}, {"exclude": -1},
                                {"exclude": 1.5}])
def test_loss_refuses_bad_parameters(kw):
    with pytest.raises(ValueError):
        BorderWeightedCrossEntropy(**kw)
    if "exclude" not in kw:
        with pytest.raises(ValueError):
            BD.border_weight_map(np.zeros((1, 4, 4), dtype=np.uint8), n_classes=2, **kw)


def test_loss_object_and_meta_round_trip():
    loss = BorderWeightedCrossEntropy()
    assert isinstance(loss, CrossEntropyLossFlat) and (loss.axis, loss.w0, loss.sigma, loss.exclude) == (1, 10.0, 5.0, None)      # the paper's
    assert loss.func.weight is None
    loss = BorderWeightedCrossEntropy(axis=1, w0=3, sigma=2.5, exclude=0)
    loss.func.weight = torch.tensor([0.5, 1.0, 2.0])                # train.py:211
    meta = {"class_weights": [float(v) for v in loss.func.weight], "focal_gamma": None, "regression": None,
            "border": {"w0": loss.w0, "sigma": loss.sigma, "exclude": loss.exclude}}
    back = _loss_from_meta(meta)
    assert type(back) is BorderWeightedCrossEntropy and (back.w0, back.sigma, back.exclude) == (3.0, 2.5, 0)
    assert torch.equal(back.func.weight, loss.func.weight)
    del meta["border"]                                              # files without the key load as they always have
    assert type(_loss_from_meta(meta)) is CrossEntropyLossFlat
    x = torch.randn(2, 3, 4, 4)
    assert torch.equal(loss.activation(x), torch.softmax(x, 1)) and torch.equal(loss.decodes(x), x.argmax(1))


def test_border_is_wired_into_the_step():
    import inspect
    from unet_amd.model import HipDynamicUnet
    from unet_amd.trainer import TrainStep
    assert "border" in inspect.signature(HipDynamicUnet.forward_loss_backward).parameters
    assert "self.border" in inspect.getsource(TrainStep)
    import train
    assert train.BorderWeightedCrossEntropy is BorderWeightedCrossEntropy


def test_new_symbols_are_in_the_library():
    from unet_amd import _lib as L
    want = {"unet_edt_workspace", "unet_border_edt", "unet_border_weight", "unet_ce_fwd_pw", "unet_ce_fwd_parts_pw", "unet_ce_bwd_pw",
            "unet_ce_bwd_pw_bf16"}
    assert want <= set(L.declared_symbols())
    for s in want:
        assert hasattr(L.lib, s), s
    assert L.lib.unet_edt_workspace(16, 512, 512) == 16 * 512 * 512 * 2
    assert L.lib.unet_edt_workspace(1, 8193, 1) == 0
    buf = torch.zeros(64)
    p = buf.data_ptr()
    assert L.lib.unet_border_edt(p, 0, 1, 8193, 4, -1, p, p, None) != 0 and b"border_edt" in L.lib.unet_last_error()
    assert L.lib.unet_border_edt(p, 0, 1, 4, 4, -2, p, p, None) != 0
    assert L.lib.unet_border_weight(p, p, None, 3, 1.0, 0.0, 16, p, None) != 0 and b"border_weight" in L.lib.unet_last_error()
    assert L.lib.unet_ce_fwd_pw(p, 8, 0, p, None, 10, 5, p, p, p, None) != 0 and b"ce_fwd_pw" in L.lib.unet_last_error()    # no weight map
    assert L.lib.unet_ce_fwd_parts_pw(p, 8, 0, p, p, 10, 65, p, p, None) != 0
    assert L.lib.unet_ce_bwd_pw(p, 8, 0, p, None, 10, 5, p, 1.0, p, 8, 0, None) != 0
