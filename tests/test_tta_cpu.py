"""Test-time augmentation without a GPU: the D4 code table, parsing of tta=, the C ABI surface of the new kernels, and the keyword that
params_and_main passes to save_predictions."""
import itertools

import pytest
import torch

import tta_ref as R


def _grid(h, w, lead=(2, 3)):
    return torch.arange(int(torch.tensor(lead).prod()) * h * w, dtype=torch.float64).view(*lead, h, w)


def test_table_matches_the_package_and_inverses_undo():
    from unet_amd import tta as T
    x = _grid(5, 5)
    for c in range(8):
        assert torch.equal(T.orient(x, c), R.g(x, c)), c
        assert torch.equal(R.g_inv(R.g(x, c), c), x), c
        assert torch.equal(R.g(R.g_inv(x, c), c), x), c
        assert T.INVERSE[c] == R.INVERSE[c]
    y = _grid(4, 6)
    for c in range(4):                                  # flips act on any shape
        assert torch.equal(T.unorient(T.orient(y, c), c), y)


def test_codes_form_a_group():
    x = _grid(4, 4, (1,))
    img = {c: R.g(x, c) for c in range(8)}
    assert len({tuple(v.flatten().tolist()) for v in img.values()}) == 8          # 8 distinct symmetries
    for a, b in itertools.product(range(8), repeat=2):
        comp = R.g(R.g(x, b), a)                                                     # a after b
        hits = [c for c in range(8) if torch.equal(img[c], comp)]
        assert len(hits) == 1, (a, b)                                                # closed under composition
    assert all(torch.equal(R.g(R.g(x, c), R.INVERSE[c]), x) for c in range(8))


def test_parse():
    from unet_amd.tta import parse
    assert parse(None) is None
    assert parse("flips") == (0, 1, 2, 3)
    assert parse("flips", [(256, 320)]) == (0, 1, 2, 3)
    assert parse("d4", [(512, 512)]) == tuple(range(8))
    assert parse((0,)) == (0,)
    assert parse([3, 1], [(8, 16)]) == (3, 1)
    assert parse((7, 0, 5), [(64, 64)]) == (7, 0, 5)
    for bad in ((1, 1), (0, 8), (-1,), (), "rot", (True,)):
        with pytest.raises(ValueError):
            parse(bad)
    for bad in ("d4", (0, 4), (5,)):
        with pytest.raises(ValueError, match='"flips"'):
            parse(bad, [(512, 512), (256, 512)])


def test_header_declares_and_library_exports_the_new_entry_points():
    from unet_amd import _lib as L
    syms = L.declared_symbols()
    for s in ("unet_window_gather_oriented", "unet_nchw_to_nhwc_oriented", "unet_tta_accumulate"):
        assert s in syms, s
        assert hasattr(L.lib, s), s
    assert L.lib.unet_abi_version() == 8
    txt = L.HEADER.read_text()
    assert "#define UNET_ABI_VERSION 8" in txt


def test_params_and_main_passes_tta_as_a_keyword(monkeypatch):
    import params_and_main as P
    import predict
    import train
    import create_tiles_unet
    assert P.TTA is None
    calls = {}
    monkeypatch.setattr(create_tiles_unet, "split_raster", lambda **kw: None)
    monkeypatch.setattr(train, "train_func", lambda *a: None)
    monkeypatch.setattr(predict, "save_predictions", lambda *a, **k: calls.setdefault("predict", (a, k)))
    monkeypatch.setattr(P, "Create_tiles", False); monkeypatch.setattr(P, "Train", False); monkeypatch.setattr(P, "Predict", True)
    monkeypatch.setattr(P, "enable_extra_parameters", True)
    monkeypatch.setattr(P, "TTA", "d4")
    P.main()
    a, k = calls.pop("predict")
    assert len(a) == 11 and k == {"tta": "d4"}
    monkeypatch.setattr(P, "enable_extra_parameters", False)        # reset with the other extra parameters
    P.main()
    a, k = calls.pop("predict")
    assert len(a) == 11 and k == {"tta": None}
