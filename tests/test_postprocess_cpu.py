"""CPU suite of the class-mask post-processing: the NumPy reference against scipy and hand-checked cases, the argument refusals (before any
model or GPU use), the C ABI surface and the params_and_main keyword."""
import numpy as np
import pytest
import torch

import postprocess_ref as R


def test_reference_labels_equal_scipy_per_class():
    ndi = pytest.importorskip("scipy.ndimage")
    structure = {4: ndi.generate_binary_structure(2, 1), 8: ndi.generate_binary_structure(2, 2)}
    for (H, W) in [(1, 1), (1, 37), (23, 1), (33, 63), (40, 70)]:
        for name, m in R.patterns(H, W).items():
            for conn in (4, 8):
                lab = R.label_components(m, conn)
                seen = set()
                for c in np.unique(m):
                    ref, nref = ndi.label(m == c, structure=structure[conn])
                    sel = m == c
                    pairs = set(zip(lab[sel].tolist(), ref[sel].tolist()))          # a bijection between our labels and scipy's
                    assert len(pairs) == nref == len({a for a, _ in pairs}) == len({b for _, b in pairs}), (name, H, W, conn, int(c))
                    seen |= {a for a, _ in pairs}
                # canonical: every label is the smallest linear index of its component
                flat = lab.ravel()
                assert all(flat[l] == l and np.flatnonzero(flat == l)[0] == l for l in seen), (name, H, W, conn)
                sizes = R.component_sizes(lab)
                assert sizes.sum() == H * W and set(np.flatnonzero(sizes.ravel()).tolist()) == seen


def test_spiral_is_two_components_and_the_comb_one_serpentine():
    for H, W in [(67, 131), (200, 136)]:
        assert len(np.unique(R.label_components(R.spiral(H, W), 4))) == 2
        m = R.comb(H, W)
        assert len(np.unique(R.label_components(m, 4)[m == 1])) == 1


def test_hand_example_1x3():
    m = np.array([[1, 0, 2]], dtype=np.uint8)
    r1, merged1, left1 = R.sieve_round(m, 2)
    assert r1.tolist() == [[1, 1, 0]] and (merged1, left1) == (2, 1)
    r2, merged2, left2 = R.sieve_round(r1, 2)
    assert r2.tolist() == [[1, 1, 1]] and (merged2, left2) == (1, 0)
    out, info = R.sieve(m, 2)
    assert out.tolist() == [[1, 1, 1]] and info == {"rounds": 3, "merged": [2, 1, 0], "small_left": 0}
    out, info = R.sieve(m, 2, max_rounds=1)
    assert out.tolist() == [[1, 1, 0]] and info == {"rounds": 1, "merged": [2], "small_left": 1}
    out, info = R.sieve(m, 1)
    assert out.tolist() == m.tolist() and info == {"rounds": 0, "merged": [], "small_left": 0}
    # frozen class 0: the middle pixel neither merges nor is merged into; its neighbours have no other neighbour
    out, info = R.sieve(m, 2, frozen_class=0)
    assert out.tolist() == m.tolist() and info == {"rounds": 1, "merged": [0], "small_left": 2}


def test_hand_majority():
    m = np.array([[0, 0, 1], [0, 2, 1], [1, 1, 1]], dtype=np.uint8)
    out = R.majority_filter(m, 3)
    # centre: five 1s win; corner (0, 0): window {0, 0, 0, 2} -> 0; (0, 2): {0, 1, 2, 1} -> 1
    assert out[1, 1] == 1 and out[0, 0] == 0 and out[0, 2] == 1
    tie = np.array([[5, 5, 3, 3]], dtype=np.uint8)              # k = 3 at x = 1: {5, 5, 3} -> 5; x = 2: {5, 3, 3} -> 3
    assert R.majority_filter(tie, 3).tolist() == [[5, 5, 3, 3]]
    tie2 = np.array([[7, 2, 9]], dtype=np.uint8)               # a three-way tie with the centre among them: the centre stays
    assert R.majority_filter(tie2, 3).tolist() == [[7, 2, 9]]
    tie3 = np.array([[7, 7, 2, 4, 4]], dtype=np.uint8)         # k = 5 at the centre: 7 and 4 tie with two votes, the centre (2) is not among them
    assert R.majority_filter(tie3, 5)[0, 2] == 4
    fr = np.array([[0, 0, 0, 1, 0]], dtype=np.uint8)           # frozen 0 does not vote and does not change: the lone 1 stays
    assert R.majority_filter(fr, 3, frozen_class=0).tolist() == fr.tolist()
    assert R.majority_filter(fr, 3).tolist() == [[0, 0, 0, 0, 0]]


def test_reference_round_counts_stay_within_the_cap():
    m = R.patterns(67, 131)["noise5"]
    for mp in (2, 8, 50, 67 * 131 + 1):
        _, info = R.sieve(m, mp)
        assert info["rounds"] <= 16 and info["merged"][-1] == 0, (mp, info)


# ------------------------------------------------------------------------------------------------------------ argument refusals

def test_postprocess_argument_errors():
    from predict import check_outputs
    from unet_amd.postprocess import PostProcess, check_postprocess
    for bad in (dict(majority=4), dict(majority=1), dict(majority=17), dict(majority=-3), dict(majority=3.0), dict(sieve=-1), dict(sieve=2.5),
                dict(connectivity=6), dict(max_rounds=0), dict(frozen_class=256), dict(frozen_class=-1)):
        with pytest.raises(ValueError):
            PostProcess(**bad)
        with pytest.raises(ValueError):
            check_postprocess(bad)
    p = PostProcess(majority=5, sieve=64, connectivity=8, frozen_class=0)
    assert check_postprocess(p) is p and check_postprocess(None) is None
    q = check_postprocess({"majority": 3})
    assert isinstance(q, PostProcess) and (q.majority, q.sieve, q.connectivity, q.max_rounds, q.frozen_class) == (3, 0, 4, 16, None)
    for kw in (dict(regression=True), dict(all_classes=True), dict(specific_class=2), dict(specific_class=0), dict(merge=False)):
        with pytest.raises(ValueError):
            check_outputs(postprocess=p, **kw)
    with pytest.raises(ValueError):
        check_postprocess({"majorty": 3})
    with pytest.raises(ValueError):
        check_postprocess("sieve")


def test_predict_entry_points_refuse_before_model_or_gpu(monkeypatch, tmp_path):
    import predict as P

    def boom(*a, **k):
        raise AssertionError("the model was loaded / the device was touched before the postprocess argument was checked")
    monkeypatch.setattr(P, "load_learner", boom)
    monkeypatch.setattr(P, "_dist_ctx", boom)

    class NoModel:
        def __getattr__(self, name):
            boom()
    for kw in (dict(postprocess={"majority": 4}), dict(postprocess={"sieve": 8}, regression=True), dict(postprocess={"sieve": 8}, all_classes=True),
               dict(postprocess={"sieve": 8}, specific_class=1), dict(postprocess={"connectivity": 5, "sieve": 8})):
        with pytest.raises(ValueError):
            P.predict_raster(NoModel(), np.zeros((1, 8, 8), dtype=np.uint8), **kw)
        kw = dict(kw)
        reg = kw.pop("regression", False)
        with pytest.raises(ValueError):
            P.save_predictions(tmp_path / "model.pkl", tmp_path, reg, merge=True, **kw)
    with pytest.raises(ValueError):
        P.save_predictions(tmp_path / "model.pkl", tmp_path, False, merge=False, postprocess={"sieve": 8})


def test_mask_larger_than_int32_is_refused_from_the_shape():
    from unet_amd import postprocess as PP
    big = torch.empty((65536, 32768), dtype=torch.uint8, device="meta")          # 2^31 px: one more than the labels can index; never allocated
    for fn in (lambda: PP.label_components(big), lambda: PP.majority_filter(big, 3), lambda: PP.sieve(big, 8), lambda: PP.PostProcess(sieve=8)(big),
               lambda: PP.component_sizes(torch.empty((65536, 32768), dtype=torch.int32, device="meta"))):
        with pytest.raises(ValueError, match="2\\^31"):
            fn()
    from unet_amd import ops
    ops.check_mask_shape("ok", (1, 2 ** 31 - 1))
    with pytest.raises(ValueError):
        ops.check_mask_shape("bad", (0, 5))


def test_host_checks_of_the_wrappers():
    from unet_amd import ops
    from unet_amd import postprocess as PP
    m = torch.zeros((4, 4), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.majority_filter(m, torch.zeros_like(m), 3)                       # not on the GPU
    with pytest.raises(ValueError):
        PP.label_components(torch.zeros((4, 4), dtype=torch.int64))          # dtype
    with pytest.raises(ValueError):
        PP.label_components(np.zeros((4, 4), dtype=np.int32))
    with pytest.raises(ValueError):
        PP.label_components(m, connectivity=6)
    with pytest.raises(ValueError):
        PP.majority_filter(m, 4)
    with pytest.raises(ValueError):
        PP.sieve(m, 8, max_rounds=0)
    with pytest.raises(ValueError):
        PP.label_components(torch.zeros((2, 4, 4), dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------------ C ABI

NEW_SYMBOLS = ("unet_cc_tile_shape", "unet_cc_label", "unet_cc_sizes", "unet_sieve_round", "unet_majority_filter", "unet_postprocess_counters")


def test_header_declares_and_library_exports_the_new_symbols():
    from unet_amd import _lib as L
    declared = L.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L.lib, s) and s in L._sig, s
    assert L.lib.unet_abi_version() == 8
    assert "#define UNET_ABI_VERSION 8" in L.HEADER.read_text()


def test_bad_arguments_return_minus_one_without_a_launch():
    from unet_amd import _lib as L
    lib = L.lib
    p = 4096          # a non-null, 16-byte aligned address that is never dereferenced: every call below fails its host check
    calls = [
        lambda: lib.unet_cc_label(None, 4, 4, 4, p, p, None),
        lambda: lib.unet_cc_label(p, 4, 4, 6, p, p, None),
        lambda: lib.unet_cc_label(p, 65536, 32768, 4, p, p, None),
        lambda: lib.unet_cc_label(p, 0, 4, 4, p, p, None),
        lambda: lib.unet_cc_label(p, 4, 4, 4, p + 4, p, None),
        lambda: lib.unet_cc_sizes(p, 65536, 32768, p, None),
        lambda: lib.unet_sieve_round(p, p, 4, 4, 4, 8, -1, p, p, p, p, None),            # in == out
        lambda: lib.unet_sieve_round(p, p + 64, 4, 4, 4, 1, -1, p, p, p, p, None),       # min_pixels < 2
        lambda: lib.unet_sieve_round(p, p + 64, 4, 4, 4, 8, 256, p, p, p, p, None),
        lambda: lib.unet_sieve_round(p, p + 64, 4, 4, 4, 8, -1, p, p, None, p, None),    # keys missing
        lambda: lib.unet_majority_filter(p, p + 64, 4, 4, 4, -1, None),
        lambda: lib.unet_majority_filter(p, p + 64, 4, 4, 17, -1, None),
        lambda: lib.unet_majority_filter(p, p, 4, 4, 3, -1, None),
        lambda: lib.unet_majority_filter(p, p + 64, 4, 4, 3, 300, None),
        lambda: lib.unet_postprocess_counters(None, None, None),
    ]
    for i, c in enumerate(calls):
        assert c() == -1, i
        assert lib.unet_last_error(), i
    th, tw = __import__("unet_amd.ops", fromlist=["ops"]).cc_tile_shape()
    assert th >= 8 and tw >= 8 and th * tw * 5 <= 64 * 1024


# ------------------------------------------------------------------------------------------------------------ params_and_main

def test_params_and_main_passes_postprocess_only_when_set(monkeypatch):
    import params_and_main as M
    import predict
    import train
    import create_tiles_unet
    assert M.POSTPROCESS is None
    calls = {}
    monkeypatch.setattr(create_tiles_unet, "split_raster", lambda **kw: None)
    monkeypatch.setattr(train, "train_func", lambda *a: None)
    monkeypatch.setattr(predict, "save_predictions", lambda *a, **k: calls.setdefault("predict", (a, k)))
    monkeypatch.setattr(M, "Create_tiles", False); monkeypatch.setattr(M, "Train", False); monkeypatch.setattr(M, "Predict", True)
    monkeypatch.setattr(M, "enable_extra_parameters", True)
    M.main()
    a, k = calls.pop("predict")
    assert len(a) == 11 and k == {"tta": None}                                  # the default call, exactly as before
    monkeypatch.setattr(M, "POSTPROCESS", {"majority": 5, "sieve": 64})
    M.main()
    a, k = calls.pop("predict")
    assert len(a) == 11 and k == {"tta": None, "postprocess": {"majority": 5, "sieve": 64}}
    monkeypatch.setattr(M, "enable_extra_parameters", False)                    # reset with the other extra parameters
    M.main()
    a, k = calls.pop("predict")
    assert len(a) == 11 and k == {"tta": None} and M.POSTPROCESS is None
