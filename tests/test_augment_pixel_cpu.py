"""The pixel-level augmentations without a GPU: Philox known answers, the statistics of the normal field, draw order and ranges of the new
transforms, cv2's Gaussian taps, the launch plan, refusals, the host restatements against tests/pixel_ref.py, and the host-side argument
checks of unet_pixel_ops / unet_fill_rects_mask / unet_blur_separable."""
import math

import numpy as np
import pytest
import torch

from pixel_ref import gaussian_taps_ref, noise_field, philox_ref, program_ref, separable_ref
from unet_amd import augment as A


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{w:08x}" for w in philox_ref(ctr, key)) == want
        got = A.philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]
        assert " ".join(f"{int(w):08x}" for w in got) == want


def test_normal_field_statistics_and_the_two_restatements_agree():
    N = 131072
    z = noise_field((7, 9), N)
    print("noise mean", z.mean(), "var", z.var())
    assert abs(z.mean()) <= 5 / math.sqrt(N)
    assert abs(z.var() - 1) <= 5 * math.sqrt(2 / N)
    assert np.abs(z).max() <= 5.8                                       # 24-bit uniforms: r <= sqrt(2 ln 2^25)
    np.testing.assert_allclose(A.normal_field((7, 9), 1001), z[:1001], rtol=0, atol=1e-12)
    # element 4q + 2h + s by hand for one counter
    w = philox_ref((5, 0, 0, 0), (7, 9))
    u = [((v >> 8) + 0.5) / 2 ** 24 for v in w]
    want = [math.sqrt(-2 * math.log(u[0])) * math.cos(2 * math.pi * u[1]), math.sqrt(-2 * math.log(u[0])) * math.sin(2 * math.pi * u[1]),
            math.sqrt(-2 * math.log(u[2])) * math.cos(2 * math.pi * u[3]), math.sqrt(-2 * math.log(u[2])) * math.sin(2 * math.pi * u[3])]
    np.testing.assert_allclose(z[20:24], want, rtol=0, atol=1e-12)


def test_draw_order_and_ranges_of_the_new_transforms():
    g, h = np.random.default_rng(3), np.random.default_rng(3)
    assert A.RandomGamma(gamma_limit=(70, 130)).get_params(g, 8, 8) == float(h.uniform(70, 130)) / 100.0
    var, k0, k1 = A.GaussNoise(var_limit=(5.0, 30.0)).get_params(g, 8, 8)
    assert var == float(h.uniform(5.0, 30.0)) and k0 == int(h.integers(0, 2 ** 32)) and k1 == int(h.integers(0, 2 ** 32))
    assert A.GaussNoise(var_limit=20).var == (0.0, 20.0) and A.GaussNoise().var == (10.0, 50.0)
    for _ in range(20):
        k, sigma = A.GaussianBlur(blur_limit=(3, 9), sigma_limit=(0.5, 2.0)).get_params(g, 8, 8)
        assert k == 3 + 2 * int(h.integers(0, 4)) and sigma == float(h.uniform(0.5, 2.0)) and k in (3, 5, 7, 9)
    k, sigma = A.GaussianBlur().get_params(g, 8, 8)
    assert k == 3 + 2 * int(h.integers(0, 3)) and sigma == float(h.uniform(0.0, 0.0)) == 0.0
    seen = set()
    for _ in range(40):
        k = A.Blur(blur_limit=7).get_params(g, 8, 8)
        assert k == 3 + 2 * int(h.integers(0, 3))
        seen.add(k)
    assert seen == {3, 5, 7} and A.Blur(blur_limit=(5, 11)).blur == (5, 11)
    drop = A.ChannelDropout(channel_drop_range=(1, 3)).get_params(g, 8, 8, 5)
    n = int(h.integers(1, 4))
    assert drop == [int(c) for c in h.choice(5, size=n, replace=False)] and len(set(drop)) == n
    assert A.ChannelShuffle().get_params(g, 8, 8, 6) == [int(c) for c in h.permutation(6)]
    assert g.random() == h.random()                                     # both streams are at the same place


def _mixed():
    return A.Compose([A.HorizontalFlip(p=0.5), A.RandomBrightnessContrast(p=0.5), A.GaussNoise(p=0.6), A.Rotate(p=0.5),
                      A.GaussianBlur(p=0.5), A.RandomGamma(p=0.5), A.CoarseDropout(p=0.5), A.ChannelDropout(p=0.5), A.ChannelShuffle(p=0.4),
                      A.Blur(p=0.3)], p=0.9)


def test_draws_of_a_mixed_pipeline_follow_per_image_compose_calls():
    pipe = _mixed()
    B, C, H, W = 12, 4, 32, 32
    ba = A.BatchAugment(pipe, n_transform_imgs=0.75, seed=4)
    fired = ba.draw(B, H, W, C)
    g = np.random.default_rng(4)
    want = {}
    for i in list(range(B))[:math.ceil(B * 0.75) - B]:
        if g.random() >= pipe.p:
            continue
        for k, t in enumerate(pipe.transforms):
            if g.random() < t.p:
                want[i, k] = t.get_params(g, H, W, C) if t.channels else t.get_params(g, H, W)
    assert fired.keys() == want.keys() and len(fired) > 10 and {k for _, k in fired} == set(range(10))
    for key in want:
        assert repr(fired[key]) == repr(want[key])
    assert ba.g.random() == g.random()


def test_gaussian_taps():
    tables = {1: [1.0], 3: [.25, .5, .25], 5: [.0625, .25, .375, .25, .0625], 7: [.03125, .109375, .21875, .28125, .21875, .109375, .03125]}
    for k, want in tables.items():
        got = A.gaussian_taps(k, 0.0)
        assert got.dtype == np.float32 and got.tolist() == want
    sigma9 = 0.3 * ((9 - 1) * 0.5 - 1) + 0.8
    x = np.arange(9) - 4.0
    want = np.exp(-x * x / (2 * sigma9 * sigma9))
    np.testing.assert_allclose(A.gaussian_taps(9, 0), (want / want.sum()).astype(np.float32), rtol=0, atol=0)
    np.testing.assert_allclose(A.gaussian_taps(9, 0), A.gaussian_taps(9, sigma9), rtol=0, atol=0)
    for k in range(1, 32, 2):
        for sigma in (0.0, 0.4, 1.0, 3.7, 12.0):
            t = A.gaussian_taps(k, sigma)
            assert len(t) == k and t.dtype == np.float32 and abs(float(t.astype(np.float64).sum()) - 1.0) <= 1e-7, (k, sigma)
            np.testing.assert_allclose(t, gaussian_taps_ref(k, sigma), rtol=0, atol=1e-7)
            assert np.array_equal(t, t[::-1])
        box = A.Blur().taps(k)
        assert len(box) == k and abs(float(box.astype(np.float64).sum()) - 1.0) <= 1e-7


def test_plan_groups_pointwise_runs():
    H, RBC, GN, Ro, GB = A.HorizontalFlip(), A.RandomBrightnessContrast(), A.GaussNoise(), A.Rotate(), A.GaussianBlur()
    RG, CD, ChD = A.RandomGamma(), A.CoarseDropout(), A.ChannelDropout()
    plan = lambda ts: A.BatchAugment(A.Compose(ts)).plan()
    assert plan([H, RBC, GN, Ro, GB, RG, CD, ChD]) == [("warp", [0]), ("pixel", [1, 2]), ("warp", [3]), ("blur", 4), ("pixel", [5, 6, 7])]
    mean = A.RandomBrightnessContrast(brightness_by_max=False)
    assert plan([RG, mean, GN, A.ChannelShuffle()]) == [("pixel", [0]), ("image", 1), ("pixel", [2, 3])]
    assert plan([A.Blur(), GB]) == [("blur", 0), ("blur", 1)]
    assert plan([H, A.VerticalFlip()]) == [("warp", [0, 1])]
    # segments() is what it was
    assert A.BatchAugment(A.Compose([H, RBC, GN, Ro, GB, RG])).segments() == [[0], 1, 2, [3], 4, 5]


def test_refusals():
    with pytest.raises(NotImplementedError, match="above 31"):
        A.GaussianBlur(blur_limit=(3, 33))
    with pytest.raises(NotImplementedError, match="above 31"):
        A.Blur(blur_limit=33)
    for bad in ((0, 7), (3, 8), (4, 7), 6, (0, 0)):
        with pytest.raises(NotImplementedError, match="blur_limit"):
            A.GaussianBlur(blur_limit=bad)
        with pytest.raises(NotImplementedError, match="blur_limit"):
            A.Blur(blur_limit=bad)
    A.GaussianBlur(blur_limit=(1, 31)), A.Blur(blur_limit=31)
    g = np.random.default_rng(0)
    mask = torch.zeros(8, 8, dtype=torch.long)
    with pytest.raises(ValueError, match="drop all channels"):
        A.ChannelDropout(channel_drop_range=(1, 3), p=1.0)(torch.rand(3, 8, 8), mask, g)
    with pytest.raises(ValueError, match="one channel"):
        A.ChannelDropout(p=1.0)(torch.rand(1, 8, 8), mask, g)
    with pytest.raises(ValueError, match="channel_drop_range"):
        A.ChannelDropout(channel_drop_range=(0, 1))
    with pytest.raises(ValueError, match="at most 16 channels"):
        A.ChannelShuffle(p=1.0)(torch.rand(17, 8, 8), mask, g)
    with pytest.raises(ValueError, match="at most 16 channels"):
        A.BatchAugment(A.Compose([A.Rotate(), A.ChannelShuffle()]), 0.5)(torch.rand(2, 17, 8, 8), torch.zeros(2, 8, 8, dtype=torch.long))
    with pytest.raises(ValueError, match="var_limit"):
        A.GaussNoise(var_limit=(-1.0, 2.0))


def test_host_restatements_match_the_reference():
    """apply_params on CPU tensors (what a per-image Compose on the host runs) against tests/pixel_ref.py"""
    g = np.random.default_rng(11)
    img = torch.from_numpy(g.random((5, 13, 10), dtype=np.float32))
    mask = torch.from_numpy(g.integers(0, 4, (13, 10)))
    x = img.numpy()
    cases = [(A.RandomGamma(), 0.8, [("gamma", 0.8)]),
             (A.GaussNoise(mean=12.0), (40.0, 123, 0xfffffff0), [("noise", 123, 0xfffffff0, 12 / 255, math.sqrt(40.0) / 255, True)]),
             (A.GaussNoise(per_channel=False), (40.0, 5, 6), [("noise", 5, 6, 0.0, math.sqrt(40.0) / 255, False)]),
             (A.ChannelDropout(channel_drop_range=(1, 2), fill_value=0.5), [3, 0], [("drop", [3, 0], 0.5)]),
             (A.ChannelShuffle(), [4, 2, 0, 1, 3], [("permute", [4, 2, 0, 1, 3])])]
    for t, prm, prog in cases:
        assert t.program(prm, 5, 13, 10)[0][0] == prog[0][0]
        out, m = t.apply_params(img, mask, prm)
        assert m is mask and out.dtype == torch.float32 and out.shape == img.shape
        np.testing.assert_allclose(out.numpy(), program_ref(x, prog), rtol=0, atol=1e-6, err_msg=type(t).__name__)
    assert torch.equal(A.ChannelShuffle().apply_params(img, mask, [4, 2, 0, 1, 3])[0], img[[4, 2, 0, 1, 3]])
    for t, prm in ((A.GaussianBlur(), (7, 0.0)), (A.GaussianBlur(), (31, 2.5)), (A.Blur(), 5), (A.Blur(), 31)):
        out, m = t.apply_params(img, mask, prm)
        assert m is mask
        np.testing.assert_allclose(out.numpy(), separable_ref(x, t.taps(prm)), rtol=0, atol=1e-6)
    # existing programs: RandomBrightnessContrast and CoarseDropout describe what their apply_params does
    rbc, cd = A.RandomBrightnessContrast(), A.CoarseDropout(fill_value=0.25, mask_fill_value=7)
    np.testing.assert_array_equal(rbc.apply_params(img, mask, (1.1, -0.05))[0].numpy(), program_ref(x, rbc.program((1.1, -0.05), 5, 13, 10)))
    holes = [(2, 3, 4, 5), (0, 0, 13, 1)]
    np.testing.assert_array_equal(cd.apply_params(img, mask, holes)[0].numpy(), program_ref(x, cd.program(holes, 5, 13, 10)))
    assert cd.mask_rects(holes) == ([(2, 3, 6, 8), (0, 0, 13, 1)], 7) and A.CoarseDropout().mask_rects(holes) is None
    assert A.RandomBrightnessContrast(brightness_by_max=False).program((1.1, 0.1), 5, 13, 10) is None


def test_pixel_entry_points_reject_bad_arguments_on_the_host():
    import ctypes as C
    from unet_amd import _lib as L
    lib = L.lib
    a, b = 0x10000, 0x20000                  # never dereferenced: every call below is refused before any launch

    def prog(image=0, ops=((L.PIXEL_GAMMA, 0, 0, 1.0, 0.0),), rects=()):
        p = L.PixelProg()
        p.image, p.nops, p.nrects = image, len(ops), len(rects)
        for k, op in enumerate(ops[:L.PIXEL_MAX_OPS]):
            p.ops[k] = L.PixelOp(*op)
        for k, r in enumerate(rects[:L.PIXEL_MAX_RECTS]):
            for q in range(4):
                p.rects[k][q] = r[q]
        return p

    def run(*ps, x=a, n=4, Cc=3, H=8, W=8, count=None):
        arr = (L.PixelProg * max(len(ps), 1))(*ps)
        return lib.unet_pixel_ops(x, n, Cc, H, W, C.addressof(arr) if ps else None, len(ps) if count is None else count, None)

    ok = prog()
    bad = [run(ok, x=None), run(), run(ok, n=0), run(ok, Cc=0), run(ok, H=0), run(ok, W=70000), run(ok, count=0), run(ok, count=9),
           run(prog(image=4)), run(prog(image=2), prog(image=2)), run(prog(image=2), prog(image=1)),
           run(prog(ops=())), run(prog(ops=((9, 0, 0, 0.0, 0.0),))), run(prog(ops=((L.PIXEL_GAMMA | 0x200, 0, 0, 1.0, 0.0),))),
           run(prog(ops=((L.PIXEL_GAMMA, 0, 0, float("nan"), 0.0),))), run(prog(ops=((L.PIXEL_GAUSS_NOISE, 1, 2, 0.0, float("inf")),))),
           run(prog(ops=((L.PIXEL_FILL_RECTS, 0, 1, 0.0, 0.0),))),                                   # names a rectangle, has none
           run(prog(ops=((L.PIXEL_FILL_RECTS, 1, 1, 0.0, 0.0),), rects=((0, 0, 2, 2),))),
           run(prog(ops=((L.PIXEL_FILL_RECTS, 0, 1, 0.0, 0.0),), rects=((0, 0, 9, 2),))),            # past the image
           run(prog(ops=((L.PIXEL_FILL_RECTS, 0, 1, 0.0, 0.0),), rects=((2, 0, 2, 2),))),            # empty
           run(prog(ops=((L.PIXEL_CHANNEL_DROP, 0b1000, 0, 0.0, 0.0),))),                            # channel 3 of 3
           run(prog(ops=((L.PIXEL_CHANNEL_PERMUTE, 0x100, 0, 0.0, 0.0),))),                          # 0, 0, 1: not a permutation
           run(prog(ops=((L.PIXEL_CHANNEL_PERMUTE, 0x310, 0, 0.0, 0.0),))),                          # names channel 3
           run(prog(ops=((L.PIXEL_CHANNEL_PERMUTE, 0x210, 0, 0.0, 0.0),)), Cc=17)]
    assert bad == [-1] * len(bad), bad
    assert b"pixel_ops" in lib.unet_last_error()

    def rset(image=0, rects=((0, 0, 2, 2),)):
        s = L.RectSet()
        s.image, s.nrects = image, len(rects)
        for k, r in enumerate(rects):
            for q in range(4):
                s.rects[k][q] = r[q]
        return s

    def fill(*ss, m=a, f32=0, n=4, H=8, W=8, v=1.0, count=None):
        arr = (L.RectSet * max(len(ss), 1))(*ss)
        return lib.unet_fill_rects_mask(m, f32, n, H, W, C.addressof(arr) if ss else None, len(ss) if count is None else count, v, None)

    bad = [fill(rset(), m=None), fill(), fill(rset(), f32=2), fill(rset(), n=0), fill(rset(), H=0), fill(rset(), count=9), fill(rset(image=4)),
           fill(rset(1), rset(1)), fill(rset(rects=())), fill(rset(rects=((0, 0, 2, 9),))), fill(rset(), v=float("nan")), fill(rset(), v=1e30)]
    assert bad == [-1] * len(bad), bad
    assert b"fill_rects_mask" in lib.unet_last_error()

    ks = (C.c_int * 17)(*([3] * 17))
    taps = (C.c_float * (31 * 17))(*([0.25] * (31 * 17)))

    def blur(src=a, dst=b, n=2, Cc=3, H=8, W=8, k=ks, t=taps):
        return lib.unet_blur_separable(src, dst, n, Cc, H, W, k, t, None)

    even, big, zero = (C.c_int * 2)(3, 4), (C.c_int * 2)(33, 3), (C.c_int * 2)(3, 0)
    nan = (C.c_float * 62)(*([float("nan")] * 62))
    bad = [blur(src=None), blur(dst=None), blur(k=None), blur(t=None), blur(dst=a), blur(n=0), blur(n=17), blur(Cc=0), blur(H=0), blur(W=-1),
           blur(k=even), blur(k=big), blur(k=zero), blur(t=nan)]
    assert bad == [-1] * len(bad), bad
    assert b"blur_separable" in lib.unet_last_error()
    assert lib.unet_abi_version() == 8
    assert C.sizeof(L.PixelProg) == 432 and C.sizeof(L.RectSet) == 264


def test_device_only_ops_say_so_on_host_tensors():
    from unet_amd import ops
    x = torch.rand(2, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pixel_ops(x, {0: [("gamma", 1.0)]})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.blur_separable(x, torch.empty_like(x), [np.ones(1, np.float32)] * 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fill_rects_mask(torch.zeros(2, 8, 8), {0: [(0, 0, 1, 1)]}, 1)
