"""The non-rigid augmentations without a GPU: the ABI, every host-side refusal, the grid node tables, the elastic taps, segments and plans
of pipelines that hold a field transform, unchanged draws of the existing pipelines, and the fp64 reference itself against scipy."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_ref as F
from unet_amd import augment as A

FIELD_SYMBOLS = ("unet_warp_field", "unet_warp_field_mask", "unet_elastic_field")


def test_header_declares_and_library_exports_the_entry_points():
    from unet_amd import _lib as L
    declared = L.declared_symbols()
    for s in FIELD_SYMBOLS:
        assert s in declared and hasattr(L.lib, s) and s in L._sig
    assert L.lib.unet_abi_version() == 8
    assert C.sizeof(L.FieldImage) == 4 + 4 * 6 + 4 * 3 + 4 * 2 * 17 and C.sizeof(L.ElasticImage) == 20
    assert C.sizeof(L.FieldImage) * L.FIELD_MAX_IMAGES + 128 <= 4096          # the descriptor block fits the kernel-argument limit
    assert C.sizeof(L.ElasticImage) * L.ELASTIC_MAX_IMAGES + 4 * L.ELASTIC_MAX_KSIZE + 128 <= 4096


def _images(L, n, **over):
    im = (L.FieldImage * n)()
    for j in range(n):
        im[j].fired = 1
        im[j].pre[:] = [1, 0, 0, 0, 1, 0]
        im[j].nodes[0][:] = list(range(17))
        im[j].nodes[1][:] = list(range(17))
    return im


def test_warp_field_entry_points_reject_bad_arguments_on_the_host():
    from unet_amd import _lib as L
    lib = L.lib
    ims = _images(L, 17)
    a, b, fld = 0x10000, 0x20000, 0x30000        # never dereferenced: every call below is refused before any launch

    def img(*, src=a, dst=b, n=2, Cc=3, H=8, W=8, kind=0, im=ims, f=fld, sx=2, sy=2, interp=1, border=4, fill=0.0):
        return lib.unet_warp_field(src, dst, n, Cc, H, W, kind, im, f, sx, sy, interp, border, fill, None)

    def msk(*, src=a, dst=b, f32=0, n=2, H=8, W=8, kind=0, im=ims, f=fld, sx=2, sy=2, border=4, fill=0.0):
        return lib.unet_warp_field_mask(src, dst, f32, n, H, W, kind, im, f, sx, sy, border, fill, None)

    for rc in (img(src=None), img(dst=None), img(im=None), img(f=None), img(dst=a), img(dst=fld), img(n=0), img(n=17), img(Cc=0), img(H=0),
               img(W=-1), img(W=(1 << 24) + 1), img(kind=3), img(kind=-1), img(interp=2), img(interp=-1), img(border=3), img(border=5),
               img(fill=float("nan")), img(fill=float("inf")), img(kind=1, sx=0), img(kind=1, sy=-2), img(kind=1, W=33, sx=2),
               img(kind=1, H=40, sy=2),
               msk(src=None), msk(dst=None), msk(im=None), msk(f=None), msk(dst=a), msk(dst=fld), msk(f32=2), msk(n=0), msk(n=17), msk(H=-3),
               msk(W=0), msk(kind=5), msk(border=3), msk(fill=float("nan")), msk(fill=1e30), msk(kind=1, sx=0), msk(kind=1, W=33, sx=2)):
        assert rc == -1
    assert b"warp_field" in lib.unet_last_error()
    for call in (img, msk):
        for m in ([2, 0, 0, 0, 1, 0], [1, 0, 1, 0, 1, 0], [-1, 0, 0, 0, 1, 0], [1, 0, 0, 0, -1, 6], [0.5, 0, 0, 0, 1, 0], [1, 1, 0, 0, 1, 0],
                  [0, 1, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0]):
            bad = _images(L, 2)
            bad[1].pre[:] = m                               # not a D4 map of the 8 x 12 grid (a transposition needs a square one)
            assert call(H=8, W=12, kind=2, im=bad) == -1 and b"not a D4 map" in lib.unet_last_error(), m
        for kind, what, msg in ((0, "pre", b"non-finite pre-map"), (2, "optical", b"non-finite optical"), (1, "nodes", b"non-finite grid node"),
                                (0, "fired", b"fired must be 0 or 1")):
            for value in ((2,) if what == "fired" else (float("nan"), float("inf"))):
                bad = _images(L, 2)
                if what == "fired":
                    bad[1].fired = value
                elif what == "nodes":
                    bad[1].nodes[1][4] = value              # 8 pixels in steps of 2: nodes 0..4 are in use
                else:
                    getattr(bad[1], what)[2] = value
                assert call(kind=kind, im=bad) == -1 and msg in lib.unet_last_error(), (kind, what, value)


def test_elastic_field_entry_point_rejects_bad_arguments_on_the_host():
    from unet_amd import _lib as L
    lib = L.lib
    taps = (C.c_float * 401)(*([1.0 / 401] * 401))
    ims = (L.ElasticImage * 65)()
    for im in ims:
        im.alpha, im.fired = 1.0, 1
    a, b = 0x10000, 0x20000

    def call(*, f=a, ws=b, n=2, H=8, W=8, im=ims, t=taps, k=5):
        return lib.unet_elastic_field(f, ws, n, H, W, im, t, k, None)

    for rc in (call(f=None), call(ws=None), call(im=None), call(t=None), call(ws=a), call(n=0), call(n=65), call(H=0), call(W=-2),
               call(W=(1 << 24) + 1), call(H=1 << 19), call(k=0), call(k=4), call(k=403), call(k=-1)):
        assert rc == -1
    assert b"elastic_field" in lib.unet_last_error()
    bad_taps = (C.c_float * 5)(0.2, 0.2, float("nan"), 0.2, 0.2)
    assert call(t=bad_taps) == -1 and b"non-finite tap" in lib.unet_last_error()
    for field, value, msg in (("alpha", float("inf"), b"non-finite alpha"), ("alpha", float("nan"), b"non-finite alpha"),
                              ("fired", 2, b"must be 0 or 1"), ("same_dxdy", -1, b"must be 0 or 1")):
        bad = (L.ElasticImage * 2)()
        setattr(bad[1], field, value)
        assert call(im=bad) == -1 and msg in lib.unet_last_error(), field


def test_ops_refuse_host_tensors_and_bad_arguments():
    from unet_amd import ops
    x, y = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.warp_field(x, y, "optical", np.zeros((1, 3)), [True])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.warp_field_mask(x[0], y[0], "optical", np.zeros((1, 3)), [True])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.elastic_field(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4), [(1, 2)], 1.0, [True], False, [1.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.ElasticTransform(sigma=2, p=1.0)(torch.rand(3, 16, 16), torch.zeros(16, 16, dtype=torch.long), np.random.default_rng(0))
    ba = A.BatchAugment(A.Compose([A.HorizontalFlip(p=1.0), A.GridDistortion(p=1.0)]), n_transform_imgs=0.5)
    assert not hasattr(ba, "flip_flags")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ba(torch.rand(4, 3, 16, 16), torch.zeros(4, 16, 16, dtype=torch.long))


@pytest.mark.parametrize("N,steps", [(512, 5), (80, 7), (5, 5), (3, 5)])
def test_grid_node_tables_equal_the_linspace_loop(N, steps):
    g = np.random.default_rng(N + steps)
    for _ in range(5):
        factors = 1.0 + g.uniform(-0.3, 0.3, steps + 1)
        step, nodes = A.grid_nodes(N, steps, factors)
        want = F.linspace_loop(N, steps, factors)
        assert step == max(N // steps, 1) and nodes.dtype == np.float32 and nodes.shape == (17,) and nodes[0] == 0
        got = F.grid_table(nodes, step, N)
        # the nodes are the loop's prev / cur rounded to fp32 (half an ulp, relative 2^-24); the linspace between two of them moves by no more
        assert np.abs(got - want).max() <= 2.0 ** -24 * max(want.max(), 1.0) + 1e-12, np.abs(got - want).max()
        cells = -(-N // step)
        assert (nodes[cells + 1:] == 0).all()
        if N % step:
            assert nodes[cells] == N                        # the clipped cell ends at N
    assert F.linspace_loop(5, 5, np.ones(6)).tolist() == [0, 1, 2, 3, 4]            # cells of one pixel get prev
    assert F.linspace_loop(3, 5, np.full(6, 1.5)).tolist() == [0, 1.5, 3.0]
    np.testing.assert_allclose(F.linspace_loop(512, 5, np.ones(6)), np.r_[np.concatenate([np.linspace(102 * i, 102 * i + 102, 102) for i in range(5)]),
                                                                         510.0, 512.0], rtol=0, atol=1e-9)


def test_grid_distortion_draws_and_refusals():
    t = A.GridDistortion(num_steps=7, distort_limit=0.2)
    fx, fy = t.get_params(np.random.default_rng(3), 48, 80)
    g = np.random.default_rng(3)
    want = [1.0 + g.uniform(-0.2, 0.2) for _ in range(16)]
    assert fx == want[:8] and fy == want[8:]                # num_steps + 1 factors per axis, x first
    sx, sy, nodes = t.field_params([(fx, fy), None], 48, 80, "cpu")
    assert (sx, sy) == (11, 6) and nodes.shape == (2, 2, 17) and not nodes[1].any()
    with pytest.raises(NotImplementedError, match="normalized"):
        A.GridDistortion(normalized=True)
    for bad in (0, 16, 40, 2.5):
        with pytest.raises(NotImplementedError, match="num_steps"):
            A.GridDistortion(num_steps=bad)
    A.GridDistortion(num_steps=1), A.GridDistortion(num_steps=15)
    with pytest.raises(ValueError, match="cells"):
        A.grid_nodes(29, 15, np.ones(16))                   # 29 cells of one pixel, 16 factors: albumentations' IndexError


def test_elastic_taps_and_the_ksize_rule():
    assert [A.elastic_ksize(s) for s in (4, 6, 50, 1, 0.3, 2.06, 49.9, 50.1)] == [33, 49, 401, 9, 3, 17, 401, 403]
    assert A.elastic_ksize(50, approximate=True) == 17 and A.elastic_ksize(0.5, approximate=True) == 17
    for sigma, k in ((4, 33), (6, 49), (50, 401), (50, 17)):
        t = A.ElasticTransform(sigma=sigma, approximate=k == 17)
        assert t.ksize == k and t.taps.dtype == np.float32 and t.taps.shape == (k,)
        i = np.arange(k) - k // 2
        g = np.exp(-i.astype(np.float64) ** 2 / (2.0 * sigma * sigma))
        np.testing.assert_array_equal(t.taps, (g / g.sum()).astype(np.float32))
        np.testing.assert_array_equal(t.taps, F.gauss_taps(sigma, k))
        assert abs(float(t.taps.astype(np.float64).sum()) - 1.0) <= k * 2.0 ** -25 and (t.taps == t.taps[::-1]).all()
    k0, k1 = A.ElasticTransform().get_params(np.random.default_rng(5), 8, 8)
    g = np.random.default_rng(5)
    assert (k0, k1) == (int(g.integers(0, 2 ** 32)), int(g.integers(0, 2 ** 32)))


def test_elastic_noise_is_a_pure_function_of_key_plane_and_index():
    key = (0x12345678, 0x9abcdef0)
    a = F.elastic_noise(key, 0, 6, 10)
    assert (np.abs(a) < 1).all() and a.std() > 0.3
    e = 37                                                  # element (3, 7): word 1 of counter (9, q, 0, 0)
    for q in (0, 1):
        w = A.philox4x32_10(np.array([[e // 4, q, 0, 0]], dtype=np.uint32), key)[0, e % 4]
        assert F.elastic_noise(key, q, 6, 10)[3, 7] == 2.0 * ((int(w) >> 8) + 0.5) * 2.0 ** -24 - 1.0
    assert not np.array_equal(a, F.elastic_noise(key, 1, 6, 10)) and not np.array_equal(a, F.elastic_noise((1, 2), 0, 6, 10))
    np.testing.assert_array_equal(F.elastic_noise(key, 0, 3, 20), a.reshape(-1).reshape(3, 20))      # the index is y W + x alone


def test_not_implemented_refusals():
    for cls in (A.ElasticTransform, A.GridDistortion, A.OpticalDistortion):
        with pytest.raises(NotImplementedError, match="wrap"):
            cls(border_mode=3)
        with pytest.raises(NotImplementedError, match="border_mode"):
            cls(border_mode=5)
        with pytest.raises(NotImplementedError, match="interpolation=2"):
            cls(interpolation=2)
        with pytest.raises(NotImplementedError, match="per-channel value"):
            cls(border_mode=0, value=(1, 2, 3))
        with pytest.raises(NotImplementedError, match="per-channel mask_value"):
            cls(border_mode=0, mask_value=[1, 2])
        t = cls(interpolation=0, border_mode=0, value=0.5, mask_value=3)
        assert t.modes() == (0, 0, 0.5, 3.0) and t.interpolating and isinstance(t, A._Geometric) and A._device_geometric(t)
    with pytest.raises(NotImplementedError, match="ShiftScaleRotate"):
        A.ElasticTransform(alpha_affine=50)
    A.ElasticTransform(alpha_affine=0), A.ElasticTransform(alpha_affine=None)
    with pytest.raises(NotImplementedError, match="403 taps, at most 401"):
        A.ElasticTransform(sigma=50.2)
    assert A.ElasticTransform(sigma=500, approximate=True).ksize == 17 and A.ElasticTransform().ksize == 401       # the default runs


def test_optical_draws():
    t = A.OpticalDistortion(distort_limit=0.3, shift_limit=(0.1, 0.2))
    k, dx, dy = t.get_params(np.random.default_rng(8), 48, 80)
    g = np.random.default_rng(8)
    assert (k, dx, dy) == (g.uniform(-0.3, 0.3), g.uniform(0.1, 0.2) * 80, g.uniform(0.1, 0.2) * 48)
    sx, sy = F.optical_coords(np.array([[0.0, 0.0, 0.0], [0.25, 3.0, -2.0]]), 5, 9)
    x, y = F.pixel_grid(5, 9)
    np.testing.assert_array_equal(sx[0], x), np.testing.assert_array_equal(sy[0], y)        # k = 0 and no shift: the identity, exactly
    u, v = (x - 4.0) / 9, (y - 2.0) / 5
    kappa = 1 + 0.25 * (u * u + v * v) + 0.25 * (u * u + v * v) ** 2
    np.testing.assert_allclose(sx[1], 9 * u * kappa + 4.0 + 3.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(sy[1], 5 * v * kappa + 2.0 - 2.0, rtol=0, atol=1e-12)


def test_segments_and_plans_with_field_transforms():
    H, V, R90, T = A.HorizontalFlip(), A.VerticalFlip(), A.RandomRotate90(), A.Transpose()
    Ro, E, G, O, N = A.Rotate(), A.ElasticTransform(sigma=4), A.GridDistortion(), A.OpticalDistortion(), A.GaussNoise()
    ba = lambda ts: A.BatchAugment(A.Compose(ts))
    seg = lambda ts: ba(ts).segments()
    assert seg([H, V, E]) == [[0, 1, 2]]                                   # D4 transforms join the field transform behind them
    assert seg([E, H, V]) == [[0], [1, 2]]                                 # first: it closes its segment
    assert seg([H, R90, T, G]) == [[0, 1, 2, 3]]
    assert seg([E, G]) == [[0], [1]] and seg([H, E, G, O]) == [[0, 1], [2], [3]]        # twice in a row
    assert seg([Ro, E]) == [[0], [1]] and seg([H, Ro, V, O]) == [[0, 1, 2], [3]]        # after Rotate: a second interpolation
    assert seg([E, Ro]) == [[0], [1]] and seg([H, G, V, Ro]) == [[0, 1], [2, 3]]
    assert seg([H, N, V, E, N, O, T]) == [[0], 1, [2, 3], 4, [5], [6]]
    assert ba([H, V, E]).plan() == [("warp", [0, 1, 2])]
    assert ba([E, N, H, G, Ro]).plan() == [("warp", [0]), ("pixel", [1]), ("warp", [2, 3]), ("warp", [4])]
    # the segments of pipelines without a field transform are what they were
    S, RBC, CD = A.ShiftScaleRotate(), A.RandomBrightnessContrast(), A.CoarseDropout()
    assert seg([H, V, R90, S, RBC, Ro]) == [[0, 1, 2, 3], 4, [5]] and seg([H, S, V, Ro, T, Ro]) == [[0, 1, 2], [3, 4], [5]]


def test_draws_of_existing_pipelines_are_unchanged():
    """the seeded generator is consumed as before: the documented order, restated here draw by draw"""
    def restated(ts, seed, B, n, H, W):
        g = np.random.default_rng(seed)
        fired = {}
        for i in list(range(B))[:int(np.ceil(B * n)) - B]:
            if g.random() >= 1.0:
                continue
            for k, (p, draw) in enumerate(ts):
                if g.random() < p:
                    fired[i, k] = draw(g)
        return fired

    got = A.BatchAugment(A.default_pipeline(), n_transform_imgs=0.5, seed=11).draw(16, 32, 32)
    assert got == restated([(0.5, lambda g: None), (0.5, lambda g: None)], 11, 16, 0.5, 32, 32) and got
    pipe = A.Compose([A.HorizontalFlip(p=0.5), A.Rotate(limit=30, p=0.7), A.ShiftScaleRotate(p=0.4)])
    got = A.BatchAugment(pipe, n_transform_imgs=0.5, seed=12).draw(16, 32, 32)
    ssr = lambda g: (float(g.uniform(-45, 45)), 1.0 + float(g.uniform(-0.1, 0.1)), float(g.uniform(-0.0625, 0.0625)), float(g.uniform(-0.0625, 0.0625)))
    assert got == restated([(0.5, lambda g: None), (0.7, lambda g: float(g.uniform(-30, 30))), (0.4, ssr)], 12, 16, 0.5, 32, 32)
    assert any(k == 1 for _, k in got) and any(k == 2 for _, k in got)
    assert hasattr(A.BatchAugment(A.default_pipeline()), "flip_flags")
    # a field transform draws only when it fires, after the transforms in front of it
    pipe = A.Compose([A.HorizontalFlip(p=0.5), A.OpticalDistortion(p=0.5), A.Rotate(limit=30, p=0.7)])
    got = A.BatchAugment(pipe, n_transform_imgs=0.5, seed=12).draw(16, 32, 32)
    opt = lambda g: (float(g.uniform(-0.05, 0.05)), float(g.uniform(-0.05, 0.05)) * 32, float(g.uniform(-0.05, 0.05)) * 32)
    assert got == restated([(0.5, lambda g: None), (0.5, opt), (0.7, lambda g: float(g.uniform(-30, 30)))], 12, 16, 0.5, 32, 32)


@pytest.mark.parametrize("kind", F.KINDS)
def test_remap_cases_keep_rounding_ties_under_the_cap(kind):
    """the inputs of the GPU remap tests (field_ref.remap_case), judged by the reference alone: at most 1 % of the pixels lie within 1e-3
    of a nearest-neighbour tie, every case has an unfired image or a single one, and dense fields reach past the image"""
    for shape in F.SHAPES:
        n, _, H, W = shape
        params, fired, pre, sx, sy = F.remap_case(shape, kind)
        assert F.tie_coords(sx, sy).mean() <= 0.01, (shape, F.tie_coords(sx, sy).mean())
        assert sx.shape == sy.shape == (n, H, W) and pre.shape == (n, 6) and (n == 1 or not fired[-1]) and fired[0]
        if kind == "dense":
            assert np.abs(params).max() > 1.4 * W and (params[:, :, 0] == np.round(params[:, :, 0])).all()


# ------------------------------------------------------------------------------------------- the reference against scipy
SCIPY_MODES = {4: "mirror", 2: "reflect", 1: "nearest", 0: "grid-constant"}


@pytest.mark.parametrize("border", [0, 1, 2, 4])
def test_remap_reference_against_scipy_map_coordinates(border):
    ndi = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(border)
    H, W = 13, 9
    img = g.random((2, 2, H, W))
    x, y = F.pixel_grid(H, W)
    sx = x[None] + g.uniform(-1.5 * W, 1.5 * W, (2, H, W))
    sy = y[None] + g.uniform(-1.5 * H, 1.5 * H, (2, H, W))
    got = F.remap_ref(img, sx, sy, 1, border, 0.375)
    for j in range(2):
        for c in range(2):
            want = ndi.map_coordinates(img[j, c], [sy[j], sx[j]], order=1, mode=SCIPY_MODES[border], cval=0.375)
            np.testing.assert_allclose(got[j, c], want, rtol=0, atol=1e-12)
    # nearest: order 0 rounds half to even where the reference takes floor(s + 0.5), so compare off the ties
    off = ~F.tie_coords(sx, sy, 1e-9)
    near = F.remap_ref(img, sx, sy, 0, border, 0.375)
    for j in range(2):
        want = ndi.map_coordinates(img[j, 0], [sy[j], sx[j]], order=0, mode=SCIPY_MODES[border], cval=0.375)
        np.testing.assert_array_equal(near[j, 0][off[j]], want[off[j]])


@pytest.mark.parametrize("H,W,k", [(32, 32, 401), (7, 5, 33), (1, 9, 17), (48, 80, 49)])
def test_smoothing_reference_against_scipy_correlate1d(H, W, k):
    ndi = pytest.importorskip("scipy.ndimage")
    plane = np.random.default_rng(k).uniform(-1, 1, (H, W))
    taps = F.gauss_taps(k / 8.0, k)
    want = ndi.correlate1d(ndi.correlate1d(plane, taps.astype(np.float64), axis=1, mode="mirror"), taps.astype(np.float64), axis=0, mode="mirror")
    np.testing.assert_allclose(F.smooth(plane, taps), want, rtol=0, atol=1e-12)
