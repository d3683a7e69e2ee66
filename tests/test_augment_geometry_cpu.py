"""Geometric augmentations (unet_amd.augment RandomRotate90 / Transpose / Rotate / ShiftScaleRotate) without a GPU: forward matrices,
D4 composition, snapping, draw order, segment split, refusals, and the host-side argument checks of unet_warp_affine[_mask]."""
import math

import numpy as np
import pytest
import torch

from unet_amd import augment as A
from warp_ref import warp_mask_ref


def _formula(angle, s, cx, cy):
    a, b = s * math.cos(math.radians(angle)), s * math.sin(math.radians(angle))
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]])


def _apply_fwd(m, H, W, grid):
    """the D4 map m (3 x 3 forward) applied to an integer image by scattering: out[m (x, y)] = grid[y, x]"""
    out = np.full_like(grid, -1)
    for y in range(H):
        for x in range(W):
            u, v, _ = m @ np.array([x, y, 1.0])
            out[int(round(v)), int(round(u))] = grid[y, x]
    return out


def test_forward_matrices_follow_get_rotation_matrix_2d():
    H, W = 40, 56
    cx, cy = (W - 1) / 2, (H - 1) / 2
    for angle in (-170.0, -33.3, 0.0, 12.5, 90.0):
        np.testing.assert_allclose(A.Rotate(limit=(angle, angle)).matrix(angle, H, W)[:2], _formula(angle, 1.0, cx, cy), atol=1e-12)
    t = A.ShiftScaleRotate()
    m = t.matrix((25.0, 1.3, 0.05, -0.02), H, W)
    want = _formula(25.0, 1.3, cx, cy)
    want[0, 2] += 0.05 * W
    want[1, 2] += -0.02 * H
    np.testing.assert_allclose(m[:2], want, atol=1e-12)
    # the inverse map sends the output pixel back to its source
    inv = A.inverse_map(m).astype(np.float64).reshape(2, 3)
    src = np.array([7.0, 11.0, 1.0])
    out = m @ src
    np.testing.assert_allclose(inv @ out, src[:2], atol=1e-4)


def test_d4_maps_are_the_numpy_permutations():
    N = 5
    grid = np.arange(N * N).reshape(N, N)
    rr = A.RandomRotate90()
    for k in range(4):
        assert np.array_equal(_apply_fwd(rr.matrix(k, N, N), N, N, grid), np.rot90(grid, k))
    assert np.array_equal(_apply_fwd(A.Transpose().matrix(None, N, N), N, N, grid), grid.T)
    assert np.array_equal(_apply_fwd(A.HorizontalFlip().matrix(None, N, N), N, N, grid), grid[:, ::-1])
    assert np.array_equal(_apply_fwd(A.VerticalFlip().matrix(None, N, N), N, N, grid), grid[::-1])
    # composition table: any product of D4 maps, as an inverse map through the nearest warp, is the sequential numpy result
    g = np.random.default_rng(0)
    ops = [("h", A.HorizontalFlip().matrix(None, N, N), lambda a: a[:, ::-1]), ("v", A.VerticalFlip().matrix(None, N, N), lambda a: a[::-1]),
           ("t", A.Transpose().matrix(None, N, N), lambda a: a.T)] + \
          [(f"r{k}", rr.matrix(k, N, N), (lambda k: lambda a: np.rot90(a, k))(k)) for k in range(4)]
    seen = set()
    for _ in range(60):
        pick = [ops[i] for i in g.integers(0, len(ops), size=int(g.integers(1, 5)))]
        fwd, want = np.eye(3), grid
        for _, m, f in pick:
            fwd, want = m @ fwd, f(want)
        inv = A.inverse_map(fwd)
        assert set(np.unique(inv)) <= {-1.0, 0.0, 1.0, float(N - 1)}, inv          # exact: entries are integers after snapping
        for border in (0, 1, 2, 4):
            assert np.array_equal(warp_mask_ref(grid[None], inv[None], border)[0], want)
        seen.add(want.tobytes())
    assert len(seen) == 8                      # all eight elements of D4 were reached


def test_rotate_by_multiples_of_90_is_the_snapped_exact_map():
    N = 512
    rr = A.RandomRotate90()
    for angle, k in ((90, 1), (180, 2), (-90, 3), (270, 3), (-180, 2)):
        t = A.Rotate(limit=(angle, angle), p=1.0)
        g = np.random.default_rng(1)
        a = t.get_params(g, N, N)
        assert a == angle
        assert np.array_equal(A.inverse_map(t.matrix(a, N, N)), A.inverse_map(rr.matrix(k, N, N)))
    inv = A.inverse_map(A.Rotate().matrix(90.0, N, N))
    assert inv.dtype == np.float32 and np.array_equal(inv, np.array([0, -1, N - 1, 1, 0, 0], np.float32))
    assert np.array_equal(A.inverse_map(np.eye(3)), np.array([1, 0, 0, 0, 1, 0], np.float32))
    # only near-multiples of 0.5 are snapped
    m = A.Rotate().matrix(10.0, N, N)
    np.testing.assert_allclose(A.inverse_map(m), np.linalg.inv(m)[:2].reshape(6), rtol=1e-6)


def test_draws_follow_per_image_compose_calls():
    pipe = A.Compose([A.HorizontalFlip(p=0.5), A.RandomRotate90(p=0.7), A.ShiftScaleRotate(p=0.6),
                      A.RandomBrightnessContrast(p=0.5), A.CoarseDropout(p=0.5), A.Rotate(p=0.5), A.Transpose(p=0.5)], p=0.9)
    B, H, W = 12, 32, 32
    ba = A.BatchAugment(pipe, n_transform_imgs=0.75, seed=4)
    fired = ba.draw(B, H, W)
    # the same stream consumed by per-image Compose semantics (p draw first, parameters only when the transform fires)
    g = np.random.default_rng(4)
    want = {}
    for i in list(range(B))[:math.ceil(B * 0.75) - B]:
        if g.random() >= pipe.p:
            continue
        for k, t in enumerate(pipe.transforms):
            if g.random() < t.p:
                want[i, k] = t.get_params(g, H, W)
    assert fired.keys() == want.keys() and len(fired) > 5
    for key in want:
        assert repr(fired[key]) == repr(want[key])
    assert all(i < 9 for i, _ in fired)                 # ceil(12 * 0.75) - 12 = -3: the first 9 images are the candidates
    assert ba.g.random() == g.random()                  # both streams are at the same place


def test_get_params_then_apply_params_is_apply():
    """the draw / apply split keeps RandomBrightnessContrast and CoarseDropout as they were: same draws, same order, same result"""
    img, mask = torch.rand(3, 24, 20), torch.randint(0, 4, (24, 20))
    for t in (A.RandomBrightnessContrast(p=1.0), A.RandomBrightnessContrast(brightness_by_max=False, p=1.0),
              A.CoarseDropout(max_holes=5, max_height=30, max_width=4, min_holes=2, mask_fill_value=7, p=1.0)):
        g1, g2 = np.random.default_rng(5), np.random.default_rng(5)
        a = t.apply(img, mask, g1)
        b = t.apply_params(img, mask, t.get_params(g2, 24, 20))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and g1.random() == g2.random()
    # the CoarseDropout draws of the former single apply(): holes, then (height, width, y, x) per hole, sizes clipped to the tile
    g = np.random.default_rng(8)
    holes = A.CoarseDropout(max_holes=3, max_height=40, max_width=2, min_holes=3, p=1.0).get_params(g, 24, 20)
    g = np.random.default_rng(8)
    assert int(g.integers(3, 4)) == len(holes) == 3
    for y1, x1, hh, ww in holes:
        h0, w0 = int(g.integers(40, 41)), int(g.integers(2, 3))
        assert (hh, ww) == (min(h0, 24), min(w0, 20))
        assert (y1, x1) == (int(g.integers(0, 24 - hh + 1)), int(g.integers(0, 20 - ww + 1)))


def test_shift_scale_rotate_draw_order_and_limits():
    t = A.ShiftScaleRotate(shift_limit=0.1, scale_limit=(-0.2, 0.3), rotate_limit=(10, 20), shift_limit_y=(0.5, 0.6))
    g, h = np.random.default_rng(2), np.random.default_rng(2)
    angle, scale, dx, dy = t.get_params(g, 8, 8)
    assert angle == h.uniform(10, 20) and scale == 1.0 + h.uniform(-0.2, 0.3)
    assert dx == h.uniform(-0.1, 0.1) and dy == h.uniform(0.5, 0.6)
    r = A.Rotate(limit=30)
    assert r.limit == (-30.0, 30.0) and A.Rotate(limit=(5, 7)).limit == (5.0, 7.0)
    assert A.RandomRotate90().get_params(np.random.default_rng(0), 8, 8) in range(4)


def test_segments_split_mixed_pipelines():
    H, V, R90, T = A.HorizontalFlip(), A.VerticalFlip(), A.RandomRotate90(), A.Transpose()
    Ro, S, RBC, CD = A.Rotate(), A.ShiftScaleRotate(), A.RandomBrightnessContrast(), A.CoarseDropout()
    seg = lambda ts: A.BatchAugment(A.Compose(ts)).segments()
    assert seg([H, V, R90, S, RBC, Ro]) == [[0, 1, 2, 3], 4, [5]]
    assert seg([H, S, V, Ro, T, Ro]) == [[0, 1, 2], [3, 4], [5]]          # a second interpolating transform starts a segment
    assert seg([RBC, R90, CD, T, H]) == [0, [1], 2, [3, 4]]
    assert seg([Ro, S]) == [[0], [1]]
    assert seg([R90]) == [[0]]


def test_refusals():
    with pytest.raises(NotImplementedError, match="wrap"):
        A.Rotate(border_mode=3)
    with pytest.raises(NotImplementedError, match="border_mode"):
        A.ShiftScaleRotate(border_mode=5)
    with pytest.raises(NotImplementedError, match="interpolation=2"):
        A.Rotate(interpolation=2)
    with pytest.raises(NotImplementedError, match="interpolation"):
        A.ShiftScaleRotate(interpolation=4)
    with pytest.raises(NotImplementedError, match="crop_border"):
        A.Rotate(crop_border=True)
    with pytest.raises(NotImplementedError, match="per-channel value"):
        A.Rotate(border_mode=0, value=(1, 2, 3))
    with pytest.raises(NotImplementedError, match="per-channel mask_value"):
        A.ShiftScaleRotate(border_mode=0, mask_value=[1, 2])
    A.Rotate(border_mode=0, value=0.5, mask_value=3)                       # scalars are fine
    for t in (A.RandomRotate90(p=1.0), A.Transpose(p=1.0)):
        ba = A.BatchAugment(A.Compose([t]), n_transform_imgs=0.5)
        with pytest.raises(ValueError, match=f"{type(t).__name__}.*32 x 48"):
            ba(torch.rand(4, 3, 32, 48), torch.zeros(4, 32, 48, dtype=torch.long))


def test_rotate_pipelines_do_not_offer_flip_flags_and_need_the_device():
    assert hasattr(A.BatchAugment(A.default_pipeline()), "flip_flags")
    assert not hasattr(A.BatchAugment(A.Compose([A.RandomRotate90()])), "flip_flags")
    assert not hasattr(A.BatchAugment(A.Compose([A.HorizontalFlip(), A.Rotate()])), "flip_flags")
    ba = A.BatchAugment(A.Compose([A.HorizontalFlip(p=1.0), A.Rotate(p=1.0)]), n_transform_imgs=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ba(torch.rand(4, 3, 16, 16), torch.zeros(4, 16, 16, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.Rotate(p=1.0)(torch.rand(3, 16, 16), torch.zeros(16, 16, dtype=torch.long), np.random.default_rng(0))


def test_warp_entry_points_reject_bad_arguments_on_the_host():
    import ctypes as C
    from unet_amd import _lib as L
    lib = L.lib
    maps = (C.c_float * (6 * 65))(*([1, 0, 0, 0, 1, 0] * 65))
    a, b = 0x10000, 0x20000                  # never dereferenced: every call below is refused before any launch

    def img(*, src=a, dst=b, n=2, Cc=3, H=8, W=8, m=maps, interp=1, border=4, fill=0.0):
        return lib.unet_warp_affine(src, dst, n, Cc, H, W, m, interp, border, fill, None)

    def msk(*, src=a, dst=b, f32=0, n=2, H=8, W=8, m=maps, border=4, fill=0.0):
        return lib.unet_warp_affine_mask(src, dst, f32, n, H, W, m, border, fill, None)

    for rc in (img(src=None), img(dst=None), img(m=None), img(dst=a), img(n=0), img(n=65), img(Cc=0), img(H=0), img(W=-1),
               img(W=(1 << 24) + 1), img(interp=2), img(interp=-1), img(border=3), img(border=5), img(fill=float("nan")),
               img(fill=float("inf")),
               msk(src=None), msk(dst=None), msk(m=None), msk(dst=a), msk(f32=2), msk(n=0), msk(n=65), msk(H=-3), msk(W=0), msk(border=3),
               msk(fill=float("nan")), msk(fill=1e30)):
        assert rc == -1
    assert b"warp_affine" in lib.unet_last_error()
    bad = (C.c_float * 12)(1, 0, 0, 0, 1, 0, 1, 0, float("nan"), 0, 1, 0)
    assert img(m=bad) == -1 and b"non-finite map" in lib.unet_last_error()
    bad[8] = float("inf")
    assert msk(m=bad) == -1 and b"non-finite map" in lib.unet_last_error()
