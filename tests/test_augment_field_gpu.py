"""The non-rigid augmentations on the device: unet_warp_field / unet_warp_field_mask / unet_elastic_field against the fp64 restatement
(tests/field_ref.py), purity of the elastic field, exact identities, guard bands, the batched pipeline against per-image sequential
application of the same draws, both feeds, and a short fit."""
import math

import numpy as np
import pytest
import torch

import field_ref as F
from guard import canary_input, guarded
from unet_amd import _lib as L
from unet_amd import augment as A
from unet_amd import ops

pytestmark = pytest.mark.gpu

IMG_TOL = 1e-4
BORDERS = (0, 1, 2, 4)


def _check_masks(got: np.ndarray, want: np.ndarray, ties: np.ndarray, what):
    assert ties.mean() <= 0.01, (what, ties.mean())
    bad = (got != want) & ~ties
    assert not bad.any(), (what, int(bad.sum()))


def _dev(params, kind):
    return torch.from_numpy(params).cuda() if kind == "dense" else params


# at 512 x 512 two (border, interp) pairs per kind, every border and both interpolations between them; all eight at the small shapes
BIG = {"dense": ((4, 1), (0, 1)), "grid": ((2, 1), (1, 0)), "optical": ((4, 0), (0, 1))}


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_remap_against_the_fp64_reference(shape, kind):
    n, Cc, H, W = shape
    g = np.random.default_rng(H * W + Cc)
    img = torch.from_numpy(g.random(shape, dtype=np.float32))
    cls = torch.from_numpy(g.integers(0, 7, (n, H, W)))
    reg = torch.from_numpy(g.normal(size=(n, H, W)).astype(np.float32))
    params, fired, pre, sx, sy = F.remap_case(shape, kind)
    ties = F.tie_coords(sx, sy)
    xd, cd, rd, pd = img.cuda(), cls.cuda(), reg.cuda(), _dev(params, kind)
    pairs = BIG[kind] if H == 512 else [(b, i) for b in BORDERS for i in (0, 1)]
    worst = 0.0
    for border, interp in pairs:
        fill, mfill = (0.375, 5) if border == 0 else (0.0, 0)
        out = torch.empty_like(xd)
        ops.warp_field(xd, out, kind, pd, fired, pre, interp, border, fill)
        err = np.abs(out.cpu().numpy() - F.remap_ref(img.numpy(), sx, sy, interp, border, fill)).max()
        worst = max(worst, err)
        assert err <= IMG_TOL, (border, interp, err)
    print(f"remap {kind} {shape}: max error {worst:.3e}")
    for border in sorted({b for b, _ in pairs}):
        mfill = 5 if border == 0 else 0
        co, ro = torch.empty_like(cd), torch.empty_like(rd)
        ops.warp_field_mask(cd, co, kind, pd, fired, pre, border, mfill)
        ops.warp_field_mask(rd, ro, kind, pd, fired, pre, border, mfill)
        _check_masks(co.cpu().numpy(), F.remap_mask_ref(cls.numpy(), sx, sy, border, mfill), ties, ("int64", border))
        _check_masks(ro.cpu().numpy(), F.remap_mask_ref(reg.numpy(), sx, sy, border, mfill), ties, ("fp32", border))
    assert torch.equal(xd.cpu(), img) and torch.equal(cd.cpu(), cls) and torch.equal(rd.cpu(), reg)      # the sources are untouched
    if kind == "dense":
        assert torch.equal(pd.cpu(), torch.from_numpy(params))


ELASTIC = [  # (n, H, W), sigma, approximate, alpha, same_dxdy
    ((3, 48, 80), 4, False, 1.0, False), ((3, 48, 80), 6, False, 120.0, True), ((2, 32, 32), 50, False, 120.0, False),
    ((2, 7, 5), 50, False, 1.0, True), ((1, 1, 9), 4, False, 120.0, False), ((2, 7, 5), 50, True, 1.0, False),
    ((3, 48, 80), 50, True, 120.0, True), ((2, 512, 512), 6, False, 120.0, False), ((2, 32, 32), 6, False, 1.0, True)]


@pytest.mark.parametrize("shape,sigma,approximate,alpha,same", ELASTIC)
def test_elastic_field_against_the_fp64_reference(shape, sigma, approximate, alpha, same):
    n, H, W = shape
    t = A.ElasticTransform(alpha=alpha, sigma=sigma, approximate=approximate, same_dxdy=same)
    assert t.ksize == {(4, False): 33, (6, False): 49, (50, False): 401}.get((sigma, approximate), 17)
    g = np.random.default_rng(t.ksize + H)
    keys = g.integers(0, 2 ** 32, (n, 2))
    field, ws = torch.empty(n, 2, H, W, device="cuda"), torch.empty(n, 2, H, W, device="cuda")
    ops.elastic_field(field, ws, keys, alpha, [True] * n, same, t.taps)
    got = field.cpu().numpy().astype(np.float64)
    bound = (2 * t.ksize + 4) * 2.0 ** -24 * alpha
    worst = 0.0
    for j in range(n):
        want = F.elastic_field_ref(keys[j], alpha, t.taps, same, H, W)
        worst = max(worst, np.abs(got[j] - want).max())
    print(f"elastic field {shape} sigma {sigma} ksize {t.ksize} alpha {alpha}: max error {worst:.3e} (bound {bound:.3e}, "
          f"{worst / (2.0 ** -24 * alpha):.2f} x 2^-24 alpha)")
    assert worst <= bound, (worst, bound)
    assert np.abs(got).max() > 0 and (same == bool(np.array_equal(got[:, 0], got[:, 1])))


def test_elastic_field_is_pure_and_unfired_images_copy():
    n, H, W = 5, 48, 80
    t = A.ElasticTransform(alpha=30.0, sigma=4)
    g = np.random.default_rng(17)
    keys = g.integers(0, 2 ** 32, (n, 2))
    fired = [True, False, True, True, True]
    alphas = np.array([30.0, 1.0, 2.5, 30.0, 7.0], np.float32)
    new = lambda m: (torch.full((m, 2, H, W), float("nan"), device="cuda"), torch.full((m, 2, H, W), float("nan"), device="cuda"))
    whole, ws = new(n)
    ops.elastic_field(whole, ws, keys, alphas, fired, False, t.taps)
    assert not torch.isnan(whole).any()
    for j in range(n):                                       # image by image
        one, w1 = new(1)
        ops.elastic_field(one, w1, keys[j:j + 1], alphas[j:j + 1], fired[j:j + 1], False, t.taps)
        assert torch.equal(one[0].view(torch.int32), whole[j].view(torch.int32)), j
    for cut in (1, 2, 4):                                    # any chunking
        parts = []
        for a, b in ((0, cut), (cut, n)):
            f, w = new(b - a)
            ops.elastic_field(f, w, keys[a:b], alphas[a:b], fired[a:b], False, t.taps)
            parts.append(f)
        assert torch.equal(torch.cat(parts).view(torch.int32), whole.view(torch.int32)), cut
    assert torch.equal(whole[1].view(torch.int32), torch.zeros(2, H, W, dtype=torch.int32, device="cuda"))     # unfired: +0.0 everywhere
    # ... and an exact copy through the remap, whatever the image holds
    x = torch.randn(n, 3, H, W, device="cuda")
    x[1, 0, 0, :3] = torch.tensor([-0.0, float("inf"), 1e-40])
    for interp in (0, 1):
        out = torch.empty_like(x)
        ops.warp_field(x, out, "dense", whole, fired, None, interp, 0, 0.5)
        assert torch.equal(out[1].view(torch.int32), x[1].view(torch.int32))
        assert not torch.equal(out[0], x[0])
    # the same key gives the same field at any batch position; another key another field
    again, w2 = new(2)
    ops.elastic_field(again, w2, keys[[3, 0]], alphas[[3, 0]], [True, True], False, t.taps)
    assert torch.equal(again[1], whole[0]) and torch.equal(again[0], whole[3]) and not torch.equal(whole[0], whole[3])


def test_identities_are_exact():
    n, H, W = 3, 40, 72
    g = torch.Generator().manual_seed(4)
    x = torch.randn(n, 4, H, W, generator=g).cuda()
    x[0, 0, :1, :3] = torch.tensor([-0.0, float("inf"), 1e-40]).cuda()
    y = torch.randint(-5, 9, (n, H, W), generator=g).cuda()
    yf = torch.randn(n, H, W, generator=g).cuda()
    zero = torch.empty(n, 2, H, W, device="cuda")
    t = A.ElasticTransform(alpha=0, sigma=4)
    ops.elastic_field(zero, torch.empty_like(zero), [(1, 2), (3, 4), (5, 6)], 0.0, [True] * n, False, t.taps)
    assert (zero == 0).all()                                 # alpha = 0
    cases = [("dense", zero), ("optical", np.zeros((n, 3), np.float32))]
    for kind, params in cases:
        for border in BORDERS:
            for interp in (0, 1):
                out = torch.empty_like(x)
                ops.warp_field(x, out, kind, params, [True] * n, None, interp, border, 0.5)
                assert torch.equal(out.view(torch.int32), x.view(torch.int32)), (kind, border, interp)
            for m in (y, yf):
                mo = torch.empty_like(m)
                ops.warp_field_mask(m, mo, kind, params, [True] * n, None, border, 3)
                assert torch.equal(mo, m), (kind, border)
    # a grid whose factors are all 1 maps every cell onto itself up to the linspace's own end point: cells of one pixel are the identity
    nodes = np.zeros((1, 2, 17), np.float32)
    nodes[0, :, :10] = np.arange(10)
    xs = torch.randn(1, 2, 9, 9, device="cuda")
    out = torch.empty_like(xs)
    ops.warp_field(xs, out, "grid", (1, 1, nodes), [True], None, 1, 4, 0.0)
    assert torch.equal(out, xs)


def test_a_translation_is_the_same_bits_through_the_affine_and_the_field_warp():
    """Two entry points, one sampler (csrc/warp_sample.h): a pure translation through warp_affine[_mask] and through warp_field[_mask]
    (optical with k = 0 and shift (dx, dy), all images fired, identity pre-map) gives the same bits.  Both paths form x + dx in fp64 from
    exactly representable operands -- on the optical path (x - c) * 0 = +-0 -- and share the sampler from there on.  The shifts: a
    fractional one, one far outside the image, an exact rounding tie.  (No D4 pre-maps here: a flipped sample uses the weights 1 - fx and
    another summation order, so it is not bit-equal.)"""
    shifts = np.array([(2.25, -3.5), (-0.75, 100.125), (0.5, 0.5)], np.float32)
    maps = np.array([(1, 0, dx, 0, 1, dy) for dx, dy in shifts], np.float32)
    optical = np.concatenate([np.zeros((3, 1), np.float32), shifts], axis=1)
    g = torch.Generator().manual_seed(12)
    for shape in ((3, 3, 40, 72), (3, 1, 1, 9)):
        n, _, H, W = shape
        x = torch.randn(shape, generator=g).cuda()
        masks = (torch.randint(-5, 9, (n, H, W), generator=g).cuda(), torch.randn(n, H, W, generator=g).cuda())
        for border in BORDERS:
            for interp in (0, 1):
                a, f = torch.empty_like(x), torch.empty_like(x)
                ops.warp_affine(x, a, maps, interp, border, 0.375)
                ops.warp_field(x, f, "optical", optical, [True] * n, None, interp, border, 0.375)
                assert torch.equal(a.view(torch.int32), f.view(torch.int32)) and not torch.equal(a, x), (shape, border, interp)
            for m in masks:
                a, f = torch.empty_like(m), torch.empty_like(m)
                ops.warp_affine_mask(m, a, maps, border, 5)
                ops.warp_field_mask(m, f, "optical", optical, [True] * n, None, border, 5)
                bits = torch.int64 if m.dtype == torch.int64 else torch.int32
                assert torch.equal(a.view(bits), f.view(bits)) and not torch.equal(a, m), (shape, border, m.dtype)


@pytest.mark.parametrize("field", ["elastic", "grid", "optical"])
def test_d4_in_front_of_a_field_transform_is_one_launch_and_the_same_bits(field):
    """[flips, Transpose, RandomRotate90, field] is ONE segment; it equals the torch permutations followed by the field transform alone"""
    B, N = 16, 32
    make = {"elastic": lambda: A.ElasticTransform(alpha=40, sigma=4, border_mode=2, p=0.7),
            "grid": lambda: A.GridDistortion(distort_limit=0.5, border_mode=0, value=0.25, mask_value=7, p=0.7),
            "optical": lambda: A.OpticalDistortion(distort_limit=1.0, shift_limit=0.2, border_mode=4, p=0.7)}[field]
    pipe = lambda: A.Compose([A.HorizontalFlip(p=0.5), A.VerticalFlip(p=0.5), A.Transpose(p=0.5), A.RandomRotate90(p=0.5), make()])
    g = torch.Generator().manual_seed(8)
    x = torch.rand(B, 3, N, N, generator=g).cuda()
    for mask_dtype in (torch.int64, torch.float32):
        y = torch.randint(0, 5, (B, N, N), generator=g).to(mask_dtype).cuda()
        ba = A.BatchAugment(pipe(), n_transform_imgs=0.5, seed=31)
        assert ba.plan() == [("warp", [0, 1, 2, 3, 4])]
        fired = A.BatchAugment(pipe(), n_transform_imgs=0.5, seed=31).draw(B, N, N)
        assert any(k == 4 for _, k in fired) and any(k == 2 for _, k in fired) and any((i, 4) not in fired and (i, 0) in fired for i in range(8))
        got_x, got_y = ba(x.clone(), y.clone())
        t = ba.aug.transforms[4]
        d4 = [lambda a: a.flip(-1), lambda a: a.flip(-2), lambda a: a.transpose(-1, -2), None]
        for i in range(B):
            xi, yi = x[i], y[i]
            for k in range(4):
                if (i, k) in fired:
                    f = (lambda a, r=fired[i, 3]: torch.rot90(a, r, (-2, -1))) if k == 3 else d4[k]
                    xi, yi = f(xi), f(yi)
            if (i, 4) in fired:
                xi, yi = t.apply_params(xi.contiguous(), yi.contiguous(), fired[i, 4])
            assert torch.equal(got_x[i].view(torch.int32), xi.contiguous().view(torch.int32)), (field, i)
            assert torch.equal(got_y[i], yi), (field, i)


def test_guard_bands_odd_shapes_and_a_batch_over_the_cap():
    """every output inside guard bands, every input inside canaries: nothing is written outside the outputs, and a read outside an input
    would carry the canary (-3e7) into an image that is bounded by 1"""
    for (n, Cc, H, W) in F.SHAPES[:4] + [(L.FIELD_MAX_IMAGES + 1, 2, 7, 5)]:
        g = np.random.default_rng(n + H)
        img, chk_img = canary_input(torch.from_numpy(g.random((n, Cc, H, W), dtype=np.float32)))
        reg, chk_reg = canary_input(torch.from_numpy(g.random((n, H, W), dtype=np.float32)))
        cls = torch.from_numpy(g.integers(0, 7, (n, H, W))).cuda()
        t = A.ElasticTransform(alpha=1.5 * W, sigma=50 if H == 32 else 4, approximate=H == 7)
        keys = g.integers(0, 2 ** 32, (n, 2))
        field, chk_field = guarded((n, 2, H, W), torch.float32, fill=float("nan"))
        ws, chk_ws = guarded((n, 2, H, W), torch.float32, fill=float("nan"))
        fired = [j != 1 for j in range(n)]
        ops.elastic_field(field, ws, keys, t.alpha, fired, False, t.taps)
        chk_field("elastic field"), chk_ws("elastic workspace")
        assert torch.isfinite(field).all() and float(field.abs().max()) <= 1.5 * W
        steps = 5 if min(H, W) >= 10 else max(H, W)
        nodes = np.stack([np.stack([A.grid_nodes(W, steps, 1.0 + g.uniform(-0.9, 0.9, steps + 1))[1],
                                    A.grid_nodes(H, steps, 1.0 + g.uniform(-0.9, 0.9, steps + 1))[1]]) for _ in range(n)])
        opt = np.stack([g.uniform(-8, 8, n), g.uniform(-2, 2, n) * W, g.uniform(-2, 2, n) * H], axis=1)
        for kind, params in (("dense", field), ("grid", (max(W // steps, 1), max(H // steps, 1), nodes)), ("optical", opt)):
            for border in BORDERS:
                for interp in (0, 1):
                    out, chk = guarded((n, Cc, H, W), torch.float32, fill=float("nan"))
                    ops.warp_field(img, out, kind, params, fired, None, interp, border, 0.5)
                    chk(f"warp_field {kind} {border} {interp}")
                    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0 + 1e-6, (kind, border, interp)        # no canary, no NaN
                mo, chk = guarded((n, H, W), torch.float32, fill=float("nan"))
                ops.warp_field_mask(reg, mo, kind, params, fired, None, border, 0.5)
                chk(f"warp_field_mask fp32 {kind} {border}")
                assert float(mo.min()) >= 0.0 and float(mo.max()) <= 1.0
                mo, chk = guarded((n, H, W), torch.int64, fill=-77)
                ops.warp_field_mask(cls, mo, kind, params, fired, None, border, 5)
                chk(f"warp_field_mask int64 {kind} {border}")
                assert int(mo.min()) >= 0 and int(mo.max()) <= 6
        chk_img("image"), chk_reg("mask"), chk_field("field after the warps")
    # a field that holds NaN, infinities and huge values samples inside the image all the same
    n, Cc, H, W = 2, 3, 7, 5
    img, _ = canary_input(torch.rand(n, Cc, H, W))
    wild = torch.tensor([float("nan"), float("inf"), -float("inf"), 3e38, -1e30, 2.0 ** 24, 0.5]).repeat(n * 2 * H * W // 7 + 1)[:n * 2 * H * W]
    wild = wild.view(n, 2, H, W).cuda()
    for border in BORDERS:
        for interp in (0, 1):
            out, chk = guarded((n, Cc, H, W), torch.float32, fill=float("nan"))
            ops.warp_field(img, out, "dense", wild, [True] * n, None, interp, border, 0.5)
            chk("wild field")
            assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0


def test_elastic_field_over_the_per_call_cap():
    n, H, W = L.ELASTIC_MAX_IMAGES + 1, 7, 5
    t = A.ElasticTransform(alpha=3, sigma=4)
    keys = np.random.default_rng(0).integers(0, 2 ** 32, (n, 2))
    field, chk = guarded((n, 2, H, W), torch.float32, fill=float("nan"))
    ws, chk_ws = guarded((n, 2, H, W), torch.float32, fill=float("nan"))
    ops.elastic_field(field, ws, keys, 3.0, [True] * n, False, t.taps)
    chk("field"), chk_ws("workspace")
    got = field.cpu().numpy()
    for j in (0, 63, 64):
        assert np.abs(got[j] - F.elastic_field_ref(keys[j], 3.0, t.taps, False, H, W)).max() <= (2 * 33 + 4) * 2.0 ** -24 * 3


PIPE = lambda: A.Compose([A.HorizontalFlip(p=0.5), A.VerticalFlip(p=0.5), A.ElasticTransform(alpha=30, sigma=4, p=0.6),
                          A.Rotate(limit=45, border_mode=2, p=0.6), A.GaussNoise(p=0.5), A.RandomRotate90(p=0.5),
                          A.GridDistortion(border_mode=0, value=0.25, mask_value=9, p=0.6), A.OpticalDistortion(distort_limit=0.5, shift_limit=0.1, p=0.6)])


def _field_coords(t, prm, H, W):
    """the fp64 source coordinates [1, H, W] of one application of a field transform, from the reference's own maps"""
    if isinstance(t, A.ElasticTransform):
        return F.dense_coords(F.elastic_field_ref(prm, t.alpha, t.taps, t.same_dxdy, H, W)[None])
    if isinstance(t, A.GridDistortion):
        sx, sy, nodes = t.field_params([prm], H, W, "cpu")
        return F.grid_coords(sx, sy, nodes, H, W)
    return F.optical_coords(np.array([prm], np.float32), H, W)


def _sequential(pipe, fired, x: torch.Tensor, y: torch.Tensor):
    """image by image, transform by transform, through the fp64 references, on the CPU; also tracks which mask pixels descend from a
    nearest-neighbour rounding tie"""
    from warp_ref import tie_pixels, warp_mask_ref, warp_ref
    B, _, H, W = x.shape
    xs, ys, ts = [], [], []
    for i in range(B):
        xi, yi = x[i].double().numpy(), y[i].numpy()
        tie = np.zeros((H, W), bool)
        for k, t in enumerate(pipe.transforms):
            if (i, k) not in fired:
                continue
            prm = fired[i, k]
            if isinstance(t, A._Field):
                sx, sy = _field_coords(t, prm, H, W)
                interp, border, fill, mfill = t.modes()
                xi = F.remap_ref(xi[None], sx, sy, interp, border, fill)[0]
                yi = F.remap_mask_ref(yi[None], sx, sy, border, mfill)[0]
                tie = F.remap_mask_ref(tie[None], sx, sy, border, False)[0] | F.tie_coords(sx, sy)[0]
            elif isinstance(t, A._Geometric):
                inv = A.inverse_map(t.matrix(prm, H, W))[None]
                interp, border, fill, mfill = t.modes()
                xi = warp_ref(xi[None], inv, interp, border, fill)[0]
                yi = warp_mask_ref(yi[None], inv, border, mfill)[0]
                tie = warp_mask_ref(tie[None], inv, border, False)[0] | tie_pixels(inv, H, W)[0]
            else:
                xo, _ = t.apply_params(torch.from_numpy(xi), torch.from_numpy(yi), prm)
                xi = xo.numpy()
        xs.append(xi), ys.append(yi), ts.append(tie)
    return np.stack(xs), np.stack(ys), np.stack(ts)


@pytest.mark.parametrize("mask_dtype", [torch.int64, torch.float32])
def test_pipeline_equals_sequential_application(mask_dtype):
    B, H, W = 12, 64, 64
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 4, H, W, generator=g)
    y = torch.randint(0, 5, (B, H, W), generator=g).to(mask_dtype)
    ba = A.BatchAugment(PIPE(), n_transform_imgs=0.5, seed=23)
    assert ba.plan() == [("warp", [0, 1, 2]), ("warp", [3]), ("pixel", [4]), ("warp", [5, 6]), ("warp", [7])]
    fired = A.BatchAugment(PIPE(), n_transform_imgs=0.5, seed=23).draw(B, H, W, 4)
    assert all(any(k == q for _, k in fired) for q in range(8))
    xd, yd = x.cuda(), y.cuda()
    xa, ya = ba(xd, yd)
    assert xa is xd and ya is yd                                     # in place, as the flip path
    want_x, want_y, ties = _sequential(ba.aug, fired, x, y)
    got_x, got_y = xa.cpu(), ya.cpu()
    err = np.abs(got_x.numpy() - want_x).max()
    print(f"pipeline max error {err:.3e}, tied mask pixels {ties.mean():.4f}")
    assert err <= IMG_TOL
    _check_masks(got_y.numpy(), want_y, ties, "pipeline")
    assert torch.equal(got_x[6:].view(torch.int32), x[6:].view(torch.int32)) and torch.equal(got_y[6:], y[6:])     # outside the slice
    xb, yb = A.BatchAugment(PIPE(), n_transform_imgs=0.5, seed=23)(x.cuda(), y.cuda())      # the same seed twice: identical batches
    assert torch.equal(xb.view(torch.int32), xa.view(torch.int32)) and torch.equal(yb, ya)


def _tiles(n, n_in, size, seed, n_cls=4):
    g = np.random.default_rng(seed)
    return ([g.integers(0, 256, (n_in, *size)).astype(np.uint8) for _ in range(n)],
            [g.integers(0, n_cls, size).astype(np.uint8) for _ in range(n)])


FIT_PIPE = lambda: A.Compose([A.HorizontalFlip(p=0.5), A.VerticalFlip(p=0.5), A.ElasticTransform(alpha=20, sigma=4, p=0.5),
                              A.GridDistortion(p=0.5), A.OpticalDistortion(p=0.5)])


def test_field_pipeline_through_either_feed(tmp_path):
    """the device feed and feed="host" hand the step identical batches, from tiles resident in memory and from tile files"""
    from unet_amd.learner import DataLoader, TileDataset
    imgs, masks = _tiles(7, 4, (48, 48), 4)
    pi, pm = [], []
    for i, (a, m) in enumerate(zip(imgs, masks)):
        np.save(tmp_path / f"i{i}.npy", a), np.save(tmp_path / f"m{i}.npy", m)
        pi.append(tmp_path / f"i{i}.npy"), pm.append(tmp_path / f"m{i}.npy")
    tfm = lambda: A.BatchAugment(FIT_PIPE(), n_transform_imgs=0.5, seed=13)
    assert not hasattr(tfm(), "flip_flags")
    runs = []
    for regression in (False, True):
        mk = [m.astype(np.float32) * 0.5 for m in masks] if regression else masks
        sets = [TileDataset(imgs, mk, "int8", regression=regression)] + ([] if regression else [TileDataset(pi, pm, "int8")])
        for ds in sets:
            host = list(DataLoader(ds, 3, True, "cuda", seed=5, batch_tfm=tfm(), feed="host"))
            dev = list(DataLoader(ds, 3, True, "cuda", seed=5, batch_tfm=tfm(), feed="device"))
            for (xa, ya), (xb, yb) in zip(host, dev):
                assert torch.equal(xa, xb) and torch.equal(ya, yb)
            runs.append(dev)
    for (xa, ya), (xb, yb) in zip(runs[0], runs[1]):                  # resident and file-fed: the same batches
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
    raw = torch.from_numpy(np.stack(imgs).astype(np.float32) / 255.0)
    assert any(not any(torch.equal(xb[0].cpu(), r) or torch.equal(xb[0].cpu(), r.flip(-1)) or torch.equal(xb[0].cpu(), r.flip(-2))
                       or torch.equal(xb[0].cpu(), r.flip(-1, -2)) for r in raw) for xb, _ in runs[0])      # something was warped


def test_three_steps_of_fit_with_a_field_pipeline(tmp_path):
    """fit_one_cycle over tile files with flips and the three field transforms: finite losses, and two seeded runs end with identical
    losses and parameters (the field and the warps are deterministic)"""
    from unet_amd.learner import CrossEntropyLossFlat, DataLoaders, Learner, TileDataset
    from unet_amd.model import HipDynamicUnet
    imgs, masks = _tiles(6, 4, (64, 64), 6, n_cls=3)
    pi, pm = [], []
    for i, (a, m) in enumerate(zip(imgs, masks)):
        np.save(tmp_path / f"i{i}.npy", a)
        np.save(tmp_path / f"m{i}.npy", m)
        pi.append(tmp_path / f"i{i}.npy")
        pm.append(tmp_path / f"m{i}.npy")
    res = []
    for _ in range(2):
        torch.manual_seed(3)
        model = HipDynamicUnet("xresnet18", 4, 3, (64, 64))
        dls = DataLoaders(TileDataset(pi, pm, "int8"), TileDataset(pi[:2], pm[:2], "int8"), 2, vocab=list("abc"), seed=7,
                          train_tfm=A.BatchAugment(FIT_PIPE(), n_transform_imgs=0.5, seed=2))
        learn = Learner(dls, model, loss_func=CrossEntropyLossFlat(axis=1), path=tmp_path)
        learn._no_logging = True
        learn.fit_one_cycle(1, lr_max=1e-3)
        torch.cuda.synchronize()
        res.append((list(learn.recorder.losses), model.flat_param.detach().clone()))
    (la, pa), (lb, pb) = res
    assert len(la) == 3 and all(math.isfinite(v) for v in la) and la == lb
    assert torch.equal(pa, pb)
