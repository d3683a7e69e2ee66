"""The pixel-level augmentations on the device: unet_pixel_ops / unet_fill_rects_mask / unet_blur_separable against the fp64 restatement
(tests/pixel_ref.py), today's transforms bit for bit against per-image application, the batched pipeline against sequential application
of the same draws, per-image Compose calls, both loaders, and a short fit."""
import math

import numpy as np
import pytest
import torch

from pixel_ref import program_ref, separable_ref
from unet_amd import augment as A
from unet_amd import ops
from warp_ref import tie_pixels, warp_mask_ref, warp_ref

pytestmark = pytest.mark.gpu

IMG_TOL = 1e-4          # the warp's (tests/test_augment_geometry_gpu.py)
PIX_TOL = 1e-5          # gamma and noise with sigma <= 0.2: |z| <= 5.8, a few fp32 ulp on log, sqrt, sincos, pow -> about 1e-6 on the output
BLUR_TOL = 1e-5         # at most 62 fp32 multiply-adds of values in [0, 1] with taps summing to 1


def _programs(g, n, C, H, W):
    """one program per image, cycling: every opcode mixed / exact ops only / none / noise alone / two rectangle ops and a second permutation"""
    def rects(k):
        out = []
        for _ in range(k):
            y0, x0 = int(g.integers(0, H)), int(g.integers(0, W))
            out.append((y0, x0, int(g.integers(y0 + 1, H + 1)), int(g.integers(x0 + 1, W + 1))))
        return out
    key = lambda: (int(g.integers(0, 2 ** 32)), int(g.integers(0, 2 ** 32)))
    perm = lambda: [int(c) for c in g.permutation(C)]
    drop = lambda: [int(c) for c in g.choice(C, size=int(g.integers(1, C)), replace=False)]
    progs, exact = {}, set()
    for j in range(n):
        kind = j % 5
        if kind == 0:
            progs[j] = [("bc", g.uniform(0.8, 1.2), g.uniform(-0.2, 0.2)), ("gamma", g.uniform(0.6, 1.5)), ("permute", perm()),
                        ("noise", *key(), g.uniform(-0.05, 0.05), g.uniform(0.0, 0.2), True), ("rects", rects(5), 0.25),
                        ("drop", drop(), 0.5), ("noise", *key(), 0.0, g.uniform(0.0, 0.2), False), ("bc", g.uniform(0.8, 1.2), 0.0)]
        elif kind == 1:
            progs[j] = [("bc", g.uniform(0.8, 1.2), g.uniform(-0.2, 0.2)), ("rects", rects(32), 0.0), ("drop", drop(), 0.75),
                        ("permute", perm()), ("bc", g.uniform(0.8, 1.2), 0.0)]
            exact.add(j)
        elif kind == 3:
            progs[j] = [("noise", *key(), 0.0, 0.2, True)]
        elif kind == 4:
            progs[j] = [("permute", perm()), ("rects", rects(3), 1.0), ("drop", drop(), 0.0), ("permute", perm()), ("rects", rects(2), 0.5)]
            exact.add(j)
    return progs, exact


@pytest.mark.parametrize("n,C,H,W", [(64, 4, 32, 32), (5, 3, 48, 80), (3, 5, 37, 53), (70, 2, 16, 24)])
def test_pointwise_programs_against_the_fp64_reference(n, C, H, W):
    g = np.random.default_rng(n * 100 + W)
    img = torch.from_numpy(g.random((n, C, H, W), dtype=np.float32))
    progs, exact = _programs(g, n, C, H, W)
    x = img.cuda()
    ops.pixel_ops(x, progs)
    got = x.cpu().numpy()
    worst = 0.0
    for j in range(n):
        if j not in progs:
            assert np.array_equal(got[j].view(np.int32), img[j].numpy().view(np.int32)), j           # no program: not touched
            continue
        want = program_ref(img[j].numpy(), progs[j])
        if j in exact:
            assert np.array_equal(got[j], want.astype(np.float32)), (j, np.abs(got[j] - want).max())
        else:
            worst = max(worst, float(np.abs(got[j] - want).max()))
    print(f"pixel_ops {(n, C, H, W)}: max |err| {worst:.3g}")
    assert worst <= PIX_TOL
    # the noise of an element does not depend on the launch: image by image gives the same bits as the whole batch
    for j in list(range(n))[:10]:
        if j in progs:
            one = img[j:j + 1].cuda()
            ops.pixel_ops(one, {0: progs[j]})
            assert torch.equal(one[0].view(torch.int32), x[j].view(torch.int32)), j


def test_long_programs_and_wide_images_split_into_launches():
    """more than 8 ops, more than 32 rectangles, and more channels than a thread holds at once"""
    g = np.random.default_rng(5)
    img = torch.from_numpy(g.random((3, 20, 12, 16), dtype=np.float32))
    rects = [(int(y), int(x), int(y) + 1, int(x) + 2) for y, x in zip(g.integers(0, 12, 40), g.integers(0, 15, 40))]
    long = [("bc", 1.0 + 0.01 * k, 0.01 * (k % 3)) for k in range(11)] + [("rects", rects, 0.5), ("drop", [19, 0, 7], 0.125)]
    progs = {0: long, 2: [("gamma", 0.9), ("noise", 3, 4, 0.0, 0.1, True), ("rects", rects[:3], 0.0)]}
    x = img.cuda()
    ops.pixel_ops(x, progs)
    got = x.cpu().numpy()
    assert np.array_equal(got[0], program_ref(img[0].numpy(), long).astype(np.float32))
    assert np.array_equal(got[1], img[1].numpy())
    assert np.abs(got[2] - program_ref(img[2].numpy(), progs[2])).max() <= PIX_TOL
    with pytest.raises(ValueError, match="at most 16 channels"):
        ops.pixel_ops(x, {0: [("permute", list(range(20)))]})


@pytest.mark.parametrize("dtype", [torch.int64, torch.float32])
def test_mask_rectangles(dtype):
    g = np.random.default_rng(6)
    n, H, W = 11, 19, 23
    mask = torch.from_numpy(g.integers(0, 5, (n, H, W))).to(dtype)
    rects = {}
    for j in (0, 3, 4, 10):
        k = 40 if j == 3 else int(g.integers(1, 6))
        y0, x0 = g.integers(0, H, k), g.integers(0, W, k)
        rects[j] = [(int(a), int(b), int(g.integers(a + 1, H + 1)), int(g.integers(b + 1, min(W, b + 4) + 1))) for a, b in zip(y0, x0)]
    m = mask.cuda()
    ops.fill_rects_mask(m, rects, 7)
    want = mask.clone()
    for j, rs in rects.items():
        for y0, x0, y1, x1 in rs:
            want[j, y0:y1, x0:x1] = 7
    assert torch.equal(m.cpu(), want)


BLUR_CASES = [((6, 4, 37, 53), (1, 3, 5, 7, 9, 31)), ((4, 2, 8, 8), (31,)), ((2, 3, 1, 9), (3, 31)), ((2, 3, 9, 1), (5, 31)),
              ((70, 1, 16, 24), (1, 3, 5, 7, 9, 31))]


@pytest.mark.parametrize("shape,ks", BLUR_CASES)
def test_blur_against_the_fp64_reference(shape, ks):
    g = np.random.default_rng(shape[0] * 10 + shape[3])
    n = shape[0]
    img = torch.from_numpy(g.random(shape, dtype=np.float32))
    img[0] = 0.625                                                      # a constant image stays constant
    taps = []
    for j in range(n):
        k = ks[j % len(ks)]
        taps.append(A.gaussian_taps(k, 0.0 if j % 4 < 2 else float(g.uniform(0.3, 6.0))) if j % 2 == 0 else A.Blur().taps(k))
    src = img.cuda()
    dst = torch.full_like(src, -1.0)
    ops.blur_separable(src, dst, taps)
    got = dst.cpu().numpy()
    assert torch.equal(src.cpu().view(torch.int32), img.view(torch.int32))               # the source is untouched
    worst = 0.0
    for j in range(n):
        if len(taps[j]) == 1:
            assert np.array_equal(got[j].view(np.int32), img[j].numpy().view(np.int32)), j           # k = 1: a copy, bit for bit
        worst = max(worst, float(np.abs(got[j] - separable_ref(img[j].numpy(), taps[j])).max()))
    print(f"blur {shape}: max |err| {worst:.3g}, constant image off by {np.abs(got[0] - 0.625).max():.3g}")
    assert worst <= BLUR_TOL
    assert np.abs(got[0] - 0.625).max() <= 1e-6


@pytest.mark.parametrize("mask_dtype", [torch.int64, torch.float32])
def test_existing_transforms_are_unchanged(mask_dtype):
    """today's pipelines through the batched launches equal per-image Compose calls (the former path of BatchAugment) bit for bit"""
    pipe = lambda: A.Compose([A.HorizontalFlip(p=0.5), A.RandomBrightnessContrast(p=0.7), A.CoarseDropout(mask_fill_value=7, p=0.7),
                              A.RandomBrightnessContrast(brightness_by_max=False, p=0.7)])
    B, H, W = 12, 64, 64
    g = torch.Generator().manual_seed(8)
    x = torch.rand(B, 4, H, W, generator=g)
    y = torch.randint(0, 5, (B, H, W), generator=g).to(mask_dtype)
    ba = A.BatchAugment(pipe(), n_transform_imgs=0.5, seed=17)
    assert ba.plan() == [("warp", [0]), ("pixel", [1, 2]), ("image", 3)]
    xa, ya = ba(x.cuda(), y.cuda())
    xs, ys = x.cuda(), y.cuda()
    ref, rng = pipe(), np.random.default_rng(17)
    for i in range(B // 2):
        xi, yi = ref(xs[i], ys[i], rng)
        xs[i], ys[i] = xi, yi
    assert torch.equal(xa.view(torch.int32), xs.view(torch.int32)) and torch.equal(ya, ys)
    assert not torch.equal(xa[:6].cpu(), x[:6]) and (ya.cpu() == 7).any() and torch.equal(xa[6:].cpu(), x[6:])
    assert ba.g.random() == rng.random()


PIPE = lambda: A.Compose([A.HorizontalFlip(p=0.5), A.RandomBrightnessContrast(p=0.6), A.GaussNoise(p=0.7), A.Rotate(limit=45, p=0.6),
                          A.GaussianBlur(blur_limit=(3, 9), sigma_limit=(0.0, 2.0), p=0.6), A.RandomGamma(p=0.6), A.CoarseDropout(p=0.6),
                          A.ChannelDropout(p=0.5)])


def _sequential(pipe, fired, x, y):
    """image by image, transform by transform, through warp_ref / pixel_ref on the CPU in fp64; tracks nearest-neighbour ties of the mask"""
    B, C, H, W = x.shape
    xs, ys, ts = [], [], []
    for i in range(B):
        xi, yi = x[i].double().numpy(), y[i].numpy()
        tie = np.zeros((H, W), bool)
        for k, t in enumerate(pipe.transforms):
            if (i, k) not in fired:
                continue
            prm = fired[i, k]
            if isinstance(t, A._Geometric):
                inv = A.inverse_map(t.matrix(prm, H, W))[None]
                interp, border, fill, mfill = t.modes()
                xi = warp_ref(xi[None], inv, interp, border, fill)[0]
                yi = warp_mask_ref(yi[None], inv, border, mfill)[0]
                tie = warp_mask_ref(tie[None], inv, border, False)[0] | tie_pixels(inv, H, W)[0]
            elif isinstance(t, A._Blur):
                xi = separable_ref(xi, t.taps(prm))
            else:
                xi = program_ref(xi, t.program(prm, C, H, W))
        xs.append(xi), ys.append(yi), ts.append(tie)
    return np.stack(xs), np.stack(ys), np.stack(ts)


def test_pipeline_equals_sequential_application():
    B, H, W = 12, 64, 64
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 4, H, W, generator=g)
    y = torch.randint(0, 5, (B, H, W), generator=g)
    ba = A.BatchAugment(PIPE(), n_transform_imgs=0.5, seed=23)
    assert ba.plan() == [("warp", [0]), ("pixel", [1, 2]), ("warp", [3]), ("blur", 4), ("pixel", [5, 6, 7])]
    fired = A.BatchAugment(PIPE(), n_transform_imgs=0.5, seed=23).draw(B, H, W, 4)
    assert {k for _, k in fired} == set(range(8))                    # every transform fired somewhere
    xd, yd = x.cuda(), y.cuda()
    xa, ya = ba(xd, yd)
    assert xa is xd and ya is yd
    want_x, want_y, ties = _sequential(ba.aug, fired, x, y)
    got_x, got_y = xa.cpu(), ya.cpu()
    err = np.abs(got_x.numpy() - want_x).max()
    print(f"pipeline: max |err| {err:.3g}")
    assert err <= IMG_TOL
    assert ties.mean() <= 0.01 and not ((got_y.numpy() != want_y) & ~ties).any()
    assert torch.equal(got_x[6:].view(torch.int32), x[6:].view(torch.int32)) and torch.equal(got_y[6:], y[6:])     # outside the slice
    xb, yb = A.BatchAugment(PIPE(), n_transform_imgs=0.5, seed=23)(x.cuda(), y.cuda())
    assert torch.equal(xb.view(torch.int32), xa.view(torch.int32)) and torch.equal(yb, ya)


def test_per_image_compose_runs_on_the_device():
    """a Compose called per image (albumentations style) runs each new transform on a single device image, as the batch kernels would"""
    x = torch.rand(4, 24, 40).cuda()
    y = torch.randint(0, 4, (24, 40)).cuda()
    for t in (A.RandomGamma(p=1.0), A.GaussNoise(p=1.0), A.GaussNoise(per_channel=False, p=1.0), A.GaussianBlur(p=1.0), A.Blur(p=1.0),
              A.ChannelDropout(p=1.0), A.ChannelShuffle(p=1.0)):
        g, h = np.random.default_rng(3), np.random.default_rng(3)
        xo, yo = A.Compose([t])(x, y, g)
        assert h.random() < 1.0 and h.random() < 1.0                  # Compose's and the transform's own p
        prm = t.draw_params(h, 4, 24, 40)
        assert xo.is_cuda and xo.shape == x.shape and yo is y and xo.data_ptr() != x.data_ptr()
        want = separable_ref(x.cpu().numpy(), t.taps(prm)) if isinstance(t, A._Blur) else program_ref(x.cpu().numpy(), t.program(prm, 4, 24, 40))
        assert np.abs(xo.cpu().numpy() - want).max() <= PIX_TOL, type(t).__name__
        host, _ = t.apply_params(x.cpu(), y.cpu(), prm)               # the host restatement says the same
        assert np.abs(host.numpy() - want).max() <= PIX_TOL, type(t).__name__


def _tiles(n, n_in, size, seed, n_cls=4):
    g = np.random.default_rng(seed)
    return ([g.integers(0, 256, (n_in, *size)).astype(np.uint8) for _ in range(n)],
            [g.integers(0, n_cls, size).astype(np.uint8) for _ in range(n)])


def test_pixel_pipeline_through_either_feed():
    from unet_amd.learner import DataLoader, TileDataset
    imgs, masks = _tiles(7, 4, (48, 48), 4)
    ds = TileDataset(imgs, masks, "int8")
    tfm = lambda: A.BatchAugment(A.Compose([A.GaussNoise(p=0.8), A.GaussianBlur(p=0.8), A.ChannelShuffle(p=0.8)]), n_transform_imgs=0.5, seed=13)
    assert not hasattr(tfm(), "flip_flags")
    host = DataLoader(ds, 3, True, "cuda", seed=5, batch_tfm=tfm(), feed="host")
    dev = DataLoader(ds, 3, True, "cuda", seed=5, batch_tfm=tfm(), feed="device")
    got = list(dev)
    for (xa, ya), (xb, yb) in zip(list(host), got):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
    raw = torch.from_numpy(np.stack(imgs).astype(np.float32) / 255.0)
    assert any(not any(torch.equal(xb[0].cpu(), r) for r in raw) for xb, _ in got)          # something was augmented


def test_three_steps_of_fit_with_the_pixel_pipeline(tmp_path):
    from unet_amd.learner import CrossEntropyLossFlat, DataLoaders, Learner, TileDataset
    from unet_amd.model import HipDynamicUnet
    imgs, masks = _tiles(6, 4, (64, 64), 6, n_cls=3)
    pi, pm = [], []
    for i, (a, m) in enumerate(zip(imgs, masks)):
        np.save(tmp_path / f"i{i}.npy", a)
        np.save(tmp_path / f"m{i}.npy", m)
        pi.append(tmp_path / f"i{i}.npy")
        pm.append(tmp_path / f"m{i}.npy")
    pipe = lambda: A.Compose([A.HorizontalFlip(p=0.5), A.RandomBrightnessContrast(p=0.5), A.GaussNoise(p=0.5), A.GaussianBlur(p=0.5), A.Blur(p=0.3),
                              A.RandomGamma(p=0.5), A.CoarseDropout(p=0.5), A.ChannelDropout(p=0.5), A.ChannelShuffle(p=0.5)])
    res = []
    for _ in range(2):
        torch.manual_seed(3)
        model = HipDynamicUnet("xresnet18", 4, 3, (64, 64))
        dls = DataLoaders(TileDataset(pi, pm, "int8"), TileDataset(pi[:2], pm[:2], "int8"), 2, vocab=list("abc"), seed=7,
                          train_tfm=A.BatchAugment(pipe(), n_transform_imgs=0.5, seed=2))
        learn = Learner(dls, model, loss_func=CrossEntropyLossFlat(axis=1), path=tmp_path)
        learn._no_logging = True
        learn.fit_one_cycle(1, lr_max=1e-3)
        torch.cuda.synchronize()
        res.append((list(learn.recorder.losses), model.flat_param.detach().clone()))
    (la, pa), (lb, pb) = res
    assert len(la) == 3 and all(math.isfinite(v) for v in la) and la == lb
    assert torch.equal(pa, pb)
