"""The geometric augmentations on the device: unet_warp_affine / unet_warp_affine_mask against the fp64 restatement (tests/warp_ref.py),
exact D4 permutations, the batched pipeline against per-image sequential application of the same draws, both loaders, and a short fit."""
import math

import numpy as np
import pytest
import torch

from unet_amd import augment as A
from unet_amd import ops
from warp_ref import tie_pixels, warp_mask_ref, warp_ref

pytestmark = pytest.mark.gpu

IMG_TOL = 1e-4


def _maps(g, n, H, W):
    """random inverse maps: angles in +-180 degrees, scales 0.05-2, shifts up to +-3 W / H"""
    out = np.empty((n, 6), np.float32)
    for j in range(n):
        m = A.rotation_matrix(g.uniform(-180, 180), math.exp(g.uniform(math.log(0.05), math.log(2.0))), H, W)
        m[0, 2] += g.uniform(-3, 3) * W
        m[1, 2] += g.uniform(-3, 3) * H
        out[j] = A.inverse_map(m)
    return out


def _check_masks(got: np.ndarray, want: np.ndarray, ties: np.ndarray, what: str):
    assert ties.mean() <= 0.01, (what, ties.mean())
    bad = (got != want) & ~ties
    assert not bad.any(), (what, int(bad.sum()))


@pytest.mark.parametrize("n,H,W", [(64, 32, 32), (5, 48, 80), (3, 512, 512)])
def test_warp_kernels_against_the_fp64_reference(n, H, W):
    g = np.random.default_rng(n * 1000 + H)
    img = torch.from_numpy(g.random((n, 4, H, W), dtype=np.float32))
    cls = torch.from_numpy(g.integers(0, 7, (n, H, W)))
    reg = torch.from_numpy(g.normal(size=(n, H, W)).astype(np.float32))
    maps = _maps(g, n, H, W)
    ties = tie_pixels(maps, H, W)
    xd, cd, rd = img.cuda(), cls.cuda(), reg.cuda()
    for border in (0, 1, 2, 4):
        fill, mfill = (0.375, 5) if border == 0 else (0.0, 0)
        for interp in (0, 1):
            out = torch.empty_like(xd)
            ops.warp_affine(xd, out, maps, interp, border, fill)
            want = warp_ref(img.numpy(), maps, interp, border, fill)
            err = np.abs(out.cpu().numpy() - want).max()
            assert err <= IMG_TOL, (border, interp, err)
        co, ro = torch.empty_like(cd), torch.empty_like(rd)
        ops.warp_affine_mask(cd, co, maps, border, mfill)
        ops.warp_affine_mask(rd, ro, maps, border, mfill)
        _check_masks(co.cpu().numpy(), warp_mask_ref(cls.numpy(), maps, border, mfill), ties, f"int64 border {border}")
        _check_masks(ro.cpu().numpy(), warp_mask_ref(reg.numpy(), maps, border, mfill), ties, f"fp32 border {border}")
    assert torch.equal(xd.cpu(), img) and torch.equal(cd.cpu(), cls)                     # out of place: the sources are untouched


def test_d4_maps_and_right_angles_are_exact():
    N = 96
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, 4, N, N, generator=g).cuda()
    x[0, 0, :3, :3] = torch.tensor([-0.0, float("inf"), 1e-40])                         # any value is copied bit for bit
    y = torch.randint(-5, 9, (6, N, N), generator=g).cuda()
    yf = torch.randn(6, N, N, generator=g).cuda()
    rr, tr, hf, vf = A.RandomRotate90(), A.Transpose(), A.HorizontalFlip(), A.VerticalFlip()
    d4 = [(rr.matrix(k, N, N), lambda a, k=k: torch.rot90(a, k, (-2, -1))) for k in range(4)]
    d4 += [(tr.matrix(None, N, N), lambda a: a.transpose(-1, -2)), (hf.matrix(None, N, N), lambda a: a.flip(-1)),
           (vf.matrix(None, N, N), lambda a: a.flip(-2)), (tr.matrix(None, N, N) @ rr.matrix(2, N, N), lambda a: torch.rot90(a, 2, (-2, -1)).transpose(-1, -2))]
    for fwd, f in d4:
        maps = np.stack([A.inverse_map(fwd)] * 6)
        for interp in (0, 1):
            for border in (0, 1, 2, 4):
                out = torch.empty_like(x)
                ops.warp_affine(x, out, maps, interp, border, 0.5)
                assert torch.equal(out.view(torch.int32), f(x).contiguous().view(torch.int32)), (interp, border)
        for m in (y, yf):
            mo = torch.empty_like(m)
            ops.warp_affine_mask(m, mo, maps, 4, 0)
            assert torch.equal(mo, f(m))
    # Rotate at +-90 / 180 degrees is RandomRotate90, and the identity copies
    for angle, k in ((90, 1), (-90, 3), (180, 2), (-180, 2)):
        a = torch.empty_like(x)
        b = torch.empty_like(x)
        ops.warp_affine(x, a, np.stack([A.inverse_map(A.Rotate().matrix(float(angle), N, N))] * 6), 1, 4, 0.0)
        ops.warp_affine(x, b, np.stack([A.inverse_map(rr.matrix(k, N, N))] * 6), 0, 4, 0.0)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    xr = torch.randn(3, 4, 40, 72, generator=g).cuda()
    ident = np.stack([A.inverse_map(np.eye(3))] * 3)
    for interp in (0, 1):
        out = torch.empty_like(xr)
        ops.warp_affine(xr, out, ident, interp, 0, 0.0)
        assert torch.equal(out.view(torch.int32), xr.view(torch.int32))


def test_more_than_64_images_run_in_chunks():
    g = np.random.default_rng(9)
    n, H, W = 70, 16, 24
    img = torch.from_numpy(g.random((n, 2, H, W), dtype=np.float32))
    maps = _maps(g, n, H, W)
    out = torch.empty_like(img.cuda())
    ops.warp_affine(img.cuda(), out, maps, 1, 2, 0.0)
    assert np.abs(out.cpu().numpy() - warp_ref(img.numpy(), maps, 1, 2)).max() <= IMG_TOL


PIPE = lambda: A.Compose([A.HorizontalFlip(p=0.5), A.VerticalFlip(p=0.5), A.RandomRotate90(p=0.5),
                          A.ShiftScaleRotate(shift_limit=0.2, scale_limit=0.3, rotate_limit=60, border_mode=0, value=0.25, mask_value=9, p=0.7),
                          A.RandomBrightnessContrast(p=0.5), A.Rotate(limit=45, border_mode=2, p=0.6)])


def _sequential(pipe, fired, x: torch.Tensor, y: torch.Tensor):
    """image by image, transform by transform, through warp_ref (geometric) or the transform itself (others), on the CPU in fp64;
    also tracks which mask pixels descend from a nearest-neighbour rounding tie"""
    B, _, H, W = x.shape
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
    ba = A.BatchAugment(PIPE(), n_transform_imgs=0.5, seed=21)
    fired = A.BatchAugment(PIPE(), n_transform_imgs=0.5, seed=21).draw(B, H, W)
    assert any(k == 3 for _, k in fired) and any(k == 5 for _, k in fired) and any(k == 2 for _, k in fired)
    xd, yd = x.cuda(), y.cuda()
    xa, ya = ba(xd, yd)
    assert xa is xd and ya is yd                                     # in place, as the flip path
    want_x, want_y, ties = _sequential(ba.aug, fired, x, y)
    got_x, got_y = xa.cpu(), ya.cpu()
    assert np.abs(got_x.numpy() - want_x).max() <= IMG_TOL
    _check_masks(got_y.numpy(), want_y, ties, "pipeline")
    assert torch.equal(got_x[6:].view(torch.int32), x[6:].view(torch.int32)) and torch.equal(got_y[6:], y[6:])     # outside the slice
    # the same seed twice: identical batches
    xb, yb = A.BatchAugment(PIPE(), n_transform_imgs=0.5, seed=21)(x.cuda(), y.cuda())
    assert torch.equal(xb.view(torch.int32), xa.view(torch.int32)) and torch.equal(yb, ya)


def test_per_image_compose_runs_on_the_device():
    """a Compose called per image (albumentations style) warps single device images"""
    g = np.random.default_rng(2)
    x = torch.rand(3, 40, 40).cuda()
    y = torch.randint(0, 4, (40, 40)).cuda()
    pipe = A.Compose([A.Rotate(limit=(90, 90), p=1.0), A.Transpose(p=1.0)])
    xo, yo = pipe(x, y, g)
    assert torch.equal(xo, torch.rot90(x, 1, (-2, -1)).transpose(-1, -2)) and torch.equal(yo, torch.rot90(y, 1).T)


def _tiles(n, n_in, size, seed, n_cls=4):
    g = np.random.default_rng(seed)
    return ([g.integers(0, 256, (n_in, *size)).astype(np.uint8) for _ in range(n)],
            [g.integers(0, n_cls, size).astype(np.uint8) for _ in range(n)])


def test_rotate_pipeline_through_either_feed():
    """the device feed and feed="host" hand the step identical batches for a rotate pipeline (same draws, same kernels)"""
    from unet_amd.learner import DataLoader, TileDataset
    imgs, masks = _tiles(7, 4, (48, 48), 4)
    for regression in (False, True):
        mk = [m.astype(np.float32) * 0.5 for m in masks] if regression else masks
        ds = TileDataset(imgs, mk, "int8", regression=regression)
        tfm = lambda: A.BatchAugment(PIPE(), n_transform_imgs=0.5, seed=13)
        assert not hasattr(tfm(), "flip_flags")
        host = DataLoader(ds, 3, True, "cuda", seed=5, batch_tfm=tfm(), feed="host")
        dev = DataLoader(ds, 3, True, "cuda", seed=5, batch_tfm=tfm(), feed="device")
        got = list(dev)
        for (xa, ya), (xb, yb) in zip(list(host), got):
            assert torch.equal(xa, xb) and torch.equal(ya, yb)
        raw = torch.from_numpy(np.stack(imgs).astype(np.float32) / 255.0)
        assert any(not any(torch.equal(xb[0].cpu(), r) for r in raw) for xb, _ in got)      # something was rotated


def test_three_steps_of_fit_with_a_rotate_pipeline(tmp_path):
    """fit_one_cycle over tile files with flips + RandomRotate90 + ShiftScaleRotate: finite losses, and two seeded runs end with identical
    parameters (the warps are deterministic)"""
    from unet_amd.learner import CrossEntropyLossFlat, DataLoaders, Learner, TileDataset
    from unet_amd.model import HipDynamicUnet
    imgs, masks = _tiles(6, 4, (64, 64), 6, n_cls=3)
    pi, pm = [], []
    for i, (a, m) in enumerate(zip(imgs, masks)):
        np.save(tmp_path / f"i{i}.npy", a)
        np.save(tmp_path / f"m{i}.npy", m)
        pi.append(tmp_path / f"i{i}.npy")
        pm.append(tmp_path / f"m{i}.npy")
    pipe = lambda: A.Compose([A.HorizontalFlip(p=0.5), A.VerticalFlip(p=0.5), A.RandomRotate90(p=0.5), A.ShiftScaleRotate(p=0.5)])
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
