"""Test-time augmentation on the device (unet_window_gather_oriented, unet_nchw_to_nhwc_oriented, unet_tta_accumulate) and through
predict_raster, save_predictions and the Learner:

  1. kernel units against the plain gather / staging / softmax and the torch code table (tests/tta_ref.py);
  2. tta=(0,) is today's path bit for bit;
  3. predict_raster(tta="d4") equals the host loop window -> g -> predict_probs -> g^-1 -> sum in code order -> / k -> merge, bit for bit;
  4. the fp32 "flips" / "d4" mosaics against the CPU oracle (fp64 arbiter for mask ties);
  5. save_predictions(merge=True, tta="d4") over split_raster's tiles equals predict_raster(tta="d4");
  6. two ranks equal one rank with tta="d4";
  7. Learner.get_preds / predict / tta against their compositions.
"""
import copy
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import tta_ref as R

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as O  # noqa: E402  (checker)


def _pair(arch, n_in, n_out, size, seed, act_dtype="f32", head_target=4.0):
    """(HIP model, oracle) with identical weights, eval mode, logits normalised to O(1)"""
    from unet_amd.model import HipDynamicUnet
    torch.manual_seed(seed)
    ref = O.DynamicUnet(arch, n_in, n_out, (size, size))
    ref.eval()
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randint(0, 256, (1, n_in, size, size), generator=g).float() / 255
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.05, generator=g)
                m.running_var.uniform_(0.7, 1.3, generator=g)
                m.weight.add_(torch.randn(m.weight.shape, generator=g) * 0.1)
        s = ref(x).abs().max().item() / head_target
        head = ref.layers[-1][0]
        head.weight.div_(s)
        head.bias.div_(s)
    model = HipDynamicUnet(arch, n_in, n_out, (size, size), act_dtype=act_dtype)
    r = model.load_state_dict(ref.state_dict())
    assert not r.missing_keys and not r.unexpected_keys
    model.eval()
    return model, ref


def _raster(seed, C, H, W, dtype=np.uint8, hi=256):
    return np.random.default_rng(seed).integers(1, hi, (C, H, W)).astype(dtype)


def _nhwc_orient(t, code):
    """g applied to the spatial axes of an NHWC tensor [n, h, w, c]"""
    return R.g(t.permute(0, 3, 1, 2), code).permute(0, 2, 3, 1)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ 1. kernel units

@pytest.mark.parametrize("rtype", ["u8", "u16", "i16"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_oriented_gather_equals_g_of_the_gather(rtype, dt):
    from unet_amd import ops
    npt = {"u8": np.uint8, "u16": np.uint16, "i16": np.int16}[rtype]
    hi = {"u8": 256, "u16": 65535, "i16": 32767}[rtype]
    img = _raster(3, 3, 70, 90, npt, hi)
    import predict as P
    data = P.torch_samples(img).cuda()
    cs, co = (16, 5) if dt == torch.bfloat16 else (8, 3)          # a strided slice: lanes outside it stay untouched
    for div2 in (False, True):
        src = ops.WindowSource(data, div255_twice=div2)
        for th, tw in ((24, 24), (16, 24)):
            wins = [(0, 0), (70 - th, 90 - tw), (13, 41), (46, 5)]
            tab = ops.window_table(wins, "cuda")
            plain = torch.full((4, th, tw, cs), 7.0, device="cuda").to(dt)
            ops.window_gather(src, tab, 0, 4, th, tw, plain, co)
            for code in range(8):
                out = torch.full((4, th, tw, cs), 7.0, device="cuda").to(dt)
                if code >= 4 and th != tw:
                    with pytest.raises(ops.L.UnetHipError):
                        ops.window_gather_oriented(src, tab, 0, 4, th, tw, out, co, code)
                    continue
                ops.window_gather_oriented(src, tab, 0, 4, th, tw, out, co, code)
                want = plain.clone()
                want[..., co:co + 3] = _nhwc_orient(plain[..., co:co + 3], code)
                assert torch.equal(_bits(out), _bits(want)), (rtype, dt, div2, th, tw, code)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_oriented_staging_equals_g_of_the_batch(dt):
    from unet_amd import ops
    x = torch.rand((3, 4, 20, 20), device="cuda")
    for code in range(8):
        out = torch.full((3, 20, 20, 16), -3.0, device="cuda").to(dt)
        ops.nchw_to_nhwc_oriented(x, out, 9, code)
        want = torch.full((3, 20, 20, 16), -3.0, device="cuda").to(dt)
        want[..., 9:13] = R.g(x, code).permute(0, 2, 3, 1).to(dt)
        assert torch.equal(_bits(out), _bits(want)), code
    xr = torch.rand((2, 4, 12, 20), device="cuda")
    out = torch.zeros((2, 12, 20, 8), device="cuda")
    ops.nchw_to_nhwc_oriented(xr, out, 0, 3)
    assert torch.equal(out[..., :4], R.g(xr, 3).permute(0, 2, 3, 1))
    with pytest.raises(ops.L.UnetHipError):
        ops.nchw_to_nhwc_oriented(xr, out, 0, 5)


def test_gather_then_inverse_accumulate_gives_the_input_back():
    from unet_amd import ops
    img = _raster(4, 4, 64, 64)
    src = ops.WindowSource(torch.from_numpy(img).cuda())
    tab = ops.window_table([(0, 0), (10, 30), (32, 32)], "cuda")
    plain = torch.zeros((3, 32, 32, 4), device="cuda")
    ops.window_gather(src, tab, 0, 3, 32, 32, plain, 0)
    for code in range(8):
        x = torch.zeros((3, 32, 32, 4), device="cuda")
        ops.window_gather_oriented(src, tab, 0, 3, 32, 32, x, 0, code)
        acc = torch.full((3, 32, 32, 8), 5.0, device="cuda")
        ops.tta_accumulate(ops.TS(x, 0, 4), 3, code, True, True, acc, 1)
        assert torch.equal(acc[..., :4], plain), code
        assert bool((acc[..., 4:] == 5.0).all()), code          # lanes above C untouched
    with pytest.raises(ops.L.UnetHipError):
        ops.tta_accumulate(ops.TS(torch.zeros((1, 8, 16, 4), device="cuda"), 0, 3), 1, 4, False, True,
                           torch.zeros((1, 8, 16, 4), device="cuda"))


def test_accumulate_equals_softmax_mapped_back_summed_in_order():
    from unet_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    n, S, C = 2, 24, 5
    codes = (1, 5, 7, 0)
    zs = {c: torch.randn((n, S, S, 8), device="cuda", generator=g) * 3 for c in codes}
    acc = torch.empty((n, S, S, 8), device="cuda")
    probs = torch.empty((n, C, S, S), device="cuda")
    amax = torch.empty((n, S, S), dtype=torch.int64, device="cuda")
    for i, c in enumerate(codes):
        last = i == len(codes) - 1
        ops.tta_accumulate(ops.TS(zs[c], 0, C), n, c, False, i == 0, acc, len(codes) if last else 0, probs if last else None,
                           amax if last else None)
    s = torch.zeros((n, C, S, S), device="cuda")
    for c in codes:
        p = torch.empty((n, C, S, S), device="cuda")
        ops.softmax_argmax(ops.TS(zs[c], 0, C), p, None)          # the arithmetic of the per-tile path
        s = s + R.g_inv(p, c)
    s = s / len(codes)
    assert torch.equal(probs, s)
    assert torch.equal(acc[..., :C], s.permute(0, 2, 3, 1))
    assert torch.equal(amax, s.argmax(1))
    # regression: raw values
    accr = torch.empty((n, S, S, 8), device="cuda")
    vals = torch.empty((n, C, S, S), device="cuda")
    for i, c in enumerate(codes):
        last = i == len(codes) - 1
        ops.tta_accumulate(ops.TS(zs[c], 0, C), n, c, True, i == 0, accr, len(codes) if last else 0, vals if last else None)
    sr = torch.zeros((n, C, S, S), device="cuda")
    for c in codes:
        sr = sr + R.g_inv(zs[c][..., :C].permute(0, 3, 1, 2), c)
    assert torch.equal(vals, sr / len(codes))


# ------------------------------------------------------------------------------------------------------------------ helpers: rasters, tiles

def _scene(tmp_path, size, nodata=250):
    """the ragged ~700 px raster of tests/test_raster_gpu.py (i): an empty corner, a nodata streak"""
    from unet_amd.tiffio import write_tiff
    img = _raster(5, 4, 700, 620, hi=250)
    img[:, :250, :250] = 0
    img[1, 300:303, 100:400] = nodata
    rpath = tmp_path / "scene.tif"
    write_tiff(rpath, img, geotransform=(400000.0, 0.5, 0.0, 5700000.0, 0.0, -0.5), nodata=nodata)
    zimg = img.copy()
    zimg[:, (img == nodata).any(axis=0)] = 0
    from unet_amd.mosaic import sliding_windows
    wins = []
    for y, x in sliding_windows(700, 620, size, 0.2):
        crop = zimg[:, y:y + size, x:x + size]
        if np.sum(crop != 0) >= crop.size * (1 - 0.9):
            wins.append((int(y), int(x)))
    return rpath, zimg, wins


def _export(tmp_path, model, n_out, size, regression=False):
    from unet_amd.learner import CrossEntropyLossFlat, DataLoaders, Learner, MSELossFlat, TileDataset
    dls = DataLoaders(TileDataset([np.zeros((4, size, size), np.uint8)], None, "int8", regression=regression), None, 1, device="cuda",
                      vocab=None if regression else [str(i) for i in range(n_out)])
    learn = Learner(dls, model, loss_func=MSELossFlat(axis=1) if regression else CrossEntropyLossFlat(axis=1), path=tmp_path)
    pkl = tmp_path / ("r.pkl" if regression else "m.pkl")
    learn.export(pkl)
    return pkl


def _host_loop(model, zimg, wins, size, codes, C, regression=False):
    """window -> torch-oriented -> predict_probs / predict_values (batch-1 plans) -> g^-1 -> sum in code order -> / k -> the
    reference's sum / count -> argmax (predict.py:284-334) on the device kernels of the per-tile path"""
    from unet_amd import ops
    from unet_amd.learner import scale_input
    oy, ox = min(w[0] for w in wins), min(w[1] for w in wins)
    MH, MW = max(w[0] for w in wins) + size - oy, max(w[1] for w in wins) + size - ox
    mosaic = torch.zeros((C, MH, MW), dtype=torch.float32, device="cuda")
    count = torch.zeros((MH, MW), dtype=torch.int32, device="cuda")
    with ops.tuning(plan_batch=1):
        for y, x in wins:
            t = torch.from_numpy(scale_input(zimg[:, y:y + size, x:x + size], "int8"))[None].cuda()
            s = None
            for c in codes:
                tg = R.g(t, c).contiguous()
                p = model.predict_values(tg) if regression else model.predict_probs(tg)[0]
                p = R.g_inv(p, c)
                s = p.clone() if s is None else s + p
            s = (s / len(codes)).contiguous()
            ops.mosaic_accumulate(s[0], mosaic, count, y - oy, x - ox)
    am = torch.empty((MH, MW), dtype=torch.uint8, device="cuda")
    ops.mosaic_finalize(mosaic, count, am)
    return mosaic.cpu().numpy(), am.cpu().numpy(), count.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ 2. (0,) is today's path

def test_identity_set_is_todays_path(tmp_path):
    import create_tiles_unet as T
    import predict as P
    from unet_amd.tiffio import read_tiff
    size = 128
    model, _ = _pair("xresnet18", 4, 3, size, seed=23)
    img = _raster(9, 4, 300, 420)
    for kw in ({}, {"all_classes": True}, {"all_classes": True, "large_file": True}, {"specific_class": 1}):
        a = P.predict_raster(model, img, size, 0.2, batch_size=3, **kw)
        b = P.predict_raster(model, img, size, 0.2, batch_size=3, tta=(0,), **kw)
        assert a.dtype == b.dtype and np.array_equal(a, b), kw
    rmodel, _ = _pair("xresnet18", 4, 1, size, seed=24)
    a = P.predict_raster(rmodel, img, size, 0.2, batch_size=3, regression=True)
    b = P.predict_raster(rmodel, img, size, 0.2, batch_size=3, regression=True, tta=(0,))
    assert np.array_equal(a, b)
    from unet_amd.tiffio import write_tiff
    rpath = tmp_path / "s.tif"
    write_tiff(rpath, img, geotransform=(0.0, 1.0, 0.0, 0.0, 0.0, -1.0))
    T.split_raster(rpath, None, tmp_path / "cut", patch_size=size, patch_overlap=0.2, split=[1], max_empty=0.9)
    tiles = tmp_path / "cut" / "img_tiles"
    pkl = _export(tmp_path, model, 3, size)
    for kw in ({"merge": True}, {"merge": True, "all_classes": True, "large_file": True}):
        fa = P.save_predictions(pkl, tiles, False, AOI="a", validation_vision=False, batch_size=3, **kw)
        fb = P.save_predictions(pkl, tiles, False, AOI="b", validation_vision=False, batch_size=3, tta=(0,), **kw)
        assert np.array_equal(read_tiff(fa)[0], read_tiff(fb)[0]), kw
    for kw in ({}, {"all_classes": True}, {"specific_class": 2}):
        da = P.save_predictions(pkl, tiles, False, validation_vision=False, batch_size=3, **kw)
        ref = {p.name: read_tiff(p)[0] for p in sorted(da.iterdir())}
        db = P.save_predictions(pkl, tiles, False, validation_vision=False, batch_size=3, tta=(0,), **kw)
        got = {p.name: read_tiff(p)[0] for p in sorted(db.iterdir())}
        assert ref.keys() == got.keys() and all(np.array_equal(ref[k], got[k]) for k in ref), kw


# ------------------------------------------------------------------------------------------------------------------ 3. device == host loop

@pytest.mark.parametrize("case", ["f32", "bf16", "regression"])
def test_d4_device_path_equals_the_host_composition(tmp_path, case):
    import predict as P
    size = 256
    reg = case == "regression"
    C = 1 if reg else 3
    model, _ = _pair("xresnet18", 4, C, size, seed=11, act_dtype="bf16" if case == "bf16" else "f32")
    rpath, zimg, wins = _scene(tmp_path, size)
    codes = tuple(range(8))
    mosaic, am, cnt = _host_loop(model, zimg, wins, size, codes, C, regression=reg)
    kw = dict(max_empty=0.9, batch_size=5, batch_invariant=True, tta="d4")
    if reg:
        out = P.predict_raster(model, rpath, size, 0.2, regression=True, **kw)
        assert np.array_equal(out[cnt > 0], mosaic[0][cnt > 0]) and bool((out[cnt == 0] == -9999).all())
        return
    out = P.predict_raster(model, rpath, size, 0.2, **kw)
    allc = P.predict_raster(model, rpath, size, 0.2, all_classes=True, **kw)
    assert np.array_equal(allc, mosaic) and np.array_equal(out, am)
    plain = P.predict_raster(model, rpath, size, 0.2, all_classes=True, max_empty=0.9, batch_size=5, batch_invariant=True)
    assert not np.array_equal(plain, allc)                  # the passes do change the numbers


# ------------------------------------------------------------------------------------------------------------------ 4. against the oracle

def test_flips_and_d4_against_the_oracle(tmp_path):
    import predict as P
    from unet_amd.learner import scale_input
    size = 256
    model, ref = _pair("xresnet18", 4, 3, size, seed=11)
    rpath, zimg, wins = _scene(tmp_path, size)
    per = {}
    for y, x in wins:
        t = torch.from_numpy(scale_input(zimg[:, y:y + size, x:x + size], "int8"))[None]
        per[(y, x)] = R.passes(ref, t, tuple(range(8)))
    for name, codes in (("flips", (0, 1, 2, 3)), ("d4", tuple(range(8)))):
        out = P.predict_raster(model, rpath, size, 0.2, max_empty=0.9, batch_size=5, tta=name)
        allc = P.predict_raster(model, rpath, size, 0.2, max_empty=0.9, batch_size=5, tta=name, all_classes=True)
        acc, cnt = np.zeros((3, 700, 620), np.float32), np.zeros((700, 620), np.int32)
        for y, x in wins:
            acc[:, y:y + size, x:x + size] += R.compose(per[(y, x)], codes)[0].numpy()
            cnt[y:y + size, x:x + size] += 1
        acc[:, cnt > 0] /= cnt[cnt > 0]
        err = float(np.abs(acc - allc).max())
        assert err < 1e-4, (name, err)
        diff = (acc.argmax(0) != out) & (cnt > 0)
        if diff.any():                                      # the fp64 arbiter: only numerical ties may differ
            ref64 = copy.deepcopy(ref).double()
            acc64 = np.zeros((3, 700, 620), np.float64)
            for y, x in wins:
                t = torch.from_numpy(scale_input(zimg[:, y:y + size, x:x + size], "int8"))[None].double()
                acc64[:, y:y + size, x:x + size] += R.tta(ref64, t, codes)[0].numpy()
            acc64[:, cnt > 0] /= cnt[cnt > 0]
            top2 = np.sort(acc64, axis=0)[-2:]
            gap = (top2[1] - top2[0])[diff]
            print(f"{name}: {int(diff.sum())} mask pixel(s) differ; fp64 margins up to {gap.max():.2e}, probability err {err:.2e}")
            assert bool((gap <= 2 * err).all()), (name, gap.max())
        assert (out[cnt == 0] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ 5. files == raster

def test_save_predictions_d4_equals_predict_raster(tmp_path):
    import create_tiles_unet as T
    import predict as P
    from unet_amd.tiffio import read_tiff
    size = 256
    model, _ = _pair("xresnet18", 4, 3, size, seed=11)
    rpath, _, wins = _scene(tmp_path, size)
    pkl = _export(tmp_path, model, 3, size)
    tiles = tmp_path / "cut"
    T.split_raster(rpath, None, tiles, patch_size=size, patch_overlap=0.2, split=[1], max_empty=0.9)
    for kw in ({}, {"all_classes": True}, {"all_classes": True, "large_file": True}):
        direct = P.predict_raster(model, rpath, size, 0.2, max_empty=0.9, batch_size=5, tta="d4", **kw)
        f = P.save_predictions(pkl, tiles / "img_tiles", False, merge=True, AOI="tta", validation_vision=False, batch_size=5, tta="d4", **kw)
        assert np.array_equal(read_tiff(f)[0], direct), kw
    nonsq = tmp_path / "ns"
    nonsq.mkdir()
    np.save(nonsq / "t.npy", _raster(1, 4, 128, 192))
    with pytest.raises(ValueError, match='"flips"'):
        P.save_predictions(pkl, nonsq, False, validation_vision=False, tta="d4")


# ------------------------------------------------------------------------------------------------------------------ 6. two ranks

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tta_worker(rank, world, port, state, img_path, outdir, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      UNET_DIST_BACKEND="gloo", UNET_FORCE_DEVICE="0")
    import torch.distributed as dist
    import predict as P
    from unet_amd.model import HipDynamicUnet
    model = HipDynamicUnet("xresnet18", 4, 3, (256, 256), device="cuda:0")
    model.load_state_dict(torch.load(state))
    model.eval()
    img = np.load(img_path)
    tm = {}
    a = P.predict_raster(model, img, 256, 0.2, batch_size=4, tta="d4", timing=tm)
    b = P.predict_raster(model, img, 256, 0.2, batch_size=4, all_classes=True, tta="d4")
    if rank == 0:
        np.save(os.path.join(outdir, "a.npy"), a)
        np.save(os.path.join(outdir, "b.npy"), b)
    else:
        assert a is None and b is None
    q.put((rank, tm["windows_this_rank"], tm["active_ranks"], tm["slab_floats_sent"]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_d4_equal_one_rank(tmp_path):
    import predict as P
    model, _ = _pair("xresnet18", 4, 3, 256, seed=31)
    img = _raster(9, 4, 750, 650)
    one = P.predict_raster(model, img, 256, 0.2, batch_size=4, tta="d4")
    one_all = P.predict_raster(model, img, 256, 0.2, batch_size=4, all_classes=True, tta="d4")
    state = tmp_path / "w.pt"
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, state)
    np.save(tmp_path / "img.npy", img)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tta_worker, args=(r, 2, port, str(state), str(tmp_path / "img.npy"), str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=900) for _ in procs)
    for p in procs:
        p.join(timeout=120)
    assert [r[2] for r in res] == [2, 2] and res[1][3] > 0, res          # both ranks active, slabs travelled
    assert np.array_equal(np.load(tmp_path / "a.npy"), one) and np.array_equal(np.load(tmp_path / "b.npy"), one_all)


# ------------------------------------------------------------------------------------------------------------------ 7. Learner

def _learner(tmp_path, size, n_valid=5, shape=None, seed=41):
    from unet_amd.learner import CrossEntropyLossFlat, DataLoaders, Learner, TileDataset
    h, w = shape or (size, size)
    model, _ = _pair("xresnet18", 4, 3, size, seed=seed)
    g = np.random.default_rng(seed)
    imgs = [g.integers(0, 256, (4, h, w)).astype(np.uint8) for _ in range(n_valid)]
    masks = [g.integers(0, 3, (h, w)).astype(np.uint8) for _ in range(n_valid)]
    dls = DataLoaders(TileDataset(imgs, masks, "int8"), TileDataset(imgs, masks, "int8"), 2, device="cuda", vocab=["a", "b", "c"])
    return Learner(dls, model, loss_func=CrossEntropyLossFlat(axis=1), path=tmp_path), imgs


def test_learner_get_preds_predict_and_tta(tmp_path):
    from unet_amd.learner import scale_input
    learn, imgs = _learner(tmp_path, 128)
    model = learn.model
    x = torch.from_numpy(np.stack([scale_input(a, "int8") for a in imgs])).cuda()
    for tta in ((0,), "flips", "d4", (6, 2)):
        codes = {"flips": (0, 1, 2, 3), "d4": tuple(range(8))}.get(tta, tta)
        want = None
        for i in range(0, len(imgs), 2):                    # the loader's batches of 2: same launch geometry
            xb = x[i:i + 2]
            s = None
            for c in codes:
                p = R.g_inv(model.predict_probs(R.g(xb, c).contiguous())[0], c)
                s = p.clone() if s is None else s + p
            s = (s / len(codes)).cpu()
            want = s if want is None else torch.cat([want, s])
        preds, targs, dec = learn.get_preds(tta=tta, with_decoded=True)
        assert torch.equal(preds, want), tta
        assert torch.equal(dec, want.argmax(1)), tta
    # predict: one tile, batch 1
    t = x[:1]
    s = None
    for c in range(8):
        p = R.g_inv(model.predict_probs(R.g(t, c).contiguous())[0], c)
        s = p.clone() if s is None else s + p
    s = (s / 8).cpu()
    dec, _, probs = learn.predict(imgs[0], tta="d4")
    assert torch.equal(probs, s[0]) and torch.equal(dec, s[0].argmax(0))

    # Learner.tta against fastai's formula from separate passes
    preds = learn.get_preds()[0]
    single = {c: learn.get_preds(tta=(c,))[0] for c in range(1, 5)}
    mean = (((single[1] + single[2]) + single[3]) + single[4]) / 4
    out, targs = learn.tta(n=4)
    assert torch.equal(targs, learn.get_preds()[1])
    assert torch.equal(learn.get_preds(tta=(1, 2, 3, 4))[0], mean)          # the device mean = the passes summed in code order, / 4
    assert torch.equal(out, torch.lerp(mean, preds, 0.25))
    (aug, p0), _ = learn.tta(n=4, beta=None)
    assert torch.equal(p0, preds) and torch.equal(aug, mean)
    mx, _ = learn.tta(n=3, use_max=True)
    assert torch.equal(mx, torch.maximum(preds, torch.maximum(torch.maximum(single[1], single[2]), single[3])))
    with pytest.raises(NotImplementedError):
        learn.tta(item_tfms=[object()])


def test_learner_tta_needs_square_tiles_beyond_flips(tmp_path):
    learn, _ = _learner(tmp_path, 128, n_valid=2, shape=(128, 192))
    out, _ = learn.tta(n=3)                                  # flips only: fine on 128 x 192
    assert out.shape == (2, 3, 128, 192)
    with pytest.raises(ValueError, match='"flips"'):
        learn.tta(n=4)
