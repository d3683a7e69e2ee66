"""DiceLoss (fastai losses.DiceLoss, params_and_main.py:16) on the device: the fused kernels (unet_dice_fwd / unet_dice_bwd / _bf16) against
the fp64 restatement of the spec (tests/dice_ref.py), the whole network against the oracle, the captured training step, the Learner
(fit, validate, export / load_learner, lr_find) and tile-DDP over two ranks on one GPU."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from dice_ref import dice_loss_ref
from util import empty_ts, outside_untouched, to_ts

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as O  # noqa: E402  (checker)


def _run(zt, y, smooth, square, mean_div, dz, gscale):
    from unet_amd import ops
    N, C = zt.N, zt.C
    loss = torch.zeros(1, device="cuda")
    coef = torch.zeros(2 * N * C, device="cuda")
    ws = torch.full((ops.dice_workspace(N, zt.H * zt.W, C),), float("nan"), device="cuda")
    ops.dice_fwd(zt, y, smooth, square, mean_div, loss, coef, ws)
    ops.dice_bwd(zt, y, square, coef, gscale, dz)
    torch.cuda.synchronize()
    return loss.clone(), coef.clone(), dz.buf.clone()


@pytest.mark.parametrize("C", [1, 2, 5, 12, 64])
@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("square_in_union", [False, True])
@pytest.mark.parametrize("smooth", [1e-6, 1.0])
def test_dice_kernels_against_the_spec(C, reduction, square_in_union, smooth):
    """loss and logit gradient on a channel slice of a wider buffer, ragged pixel count, targets -100 and C (all-zero one-hot rows),
    gscale 0.5; fp32 and direct-bf16 gradients; two runs bit-identical; nothing outside the gradient slice written"""
    from unet_amd import ops
    g = torch.Generator().manual_seed(C * 8 + 4 * (reduction == "mean") + 2 * square_in_union + (smooth == 1.0))
    N, H, W = 3, 37, 29
    z = torch.randn(N, C, H, W, generator=g) * 2.0
    y = torch.randint(0, C, (N, H, W), generator=g)
    y[0, 3, :5] = -100
    y[2, 10, 4:9] = C
    z64 = z.double().requires_grad_(True)
    ref_loss = dice_loss_ref(z64, y, smooth, reduction, square_in_union)
    ref_loss.backward()
    ref = 0.5 * z64.grad
    zt = to_ts(z, cs=ops.rup4(C) + 8, co=4)
    yd = y.cuda().contiguous()
    mean_div = N * C if reduction == "mean" else 0
    dz = empty_ts(N, H, W, C, cs=ops.rup4(C) + 4, co=4)
    loss, coef, buf = _run(zt, yd, smooth, square_in_union, mean_div, dz, 0.5)
    assert abs(loss.item() - ref_loss.item()) <= 2e-6 * abs(ref_loss.item()) + 1e-12, (loss.item(), ref_loss.item())
    got = dz.view().permute(0, 3, 1, 2).double().cpu()
    scale = ref.abs().max().item()
    assert (got - ref).abs().max().item() <= 2e-6 * scale + 1e-15, ((got - ref).abs().max().item(), scale)
    assert outside_untouched(dz)
    # bit-reproducible: no atomics, fixed-order sums
    dz2 = empty_ts(N, H, W, C, cs=ops.rup4(C) + 4, co=4)
    loss2, coef2, buf2 = _run(zt, yd, smooth, square_in_union, mean_div, dz2, 0.5)
    assert torch.equal(loss, loss2) and torch.equal(coef, coef2) and torch.equal(buf, buf2)
    # bf16 gradient slice written directly (logits stay fp32)
    dzb = ops.TS(torch.zeros((N, H, W, ops.rupv(C, torch.bfloat16) + 8), dtype=torch.bfloat16, device="cuda"), 8, C)
    ops.dice_bwd(zt, yd, square_in_union, coef, 0.5, dzb)
    gb = dzb.view().permute(0, 3, 1, 2).double().cpu()
    assert (gb - ref).abs().max().item() <= 2.0 ** -8 * scale + 1e-15
    outside = torch.ones(dzb.cs, dtype=torch.bool)
    outside[dzb.co:dzb.co + C] = False
    assert (dzb.buf[..., outside] == 0).all()


def _smooth_pair(arch, n_in, n_out, size, dtype):
    """oracle + HIP network with the same weights; a smooth network (large BN shifts, small convs: no ReLU flips) as in the focal test"""
    import torch.nn as nn
    from unet_amd.model import HipDynamicUnet
    torch.manual_seed(3)
    ref = O.DynamicUnet(arch, n_in, n_out, size)
    O.randomize_bn_and_zero_gammas(ref, seed=4)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.bias.fill_(8.0)
            elif isinstance(m, nn.Conv2d) and m.bias is not None:
                m.weight.mul_(0.01)
                m.bias.fill_(1.0)
    model = HipDynamicUnet(arch, n_in, n_out, size, act_dtype=dtype)
    model.load_state_dict(ref.state_dict())
    return ref, model


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("reduction", ["sum", "mean"])
def test_training_step_with_dice_loss(dtype, reduction):
    """forward + DiceLoss + backward of the whole network against the oracle network + the restated loss (tolerances of
    test_training_step_with_focal_loss)"""
    from unet_amd.learner import DiceLoss
    ref, model = _smooth_pair("xresnet18", 4, 3, (64, 64), dtype)
    x, y = O.synthetic_batch(2, 4, 64, 64, 3)
    ref.train(); model.train()
    loss_ref = dice_loss_ref(ref(x), y, 1e-6, reduction, False)
    loss_ref.backward()
    loss = model.forward_loss_backward(x.cuda(), y.cuda(), torch.tensor([0.5, 1.5, 1.0], device="cuda"), dice=DiceLoss(reduction=reduction))
    torch.cuda.synchronize()
    tol = 1e-4 if dtype == "f32" else 3e-2
    assert abs(loss.item() - loss_ref.item()) < tol * max(1.0, abs(loss_ref.item())), (loss.item(), loss_ref.item())
    g_hip = torch.cat([p.grad.flatten().cpu() for p in model.parameters()])
    g_ref = torch.cat([p.grad.flatten() for p in ref.parameters()])
    cos = torch.nn.functional.cosine_similarity(g_hip.double(), g_ref.double(), dim=0).item()
    assert cos > (1 - 1e-6 if dtype == "f32" else 0.99), cos
    if dtype == "f32":
        worst = max((p.grad.cpu() - q.grad).abs().max().item() / (q.grad.abs().max().item() + 1e-12)
                    for p, q in zip(model.parameters(), ref.parameters()) if q.grad.abs().max().item() > 1e-20)
        assert worst < 2e-3, worst


def test_hipgraph_step_with_dice_matches_eager():
    """TrainStep(use_graph=True) replays the Dice step: 6 steps agree with the eager launch stream (bars of
    test_hipgraph_step_and_predict_match_eager)"""
    from unet_amd.learner import DiceLoss
    from unet_amd.model import HipDynamicUnet
    from unet_amd.optimizer import FlatAdam
    from unet_amd.trainer import TrainStep
    torch.manual_seed(11)
    sd = O.DynamicUnet("xresnet18", 4, 5, (64, 64)).state_dict()
    xs = [O.synthetic_batch(2, 4, 64, 64, 5, seed=s) for s in range(6)]
    outs = []
    for use_graph in (False, True):
        model = HipDynamicUnet("xresnet18", 4, 5, (64, 64))
        model.load_state_dict(sd)
        model.train()
        opt = FlatAdam(model, [1e-4, 3e-4, 1e-3])
        step = TrainStep(model, opt, None, 1, use_graph=use_graph)
        step.dice = DiceLoss(smooth=0.5, reduction="mean", square_in_union=True)
        losses = []
        for i, (x, y) in enumerate(xs):
            opt.set_lr([1e-4 * (i + 1), 3e-4, 1e-3 / (i + 1)])
            opt.mom = 0.95 - 0.01 * i
            losses.append(step(x.cuda(), y.cuda()).clone())
        torch.cuda.synchronize()
        assert (step._graph is not None) == use_graph
        outs.append((torch.stack(losses).cpu(), model.flat_param.clone().cpu()))
    assert torch.isfinite(outs[0][0]).all()
    assert torch.allclose(outs[0][0], outs[1][0], rtol=1e-6, atol=1e-7), (outs[0][0], outs[1][0])
    assert (outs[0][1] - outs[1][1]).abs().max().item() < 1e-6


def test_learner_fits_validates_exports_with_dice_loss(tmp_path):
    """train.train_unet's sequence with loss_func=DiceLoss(): class weights assigned to .func.weight (train.py:211) and ignored, one epoch,
    valid_loss = the batch-size-weighted mean of the restated per-batch Dice losses of the oracle network (fastai AvgLoss), export /
    load_learner keep the loss and its arguments, lr_find runs through the fused step"""
    from unet_amd.learner import DataLoaders, DiceLoss, DiceMulti, Learner, TileDataset, load_learner
    from unet_amd.model import HipDynamicUnet
    g = np.random.default_rng(0)
    imgs = [g.integers(0, 255, (4, 64, 64)).astype(np.uint8) for _ in range(4)]
    masks = [g.integers(0, 3, (64, 64)).astype(np.uint8) for _ in range(4)]
    torch.manual_seed(1)
    model = HipDynamicUnet("xresnet18", 4, 3, (64, 64))
    dls = DataLoaders(TileDataset(imgs, masks, "int8"), TileDataset(imgs[:3], masks[:3], "int8"), 2, vocab=list("abc"))
    loss = DiceLoss(axis=1, smooth=0.1, reduction="sum", square_in_union=True)
    loss.func.weight = torch.tensor([0.2, 0.3, 0.5])
    learn = Learner(dls, model, loss_func=loss, metrics=[DiceMulti()], path=tmp_path)
    learn._no_logging = True
    learn.fit_one_cycle(1, lr_max=slice(1e-4, 1e-3))
    torch.cuda.synchronize()
    assert len(learn.recorder.losses) == 2 and all(np.isfinite(learn.recorder.losses))
    ref = O.DynamicUnet("xresnet18", 4, 3, (64, 64))
    ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    ref.eval()
    with torch.no_grad():
        xs = torch.from_numpy(np.stack(imgs[:3]).astype(np.float32) / 255.0)
        ys = torch.from_numpy(np.stack(masks[:3]).astype(np.int64))
        # validation batches of 2 + 1 tiles: sum of loss * bs / sum of bs
        b1 = dice_loss_ref(ref(xs[:2]), ys[:2], 0.1, "sum", True).item()
        b2 = dice_loss_ref(ref(xs[2:]), ys[2:], 0.1, "sum", True).item()
    want = (2 * b1 + 1 * b2) / 3
    got = learn.validate()[0]
    assert abs(got - want) < 1e-4 * max(1.0, abs(want)), (got, want)
    learn.export(tmp_path / "dice.pkl")
    back = load_learner(tmp_path / "dice.pkl")
    d = back.loss_func
    assert isinstance(d, DiceLoss) and (d.smooth, d.reduction, d.square_in_union) == (0.1, "sum", True)
    assert torch.equal(back.model.flat_param, model.flat_param)
    before = model.flat_param.clone()
    learn.lr_find(start_lr=1e-6, end_lr=1e-3, num_it=6)
    lrs, losses = learn.lr_find_curve
    assert len(losses) == 6 and np.isfinite(losses).all()
    assert torch.equal(model.flat_param, before)          # lr_find restores the weights


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ddp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from unet_amd.distributed import broadcast_parameters, init_from_env
    from unet_amd.learner import DiceLoss
    from unet_amd.model import HipDynamicUnet
    from unet_amd.optimizer import FlatAdam
    from unet_amd.trainer import TrainStep
    init_from_env(backend="gloo")
    torch.manual_seed(100 + rank)
    model = HipDynamicUnet("xresnet18", 4, 5, (64, 64), device="cuda:0")
    model.train()
    g = torch.Generator().manual_seed(7 + rank)
    x = (torch.randint(0, 256, (2, 4, 64, 64), generator=g).float() / 255).cuda()
    y = torch.randint(0, 5, (2, 64, 64), generator=g).cuda()
    out = []
    for reduction in ("sum", "mean"):
        d = DiceLoss(reduction=reduction)
        broadcast_parameters(model.flat_param, list(model.buffers()))
        model.mark_weights_dirty()
        local_loss = float(model.forward_loss_backward(x, y, None, dice=d).item())      # this rank's own world-1 loss and gradient
        local = model.flat_grad.clone()
        broadcast_parameters(model.flat_param, list(model.buffers()))
        opt = FlatAdam(model, [1e-4, 3e-4, 1e-3])
        step = TrainStep(model, opt, None, world, max_bucket_elems=1 << 20)
        step.dice = d
        step.reducer.reset()
        loss = float(model.forward_loss_backward(x, y, None, world=world, dice=d).item())
        step.reducer.finish()
        torch.cuda.synchronize()
        # 'sum': the terms of one sample do not see the other rank -> reduced gradient = sum of the world-1 gradients;
        # 'mean': the global count of the terms is world times the local one
        want = local.clone()
        dist.all_reduce(want)
        if reduction == "mean":
            want /= world
        ok_grad = bool(((model.flat_grad - want).abs().max() <= 1e-6 * want.abs().max() + 1e-12).item())
        for _ in range(2):
            step(x, y)
        torch.cuda.synchronize()
        p = model.flat_param.clone()
        ref = p.clone()
        dist.broadcast(ref, 0)
        model.grad_ready_hook = None
        out.append((reduction, ok_grad, bool(torch.equal(p, ref)), local_loss, loss))
    q.put((rank, out))
    dist.destroy_process_group()


def test_dice_two_ranks_one_gpu_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=120)
    for i, reduction in enumerate(("sum", "mean")):
        r0, r1 = res[0][i], res[1][i]
        assert r0[:3] == (reduction, True, True) and r1[:3] == (reduction, True, True), res
        want = r0[3] + r1[3] if reduction == "sum" else (r0[3] + r1[3]) / 2
        assert abs(r0[4] - want) <= 1e-6 * abs(want) and r0[4] == r1[4], res
