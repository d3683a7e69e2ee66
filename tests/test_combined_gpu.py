"""CombinedLoss (focal + alpha * Dice) on the device: the fused kernel pair (unet_combined_fwd / unet_combined_bwd / _bf16) against the fp64
restatement (tests/combined_ref.py) and, term by term, against the focal and Dice kernels it replaces; the whole network against the oracle,
the captured training step, the Learner (fit, validate, export / load_learner) and tile-DDP over two ranks on one GPU."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from combined_ref import combined_loss_ref, combined_terms_ref
from util import empty_ts, from_ts, outside_untouched, to_ts

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as O  # noqa: E402  (checker)

ALPHA = 0.7


def _inputs(C, seed):
    """the inputs of test_dice_kernels_against_the_spec: ragged pixel count, targets -100 and C, plus class weights"""
    g = torch.Generator().manual_seed(seed)
    N, H, W = 3, 37, 29
    z = torch.randn(N, C, H, W, generator=g) * 2.0
    y = torch.randint(0, C, (N, H, W), generator=g)
    y[0, 3, :5] = -100
    y[2, 10, 4:9] = C
    w = torch.rand(C, generator=g) + 0.3
    return z, y, w


def _run(zt, y, w, gamma, smooth, square, mean_div, dz, fscale, dscale):
    from unet_amd import ops
    N, C = zt.N, zt.C
    terms = torch.zeros(2, device="cuda")
    coef = torch.zeros(2 * N * C, device="cuda")
    ws = torch.full((ops.combined_workspace(N, zt.H * zt.W, C),), float("nan"), device="cuda")
    ops.combined_fwd(zt, y, w, gamma, smooth, square, mean_div, terms, coef, ws)
    ops.combined_bwd(zt, y, w, gamma, square, coef, fscale, dscale, dz)
    torch.cuda.synchronize()
    return terms.clone(), coef.clone(), dz.buf.clone()


@pytest.mark.parametrize("C", [1, 2, 5, 12, 64])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("square_in_union", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_combined_kernels_against_the_restatement(C, gamma, reduction, square_in_union, weighted):
    """both terms, their sum and the logit gradient on a channel slice of a wider buffer (every CB instantiation and both of its edges), gradient
    scale 0.5; fp32 and direct-bf16 gradients; a NaN-filled workspace; two runs bit-identical; nothing outside the gradient slice written.
    Bars: the ones tests/test_dice_gpu.py and tests/test_focal_gpu.py hold the separate kernels to."""
    from unet_amd import ops
    z, y, w = _inputs(C, C * 64 + int(gamma * 10) * 4 + 2 * (reduction == "mean") + square_in_union)
    w = w if weighted else None
    smooth = 1.0
    N, H, W = y.shape
    z64 = z.double().requires_grad_(True)
    w64 = None if w is None else w.double()
    ref_f, ref_d = combined_terms_ref(z64, y, smooth, gamma, reduction, square_in_union, w64)
    ref_loss = ref_f + ALPHA * ref_d
    ref_loss.backward()
    ref = 0.5 * z64.grad
    f32, d32 = combined_terms_ref(z, y, smooth, gamma, reduction, square_in_union, w, dtype=torch.float32)
    zt = to_ts(z, cs=ops.rup4(C) + 8, co=4)
    yd = y.cuda().contiguous()
    wd = None if w is None else w.cuda()
    mean_div = N * C if reduction == "mean" else 0
    dz = empty_ts(N, H, W, C, cs=ops.rup4(C) + 4, co=4)
    terms, coef, buf = _run(zt, yd, wd, gamma, smooth, square_in_union, mean_div, dz, 0.5, 0.5 * ALPHA)
    got_f, got_d = terms.double().cpu().tolist()
    for what, got, r64, r32 in (("focal", got_f, ref_f.item(), f32.item()), ("dice", got_d, ref_d.item(), d32.item()),
                                ("loss", got_f + ALPHA * got_d, ref_loss.item(), f32.item() + ALPHA * d32.item())):
        print(what, got, r64, r32)
        assert abs(got - r64) <= max(2e-6 * abs(r64), 3 * abs(r32 - r64)), (what, got, r64, r32)
    got = dz.view().permute(0, 3, 1, 2).double().cpu()
    scale = ref.abs().max().item()
    print("grad", (got - ref).abs().max().item(), scale)
    assert (got - ref).abs().max().item() <= 2e-6 * scale, ((got - ref).abs().max().item(), scale)
    assert outside_untouched(dz)
    # bit-reproducible: no atomics, fixed-order sums
    dz2 = empty_ts(N, H, W, C, cs=ops.rup4(C) + 4, co=4)
    terms2, coef2, buf2 = _run(zt, yd, wd, gamma, smooth, square_in_union, mean_div, dz2, 0.5, 0.5 * ALPHA)
    assert torch.equal(terms, terms2) and torch.equal(coef, coef2) and torch.equal(buf, buf2)
    # bf16 gradient slice written directly (logits stay fp32)
    dzb = ops.TS(torch.zeros((N, H, W, ops.rupv(C, torch.bfloat16) + 8), dtype=torch.bfloat16, device="cuda"), 8, C)
    ops.combined_bwd(zt, yd, wd, gamma, square_in_union, coef, 0.5, 0.5 * ALPHA, dzb)
    gb = dzb.view().permute(0, 3, 1, 2).double().cpu()
    assert (gb - ref).abs().max().item() <= 2.0 ** -8 * scale
    outside = torch.ones(dzb.cs, dtype=torch.bool)
    outside[dzb.co:dzb.co + C] = False
    assert (dzb.buf[..., outside] == 0).all()


@pytest.mark.parametrize("C", [5, 12, 64])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("square_in_union", [False, True])
def test_each_term_alone_is_the_existing_kernel(C, gamma, square_in_union):
    """alpha = 0 (Dice scale 0): the gradient of unet_focal_bwd; focal scale 0: the gradient of unet_dice_bwd -- same expressions per
    pixel, so a rounding or two (2e-7 of the largest magnitude) is all that may differ"""
    from unet_amd import ops
    z, y, w = _inputs(C, 900 + C)
    N, H, W = y.shape
    zt = to_ts(z, cs=ops.rup4(C) + 8, co=4)
    yd, wd = y.cuda().contiguous(), w.cuda()
    mean_div = N * C

    def grad(fscale, dscale):
        dz = empty_ts(N, H, W, C)
        _run(zt, yd, wd, gamma, 1.0, square_in_union, mean_div, dz, fscale, dscale)
        return from_ts(dz).double()

    want = empty_ts(N, H, W, C)
    ops.focal_bwd(zt, yd, wd, gamma, 0.5, want)
    want = from_ts(want).double()
    got = grad(0.5, 0.0)
    assert (got - want).abs().max().item() <= 2e-7 * want.abs().max().item(), ((got - want).abs().max().item(), want.abs().max().item())

    loss, coef = torch.zeros(1, device="cuda"), torch.zeros(2 * N * C, device="cuda")
    ops.dice_fwd(zt, yd, 1.0, square_in_union, mean_div, loss, coef, torch.empty(ops.dice_workspace(N, H * W, C), device="cuda"))
    want = empty_ts(N, H, W, C)
    ops.dice_bwd(zt, yd, square_in_union, coef, 0.5, want)
    want = from_ts(want).double()
    got = grad(0.0, 0.5)
    assert (got - want).abs().max().item() <= 2e-7 * want.abs().max().item(), ((got - want).abs().max().item(), want.abs().max().item())


def test_combined_saturated_pixels_and_ignored_targets():
    """the inputs of test_focal_saturated_pixels_and_ignored_targets: a pixel whose cross-entropy is exactly 0 in fp32 and a target of -100
    have no focal gradient -- what they receive is the Dice gradient alone -- and everything stays finite for gamma < 1"""
    from unet_amd import ops
    z = torch.zeros(1, 3, 2, 2)
    z[0, :, 0, 0] = torch.tensor([40.0, -40.0, -40.0])      # ce == 0 exactly
    z[0, :, 0, 1] = torch.tensor([0.3, -0.2, 0.1])
    z[0, :, 1, 0] = torch.tensor([1.0, 2.0, 3.0])
    y = torch.tensor([[[0, 2], [-100, 1]]])
    zt, yd = to_ts(z), y.cuda()
    for gamma in (0.5, 2.0):
        dz = empty_ts(1, 2, 2, 3)
        terms, coef, _ = _run(zt, yd, None, gamma, 1.0, False, 0, dz, 1.0, ALPHA)
        got = from_ts(dz).double()
        assert torch.isfinite(got).all() and torch.isfinite(terms).all() and torch.isfinite(coef).all()
        only = empty_ts(1, 2, 2, 3)
        ops.dice_bwd(zt, yd, False, coef, ALPHA, only)
        only = from_ts(only).double()
        assert only[0, :, 1, 0].abs().max().item() > 1e-3          # the ignored pixel does get a Dice gradient
        tol = 2e-7 * only.abs().max().item()
        assert (got - only)[0, :, 1, 0].abs().max().item() <= tol and (got - only)[0, :, 0, 0].abs().max().item() <= tol
        zz = z.double().requires_grad_(True)
        ref = combined_loss_ref(zz, y, 1.0, ALPHA, gamma)
        ref.backward()
        assert abs(terms[0].item() + ALPHA * terms[1].item() - ref.item()) < 1e-6
        assert (got - zz.grad).abs().max().item() < 1e-6


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
def test_training_step_with_combined_loss(dtype, reduction):
    """forward + CombinedLoss + backward of the whole network against the oracle network + the restated loss (bars of
    test_training_step_with_dice_loss)"""
    from unet_amd.learner import CombinedLoss
    ref, model = _smooth_pair("xresnet18", 4, 3, (64, 64), dtype)
    x, y = O.synthetic_batch(2, 4, 64, 64, 3)
    w = torch.tensor([0.5, 1.5, 1.0])
    ref.train(); model.train()
    loss_ref = combined_loss_ref(ref(x), y, 1.0, ALPHA, 2.0, reduction, False, w.double())
    loss_ref.backward()
    loss = model.forward_loss_backward(x.cuda(), y.cuda(), w.cuda(), combined=CombinedLoss(1, 1.0, ALPHA, gamma=2.0, reduction=reduction))
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


def test_hipgraph_step_with_combined_loss_matches_eager():
    """TrainStep(use_graph=True) replays the CombinedLoss step (alpha applied on the device, no host sync inside): 6 steps agree with the
    eager launch stream (bars of test_hipgraph_step_with_dice_matches_eager)"""
    from unet_amd.learner import CombinedLoss
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
        step = TrainStep(model, opt, torch.tensor([0.3, 2.0, 1.0, 0.5, 1.7], device="cuda"), 1, use_graph=use_graph)
        step.combined = CombinedLoss(1, 0.5, ALPHA, gamma=0.5, reduction="mean", square_in_union=True)
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


def test_learner_fits_validates_exports_with_combined_loss(tmp_path):
    """train.train_unet's sequence with loss_func=CombinedLoss(): class weights assigned to .func.weight (train.py:211) feed the focal term,
    one epoch of two batches, valid_loss = the batch-size-weighted mean of the restated per-batch losses of the oracle network (fastai
    AvgLoss), export / load_learner keep the loss, its arguments and its weights"""
    from unet_amd.learner import CombinedLoss, DataLoaders, DiceMulti, Learner, TileDataset, load_learner
    from unet_amd.model import HipDynamicUnet
    g = np.random.default_rng(0)
    imgs = [g.integers(0, 255, (4, 64, 64)).astype(np.uint8) for _ in range(4)]
    masks = [g.integers(0, 3, (64, 64)).astype(np.uint8) for _ in range(4)]
    torch.manual_seed(1)
    model = HipDynamicUnet("xresnet18", 4, 3, (64, 64))
    dls = DataLoaders(TileDataset(imgs, masks, "int8"), TileDataset(imgs[:3], masks[:3], "int8"), 2, vocab=list("abc"))
    loss = CombinedLoss(1, 0.1, ALPHA, gamma=0.5, reduction="sum", square_in_union=True)
    w = torch.tensor([0.2, 0.3, 0.5])
    loss.func.weight = w
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
        b1 = combined_loss_ref(ref(xs[:2]), ys[:2], 0.1, ALPHA, 0.5, "sum", True, w.double()).item()
        b2 = combined_loss_ref(ref(xs[2:]), ys[2:], 0.1, ALPHA, 0.5, "sum", True, w.double()).item()
    want = (2 * b1 + 1 * b2) / 3
    got = learn.validate()[0]
    assert abs(got - want) < 1e-4 * max(1.0, abs(want)), (got, want)
    learn.export(tmp_path / "combined.pkl")
    back = load_learner(tmp_path / "combined.pkl")
    c = back.loss_func
    assert isinstance(c, CombinedLoss)
    assert (c.smooth, c.alpha, c.gamma, c.reduction, c.square_in_union) == (0.1, ALPHA, 0.5, "sum", True)
    assert torch.allclose(torch.as_tensor(c.func.weight), w)
    assert torch.equal(back.model.flat_param, model.flat_param)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ddp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from unet_amd.distributed import broadcast_parameters, init_from_env
    from unet_amd.learner import CombinedLoss
    from unet_amd.model import HipDynamicUnet
    from unet_amd.optimizer import FlatAdam
    from unet_amd.trainer import TrainStep
    init_from_env(backend="gloo")
    torch.manual_seed(100 + rank)
    model = HipDynamicUnet("xresnet18", 4, 5, (64, 64), device="cuda:0")
    model.train()
    g = torch.Generator().manual_seed(7 + rank)
    x = (torch.randint(0, 256, (2, 4, 64, 64), generator=g).float() / 255).cuda()
    y = torch.randint(0, 5, (2, 64, 64), generator=g)
    if rank == 0:                                   # unequal class mixes: rank 0's tiles are mostly background
        y = torch.where(torch.rand(y.shape, generator=g) < 0.8, torch.zeros_like(y), y)
    y = y.cuda()
    w = torch.tensor([0.3, 2.0, 1.0, 0.5, 1.7], device="cuda")
    out = []
    for reduction in ("sum", "mean"):
        cl = CombinedLoss(1, 1.0, ALPHA, gamma=2.0, reduction=reduction)
        # this rank's share of the global batch from a world-1 step: the focal mean runs over world times as many pixels (1 / world); a Dice
        # term sees one sample only, so 'sum' keeps it whole (alpha * world undoes the 1 / world) and 'mean' divides by world times the count
        share = CombinedLoss(1, 1.0, ALPHA * world if reduction == "sum" else ALPHA, gamma=2.0, reduction=reduction)
        broadcast_parameters(model.flat_param, list(model.buffers()))
        model.mark_weights_dirty()
        local_loss = float(model.forward_loss_backward(x, y, w, grad_scale=1.0 / world, combined=share).item()) / world
        local = model.flat_grad.clone()
        broadcast_parameters(model.flat_param, list(model.buffers()))
        opt = FlatAdam(model, [1e-4, 3e-4, 1e-3])
        step = TrainStep(model, opt, w, world, max_bucket_elems=1 << 20)
        step.combined = cl
        step.reducer.reset()
        loss = float(model.forward_loss_backward(x, y, w, world=world, combined=cl).item())
        step.reducer.finish()
        torch.cuda.synchronize()
        # the restated loss of the concatenated batch, from the logits every rank produced (BatchNorm statistics stay per rank in tile-DDP:
        # "the global batch" is one batch from the logits on)
        z = model.logits_ts().view().permute(0, 3, 1, 2).float().cpu().contiguous()
        zs, ys = [torch.empty_like(z) for _ in range(world)], [torch.empty_like(y.cpu()) for _ in range(world)]
        dist.all_gather(zs, z)
        dist.all_gather(ys, y.cpu())
        restated = combined_loss_ref(torch.cat(zs), torch.cat(ys), 1.0, ALPHA, 2.0, reduction, False, w.cpu().double()).item()
        want = local.clone()
        dist.all_reduce(want)
        ok_grad = bool(((model.flat_grad - want).abs().max() <= 1e-6 * want.abs().max() + 1e-12).item())
        for _ in range(2):
            step(x, y)
        torch.cuda.synchronize()
        p = model.flat_param.clone()
        ref = p.clone()
        dist.broadcast(ref, 0)
        model.grad_ready_hook = None
        out.append((reduction, ok_grad, bool(torch.equal(p, ref)), local_loss, loss, restated))
    q.put((rank, out))
    dist.destroy_process_group()


def test_combined_two_ranks_one_gpu_gloo():
    """unequal class mixes per rank, non-uniform class weights, both reductions: the loss every rank reports is the loss of the concatenated
    batch, and the SUM all-reduce of the gradients is the sum of the ranks' shares of that batch's gradient (bars of
    test_dice_two_ranks_one_gpu_gloo; against the fp64 restatement the kernels' own 2e-6)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=300) for _ in procs)
    finally:
        for p in procs:                             # each child under its own time limit
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for i, reduction in enumerate(("sum", "mean")):
        r0, r1 = res[0][i], res[1][i]
        assert r0[:3] == (reduction, True, True) and r1[:3] == (reduction, True, True), res
        want = r0[3] + r1[3]
        assert abs(r0[4] - want) <= 1e-6 * abs(want) and r0[4] == r1[4], res
        assert abs(r0[4] - r0[5]) <= 2e-6 * abs(r0[5]) and r0[5] == r1[5], res
