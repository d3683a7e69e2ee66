"""GPU suite of the border-weighted cross-entropy: the border distance (csrc/edt.hip) compared for exact integer equality with the NumPy /
scipy restatement (tests/border_ref.py), the weight map against float64, the per-pixel-weighted cross-entropy kernels against the
class-weighted ones (bit for bit) and against torch float64, and the whole step: oracle network, captured step, two ranks, Learner.
Every device buffer of unet_amd/border.py sits in a guard-banded allocation that is checked after every call."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import border_ref as R
from guard import guarded
from unet_amd import border as BD  # the feature: without it this module does not import
from util import empty_ts, from_ts, outside_untouched, to_ts

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as O  # noqa: E402  (checker)

_FILL = {torch.uint8: 0xA5, torch.int32: -7, torch.int64: -7, torch.float32: -3.0e7}
_NP = {"uint8": np.uint8, "int64": np.int64}


class Guards:
    def __init__(self):
        self.checks = []

    def alloc(self, shape, dtype, device):
        t, c = guarded(shape, dtype, device, _FILL[dtype])
        self.checks.append(c)
        return t

    def upload(self, a: np.ndarray) -> torch.Tensor:
        src = torch.from_numpy(np.ascontiguousarray(a))
        t = self.alloc(src.shape, src.dtype, "cuda")
        t.copy_(src)
        return t

    def check(self, what=""):
        torch.cuda.synchronize()
        for c in self.checks:
            c(what)


@pytest.fixture
def guards(monkeypatch):
    from unet_amd import ops
    g = Guards()
    monkeypatch.setattr(BD, "_alloc", g.alloc)
    for name in ("border_edt", "border_weight"):
        def wrapped(*a, _fn=getattr(ops, name), _name=name, **k):
            r = _fn(*a, **k)
            g.check(_name)
            return r
        monkeypatch.setattr(ops, name, wrapped)
    return g


def _inputs(shape, dt):
    """(name, mask [B', H, W], exclude) of one shape: blocky classes, salt noise, a uniform image between two busy ones, the corner mask
    (the farthest search: at 512^2 D2 reaches 511^2 + 510^2) and exclude=0 where class 0 touches the other classes"""
    B, H, W = shape
    rng = np.random.default_rng(B * 1000003 + H * 1009 + W)
    blocky, salt = R.blocky(rng, B, H, W, dtype=dt), R.salt(rng, B, H, W, dtype=dt)
    mid = np.stack([blocky[0], np.full((H, W), 2, dtype=dt), salt[0]])
    return [("blocky", blocky, None), ("salt", salt, None), ("uniform between busy", mid, None), ("corner", R.corner(B, H, W, dt), None),
            ("blocky exclude 0", blocky, 0), ("salt exclude 0", salt, 0), ("uniform exclude its class", mid, 2)]


@pytest.mark.parametrize("dtype", ["uint8", "int64"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_distance_equals_the_reference_exactly(guards, shape, dtype):
    """D2 == the reference on int32, for both mask dtypes; two runs give the same bits; host and NumPy input come back as their kind"""
    dt = _NP[dtype]
    for name, m, ex in _inputs(shape, dt):
        want = R.d2_scipy(m, ex)
        md = guards.upload(m)
        got = BD.distance_to_border(md, exclude=ex)
        guards.check(name)
        assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == m.shape
        bad = np.argwhere(got.cpu().numpy() != want)
        assert len(bad) == 0, (name, shape, dtype, len(bad), bad[:4], got.cpu().numpy()[tuple(bad[0])], want[tuple(bad[0])])
        if name == "uniform between busy":
            assert (got[1] == BD.NO_BORDER).all() and (got[0] != BD.NO_BORDER).any() == bool(R.edge_set(m[0]).any())
        if name == "blocky":
            assert torch.equal(BD.distance_to_border(md), got)
            h = BD.distance_to_border(torch.from_numpy(m))
            assert isinstance(h, torch.Tensor) and not h.is_cuda and np.array_equal(h.numpy(), want)
            n = BD.distance_to_border(m[0])                                  # one [H, W] image, NumPy in and out
            assert isinstance(n, np.ndarray) and n.dtype == np.int32 and np.array_equal(n, want[0])
            guards.check("host input")
        guards.checks.clear()


def _close(got, ref, rtol=1e-5, atol=1e-30):
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > atol + rtol * np.abs(ref)
    assert not bad.any(), (int(bad.sum()), float((err / np.maximum(np.abs(ref), 1e-300))[bad].max()))


@pytest.mark.parametrize("sigma", [5.0, 3.3, 40.0])
@pytest.mark.parametrize("shape", [(2, 37, 53), (3, 64, 64), (1, 512, 512)], ids=lambda s: "x".join(map(str, s)))
def test_weight_map_against_float64(guards, shape, sigma):
    """rtol 1e-5, atol 1e-30 against the float64 restatement.  The exponent is rounded once to fp32 (relative 6e-8: at a magnitude of 87,
    where the result leaves the fp32 range, 5e-6 absolute = 5e-6 relative in the result), expf and the sum add a few 1e-7.  The sentinel
    gives exactly class_w[y]; targets outside [0, C) give exactly 0."""
    B, H, W = shape
    rng = np.random.default_rng(H + W)
    C, w0 = 4, 10.0
    cw = np.array([0.5, 1.5, 0.0, 2.0], dtype=np.float32)
    m = R.blocky(rng, B, H, W, dtype=np.int64) if H < 512 else R.corner(B, H, W, np.int64)
    m[0, 0, : min(W, 5)] = -100
    m[0, H - 1, : min(W, 3)] = C
    for cwi, ex in ((cw, None), (None, 0)):
        d2 = R.d2_scipy(m, ex)
        ref = R.weight_map(m, d2, cwi, w0, sigma, C)
        got = BD.border_weight_map(guards.upload(m), None if cwi is None else torch.from_numpy(cwi), w0, sigma, ex, n_classes=C)
        guards.check("weight map")
        assert got.is_cuda and got.dtype == torch.float32
        g = got.cpu().numpy()
        _close(g, ref)
        assert (g[(m < 0) | (m >= C)] == 0).all()
        guards.checks.clear()
    u8 = R.blocky(rng, B, H, W, dtype=np.uint8)
    u8[B - 1] = 3                                                            # an image without a border: exactly the class weight
    got = BD.border_weight_map(u8, cw, w0, sigma)
    guards.check("uint8 NumPy input")
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and (got[B - 1] == cw[3]).all()
    _close(got, R.weight_map(u8, R.d2_scipy(u8), cw, w0, sigma, C))


def _ce_case(C, seed):
    from unet_amd import ops
    g = torch.Generator().manual_seed(seed)
    N, H, W = 3, 37, 29
    z = torch.randn(N, C, H, W, generator=g) * 3
    y = torch.randint(0, C, (N, H, W), generator=g)
    y[0, 3, :5] = -100
    y[2, 10, 4:9] = C
    zt = to_ts(z, cs=ops.rup4(C) + 8, co=4)
    return N, H, W, z, y, zt, y.cuda().contiguous()


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("C", [1, 2, 5, 12, 64])
def test_pw_kernels_reproduce_the_class_weighted_ones(C, weighted):
    """pw[p] = w[y(p)] (1 without class weights; anything on ignored targets): ce_fwd_pw / ce_fwd_parts_pw / ce_bwd_pw give the bits of
    ce_fwd / ce_fwd_parts / ce_bwd, in fp32 and bf16 dz, on a strided logits slice"""
    from unet_amd import ops
    N, H, W, z, y, zt, yd = _ce_case(C, 40 + C)
    g = torch.Generator().manual_seed(C)
    w = (torch.rand(C, generator=g) + 0.2).cuda() if weighted else None
    ok = (yd >= 0) & (yd < C)
    pw = torch.where(ok, (w if weighted else torch.ones(C, device="cuda"))[yd.clamp(0, C - 1)], torch.full_like(yd, 9, dtype=torch.float32))
    pw = pw.reshape(-1).contiguous()
    P = N * H * W
    outs = []
    for fwd, parts, bwd, wt in ((ops.ce_fwd, ops.ce_fwd_parts, ops.ce_bwd, w), (ops.ce_fwd_pw, ops.ce_fwd_parts_pw, ops.ce_bwd_pw, pw)):
        ws = torch.full((ops.ce_workspace(P),), float("nan"), device="cuda")
        lo, den, nd = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(2, device="cuda")
        fwd(zt, yd, wt, lo, den, ws)
        parts(zt, yd, wt, nd, ws)
        dz = empty_ts(N, H, W, C, cs=ops.rup4(C) + 8, co=4)
        bwd(zt, yd, wt, den, 0.5, dz)
        dzb = ops.TS(torch.zeros((N, H, W, ops.rupv(C, torch.bfloat16) + 8), dtype=torch.bfloat16, device="cuda"), 8, C)
        bwd(zt, yd, wt, den, 0.5, dzb)
        torch.cuda.synchronize()
        assert outside_untouched(dz)
        outs.append((lo.cpu(), den.cpu(), nd.cpu(), dz.buf.cpu(), dzb.buf.cpu()))
    assert torch.isfinite(outs[0][0]).all() and outs[0][1].item() > 0
    for a, b, what in zip(outs[0], outs[1], ("loss", "denom", "parts", "dz", "dz bf16")):
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                           b.view(torch.int32 if b.dtype == torch.float32 else torch.int16)), what


@pytest.mark.parametrize("C", [1, 2, 5, 12, 64])
def test_pw_kernels_against_float64(C):
    """a random positive map: loss within 1e-5 max(1, |loss|), gradient rtol 1e-4 atol 1e-9 (the bars of test_cross_entropy); the parts are
    the undivided sums; a rank whose map is zero everywhere gets parts (0, 0), not NaN"""
    from unet_amd import ops
    N, H, W, z, y, zt, yd = _ce_case(C, 60 + C)
    g = torch.Generator().manual_seed(7 * C)
    pw = torch.rand(N * H * W, generator=g) * 3 + 0.01
    loss, grad, num, den = R.pw_ce(z.permute(0, 2, 3, 1).reshape(-1, C), y.reshape(-1), pw)
    P = N * H * W
    ws = torch.full((ops.ce_workspace(P),), float("nan"), device="cuda")
    lo, dn, nd = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda"), torch.full((2,), float("nan"), device="cuda")
    pwd = pw.cuda()
    ops.ce_fwd_pw(zt, yd, pwd, lo, dn, ws)
    ops.ce_fwd_parts_pw(zt, yd, pwd, nd, ws)
    dz = empty_ts(N, H, W, C, cs=ops.rup4(C) + 8, co=4, fill=0.0)
    ops.ce_bwd_pw(zt, yd, pwd, dn, 1.0, dz)
    torch.cuda.synchronize()
    print("loss", lo.item(), loss.item(), "parts", nd.tolist(), num.item(), den.item())
    assert abs(lo.item() - loss.item()) <= 1e-5 * max(1.0, abs(loss.item()))
    assert abs(nd[0].item() - num.item()) <= 1e-5 * max(1.0, abs(num.item())) and abs(nd[1].item() - den.item()) <= 1e-5 * den.item()
    assert dn.item() == nd[1].item()
    ref = grad.reshape(N, H, W, C).permute(0, 3, 1, 2)
    got = from_ts(dz).double()
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    print("grad err", err, "scale", scale)
    assert err <= 1e-4 * scale + 1e-9
    ops.ce_fwd_parts_pw(zt, yd, torch.zeros(P, device="cuda"), nd, ws)
    torch.cuda.synchronize()
    assert nd.tolist() == [0.0, 0.0]
    for bad in (pwd[:-1], pwd.double(), pwd.cpu(), torch.ones(2 * P, device="cuda")[::2]):
        with pytest.raises(ValueError):
            ops.ce_fwd_pw(zt, yd, bad, lo, dn, ws)
        with pytest.raises(ValueError):
            ops.ce_bwd_pw(zt, yd, bad, dn, 1.0, dz)


def _smooth_pair(arch, n_in, n_out, size, dtype):
    """oracle + HIP network with the same weights; a smooth network (large BN shifts, small convs: no ReLU flips) as in the Dice test"""
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


def _ref_loss(logits, y, cw, w0, sigma, exclude):
    """the restated loss on the oracle network's logits [B, C, H, W] (torch, differentiable)"""
    C = logits.shape[1]
    pw = torch.from_numpy(R.weight_map(y.numpy(), R.d2_scipy(y.numpy(), exclude), cw, w0, sigma, C)).to(logits.dtype)
    nll = torch.nn.functional.cross_entropy(logits, y, reduction="none")
    return (pw * nll).sum() / pw.sum()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_step_with_border_loss(dtype):
    """forward + border-weighted cross-entropy + backward of the whole network against the oracle network + the restated loss, at the
    tolerances of test_training_step_with_dice_loss; the generic torch path of the loss object gives the same number; the step refuses
    border= together with another loss"""
    from unet_amd.learner import BorderWeightedCrossEntropy, DiceLoss
    ref, model = _smooth_pair("xresnet18", 4, 3, (64, 64), dtype)
    x, y = O.synthetic_batch(2, 4, 64, 64, 3)
    cw = [0.5, 1.5, 1.0]
    b = BorderWeightedCrossEntropy(weight=torch.tensor(cw), w0=10.0, sigma=5.0, exclude=0)
    ref.train(); model.train()
    out = ref(x)
    loss_ref = _ref_loss(out, y, cw, b.w0, b.sigma, b.exclude)
    loss_ref.backward()
    loss = model.forward_loss_backward(x.cuda(), y.cuda(), torch.tensor(cw, device="cuda"), border=b)
    torch.cuda.synchronize()
    tol = 1e-4 if dtype == "f32" else 3e-2
    print("loss", loss.item(), loss_ref.item())
    assert abs(loss.item() - loss_ref.item()) < tol * max(1.0, abs(loss_ref.item())), (loss.item(), loss_ref.item())
    g_hip = torch.cat([p.grad.flatten().cpu() for p in model.parameters()])
    g_ref = torch.cat([p.grad.flatten() for p in ref.parameters()])
    cos = torch.nn.functional.cosine_similarity(g_hip.double(), g_ref.double(), dim=0).item()
    print("cos", cos)
    assert cos > (1 - 1e-6 if dtype == "f32" else 0.99), cos
    if dtype == "f32":
        worst = max((p.grad.cpu() - q.grad).abs().max().item() / (q.grad.abs().max().item() + 1e-12)
                    for p, q in zip(model.parameters(), ref.parameters()) if q.grad.abs().max().item() > 1e-20)
        print("worst", worst)
        assert worst < 2e-3, worst
        generic = b(out.detach().cuda(), y.cuda())
        assert abs(generic.item() - loss_ref.item()) < 1e-5 * max(1.0, abs(loss_ref.item()))
        for kw in ({"dice": DiceLoss()}, {"focal_gamma": 2.0}, {"reg_kind": "mse"}, {"combined": object()}):
            with pytest.raises(ValueError):
                model.forward_loss_backward(x.cuda(), y.cuda(), None, border=b, **kw)


def test_hipgraph_step_with_border_loss_equals_eager():
    """TrainStep(use_graph=True) captures the border step (no host sync inside): the two eager warm-up steps and three replays equal five
    eager steps bit for bit (both runs without the second stream of the weight gradients, which a captured step never uses)"""
    from unet_amd.learner import BorderWeightedCrossEntropy
    from unet_amd.model import HipDynamicUnet
    from unet_amd.optimizer import FlatAdam
    from unet_amd.trainer import TrainStep
    torch.manual_seed(11)
    sd = O.DynamicUnet("xresnet18", 4, 5, (64, 64)).state_dict()
    xs = [O.synthetic_batch(2, 4, 64, 64, 5, seed=s) for s in range(5)]
    outs = []
    for use_graph in (False, True):
        model = HipDynamicUnet("xresnet18", 4, 5, (64, 64))
        model.load_state_dict(sd)
        model.train()
        model.ctx.wgrad_overlap = False
        opt = FlatAdam(model, [1e-4, 3e-4, 1e-3])
        step = TrainStep(model, opt, torch.tensor([0.3, 2.0, 1.0, 0.5, 1.7], device="cuda"), 1, use_graph=use_graph)
        step.border = BorderWeightedCrossEntropy(w0=6.0, sigma=3.0, exclude=0)
        losses = []
        for i, (x, y) in enumerate(xs):
            opt.set_lr([1e-4 * (i + 1), 3e-4, 1e-3 / (i + 1)])
            opt.mom = 0.95 - 0.01 * i
            losses.append(step(x.cuda(), y.cuda()).clone())
        torch.cuda.synchronize()
        assert (step._graph is not None) == use_graph
        outs.append((torch.stack(losses).cpu(), model.flat_param.clone().cpu()))
    print("losses", outs[0][0].flatten().tolist(), outs[1][0].flatten().tolist(), "param diff", (outs[0][1] - outs[1][1]).abs().max().item())
    assert torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0]), (outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])


def test_learner_fits_validates_exports_with_border_loss(tmp_path):
    """train.train_unet's sequence with loss_func=BorderWeightedCrossEntropy(): class weights through .func.weight (train.py:211), one epoch,
    valid_loss = sum of the batches' numerators / sum of their denominators of the restated loss on the oracle network, export /
    load_learner keep the loss and its three numbers, lr_find runs through the fused step"""
    from unet_amd.learner import BorderWeightedCrossEntropy, DataLoaders, DiceMulti, Learner, TileDataset, load_learner
    from unet_amd.model import HipDynamicUnet
    g = np.random.default_rng(0)
    imgs = [g.integers(0, 255, (4, 64, 64)).astype(np.uint8) for _ in range(4)]
    masks = [R.blocky(g, 1, 64, 64, n_classes=3)[0] for _ in range(4)]
    torch.manual_seed(1)
    model = HipDynamicUnet("xresnet18", 4, 3, (64, 64))
    dls = DataLoaders(TileDataset(imgs, masks, "int8"), TileDataset(imgs[:3], masks[:3], "int8"), 2, vocab=list("abc"))
    loss = BorderWeightedCrossEntropy(axis=1, w0=4.0, sigma=2.5, exclude=0)
    cw = [0.2, 0.3, 0.5]
    loss.func.weight = torch.tensor(cw)
    learn = Learner(dls, model, loss_func=loss, metrics=[DiceMulti()], path=tmp_path)
    learn._no_logging = True
    assert "BorderWeightedCrossEntropy" in learn.summary()
    learn.fit_one_cycle(1, lr_max=slice(1e-4, 1e-3))
    torch.cuda.synchronize()
    assert len(learn.recorder.losses) == 2 and all(np.isfinite(learn.recorder.losses))
    ref = O.DynamicUnet("xresnet18", 4, 3, (64, 64))
    ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    ref.eval()
    with torch.no_grad():
        xs = torch.from_numpy(np.stack(imgs[:3]).astype(np.float32) / 255.0)
        ys = torch.from_numpy(np.stack(masks[:3]).astype(np.int64))
        pw = torch.from_numpy(R.weight_map(ys.numpy(), R.d2_scipy(ys.numpy(), 0), cw, 4.0, 2.5, 3))
        nll = torch.nn.functional.cross_entropy(ref(xs).double(), ys, reduction="none")
        want = ((pw * nll).sum() / pw.sum()).item()
    got = learn.validate()[0]
    print("valid_loss", got, want)
    assert abs(got - want) < 1e-4 * max(1.0, abs(want)), (got, want)
    learn.export(tmp_path / "border.pkl")
    back = load_learner(tmp_path / "border.pkl")
    d = back.loss_func
    assert type(d) is BorderWeightedCrossEntropy and (d.w0, d.sigma, d.exclude) == (4.0, 2.5, 0)
    assert torch.allclose(torch.as_tensor(d.func.weight), torch.tensor(cw))
    assert torch.equal(back.model.flat_param, model.flat_param)
    before = model.flat_param.clone()
    learn.lr_find(start_lr=1e-6, end_lr=1e-3, num_it=6)
    lrs, losses = learn.lr_find_curve
    assert len(losses) == 6 and np.isfinite(losses).all()
    assert torch.equal(model.flat_param, before)          # lr_find restores the weights


def test_plain_cross_entropy_step_is_untouched():
    """a plain CrossEntropyLossFlat step gives the bits of the same launches made here through ops.ce_fwd / ops.ce_bwd: loss, logit
    gradient and the whole flat gradient"""
    from unet_amd import ops
    from unet_amd.model import HipDynamicUnet
    torch.manual_seed(5)
    model = HipDynamicUnet("xresnet18", 4, 3, (64, 64))
    model.train()
    x, y = O.synthetic_batch(2, 4, 64, 64, 3)
    xd, yd = x.cuda(), y.cuda().contiguous()
    w = torch.tensor([0.5, 1.5, 1.0], device="cuda")
    loss = model.forward_loss_backward(xd, yd, w).clone()
    grad = model.flat_grad.clone()
    z = model._hip_forward(xd, True)
    dz = model.ctx.act(model, "dlogits", z.N, z.H, z.W, z.C, zero=True)
    lo, den = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    ops.ce_fwd(z, yd, w, lo, den, torch.empty(ops.ce_workspace(z.P), device="cuda"))
    ops.ce_bwd(z, yd, w, den, 1.0, dz)
    model._ensure_grad_views()
    model._hip_backward(dz)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and grad.abs().sum().item() > 0
    assert torch.equal(lo, loss)
    assert torch.equal(model.flat_grad, grad)
    assert grad.double().sum().item() == model.flat_grad.double().sum().item()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ddp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from unet_amd.distributed import broadcast_parameters, init_from_env
    from unet_amd.learner import BorderWeightedCrossEntropy
    from unet_amd.model import HipDynamicUnet
    from unet_amd.optimizer import FlatAdam
    from unet_amd.trainer import TrainStep
    init_from_env(backend="gloo")
    torch.manual_seed(100 + rank)
    model = HipDynamicUnet("xresnet18", 4, 5, (64, 64), device="cuda:0")
    model.train()
    g = np.random.default_rng(7 + rank)
    x = torch.from_numpy(g.integers(0, 256, (2, 4, 64, 64)).astype(np.float32) / 255).cuda()
    y = torch.from_numpy(R.blocky(g, 2, 64, 64, n_classes=5, block=4 + 4 * rank, dtype=np.int64)).cuda()      # different border densities
    w = torch.tensor([0.3, 2.0, 1.0, 0.5, 1.7], device="cuda")
    b = BorderWeightedCrossEntropy(w0=10.0, sigma=5.0, exclude=0)
    broadcast_parameters(model.flat_param, list(model.buffers()))
    model.mark_weights_dirty()
    local_loss = float(model.forward_loss_backward(x, y, w, border=b).item())      # this rank's own world-1 loss and gradient
    local_den = model.ctx.vec(model, "denom", 1).clone()
    local = model.flat_grad.clone() * local_den            # = the gradient of this rank's numerator
    broadcast_parameters(model.flat_param, list(model.buffers()))
    opt = FlatAdam(model, [1e-4, 3e-4, 1e-3])
    step = TrainStep(model, opt, w, world, max_bucket_elems=1 << 20)
    step.border = b
    step.reducer.reset()
    loss = float(model.forward_loss_backward(x, y, w, world=world, border=b).item())
    step.reducer.finish()
    torch.cuda.synchronize()
    # one cross-entropy over the global batch: sum of the ranks' numerators (and of their gradients) over the sum of their denominators
    want, den = local.clone(), local_den.clone()
    dist.all_reduce(want)
    dist.all_reduce(den)
    want /= den
    ok_grad = bool(((model.flat_grad - want).abs().max() <= 1e-6 * want.abs().max() + 1e-12).item())
    for _ in range(2):
        step(x, y)
    torch.cuda.synchronize()
    p = model.flat_param.clone()
    ref = p.clone()
    dist.broadcast(ref, 0)
    model.grad_ready_hook = None
    q.put((rank, (ok_grad, bool(torch.equal(p, ref)), local_loss, float(local_den.item()), loss)))
    dist.destroy_process_group()


def test_border_two_ranks_one_gpu_gloo():
    """two ranks with different tiles (and different denominators) equal one cross-entropy over the concatenated batch: the loss is
    sum num_r / sum den_r, the reduced gradient its gradient, and both ranks hold the same parameters after two steps"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=120)
    r0, r1 = res[0], res[1]
    assert r0[:2] == (True, True) and r1[:2] == (True, True), res
    want = (r0[2] * r0[3] + r1[2] * r1[3]) / (r0[3] + r1[3])
    assert r0[3] != r1[3]
    assert abs(r0[4] - want) <= 1e-6 * abs(want) and r0[4] == r1[4], res
