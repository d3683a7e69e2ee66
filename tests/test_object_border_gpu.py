"""GPU suite of the two-object border weight (csrc/object_edt.hip): D1 and D2 compared for exact integer equality with the NumPy / scipy
restatement (tests/object_border_ref.py), the weight map against float64, and the whole step with objects=True: oracle network, captured
step, Learner, two ranks.  Every device buffer of unet_amd/border.py sits in a guard-banded allocation that is checked after every call.
With the new arguments at their defaults nothing new is launched and every bit is what it was."""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import border_ref as BR
import object_border_ref as R
from guard import guarded
from unet_amd import border as BD

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as O  # noqa: E402  (checker)

_FILL = {torch.uint8: 0xA5, torch.int32: -7, torch.int64: -7, torch.float32: -3.0e7}
_NP = {"uint8": np.uint8, "int64": np.int64}
_NEW_OPS = ("object_edt", "object_border_weight")
NO = R.NO_OBJECT

SHAPES = [(1, 1, 1), (1, 1, 70), (1, 70, 1), (2, 37, 53), (3, 64, 64), (1, 65, 130), (1, 8, 1030), (2, 512, 512)]


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
    for name in _NEW_OPS:
        def wrapped(*a, _fn=getattr(ops, name), _name=name, **k):
            r = _fn(*a, **k)
            g.check(_name)
            return r
        monkeypatch.setattr(ops, name, wrapped)
    return g


def _radii(shape):
    """1, 7, 30, and 255 on the small shapes"""
    return (1, 7, 30) if shape[1] * shape[2] > 1 << 14 else (1, 7, 30, 255)


@functools.lru_cache(maxsize=None)
def _masks(shape):
    """(name, int64 mask [B', H, W] with values 0 ... 3, keywords) of one shape.  Blocky classes and salt noise (at 512^2: larger blocks and
    sparser salt, which keep the reference's per-object search short); an all-background and an all-object image between two busy ones; the
    same class on the last row of image 0 and the first row of image 1; class 2 excluded; values >= n_classes; another background class"""
    B, H, W = shape
    rng = np.random.default_rng(B * 1000003 + H * 1009 + W)
    big = H * W > 1 << 14
    blocky = R.blocky(rng, B, H, W, block=64 if big else 8, dtype=np.int64)
    salt = R.salt(rng, B, H, W, density=0.002 if big else 0.15, dtype=np.int64)
    seam = np.zeros((2, H, W), dtype=np.int64)
    seam[0, H - 1, :] = 1
    seam[1, 0, :] = 1
    out = [("blocky", blocky, {}), ("salt", salt, {}), ("seam", seam, {}), ("blocky exclude 2", blocky, {"exclude": 2})]
    if not big:
        between = np.stack([blocky[0], np.zeros((H, W), dtype=np.int64), np.ones((H, W), dtype=np.int64), salt[0]])
        out += [("uniform between busy", between, {}), ("salt exclude 2", salt, {"exclude": 2}), ("blocky n_classes 3", blocky, {"n_classes": 3}),
                ("blocky background 1", blocky, {"background": 1, "exclude": 0})]
    return out


@functools.lru_cache(maxsize=None)
def _want(shape, name, radius):
    """the reference of one case, computed once for both mask dtypes"""
    m, kw = next((m, kw) for n, m, kw in _masks(shape) if n == name)
    return R.d1d2(m, radius=radius, **kw)


def _assert_equal(got, want, what):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = np.argwhere(g != want)
    assert len(bad) == 0, (what, len(bad), bad[:4], g[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("dtype", ["uint8", "int64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_distances_equal_the_reference_exactly(guards, shape, dtype):
    """D1 == and D2 == the reference on int32 for both mask dtypes and every radius; two runs give the same bits; host and NumPy input come
    back as their kind"""
    dt = _NP[dtype]
    for name, m64, kw in _masks(shape):
        m = m64.astype(dt)
        md = guards.upload(m)
        for radius in _radii(shape):
            w1, w2 = _want(shape, name, radius)
            d1, d2 = BD.distance_to_objects(md, radius=radius, **kw)
            guards.check(name)
            assert d1.is_cuda and d1.dtype == torch.int32 and tuple(d1.shape) == m.shape and d2.dtype == torch.int32
            _assert_equal(d1, w1, (name, shape, dtype, radius, "D1"))
            _assert_equal(d2, w2, (name, shape, dtype, radius, "D2"))
            if name == "seam":                                               # distinct objects, and no distance across the seam
                H = shape[1]
                assert (w2 == NO).all() and w1[0, 0, 0] == ((H - 1) ** 2 if 0 < H - 1 <= radius else NO)
            if name == "uniform between busy":
                assert (d1[1] == NO).all() and (d1[2] == NO).all() and (d2[1:3] == NO).all()
            if name == "blocky" and radius == 7:
                e1, e2 = BD.distance_to_objects(md, radius=radius)
                assert torch.equal(e1, d1) and torch.equal(e2, d2)
                h1, h2 = BD.distance_to_objects(torch.from_numpy(m), radius=radius)
                assert isinstance(h1, torch.Tensor) and not h1.is_cuda and np.array_equal(h1.numpy(), w1) and np.array_equal(h2.numpy(), w2)
                n1, n2 = BD.distance_to_objects(m[0], radius=radius)         # one [H, W] image, NumPy in and out
                assert isinstance(n1, np.ndarray) and n1.dtype == np.int32 and np.array_equal(n1, w1[0]) and np.array_equal(n2, w2[0])
                guards.check("host input")
        guards.checks.clear()


def _scene(h, w, *objs, fill=0):
    m = np.full((1, h, w), fill, dtype=np.int64)
    for y, x, v in objs:
        m[0, y, x] = v
    return m


def test_hand_scenes(guards):
    """the cases that single out one rule each, checked against the reference and against the number the rule gives by hand"""
    def run(m, radius, **kw):
        w1, w2 = R.d1d2(m, radius=radius, **kw)
        for dt in (np.uint8, np.int64):
            if dt == np.uint8 and (m.min() < 0 or m.max() > 255):
                continue
            d1, d2 = BD.distance_to_objects(guards.upload(m.astype(dt)), radius=radius, **kw)
            guards.check("scene")
            _assert_equal(d1, w1, ("D1", radius, kw))
            _assert_equal(d2, w2, ("D2", radius, kw))
        guards.checks.clear()
        return w1[0], w2[0]
    # three different objects stacked in one column within the radius: the third is dropped by the column pass and must not be missed
    m = _scene(24, 9, (2, 4, 1), (4, 4, 2), (6, 4, 1), (8, 4, 3), (20, 4, 2))
    for r in (3, 7, 30):
        D1, D2 = run(m, r)
    assert (D1[10, 4], D2[10, 4]) == (4, 16) and (D1[5, 4], D2[5, 4]) == (1, 1) and (D1[5, 0], D2[5, 0]) == (17, 17)
    # a column of three whose third is the nearest for a pixel far to the side of the fourth column
    m = _scene(9, 40, (1, 0, 1), (4, 0, 2), (7, 0, 3), (4, 30, 1))
    D1, D2 = run(m, 30)
    assert (D1[1, 29], D2[1, 29]) == (10, 29 * 29)
    # a U-shaped single object around background: D1 small, D2 NO_OBJECT, the term 0
    m = _scene(12, 12)
    m[0, 2:10, 2] = m[0, 2:10, 9] = m[0, 9, 2:10] = 1
    D1, D2 = run(m, 30)
    assert D1[5, 5] == 9 and (D2 == NO).all()
    pw = BD.border_weight_map(guards.upload(m), None, 10.0, 5.0, n_classes=2, objects=True)
    guards.check("U")
    assert (pw == 1.0).all()
    guards.checks.clear()
    # two objects at equal distance
    D1, D2 = run(_scene(9, 15, (4, 2, 1), (4, 12, 1)), 7)
    assert (D1[4, 7], D2[4, 7]) == (25, 25)
    # delta == radius^2 counts, radius^2 + 1 does not: axis-aligned and on a diagonal, radius 5
    D1, D2 = run(_scene(21, 21, (10, 15, 1), (13, 14, 2)), 5)            # (0, 5) and (3, 4): both 25
    assert (D1[10, 10], D2[10, 10]) == (25, 25)
    D1, D2 = run(_scene(21, 21, (10, 16, 1), (14, 14, 2), (5, 9, 3)), 5)  # (0, 6): 36, (4, 4): 32, (-5, -1): 26
    assert (D1[10, 10], D2[10, 10]) == (NO, NO)
    D1, D2 = run(_scene(21, 21, (15, 10, 1), (6, 7, 2), (10, 4, 3)), 5)   # (5, 0): 25, (-4, -3): 25, (0, -6): 36
    assert (D1[10, 10], D2[10, 10]) == (25, 25)
    # exclude pixels between a background pixel and an object are transparent, and they separate nothing by themselves
    m = _scene(5, 12, (2, 6, 1), (2, 7, 1))
    m[0, :, 3:6] = 9
    D1, D2 = run(m, 30, exclude=9)
    assert (D1[2, 0], D2[2, 0]) == (36, NO) and D1[2, 4] == NO
    # values >= n_classes and negative ones are excluded too
    m = _scene(5, 12, (2, 6, 1), (2, 9, 2), (2, 3, 5), (0, 0, -100), (4, 4, 1000))
    D1, D2 = run(m, 30, n_classes=3)
    assert (D1[2, 2], D2[2, 2]) == (16, 49) and D1[2, 3] == NO


def _close(got, ref, rtol=1e-5, atol=1e-30):
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > atol + rtol * np.abs(ref)
    assert not bad.any(), (int(bad.sum()), float((err / np.maximum(np.abs(ref), 1e-300))[bad].max()))


@pytest.mark.parametrize("sigma,radius", [(5.0, None), (3.3, None), (40.0, 60)])
@pytest.mark.parametrize("shape", [(2, 37, 53), (3, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_weight_map_against_float64(guards, shape, sigma, radius):
    """rtol 1e-5, atol 1e-30 against the float64 restatement, the bars of the nearest-border map's test, for its reason: the exponent, of
    a magnitude up to (2 * 6 sigma)^2 / (2 sigma^2) = 72 < 87, is rounded once to fp32 (relative 6e-8, so at most 5e-6 in the result), expf
    and the sum add a few 1e-7.  The background's class weight is 0 in one pass, so the term is compared on its own there.  The term is
    exactly 0 where the reference's D2 is NO_OBJECT; targets outside [0, C) give exactly 0."""
    B, H, W = shape
    rng = np.random.default_rng(H + W)
    C, w0 = 4, 10.0
    m = R.blocky(rng, B, H, W, block=6, dtype=np.int64)
    m[0, 0, : min(W, 5)] = -100
    m[0, H - 1, : min(W, 3)] = C
    m[B - 1] = 0
    m[B - 1, 3:6, 3:6] = 1                                                   # one object alone: D1 finite, D2 NO_OBJECT, no term
    rr = R.default_radius(sigma) if radius is None else radius
    for cwi, ex in ((np.array([0.0, 1.5, 0.5, 2.0], dtype=np.float32), None), (None, 3)):
        D1, D2 = R.d1d2(m, 0, ex, rr, C)
        ref = R.weight_map(m, D1, D2, cwi, w0, sigma, C)
        assert (D2 != NO).any() and ((D2 == NO) & (D1 != NO)).any()
        got = BD.border_weight_map(guards.upload(m), None if cwi is None else torch.from_numpy(cwi), w0, sigma, ex, n_classes=C, objects=True,
                                   radius=radius)
        guards.check("weight map")
        assert got.is_cuda and got.dtype == torch.float32
        g = got.cpu().numpy()
        _close(g, ref)
        ok = (m >= 0) & (m < C)
        assert (g[~ok] == 0).all()
        base = (np.ones(C, dtype=np.float32) if cwi is None else cwi)[np.where(ok, m, 0)]
        assert (g[ok & (D2 == NO)] == base[ok & (D2 == NO)]).all()
        guards.checks.clear()
    u8 = R.blocky(rng, B, H, W, block=6, dtype=np.uint8)
    u8[B - 1] = 0                                                            # an image without an object: exactly the class weight
    cw = np.array([0.5, 1.5, 0.25, 2.0], dtype=np.float32)
    got = BD.border_weight_map(u8, cw, w0, sigma, objects=True, radius=radius)
    guards.check("uint8 NumPy input")
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and (got[B - 1] == cw[0]).all()
    D1, D2 = R.d1d2(u8, radius=rr, n_classes=C)
    _close(got, R.weight_map(u8, D1, D2, cw, w0, sigma, C))


def _smooth_pair(arch, n_in, n_out, size, dtype):
    """oracle + HIP network with the same weights; a smooth network (large BN shifts, small convs: no ReLU flips) as in the border test"""
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


def _ref_map(y, cw, b, C):
    D1, D2 = R.d1d2(y, b.background, b.exclude, R.default_radius(b.sigma) if b.radius is None else b.radius, C)
    return R.weight_map(y, D1, D2, cw, b.w0, b.sigma, C)


def _masks64(seed, B, n_classes, block=8):
    return torch.from_numpy(R.blocky(np.random.default_rng(seed), B, 64, 64, n_classes=n_classes, block=block, dtype=np.int64))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_step_with_object_border_loss(dtype):
    """forward + cross-entropy with the two-object map + backward of the whole network against the oracle network + the restated map, at
    the bars of test_training_step_with_border_loss; the generic torch path of the loss object gives the same number"""
    from unet_amd.learner import BorderWeightedCrossEntropy
    ref, model = _smooth_pair("xresnet18", 4, 3, (64, 64), dtype)
    x, _ = O.synthetic_batch(2, 4, 64, 64, 3)
    y = _masks64(5, 2, 3)
    cw = [0.5, 1.5, 1.0]
    b = BorderWeightedCrossEntropy(weight=torch.tensor(cw), w0=10.0, sigma=5.0, objects=True)
    ref.train(); model.train()
    out = ref(x)
    pw = torch.from_numpy(_ref_map(y.numpy(), cw, b, 3)).to(out.dtype)
    assert (pw > 2.0).any()                                                  # the gaps between objects carry the term
    nll = torch.nn.functional.cross_entropy(out, y, reduction="none")
    loss_ref = (pw * nll).sum() / pw.sum()
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
        first = loss.item()                                                  # the loss lives in a buffer that the next step overwrites
        plain = BorderWeightedCrossEntropy(weight=torch.tensor(cw), w0=10.0, sigma=5.0)
        other = model.forward_loss_backward(x.cuda(), y.cuda(), torch.tensor(cw, device="cuda"), border=plain).item()
        assert abs(other - first) > 1e-4 * abs(first), (other, first)        # the two forms are different losses on this batch


def test_hipgraph_step_with_object_border_loss_equals_eager():
    """TrainStep(use_graph=True) captures the step with objects=True (no host sync inside, the labelling's launches included): the two
    eager warm-up steps and three replays equal five eager steps bit for bit"""
    from unet_amd.learner import BorderWeightedCrossEntropy
    from unet_amd.model import HipDynamicUnet
    from unet_amd.optimizer import FlatAdam
    from unet_amd.trainer import TrainStep
    torch.manual_seed(11)
    sd = O.DynamicUnet("xresnet18", 4, 5, (64, 64)).state_dict()
    xs = [(O.synthetic_batch(2, 4, 64, 64, 5, seed=s)[0], _masks64(20 + s, 2, 5)) for s in range(5)]
    outs = []
    for use_graph in (False, True):
        model = HipDynamicUnet("xresnet18", 4, 5, (64, 64))
        model.load_state_dict(sd)
        model.train()
        model.ctx.wgrad_overlap = False
        opt = FlatAdam(model, [1e-4, 3e-4, 1e-3])
        step = TrainStep(model, opt, torch.tensor([0.3, 2.0, 1.0, 0.5, 1.7], device="cuda"), 1, use_graph=use_graph)
        step.border = BorderWeightedCrossEntropy(w0=6.0, sigma=3.0, exclude=4, objects=True)
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


def test_learner_fits_validates_exports_with_object_border_loss(tmp_path):
    """train.train_unet's sequence with loss_func=BorderWeightedCrossEntropy(objects=True): one epoch, valid_loss = the restated loss on the
    oracle network over the validation set, export / load_learner keep the loss and its numbers, lr_find runs through the fused step"""
    from unet_amd.learner import BorderWeightedCrossEntropy, DataLoaders, DiceMulti, Learner, TileDataset, load_learner
    from unet_amd.model import HipDynamicUnet
    g = np.random.default_rng(0)
    imgs = [g.integers(0, 255, (4, 64, 64)).astype(np.uint8) for _ in range(4)]
    masks = [R.blocky(g, 1, 64, 64, n_classes=3)[0] for _ in range(4)]
    torch.manual_seed(1)
    model = HipDynamicUnet("xresnet18", 4, 3, (64, 64))
    dls = DataLoaders(TileDataset(imgs, masks, "int8"), TileDataset(imgs[:3], masks[:3], "int8"), 2, vocab=list("abc"))
    loss = BorderWeightedCrossEntropy(axis=1, w0=4.0, sigma=2.5, objects=True, radius=12)
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
        pw = torch.from_numpy(_ref_map(ys.numpy(), cw, loss, 3))
        nll = torch.nn.functional.cross_entropy(ref(xs).double(), ys, reduction="none")
        want = ((pw * nll).sum() / pw.sum()).item()
    got = learn.validate()[0]
    print("valid_loss", got, want)
    assert abs(got - want) < 1e-4 * max(1.0, abs(want)), (got, want)
    learn.export(tmp_path / "objects.pkl")
    back = load_learner(tmp_path / "objects.pkl")
    d = back.loss_func
    assert type(d) is BorderWeightedCrossEntropy and (d.w0, d.sigma, d.exclude, d.objects, d.background, d.radius) == (4.0, 2.5, None, True, 0, 12)
    assert torch.allclose(torch.as_tensor(d.func.weight), torch.tensor(cw))
    assert torch.equal(back.model.flat_param, model.flat_param)
    before = model.flat_param.clone()
    learn.lr_find(start_lr=1e-6, end_lr=1e-3, num_it=6)
    lrs, losses = learn.lr_find_curve
    assert len(losses) == 6 and np.isfinite(losses).all()
    assert torch.equal(model.flat_param, before)          # lr_find restores the weights


def _spy(monkeypatch):
    from unet_amd import ops
    calls = []
    for name in _NEW_OPS:
        def wrapped(*a, _fn=getattr(ops, name), _name=name, **k):
            calls.append(_name)
            return _fn(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    return calls


def test_defaults_are_untouched(monkeypatch):
    """BorderWeightedCrossEntropy() and border_weight_map(...) without the new arguments give the bits of border_edt + border_weight and
    launch none of the new kernels; the step with the default loss gives the bits of the same launches made by hand"""
    from unet_amd import ops
    from unet_amd.learner import BorderWeightedCrossEntropy
    from unet_amd.model import HipDynamicUnet
    calls = _spy(monkeypatch)
    rng = np.random.default_rng(3)
    m = torch.from_numpy(BR.blocky(rng, 2, 37, 53, dtype=np.int64)).cuda()
    cw = torch.tensor([0.5, 1.5, 0.25, 2.0], device="cuda")
    for ex in (None, 0):
        d2 = torch.empty(m.shape, dtype=torch.int32, device="cuda")
        ops.border_edt(m, d2, torch.empty(ops.edt_workspace(2, 37, 53), dtype=torch.uint8, device="cuda"), ex)
        pw = torch.empty(m.shape, device="cuda")
        ops.border_weight(d2, m, cw, 4, 10.0, 5.0, pw)
        got = BD.border_weight_map(m, cw, exclude=ex)
        assert torch.equal(got.view(torch.int32), pw.view(torch.int32))
        assert torch.equal(BD.border_weight_map(m, cw, 10.0, 5.0, ex, 4, False, 0, None).view(torch.int32), pw.view(torch.int32))
    b = BorderWeightedCrossEntropy()
    assert (b.objects, b.background, b.radius) == (False, 0, None)
    torch.manual_seed(5)
    model = HipDynamicUnet("xresnet18", 4, 4, (64, 64))
    model.train()
    x, _ = O.synthetic_batch(2, 4, 64, 64, 4)
    xd, yd = x.cuda(), torch.from_numpy(BR.blocky(rng, 2, 64, 64, dtype=np.int64)).cuda()
    loss = model.forward_loss_backward(xd, yd, cw, border=b).clone()
    grad = model.flat_grad.clone()
    z = model._hip_forward(xd, True)
    d2 = torch.empty(yd.shape, dtype=torch.int32, device="cuda")
    ops.border_edt(yd, d2, torch.empty(ops.edt_workspace(2, 64, 64), dtype=torch.uint8, device="cuda"), None)
    pw = torch.empty(yd.numel(), device="cuda")
    ops.border_weight(d2, yd, cw, 4, 10.0, 5.0, pw)
    assert torch.equal(model.border_weights(yd, cw, b, 4).view(torch.int32), pw.view(torch.int32))
    dz = model.ctx.act(model, "dlogits", z.N, z.H, z.W, z.C, zero=True)
    lo, den = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    ops.ce_fwd_pw(z, yd, pw, lo, den, torch.empty(ops.ce_workspace(z.P), device="cuda"))
    ops.ce_bwd_pw(z, yd, pw, den, 1.0, dz)
    model._ensure_grad_views()
    model._hip_backward(dz)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and grad.abs().sum().item() > 0
    assert torch.equal(lo, loss)
    assert torch.equal(model.flat_grad, grad)
    assert torch.isfinite(b(torch.randn(2, 4, 64, 64, device="cuda"), yd))       # the generic path of the default loss
    assert calls == []
    BD.border_weight_map(m, cw, objects=True)                                # the spy does see the new path
    assert calls == ["object_border_weight"]


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
    y = torch.from_numpy(R.blocky(g, 2, 64, 64, n_classes=5, block=4 + 4 * rank, dtype=np.int64)).cuda()      # different gap densities
    w = torch.tensor([0.3, 2.0, 1.0, 0.5, 1.7], device="cuda")
    b = BorderWeightedCrossEntropy(w0=10.0, sigma=5.0, objects=True)
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


def test_object_border_two_ranks_one_gpu_gloo():
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
