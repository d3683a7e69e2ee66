"""Host side of the two-object border weight: the NumPy restatement (tests/object_border_ref.py) against a second, independent brute
force in plain Python, the argument checks that need no device, the loss object's pickle and export compatibility and the C ABI's new
symbols."""
import pickle
from collections import deque

import numpy as np
import pytest
import torch

import object_border_ref as R
from unet_amd import border as BD
from unet_amd.learner import BorderWeightedCrossEntropy, _loss_from_meta


def _brute(img, background, exclude, radius, n_classes):
    """(D1, D2) of one image by flood fill and a loop over every pair of a background pixel and an object pixel"""
    H, W = img.shape
    hi = 256 if n_classes is None else n_classes
    kind = [["x" if (v < 0 or v >= hi or v == exclude) else "b" if v == background else "o" for v in row] for row in img.tolist()]
    lab = [[-1] * W for _ in range(H)]
    n = 0
    for y in range(H):
        for x in range(W):
            if kind[y][x] != "o" or lab[y][x] >= 0:
                continue
            lab[y][x] = n
            todo = deque([(y, x)])
            while todo:
                cy, cx = todo.popleft()
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < H and 0 <= nx < W and kind[ny][nx] == "o" and lab[ny][nx] < 0 and img[ny, nx] == img[cy, cx]:
                        lab[ny][nx] = n
                        todo.append((ny, nx))
            n += 1
    objs = [(y, x, lab[y][x]) for y in range(H) for x in range(W) if lab[y][x] >= 0]
    D1 = np.full((H, W), R.NO_OBJECT, dtype=np.int32)
    D2 = D1.copy()
    for y in range(H):
        for x in range(W):
            if kind[y][x] != "b":
                continue
            best = {}
            for qy, qx, l in objs:
                d = (y - qy) ** 2 + (x - qx) ** 2
                if d <= radius * radius and d < best.get(l, 1 << 40):
                    best[l] = d
            s = sorted(best.values())
            if s:
                D1[y, x] = s[0]
            if len(s) > 1:
                D2[y, x] = s[1]
    return D1, D2


@pytest.mark.parametrize("radius", [1, 3, 7, 30])
def test_reference_agrees_with_a_plain_brute_force(radius):
    rng = np.random.default_rng(radius)
    masks = [R.blocky(rng, 2, 13, 17, block=3), R.salt(rng, 2, 11, 19, density=0.2), R.blocky(rng, 1, 1, 23, block=2), R.blocky(rng, 1, 23, 1, block=2),
             np.zeros((1, 5, 5), dtype=np.uint8), np.ones((1, 5, 5), dtype=np.uint8)]
    m = R.blocky(rng, 1, 12, 12, n_classes=6, block=2).astype(np.int64)
    m[0, 3, :] = -100
    masks.append(m)
    for m in masks:
        for bgv, ex, nc in ((0, None, None), (0, 2, None), (1, 0, 4), (0, None, 3)):
            D1, D2 = R.d1d2(m, bgv, ex, radius, nc)
            assert D1.dtype == np.int32 and D2.dtype == np.int32
            for b in range(m.shape[0]):
                w1, w2 = _brute(m[b].astype(np.int64), bgv, ex, radius, nc)
                assert np.array_equal(D1[b], w1) and np.array_equal(D2[b], w2), (m[b], bgv, ex, nc, radius)


def test_hand_cases():
    m = np.zeros((1, 5, 9), dtype=np.uint8)
    m[0, 2, 1] = 1
    m[0, 2, 7] = 1                                                   # two objects of one class, 6 px apart
    D1, D2 = R.d1d2(m, radius=5)
    assert (D1[0, 2, 4], D2[0, 2, 4]) == (9, 9)                      # equal distances: D2 == D1
    assert (D1[0, 2, 2], D2[0, 2, 2]) == (1, 25)                     # the farther one at exactly radius^2
    assert (D1[0, 2, 0], D2[0, 2, 0]) == (1, R.NO_OBJECT)            # 7 px away: outside the radius
    assert D1[0, 2, 1] == R.NO_OBJECT and D2[0, 2, 1] == R.NO_OBJECT  # an object pixel
    w = R.weight_map(m, D1, D2, [1.0, 3.0], 10.0, 5.0, 2)
    assert w[0, 2, 0] == 1.0 and w[0, 2, 1] == 3.0 and w[0, 2, 4] == 1.0 + 10.0 * np.exp(-36.0 / 50.0)
    m[0, 2, 2:7] = 1                                                 # joined: one object
    D1, D2 = R.d1d2(m, radius=5)
    assert (D2 == R.NO_OBJECT).all() and D1[0, 1, 4] == 1
    m[0, 2, 4] = 2                                                   # another class in between: three objects
    D1, D2 = R.d1d2(m, radius=5)
    assert (D1[0, 1, 4], D2[0, 1, 4]) == (1, 2)
    D1, D2 = R.d1d2(m, radius=5, exclude=2)                          # excluded: transparent, no term, and it does not join its neighbours
    assert (D1[0, 1, 4], D2[0, 1, 4]) == (2, 2) and D1[0, 2, 4] == R.NO_OBJECT
    assert BD.NO_OBJECT == R.NO_OBJECT and R.default_radius(5.0) == 30 and R.default_radius(3.3) == 20


_M = np.zeros((1, 4, 4), dtype=np.uint8)


@pytest.mark.parametrize("kw", [{"radius": 0}, {"radius": 256}, {"radius": 2.5}, {"radius": True}, {"background": -1}, {"background": 256},
                                {"background": 1.0}, {"sigma": 50.0}, {"exclude": 0}, {"objects": 1}])
def test_bad_arguments_are_refused_before_any_launch(kw):
    """radius outside 1 ... 255, sigma = 50 with radius=None (ceil(6 sigma) = 300), a background that is no class id or equals exclude"""
    with pytest.raises(ValueError):
        BorderWeightedCrossEntropy(**{"objects": True, **kw})
    with pytest.raises(ValueError):
        BD.border_weight_map(_M, n_classes=2, **{"objects": True, **kw})
    if "sigma" not in kw and "objects" not in kw:
        with pytest.raises(ValueError):
            BD.distance_to_objects(_M, **kw)


def test_more_argument_checks():
    with pytest.raises(ValueError, match="explicit radius"):
        BorderWeightedCrossEntropy(sigma=50.0, objects=True)
    assert BorderWeightedCrossEntropy(sigma=50.0, objects=True, radius=255).radius == 255
    assert BorderWeightedCrossEntropy(sigma=42.5, objects=True).radius is None           # ceil(255.0) = 255
    assert BorderWeightedCrossEntropy(sigma=50.0).objects is False                       # the cap concerns objects=True alone
    with pytest.raises(ValueError):
        BorderWeightedCrossEntropy(radius=0)                                             # checked even where it is unused
    with pytest.raises(ValueError):
        BD.distance_to_objects(_M, radius=None)
    for nc in (0, 257, 2.0):
        with pytest.raises(ValueError):
            BD.distance_to_objects(_M, n_classes=nc)
    with pytest.raises(ValueError):
        BD.border_weight_map(_M, n_classes=300, objects=True)
    for shape in [(1, 1, 8193), (0, 4, 4), (4,), (40000, 300, 300)]:
        with pytest.raises(ValueError):
            BD.distance_to_objects(np.broadcast_to(np.zeros((), dtype=np.uint8), shape))
    with pytest.raises(ValueError):
        BD.distance_to_objects(np.zeros((1, 4, 4), dtype=np.float32))
    assert BD.object_radius(5.0) == 30 and BD.object_radius(3.3) == 20 and BD.object_radius(0.01) == 1 and BD.object_radius(5.0, 7) == 7


def test_an_old_pickle_loads_as_objects_false():
    """a loss pickled before the new arguments existed has none of the new attributes: it reads them as objects=False, background 0, radius
    None; a new one keeps its own; export metadata without the keys loads as before"""
    new = BorderWeightedCrossEntropy(w0=3.0, sigma=2.0, exclude=1, objects=True, background=0, radius=9)
    back = pickle.loads(pickle.dumps(new))
    assert (back.objects, back.background, back.radius, back.w0, back.sigma, back.exclude) == (True, 0, 9, 3.0, 2.0, 1)
    old = BorderWeightedCrossEntropy(w0=3.0, sigma=2.0, exclude=0)
    for k in ("objects", "background", "radius"):
        del old.__dict__[k]                                          # the instance dictionary of the earlier class
    back = pickle.loads(pickle.dumps(old))
    assert "objects" not in back.__dict__
    assert (back.objects, back.background, back.radius) == (False, 0, None) and (back.w0, back.sigma, back.exclude) == (3.0, 2.0, 0)
    meta = {"class_weights": None, "focal_gamma": None, "regression": None, "border": {"w0": 3.0, "sigma": 2.0, "exclude": 0}}
    d = _loss_from_meta(meta)
    assert type(d) is BorderWeightedCrossEntropy and (d.objects, d.background, d.radius) == (False, 0, None)
    meta["border"].update(objects=True, background=2, radius=None)
    d = _loss_from_meta(meta)
    assert (d.objects, d.background, d.radius, d.exclude) == (True, 2, None, 0)


def test_new_symbols_are_in_the_library():
    from unet_amd import _lib as L
    from unet_amd import ops
    want = {"unet_object_edt_workspace", "unet_object_edt"}
    assert want <= set(L.declared_symbols())
    for s in want:
        assert hasattr(L.lib, s), s
    n = 16 * 512 * 512
    assert L.lib.unet_object_edt_workspace(16, 512, 512) == 18 * n + 16 == ops.object_edt_workspace(16, 512, 512)
    assert L.lib.unet_object_edt_workspace(1, 8193, 1) == 0 and L.lib.unet_object_edt_workspace(64, 8192, 8192) == 0
    p = 4096                                                         # a non-null, aligned address that is never dereferenced
    bad = [(p, 0, 1, 8193, 4, 0, -1, 4, 30, p, p, p, None, 1.0, 1.0, p, None), (p, 0, 1, 4, 4, 0, 0, 4, 30, p, p, p, None, 1.0, 1.0, p, None),
           (p, 0, 1, 4, 4, 0, -1, 4, 0, p, p, p, None, 1.0, 1.0, p, None), (p, 0, 1, 4, 4, 0, -1, 4, 256, p, p, p, None, 1.0, 1.0, p, None),
           (p, 0, 1, 4, 4, 0, -1, 257, 30, p, p, p, None, 1.0, 1.0, p, None), (p, 0, 1, 4, 4, -1, -1, 4, 30, p, p, p, None, 1.0, 1.0, p, None),
           (p, 0, 1, 4, 4, 0, -1, 4, 30, p + 4, p, p, None, 1.0, 1.0, p, None), (p, 0, 1, 4, 4, 0, -1, 4, 30, p, p, None, None, 1.0, 1.0, p, None),
           (p, 0, 1, 4, 4, 0, -1, 4, 30, p, None, None, None, 1.0, 1.0, None, None), (p, 0, 1, 4, 4, 0, -1, 4, 30, p, None, None, None, 1.0, 0.0, p, None)]
    for a in bad:
        assert L.lib.unet_object_edt(*a) != 0 and b"object_edt" in L.lib.unet_last_error(), a
