"""GPU suite of the float statistics per object (csrc/object_values.hip, unet_amd/objects.py): the tables against the
restatement of the rules in NumPy and Python integers (tests/object_values_ref.py) on every tail length, alignment, object pattern and value
pattern; spans of several steps; fixed shifts; bad labels; the composition through zonal_values.  Every comparison is exact equality, the
extremes as bit patterns and the derived shift included.  Every buffer a kernel writes sits in a guard-banded allocation and every input
between canaries (the float canary is a finite -3e7, so a read outside a plane shows in the sums and in min); all of them are checked after
every launcher, and the inputs are compared unchanged afterwards.  (The entry points: tests/test_object_values_e2e_gpu.py.)"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

import object_values_ref as VR  # noqa: E402
import objects_cases as OC  # noqa: E402
import objects_ref as OR  # noqa: E402
from guard import canary_input, guarded  # noqa: E402

_FILL = {torch.uint8: 0xA5, torch.int32: -7, torch.int64: -7}
_LAUNCHERS = ("inst_marks", "vec_scan", "vec_read", "obj_compact", "obj_accumulate", "obj_point", "obj_absmax", "obj_values", "zonal_absmax",
              "zonal_values")
SHAPES = [(1, 1), (1, 3), (1, 4), (1, 5), (3, 15), (2, 16), (3, 17), (5, 63), (7, 257), (33, 300)]
SEQUENTIAL = 2000          # pixels up to which the sequential reference runs; beyond it its vectorised form (equal: test_object_values_cpu.py)
_INTS = ("valid", "sum_q", "sq_lo", "sq_hi")


def _ob():
    from unet_amd import objects
    return objects


class Guards:
    def __init__(self):
        self.checks, self.by_name = [], {}

    def alloc(self, shape, dtype, device):
        t, c = guarded(shape, dtype, device, _FILL[dtype])
        self.checks.append(c)
        return t

    def upload(self, a) -> torch.Tensor:
        t, c = canary_input(torch.from_numpy(np.ascontiguousarray(a)))
        self.checks.append(c)
        return t

    def check(self, what=""):
        for c in self.checks:
            c(what)

    def clear(self):
        self.check("end of case")
        self.checks.clear()


@pytest.fixture
def guards(monkeypatch):
    from unet_amd import ops, zonal
    g = Guards()
    monkeypatch.setattr(_ob(), "_alloc", g.alloc)
    monkeypatch.setattr(zonal, "_alloc", g.alloc)
    for name in _LAUNCHERS:
        def wrapped(*a, _fn=getattr(ops, name), _name=name, **k):
            r = _fn(*a, **k)
            g.by_name[_name] = g.by_name.get(_name, 0) + 1
            g.check(_name)
            return r
        monkeypatch.setattr(ops, name, wrapped)
    return g


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _reference(m, lab, v, exclude=(), nodata=None, shift=None):
    return (VR.tables if m.size <= SEQUENTIAL else VR.tables_fast)(m, lab, v, exclude, nodata, shift)


def _same(host, want, what):
    assert host.label.dtype == torch.int32 and host.label.tolist() == want["label"], (what, "label")
    for k in _INTS:
        assert getattr(host, k).dtype == torch.int64 and getattr(host, k).tolist() == want[k], (what, k)
    for k in ("min", "max"):
        assert getattr(host, k).dtype == torch.float32 and np.array_equal(_bits(getattr(host, k).numpy()), _bits(want[k])), (what, k)
    for k in ("argmin", "argmax"):
        assert getattr(host, k).dtype == torch.int32 and getattr(host, k).tolist() == want[k], (what, k)
    assert host.shift == want["shift"] and tuple(host.shape) == want["shape"], (what, "shift")


def _run(guards, m, lab, v, exclude=None, nodata=None, shift=None, planes=None):
    """object_values on guarded copies (or on the given device planes); the inputs come back unchanged; returns the host tables"""
    dm, dl, dv = planes if planes is not None else (guards.upload(m), guards.upload(lab), guards.upload(v))
    before = dict(guards.by_name)
    stats = _ob().object_values(dm, dv, dl, exclude, nodata, shift)
    assert guards.by_name.get("obj_absmax", 0) - before.get("obj_absmax", 0) == (1 if shift is None else 0)
    assert guards.by_name["obj_values"] - before.get("obj_values", 0) == 1
    assert guards.by_name.get("obj_accumulate", 0) == before.get("obj_accumulate", 0)          # the table of attributes is not measured again
    P = stats.n_objects
    for name in _INTS + ("label", "min", "max", "argmin", "argmax"):
        t = getattr(stats, name)
        assert t.is_cuda and tuple(t.shape) == (P,), name
    assert np.array_equal(dm.cpu().numpy(), m) and np.array_equal(dl.cpu().numpy(), lab) and np.array_equal(_bits(dv.cpu().numpy()), _bits(v))
    host = stats.cpu()
    guards.clear()
    return host


def _check(guards, m, lab, v, what, exclude=None, nodata=None, shift=None, planes=None):
    ex = () if exclude is None else ((exclude,) if isinstance(exclude, int) else tuple(exclude))
    want = _reference(m, lab, v, ex, nodata, shift)
    assert not want["bad"] and not want["overflow"], what
    host = _run(guards, m, lab, v, exclude, nodata, shift, planes)
    _same(host, want, what)
    assert sum(want["valid"]) == int(VR.valid_mask(m, v, ex, nodata).sum())
    return host


# ------------------------------------------------------------------------------------------------------------ patterns

def object_patterns(H, W, seed):
    """{name: (mask, labels, exclude)}: the patterns of objects_cases (components and hand-made instance labels), one-pixel objects, stripes
    one pixel wide, a single object, an excluded class between objects, everything excluded"""
    p = {k: (m, lab, None) for k, (m, lab) in OC.patterns(H, W, seed).items()}
    p["noise_excluded"] = (*OC.patterns(H, W, seed)["noise"], 1)                      # class 1 lies between the objects of 0 and 2
    p["blocks_excluded"] = (*OC.patterns(H, W, seed)["blocks"], (0, 2))
    p["none"] = (*OC.patterns(H, W, seed)["vstripes"], (0, 1, 2))                     # P = 0
    shapes = OC.placed((H, W), OC.ring(), (0, 0))                                       # a ring, and a U beside it where there is room
    p["shapes"] = (shapes | OC.placed((H, W), OC.u_shape(), (0, 12)) if W > 12 else shapes, None, 0)
    out = {}
    for name, (m, lab, ex) in p.items():
        m = np.ascontiguousarray(m, dtype=np.uint8)
        out[name] = (m, OC.R.label_components(m, 4) if lab is None else lab, ex)
    return out


def value_patterns(H, W, seed):
    """{name: (float32 [H, W], nodata, shift)}"""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    n = H * W
    noise = lambda s: (rng.standard_normal((H, W)) * s).astype(f32)  # noqa: E731
    p = {"constant": (np.full((H, W), 0.75, dtype=f32), None, None)}          # every pixel attains both extremes: the first one has them
    p["ramp"] = ((np.arange(n, dtype=np.float64) * 0.25 - n / 9).astype(f32).reshape(H, W), None, None)
    p["ramp_down"] = (-p["ramp"][0], None, None)
    plateau = np.clip(noise(1.0), -0.5, 0.5)                    # equal maxima and equal minima, many of each in every object
    p["plateau"] = (plateau, None, None)
    p["negzero"] = (np.where(rng.random((H, W)) < 0.5, f32(0.0), f32(-0.0)).astype(f32), None, None)
    p["mixed"] = (noise(40.0), None, None)
    p["denormal"] = ((rng.integers(-2 ** 20, 2 ** 20, (H, W)).astype(np.int64) * 2.0 ** -149).astype(f32), None, None)
    p["huge"] = ((rng.choice(np.array([3.0e38, -3.0e38, 2.9e38, 1.0, -2.5e38], dtype=f32), (H, W))), None, None)
    special = noise(50.0)
    for value in (np.nan, np.inf, -np.inf, -9999.0):
        special[rng.random((H, W)) < 0.08] = value
    special.reshape(-1)[:4] = np.array([np.nan, np.inf, -np.inf, -9999.0], dtype=f32)[:n]          # each of them at least once
    p["special"], p["special_nodata"] = (special, None, None), (special, -9999, None)
    half = rng.choice(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5, 0.0, 7.0], dtype=f32), (H, W))
    p["half"] = (half, None, 0)                                 # round half to even under an explicit shift
    return p


@pytest.mark.parametrize("shape", SHAPES)
def test_patterns_equal_the_reference_on_every_tail(guards, shape):
    H, W = shape
    values = value_patterns(H, W, seed=H * 1000 + W)
    assert np.isnan(values["special"][0]).any() and values["denormal"][0].dtype == np.float32
    names = sorted(values)
    objects = object_patterns(H, W, seed=W)
    assert {"one", "checker", "hstripes", "vstripes", "split", "noise", "none", "shapes", "noise_excluded"} <= set(objects)
    launches = 0
    for i, (oname, (m, lab, ex)) in enumerate(sorted(objects.items())):
        # every object pattern with the plateau, the specials under nodata and three more value patterns in rotation: all pairs over the shapes
        for vname in sorted({"plateau", "special_nodata", names[i % len(names)], names[(i + 4) % len(names)], names[(i + 7) % len(names)]}):
            v, nodata, shift = values[vname]
            host = _check(guards, m, lab, v, (shape, oname, vname), ex, nodata, shift)
            launches += 1
            if oname == "none":
                assert host.n_objects == 0
            if oname == "one":
                assert host.label.tolist() == [0]
                if vname in ("constant", "ramp_down"):
                    assert host.argmax.tolist() == [0]            # the smallest index among equal maxima / the first of a falling ramp
                if vname == "ramp":
                    assert host.argmax.tolist() == [H * W - 1] and host.argmin.tolist() == [0]
            if vname == "negzero":
                has = (host.valid > 0).numpy()
                mn, mx = host.min.numpy()[has], host.max.numpy()[has]
                assert ((mn == 0) & (mx == 0)).all()
    assert guards.by_name["obj_values"] == launches


def test_extremes_ties_signed_zeros_and_objects_without_a_valid_pixel(guards):
    H, W = 9, 23
    m = OC.placed((H, W), OC.ring(), (0, 0)) | OC.placed((H, W), OC.u_shape(), (0, 12))
    lab = OC.R.label_components(m, 4)
    ring, u = int(lab[1, 1]), int(lab[1, 13])
    v = np.full((H, W), 1.0, dtype=np.float32)
    v[2, 5] = v[7, 3] = v[5, 1] = 8.0                            # a plateau of three maxima in the ring: the peak is the first
    v[4, 2] = v[6, 9] = -3.0                                    # two equal minima
    v[m == 2] = np.nan                                          # the U has no valid pixel
    v[0, 0] = 99.0                                              # the background is excluded: its values count nowhere
    host = _check(guards, m, lab, v, "ties", exclude=0)
    assert host.label.tolist() == [ring, u] and host.shift == 30 - 4
    assert host.argmax.tolist() == [2 * W + 5, -1] and host.argmin.tolist() == [4 * W + 2, -1]
    assert host.valid.tolist() == [int((m == 1).sum()), 0] and float(host.min[1]) == np.inf and float(host.max[1]) == -np.inf
    rows = _ob().object_value_rows(host, (100.0, 2.0, 0.0, 50.0, 0.0, -2.0), "h")
    assert rows == VR.rows(_reference(m, lab, v, (0,)), (100.0, 2.0, 0.0, 50.0, 0.0, -2.0), "h")
    assert rows[0]["h_peak_x"] == 100.0 + 5.5 * 2.0 and rows[0]["h_peak_y"] == 50.0 - 2.5 * 2.0 and set(rows[1].values()) == {None}
    # +0.0 and -0.0 in one object: min is -0.0 at its first place, max +0.0 at its first place
    z = np.zeros((H, W), dtype=np.float32)
    z[m == 1] = -0.0
    z[3, 1] = z[5, 9] = 0.0
    host = _check(guards, m, lab, z, "zeros", exclude=(0, 2))
    assert np.signbit(host.min.numpy()[0]) and not np.signbit(host.max.numpy()[0])
    assert host.argmax.tolist() == [3 * W + 1] and host.argmin.tolist() == [ring] and host.shift == 30
    # nodata: all of the ring's pixels but one
    v = np.full((H, W), -9999.0, dtype=np.float32)
    v[6, 2] = 12.5
    host = _check(guards, m, lab, v, "nodata", exclude=0, nodata=-9999)
    assert host.valid.tolist() == [1, 0] and host.argmax.tolist() == [6 * W + 2, -1] == host.argmin.tolist()
    assert _check(guards, m, lab, v, "no nodata", exclude=0).valid.tolist() == [int((m == 1).sum()), int((m == 2).sum())]


def test_instance_labels_and_labels_none(guards):
    from unet_amd import instances as I
    m = OC.two_blobs()
    d = torch.from_numpy(m).cuda()
    labels = I.split_instances(d, classes=[1], radius=16, min_depth=1.0)[0].cpu().numpy()
    yy, xx = np.mgrid[0:m.shape[0], 0:m.shape[1]]
    v = (20.0 - np.hypot(yy - 20, xx - 20) * 0.5).astype(np.float32)          # a peak in the left disc
    host = _check(guards, m, labels, v, "instances", exclude=0)
    assert host.n_objects == 2 and 20 * m.shape[1] + 20 in host.argmax.tolist()
    # labels None are the components; host inputs are uploaded
    stats = _ob().object_values(m, v, None, 0)
    _same(stats.cpu(), _reference(m, OC.R.label_components(m, 4), v, (0,)), "components")
    assert stats.n_objects == 1 and stats.valid.is_cuda
    guards.clear()


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_planes_at_addresses_that_are_only_element_aligned(guards, offset):
    # views that start `offset` elements into guarded allocations: no wide access is possible on that plane, and none may touch the bands
    onames = ["noise", "blocks", "vstripes", "split", "hstripes", "one", "checker", "noise_excluded", "shapes", "noise"]
    vnames = ["special_nodata", "plateau", "ramp", "special", "half", "denormal", "huge", "negzero", "mixed", "special_nodata"]
    for i, (H, W) in enumerate(SHAPES):
        m, lab, ex = object_patterns(H, W, seed=offset)[onames[i]]
        v, nodata, shift = value_patterns(H, W, seed=offset)[vnames[i]]
        n = H * W
        off = {}
        for key, a in (("m", m), ("l", lab), ("v", v)):
            flat = guards.upload(np.concatenate([np.full(offset, a.reshape(-1)[0], a.dtype), a.reshape(-1)]))
            off[key] = flat[offset:offset + n].view(H, W)
        assert off["l"].data_ptr() % 16 != 0 and off["v"].data_ptr() % 16 != 0 and off["m"].data_ptr() % 4 != 0 and off["l"].is_contiguous()
        _check(guards, m, lab, v, (H, W, "labels off"), ex, nodata, shift, planes=(guards.upload(m), off["l"], guards.upload(v)))
        _check(guards, m, lab, v, (H, W, "values off"), ex, nodata, shift, planes=(guards.upload(m), guards.upload(lab), off["v"]))
        _check(guards, m, lab, v, (H, W, "mask off"), ex, nodata, shift, planes=(off["m"], guards.upload(lab), guards.upload(v)))
        _check(guards, m, lab, v, (H, W, "all off"), ex, nodata, shift, planes=(off["m"], off["l"], off["v"]))


@pytest.mark.parametrize("pattern", ["one", "stripes", "carry"])
def test_spans_of_several_steps_per_wavefront(guards, pattern):
    # The launcher's grid rule: at most 1024 workgroups of 4 wavefronts, a span a multiple of 128 groups of 4 pixels.  3.15 M pixels are 787 k
    # groups over 4096 wavefronts: 193 groups each, a span of 256 groups = four steps of 256 pixels per wavefront, so the pending record is
    # carried from step to step, flushed where the key changes inside a span and at its end
    H, W = 1537, 2049
    groups = (H * W + 3) // 4
    assert groups > 1024 * 256 and -(-groups // 4096) > 2 * 64 and (-(-groups // 4096) + 127) // 128 * 128 >= 3 * 64
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    if pattern == "one":
        m, lab = np.full((H, W), 2, dtype=np.uint8), np.zeros((H, W), dtype=np.int32)
    elif pattern == "stripes":                                  # rows of 300 form one object: 600 k pixels each, wider than a span
        m = ((yy // 300) % 3).astype(np.uint8)
        lab = ((yy // 300) * 300 * W).astype(np.int32)
    else:
        m, lab = OC.carry_case(H, W)
    v = (rng.standard_normal((H, W)) * 3.0 + 20.0).astype(np.float32)
    v[rng.random((H, W)) < 0.001] = np.nan
    v[700:720] = -9999.0
    v[100:120] = 0.125                                          # a span of one constant
    v[1000, 1000] = v[1200, 17] = 63.5                          # two equal maxima far apart, in different spans
    exclude = 1 if pattern == "stripes" else None
    host = _check(guards, m, lab, v, pattern, exclude, nodata=-9999)
    assert host.shift == 24
    if pattern == "one":
        assert host.argmax.tolist() == [1000 * W + 1000] and host.argmin.tolist() == [100 * W]
        ok = np.isfinite(v) & (v != -9999.0)
        assert int(host.valid[0]) == int(ok.sum())
        # the mean against float64 within the derived bound: E = 6 here (A in 32 .. 64), so 2^-25, plus float64 rounding
        mean = _ob().object_value_rows(host)[0]["value_mean"]
        assert abs(mean - v[ok].astype(np.float64).mean()) <= 2.0 ** -25 + 32 * np.spacing(64.0)
    for _ in range(2):                                          # two more runs of one input are equal
        again = _run(guards, m, lab, v, exclude, -9999)
        for k in _INTS + ("argmin", "argmax"):
            assert torch.equal(getattr(again, k), getattr(host, k)), k
        assert np.array_equal(_bits(again.max.numpy()), _bits(host.max.numpy())) and np.array_equal(_bits(again.min.numpy()), _bits(host.min.numpy()))


# ------------------------------------------------------------------------------------------------------------ shifts

def test_derived_and_fixed_shifts(guards):
    H, W = 7, 257
    m, lab, _ = object_patterns(H, W, seed=3)["blocks"]
    values = value_patterns(H, W, seed=3)
    for name, s in {"constant": 30, "negzero": 30, "half": 0}.items():
        v, nodata, shift = values[name]
        assert _check(guards, m, lab, v, name, None, nodata, shift).shift == s, name
    assert _check(guards, m, lab, values["denormal"][0], "denormal").shift >= 30 + 126 + 3          # denormals are not flushed: E <= -129
    assert _check(guards, m, lab, values["huge"][0], "huge").shift == 30 - 128
    v = values["mixed"][0].copy()
    v[np.abs(v) > 4.0] = 1.0
    v[3, 100] = 5.0                                             # E = 3: the derived shift is 27
    assert _check(guards, m, lab, v, "derived").shift == 27
    # the largest magnitude lies in an excluded class: it does not count
    big = v.copy()
    big[m == 0] = 1000.0
    assert m[3, 100] != 0 and _check(guards, m, lab, big, "excluded", exclude=0).shift == 27
    whole = _check(guards, m, lab, v, "smaller", shift=20)
    # tables of one shift add up over a split of the plane into two rasters of whole rows (blocks are two rows high)
    top, bottom = _check(guards, m[:4], lab[:4], v[:4], "top", shift=20), _check(guards, m[4:], lab[4:] - 4 * W, v[4:], "bottom", shift=20)
    assert sum(top.valid.tolist()) + sum(bottom.valid.tolist()) == sum(whole.valid.tolist())
    assert sum(top.sum_q.tolist()) + sum(bottom.sum_q.tolist()) == sum(whole.sum_q.tolist())


def test_a_shift_too_large_for_the_data_raises(guards):
    from unet_amd import ops
    OB = _ob()
    H, W = 7, 257
    m, lab, _ = object_patterns(H, W, seed=3)["blocks"]
    v = np.clip(value_patterns(H, W, seed=3)["mixed"][0], -4.0, 4.0)
    v[3, 100] = 5.0
    dm, dl, dv = guards.upload(m), guards.upload(lab), guards.upload(v)
    with pytest.raises(ValueError, match="shift=28 is too large"):
        OB.object_values(dm, dv, dl, shift=28)
    guards.check("raise")
    want = VR.tables(m, lab, v, shift=28)
    assert want["overflow"] and not want["bad"]
    offs, P, label, _ = OB._object_index(dm, dl, ())
    table, word = guards.alloc((6, P), torch.int64, "cuda"), guards.alloc((1,), torch.int64, "cuda")
    ops.obj_values(dm, dl, dv, offs, (), P, None, 28, table, word)
    assert int(word.cpu()[0]) == 8
    _same(OB.ObjectValues.of_table(label, table, 28, (H, W)).cpu(), want, "overflow")          # such a pixel is left out of every table
    # an exact power of two at |q| = 2^30 is no overflow
    v[3, 100] = 4.0
    k = want["label"].index(int(lab[3, 100]))
    assert int(_check(guards, m, lab, v, "2^30", shift=28).sq_hi[k]) >= 2 ** 30               # q^2 = 2^60 = 2^30 * 2^30 + 0
    guards.clear()


# ------------------------------------------------------------------------------------------------------------ existing code

@pytest.mark.parametrize("pattern", ["noise", "blocks_excluded", "split"])
def test_the_dense_id_composition_through_zonal_values_gives_equal_tables(guards, pattern):
    from unet_amd import zonal
    H, W = 33, 300
    m, lab, ex = object_patterns(H, W, seed=8)[pattern]
    v, nodata, _ = value_patterns(H, W, seed=8)["special_nodata"]
    host = _check(guards, m, lab, v, pattern, ex, nodata)
    P = host.n_objects
    dm, dl, dv = guards.upload(m), guards.upload(lab), guards.upload(v)
    excl = () if ex is None else ((ex,) if isinstance(ex, int) else ex)
    offs = _ob()._object_index(dm, dl, excl)[0]
    ids = offs.view(-1)[dl.view(-1).long()].view(H, W)
    kept = torch.ones(256, dtype=torch.bool)
    kept[list(excl)] = False
    ids = torch.where(kept.cuda()[dm.long()], ids, torch.full_like(ids, -1)).contiguous()
    z = zonal.zonal_values(ids, dv, P, nodata, host.shift).cpu()
    for k in _INTS:
        assert torch.equal(getattr(z, k), getattr(host, k)), k
    assert np.array_equal(_bits(z.min.numpy()), _bits(host.min.numpy())) and np.array_equal(_bits(z.max.numpy()), _bits(host.max.numpy()))
    t = OR.table(m, lab, ex)
    assert z.pixels.tolist() == t["pixels"].tolist() and host.label.tolist() == t["label"].tolist()          # the objects of measure_objects
    guards.clear()


# ------------------------------------------------------------------------------------------------------------ bad input

def test_bad_labels_raise_and_store_nothing_outside_the_tables(guards):
    from unet_amd import ops
    OB = _ob()
    launches = 0
    for H, W in ((3, 17), (33, 300)):
        m, lab = OC.patterns(H, W, seed=5)["blocks"]
        v = value_patterns(H, W, seed=5)["mixed"][0]
        n = H * W
        for what, plane, at, value, text, bit in (("beyond the raster", "lab", n // 2, n, "outside 0", 1), ("far beyond", "lab", n - 1, 2 ** 31 - 1, "outside 0", 1),
                                                  ("negative", "lab", 0, -5, "outside 0", 1), ("not canonical", "lab", n - 1, 1, "not canonical", 2),
                                                  ("a chain", "lab", 3, 2 * W + 3, "not canonical", 2), ("class of the anchor", "m", 1, 9, "class differs", 4)):
            mm, ll = m.copy(), lab.copy()
            (ll if plane == "lab" else mm).reshape(-1)[at] = value
            assert OR.bad_bits(mm, ll), what
            dm, dl, dv = guards.upload(mm), guards.upload(ll), guards.upload(v)
            with pytest.raises(ValueError) as ours:
                OB.object_values(dm, dv, dl)
            with pytest.raises(ValueError) as theirs:
                OB.measure_objects(dm, dl)
            assert text in str(ours.value) and str(ours.value).replace("object_values", "measure_objects") == str(theirs.value), what
            guards.check(what)
            with pytest.raises(ValueError, match=text):
                OB.object_values(dm, dv, dl, exclude=(0, 1, 2, 3), shift=10)                  # with no object kept the planes are still checked
            # the tables of all other pixels are those of the reference
            want = VR.tables(mm, ll, v, shift=20)
            assert want["bad"] & bit and not want["bad"] & 8, what                          # (a broken anchor breaks its object's other pixels too)
            offs, P, label, _ = OB._object_index(dm, dl, ())
            table, word = guards.alloc((6, P), torch.int64, "cuda"), guards.alloc((1,), torch.int64, "cuda")
            ops.obj_values(dm, dl, dv, offs, (), P, None, 20, table, word)
            assert int(word.cpu()[0]) == want["bad"], what
            _same(OB.ObjectValues.of_table(label, table, 20, (H, W)).cpu(), want, what)
            assert np.array_equal(dm.cpu().numpy(), mm) and np.array_equal(dl.cpu().numpy(), ll)
            guards.clear()
            launches += 3
    assert guards.by_name["obj_values"] == launches


def test_arguments_are_refused_before_any_launch(guards):
    OB = _ob()
    m, lab = OC.patterns(3, 17, seed=1)["blocks"]
    v = np.ones((3, 17), dtype=np.float32)
    for kw, text in ((dict(values=v.astype(np.float64)), "float32"), (dict(values=v[:2]), "has shape"), (dict(labels=lab.astype(np.int64)), "int32"),
                     (dict(nodata="x"), "nodata"), (dict(nodata=float("nan")), "nodata"), (dict(shift=179), "shift"), (dict(shift=1.0), "shift"),
                     (dict(exclude=256), "exclude")):
        args = dict(mask=m, values=v, labels=lab)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            OB.object_values(**args)
    assert not guards.by_name
