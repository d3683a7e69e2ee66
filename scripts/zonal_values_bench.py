"""Cost of the zonal statistics of a float plane (unet_amd/zonal.py zonal_values, csrc/zonal_values.hip) on a 20000 x 20000 plane.
usage: python scripts/zonal_values_bench.py [side=20000] [reps=5]
Prints one JSON line per measurement and writes them to profiles/zonal_values_bench.json.
The workload is that of scripts/zonal_bench.py with a float32 plane in place of the mask: the fixed-seed synthetic 5-class mask, raw and after
PostProcess(majority=5, sieve=64), gives three zone sets -- (a) a 10 x 10 grid of square zones, (b) the cleaned mask's own polygons, (c) the raw
mask's polygons (2 % salt: hardly any wavefront with one zone) --, and the value plane is 20 + 5 * normal noise with 1 % nodata (-9999) and a
sprinkle of NaN.  Per set, the median of `reps` samples (least and largest beside it) after two warm-up calls; a sample is a run of back-to-back calls of
about 0.3 s that ends in a device synchronise:
  copy       a float32 copy of one plane in the same run: the rate the shares below refer to
  absmax     ops.zonal_absmax alone; it must read 8 bytes per pixel (3.2 GB at 20000^2)
  values     ops.zonal_values alone (initialisation, the pass, the decoding of min and max); the same 8 bytes per pixel
  module     zonal.zonal_values with a derived shift: both passes and the two host reads
  baseline   the composition a user would write in the same process: index_add_ of float64 values and squares keyed by zone, bincount, and
             scatter_reduce_ amin / amax, over the valid pixels; and whether the means agree within the derived bound 2^(E-31) plus the
             float64 rounding of the baseline's own atomic sum (n eps A at worst, stated in the record)
No hardware counters are taken here: what limits the kernel is not measured by this script."""
import json
import math
import os
import sys
import time
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, HERE)
import torch  # noqa: E402

OUT = os.path.join(HERE, "..", "profiles", "zonal_values_bench.json")
RESULTS = []
NODATA = -9999.0


def emit(rec):
    """print the record and rewrite the file, so that a run that ends early leaves what it measured"""
    from unet_amd.build import source_hash
    RESULTS.append(rec)
    print(json.dumps(rec), flush=True)
    doc = {}
    if os.path.exists(OUT):          # records that other commands put beside these (the end-to-end series) stay
        with open(OUT) as f:
            doc = json.load(f)
    doc.update({"device": torch.cuda.get_device_name(0), "results": RESULTS, "kernel_source_hash": source_hash(),
                "command": "python scripts/zonal_values_bench.py " + " ".join(sys.argv[1:])})
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


WINDOW_S = 0.3          # every sample times at least this much work


def timed(fn, reps, warm=2):
    """(Timing: median, least and largest milliseconds per call and the calls per sample; the last result) over `reps` samples; a sample is a
    run of back-to-back calls that ends in a device synchronise and lasts about WINDOW_S, its length taken from the last warm-up call"""
    for _ in range(warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        once = time.perf_counter() - t0
    calls = max(1, min(1000, math.ceil(WINDOW_S / max(once, 1e-6))))
    samples = []
    for _ in range(reps):
        out = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            out = fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) * 1e3 / calls)
    samples.sort()
    return Timing(samples[len(samples) // 2], samples[0], samples[-1], calls), out


class Timing(NamedTuple):
    ms: float
    least: float
    largest: float
    calls: int

    def record(self) -> dict:
        return {"ms": round(self.ms, 3), "ms_least": round(self.least, 3), "ms_largest": round(self.largest, 3), "calls_per_sample": self.calls}


def rate(nbytes: int, t: Timing, copy_tbs: float) -> dict:
    tbs = nbytes / (t.ms * 1e-3) / 1e12
    return {**t.record(), "bytes_read": nbytes, "TB_per_s": round(tbs, 3), "share_of_copy_rate": round(tbs / copy_tbs, 3)}


def value_plane(side: int) -> torch.Tensor:
    g = torch.Generator(device="cuda").manual_seed(7)
    v = torch.randn((side, side), generator=g, device="cuda") * 5.0 + 20.0
    u = torch.rand((side, side), generator=g, device="cuda")
    v[u < 0.01] = NODATA
    v[u > 0.9999] = float("nan")
    return v


def one_set(name, rings, values, reps, copy_tbs):
    from unet_amd import ops
    from unet_amd import zonal as ZN
    n, Z = values.numel(), rings.n_features
    torch.cuda.empty_cache()
    ids = ZN.rasterize_ids(rings, values.shape)
    word = torch.zeros(2, dtype=torch.int64, device="cuda")
    table = torch.empty((6, Z), dtype=torch.int64, device="cuda")
    absmax_ms, _ = timed(lambda: ops.zonal_absmax(ids, values, Z, NODATA, word[0:1]), reps)
    shift = ZN.shift_of_absmax(int(word[0]))
    values_ms, _ = timed(lambda: ops.zonal_values(ids, values, Z, NODATA, shift, table[:5], table[5].view(torch.float32).view(2, Z), word[1:2]), reps)
    module_ms, stats = timed(lambda: ZN.zonal_values(ids, values, Z, NODATA), reps)
    assert int(word[1]) == 0 and stats.shift == shift and torch.equal(stats.table, table)

    def baseline():
        ok = (ids >= 0) & torch.isfinite(values) & (values != NODATA)
        key, x = ids[ok].long(), values[ok].double()
        s = torch.zeros(Z, dtype=torch.float64, device="cuda").index_add_(0, key, x)
        sq = torch.zeros(Z, dtype=torch.float64, device="cuda").index_add_(0, key, x * x)
        cnt = torch.bincount(key, minlength=Z)
        lo = torch.full((Z,), float("inf"), dtype=torch.float64, device="cuda").scatter_reduce_(0, key, x, "amin")
        hi = torch.full((Z,), float("-inf"), dtype=torch.float64, device="cuda").scatter_reduce_(0, key, x, "amax")
        return s, sq, cnt, lo, hi

    base_ms, (s, sq, cnt, lo, hi) = timed(baseline, 1, warm=1)          # seconds per call: one sample behind one warm-up
    host = stats.cpu()
    cnt, s, lo, hi = cnt.cpu(), s.cpu(), lo.cpu(), hi.cpu()
    E = 30 - shift
    A = 2.0 ** E
    has = host.valid > 0
    # vectorised over up to millions of zones: sum_q / valid in float64 (|sum_q| < 2^53 here) adds two roundings to zonal_value_rows' mean
    mean = torch.ldexp(host.sum_q[has].double() / host.valid[has].double(), torch.tensor(-shift))
    diff = (mean - s[has] / cnt[has].double()).abs()
    allowed = 2.0 ** (E - 31) + (cnt[has].double() + 4) * 2.0 ** -53 * A          # the fixed-point bound + the worst case of the float64 atomic sum
    agree = bool(torch.equal(host.valid, cnt)) and bool((diff <= allowed).all())
    k = int((diff - allowed).argmax())
    worst, worst_allowed, checked = float(diff[k]), float(allowed[k]), int(has.sum())
    assert ZN.zonal_value_rows(ZN.ZonalValues(*(t[:100] for t in (host.pixels, host.valid, host.sum_q, host.sq_lo, host.sq_hi, host.min, host.max)), shift))
    extremes = bool(torch.equal(host.min[has].double(), lo[has]) and torch.equal(host.max[has].double(), hi[has]))
    emit({"what": f"zone set {name}", "plane": f"{values.shape[0]} x {values.shape[1]} float32", "reps": reps, "zones": Z, "shift": shift,
          "pixels_in_a_zone": int(host.pixels.sum()), "valid_pixels": int(host.valid.sum()),
          "absmax": rate(8 * n, absmax_ms, copy_tbs), "values": rate(8 * n, values_ms, copy_tbs), "module_both_passes_and_host_reads": module_ms.record(),
          "baseline_index_add_float64_ms": round(base_ms.ms, 3), "baseline_over_both_passes": round(base_ms.ms / module_ms.ms, 2),
          "means_agree_within_the_bound": agree, "zones_compared": checked, "largest_mean_difference_vs_its_bound": [worst, worst_allowed],
          "fixed_point_bound": 2.0 ** (E - 31), "min_max_equal_the_baseline": extremes})
    del ids, table


def main(side, reps):
    from postprocess_bench import synthetic_mask
    from zonal_bench import grid_rings
    from unet_amd import rasterize as RZ
    from unet_amd import vectorize as VZ
    from unet_amd.postprocess import PostProcess
    values = value_plane(side)
    dst = torch.empty_like(values)
    copy_ms, _ = timed(lambda: dst.copy_(values), reps)
    del dst
    n = values.numel()
    copy_tbs = 8 * n / (copy_ms.ms * 1e-3) / 1e12          # 4 bytes read and 4 written per pixel
    emit({"what": "float32 copy of one plane (torch, the same run)", **copy_ms.record(), "bytes_moved": 8 * n, "TB_per_s": round(copy_tbs, 3)})
    mask = synthetic_mask(side)
    clean = PostProcess(majority=5, sieve=64)(mask)
    one_set("(a): a 10 x 10 grid of squares", grid_rings(side), values, reps, copy_tbs)
    rings = RZ.rings_from_polygons(VZ.polygonize(clean))
    del clean
    one_set("(b): the cleaned mask's own polygons", rings, values, reps, copy_tbs)
    del rings
    torch.cuda.empty_cache()
    rings = RZ.rings_from_polygons(VZ.polygonize(mask))
    del mask
    one_set("(c): the raw mask's own polygons (2 % salt)", rings, values, reps, copy_tbs)


if __name__ == "__main__":
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if not torch.cuda.is_available():
        sys.exit("zonal_values_bench.py measures on the GPU and there is no device")
    assert math.isfinite(NODATA)
    main(side, reps)
