"""Cost of the float statistics per object (unet_amd/objects.py object_values, csrc/object_values.hip) on a 20000 x 20000 plane.
usage: python scripts/object_values_bench.py [side=20000] [reps=5]
Prints one JSON line per measurement and writes them to profiles/object_values_bench.json.
The masks are those of scripts/objects_bench.py -- the fixed-seed synthetic 5-class mask raw (2 % salt: millions of objects), after
PostProcess(majority=5, sieve=64), and the cleaned mask with classes 1 and 3 split into instances --, the value plane that of
scripts/zonal_values_bench.py (20 + 5 * normal noise, 1 % nodata -9999, a sprinkle of NaN); class 0 is excluded.  Per state, after two warm-up
calls each, `reps` rounds of one sample per function taken in turn in one process -- absmax, values, the composition and its two parts
-- and the median of each (least
and largest beside it); a sample is a run of back-to-back calls of about 0.3 s that ends in a device synchronise:
  absmax       ops.obj_absmax alone; it must read 5 bytes per pixel (mask and values)
  values       ops.obj_values alone (initialisation, the pass, the decoding of the extremes); 9 bytes per pixel (mask, labels, values)
  composition  what existing code offers: a dense id plane offs[labels] (-1 on the excluded class) by torch indexing, then
               zonal.zonal_values with the same shift; its two parts are timed apart as well.  Its valid, sum_q, sq_lo, sq_hi, min and max
               must equal the new tables (asserted); it has no argmin / argmax
No hardware counters are taken here: what limits the kernel is not measured by this script."""
import json
import math
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, HERE)
import torch  # noqa: E402

OUT = os.path.join(HERE, "..", "profiles", "object_values_bench.json")
RESULTS = []
NODATA = -9999.0
EXCLUDE = (0,)
CLASSES = (1, 3)
WINDOW_S = 0.3          # every sample times at least this much work


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
                "command": "python scripts/object_values_bench.py " + " ".join(sys.argv[1:])})
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def alternated(fns: dict, reps: int, warm: int = 2) -> dict:
    """{name: [milliseconds per call, one per round]}: `reps` rounds, in each one sample of every function in turn; a sample is a run of
    back-to-back calls that ends in a device synchronise and lasts about WINDOW_S, its length taken from the last warm-up call"""
    calls = {}
    for name, fn in fns.items():
        for _ in range(warm):
            t, _ = once(fn)
        calls[name] = max(1, min(1000, math.ceil(WINDOW_S / max(t, 1e-6))))
    samples = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            def run(fn=fn, k=calls[name]):
                for _ in range(k):
                    fn()
            t, _ = once(run)
            samples[name].append(t * 1e3 / calls[name])
    return samples


def record(samples, nbytes=None) -> dict:
    s = sorted(samples)
    rec = {"ms": round(s[len(s) // 2], 3), "ms_least": round(s[0], 3), "ms_largest": round(s[-1], 3), "samples_ms": [round(x, 3) for x in samples]}
    if nbytes is not None:
        rec.update(bytes_read=nbytes, TB_per_s=round(nbytes / (rec["ms"] * 1e-3) / 1e12, 3))
    return rec


def one_state(name, mask, labels, values, reps):
    from unet_amd import objects as OB
    from unet_amd import ops
    from unet_amd import zonal as ZN
    n = mask.numel()
    torch.cuda.empty_cache()
    offs, P, label, _ = OB._object_index(mask, labels, EXCLUDE)
    words = torch.zeros(2, dtype=torch.int64, device="cuda")
    table = torch.empty((6, P), dtype=torch.int64, device="cuda")
    ops.obj_absmax(mask, values, EXCLUDE, NODATA, words[0:1])
    shift = ZN.shift_of_absmax(int(words[0]))
    kept = torch.ones(256, dtype=torch.bool, device="cuda")
    kept[list(EXCLUDE)] = False
    minus = torch.full((), -1, dtype=torch.int32, device="cuda")

    def dense_ids():
        return torch.where(kept[mask.long()], offs.view(-1)[labels.view(-1).long()].view(mask.shape), minus)

    def composition():
        return ZN.zonal_values(dense_ids(), values, P, NODATA, shift)

    fns = {"absmax": lambda: ops.obj_absmax(mask, values, EXCLUDE, NODATA, words[0:1]),
           "values": lambda: ops.obj_values(mask, labels, values, offs, EXCLUDE, P, NODATA, shift, table, words[1:2])}
    possible = P < ops.RAS_MAX_FEATURES          # zonal_values takes fewer than 2^23 zones
    if possible:
        ids = dense_ids()
        fns.update({"composition": composition, "composition_ids_alone": dense_ids,
                    "composition_zonal_values_alone": lambda: ZN.zonal_values(ids, values, P, NODATA, shift)})
    samples = alternated(fns, reps)
    assert int(words[1]) == 0
    new = OB.ObjectValues.of_table(label, table, shift, tuple(mask.shape))
    module = OB.object_values(mask, values, labels, EXCLUDE, NODATA)
    assert module.shift == shift and all(torch.equal(getattr(module, k), getattr(new, k)) for k in ("valid", "sum_q", "sq_lo", "sq_hi", "argmin", "argmax"))
    flat = values.view(-1)
    has = new.valid > 0
    peaks = bool(torch.equal(flat[new.argmax[has].long()], new.max[has]) and torch.equal(flat[new.argmin[has].long()], new.min[has]))
    assert peaks
    head = {"what": name, "plane": f"{mask.shape[0]} x {mask.shape[1]}", "reps": reps, "objects": P, "shift": shift, "excluded": list(EXCLUDE),
            "valid_pixels": int(new.valid.sum()), "objects_without_a_valid_pixel": int((~has).sum()),
            "absmax": record(samples["absmax"], 5 * n), "values": record(samples["values"], 9 * n), "values_at_argmin_argmax_are_min_max": peaks}
    if not possible:
        emit({**head, "composition_offs_labels_then_zonal_values": f"not possible: {P} objects, zonal_values takes fewer than 2^23 zones"})
        return
    z = composition()
    equal = all(torch.equal(getattr(z, k), getattr(new, k)) for k in ("valid", "sum_q", "sq_lo", "sq_hi")) and \
        torch.equal(z.min.view(torch.int32), new.min.view(torch.int32)) and torch.equal(z.max.view(torch.int32), new.max.view(torch.int32))
    assert equal, "the composition through zonal_values differs from the new tables"
    v, c = head["values"], record(samples["composition"])
    emit({**head, "composition_offs_labels_then_zonal_values": c,
          "composition_ids_alone": record(samples["composition_ids_alone"]),
          "composition_zonal_values_alone": record(samples["composition_zonal_values_alone"]),
          "composition_over_values": round(c["ms"] / v["ms"], 2), "tables_equal_the_composition": equal})


def main(side, reps):
    from postprocess_bench import synthetic_mask
    from zonal_values_bench import value_plane
    from unet_amd import instances as IN
    from unet_amd.postprocess import PostProcess, label_components
    values = value_plane(side)
    mask = synthetic_mask(side)
    labels = label_components(mask, 4)
    one_state("raw: 5 classes, smooth regions + 2 % salt", mask, labels, values, reps)
    del labels
    clean = PostProcess(majority=5, sieve=64)(mask)
    del mask
    torch.cuda.empty_cache()
    labels = label_components(clean, 4)
    one_state("after PostProcess(majority=5, sieve=64)", clean, labels, values, reps)
    del labels
    torch.cuda.empty_cache()
    labels, _ = IN.split_instances(clean, CLASSES, 64, 2.0)
    one_state(f"the cleaned mask with classes {list(CLASSES)} split into instances (radius 64, min_depth 2)", clean, labels, values, reps)


if __name__ == "__main__":
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if not torch.cuda.is_available():
        sys.exit("object_values_bench.py measures on the GPU and there is no device")
    main(side, reps)
