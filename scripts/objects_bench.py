"""Cost of the object attributes (unet_amd/objects.py) on a 20000 x 20000 mask.
usage: python scripts/objects_bench.py [side=20000] [reps=3]
Prints one JSON line per measurement and writes them to profiles/objects_bench.json.
The fixed-seed synthetic 5-class mask of scripts/postprocess_bench.py (smooth regions + 2 % salt) in three states: raw (millions of
objects), after PostProcess(majority=5, sieve=64), and the cleaned mask with classes 1 and 3 split into instances (radius 64, min_depth 2).
Per state: measure_objects in milliseconds in total (best of `reps` after one warm-up, device synchronised; the label image is made
beforehand) and per stage -- index, accumulate, point -- from a second set of runs that synchronises after every stage; the bytes the
accumulation and the point pass must read (5 per pixel each: the label plane and the mask once) with the rate that makes and its share
of the 6.29 TB/s a float4 copy reaches on this GPU; and the same tables by the torch composition a user would write, in the same process:
index_add_ and scatter_reduce_ on int64 keyed by a dense id per pixel.  The baseline is GIVEN that dense id (offs[labels], made outside its
timed region); its tables must equal the kernels'."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, HERE)
import torch  # noqa: E402

OUT = os.path.join(HERE, "..", "profiles", "objects_bench.json")
RESULTS = []
COPY_TBS = 6.29          # MI355X: a float4 copy as measured
CLASSES = (1, 3)


def emit(rec):
    """print the record and rewrite the file, so that a run that ends early leaves what it measured"""
    from unet_amd.build import source_hash
    RESULTS.append(rec)
    print(json.dumps(rec), flush=True)
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": RESULTS, "kernel_source_hash": source_hash(),
                   "command": "python scripts/objects_bench.py " + " ".join(sys.argv[1:])}, f, indent=1)
        f.write("\n")


def timed(fn, reps):
    best, out = None, None
    for r in range(reps + 1):
        out = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        if r and (best is None or dt < best):
            best = dt
    return best, out


def rate(n: int, per_pixel: int, ms: float) -> dict:
    tbs = n * per_pixel / (ms * 1e-3) / 1e12
    return {"ms": round(ms, 3), "bytes_read": n * per_pixel, "TB_per_s": round(tbs, 3), "share_of_copy_rate": round(tbs / COPY_TBS, 3)}


def torch_tables(labels, dense, P):
    """the tables of measure_objects(mask, labels) by torch's keyed reductions on int64; dense: the object index of every pixel"""
    H, W = labels.shape
    dev = labels.device
    n = H * W
    k = dense.view(-1)
    p = torch.arange(n, device=dev, dtype=torch.int64)
    x, y = p % W, p // W
    pixels = torch.bincount(k, minlength=P)
    sum_x = torch.zeros(P, dtype=torch.int64, device=dev).index_add_(0, k, x)
    sum_y = torch.zeros(P, dtype=torch.int64, device=dev).index_add_(0, k, y)
    x0 = torch.full((P,), W, dtype=torch.int64, device=dev).scatter_reduce_(0, k, x, "amin")
    y0 = torch.full((P,), H, dtype=torch.int64, device=dev).scatter_reduce_(0, k, y, "amin")
    x1 = torch.zeros(P, dtype=torch.int64, device=dev).scatter_reduce_(0, k, x + 1, "amax")
    y1 = torch.zeros(P, dtype=torch.int64, device=dev).scatter_reduce_(0, k, y + 1, "amax")
    ev, eh = torch.zeros((H, W), dtype=torch.int64, device=dev), torch.zeros((H, W), dtype=torch.int64, device=dev)
    ev[:, 0] += 1
    ev[:, -1] += 1
    eh[0] += 1
    eh[-1] += 1
    dv, dh = labels[:, 1:] != labels[:, :-1], labels[1:] != labels[:-1]
    ev[:, 1:] += dv
    ev[:, :-1] += dv
    eh[1:] += dh
    eh[:-1] += dh
    edges_v = torch.zeros(P, dtype=torch.int64, device=dev).index_add_(0, k, ev.view(-1))
    edges_h = torch.zeros(P, dtype=torch.int64, device=dev).index_add_(0, k, eh.view(-1))
    del ev, eh, dv, dh
    cx, cy = sum_x // pixels, sum_y // pixels
    d2 = (x - cx[k]) ** 2 + (y - cy[k]) ** 2
    best = torch.full((P,), 2 ** 62, dtype=torch.int64, device=dev).scatter_reduce_(0, k, d2, "amin")
    cand = torch.where(d2 == best[k], p, torch.full_like(p, n))
    point = torch.full((P,), n, dtype=torch.int64, device=dev).scatter_reduce_(0, k, cand, "amin")
    return pixels, sum_x, sum_y, torch.stack([x0, y0, x1, y1], 1), edges_v, edges_h, point


def one_state(name, mask, labels, reps):
    from unet_amd import objects as OB
    from unet_amd import ops
    n = mask.numel()
    torch.cuda.empty_cache()
    ms, table = timed(lambda: OB.measure_objects(mask, labels), reps)
    stages = None
    for _ in range(reps):
        s = {}
        OB.measure_objects(mask, labels, stages=s)
        stages = s if stages is None else {k: min(v, stages[k]) for k, v in s.items()}
    P = table.n_objects
    # the dense id per pixel, given to the baseline
    mark, offs = torch.empty_like(mask), torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    blocks = torch.empty(ops.vec_scan_words(n), dtype=torch.int64, device=mask.device)
    ops.inst_marks(mask, labels, tuple(range(256)), mark)
    ops.vec_scan(mark, offs, blocks)
    dense = offs.view(-1)[labels.view(-1).long()].long().view(mask.shape)
    del mark, offs, blocks
    torch.cuda.empty_cache()
    base_ms, theirs = timed(lambda: torch_tables(labels, dense, P), max(1, reps - 1))
    ours = (table.pixels, table.sum_x, table.sum_y, table.bbox.long(), table.edges_v, table.edges_h, table.point.long())
    equal = all(bool(torch.equal(a, b)) for a, b in zip(ours, theirs))
    assert equal, f"{name}: the torch composition and the kernels disagree"
    emit({"what": f"measure_objects, {name}", "mask": f"{mask.shape[0]} x {mask.shape[1]}", "reps": reps, "objects": P,
          "largest_object_pixels": int(table.pixels.max()), "point_passes": 1 if ops.obj_point_packed(*mask.shape) else 2,
          "ms": round(ms, 3), "ns_per_pixel": round(ms * 1e6 / n, 4), "stage_ms": {k: round(v, 3) for k, v in stages.items()},
          "accumulate": rate(n, 5, stages["accumulate"]), "point": rate(n, 5, stages["point"]),
          "torch_composition_ms": round(base_ms, 3), "torch_over_kernels": round(base_ms / ms, 2), "faster_than_torch": bool(ms < base_ms),
          "tables_equal": equal})
    del theirs, dense, table


def main(side, reps):
    from postprocess_bench import synthetic_mask
    from unet_amd import instances as IN
    from unet_amd.postprocess import PostProcess, label_components
    mask = synthetic_mask(side)
    labels = label_components(mask, 4)
    one_state("raw: 5 classes, smooth regions + 2 % salt", mask, labels, reps)
    del labels
    clean = PostProcess(majority=5, sieve=64)(mask)
    del mask
    torch.cuda.empty_cache()
    labels = label_components(clean, 4)
    one_state("after PostProcess(majority=5, sieve=64)", clean, labels, reps)
    del labels
    torch.cuda.empty_cache()
    labels, _ = IN.split_instances(clean, CLASSES, 64, 2.0)
    one_state(f"the cleaned mask with classes {list(CLASSES)} split into instances (radius 64, min_depth 2)", clean, labels, reps)


if __name__ == "__main__":
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    if not torch.cuda.is_available():
        sys.exit("objects_bench.py measures on the GPU and there is no device")
    main(side, reps)
