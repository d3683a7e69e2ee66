"""Prediction entry points of the tile workflow on the MI355X hot path.

``save_predictions`` mirrors the reference's (``predict.py:146-147``): a folder of tile files -> per-tile predictions or ONE merged
raster.  ``predict_raster`` is BASELINE.json configs[4] as one call: sliding-window inference over a whole raster that stays in HBM as
the integers it was read as -- the reference needs two steps for it, ``create_tiles_unet.split_raster`` (tile files on disk,
``create_tiles_unet.py:252-434``) and ``save_predictions(merge=True)`` (``predict.py:191-222,257-334``), and produces the same mosaic.

Differences that keep the results but not the schedule:
* tiles are predicted in BATCHES (the reference loops ``learn.predict`` one tile at a time, ``predict.py:191-193``); windows / tiles are cut,
  cast and scaled on the device (``unet_window_gather``) from uint8 / uint16 samples, a prefetch thread decodes the next tile files into pinned
  memory while the current batch runs;
* the overlap merge -- sum of softmax probabilities + hit counter -> divide -> argmax (``predict.py:284-334``) -- runs on the GPU, batch by
  batch (``unet_mosaic_accumulate_windows``), in ONE defined order (placements sorted by row, then column; the reference uses the directory
  order of ``glob``);
* under N ranks (one process per GPU) the mosaic is partitioned by rows (``unet_amd/mosaic.py``): every rank keeps only its strip, overlap rows
  travel as per-window slabs to the neighbouring rank, and only the requested band(s) -- the uint8 argmax by default -- reach rank 0 and the host.
``regression`` predicts the raw single-band output (merged mosaic = mean of the overlapping tiles, nodata -9999 where no tile was
placed).  The confusion-matrix plots (``predict.py:56-143``) are reporting and out of scope.

Beyond the reference: ``tta=`` (None | "flips" | "d4" | a tuple of D4 codes, ``unet_amd/tta.py``) adds test-time augmentation to both entry
points, merged and per tile.  Every batch runs k forwards of the same geometry on oriented windows (``unet_window_gather_oriented``); the
outputs are mapped back and averaged per window on the device in code order (``unet_tta_accumulate``), and that mean takes the place of the
window's softmax probabilities in the merge, the slabs, the int8 ``large_file`` merge and the per-tile outputs.  The hit counter still counts
windows.

Also beyond the reference: ``blend=`` ("mean" | "gaussian") of both entry points' merged outputs.  "mean" is the reference's merge above.
"gaussian" weights every window's contribution to a pixel with a centre-peaked importance map (the product of two 1-D Gaussians, sigma =
window side / 8, ``unet_amd/mosaic.py``), as nnU-Net and MONAI's sliding-window inference do, so that pixels near a window's edge -- predicted
with half their context -- count less than the same pixels seen from the middle of the next window and the seams fade.  The weighted sum
and the weight sum are accumulated on the device in the same order as the mean (``unet_mosaic_accumulate_windows_weighted``, the weighted
slab add and finalisation), so N ranks equal 1 rank bit for bit here too.  Refused (ValueError) for ``large_file`` and per-tile outputs.

The output options beyond the reference, each described at ``predict_raster``: ``postprocess=`` (majority filter / sieve of the merged class
mask, ``unet_amd/postprocess.py``), ``compress=`` / ``predictor=`` / ``tile=`` / ``overviews=`` (LZW GeoTIFFs, tiled and with overviews),
``vector_path=`` / ``vector=True`` with ``vector_exclude=`` and ``vector_simplify=`` (the mask's polygons as GeoJSON, ``unet_amd/vectorize.py``) and
``instances=`` (touching objects split into instances, ``unet_amd/instances.py``) and ``zones_path=`` / ``zones=`` with ``zonal_objects=`` (pixels, shares
and objects of every class per polygon zone, ``unet_amd/zonal.py``; with ``zonal_values=`` the mean, std, min, max and sum of a regression or
``specific_class`` plane per zone instead).  ``check_outputs``, the first statement of both entry points,
checks them from the arguments alone (ValueError before the model is loaded) into one ``OutputPlan``.  ``_write_outputs`` is the one output stage,
on rank 0 and on the assembled mask, so N ranks equal 1 rank by construction: instances, the vector file, the zonal table, the raster.  The plan keeps the merged
array where the merge assembled it while a stage needs it there: with one rank the mask goes from the argmax through the filters, the split and
the polygonizer into the LZW encoder (``unet_amd/tiffenc.py``) on the device; the int8 ``large_file`` merge, gloo ranks and per-tile outputs use
the host encoder of ``unet_amd/tiffio.py``: the same file.
"""
from __future__ import annotations

import contextlib
import dataclasses
import os
import queue
import threading
import time
import warnings
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from unet_amd import ops
from unet_amd.feed import BatchFeeder, default_workers, torch_samples
from unet_amd.learner import load_learner, open_tile
from unet_amd.postprocess import PostProcess, check_postprocess
from unet_amd.mosaic import MergePlan, blend_profile, check_blend, keep_windows, merge_order, sliding_windows
from unet_amd.tiffio import check_compress, check_tiling, read_tiff, resolve_overviews, tiff_info, write_tiff
from unet_amd.tta import parse as tta_codes
from unet_amd.vectorize import check_vector, epsg_of_tags, vectorize_mask
from unet_amd.instances import Instances, check_instances
from unet_amd.zonal import check_zones, zonal_mask, zonal_plane
from unet_amd.objects import check_object_planes, check_objects, objects_mask, read_value_raster


def store_tif(output_file, data, geotrans=None, tags=None, nodata=None, class_zero=False, compress=None, predictor=1,
              timing: Optional[dict] = None, tile=None, overviews=None):
    """predict.py:19-52: GeoTIFF writer; class_zero shifts class ids back by one (0 was reserved for nodata).
    compress="lzw" (predictor=2: horizontal differencing, integer samples): LZW strips -- a device tensor is shifted and encoded on the
    device (unet_amd/tiffenc.py), a host array by the host encoder (tiffio.write_tiff); the two write the same file.  timing gains
    write_seconds and file_bytes.  tile / overviews ("mode" | "average" | "nearest"; needs compress="lzw"): square LZW tiles and the overview
    pyramid behind the full-resolution image (tiffio.TileWriter), built and encoded by whichever of the two writers applies."""
    t0 = time.perf_counter()
    if isinstance(data, torch.Tensor) and data.is_cuda and compress is not None:
        from unet_amd.tiffenc import write_tiff_device
        t = data
        if class_zero and not t.dtype.is_floating_point and t.dtype != torch.bool:
            t = t - 1 if t.dtype.is_signed else (t.to(torch.int16) - 1)          # the dtypes of the host path below
        write_tiff_device(output_file, t, geotransform=geotrans, tags=tags, nodata=nodata, compress=compress, predictor=predictor,
                          tile=tile, overviews=overviews)
    else:
        a = data.cpu().numpy() if isinstance(data, torch.Tensor) else np.asarray(data)
        if class_zero and a.dtype.kind in "ui":
            a = a - 1 if a.dtype.kind == "i" else (a.astype(np.int16) - 1)
        write_tiff(output_file, a, geotransform=geotrans, tags=tags, nodata=nodata, compress=compress, predictor=predictor, tile=tile,
                   overviews=overviews)
    if timing is not None:
        timing.update(write_seconds=time.perf_counter() - t0, file_bytes=os.path.getsize(output_file))


@dataclasses.dataclass(frozen=True)
class OutputPlan:
    """The output arguments of predict_raster / save_predictions as check_outputs resolved them, before the model is loaded or anything touches
    the GPU.  Nothing downstream decides about the outputs itself: every derived value is a property (of p, the plan), stated here only."""
    regression: bool = False
    all_classes: bool = False
    specific_class: Optional[int] = None
    large_file: bool = False
    merge: bool = True
    class_zero: bool = False
    raster: bool = True                               # the prediction is written as a GeoTIFF (False: predict_raster without out_path)
    blend: str = "mean"
    postprocess: Optional[PostProcess] = None
    compress: Optional[str] = None
    predictor: int = 1
    tile: Optional[int] = None
    overviews: Optional[str] = None                   # "mode" | "average" | "nearest": "auto" is resolved
    vector: Optional[tuple] = None                    # the classes that get no polygon; None: no vector file
    vector_simplify: Optional[float] = None
    instances: Optional[Instances] = None
    instances_raster: bool = False
    objects_values: Optional[str] = None              # the column prefix of the value raster's statistics per object; None: no value raster
    objects_confidence: bool = False                  # the objects file gains confidence_*: the merged probability of the chosen class
    zones: bool = False                               # a zonal table is written
    zonal_values: bool = False                        # ... of the float plane (zonal_plane) instead of the class mask (zonal_mask)
    zonal_objects: bool = False
    objects: Optional[tuple] = None                   # the classes that are not measured; None: no objects file

    mask = property(lambda p: not (p.regression or p.all_classes or p.specific_class is not None))       # the output is the class mask
    want = property(lambda p: 0 if p.regression else "all" if p.all_classes else "argmax" if p.mask else int(p.specific_class))    # _Merge.finish
    floats = property(lambda p: p.regression or not (p.mask or p.large_file))       # no Predictor 2, no "mode" overviews (large_file: int8 planes)
    int8_merge = property(lambda p: p.large_file and not p.regression)
    nodata = property(lambda p: -9999 if p.regression else None)
    # a compressed raster is written from the tensor the merge assembled: on the device with one rank or RCCL, where only the bytes reach the host
    encode_in_place = property(lambda p: p.compress is not None and p.raster)
    keep = property(lambda p: p.encode_in_place or p.vector is not None or p.instances is not None or p.zones or p.objects is not None)       # the merged array stays a tensor there

    def needs_mask(self, subject: str, done: str, one_device: bool = True):
        """the rule of every option that works on the class mask of a merged prediction"""
        if not self.mask:
            raise ValueError(f"{subject} needs the class mask: not with regression, all_classes or specific_class")
        if one_device and self.large_file:
            raise ValueError(f"{subject} needs the class mask on one device: not with large_file")
        if not self.merge:
            raise ValueError(f"{subject} needs merge=True: per-tile outputs are not {done}")

    def needs_plane(self, zones: bool, zonal_objects: bool):
        """the rule of zonal_values: the statistics of the output's one float plane per zone"""
        if not zones:
            raise ValueError("zonal_values without zones")
        if zonal_objects:
            raise ValueError("zonal_values with zonal_objects: objects are counted on the class mask")
        if self.mask:
            raise ValueError("zonal_values needs a float plane, regression or specific_class: the class mask has none (its table is zones "
                             "without zonal_values)")
        if self.all_classes:
            raise ValueError("zonal_values needs one float plane: not with all_classes")
        if self.large_file:
            raise ValueError("zonal_values needs the float plane on one device: not with large_file")
        if not self.merge:
            raise ValueError("zonal_values needs merge=True: per-tile outputs are not summarised")


def check_outputs(regression=False, all_classes=False, specific_class=None, large_file=False, merge=True, class_zero=False, blend="mean",
                  postprocess=None, compress=None, predictor=1, tile=None, overviews=None, vector=None, vector_exclude=None, vector_simplify=None,
                  instances=None, instances_raster=False, raster=True, return_array=True, raster_arg="instances_raster", *, zonal_values=False,
                  objects_values=None, objects_values_name="value", objects_confidence=False, objects=None, objects_exclude=None, zones=None,
                  zonal_objects=False) -> OutputPlan:
    """Every check of the two entry points' output arguments, from the arguments alone and in one order -> the OutputPlan.  vector: vector= or
    vector_path=; instances_raster: whether the argument named raster_arg asks for the instance raster; raster: whether out_path is given;
    objects: objects= or objects_path=; zones: zones= or zones_path= (the entry points check that its output path is there); zonal_values:
    the table summarises the one float plane of the output (regression, specific_class) instead of the class mask; objects_values:
    objects_values= or objects_values_path=, the value raster whose statistics per object join the objects file as <objects_values_name>_*;
    objects_confidence: the same of the merged probability of the chosen class, as confidence_*.  Everything from
    zonal_values on is passed by keyword, as both entry points always did, so that a new argument can never shift a positional one"""
    mode = OutputPlan(bool(regression), bool(all_classes), specific_class, bool(large_file), bool(merge), bool(class_zero), bool(raster))
    check_blend(blend, large_file, merge)
    post = check_postprocess(postprocess)
    if post is not None:
        mode.needs_mask("postprocess", "post-processed", one_device=False)       # the mask of the int8 merge is uploaded for it
    compress, predictor = check_compress(compress, predictor, mode.floats)
    tile, overviews = check_tiling(compress, tile, overviews, auto=True)
    tile, overviews = check_tiling(compress, tile, resolve_overviews(overviews, mode.mask), mode.floats)
    vec = check_vector(vector, vector_exclude, class_zero, vector_simplify)
    if vec is not None:
        mode.needs_mask("a vector output", "polygonized")
    if instances is None and instances_raster:
        raise ValueError(f"{raster_arg} without instances")
    obj = check_objects(objects, objects_exclude, class_zero)
    if obj is not None:
        mode.needs_mask("object attributes", "measured")
    values_name = check_object_planes(objects_values, objects_values_name, objects_confidence, obj is not None)
    inst = check_instances(instances)
    if inst is not None:
        mode.needs_mask("instances", "split")
        if vec is None and not instances_raster and zones is None and obj is None:
            raise ValueError("instances without an output: ask for the vector file, the instance raster or both")
    zonal = check_zones(zones, zonal_objects)
    if zonal_values:
        mode.needs_plane(zonal, zonal_objects)
    elif zonal:
        mode.needs_mask("zonal statistics", "summarised")
    if not return_array and not raster and vec is None and not zonal and obj is None:
        raise ValueError("return_array=False needs out_path: the prediction would go nowhere")
    return dataclasses.replace(mode, blend=blend, postprocess=post, compress=compress, predictor=predictor, tile=tile, overviews=overviews,
                               vector=vec, vector_simplify=vector_simplify, instances=inst, instances_raster=bool(instances_raster),
                               zones=zonal, zonal_values=bool(zonal_values), zonal_objects=bool(zonal_objects), objects_values=values_name,
                               objects_confidence=bool(objects_confidence), objects=obj)


def _write_outputs(plan: OutputPlan, out, device, gt, tags, raster_path, vector_path, instances_path, class_names, timing, zones_path=None,
                   zonal_path=None, objects_path=None, object_planes=None):
    """Rank 0's output stage on the merged array `out` of _Merge.finish (a tensor under plan.keep, else a NumPy array): the instance split (its
    dense ids as a uint32 GeoTIFF with the mask's geo tags, by tiffio.write_tiff, so compress, predictor and tile apply to it as to the mask),
    the object attributes (of the instances where there are any, else of the components; a vector file written too carries them on its
    features), the vector file, the zonal table (its objects are the instances where there are any, else the components), the move to the host unless
    the raster is encoded from the tensor, the raster.  object_planes: None or {name: (float32 plane on the output's grid, nodata)} -- the value
    raster and the confidence plane, whose statistics per object (objects.object_values, after measure_objects on the same mask and labels:
    the instance labels where there are any) join the objects file and the polygon features; timing gains objects_values_seconds.  Returns
    what the raster is written from."""
    labels = ids = None
    if plan.instances is not None:
        out = torch.as_tensor(out)
        out = (out if out.is_cuda else out.to(device)).contiguous()
        labels, ids, _ = plan.instances.run(out, timing)
        if instances_path is not None:
            t0 = time.perf_counter()
            write_tiff(instances_path, ids.cpu().numpy().view(np.uint32), gt, tags, compress=plan.compress, predictor=plan.predictor, tile=plan.tile)
            if timing is not None:
                timing.update(instances_write_seconds=time.perf_counter() - t0, instances_file_bytes=os.path.getsize(instances_path))
    attributes = None
    if plan.objects is not None:
        out = torch.as_tensor(out)
        out = (out if out.is_cuda else out.to(device)).contiguous()
        more = {}
        if object_planes:          # without planes: the call it was
            more["values"] = {name: (torch.as_tensor(a).to(out.device).contiguous(), nd) for name, (a, nd) in object_planes.items()}
        attributes = objects_mask(out, objects_path, plan.objects, gt, epsg_of_tags(tags), class_names, plan.class_zero, labels, ids, timing, **more)
    if plan.vector is not None:
        extra = {} if attributes is None else {"attributes": attributes}          # without objects: the call it was
        vectorize_mask(out, vector_path, plan.vector, gt, epsg_of_tags(tags), class_names, plan.class_zero, timing, plan.vector_simplify, labels, ids,
                       **extra)
    if plan.zones:
        out = torch.as_tensor(out)
        out = (out if out.is_cuda else out.to(device)).contiguous()
        if plan.zonal_values:
            zonal_plane(out, zones_path, zonal_path, gt, tags, plan.nodata, timing)
        else:
            zonal_mask(out, zones_path, zonal_path, gt, tags, class_names, plan.class_zero, labels, plan.zonal_objects, timing)
    if not plan.encode_in_place and isinstance(out, torch.Tensor):
        out = out.cpu().numpy()
    if raster_path is not None:
        store_tif(raster_path, out, gt, tags, plan.nodata, plan.class_zero, plan.compress, plan.predictor, timing, plan.tile, plan.overviews)
    return out


def _geo(path):
    """(geotransform, GeoTIFF tags, height, width) from the header alone (.npy tiles carry no georeference)"""
    if Path(path).suffix == ".npy":
        a = np.load(path, mmap_mode="r")
        return None, {}, int(a.shape[-2]), int(a.shape[-1])
    meta = tiff_info(path)
    return meta["geotransform"], meta["tags"], meta["height"], meta["width"]


LARGE_FILE_SCALE = (128 / 4) - 1        # predict.py:209-214: probabilities stretched to int8 as around(p * 31)


# ----------------------------------------------------------------------------------------------- p2p plumbing (RCCL, or gloo in tests)

def _dist():
    import torch.distributed as dist
    return dist


def _exchange(send: Optional[torch.Tensor], dst: int, recv_numel: int, src: int, dtype, device) -> Optional[torch.Tensor]:
    """one simultaneous isend / irecv pair between neighbouring ranks (either side may be absent); gloo moves host memory"""
    dist = _dist()
    host = dist.get_backend() == "gloo"
    ops_, rbuf = [], None
    if recv_numel:
        rbuf = torch.empty(recv_numel, dtype=dtype, device="cpu" if host else device)
        ops_.append(dist.P2POp(dist.irecv, rbuf, src))
    if send is not None and send.numel():
        ops_.append(dist.P2POp(dist.isend, send.cpu() if host else send, dst))
    if ops_:
        for w in dist.batch_isend_irecv(ops_):
            w.wait()
    return None if rbuf is None else rbuf.to(device)


# ----------------------------------------------------------------------------------------------- the merge engine

class _Merge:
    """Runs one rank's share of a merged prediction: forward of its placements in batches, accumulation into its strip of the
    mosaic, slab exchange with the neighbours, finalisation, gather of the requested output on rank 0."""

    def __init__(self, model, places: np.ndarray, MH: int, MW: int, regression: bool, int8_merge: bool, rank: int, world: int, blend: str = "mean"):
        self.model, self.dev = model, model._device
        self.C = model.n_out
        self.raw, self.int8 = bool(regression), bool(int8_merge)
        self.rank, self.world = rank, world
        self.plan = MergePlan(places, MH, MW, world)
        self.lo, self.hi = self.plan.own[rank]
        rows = self.hi - self.lo
        if self.int8:       # the reference's int8 arrays: merged raster AND hit counter are int8 per class (predict.py:276-281)
            self.mosaic = torch.zeros((self.C, max(rows, 1), MW), dtype=torch.int8, device=self.dev)
            self.count = torch.zeros((self.C, max(rows, 1), MW), dtype=torch.int8, device=self.dev)
        else:
            self.mosaic = torch.zeros((self.C, max(rows, 1), MW), dtype=torch.float32, device=self.dev)
            self.count = torch.zeros((max(rows, 1), MW), dtype=torch.int32, device=self.dev)
        # Gaussian blending: the weight sum of every strip pixel (the divisor in place of the hit counter) and the device profile tables,
        # one per window side length, uploaded once per call
        self.blend = check_blend(blend, self.int8)
        self.wsum = torch.zeros((max(rows, 1), MW), dtype=torch.float32, device=self.dev) if self.blend == "gaussian" else None
        self._profiles = {}
        self.acc_table = ops.window_table(self.plan.places[:, :2].tolist(), self.dev)       # (y0, x0) in mosaic coordinates
        self.my_slabs = self.plan.slabs(rank)
        self._slab_off, off = {}, 0
        for i, r in self.my_slabs:
            self._slab_off[i] = (off, r)
            off += self.C * r * int(self.plan.places[i, 3])
        self.sendbuf = torch.empty(off, dtype=torch.float32, device=self.dev) if off else None

    def _profile(self, n: int) -> torch.Tensor:
        t = self._profiles.get(n)
        if t is None:
            t = self._profiles[n] = torch.from_numpy(blend_profile(n)).to(self.dev)
        return t

    # -- int8 "large_file" accumulation of one window's probabilities [C, rows, w] at strip row y (may be clipped), column x
    def _add_int8(self, probs: torch.Tensor, y: int, x: int):
        q = torch.round(probs * LARGE_FILE_SCALE).to(torch.int8)            # np.around: half to even, as torch.round
        r0, r1 = max(0, -y), min(q.shape[1], self.hi - self.lo - y)
        if r1 <= r0:
            return
        self.mosaic[:, y + r0:y + r1, x:x + q.shape[2]] += q[:, r0:r1]
        self.count[:, y + r0:y + r1, x:x + q.shape[2]] += 1

    def add_batch(self, first: int, n: int, z: ops.TS, values: bool = False):
        """logits z [>= n, h, w, C] of placements [first, first + n); values=True: z already holds the window's probabilities (or
        regression outputs) -- the finalised TTA accumulator -- and is added as it is"""
        rows = self.hi - self.lo
        raw = self.raw or values
        if rows > 0:
            if self.int8:
                probs = torch.empty((n, self.C, z.H, z.W), dtype=torch.float32, device=self.dev)
                if values:
                    ops.nhwc_to_nchw(ops.TS(z.buf[:n], z.co, z.C), probs)
                else:
                    ops.softmax_argmax(ops.TS(z.buf[:n], z.co, z.C), probs, None)
                for j in range(n):
                    y0, x0 = self.plan.places[first + j, :2]
                    self._add_int8(probs[j], int(y0) - self.lo, int(x0))
            elif self.wsum is None:
                ops.mosaic_accumulate_windows(z, self.acc_table, first, n, (self.lo, 0), self.mosaic, self.count, 0, rows, raw=raw)
            else:
                ops.mosaic_accumulate_windows_weighted(z, self.acc_table, first, n, (self.lo, 0), self.mosaic, self.count, self.wsum,
                                                       self._profile(z.H), self._profile(z.W), 0, rows, raw=raw)
        for j in range(n):          # rows that belong to the strip above: per-window slabs for rank - 1
            ent = self._slab_off.get(first + j)
            if ent is None:
                continue
            off, r = ent
            w = int(self.plan.places[first + j, 3])
            out = self.sendbuf[off:off + self.C * r * w].view(1, self.C, r, w)
            zs = ops.TS(z.buf[j:j + 1, :r], z.co, z.C)
            if raw:
                ops.nhwc_to_nchw(zs, out)
            else:
                ops.softmax_argmax(zs, out, None)

    def exchange(self):
        """slabs up to rank - 1, slabs of rank + 1 added on top of the own windows (in placement order); a blended merge weights a slab
        here, on the receiving side, with rows [0, rr) of the sender window's vertical profile"""
        if self.world == 1 or self.plan.active == 1:
            return
        r, act = self.rank, self.plan.active
        if r >= act:
            return
        nrecv = self.plan.slab_floats(r + 1, self.C) if r + 1 < act else 0
        got = _exchange(self.sendbuf if r > 0 else None, r - 1, nrecv, r + 1, torch.float32, self.dev)
        if got is None:
            return
        off = 0
        for i, rr in self.plan.slabs(r + 1):
            y0, x0, h, w = (int(v) for v in self.plan.places[i])
            slab = got[off:off + self.C * rr * w].view(self.C, rr, w)
            off += self.C * rr * w
            if self.int8:
                self._add_int8(slab, y0 - self.lo, x0)
            elif self.wsum is None:
                ops.mosaic_accumulate(slab, self.mosaic, self.count, y0 - self.lo, x0)
            else:
                ops.mosaic_accumulate_weighted(slab, self._profile(h), self._profile(w), self.mosaic, self.count, self.wsum, y0 - self.lo, x0)

    def finish(self, want, postprocess=None, timing: Optional[dict] = None, keep: bool = False, extra: Optional[dict] = None):
        """want: "argmax" | "all" | int class index.  Returns (on rank 0) the full-size numpy array, None elsewhere.  postprocess: a
        PostProcess applied to the assembled class mask on rank 0 (want == "argmax" only: check_outputs).  keep (OutputPlan.keep): the result
        comes back as the tensor it was assembled in -- on the device with one rank or RCCL, on the host for the int8 merge and gloo.
        extra: a dict that asks for the confidence plane (want == "argmax", no int8 merge: check_outputs) and receives it on rank 0 as
        extra["confidence"], float32 [MH, MW] in the tensor it was assembled in: c[p] = the maximum over the classes of the finalised mosaic at
        p -- the merged probability of the class that the argmax chose, before postprocess.  Every rank takes the plane of its own rows and
        rank 0 assembles it behind the mask, as it does a specific_class plane.  A pixel that no window covered holds 0.0 there: the
        finalisation divides only where the hit count is positive, so all classes keep the zero they started from (and the mask class 0)"""
        rows, MW, MH = self.hi - self.lo, self.plan.MW, self.plan.MH
        if self.int8:
            merged, counter = self.mosaic[:, :rows].cpu().numpy(), self.count[:, :rows].cpu().numpy()
            m = counter > 0
            merged[m] //= counter[m]                        # predict.py:324-329: integer floor division, numpy semantics
            part = merged.argmax(axis=0).astype(np.uint8) if want == "argmax" else (merged if want == "all" else merged[want])
            part = torch.from_numpy(np.ascontiguousarray(part))
        else:
            am = torch.empty((max(rows, 1), MW), dtype=torch.uint8, device=self.dev) if want == "argmax" else None
            if rows > 0 and self.wsum is None:
                ops.mosaic_finalize_rows(self.mosaic, self.count, 0, rows, am, fill=-9999.0 if self.raw else None)
            elif rows > 0:
                ops.mosaic_finalize_rows_weighted(self.mosaic, self.count, self.wsum, 0, rows, am, fill=-9999.0 if self.raw else None)
            part = am[:rows] if want == "argmax" else (self.mosaic[:, :rows] if want == "all" else self.mosaic[want, :rows])
        conf = torch.amax(self.mosaic[:, :rows], dim=0) if extra is not None else None          # a maximum is exact
        if postprocess is None:
            out = self._gather_rows(part, want == "all", True) if keep else self._gather_rows(part, want == "all")
            if conf is not None:
                extra["confidence"] = self._gather_rows(conf, False, True)
            return out
        # one rank: the mask goes from the argmax to the filters on the device; N ranks: rank 0 uploads the assembled mask again
        full = part if self.world == 1 else self._gather_rows(part, False)
        if conf is not None:
            extra["confidence"] = self._gather_rows(conf, False, True)
        if full is None:
            return None
        t0 = time.perf_counter()
        out, info = postprocess.run(torch.as_tensor(full).to(self.dev))
        if not keep:
            out = out.cpu().numpy()
        if timing is not None:
            timing.update(postprocess_seconds=time.perf_counter() - t0, postprocess=info)
        return out

    def _gather_rows(self, part: torch.Tensor, planes: bool, keep: bool = False):
        """row strips of the ranks -> one array on rank 0 (only the requested band(s) travel); keep: the tensor it was assembled in"""
        MW, MH = self.plan.MW, self.plan.MH
        if self.world == 1:
            return part if keep else part.cpu().numpy()
        dist = _dist()
        host = dist.get_backend() == "gloo"
        part = (part.cpu() if host else part.to(self.dev)).contiguous()
        if self.rank != 0:
            if part.numel():
                dist.send(part, 0)
            return None
        shape = (self.C, MH, MW) if planes else (MH, MW)
        full = torch.empty(shape, dtype=part.dtype, device="cpu" if host else self.dev)
        sl = (slice(None),) if planes else ()
        full[sl + (slice(self.lo, self.hi),)] = part
        for r in range(1, self.plan.active):
            lo, hi = self.plan.own[r]
            if hi <= lo:
                continue
            buf = torch.empty(((self.C,) if planes else ()) + (hi - lo, MW), dtype=part.dtype, device=full.device)
            dist.recv(buf, r)
            full[sl + (slice(lo, hi),)] = buf
        return full if keep else full.cpu().numpy()


def _run_merge(model, places, MH, MW, regression, int8_merge, rank, world, batch, make_input: Callable, want, timing: Optional[dict] = None,
               tta: Optional[Tuple[int, ...]] = None, blend: str = "mean", postprocess=None, keep: bool = False, extra: Optional[dict] = None):
    """make_input(first, n, n_pad) -> ops.WindowBatch of placements [first, first + n) padded to n_pad windows (so that every
    forward runs on ONE batch geometry and no second set of activation buffers is allocated).  tta: parsed codes -- every batch runs
    len(tta) forwards of that same geometry, their mean takes the place of the softmax in the merge.  extra: _Merge.finish's.  The rest:
    OutputPlan's values"""
    mg = _Merge(model, places, MH, MW, regression, int8_merge, rank, world, blend)
    t0 = time.perf_counter()
    batches = mg.plan.batches(rank, batch)
    n_pad = max((n for _, n in batches), default=0)
    acc = None      # the dense fp32 NHWC TTA accumulator [n_pad, h, w, C] of the call (re-made only when a batch of another tile size arrives)
    for first, n in batches:
        wb = make_input(first, n, n_pad)
        if tta is None:
            mg.add_batch(first, n, model.forward_windows(wb))
        else:
            mean = model.forward_tta(wb, n, tta, bool(regression), acc)
            acc = mean.buf
            mg.add_batch(first, n, mean, values=True)
    mg.exchange()
    if timing is not None and not int8_merge and mg.hi > mg.lo:      # coverage of this rank's strip (before the division consumes nothing of it)
        timing.update(hits_min=int(mg.count.min().item()), hits_max=int(mg.count.max().item()))
    out = mg.finish(want, postprocess, timing, keep, extra)
    if timing is not None:
        torch.cuda.synchronize()
        timing.update(seconds=time.perf_counter() - t0, windows_this_rank=sum(n for _, n in batches), windows=len(mg.plan.places),
                      active_ranks=mg.plan.active, strip_rows=mg.hi - mg.lo, slab_floats_sent=0 if mg.sendbuf is None else mg.sendbuf.numel())
    return out


def _dist_ctx():
    from unet_amd.distributed import init_from_env
    return init_from_env()


# ----------------------------------------------------------------------------------------------- configs[4]: a whole raster

def _check_windows(rows, th: int, tw: int, H: int, W: int, sources: int = 1):
    """host check of a window table before it is uploaded: every row (y0, x0[, source]) must cut a th x tw window out of one of
    `sources` H x W images -- the gather kernels are not told the raster's height and trust the table"""
    a = np.asarray(rows, dtype=np.int64).reshape(len(rows), -1)
    if not len(a):
        return
    src = a[:, 2] if a.shape[1] > 2 else np.zeros(len(a), dtype=np.int64)
    bad = (a[:, 0] < 0) | (a[:, 1] < 0) | (a[:, 0] + th > H) | (a[:, 1] + tw > W) | (src < 0) | (src >= sources)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"window {i} {a[i].tolist()} of {th} x {tw} px does not lie inside the {sources} source(s) of {H} x {W} px")


def _check_batch(first: int, n: int, n_pad: int, table_rows: int):
    """a batch reads table rows [first, first + n_pad) (n real windows, the rest repeats): they must exist"""
    if not (first >= 0 and 0 < n <= n_pad and first + n_pad <= table_rows):
        raise ValueError(f"batch of table rows [{first}, {first + n_pad}) (n = {n}) outside a table of {table_rows} rows")


def _raster_plan(wins: np.ndarray, size: int, H: int, W: int, batch_size: int):
    """kept windows (y0, x0) in merge order -> (placements [n, 4] in mosaic coordinates, MH, MW, oy, ox, gather-table rows in raster
    coordinates, padded at the end with batch_size repeats of the last window so that the last batch of any rank can be filled up)"""
    _check_windows(wins, size, size, H, W)
    oy, ox = int(wins[:, 0].min()), int(wins[:, 1].min())                          # extent of the tiles present (predict.py:259-270)
    MH, MW = int(wins[:, 0].max()) + size - oy, int(wins[:, 1].max()) + size - ox
    places = np.concatenate([wins - np.array([oy, ox]), np.full((len(wins), 2), size, dtype=np.int64)], axis=1)
    rows = wins.tolist() + [wins[-1].tolist()] * batch_size
    return places, MH, MW, oy, ox, rows


def predict_raster(model, raster, size: int = 512, overlap: float = 0.2, *, max_empty: float = 0.9, dtype: str = "int8", nodata=None,
                   regression: bool = False, all_classes: bool = False, specific_class: Optional[int] = None, large_file: bool = False,
                   batch_size: int = 16, out_path=None, class_zero: bool = False, timing: Optional[dict] = None,
                   batch_invariant: bool = False, tta=None, blend: str = "mean", postprocess=None, compress=None, predictor: int = 1,
                   return_array: bool = True, tile=None, overviews=None, vector_path=None, vector_exclude=None, vector_simplify=None,
                   instances=None, instances_path=None, zones_path=None, zonal_path=None, zonal_objects: bool = False,
                   objects_path=None, objects_exclude=None, zonal_values: bool = False, objects_values_path=None, objects_values_name: str = "value",
                   objects_confidence: bool = False):
    """Sliding-window prediction of a whole raster: equals split_raster(raster, patch_size=size, patch_overlap=overlap, max_empty) ->
    save_predictions(merge=True) on the tiles it writes (create_tiles_unet.py:252-434, predict.py:146-334).

    model    HipDynamicUnet (eval weights) or a Learner
    raster   path of a GeoTIFF, or an integer array [C, H, W] (numpy / torch, host or device)
    dtype    "int8" | "int16": the reference's DATATYPE switch -- int16 rasters are divided by 255 twice (utils.py:248-249 + IntToFloatTensor)
    batch_size  windows per forward launch.  Results are bit-reproducible for a FIXED batch_size (any rank count, any run); a different
             batch_size changes the launch grids and with them which deep-stage convs run as split reductions, i.e. the
             logits at rounding level (<= 2e-5 of the logit scale, tests/test_fullsize_gpu.py): masks can differ in numerical-tie pixels.
             The reference's own loop is batch 1 (predict.py:191-193)
    batch_invariant  True: every launch is planned as if its batch were ONE window (unet_tuning.plan_batch = 1), so each window runs exactly
             the kernels and split chains it would run alone: the result is bit-identical for every batch_size (and equals the
             tile-by-tile loop), at the price of batch-1 plans on full grids
    large_file  the reference's int8 merge (predict.py:209-214,288-289,324-329): probabilities as around(p * 31) in int8 rasters, int8 hit
             counters, integer floor division -- same numbers as save_predictions(merge=True, large_file=True)
    tta      None | "flips" | "d4" | a tuple of D4 codes (unet_amd/tta.py): test-time augmentation -- every window's probabilities (regression:
             values) are the mean of g^-1(f(g(window))) over the set, computed before the merge; the hit counter still counts windows
    blend    "mean" (the reference's merge: unweighted mean of the windows that cover a pixel) | "gaussian": every window's contribution
             is weighted with a centre-peaked Gaussian importance map (sigma = window side / 8, unet_amd/mosaic.py blend_profile) and the
             pixel is the weighted mean; not with large_file (ValueError)
    postprocess  None | PostProcess | dict of its arguments (unet_amd/postprocess.py): majority filter and / or small-region sieve of the
             merged class mask on the device, before it is returned / written; only for the class mask (not regression, all_classes,
             specific_class: ValueError); timing gains postprocess_seconds and postprocess (the sieve's info)
    compress  None | "lzw": out_path is written with LZW strips (predictor=2: horizontal differencing, integer outputs only).  The merged
             array is encoded on the device where it was assembled there (one rank, RCCL ranks) and only the compressed bytes reach the
             host; the int8 large_file merge and gloo ranks, which assemble on the host, use the host encoder -- the same file either way.
             timing gains write_seconds and file_bytes
    tile     None | a multiple of 16 in 16..1024 (256 is the usual choice; needs compress="lzw"): out_path is written as square LZW tiles
             instead of strips (tiffio.TileWriter)
    overviews  None | "auto" | "mode" | "average" | "nearest" (needs tile): the overview pyramid is written behind the full-resolution image,
             each level from the one before it down to the first that fits one tile -- a cloud-optimised GeoTIFF.  "auto": "mode" for a
             class mask, "average" for float probabilities, regression and the int8 large_file planes; "mode" on float outputs is refused.
             The pyramid is built and encoded on the device wherever the merged array is encoded there
    return_array  False (needs out_path): nothing is returned, and with compress="lzw" the merged array never goes to the host
    vector_path  None | path of a GeoJSON file: the class mask (after postprocess) is polygonized on the device of the rank that assembled it
             (unet_amd/vectorize.py: 4-connected components, one Polygon feature each, map coordinates of the output raster, the "crs"
             member from the raster's GeoKeyDirectory); only for the class mask and not with large_file (ValueError).  Under class_zero
             the NO_Data class 0 gets no polygon and the other ids are shifted as in the raster.  timing gains vector_seconds,
             vector_polygons and vector_vertices
    vector_exclude  None | int | iterable of class ids (the model's, before the class_zero shift) whose components get no polygon
    vector_simplify  None | a tolerance in pixels, 0..4096 (needs vector_path): the rings are simplified on the device before they are written,
             by a Douglas-Peucker on the arcs between the junctions of the borders, so that neighbouring polygons keep one common border
             (unet_amd/vectorize.py); polygons that shrink to fewer than 3 vertices get no feature.  timing gains vector_vertices_raw
    instances  None | Instances | dict of its arguments (unet_amd/instances.py: classes, radius=64, min_depth=2.0): touching objects of the
             named classes (the model's ids) are split into instances on the device, after postprocess and on the same tensor, so the
             result does not depend on the rank count.  Needs vector_path, instances_path or both; only for the class mask and not with
             large_file (ValueError).  With vector_path the GeoJSON has one feature per instance, with the added property `instance`, the
             id of the instance raster (0 for components of classes that are not split).  timing gains instances_seconds and instances
    instances_path  None | path of a uint32 GeoTIFF (needs instances): a dense id 1..N, in ascending label order, on every pixel of a
             split class and 0 elsewhere, with the geo tags of the mask; compress, predictor and tile apply to it (host encoder)
    zones_path / zonal_path  None | the path of a GeoJSON file of Polygon / MultiPolygon zones in the raster's coordinates, and the path of the
             table to write (.geojson: the zones with their geometry and properties; .csv: one row per zone); both or neither (ValueError).
             The zones are burnt onto the output grid on the device (the rasterizer's rules: pixel centre, even-odd, the last zone wins) and
             the pixels of every class per zone are counted there (unet_amd/zonal.py: pixels, area, px_<class>, frac_<class>, majority per
             zone); only for the class mask and not with large_file (ValueError); a zones file whose EPSG code differs from the raster's
             is refused (no reprojection).  timing gains zonal_seconds, zonal_zones and zonal_pixels
    zonal_objects  True (needs zones_path): also n_<class>, the objects per zone and class -- the instances with instances=, else the
             4-connected components; an object counts in the zone that holds its first pixel in row-major order
    objects_path  None | the path of a .geojson or .csv file: every object of the class mask (after postprocess) -- the instances with
             instances=, else the 4-connected components -- is measured on the device (unet_amd/objects.py: pixels, area, perimeter,
             centroid, bbox, diameter, compactness, on_edge and one representative pixel inside the object) and written as one Point
             feature (or one row) per object in map coordinates; with vector_path the polygon features carry the same attributes.  Only
             for the class mask and not with large_file (ValueError).  Under class_zero the NO_Data class 0 is not measured.  timing gains
             objects_seconds and objects
    objects_exclude  None | int | iterable of class ids (the model's, before the class_zero shift) whose objects are not measured
    zonal_values  True (needs zones_path): the table summarises the one float plane of the output instead of the class mask -- regression
             (nodata -9999 is not a valid pixel) or specific_class -- as pixels, area, valid, mean, std, min, max and sum per zone, summed
             on the device in fixed point so that the table does not depend on scheduling (unet_amd/zonal.py); not for the class mask,
             all_classes, large_file or with zonal_objects (ValueError)
    objects_values_path  None | the path of a one-band GeoTIFF on the OUTPUT's grid (needs objects_path): a canopy height model, an NDVI, a slope.
             Every object gains <objects_values_name>_valid, _mean, _std, _sum, _min, _max and _peak_x, _peak_y, the centre of the pixel where
             the value peaks (the treetop), summed on the device in fixed point (unet_amd/objects.py, object_values).  The raster must have
             the output's height, width and six geotransform numbers exactly (ValueError names both grids; there is no resampling; where the
             input is an array, so that the output has no georeference, the shape alone is compared); float32 is taken as it is, uint8, uint16
             and int16 are converted (exactly), anything else is refused; nodata comes from the file.  Rank 0 reads it and uploads it once.
             timing gains objects_values_seconds
    objects_values_name  the prefix of those columns ("value"; e.g. "height")
    objects_confidence  True (needs objects_path): every object gains confidence_valid, _mean, _std, _sum, _min, _max, _peak_x, _peak_y of the
             merged probability of the class that the merge chose at each pixel -- the maximum over the classes of the finalised mosaic,
             before postprocess (a pixel that postprocess moved to another class keeps the probability of the class it had; a pixel that no
             window covered holds 0.0).  The plane exists only with this option
    Returns on rank 0 the merged array (uint8 argmax [H', W'] by default; float32 [C, H', W'] for all_classes; one float32 plane for
    specific_class / regression; int8 planes with large_file) where H' x W' is the extent of the kept windows, None on the other ranks;
    with out_path it is also written as a GeoTIFF (class_zero shifts the class ids back, predict.py:19-52)."""
    if (zones_path is None) != (zonal_path is None):
        raise ValueError("zones_path and zonal_path go together: the zones to read and the table to write")
    plan = check_outputs(regression, all_classes, specific_class, large_file, True, class_zero, blend, postprocess, compress, predictor, tile,
                         overviews, vector_path, vector_exclude, vector_simplify, instances, instances_raster=instances_path is not None,
                         raster=out_path is not None, return_array=return_array, raster_arg="instances_path", objects=objects_path,
                         objects_exclude=objects_exclude, zones=zones_path, zonal_objects=zonal_objects,
                         zonal_values=zonal_values, objects_values=objects_values_path, objects_values_name=objects_values_name,
                         objects_confidence=objects_confidence)
    model = getattr(model, "model", model)
    codes = tta_codes(tta, [(size, size)])
    rank, _, world = _dist_ctx()
    dev = model._device
    gt, tags = None, {}
    if isinstance(raster, (str, os.PathLike)):
        arr, meta = read_tiff(raster)
        gt, tags = meta["geotransform"], meta["tags"]
        nodata = meta.get("nodata") if nodata is None else nodata
        raster = arr[None] if arr.ndim == 2 else arr
    if isinstance(raster, np.ndarray):
        raster = torch_samples(raster)
    if raster.dim() == 2:
        raster = raster[None]
    if raster.dtype not in ops.RASTER_TYPES:
        raster = raster.to(torch.int32)
    data = raster.to(dev).contiguous()
    if nodata is not None and data.data_ptr() == raster.data_ptr():
        data = data.clone()                                                        # never modify the caller's tensor
    src = ops.WindowSource(data, div255_twice=(dtype == "int16"))
    if nodata is not None:
        ops.raster_nodata_zero(src, nodata)                                        # create_tiles_unet.py:344-352
    Cb, H, W = src.C, src.H, src.W
    wins = sliding_windows(H, W, size, overlap)                                    # create_tiles_unet.py:52-54
    _check_windows(wins, size, size, H, W)
    table_all = ops.window_table(wins.tolist(), dev)
    nz = ops.window_nonzero(src, table_all, size, size).cpu().numpy()
    keep = keep_windows(nz, Cb, size, size, max_empty)                             # create_tiles_unet.py:379
    wins = wins[keep]
    if len(wins) == 0:
        raise ValueError("every window of the raster is emptier than max_empty: nothing to predict")
    places, MH, MW, oy, ox, rows = _raster_plan(wins, size, H, W, batch_size)
    gtab = ops.window_table(rows, dev)
    ogt = None if gt is None else [gt[0] + ox * gt[1], gt[1], 0.0, gt[3] + oy * gt[5], 0.0, gt[5]]
    planes = {}
    if plan.objects_values is not None and rank == 0:          # read and checked before the merge, uploaded once
        values, values_nodata = read_value_raster(objects_values_path, (MH, MW), ogt)
        planes[plan.objects_values] = (torch.from_numpy(values).to(dev), values_nodata)

    def make_input(first, n, n_pad):
        _check_batch(first, n, n_pad, len(rows))
        return ops.WindowBatch(src, gtab, first, n_pad, size, size)

    more = {"extra": {}} if plan.objects_confidence else {}          # without the option: the call it was
    with (ops.tuning(plan_batch=1) if batch_invariant else contextlib.nullcontext()):
        out = _run_merge(model, places, MH, MW, plan.regression, plan.int8_merge, rank, world, batch_size, make_input, plan.want, timing, codes,
                         plan.blend, plan.postprocess, plan.keep, **more)
    if rank == 0:
        if plan.objects_confidence:
            planes["confidence"] = (more["extra"]["confidence"], None)
        out = _write_outputs(plan, out, dev, ogt, tags, out_path, vector_path, instances_path, None, timing, zones_path, zonal_path, objects_path,
                             planes or None)
    if timing is not None:
        timing.update(kept_windows=len(wins), all_windows=int(len(keep)), mosaic=(MH, MW))
    if rank != 0 or not return_array:
        return None
    return out.cpu().numpy() if isinstance(out, torch.Tensor) else out


# ----------------------------------------------------------------------------------------------- tile files: decode ahead of the GPU

class _Prefetcher:
    """What the prediction loops ask of a tile prefetcher.  Iteration yields (first, n, device buffer [n_pad, C, h, w]) per batch of tiles
    [first, first + n), as the integer samples the files hold (rows beyond n: leftovers of an earlier batch, their windows are dropped);
    done() after the last kernel that reads the buffer yielded last has been issued; close() -- or leaving the with block -- ends the decode
    threads, also under a consumer that stops early."""

    def done(self):
        pass

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _TilePrefetcher(_Prefetcher):
    """A thread decodes the tile files of the coming batches into pinned host buffers; the main thread uploads the integer samples
    (asynchronous copy) and cuts / scales them on the device.  A pinned buffer goes back to the producer with the event recorded behind its
    upload, the producer waits for that event before it overwrites the buffer.  Serves tile sets of MIXED sizes (a batch is one size)."""

    def __init__(self, tiles: Sequence[Path], batches: List[Tuple[int, int]], device, depth: int = 3):
        self.tiles, self.batches, self.device = tiles, batches, device
        self.n_pad = max((n for _, n in batches), default=0)
        self.q: "queue.Queue" = queue.Queue(maxsize=depth)
        self.depth = depth
        self._free, self._made = {}, {}
        self.err = None
        self._stop = False
        self.t = threading.Thread(target=self._work, daemon=True)
        self.t.start()

    def _buf(self, key, shape, dt):
        fq = self._free.setdefault(key, queue.Queue())
        if fq.empty() and self._made.get(key, 0) < self.depth + 2:
            self._made[key] = self._made.get(key, 0) + 1
            return torch.empty(shape, dtype=dt, pin_memory=torch.cuda.is_available())
        buf, ev = fq.get()
        if ev is not None:
            ev.synchronize()
        return buf

    def _work(self):
        # tile files are decoded by a small pool (file read, strip copies and the band de-interleave release the GIL), `depth` batches ahead
        from concurrent.futures import ThreadPoolExecutor
        try:
            with ThreadPoolExecutor(max_workers=min(8, default_workers())) as ex:
                load = lambda path: torch_samples(open_tile(path))
                pending, nxt = [], 0
                for bi, (first, n) in enumerate(self.batches):
                    if self._stop:
                        break
                    while nxt < len(self.batches) and nxt <= bi + self.depth:
                        f0, n0 = self.batches[nxt]
                        pending.append([ex.submit(load, self.tiles[f0 + j]) for j in range(n0)])
                        nxt += 1
                    self._emit(first, n, [f.result() for f in pending.pop(0)])
            self.q.put(None)
        except BaseException as e:      # noqa: BLE001  (surfaces in the consumer)
            self.err = e
            self.q.put(None)

    def _emit(self, first, n, samples):
        t0 = samples[0]
        buf = self._buf((tuple(t0.shape), t0.dtype), (self.n_pad,) + tuple(t0.shape), t0.dtype)
        for j, t in enumerate(samples):
            buf[j].copy_(t)
        self.q.put((first, n, buf))

    def __iter__(self):
        while True:
            it = self.q.get()
            if it is None:
                if self.err is not None:
                    raise self.err
                return
            first, n, buf = it
            yield first, n, self._upload(buf)

    def _upload(self, buf: torch.Tensor) -> torch.Tensor:
        """asynchronous host -> device copy of a filled buffer; the buffer goes back to the producer behind the copy"""
        d = buf.to(self.device, non_blocking=True)
        ev = None
        if d.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
        self._free[(tuple(buf.shape[1:]), buf.dtype)].put((buf, ev))
        return d

    def close(self):
        """the producer stops after the batch it is working on; what it still queues is dropped, so that it never waits on a full queue"""
        self._stop = True
        while self.t.is_alive():
            with contextlib.suppress(queue.Empty):
                self.q.get(timeout=0.05)


class _FeedPrefetcher(_Prefetcher):
    """The same on the training feed's machinery (unet_amd/feed.py): every pool task reads ONE tile file and copies it straight into
    its slot of a pinned staging buffer (the producer thread above copies the 16 tiles of a batch one after the other), uploads go out on a
    copy stream one batch ahead.  For tile sets of one height x width -- what split_raster writes (a tile with other bands or another sample
    type makes the feeder raise); sets of mixed sizes keep _TilePrefetcher."""

    def __init__(self, tiles: Sequence[Path], batches: List[Tuple[int, int]], device, depth: int = 3):
        self.tiles, self.batches = tiles, batches
        self.n_pad = max((n for _, n in batches), default=0)
        self.feeder = BatchFeeder(lambda i: (open_tile(self.tiles[i]),), self.n_pad, device, depth=depth)
        self._slot = None           # the staging slot of the batch yielded last, until done()

    def __iter__(self):
        for (first, n), self._slot in zip(self.batches, self.feeder.run([range(first, first + n) for first, n in self.batches])):
            yield first, n, self._slot.dev[0]

    def done(self):
        if self._slot is not None:
            self._slot.release()
            self._slot = None

    def close(self):
        self.feeder.close()


def _prefetcher(tiles, batches, sizes, device):
    """_FeedPrefetcher when every tile has the same height x width, else the general one"""
    if len(set(sizes)) == 1 and device.type == "cuda":
        return _FeedPrefetcher(tiles, batches, device)
    return _TilePrefetcher(tiles, batches, device)


def _tile_windows(batch_size: int, device, div255_twice: bool) -> Callable:
    """-> windows(d, n): a staged device buffer d [n_pad, C, h, w] whose first n tiles are real, as the checked ops.WindowBatch of its
    n_pad whole tiles (window j = tile j from its corner).  The table of batch_size rows is uploaded once per call."""
    zrows = [[0, 0, j, 0] for j in range(batch_size)]
    ztab = ops.window_table(zrows, device)

    def windows(d: torch.Tensor, n: int) -> ops.WindowBatch:
        n_pad, _, h, w = d.shape
        _check_batch(0, n, n_pad, len(zrows))
        _check_windows(zrows[:n_pad], h, w, h, w, sources=n_pad)
        return ops.WindowBatch(ops.WindowSource(d, div255_twice=div255_twice), ztab, 0, n_pad, h, w)
    return windows


def save_predictions(predict_model, predict_path, regression, merge=False, all_classes=False, specific_class=None, large_file=False,
                     AOI=None, year=None, validation_vision=True, class_zero=False, batch_size=16, timing: Optional[dict] = None,
                     batch_invariant: bool = False, tta=None, blend: str = "mean", postprocess=None, compress=None, predictor: int = 1,
                     tile=None, overviews=None, vector: bool = False, vector_exclude=None, vector_simplify=None, instances=None,
                     instances_raster: bool = False, zones=None, zonal_objects: bool = False, objects: bool = False, objects_exclude=None,
                     zonal_values: bool = False, objects_values=None, objects_values_name: str = "value", objects_confidence: bool = False):
    """tta, blend, postprocess, compress / predictor, tile / overviews, vector_exclude, vector_simplify and instances are predict_raster's (see
    there); the ValueErrors of check_outputs come before the model is loaded.  What differs here: tta applies to merged and per-tile outputs
    alike; blend, postprocess, vector and instances need merge=True (per-tile outputs: no overlap to blend, not post-processed, polygonized, split).
    compress / predictor: the merged raster is encoded where the merge assembled it (on the device with one rank or RCCL); per-tile outputs
    (merge=False) use the host encoder.  tile / overviews: of the MERGED raster only; per-tile outputs ignore them, as a tile is one block anyway.
    vector (predict_raster's vector_path): True writes <merged raster stem>.geojson beside the merged raster, with the class names of the
    model's vocab.  instances_raster (predict_raster's instances_path): True writes <merged raster stem>_instances.tif beside it; instances
    needs vector=True, instances_raster=True, zones or any of them.  zones (predict_raster's zones_path, with zonal_objects): the path of the
    zones file; the table is written as <merged raster stem>_zonal.geojson beside the merged raster, with the class names of the vocab.
    objects (predict_raster's objects_path, with objects_exclude): True writes <merged raster stem>_objects.geojson beside the merged raster,
    one Point feature per object with its attributes and the class names of the vocab; it counts as an output of instances.
    zonal_values (predict_raster's, needs zones and merge=True): <merged raster stem>_zonal.geojson holds the statistics of the float plane.
    objects_values (predict_raster's objects_values_path: the path of the value raster, on the merged raster's grid), objects_values_name and
    objects_confidence need objects=True; the columns join <merged raster stem>_objects.geojson and, with vector=True, the polygon features.
    validation_vision is accepted and ignored: the per-tile majority-class confusion plots (predict.py:56-143) are reporting, out of scope"""
    plan = check_outputs(regression, all_classes, specific_class, large_file, merge, class_zero, blend, postprocess, compress, predictor, tile,
                         overviews, vector or None, vector_exclude, vector_simplify, instances, instances_raster, objects=objects or None,
                         objects_exclude=objects_exclude, zones=zones, zonal_objects=zonal_objects,
                         zonal_values=zonal_values, objects_values=objects_values, objects_values_name=objects_values_name,
                         objects_confidence=objects_confidence)
    rank, local_rank, world = _dist_ctx()
    learn = load_learner(Path(predict_model), device=f"cuda:{local_rank}" if world > 1 else "cuda")
    model = learn.model
    path = Path(predict_path)
    output_folder = path.parent if merge else path.parent / ("predicted_tiles_" + Path(predict_model).stem)
    if rank == 0:
        output_folder.mkdir(parents=True, exist_ok=True)
    model_name = os.path.basename(predict_model).split(".")[0]
    tiles = sorted([p for p in path.iterdir() if p.suffix.lower() in (".tif", ".tiff", ".npy")])
    if rank == 0:
        print(f"Started at: {time.strftime('%H:%M:%S')}  ({len(tiles)} tiles)")
    geos = [_geo(t) for t in tiles]
    codes = tta_codes(tta, [(g[2], g[3]) for g in geos])
    t_start = time.perf_counter()
    windows = _tile_windows(batch_size, model._device, learn.dls.train_ds.dtype == "int16")
    if merge:
        extra = {} if plan.objects_confidence else None
        out, gt = _save_merged(model, tiles, geos, windows, rank, world, plan, batch_size, batch_invariant, codes, timing, extra)
    else:
        _save_tiles(model, tiles, geos, windows, rank, world, output_folder, plan, batch_size, batch_invariant, codes)
        if world > 1:
            _dist().barrier()
    if timing is not None:
        timing["tiles_per_s_end_to_end"] = len(tiles) / (time.perf_counter() - t_start)
    if not merge:
        if rank == 0:
            print(f"Prediction stored in {output_folder}.")
        return output_folder
    if rank != 0:
        return None
    name = "_".join(filter(None, [AOI, year, model_name, "prediction"])) + ".tif"
    vocab = getattr(learn.dls, "vocab", None) if plan.vector is not None or plan.zones or plan.objects is not None else None
    names = list(vocab) if vocab is not None and len(vocab) >= model.n_out else None
    planes = {}
    if plan.objects_values is not None:
        values, values_nodata = read_value_raster(objects_values, tuple(out.shape), gt)
        planes[plan.objects_values] = (torch.from_numpy(values).to(model._device), values_nodata)
    if plan.objects_confidence:
        planes["confidence"] = (extra["confidence"], None)
    _write_outputs(plan, out, model._device, gt, geos[0][1], output_folder / name, (output_folder / name).with_suffix(".geojson"),
                   output_folder / (Path(name).stem + "_instances.tif") if plan.instances_raster else None, names, timing,
                   zones, output_folder / (Path(name).stem + "_zonal.geojson") if plan.zones else None,
                   output_folder / (Path(name).stem + "_objects.geojson") if plan.objects is not None else None, planes or None)
    print(f"Prediction stored in {output_folder}.")
    return output_folder if regression else output_folder / name


def _save_merged(model, tiles, geos, windows: Callable, rank, world, plan: OutputPlan, batch_size, batch_invariant, codes, timing, extra=None):
    """overlap merge (predict.py:257-355) of this rank's share of the tiles -> (merged array on rank 0, None elsewhere; geotransform of
    the mosaic).  The extent follows from the tiles' geotransforms and sizes, which are known from the headers BEFORE any tile is
    predicted: every batch is accumulated into the device mosaic as soon as it is computed and its probabilities are dropped (the
    reference keeps all tiles' probabilities until the end).  extra: _Merge.finish's."""
    if any(g[0] is None for g in geos):
        raise ValueError("merge=True needs georeferenced tiles (.npy tiles carry no geotransform)")
    gts = np.array([[g[0][0], g[3], g[0][1], g[0][3], g[2], g[0][5]] for g in geos], dtype=np.float64)
    ulx_full, uly_full = gts[:, 0].min(), gts[:, 3].max()
    xres, yres = gts[0, 2], gts[0, 5]
    xmax_i, ymin_i = gts[:, 0].argmax(), gts[:, 3].argmin()
    lrx_full = gts[:, 0].max() + gts[xmax_i, 1] * gts[xmax_i, 2]
    lry_full = gts[:, 3].min() + gts[ymin_i, 4] * gts[ymin_i, 5]
    if len(set(gts[:, 1])) != 1 or len(set(gts[:, 4])) != 1:
        warnings.warn("Not all tiles have the same resolution.")
    MW, MH = round((lrx_full - ulx_full) / xres), round((lry_full - uly_full) / yres)
    if rank == 0:
        print(f"True merged raster size: {model.n_out * MH * MW * (1 if plan.int8_merge else 4) / (1024 ** 2): .1f}MB.")
    places = np.array([[round((gts[i, 3] - uly_full) / yres), round((gts[i, 0] - ulx_full) / xres), geos[i][2], geos[i][3]]
                       for i in range(len(tiles))], dtype=np.int64)
    order = merge_order(places)
    places, tiles_o = places[order], [tiles[i] for i in order]
    batches = MergePlan(places, MH, MW, world).batches(rank, batch_size)
    sizes = [(int(p_[2]), int(p_[3])) for p_ in places]
    # (the decode pool and its pinned ring live for one call)
    with _prefetcher(tiles_o, batches, sizes, model._device) as pf, contextlib.closing(iter(pf)) as feed:
        def make_input(first, n, n_pad):
            pf.done()          # staging of the batch in flight: released once the NEXT batch is asked for (its gather has been issued by then)
            f, nn, d = next(feed)
            assert (f, nn) == (first, n) and d.shape[0] == n_pad, ((f, nn, d.shape[0]), (first, n, n_pad))
            return windows(d, n)

        with (ops.tuning(plan_batch=1) if batch_invariant else contextlib.nullcontext()):          # (see predict_raster)
            more = {} if extra is None else {"extra": extra}          # without the option: the call it was
            out = _run_merge(model, places, MH, MW, plan.regression, plan.int8_merge, rank, world, batch_size, make_input, plan.want, timing, codes,
                         plan.blend, plan.postprocess, plan.keep, **more)
    return out, [ulx_full, xres, 0.0, uly_full, 0.0, yres]


def _save_tiles(model, tiles, geos, windows: Callable, rank, world, output_folder, plan: OutputPlan, batch_size, batch_invariant, codes):
    """one output file per tile (predict.py:224-254); tile i -> rank i mod world"""
    dev, C = model._device, model.n_out
    mine = list(range(rank, len(tiles), world))
    sizes = [(geos[i][2], geos[i][3]) for i in mine]
    batches, i = [], 0
    while i < len(mine):
        n = 1
        while n < batch_size and i + n < len(mine) and sizes[i + n] == sizes[i]:
            n += 1
        batches.append((i, n))
        i += n
    mtiles = [tiles[i] for i in mine]
    need_p = not plan.mask
    acc = None      # the TTA accumulator, used again by every batch of the same tile size (see _run_merge)
    with _prefetcher(mtiles, batches, sizes, dev) as pf:
        for first, n, d in pf:
            wb = windows(d, n)
            h, w = d.shape[2], d.shape[3]
            probs = torch.empty((n, C, h, w), dtype=torch.float32, device=dev) if need_p else None
            amax = None if need_p else torch.empty((n, h, w), dtype=torch.int64, device=dev)
            with (ops.tuning(plan_batch=1) if batch_invariant else contextlib.nullcontext()):
                if codes is None:
                    z = model.forward_windows(wb)
                else:                # TTA: the finalising accumulate writes the mean probabilities (values) / their argmax
                    acc = model.forward_tta(wb, n, codes, plan.regression, acc, probs, amax).buf
            pf.done()                  # (the gather that reads the staging buffer has been issued)
            if codes is None:
                zs = ops.TS(z.buf[:n], z.co, z.C)
                if plan.regression:       # predict.py:195-197: tile_preds[1] = raw outputs [1,H,W]
                    ops.nhwc_to_nchw(zs, probs)
                else:
                    ops.softmax_argmax(zs, probs, amax)
            outs = (probs if probs is not None else amax.to(torch.uint8)).cpu().numpy()
            for j in range(n):
                t = mtiles[first + j]
                gt, tags = geos[mine[first + j]][0], geos[mine[first + j]][1]
                out = outs[j] if plan.regression or plan.all_classes or plan.specific_class is None else outs[j, plan.specific_class]
                if plan.large_file and out.dtype.kind == "f" and out.max() <= 1 and (plan.all_classes or plan.specific_class):
                    out = np.around(out * LARGE_FILE_SCALE).astype(np.int8)
                name = t.name if t.suffix != ".npy" else t.stem + ".tif"
                store_tif(output_folder / name, out, gt, tags, None, plan.class_zero, plan.compress, plan.predictor)
