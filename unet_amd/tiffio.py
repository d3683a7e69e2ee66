"""Minimal GeoTIFF reader / writer (no GDAL, no rasterio, no tifffile: none of them is installed here).

Covers what the tile workflow of the reference needs (``data.py:18-28`` reads tiles with rasterio, ``predict.py:19-52``
writes them with GDAL; ``create_tiles_unet.py:252-434`` opens whole scenes with GDAL): classic TIFF and BigTIFF, little/big endian,
strips or tiles, chunky or planar, 8/16/32/64-bit unsigned / signed / float samples, the compressions GDAL writes by default or
on request -- none, LZW (5), Deflate (8 / 32946), PackBits (32773) -- with horizontal differencing (Predictor 2), plus the GeoTIFF
georeferencing tags (ModelPixelScale 33550, ModelTiepoint 33922, GeoKeyDirectory 34735, GeoDoubleParams 34736, GeoAsciiParams
34737, GDAL_NODATA 42113) which are passed through verbatim.  Floating-point differencing (Predictor 3) is undone on float samples.
JPEG-in-TIFF (Compression 7 with the JPEGTables tag: baseline 8-bit, what GDAL's COMPRESS=JPEG writes; PhotometricInterpretation 6 comes back
as RGB, as it does from GDAL) is decoded to the bytes libtiff + libjpeg produce (csrc/host/tiff_jpeg.cpp).  Anything else (old-style JPEG 6,
12-bit / progressive JPEG, CCITT, ...) raises loudly.
The byte-oriented decoders are C functions (csrc/tiff_codecs.hip: in libunet_hip.so, and linked by g++ alone -- together with the JPEG
decoder -- into the host-only libunet_tiff.so); files are memory-mapped for reading and written uncompressed, or with compress="lzw" as
LZW strips (unet_tiff_lzw_encode in the same file; StripWriter is the layout, shared with the device encoder of unet_amd/tiffenc.py).
"""
from __future__ import annotations

import struct
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np

_TYPES = {1: ("B", 1), 2: ("c", 1), 3: ("H", 2), 4: ("I", 4), 5: ("II", 8), 6: ("b", 1), 7: ("B", 1), 8: ("h", 2), 9: ("i", 4),
          10: ("ii", 8), 11: ("f", 4), 12: ("d", 8), 16: ("Q", 8), 17: ("q", 8), 18: ("Q", 8)}
GEO_TAGS = (33550, 33922, 34735, 34736, 34737, 42113)


def _dtype(bits: int, fmt: int, bo: str) -> np.dtype:
    kind = {1: "u", 2: "i", 3: "f"}.get(fmt, "u")
    return np.dtype(f"{bo}{kind}{bits // 8}")


def _header(b, path):
    """(offset of IFD 0, BigTIFF?, byte-order prefix) of a TIFF: classic (magic 42, 32-bit offsets) or BigTIFF (magic 43, 64-bit)"""
    bo = {b"II": "<", b"MM": ">"}[bytes(b[:2])]
    magic = struct.unpack(bo + "H", b[2:4])[0]
    if magic == 42:
        return struct.unpack(bo + "I", b[4:8])[0], False, bo
    if magic == 43:
        osz, zero = struct.unpack(bo + "HH", b[4:8])
        if osz != 8 or zero != 0:
            raise NotImplementedError(f"{path}: BigTIFF with offset size {osz}")
        return struct.unpack(bo + "Q", b[8:16])[0], True, bo
    raise NotImplementedError(f"{path}: not a TIFF (magic {magic})")


def _parse_tags(b, path, level: int = 0):
    """IFD `level` of a TIFF held in a bytes-like object (bytes or mmap): {tag: values}, byte-order prefix.  level 0 reads the first IFD
    alone; a higher level walks the chain (_ifd_offsets)."""
    off, big, bo = _header(b, path)
    if level:
        offs = _ifd_offsets(b, path, off, big, bo)
        if level >= len(offs):
            raise ValueError(f"{path}: level {level} of a file with {len(offs)} image(s)")
        off = offs[level]
    return _parse_ifd(b, path, off, big, bo), bo


def _parse_ifd(b, path, off: int, big: bool, bo: str) -> Dict[int, tuple]:
    if big:
        n = struct.unpack(bo + "Q", b[off:off + 8])[0]
        base, esz, cfmt, inl = off + 8, 20, "Q", 8
    else:
        n = struct.unpack(bo + "H", b[off:off + 2])[0]
        base, esz, cfmt, inl = off + 2, 12, "I", 4
    if base + esz * n > len(b):
        raise ValueError(f"{path}: the IFD at offset {off} holds {n} entries: past the end of the file ({len(b)} bytes)")
    tags: Dict[int, tuple] = {}
    for i in range(n):
        e = bytes(b[base + esz * i: base + esz * (i + 1)])
        tag, typ = struct.unpack(bo + "HH", e[:4])
        cnt = struct.unpack(bo + cfmt, e[4:4 + inl])[0]
        if typ not in _TYPES:
            continue
        fmt, sz = _TYPES[typ]
        total = sz * cnt
        if total <= inl:
            data = e[4 + inl:4 + inl + total]
        else:
            o = struct.unpack(bo + cfmt, e[4 + inl:4 + 2 * inl])[0]
            if o + total > len(b):          # (a damaged count would otherwise become a format string of that many characters)
                raise ValueError(f"{path}: tag {tag} holds {cnt} values at offset {o}: past the end of the file ({len(b)} bytes)")
            data = bytes(b[o:o + total])
        if typ == 2:
            tags[tag] = (data.rstrip(b"\0").decode("latin1"),)
        else:
            tags[tag] = struct.unpack(bo + fmt[0] * (cnt * len(fmt)), data)
    return tags


def _ifd_offsets(b, path, first: int, big: bool, bo: str):
    """the offsets of the chained IFDs, first to last.  The chain is user data: an IFD (its count, entries and next pointer) must lie
    inside the file, and an offset that was already visited -- a cycle -- is refused.  Every IFD takes at least 6 bytes of its own, so
    the walk ends after at most len(b) / 6 steps."""
    cnt_fmt, cnt_sz, esz, nxt_fmt, nxt_sz = ("Q", 8, 20, "Q", 8) if big else ("H", 2, 12, "I", 4)
    offs, seen, off = [], set(), first
    while off:
        if off in seen:
            raise ValueError(f"{path}: the IFD chain returns to offset {off}: a cycle")
        if off + cnt_sz > len(b):
            raise ValueError(f"{path}: IFD {len(offs)} at offset {off} lies past the end of the file ({len(b)} bytes)")
        n = struct.unpack(bo + cnt_fmt, b[off:off + cnt_sz])[0]
        end = off + cnt_sz + esz * n
        if end + nxt_sz > len(b):
            raise ValueError(f"{path}: IFD {len(offs)} at offset {off} holds {n} entries: past the end of the file ({len(b)} bytes)")
        seen.add(off)
        offs.append(off)
        off = struct.unpack(bo + nxt_fmt, b[end:end + nxt_sz])[0]
    return offs


_codec_lib = None


def _codecs():
    """the two byte-oriented TIFF decoders and the LZW encoder (csrc/tiff_codecs.hip: plain C++, no device code).  ``python -m unet_amd.build`` also links them
    into a host-only ``libunet_tiff.so`` (g++), so a tile-preparation box without the HIP runtime reads the rasters GDAL writes by default;
    libunet_hip.so exports the same symbols."""
    global _codec_lib
    if _codec_lib is None:
        import ctypes as C
        from ._abi import signatures
        here = Path(__file__).resolve().parent
        host, include = here / "lib" / "libunet_tiff.so", here.parent / "include"
        if host.exists():
            lib = C.CDLL(str(host))
        else:
            from ._lib import lib
        sig = signatures(include / "unet_hip.h", {}, only=("unet_tiff_lzw_decode", "unet_tiff_packbits_decode", "unet_tiff_lzw_encode"))
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        try:                       # include/unet_tiff.h: the JPEG decoder lives in the host-only library alone
            fn = lib.unet_tiff_jpeg_decode
            fn.restype, fn.argtypes = signatures(include / "unet_tiff.h", {})["unet_tiff_jpeg_decode"]
            lib.has_jpeg = True
        except AttributeError:     # libunet_hip.so, or a libunet_tiff.so built before the decoder existed
            lib.has_jpeg = False
        _codec_lib = lib
    return _codec_lib


def _threads() -> int:
    """threads of the strip decode / encode pools: from the CPU affinity (2..8), UNET_TIFF_THREADS overrides"""
    import os
    try:
        nthr = max(2, min(8, len(os.sched_getaffinity(0))))
    except (AttributeError, OSError):
        nthr = 4
    return int(os.environ.get("UNET_TIFF_THREADS", nthr))


def _decoder(comp: int, path):
    """(uint8 array view of one compressed strip / tile, capacity) -> decoded bytes (a uint8 array of at most `cap` bytes)"""
    if comp == 1:
        return lambda raw, cap: raw
    if comp in (8, 32946):
        import zlib

        def inflate(raw, cap):
            d = zlib.decompressobj()
            out = d.decompress(raw, cap)                   # bounded: a crafted strip cannot expand beyond what the image needs
            if d.unconsumed_tail and d.decompress(d.unconsumed_tail, 1):
                raise ValueError(f"{path}: Deflate strip decodes to more than the {cap} bytes its rows hold")
            return np.frombuffer(out, dtype=np.uint8)
        return inflate
    if comp in (5, 32773):
        lib = _codecs()
        fn = lib.unet_tiff_lzw_decode if comp == 5 else lib.unet_tiff_packbits_decode

        def dec(raw, cap):
            src = np.ascontiguousarray(raw)
            dst = np.empty(cap, dtype=np.uint8)
            got = fn(src.ctypes.data, src.size, dst.ctypes.data, cap)       # (ctypes releases the GIL: the feed's decode pool runs these in parallel)
            if got < 0:
                raise ValueError(f"{path}: corrupt {'LZW' if comp == 5 else 'PackBits'} data")
            return dst[:got]
        return dec
    raise NotImplementedError(f"{path}: TIFF compression {comp} is not supported (none, LZW, Deflate, PackBits and new-style JPEG (7) are)")


def _jpeg_decoder(tags, path):
    """(compressed strip / tile, rows, cols, samples per pixel) -> uint8 [rows', cols', samples] with the frame size the JPEG stream itself states
    (libtiff writes a short last strip as a short frame, tiles always whole).  TIFF Technical Note 2: tag 347 holds the shared tables."""
    import ctypes as C
    lib = _codecs()
    if not lib.has_jpeg:
        raise RuntimeError(f"{path}: JPEG-in-TIFF needs unet_amd/lib/libunet_tiff.so (python -m unet_amd.build)")
    tables = np.array(tags[347], dtype=np.uint8) if 347 in tags else None
    ycc = 1 if tags.get(262, (1,))[0] == 6 else 0

    import threading
    tl = threading.local()          # one output buffer per decoding thread (a fresh >= 128 KB array per strip is an mmap + its page faults, and
                                    # those serialise the threads of a large scene); the caller copies the block out before its next call

    def dec(raw, rows, cols, pix):
        src = np.ascontiguousarray(raw)
        cap = rows * cols * pix
        dst = getattr(tl, "buf", None)
        if dst is None or dst.size < cap:
            dst = tl.buf = np.empty(cap, dtype=np.uint8)
        dims = (C.c_int * 3)()
        got = lib.unet_tiff_jpeg_decode(None if tables is None else tables.ctypes.data, 0 if tables is None else tables.size, src.ctypes.data,
                                        src.size, ycc, dst.ctypes.data, cap, dims)
        if got == -2:
            raise NotImplementedError(f"{path}: this JPEG process is not supported (baseline / extended sequential Huffman, 8 bit, "
                                      f"chroma at 1:1, 2:1 horizontally or 2:1 in both directions are)")
        h, w, c = dims
        if got < 0 or c != pix or h > rows or w > cols:
            raise ValueError(f"{path}: corrupt JPEG strip / tile (decoder returned {got}, frame {h} x {w} x {c} for a {rows} x {cols} x {pix} block)")
        return dst[:got].reshape(h, w, c)
    return dec


def _unpredict(block: np.ndarray, predictor: int, path) -> np.ndarray:
    """undo Predictor 2 (horizontal differencing per sample, TIFF 6.0 section 14) on a [rows, width, samples] block"""
    if predictor == 1:
        return block
    if predictor != 2 or block.dtype.kind == "f":
        raise NotImplementedError(f"{path}: TIFF predictor {predictor} on {block.dtype} is not supported")
    return np.cumsum(block, axis=1, dtype=block.dtype)


def _unpredict_float(raw: np.ndarray, rows: int, cols: int, pix: int, dt: np.dtype) -> np.ndarray:
    """undo Predictor 3 (floating-point horizontal differencing, Adobe Photoshop TIFF Technical Note 3; what GDAL writes with PREDICTOR=3):
    every row is stored as byte planes -- byte 0 (the most significant) of all its samples, then byte 1, ... -- independent of the file's byte
    order, and that byte row is differenced with a stride of `pix` bytes.  Returns [rows, cols, pix] in native byte order."""
    bps, n = dt.itemsize, cols * pix
    acc = np.cumsum(raw[:rows * n * bps].reshape(rows, n * bps // pix, pix), axis=1, dtype=np.uint8)          # (wraps modulo 256, as the bytes do)
    planes = acc.reshape(rows, bps, n)
    be = np.ascontiguousarray(np.moveaxis(planes, 1, 2))                                                          # [rows, n, bps] big-endian samples
    return be.view(np.dtype(f">f{bps}")).reshape(rows, cols, pix).astype(dt.newbyteorder("="))


def _geo_meta(tags) -> Dict:
    meta = {"tags": {t: tags[t] for t in GEO_TAGS if t in tags}, "geotransform": None}
    if 33550 in tags and 33922 in tags:
        sx, sy = tags[33550][0], tags[33550][1]
        i, j, _, x, y, _ = tags[33922][:6]
        meta["geotransform"] = (x - i * sx, sx, 0.0, y + j * sy, 0.0, -sy)
    if 42113 in tags:
        try:
            meta["nodata"] = float(tags[42113][0])
        except ValueError:
            meta["nodata"] = None
    return meta


def _one_error_contract(fn):
    """One error contract for the readers: a file this module does not implement raises NotImplementedError, a damaged one ValueError naming
    the file -- whatever the damage tripped inside (a missing tag, an offset past the end, a count that does not fit, zlib's own error, an
    allocation the header asks for and the file cannot justify).  GDAL, which the reference reads through, reports a read error there."""
    import functools
    import zlib

    @functools.wraps(fn)
    def reader(path, *args):
        try:
            return fn(path, *args)
        except (ValueError, NotImplementedError, OSError):
            raise
        except (KeyError, IndexError, struct.error, zlib.error, MemoryError, ArithmeticError, TypeError, UnicodeError) as e:
            raise ValueError(f"{path}: damaged TIFF ({type(e).__name__}: {e})") from e
    return reader


@_one_error_contract
def tiff_info(path) -> Dict:
    """Header-only read (memory-mapped: the pixel data is never touched): meta of read_tiff plus 'height', 'width', 'bands'.
    What the prediction merge needs from every tile before any of them is predicted (reference predict.py:206-222 takes the same
    numbers from gdal.Open(...).GetGeoTransform() / RasterXSize / RasterYSize)."""
    import mmap
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as b:
        tags, _ = _parse_tags(b, path)
    meta = _geo_meta(tags)
    meta.update(height=tags[257][0], width=tags[256][0], bands=tags.get(277, (1,))[0])
    return meta


@_one_error_contract
def tiff_levels(path) -> list:
    """One {"height", "width", "subfile_type"} per IFD of the file, in chain order: the full-resolution image first, then the overviews
    a tiled writer placed behind it (NewSubfileType 1), largest first.  Header-only, memory-mapped."""
    import mmap
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as b:
        off, big, bo = _header(b, path)
        out = [_parse_ifd(b, path, o, big, bo) for o in _ifd_offsets(b, path, off, big, bo)]
    return [{"height": t[257][0], "width": t[256][0], "subfile_type": t.get(254, (0,))[0]} for t in out]


def read_tiff(path) -> Tuple[np.ndarray, Dict]:
    """Returns (array [C,H,W] (or [H,W] for one band), meta) with meta['geotransform'] = (ulx, xres, 0, uly, 0, -yres)
    when the file is georeferenced and meta['tags'] holding the raw GeoTIFF tags.  The file is memory-mapped (copy-on-write), never slurped:
    an uncompressed native-endian file with contiguous strips comes back as a VIEW of the mapping (no copy at all: the training feed's one
    copy is the one into its pinned staging buffer); everything else is decoded strip by strip into one output array."""
    return _read_ifd(path, 0)


def read_tiff_level(path, level: int) -> np.ndarray:
    """The array of IFD `level` of the file (0: the full-resolution image, what read_tiff returns; 1...: the overviews, see tiff_levels),
    through the decoders and the error contract of read_tiff."""
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or level < 0:
        raise ValueError(f"level must be an int >= 0, got {level!r}")
    return _read_ifd(path, int(level))[0]


@_one_error_contract
def _read_ifd(path, level):
    import mmap
    import os
    with open(path, "rb") as f:
        if os.environ.get("UNET_TIFF_MMAP", "1") == "0":      # (A/B switch: read the file instead of mapping it)
            mm = bytearray(f.read())
        else:
            mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_COPY)
    b = np.frombuffer(mm, dtype=np.uint8)           # (keeps the mapping alive for as long as a view of it exists)
    tags, bo = _parse_tags(mm, path, level)
    W, H = tags[256][0], tags[257][0]
    spp = tags.get(277, (1,))[0]
    bits = tags.get(258, (1,))[0]
    fmt = tags.get(339, (1,))[0]
    comp, predictor = tags.get(259, (1,))[0], tags.get(317, (1,))[0]
    planar = tags.get(284, (1,))[0]
    if bits not in (8, 16, 32, 64) or len(set(tags.get(258, (bits,)))) != 1:
        raise NotImplementedError(f"{path}: {tags.get(258)}-bit samples are not supported (8 / 16 / 32 / 64, the same for every band, are)")
    dt = _dtype(bits, fmt, bo)
    native = dt.newbyteorder("=")
    planes = spp if planar == 2 else 1
    pix = 1 if planar == 2 else spp
    meta = _geo_meta(tags)
    meta["dtype"] = native

    def finish(out):          # out: [planes, H, W, pix]
        arr = out[:, :, :, 0] if planar == 2 else np.moveaxis(out[0], -1, 0)
        return (arr[0] if arr.shape[0] == 1 else arr), meta

    if comp == 1 and predictor == 1 and 324 not in tags and dt.isnative:
        offs = tags[273]
        rps = min(tags.get(278, (H,))[0], H)
        total = planes * H * W * pix * dt.itemsize
        cnts = tags.get(279)
        contiguous = len(offs) == 1 or (cnts is not None and all(offs[k] + cnts[k] == offs[k + 1] for k in range(len(offs) - 1))
                                        and (planes == 1 or H % rps == 0))
        if contiguous and offs[0] + total <= b.size:
            return finish(b[offs[0]:offs[0] + total].view(dt).reshape(planes, H, W, pix))

    if comp == 7:
        if bits != 8 or predictor != 1:
            raise NotImplementedError(f"{path}: JPEG-in-TIFF with {bits}-bit samples / predictor {predictor} is not supported")
        jpeg = _jpeg_decoder(tags, path)
    decode = _decoder(comp, path) if comp != 7 else None
    # what the header asks for against what the file can hold: Deflate tops out at 1032 : 1, LZW and PackBits below that, a flat JPEG near
    # 100 : 1 -- a damaged ImageWidth / ImageLength (65535 x 65535 x 4 is 17 GB) is refused here instead of being allocated and decoded into
    if W <= 0 or H <= 0 or spp <= 0 or planes * H * W * pix * dt.itemsize > (1 << 20) + (b.size << (12 if comp != 1 else 0)):
        raise ValueError(f"{path}: {planes * pix} x {H} x {W} {dt} samples cannot come out of a file of {b.size} bytes (compression {comp})")
    out = np.zeros((planes, H, W, pix), dtype=native)

    def block(off, nbytes, rows, cols):
        """one strip / tile as [rows, cols, pix] in native byte order, decompressed and un-differenced"""
        if comp == 7:
            return jpeg(b[off:off + nbytes], rows, cols, pix)
        need = rows * cols * pix * dt.itemsize
        raw = decode(b[off:off + nbytes], need) if comp != 1 else b[off:off + need]
        if len(raw) < need:
            raise ValueError(f"{path}: strip / tile holds {len(raw)} bytes, {need} expected")
        if predictor == 3 and dt.kind == "f":
            return _unpredict_float(np.frombuffer(raw, dtype=np.uint8, count=need) if not isinstance(raw, np.ndarray) else raw[:need].view(np.uint8),
                                    rows, cols, pix, dt)
        t = raw[:need].view(dt).reshape(rows, cols, pix)
        return _unpredict(t.astype(native, copy=False), predictor, path)

    # every strip / tile is independent: a list of jobs (offset, bytes, block shape, destination), run by a few threads when the scene is
    # large (the codecs and zlib release the GIL) -- a 20000 x 20000 x 4 LZW scene is 1.6 GB to decode in front of a 5 s prediction
    jobs = []
    if 324 in tags:        # tiled
        tw, th = tags[322][0], tags[323][0]
        offs, cnts = tags[324], tags[325]
        tx, ty = -(-W // tw), -(-H // th)
        k = 0
        for p in range(planes):
            for j in range(ty):
                for i in range(tx):
                    h, w = min(th, H - j * th), min(tw, W - i * tw)
                    jobs.append((offs[k], cnts[k], th, tw, p, j * th, h, i * tw, w))
                    k += 1
    else:
        rps = min(tags.get(278, (H,))[0], H)
        offs = tags[273]
        spi = -(-H // rps)
        cnts = tags.get(279) or tuple(min(rps, H - (s % spi) * rps) * W * pix * dt.itemsize for s in range(planes * spi))
        for p in range(planes):
            for s_ in range(spi):
                r0 = s_ * rps
                rows = min(rps, H - r0)
                jobs.append((offs[p * spi + s_], cnts[p * spi + s_], rows, W, p, r0, rows, 0, W))

    def run(chunk):
        for off, nbytes, brows, bcols, p, r0, h, c0, w in chunk:
            t = block(off, nbytes, brows, bcols)
            if t.shape[0] < h or t.shape[1] < w:
                raise ValueError(f"{path}: strip / tile decodes to {t.shape[0]} x {t.shape[1]} samples, {h} x {w} needed")
            out[p, r0:r0 + h, c0:c0 + w] = t[:h, :w]

    total = planes * H * W * pix * dt.itemsize
    nthr = _threads()
    if comp != 1 and len(jobs) >= 16 and total >= (32 << 20) and nthr > 1:
        from concurrent.futures import ThreadPoolExecutor
        step = max(1, -(-len(jobs) // (nthr * 8)))
        with ThreadPoolExecutor(max_workers=nthr) as ex:
            list(ex.map(run, [jobs[i:i + step] for i in range(0, len(jobs), step)]))
    else:
        run(jobs)
    return finish(out)


def lzw_cap(n: int) -> int:
    """bytes that always hold the LZW stream of an n-byte strip: at most one 12-bit code per byte, one Clear per 3836 table additions,
    the Clear / EOI frame"""
    return (3 * (n + n // 3836 + 4) + 1) // 2


def check_compress(compress, predictor=1, floats: bool = False):
    """the compress= / predictor= arguments of the writers, validated from the arguments alone -> (compress, predictor)"""
    if compress not in (None, "lzw"):
        raise ValueError(f"compress must be None or 'lzw', got {compress!r}")
    if isinstance(predictor, bool) or predictor not in (1, 2):
        raise ValueError(f"predictor must be 1 or 2 (horizontal differencing), got {predictor!r}")
    if predictor == 2 and compress is None:
        raise ValueError("predictor=2 needs compress='lzw': an uncompressed file is not differenced")
    if predictor == 2 and floats:
        raise ValueError("predictor=2 is horizontal differencing of integer samples; floating-point differencing (Predictor 3) is not written")
    return compress, int(predictor)


def _samples(arr) -> np.ndarray:
    """[C, H, W] samples of a type the writers store (bool -> uint8, int64 -> int32, float64 -> float32)"""
    a = np.asarray(arr)
    if a.ndim == 2:
        a = a[None]
    for src, dst in ((np.bool_, np.uint8), (np.int64, np.int32), (np.float64, np.float32)):
        if a.dtype == src:
            a = a.astype(dst)
    return a


def _geo_dict(tags, geotransform, nodata) -> Dict[int, tuple]:
    """the georeferencing tags of a writer: the caller's tags, ModelPixelScale / ModelTiepoint of the geotransform, GDAL_NODATA"""
    geo = dict(tags or {})
    if geotransform is not None:
        ulx, xres, _, uly, _, yres = geotransform
        geo[33550] = (abs(xres), abs(yres), 0.0)
        geo[33922] = (0.0, 0.0, 0.0, ulx, uly, 0.0)
    if nodata is not None:
        geo[42113] = (str(nodata),)
    return geo


def _image_specs(W: int, H: int, C: int, dtype: np.dtype, predictor: int) -> list:
    """(tag, type, values) of what every LZW image of the writers states, strips or tiles, full resolution or overview: size, samples,
    Compression 5, band-sequential planes (PlanarConfiguration 2 for C > 1), Predictor, ExtraSamples, SampleFormat"""
    specs = [(256, 4, [W]), (257, 4, [H]), (258, 3, [dtype.itemsize * 8] * C), (259, 3, [5]), (262, 3, [1]), (277, 3, [C]),
             (284, 3, [2 if C > 1 else 1]), (339, 3, [{"u": 1, "i": 2, "f": 3}[dtype.kind]] * C)]
    if predictor == 2:
        specs.append((317, 3, [2]))
    if C > 1:
        specs.append((338, 3, [0] * (C - 1)))
    return specs


def _geo_specs(geo: Dict[int, tuple]) -> list:
    out = []
    for t in sorted(geo):
        v = geo[t]
        if t in (34737, 42113):
            out.append((t, 2, v[0] if isinstance(v, tuple) else v))
        elif t == 34735:
            out.append((t, 3, list(v)))
        else:
            out.append((t, 12, list(v)))
    return out


def _tag_entries(specs) -> list:
    """(tag, type, values) -> (tag, type, count, little-endian payload), sorted by tag as an IFD must be"""
    entries = []
    for tag, typ, vals in specs:
        if typ == 2:
            payload = vals.encode("latin1") + b"\0"
            cnt = len(payload)
        else:
            payload = struct.pack("<" + _TYPES[typ][0][0] * len(vals), *vals)
            cnt = len(vals)
        entries.append((tag, typ, cnt, payload))
    entries.sort(key=lambda e: e[0])
    return entries


def _pack_ifd(entries, ifd_off: int, big: bool, next_ifd: int = 0) -> bytes:
    """one IFD placed at ifd_off: entry count, entries, the offset of the next IFD, then the values that do not fit an entry (each on a
    word boundary).  Its length depends on the tags' types and counts alone, not on their values."""
    off_fmt, inl = ("Q", 8) if big else ("I", 4)
    n = len(entries)
    extra_off = ifd_off + (8 + 20 * n + 8 if big else 2 + 12 * n + 4)
    extra, body = b"", b""
    for tag, typ, cnt, payload in entries:
        if len(payload) <= inl:
            val = payload.ljust(inl, b"\0")
        else:
            if len(extra) % 2:
                extra += b"\0"
            val = struct.pack("<" + off_fmt, extra_off + len(extra))
            extra += payload
        body += struct.pack("<HH" + off_fmt, tag, typ, cnt) + val
    return struct.pack("<Q" if big else "<H", n) + body + struct.pack("<" + off_fmt, next_ifd) + extra


class StripWriter:
    """The file layout of compress="lzw", filled strip by strip by whoever encodes (write_tiff below: the host encoder; unet_amd/tiffenc.py:
    the device).  Little-endian; LZW strips of rows_per_strip rows (default: the largest row count whose strip is at most 64 KiB, at
    least one row); PlanarConfiguration 2 for C > 1 -- strip p * strips_per_plane + s is strip s of band p, GDAL's INTERLEAVE=BAND;
    Predictor tag 317 when predictor == 2.  The strip byte counts are known only after encoding, so the IFD is placed AFTER the data:
    header, strips in order, IFD with its StripOffsets / StripByteCounts arrays, and close() patches the header's IFD offset.  BigTIFF
    is chosen from the worst-case byte count (every strip at its capacity), so the choice does not depend on the content.
    The georeferencing tags, GDAL_NODATA, SampleFormat and ExtraSamples are those of the uncompressed writer."""

    def __init__(self, path, C: int, H: int, W: int, dtype, rows_per_strip=None, predictor: int = 1, geotransform=None,
                 tags: Optional[Dict[int, tuple]] = None, nodata=None, bigtiff: Optional[bool] = None):
        self.dtype = np.dtype(dtype)
        if self.dtype.kind not in "uif" or self.dtype.itemsize not in (1, 2, 4) or (self.dtype.kind == "f" and self.dtype.itemsize != 4):
            raise ValueError(f"compress='lzw': {self.dtype} samples are not written (8 / 16 / 32-bit integers and float32 are)")
        check_compress("lzw", predictor, self.dtype.kind == "f")
        if min(C, H, W) < 1:
            raise ValueError(f"compress='lzw': empty image {C} x {H} x {W}")
        es = self.dtype.itemsize
        if rows_per_strip is None:
            rows_per_strip = max(1, (64 << 10) // (W * es))
        if isinstance(rows_per_strip, bool) or not isinstance(rows_per_strip, (int, np.integer)) or rows_per_strip < 1:
            raise ValueError(f"rows_per_strip must be None or an int >= 1, got {rows_per_strip!r}")
        self.C, self.H, self.W, self.predictor = C, H, W, predictor
        self.rows_per_strip = rps = min(int(rows_per_strip), H)
        self.strips_per_plane = spp = -(-H // rps)
        self.strips = [(p, s * rps, min(rps, H - s * rps)) for p in range(C) for s in range(spp)]          # (band, first row, rows) in file order
        worst = sum(lzw_cap(rows * W * es) for _, _, rows in self.strips[:spp]) * C
        self.big = (worst > (1 << 32) - (1 << 20)) if bigtiff is None else bool(bigtiff)
        self.geo = _geo_dict(tags, geotransform, nodata)
        self.offsets, self.counts = [], []
        self.f = open(path, "wb")
        self.f.write(b"II" + (struct.pack("<HHHQ", 43, 8, 0, 0) if self.big else struct.pack("<HI", 42, 0)))
        self.pos = 16 if self.big else 8

    def append(self, data, sizes) -> None:
        """the next len(sizes) strips: `data` (bytes-like) holds their streams back to back"""
        sizes = [int(s) for s in sizes]
        if len(self.counts) + len(sizes) > len(self.strips) or sum(sizes) != len(data):
            raise ValueError(f"StripWriter.append: {len(sizes)} strips of {sum(sizes)} bytes do not match the data ({len(data)} bytes) or the layout")
        for s in sizes:
            self.offsets.append(self.pos)
            self.counts.append(s)
            self.pos += s
        self.f.write(data)

    def close(self) -> int:
        """writes the IFD behind the data and closes the file -> the file's size in bytes"""
        if len(self.counts) != len(self.strips):
            self.f.close()
            raise ValueError(f"StripWriter.close: {len(self.counts)} of {len(self.strips)} strips were written")
        big, C = self.big, self.C
        if not big and self.pos > (1 << 32) - (1 << 20):
            self.f.close()
            raise ValueError("the compressed data does not fit a classic TIFF's 32-bit offsets: pass bigtiff=None or True")
        off_t = 16 if big else 4
        specs = _image_specs(self.W, self.H, C, self.dtype, self.predictor)
        specs += [(273, off_t, self.offsets), (278, 4, [self.rows_per_strip]), (279, off_t, self.counts)] + _geo_specs(self.geo)
        pad = self.pos % 2                                          # an IFD starts on a word boundary
        ifd_off = self.pos + pad
        self.f.write(b"\0" * pad + _pack_ifd(_tag_entries(specs), ifd_off, big))
        size = self.f.tell()
        self.f.seek(8 if big else 4)
        self.f.write(struct.pack("<Q" if big else "<I", ifd_off))
        self.f.close()
        return size


RESAMPLINGS = ("mode", "average", "nearest")


def check_tiling(compress, tile, overviews, floats: bool = False, auto: bool = False):
    """the tile= / overviews= arguments of the writers, validated from the arguments alone -> (tile, overviews).  auto: "auto" is accepted
    (the prediction entry points resolve it with resolve_overviews)."""
    if tile is None:
        if overviews is not None:
            raise ValueError(f"overviews={overviews!r} needs tile=: overviews are written into tiled files only")
        return None, None
    if isinstance(tile, bool) or not isinstance(tile, (int, np.integer)) or not 16 <= tile <= 1024 or tile % 16:
        raise ValueError(f"tile must be None or a multiple of 16 in 16..1024, got {tile!r}")
    if compress != "lzw":
        raise ValueError("tile= needs compress='lzw': uncompressed tiled files are not written")
    if overviews is not None and overviews not in RESAMPLINGS and not (auto and overviews == "auto"):
        raise ValueError(f"overviews must be None, {', '.join(repr(r) for r in RESAMPLINGS)}{' or auto' if auto else ''}: got {overviews!r}")
    if overviews == "mode" and floats:
        raise ValueError("overviews='mode' counts equal values: it is for class masks and integer samples, not for float samples")
    return int(tile), overviews


def resolve_overviews(overviews, class_mask: bool):
    """ "auto" -> "mode" for a class mask, "average" for everything else (probabilities, regression, the int8 stretch)"""
    return ("mode" if class_mask else "average") if overviews == "auto" else overviews


def overview_shapes(H: int, W: int, tile: int) -> list:
    """[(H_1, W_1), (H_2, W_2), ...]: level k + 1 has ceil(H_k / 2) x ceil(W_k / 2) samples and levels are added while
    max(H_k, W_k) > tile, so the last one fits one tile; a raster no larger than a tile has none"""
    out = []
    while max(H, W) > tile:
        H, W = -(-H // 2), -(-W // 2)
        out.append((H, W))
    return out


def nodata_sample(nodata, dtype):
    """`nodata` as a sample of `dtype`, or None when no sample can equal it (none given; not a whole number or out of range for an
    integer type) -- then every sample is valid.  Float samples are compared with float32(nodata)."""
    dtype = np.dtype(dtype)
    if nodata is None:
        return None
    nd = float(nodata)
    if dtype.kind == "f":
        return dtype.type(nd)
    if nd != nd or nd != int(nd) or not np.iinfo(dtype).min <= int(nd) <= np.iinfo(dtype).max:
        return None
    return dtype.type(int(nd))


def reduce_level(a: np.ndarray, resampling: str, nodata=None) -> np.ndarray:
    """The next overview level of [C, H, W] samples, [C, ceil(H / 2), ceil(W / 2)] -- the pyramid rule of unet_amd/tiffenc.py (module
    docstring) for host arrays; csrc/tiff_pyramid.hip computes the same samples on the device."""
    if resampling not in RESAMPLINGS:
        raise ValueError(f"resampling must be one of {RESAMPLINGS}, got {resampling!r}")
    if resampling == "mode" and a.dtype.kind == "f":
        raise ValueError("resampling 'mode' is not for float samples")
    C, H, W = a.shape
    h, w = -(-H // 2), -(-W // 2)
    nd = nodata_sample(nodata, a.dtype)
    if resampling == "nearest":
        return np.ascontiguousarray(a[:, ::2, ::2])
    v, m = [], []                                            # the block in row-major order (TL, TR, BL, BR) and which of it counts
    for dy in (0, 1):
        for dx in (0, 1):
            s = np.zeros((C, h, w), a.dtype)
            inside = np.zeros((C, h, w), bool)
            part = a[:, dy::2, dx::2]
            s[:, :part.shape[1], :part.shape[2]] = part
            inside[:, :part.shape[1], :part.shape[2]] = True
            if nd is not None:
                inside &= ~np.isnan(s) if nd != nd else (s != nd)
            v.append(s)
            m.append(inside)
    n = m[0].astype(np.int64) + m[1] + m[2] + m[3]
    fill = a.dtype.type(0) if nd is None else nd              # (n == 0 needs a nodata: without one the top-left sample always counts)
    if resampling == "average":
        if a.dtype.kind == "f":
            acc = np.zeros((C, h, w), np.float32)
            for s, ok in zip(v, m):
                acc = np.where(ok, acc + s, acc)              # sequential fp32 sum in row-major order
            with np.errstate(invalid="ignore", divide="ignore"):
                out = acc / n.astype(np.float32)
        else:
            tot = sum(np.where(ok, s.astype(np.int64), 0) for s, ok in zip(v, m))
            out = (2 * tot + n) // np.maximum(2 * n, 1)        # round half up; // floors, so negative means round the same way
        return np.where(n > 0, out, fill).astype(a.dtype)
    best, best_n = np.full((C, h, w), fill, a.dtype), np.zeros((C, h, w), np.int64)
    for k in range(4):
        cnt = sum((m[k] & m[j] & (v[j] == v[k])).astype(np.int64) for j in range(4))
        take = cnt > best_n                                   # strictly more: a tie stays with the value that came first
        best, best_n = np.where(take, v[k], best), np.where(take, cnt, best_n)
    return best


def build_overviews(a: np.ndarray, tile: int, resampling: str, nodata=None) -> list:
    """the overview levels of [C, H, W] samples, each computed from the one before it"""
    out = []
    for _ in overview_shapes(a.shape[1], a.shape[2], tile):
        a = reduce_level(a, resampling, nodata)
        out.append(a)
    return out


class TileWriter:
    """The tiled layout of compress="lzw" with tile=: square LZW tiles of `tile` samples a side, band-sequential, and -- with
    levels beyond the first -- the overview images of a cloud-optimised GeoTIFF.  Header, then ALL IFDs (IFD 0: full resolution with the
    georeferencing tags; then one IFD per overview in decreasing size with NewSubfileType 1, its own tile arrays and the same sample,
    Predictor and GDAL_NODATA tags), then the tile data: the smallest overview first, the full resolution last; within a level tile
    k = (p * tiles_down + j) * tiles_across + i.  The tile counts are known before anything is encoded, so the IFD block has a known size:
    it is reserved on open and written with the real TileOffsets / TileByteCounts by close().  BigTIFF is chosen from the worst case
    (every tile at its capacity).  Edge tiles are whole tiles, padded with zeros by whoever encodes them.  The GDAL ghost area and the
    per-tile leader / trailer bytes, both optional in the COG specification, are not written."""

    def __init__(self, path, C: int, shapes, dtype, tile: int, predictor: int = 1, geotransform=None, tags: Optional[Dict[int, tuple]] = None,
                 nodata=None, bigtiff: Optional[bool] = None):
        self.dtype = np.dtype(dtype)
        if self.dtype.kind not in "uif" or self.dtype.itemsize not in (1, 2, 4) or (self.dtype.kind == "f" and self.dtype.itemsize != 4):
            raise ValueError(f"compress='lzw': {self.dtype} samples are not written (8 / 16 / 32-bit integers and float32 are)")
        check_compress("lzw", predictor, self.dtype.kind == "f")
        check_tiling("lzw", tile, None)
        self.shapes = [(int(h), int(w)) for h, w in shapes]          # level 0 first
        if C < 1 or not self.shapes or min(min(s) for s in self.shapes) < 1:
            raise ValueError(f"compress='lzw': empty image {C} x {self.shapes}")
        self.C, self.tile, self.predictor = C, int(tile), predictor
        self.grid = [(-(-h // tile), -(-w // tile)) for h, w in self.shapes]          # (tiles down, tiles across) of a level
        self.per_level = [C * ty * tx for ty, tx in self.grid]
        self.order = tuple(range(len(self.shapes) - 1, -1, -1))                     # levels in file order: smallest first
        self._open = list(self.order)                                               # levels that still take tiles
        self.slot_cap = lzw_cap(tile * tile * self.dtype.itemsize)
        self.geo = _geo_dict(tags, geotransform, nodata)
        self.offsets = [[] for _ in self.shapes]
        self.counts = [[] for _ in self.shapes]
        self.big = False
        if bigtiff is None:
            self.big = len(self._ifds(True)) + sum(self.per_level) * self.slot_cap > (1 << 32) - (1 << 20)
        else:
            self.big = bool(bigtiff)
        self.f = open(path, "wb")
        head = 16 if self.big else 8
        self.f.write(b"II" + (struct.pack("<HHHQ", 43, 8, 0, head) if self.big else struct.pack("<HI", 42, head)))
        self.f.write(self._ifds(True))
        self.pos = self.f.tell()

    def _ifds(self, reserve: bool) -> bytes:
        """the block of all IFDs as it stands behind the header (reserve: with zeros for the tile arrays, which has the same length)"""
        big = self.big
        off_t = 16 if big else 4
        pos = 16 if big else 8
        out = b""
        for k, (h, w) in enumerate(self.shapes):
            n = self.per_level[k]
            specs = _image_specs(w, h, self.C, self.dtype, self.predictor)
            specs += [(322, 3, [self.tile]), (323, 3, [self.tile]), (324, off_t, [0] * n if reserve else self.offsets[k]),
                      (325, off_t, [0] * n if reserve else self.counts[k])]
            if k == 0:
                specs += _geo_specs(self.geo)
            else:
                specs += [(254, 4, [1])] + _geo_specs({t: v for t, v in self.geo.items() if t == 42113})
            entries = _tag_entries(specs)
            size = len(_pack_ifd(entries, pos, big))
            size += size % 2                                                       # the next IFD starts on a word boundary
            last = k == len(self.shapes) - 1
            out += _pack_ifd(entries, pos, big, 0 if last else pos + size).ljust(size, b"\0")
            pos += size
        return out

    def append(self, data, sizes) -> None:
        """the next len(sizes) tiles in file order (levels from the smallest to the full resolution, tile order within a level):
        `data` (bytes-like) holds their streams back to back"""
        sizes = [int(s) for s in sizes]
        if sum(sizes) != len(data):
            raise ValueError(f"TileWriter.append: {len(sizes)} tiles of {sum(sizes)} bytes do not match the data ({len(data)} bytes)")
        for s in sizes:
            while self._open and len(self.counts[self._open[0]]) == self.per_level[self._open[0]]:
                self._open.pop(0)
            if not self._open:
                raise ValueError("TileWriter.append: more tiles than the layout holds")
            self.offsets[self._open[0]].append(self.pos)
            self.counts[self._open[0]].append(s)
            self.pos += s
        self.f.write(data)

    def close(self) -> int:
        """fills in the reserved IFD block and closes the file -> the file's size in bytes"""
        if [len(c) for c in self.counts] != self.per_level:
            self.f.close()
            raise ValueError(f"TileWriter.close: {[len(c) for c in self.counts]} of {self.per_level} tiles were written")
        if not self.big and self.pos > (1 << 32) - (1 << 20):
            self.f.close()
            raise ValueError("the compressed data does not fit a classic TIFF's 32-bit offsets: pass bigtiff=None or True")
        size = self.f.tell()
        self.f.seek(16 if self.big else 8)
        self.f.write(self._ifds(False))
        self.f.close()
        return size


def tile_block(a: np.ndarray, p: int, j: int, i: int, tile: int) -> np.ndarray:
    """tile (p, j, i) of [C, H, W] samples as a whole [tile, tile] block: what lies beyond the right or bottom edge is zero"""
    part = a[p, j * tile:(j + 1) * tile, i * tile:(i + 1) * tile]
    if part.shape == (tile, tile):
        return part
    block = np.zeros((tile, tile), a.dtype)
    block[:part.shape[0], :part.shape[1]] = part
    return block


def _lzw_stream(lib, src: np.ndarray, path) -> np.ndarray:
    cap = lzw_cap(src.size)
    dst = np.empty(cap, dtype=np.uint8)
    got = lib.unet_tiff_lzw_encode(src.ctypes.data, src.size, dst.ctypes.data, cap)
    if got < 0:
        raise RuntimeError(f"{path}: the LZW encoder overran its capacity of {cap} bytes for a block of {src.size}")
    return dst[:got]


def _write_tiled(path, a: np.ndarray, geotransform, tags, nodata, bigtiff, predictor, tile, overviews) -> int:
    """write_tiff(compress="lzw", tile=) of host samples: the pyramid by reduce_level, the tiles by unet_tiff_lzw_encode on a thread
    pool, a batch at a time, appended in file order -- the file does not depend on the thread count.  Predictor 2 runs along the whole
    padded tile row (the first padded sample holds 0 - last), as libtiff does."""
    lib = _codecs()
    levels = [a] + (build_overviews(a, tile, overviews, nodata) if overviews is not None else [])
    w = TileWriter(path, a.shape[0], [l.shape[1:] for l in levels], a.dtype, tile, predictor, geotransform, tags, nodata, bigtiff)
    jobs = [(k, p, j, i) for k in w.order for p in range(w.C) for j in range(w.grid[k][0]) for i in range(w.grid[k][1])]

    def encode(job):
        k, p, j, i = job
        return _lzw_stream(lib, _predicted_le(tile_block(levels[k], p, j, i, tile), predictor), path)

    try:
        nthr = _threads()
        if nthr > 1 and len(jobs) >= 16 and a.nbytes >= (4 << 20):
            from concurrent.futures import ThreadPoolExecutor
            step = nthr * 16
            with ThreadPoolExecutor(max_workers=nthr) as ex:
                for n in range(0, len(jobs), step):
                    enc = list(ex.map(encode, jobs[n:n + step]))
                    w.append(b"".join(e.data for e in enc), [e.size for e in enc])
        else:
            for job in jobs:
                e = encode(job)
                w.append(e.data, [e.size])
    except BaseException:
        w.f.close()
        raise
    return w.close()


def _predicted_le(block: np.ndarray, predictor: int) -> np.ndarray:
    """[rows, W] samples -> the strip's bytes: differences per sample along the row modulo 2^bits (Predictor 2), then little-endian"""
    if predictor == 2:
        d = block.copy()
        d[:, 1:] -= block[:, :-1]          # (integer arrays wrap)
        block = d
    return np.ascontiguousarray(block.astype(block.dtype.newbyteorder("<"), copy=False)).view(np.uint8).reshape(-1)


def _write_lzw(path, a: np.ndarray, geotransform, tags, nodata, bigtiff, predictor, rows_per_strip) -> int:
    """write_tiff(compress="lzw") of host samples: the strips are encoded by unet_tiff_lzw_encode on a thread pool (ctypes releases the
    GIL), a batch of strips at a time, and appended in order -- the file does not depend on the thread count"""
    lib = _codecs()
    C, H, W = a.shape
    w = StripWriter(path, C, H, W, a.dtype, rows_per_strip, predictor, geotransform, tags, nodata, bigtiff)

    def encode(strip):
        p, r0, rows = strip
        src = _predicted_le(a[p, r0:r0 + rows], predictor)
        cap = lzw_cap(src.size)
        dst = np.empty(cap, dtype=np.uint8)
        got = lib.unet_tiff_lzw_encode(src.ctypes.data, src.size, dst.ctypes.data, cap)
        if got < 0:
            raise RuntimeError(f"{path}: the LZW encoder overran its capacity of {cap} bytes for a strip of {src.size}")
        return dst[:got]

    try:
        nthr = _threads()
        if nthr > 1 and len(w.strips) >= 16 and a.nbytes >= (4 << 20):
            from concurrent.futures import ThreadPoolExecutor
            step = nthr * 16
            with ThreadPoolExecutor(max_workers=nthr) as ex:
                for i in range(0, len(w.strips), step):
                    enc = list(ex.map(encode, w.strips[i:i + step]))
                    w.append(b"".join(e.data for e in enc), [e.size for e in enc])
        else:
            for strip in w.strips:
                e = encode(strip)
                w.append(e.data, [e.size])
    except BaseException:
        w.f.close()
        raise
    return w.close()


def write_tiff(path, arr: np.ndarray, geotransform=None, tags: Optional[Dict[int, tuple]] = None, nodata=None, bigtiff: Optional[bool] = None,
               compress=None, predictor: int = 1, rows_per_strip=None, tile=None, overviews=None) -> None:
    """Uncompressed, single strip, pixel-interleaved little-endian TIFF of a [C,H,W] or [H,W] array.  bigtiff None: BigTIFF (64-bit offsets)
    when the file would not fit 32-bit offsets -- what GDAL's BIGTIFF=IF_NEEDED does for the reference's outputs (predict.py:19-52): the
    all-classes probabilities of a 20000 x 20000 scene are 8 GB.
    compress="lzw": LZW strips in the layout of StripWriter (band-sequential, IFD behind the data), encoded on the host; predictor=2 adds
    horizontal differencing (integer samples only); rows_per_strip None: strips of at most 64 KiB.
    tile (a multiple of 16 in 16..1024, needs compress="lzw"): square LZW tiles in the layout of TileWriter instead of strips;
    overviews "mode" | "average" | "nearest" (needs tile): the overview pyramid of reduce_level behind the full-resolution image, down to
    the first level that fits one tile -- a cloud-optimised GeoTIFF.  nodata then also marks the samples the overviews leave out."""
    if compress is not None or predictor != 1 or rows_per_strip is not None or tile is not None or overviews is not None:
        a = _samples(arr)
        check_compress(compress, predictor, a.dtype.kind == "f")
        tile, overviews = check_tiling(compress, tile, overviews, a.dtype.kind == "f")
        if tile is not None:
            if rows_per_strip is not None:
                raise ValueError("rows_per_strip is for strips: a tiled file (tile=) has none")
            _write_tiled(path, a, geotransform, tags, nodata, bigtiff, predictor, tile, overviews)
            return
        if compress is None:
            raise ValueError("rows_per_strip needs compress='lzw': the uncompressed file is one strip")
        _write_lzw(path, a, geotransform, tags, nodata, bigtiff, predictor, rows_per_strip)
        return
    a = np.asarray(arr)
    if a.ndim == 2:
        a = a[None]
    C, H, W = a.shape
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if a.dtype == np.int64:
        a = a.astype(np.int32)
    if a.dtype == np.float64:
        a = a.astype(np.float32)
    kind = {"u": 1, "i": 2, "f": 3}[a.dtype.kind]
    nbytes = C * H * W * a.dtype.itemsize
    big = (nbytes > (1 << 32) - (1 << 20)) if bigtiff is None else bool(bigtiff)
    entries = []          # (tag, type, count, payload-bytes)
    off_t, off_fmt = (16, "Q") if big else (4, "I")          # LONG8 / LONG for offsets and byte counts

    def add(tag, typ, vals):
        if typ == 2:
            payload = vals.encode("latin1") + b"\0"
            cnt = len(payload)
        else:
            fmt = _TYPES[typ][0]
            payload = struct.pack("<" + fmt[0] * len(vals), *vals)
            cnt = len(vals)
        entries.append((tag, typ, cnt, payload))

    add(256, 4, [W]); add(257, 4, [H]); add(258, 3, [a.dtype.itemsize * 8] * C); add(259, 3, [1])
    add(262, 3, [1]); add(273, off_t, [0]); add(277, 3, [C]); add(278, 4, [H]); add(279, off_t, [nbytes]); add(284, 3, [1])
    if C > 1:
        add(338, 3, [0] * (C - 1))      # ExtraSamples: unspecified (what GDAL writes for MINISBLACK multi-band)
    add(339, 3, [kind] * C)
    geo = dict(tags or {})
    if geotransform is not None:
        ulx, xres, _, uly, _, yres = geotransform
        geo[33550] = (abs(xres), abs(yres), 0.0)
        geo[33922] = (0.0, 0.0, 0.0, ulx, uly, 0.0)
    if nodata is not None:
        geo[42113] = (str(nodata),)
    for t in sorted(geo):
        v = geo[t]
        if t in (34737, 42113):
            add(t, 2, v[0] if isinstance(v, tuple) else v)
        elif t == 34735:
            add(t, 3, list(v))
        else:
            add(t, 12, list(v))
    entries.sort(key=lambda e: e[0])
    n = len(entries)
    inl = 8 if big else 4                                     # bytes of the inline value / offset field
    ifd_off = 16 if big else 8
    extra_off = ifd_off + (8 + 20 * n + 8 if big else 2 + 12 * n + 4)
    extra = b""
    placed = []
    for tag, typ, cnt, payload in entries:
        if len(payload) <= inl:
            placed.append((tag, typ, cnt, payload.ljust(inl, b"\0")))
        else:
            if len(extra) % 2:
                extra += b"\0"
            placed.append((tag, typ, cnt, struct.pack("<" + off_fmt, extra_off + len(extra))))
            extra += payload
    if len(extra) % 2:
        extra += b"\0"
    data_off = extra_off + len(extra)
    body = b""
    for tag, typ, cnt, val in placed:
        if tag == 273:
            val = struct.pack("<" + off_fmt, data_off)
        body += struct.pack("<HH" + ("Q" if big else "I"), tag, typ, cnt) + val
    if big:
        head = b"II" + struct.pack("<HHHQ", 43, 8, 0, ifd_off) + struct.pack("<Q", n) + body + struct.pack("<Q", 0)
    else:
        head = b"II" + struct.pack("<HI", 42, ifd_off) + struct.pack("<H", n) + body + struct.pack("<I", 0)
    with open(path, "wb") as f:                               # the pixel data is streamed band-interleaved row block by row block: no second copy
        f.write(head + extra)
        le = a.dtype.newbyteorder("<")
        rows = max(1, (64 << 20) // max(1, C * W * a.dtype.itemsize))
        for r0 in range(0, H, rows):
            f.write(np.ascontiguousarray(np.moveaxis(a[:, r0:r0 + rows], 0, -1)).astype(le, copy=False).tobytes())
