"""The rules of the zonal statistics of a float plane (unet_amd/zonal.py) in NumPy and Python integers: sequential, with no
tolerance anywhere.  The device tables equal these bit for bit.

Inputs      zones int32 [H, W] (-1 = no zone, else 0 .. Z - 1), values float32 [H, W], nodata a number or None.
Valid       a pixel is valid iff its zone is >= 0, its value is finite and its value does not equal float32(nodata).  pixels[z] counts all
            pixels of zone z, valid[z] the valid ones.
Fixed point A = the largest |v| over the valid pixels; E = 0 when A = 0, else frexp's exponent (2^(E-1) <= A < 2^E); s = 30 - E;
            q = rint(double(v) * 2^s), half to even, |q| <= 2^30.  A given shift replaces s; a valid pixel with |q| > 2^30 is then an
            overflow: it is left out of the sums and the call raises.
Tables      sum_q = sum q; q^2 = hi * 2^30 + lo with 0 <= lo < 2^30, sq_lo = sum lo, sq_hi = sum hi (each sum <= 2^30 * 2^31 = 2^61); min and
            max the extremes of the valid pixels in the order of the unsigned image of the float bits (-0.0 below +0.0); +inf and -inf for
            a zone without a valid pixel.
Derived     mean = sum_q / valid * 2^-s, std = sqrt(SQ * valid - sum_q^2) / valid * 2^-s with SQ = sq_hi * 2^30 + sq_lo, sum = sum_q * 2^-s in
            Python integers and one division; None for all of mean, std, min, max, sum where valid == 0.
Bad input   a zone outside -1 .. Z - 1 is counted nowhere and reported."""
import math

import numpy as np

Q_BITS = 30


def key(bits: np.ndarray) -> np.ndarray:
    """the order-preserving unsigned image of float32 bit patterns (uint32 -> uint32)"""
    bits = bits.astype(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def valid_mask(zones, values, Z, nodata=None) -> np.ndarray:
    ok = (zones >= 0) & (zones < Z) & np.isfinite(values)
    if nodata is not None:
        ok &= values != np.float32(nodata)
    return ok


def absmax_bits(zones, values, Z, nodata=None) -> int:
    ok = valid_mask(zones, values, Z, nodata)
    return int((values[ok].view(np.uint32) & np.uint32(0x7FFFFFFF)).max()) if ok.any() else 0


def shift_of(zones, values, Z, nodata=None) -> int:
    a = float(np.array([absmax_bits(zones, values, Z, nodata)], dtype=np.uint32).view(np.float32)[0])
    return Q_BITS - (math.frexp(a)[1] if a else 0)


def tables(zones, values, Z, nodata=None, shift=None) -> dict:
    """{pixels, valid, sum_q, sq_lo, sq_hi: lists of Python ints; min, max: float32 arrays; shift; bad_zone, overflow: bools}, pixel by pixel"""
    zones, values = np.asarray(zones), np.asarray(values)
    assert zones.dtype == np.int32 and values.dtype == np.float32 and zones.shape == values.shape
    s = shift_of(zones, values, Z, nodata) if shift is None else int(shift)
    ok = valid_mask(zones, values, Z, nodata).ravel()
    q = np.zeros(zones.size, dtype=np.int64)
    scaled = np.rint(np.ldexp(values.ravel()[ok].astype(np.float64), s))
    over = np.abs(scaled) > 2.0 ** Q_BITS
    q[ok] = np.where(over, 0, scaled).astype(np.int64)
    idx = np.flatnonzero(ok)
    ok[idx[over]] = False
    keys = key(values.ravel().view(np.uint32))
    t = {k: [0] * Z for k in ("pixels", "valid", "sum_q", "sq_lo", "sq_hi")}
    kmin, kmax = [int(key(np.float32(np.inf).view(np.uint32)))] * Z, [int(key(np.float32(-np.inf).view(np.uint32)))] * Z
    bad_zone = False
    for p, z in enumerate(zones.ravel().tolist()):
        if z < -1 or z >= Z:
            bad_zone = True
        if z < 0 or z >= Z:
            continue
        t["pixels"][z] += 1
        if ok[p]:
            qq = int(q[p])
            t["valid"][z] += 1
            t["sum_q"][z] += qq
            t["sq_lo"][z] += (qq * qq) & ((1 << Q_BITS) - 1)
            t["sq_hi"][z] += (qq * qq) >> Q_BITS
            kmin[z], kmax[z] = min(kmin[z], int(keys[p])), max(kmax[z], int(keys[p]))
    unkey = lambda ks: np.array([k ^ 0x80000000 if k & 0x80000000 else ~k & 0xFFFFFFFF for k in ks], dtype=np.uint32).view(np.float32)  # noqa: E731
    t.update(min=unkey(kmin), max=unkey(kmax), shift=s, bad_zone=bad_zone, overflow=bool(over.any()))
    return t


def tables_fast(zones, values, Z, nodata=None, shift=None) -> dict:
    """the same tables by np.add.at / np.minimum.at on int64 (for planes of millions of pixels: every sum stays far below 2^63)"""
    zones, values = np.asarray(zones).ravel(), np.asarray(values).ravel()
    s = shift_of(zones, values, Z, nodata) if shift is None else int(shift)
    inzone = (zones >= 0) & (zones < Z)
    ok = valid_mask(zones, values, Z, nodata)
    scaled = np.rint(np.ldexp(values[ok].astype(np.float64), s))
    assert not (np.abs(scaled) > 2.0 ** Q_BITS).any()
    q = scaled.astype(np.int64)
    zq = zones[ok].astype(np.int64)
    q2 = q * q
    t = {"pixels": np.bincount(zones[inzone], minlength=Z).astype(np.int64), "valid": np.bincount(zq, minlength=Z).astype(np.int64)}
    for name, term in (("sum_q", q), ("sq_lo", q2 & ((1 << Q_BITS) - 1)), ("sq_hi", q2 >> Q_BITS)):
        acc = np.zeros(Z, dtype=np.int64)
        np.add.at(acc, zq, term)
        t[name] = acc
    keys = key(values[ok].view(np.uint32))
    kmin, kmax = np.full(Z, 0xFF800000, dtype=np.uint32), np.full(Z, 0x007FFFFF, dtype=np.uint32)
    np.minimum.at(kmin, zq, keys)
    np.maximum.at(kmax, zq, keys)
    unkey = lambda k: np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)  # noqa: E731
    t.update(min=unkey(kmin), max=unkey(kmax), shift=s, bad_zone=bool(((zones < -1) | (zones >= Z)).any()), overflow=False)
    return {k: (v.tolist() if k in ("pixels", "valid", "sum_q", "sq_lo", "sq_hi") else v) for k, v in t.items()}


def rows(t: dict, pixel_area: float = 1.0) -> list:
    """the added properties per zone from the tables, in Python integers and one division"""
    s = t["shift"]
    out = []
    for z in range(len(t["pixels"])):
        n, sq_sum = t["valid"][z], t["sum_q"][z]
        row = {"pixels": t["pixels"][z], "area": t["pixels"][z] * float(pixel_area), "valid": n}
        if n:
            SQ = (t["sq_hi"][z] << Q_BITS) + t["sq_lo"][z]
            row.update(mean=math.ldexp(sq_sum / n, -s), std=math.ldexp(math.sqrt(SQ * n - sq_sum * sq_sum) / n, -s), min=float(t["min"][z]),
                       max=float(t["max"][z]), sum=math.ldexp(float(sq_sum), -s))
        else:
            row.update(mean=None, std=None, min=None, max=None, sum=None)
        out.append(row)
    return out
