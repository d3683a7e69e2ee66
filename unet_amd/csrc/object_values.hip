// Statistics of a float plane per object of a label image, with the place of the extremes (unet_amd/objects.py, DESIGN 3.26, where the rules
// are): the keyed pass of zonal_values.hip on (mask, labels, values) instead of a zone plane, under the walk and the checks of objects.hip.
//   unet_obj_absmax   *absmax = the largest bit pattern of |v| over the valid pixels (the host derives the fixed-point shift from it)
//   unet_obj_values   valid, sum_q, sq_lo, sq_hi and (min, argmin), (max, argmax) of every object in one pass
// A pixel p is valid iff mask[p] is not excluded, values[p] is finite and values[p] differs from nodata; it belongs to object
// offs[labels[p]].  A valid value becomes q = rint(double(v) * 2^shift) (half to even; the product is exact), |q| <= 2^30, and q^2 = hi * 2^30
// + lo with 0 <= lo < 2^30 is split before anything is summed: a plane holds fewer than 2^31 pixels, so no int64 wraps.  The extremes carry
// their place in one 64-bit word each: max takes key(v) << 32 | (0xFFFFFFFF - p) by an unsigned maximum from 0, min takes key(v) << 32 | p
// by an unsigned minimum from all ones, with key() the order-preserving unsigned image of the float bits (-0.0 below +0.0).  So argmax and
// argmin are the smallest linear index that attains the extreme.  Neither initial word is the image of a valid pixel (key 0 and key
// 0xFFFFFFFF are NaNs), so it marks an object without one: +inf, -inf and index -1 after the decoding launch.
// The memory shape: a lane owns 4 consecutive pixels per step -- one 16-byte load of the labels, one of the values, one 4-byte load of the
// mask --, two such groups 64 lanes apart are loaded before either is used, and a wavefront walks ONE contiguous span of the plane.  The
// key of a pixel is (label, mask value); equal keys are merged before anything reaches memory:
//   - a wavefront whose 256 pixels hold one key adds nothing across lanes: every lane adds its partials to a pending record of its own in
//     registers, and the wave reduction of those records and the flush of lane 0 happen once, when the key changes or the span ends;
//   - otherwise the keys form runs along the lanes (they may cross row ends: no column sums are taken): the ballot of the run heads guards
//     a segmented reduction by shuffles, the 64-bit fields moved as two halves, after which the head of a run holds the run and flushes it;
//     a lane with several keys merges equal neighbours among its 4 pixels and flushes those itself.
// A flush reads labels[L], mask[L] and offs[L] at the run's label L -- the check of obj_accumulate: L outside 0 .. n - 1 (bit 0 of *bad),
// labels[L] != L (bit 1), mask[L] != the run's mask value (bit 2); such a run is dropped.  offs[L] is below P because L is an anchor of a
// kept class, and it is compared with P all the same.  Bit 3: a valid pixel with |q| > 2^30 -- possible only under a shift that the caller
// chose --, which is left out of every table.  So nothing is stored outside the tables whatever the planes hold.  Only a run with a valid
// pixel issues its four 64-bit adds and two 64-bit extremes.  Where a base pointer is not aligned for the wide loads, and on the last n % 4
// pixels, a lane loads its pixels one by one: no access touches a byte outside the n elements.
#include "common.h"

using namespace unet;

namespace {

constexpr int OV_MAX_SIDE = 1 << 20;
constexpr long long OV_MAX_PIXELS = 2147483647LL;      // int32 labels, and the bound of the sums: 2^30 * 2^31 = 2^61
constexpr int OV_MIN_SHIFT = -98, OV_MAX_SHIFT = 178;  // 30 - E for the frexp exponents E of float32
constexpr int OVT = 256, OVWAVES = OVT / 64;
constexpr int OV_MAX_GRID = 1024;                      // 4 workgroups per CU, as obj_accumulate and zonal_values
constexpr unsigned OV_POS_INF = 0x7F800000u, OV_NEG_INF = 0xFF800000u;
constexpr unsigned long long LO_MASK = (1ull << 30) - 1;

__device__ __forceinline__ unsigned key_of_bits(unsigned b) { return (b & 0x80000000u) ? ~b : b | 0x80000000u; }
__device__ __forceinline__ unsigned bits_of_key(unsigned k) { return (k & 0x80000000u) ? k ^ 0x80000000u : ~k; }

struct ClassSet { uint32_t w[8]; };

__device__ __forceinline__ bool in_set(const ClassSet& s, unsigned c) { return (s.w[(c >> 5) & 7] >> (c & 31)) & 1u; }

struct Planes {
    const uint8_t* mask;
    const int* labels;
    const float* values;
    const int* offs;
    long long n;
    int P;
    ClassSet exclude;
};

struct Tables {          // every table is [P]
    unsigned long long *valid, *sum_q, *sq_lo, *sq_hi, *mn, *mx;
};

struct Rec {             // the partial sums of some pixels of one key
    unsigned val;
    long long sq;
    unsigned long long lo, hi, mn, mx;
};

__device__ __forceinline__ Rec rec_zero() { return Rec{0u, 0ll, 0ull, 0ull, ~0ull, 0ull}; }

__device__ __forceinline__ void rec_add(Rec& a, const Rec& b) {
    a.val += b.val;
    a.sq += b.sq;
    a.lo += b.lo;
    a.hi += b.hi;
    a.mn = a.mn < b.mn ? a.mn : b.mn;
    a.mx = a.mx > b.mx ? a.mx : b.mx;
}

__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {          // two 32-bit halves
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ Rec rec_shfl(const Rec& r, int src) {
    Rec o;
    o.val = (unsigned)__shfl((int)r.val, src);
    o.sq = (long long)shfl64((unsigned long long)r.sq, src);
    o.lo = shfl64(r.lo, src);
    o.hi = shfl64(r.hi, src);
    o.mn = shfl64(r.mn, src);
    o.mx = shfl64(r.mx, src);
    return o;
}

__device__ __forceinline__ Rec rec_wave_sum(Rec r) {          // the plain reduction: afterwards every lane holds the wave's record
    for (int d = 32; d >= 1; d >>= 1) {
        const Rec o = rec_shfl(r, (int)((threadIdx.x & 63) ^ d));
        rec_add(r, o);
    }
    return r;
}

// the check of the run's label, then the 6 atomics of a run with a valid pixel
__device__ __forceinline__ void ov_flush(const Planes& pl, const Tables& t, int label, unsigned cls, const Rec& r, unsigned& badbits) {
    const long long L = label;
    if (L < 0 || L >= pl.n) { badbits |= 1u; return; }
    const int anchor = pl.labels[L];                  // three independent loads: one round trip
    const unsigned c = pl.mask[L];
    const int k = pl.offs[L];
    if (anchor != label) { badbits |= 2u; return; }
    if (c != cls) { badbits |= 4u; return; }
    if (r.val == 0 || in_set(pl.exclude, cls)) return;
    if ((unsigned)k >= (unsigned)pl.P) return;          // cannot happen: L is an anchor of a kept class
    atomicAdd(t.valid + k, (unsigned long long)r.val);
    atomicAdd(t.sum_q + k, (unsigned long long)r.sq);
    atomicAdd(t.sq_lo + k, r.lo);
    atomicAdd(t.sq_hi + k, r.hi);
    atomicMin(t.mn + k, r.mn);
    atomicMax(t.mx + k, r.mx);
}

struct Group {          // the 4 pixels of one lane
    int l[4];
    unsigned m[4];
    float v[4];
    bool whole;          // all 4 inside the plane and inside the wavefront's span
};

__device__ __forceinline__ void ov_load(const Planes& pl, long long g, long long last, int vec, Group& p) {
    const long long i0 = g * 4;
    p.whole = g < last && i0 + 4 <= pl.n;
    for (int j = 0; j < 4; ++j) {
        p.l[j] = -1;
        p.m[j] = 0u;
        p.v[j] = 0.0f;
    }
    if (p.whole && vec) {
        const int4 ll = *reinterpret_cast<const int4*>(pl.labels + i0);
        const float4 vv = *reinterpret_cast<const float4*>(pl.values + i0);
        const unsigned mm = *reinterpret_cast<const unsigned*>(pl.mask + i0);
        p.l[0] = ll.x; p.l[1] = ll.y; p.l[2] = ll.z; p.l[3] = ll.w;
        p.v[0] = vv.x; p.v[1] = vv.y; p.v[2] = vv.z; p.v[3] = vv.w;
        p.m[0] = mm & 255u; p.m[1] = (mm >> 8) & 255u; p.m[2] = (mm >> 16) & 255u; p.m[3] = mm >> 24;
    } else if (g < last) {
        for (int j = 0; j < 4; ++j)
            if (i0 + j < pl.n) {
                p.l[j] = pl.labels[i0 + j];
                p.m[j] = pl.mask[i0 + j];
                p.v[j] = pl.values[i0 + j];
            }
    }
}

__device__ __forceinline__ bool ov_valid_value(float v, int has_nodata, float nodata) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x7F800000u) != 0x7F800000u && !(has_nodata && v == nodata);
}

// the record of pixel p of a kept class; bit 3 of badbits for |q| > 2^30
__device__ __forceinline__ Rec ov_pixel(float v, unsigned p, int has_nodata, float nodata, double scale, unsigned& badbits) {
    Rec r = rec_zero();
    if (!ov_valid_value(v, has_nodata, nodata)) return r;
    const double t = rint((double)v * scale);          // exact product, then half to even
    if (fabs(t) > 1073741824.0) {
        badbits |= 8u;
        return r;
    }
    const long long q = (long long)t;
    const unsigned long long q2 = (unsigned long long)(q * q);          // <= 2^60
    const unsigned long long key = (unsigned long long)key_of_bits(__float_as_uint(v)) << 32;
    r.val = 1;
    r.sq = q;
    r.lo = q2 & LO_MASK;
    r.hi = q2 >> 30;
    r.mn = key | p;
    r.mx = key | (0xFFFFFFFFu - p);
    return r;
}

// span: the groups of 4 pixels that one wavefront walks, a multiple of 128 (two groups per lane and loop turn: two steps of 256 pixels)
__global__ __launch_bounds__(OVT) void obj_values_kernel(Planes pl, Tables t, long long span, int vec, int has_nodata, float nodata, double scale,
                                                         unsigned long long* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const long long n = pl.n;
    const long long groups = (n + 3) / 4;
    const long long wave = (long long)blockIdx.x * OVWAVES + (threadIdx.x >> 6);
    const long long first = wave * span;
    const long long last = first + span < groups ? first + span : groups;
    unsigned badbits = 0;
    bool has_pend = false;                             // the pending key: the same in all lanes of the wave
    int pend_label = -1;
    unsigned pend_cls = 0;
    Rec pend = rec_zero();                             // this lane's share of the pending record
    for (long long g0 = first; g0 < last; g0 += 128) {
        Group px[2];
        ov_load(pl, g0 + lane, last, vec, px[0]);
        ov_load(pl, g0 + 64 + lane, last, vec, px[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const Group& p = px[h];
            const long long g = g0 + 64 * h + lane, i0 = g * 4;
            bool inside[4];
            Rec one[4];
            for (int j = 0; j < 4; ++j) {
                inside[j] = g < last && i0 + j < n;
                one[j] = inside[j] && !in_set(pl.exclude, p.m[j]) ? ov_pixel(p.v[j], (unsigned)(i0 + j), has_nodata, nodata, scale, badbits)
                                                                  : rec_zero();
            }
            // runs of one key along the lanes: a lane is the head of a run unless it and its left neighbour hold one and the same key on all
            // their pixels
            const bool same = p.whole && p.l[0] == p.l[1] && p.l[1] == p.l[2] && p.l[2] == p.l[3] && p.m[0] == p.m[1] && p.m[1] == p.m[2] &&
                              p.m[2] == p.m[3];
            const int left_l = __shfl_up(p.l[3], 1);
            const unsigned left_m = (unsigned)__shfl_up((int)p.m[3], 1);
            const int left_same = __shfl_up((int)same, 1);
            const bool head = lane == 0 || !same || !left_same || left_l != p.l[0] || left_m != p.m[0];
            const unsigned long long heads = __ballot(head);
            if (heads == 1ull && __shfl((int)same, 0)) {          // one run over the wavefront: it joins the pending record, lane by lane
                const int k = __shfl(p.l[0], 0);
                const unsigned c = (unsigned)__shfl((int)p.m[0], 0);
                if (!has_pend || k != pend_label || c != pend_cls) {
                    if (has_pend) {
                        const Rec all = rec_wave_sum(pend);
                        if (lane == 0) ov_flush(pl, t, pend_label, pend_cls, all, badbits);
                    }
                    has_pend = true;
                    pend_label = k;
                    pend_cls = c;
                    pend = rec_zero();
                }
                for (int j = 0; j < 4; ++j) rec_add(pend, one[j]);
            } else {
                Rec run = one[0];
                for (int j = 1; j < 4; ++j) rec_add(run, one[j]);          // meaningful where `same`
                // segmented reduction: after the step of distance d a lane holds the sum of the lanes from itself to the end of its run or to
                // lane + 2 d - 1; it takes lane + d iff no head lies in lane + 1 .. lane + d
                const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
                for (int d = 1; d < 64; d <<= 1) {
                    const Rec o = rec_shfl(run, lane + d < 64 ? lane + d : lane);
                    if (lane + d < 64 && (after & ((1ull << d) - 1)) == 0) rec_add(run, o);
                }
                if (head) {
                    if (same) {
                        ov_flush(pl, t, p.l[0], p.m[0], run, badbits);
                    } else {          // several keys (or a ragged end): equal neighbours among the 4 pixels are merged
                        bool open = false;
                        int k = -1;
                        unsigned c = 0;
                        Rec r = rec_zero();
                        for (int j = 0; j < 4; ++j) {
                            if (!inside[j]) continue;
                            if (open && (p.l[j] != k || p.m[j] != c)) {
                                ov_flush(pl, t, k, c, r, badbits);
                                open = false;
                            }
                            if (!open) {
                                k = p.l[j];
                                c = p.m[j];
                                r = rec_zero();
                                open = true;
                            }
                            rec_add(r, one[j]);
                        }
                        if (open) ov_flush(pl, t, k, c, r, badbits);
                    }
                }
            }
        }
    }
    if (has_pend) {
        const Rec all = rec_wave_sum(pend);
        if (lane == 0) ov_flush(pl, t, pend_label, pend_cls, all, badbits);
    }
    if (badbits) atomicOr(bad, (unsigned long long)badbits);
}

__global__ __launch_bounds__(OVT) void ov_init_kernel(Tables t, long long P) {
    for (long long k = (long long)blockIdx.x * OVT + threadIdx.x; k < P; k += (long long)gridDim.x * OVT) {
        t.valid[k] = t.sum_q[k] = t.sq_lo[k] = t.sq_hi[k] = 0ull;
        t.mn[k] = ~0ull;
        t.mx[k] = 0ull;
    }
}

// (key << 32 | place) -> the float bits in the low half of the word and the index in the high half, in place
__global__ __launch_bounds__(OVT) void ov_decode_kernel(Tables t, long long P) {
    for (long long k = (long long)blockIdx.x * OVT + threadIdx.x; k < P; k += (long long)gridDim.x * OVT) {
        const unsigned long long mn = t.mn[k], mx = t.mx[k];
        const unsigned long long none = 0xFFFFFFFFull << 32;          // index -1
        t.mn[k] = mn == ~0ull ? none | OV_POS_INF : (mn & 0xFFFFFFFFull) << 32 | bits_of_key((unsigned)(mn >> 32));
        t.mx[k] = mx == 0ull ? none | OV_NEG_INF : (unsigned long long)(0xFFFFFFFFu - (unsigned)mx) << 32 | bits_of_key((unsigned)(mx >> 32));
    }
}

// one wave-level maximum, then one atomic per wavefront
__global__ __launch_bounds__(OVT) void obj_absmax_kernel(const uint8_t* __restrict__ mask, const float* __restrict__ values, long long n, int vec,
                                                         ClassSet exclude, int has_nodata, float nodata, unsigned* __restrict__ absmax) {
    const long long groups = (n + 3) / 4;
    unsigned m = 0;
    for (long long g = (long long)blockIdx.x * OVT + threadIdx.x; g < groups; g += (long long)gridDim.x * OVT) {
        const long long i0 = g * 4;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        unsigned c[4] = {0, 0, 0, 0};
        bool inside[4];
        for (int j = 0; j < 4; ++j) inside[j] = i0 + j < n;
        if (i0 + 4 <= n && vec) {
            const float4 vv = *reinterpret_cast<const float4*>(values + i0);
            const unsigned mm = *reinterpret_cast<const unsigned*>(mask + i0);
            v[0] = vv.x; v[1] = vv.y; v[2] = vv.z; v[3] = vv.w;
            c[0] = mm & 255u; c[1] = (mm >> 8) & 255u; c[2] = (mm >> 16) & 255u; c[3] = mm >> 24;
        } else {
            for (int j = 0; j < 4; ++j)
                if (inside[j]) {
                    v[j] = values[i0 + j];
                    c[j] = mask[i0 + j];
                }
        }
        for (int j = 0; j < 4; ++j)
            if (inside[j] && !in_set(exclude, c[j]) && ov_valid_value(v[j], has_nodata, nodata)) {
                const unsigned a = __float_as_uint(v[j]) & 0x7FFFFFFFu;
                m = a > m ? a : m;
            }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, d);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(absmax, m);
}

bool shape_ok(int H, int W) { return H >= 1 && W >= 1 && H < OV_MAX_SIDE && W < OV_MAX_SIDE && (long long)H * W <= OV_MAX_PIXELS; }

int walk_grid(long long groups) { return groups > (long long)OV_MAX_GRID * OVT ? OV_MAX_GRID : ew_grid(groups, OVT); }

}  // namespace

extern "C" int unet_obj_absmax(const uint8_t* mask, const float* values, int H, int W, const uint32_t* exclude8, int has_nodata, float nodata,
                               long long* absmax, void* stream) {
    UNET_CHECK_ARG(mask && values && exclude8 && absmax, "obj_absmax: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W), "obj_absmax: H, W must be in 1..2^20 - 1 and H * W at most 2^31 - 1 (got %d x %d)", H, W);
    UNET_CHECK_ARG(has_nodata == 0 || has_nodata == 1, "obj_absmax: has_nodata must be 0 or 1 (got %d)", has_nodata);
    const long long n = (long long)H * W;
    hipStream_t st = (hipStream_t)stream;
    UNET_CHECK_HIP(hipMemsetAsync(absmax, 0, sizeof(long long), st));
    ClassSet ex;
    for (int i = 0; i < 8; ++i) ex.w[i] = exclude8[i];
    const int vec = aligned16(values) && (((uintptr_t)mask) & 3) == 0 ? 1 : 0;
    hipLaunchKernelGGL(obj_absmax_kernel, dim3(walk_grid((n + 3) / 4)), dim3(OVT), 0, st, mask, values, n, vec, ex, has_nodata, nodata,
                       reinterpret_cast<unsigned*>(absmax));          // the low half of the little-endian word
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_obj_values(const uint8_t* mask, const int32_t* labels, const float* values, const int32_t* offs, int H, int W,
                               const uint32_t* exclude8, long long P, int has_nodata, float nodata, int shift, long long* table, long long* bad,
                               void* stream) {
    UNET_CHECK_ARG(mask && labels && values && offs && exclude8 && bad, "obj_values: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W), "obj_values: H, W must be in 1..2^20 - 1 and H * W at most 2^31 - 1 (got %d x %d)", H, W);
    const long long n = (long long)H * W;
    UNET_CHECK_ARG(P >= 0 && P <= n && (P == 0 || table), "obj_values: P must be in 0..H * W, with a table unless it is 0 (got %lld)", P);
    UNET_CHECK_ARG(has_nodata == 0 || has_nodata == 1, "obj_values: has_nodata must be 0 or 1 (got %d)", has_nodata);
    UNET_CHECK_ARG(shift >= OV_MIN_SHIFT && shift <= OV_MAX_SHIFT, "obj_values: shift must be in -98..178 (got %d)", shift);
    hipStream_t st = (hipStream_t)stream;
    UNET_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(long long), st));
    Planes pl;
    pl.mask = mask; pl.labels = labels; pl.values = values; pl.offs = offs; pl.n = n; pl.P = (int)P;
    for (int i = 0; i < 8; ++i) pl.exclude.w[i] = exclude8[i];
    unsigned long long* s = reinterpret_cast<unsigned long long*>(table);
    const Tables t{s, s + P, s + 2 * P, s + 3 * P, s + 4 * P, s + 5 * P};          // never dereferenced where P = 0
    const int pgrid = ew_grid(P ? P : 1, OVT);
    if (P) {
        hipLaunchKernelGGL(ov_init_kernel, dim3(pgrid), dim3(OVT), 0, st, t, P);
        UNET_CHECK_LAUNCH();
    }
    const long long groups = (n + 3) / 4;
    const int grid = walk_grid(groups);
    const long long waves = (long long)grid * OVWAVES;
    const long long span = ((groups + waves - 1) / waves + 127) / 128 * 128;          // grid * OVWAVES * span >= groups
    const int vec = aligned16(labels) && aligned16(values) && (((uintptr_t)mask) & 3) == 0 ? 1 : 0;
    hipLaunchKernelGGL(obj_values_kernel, dim3(grid), dim3(OVT), 0, st, pl, t, span, vec, has_nodata, nodata, ldexp(1.0, shift),
                       reinterpret_cast<unsigned long long*>(bad));
    UNET_CHECK_LAUNCH();
    if (P) {
        hipLaunchKernelGGL(ov_decode_kernel, dim3(pgrid), dim3(OVT), 0, st, t, P);
        UNET_CHECK_LAUNCH();
    }
    return UNET_OK;
}
