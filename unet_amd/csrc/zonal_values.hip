// Zonal statistics of a float plane: count, sum, sum of squares, minimum and maximum of a value plane per zone (unet_amd/zonal.py, DESIGN
// 3.25, where the rules are).
//   unet_zonal_absmax     *absmax = the largest bit pattern of |v| over the valid pixels (the host derives the fixed-point shift from it)
//   unet_zonal_values     the tables of every zone in one pass, every accumulation an integer add, minimum or maximum
// A pixel is valid iff its zone lies in 0 .. Z - 1, its value is finite and its value differs from nodata.  A valid value becomes the
// integer q = rint(double(v) * 2^shift) (half to even; the product is exact), |q| <= 2^30, and q^2 = hi * 2^30 + lo with 0 <= lo < 2^30 is
// split BEFORE anything is summed: a plane holds fewer than 2^31 pixels, so sum q, sum lo and sum hi stay within 2^30 * 2^31 = 2^61 and no
// int64 wraps.  Minimum and maximum are taken on the order-preserving unsigned image of the float bits (key(a) < key(b) iff a < b, and
// -0.0 below +0.0), so they are the exact float32 extremes.  Nothing depends on the order of arrival.
// The memory shape is that of zonal_counts_kernel (zonal.hip): a lane owns 4 consecutive pixels per step -- one 16-byte load of the zones,
// one of the values --, two such groups 64 lanes apart are loaded before either is used, and a wavefront walks ONE contiguous span of the
// plane.  Equal zones are merged before anything is added:
//   - a wavefront whose 256 pixels hold one zone adds nothing across lanes at all: every lane adds its partials to a pending record of its
//     own in registers, and the plain wave reduction of those records and the atomics of lane 0 happen once, when the zone changes or the
//     span ends -- a zone that covers the raster costs 7 atomics per span;
//   - otherwise the zones form runs along the lanes: a lane whose 4 pixels hold one zone and whose left neighbour holds the same is no head;
//     the ballot of the heads guards a segmented reduction by shuffles (6 steps, the 64-bit sums moved as two 32-bit halves), after which
//     the head of a run holds the run and issues its atomics; a lane with several zones merges equal neighbours among its 4 pixels and
//     adds those itself.
// Where a base pointer is not 16-byte aligned, and on the last n % 4 pixels, a lane loads its pixels one by one: no access touches a byte
// outside the n elements.  A zone outside -1 .. Z - 1 is counted nowhere and indexes nothing (bit 1 of *bad); a valid pixel with
// |q| > 2^30 -- possible only under a shift that the caller chose -- is left out of the sums (bit 2).
#include "common.h"

using namespace unet;

namespace {

constexpr int ZV_MAX_SIDE = 1 << 20;                   // as the rasterizer
constexpr int ZV_MAX_ZONES = 1 << 23;                  // as the rasterizer's feature limit
constexpr long long ZV_MAX_PIXELS = 2147483647LL;      // the bound of the sums: 2^30 * 2^31 = 2^61
constexpr int ZV_MIN_SHIFT = -98, ZV_MAX_SHIFT = 178;  // 30 - E for the frexp exponents E of float32: -148 .. 128
constexpr int ZVT = 256, ZVWAVES = ZVT / 64;
constexpr int ZV_MAX_GRID = 1024;                      // 4 workgroups per CU, all resident at once (the rule of zonal.hip)
constexpr unsigned KEY_POS_INF = 0xFF800000u;          // key(+inf): what `min` holds for a zone without a valid pixel
constexpr unsigned KEY_NEG_INF = 0x007FFFFFu;          // key(-inf): the same for `max`
constexpr unsigned long long LO_MASK = (1ull << 30) - 1;

__device__ __forceinline__ unsigned key_of_bits(unsigned b) { return (b & 0x80000000u) ? ~b : b | 0x80000000u; }
__device__ __forceinline__ unsigned bits_of_key(unsigned k) { return (k & 0x80000000u) ? k ^ 0x80000000u : ~k; }

struct Tables {          // every table is [Z]
    unsigned long long *pixels, *valid, *sum_q, *sq_lo, *sq_hi;
    unsigned *mn, *mx;          // keys while the pass runs, float bits after zv_decode_kernel
};

struct Rec {             // the partial sums of some pixels of one zone
    unsigned pix, val;
    long long sq;
    unsigned long long lo, hi;
    unsigned mn, mx;
};

__device__ __forceinline__ Rec rec_zero() { return Rec{0u, 0u, 0ll, 0ull, 0ull, 0xFFFFFFFFu, 0u}; }

__device__ __forceinline__ void rec_add(Rec& a, const Rec& b) {
    a.pix += b.pix;
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
    o.pix = (unsigned)__shfl((int)r.pix, src);
    o.val = (unsigned)__shfl((int)r.val, src);
    o.sq = (long long)shfl64((unsigned long long)r.sq, src);
    o.lo = shfl64(r.lo, src);
    o.hi = shfl64(r.hi, src);
    o.mn = (unsigned)__shfl((int)r.mn, src);
    o.mx = (unsigned)__shfl((int)r.mx, src);
    return o;
}

// the 7 atomics of one record (1 when it holds no valid pixel): 64-bit adds, sum_q in two's complement, and a 32-bit min and max
__device__ __forceinline__ void rec_emit(const Tables& t, int z, const Rec& r) {
    if (z < 0 || r.pix == 0) return;
    atomicAdd(t.pixels + z, (unsigned long long)r.pix);
    if (r.val == 0) return;
    atomicAdd(t.valid + z, (unsigned long long)r.val);
    atomicAdd(t.sum_q + z, (unsigned long long)r.sq);
    atomicAdd(t.sq_lo + z, r.lo);
    atomicAdd(t.sq_hi + z, r.hi);
    atomicMin(t.mn + z, r.mn);
    atomicMax(t.mx + z, r.mx);
}

struct Group {          // the 4 pixels of one lane
    int z[4];
    float v[4];
    bool whole;          // all 4 inside the plane and inside the wavefront's span
};

__device__ __forceinline__ void zv_load(const int* __restrict__ zones, const float* __restrict__ values, long long g, long long last, long long n,
                                        int vec, Group& p) {
    const long long i0 = g * 4;
    p.whole = g < last && i0 + 4 <= n;
    for (int j = 0; j < 4; ++j) {
        p.z[j] = -1;
        p.v[j] = 0.0f;
    }
    if (p.whole && vec) {
        const int4 zz = *reinterpret_cast<const int4*>(zones + i0);
        const float4 vv = *reinterpret_cast<const float4*>(values + i0);
        p.z[0] = zz.x; p.z[1] = zz.y; p.z[2] = zz.z; p.z[3] = zz.w;
        p.v[0] = vv.x; p.v[1] = vv.y; p.v[2] = vv.z; p.v[3] = vv.w;
    } else if (g < last) {
        for (int j = 0; j < 4; ++j)
            if (i0 + j < n) {
                p.z[j] = zones[i0 + j];
                p.v[j] = values[i0 + j];
            }
    }
}

__device__ __forceinline__ bool zv_valid_value(float v, int has_nodata, float nodata) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x7F800000u) != 0x7F800000u && !(has_nodata && v == nodata);
}

// the record of one pixel of a zone (z >= 0); bit 2 of badbits for |q| > 2^30
__device__ __forceinline__ Rec zv_pixel(float v, int has_nodata, float nodata, double scale, unsigned& badbits) {
    Rec r = rec_zero();
    r.pix = 1;
    if (!zv_valid_value(v, has_nodata, nodata)) return r;
    const double t = rint((double)v * scale);          // exact product, then half to even
    if (fabs(t) > 1073741824.0) {
        badbits |= 4u;
        return r;
    }
    const long long q = (long long)t;
    const unsigned long long q2 = (unsigned long long)(q * q);          // <= 2^60
    r.val = 1;
    r.sq = q;
    r.lo = q2 & LO_MASK;
    r.hi = q2 >> 30;
    r.mn = r.mx = key_of_bits(__float_as_uint(v));
    return r;
}

__device__ __forceinline__ Rec rec_wave_sum(Rec r) {          // the plain reduction: afterwards every lane holds the wave's record
    for (int d = 32; d >= 1; d >>= 1) {
        const Rec o = rec_shfl(r, (int)((threadIdx.x & 63) ^ d));
        rec_add(r, o);
    }
    return r;
}

// span: the groups of 4 pixels that one wavefront walks, a multiple of 128 (two groups per lane and step)
__global__ __launch_bounds__(ZVT) void zonal_values_kernel(const int* __restrict__ zones, const float* __restrict__ values, long long n, long long span,
                                                           int Z, int vec, int has_nodata, float nodata, double scale, Tables t,
                                                           unsigned long long* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const long long groups = (n + 3) / 4;
    const long long wave = (long long)blockIdx.x * ZVWAVES + (threadIdx.x >> 6);
    const long long first = wave * span;
    const long long last = first + span < groups ? first + span : groups;
    unsigned badbits = 0;
    int pend_zone = -1;                                // the same in all lanes of the wave
    Rec pend = rec_zero();                             // this lane's share of the pending record
    for (long long g0 = first; g0 < last; g0 += 128) {
        Group px[2];
        zv_load(zones, values, g0 + lane, last, n, vec, px[0]);
        zv_load(zones, values, g0 + 64 + lane, last, n, vec, px[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const Group& p = px[h];
            const long long g = g0 + 64 * h + lane, i0 = g * 4;
            int zone[4];
            Rec one[4];
            for (int j = 0; j < 4; ++j) {
                const bool inside = g < last && i0 + j < n;
                const bool zbad = inside && (p.z[j] < -1 || p.z[j] >= Z);
                badbits |= zbad ? 2u : 0u;
                zone[j] = (!inside || zbad) ? -1 : p.z[j];          // a bad zone indexes nothing
                one[j] = zone[j] >= 0 ? zv_pixel(p.v[j], has_nodata, nodata, scale, badbits) : rec_zero();
            }
            // runs of one zone along the lanes: a lane is the head of a run unless it and its left neighbour hold one and the same zone on all
            // their pixels
            const bool same = p.whole && zone[0] == zone[1] && zone[1] == zone[2] && zone[2] == zone[3];
            const int left_zone = __shfl_up(zone[3], 1);
            const int left_same = __shfl_up((int)same, 1);
            const bool head = lane == 0 || !same || !left_same || left_zone != zone[0];
            const unsigned long long heads = __ballot(head);
            if (heads == 1ull && __shfl((int)same, 0)) {          // one run over the wavefront: it joins the pending record, lane by lane
                const int k = __shfl(zone[0], 0);
                if (k != pend_zone) {
                    const Rec all = rec_wave_sum(pend);
                    if (lane == 0) rec_emit(t, pend_zone, all);
                    pend_zone = k;
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
                        rec_emit(t, zone[0], run);
                    } else {          // several zones (or a ragged end): equal neighbours among the 4 pixels are merged
                        int k = zone[0];
                        Rec r = one[0];
                        for (int j = 1; j < 4; ++j) {
                            if (zone[j] == k) {
                                rec_add(r, one[j]);
                            } else {
                                rec_emit(t, k, r);
                                k = zone[j];
                                r = one[j];
                            }
                        }
                        rec_emit(t, k, r);
                    }
                }
            }
        }
    }
    {
        const Rec all = rec_wave_sum(pend);
        if (lane == 0) rec_emit(t, pend_zone, all);
    }
    if (badbits) atomicOr(bad, (unsigned long long)badbits);
}

__global__ __launch_bounds__(ZVT) void zv_init_kernel(Tables t, int Z) {
    for (int z = blockIdx.x * ZVT + threadIdx.x; z < Z; z += gridDim.x * ZVT) {
        t.pixels[z] = t.valid[z] = t.sum_q[z] = t.sq_lo[z] = t.sq_hi[z] = 0ull;
        t.mn[z] = KEY_POS_INF;
        t.mx[z] = KEY_NEG_INF;
    }
}

__global__ __launch_bounds__(ZVT) void zv_decode_kernel(Tables t, int Z) {          // keys -> float bits, in place
    for (int z = blockIdx.x * ZVT + threadIdx.x; z < Z; z += gridDim.x * ZVT) {
        t.mn[z] = bits_of_key(t.mn[z]);
        t.mx[z] = bits_of_key(t.mx[z]);
    }
}

// one wave-level maximum, then one atomic per wavefront
__global__ __launch_bounds__(ZVT) void zonal_absmax_kernel(const int* __restrict__ zones, const float* __restrict__ values, long long n, int Z, int vec,
                                                           int has_nodata, float nodata, unsigned* __restrict__ absmax) {
    const long long groups = (n + 3) / 4;
    unsigned m = 0;
    for (long long g = (long long)blockIdx.x * ZVT + threadIdx.x; g < groups; g += (long long)gridDim.x * ZVT) {
        Group p;
        zv_load(zones, values, g, groups, n, vec, p);          // outside the plane: zone -1
        for (int j = 0; j < 4; ++j)
            if (p.z[j] >= 0 && p.z[j] < Z && zv_valid_value(p.v[j], has_nodata, nodata)) {
                const unsigned a = __float_as_uint(p.v[j]) & 0x7FFFFFFFu;
                m = a > m ? a : m;
            }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, d);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(absmax, m);
}

}  // namespace

#define ZV_CHECK_PLANE(what)                                                                                                                     \
    UNET_CHECK_ARG(H >= 1 && W >= 1 && H < ZV_MAX_SIDE && W < ZV_MAX_SIDE, what ": H, W must be in 1..2^20 - 1 (got %d x %d)", H, W);            \
    UNET_CHECK_ARG((long long)H * W <= ZV_MAX_PIXELS, what ": at most 2^31 - 1 pixels (got %lld)", (long long)H * W);                           \
    UNET_CHECK_ARG(Z >= 1 && Z < ZV_MAX_ZONES, what ": Z must be in 1..2^23 - 1 (got %d)", Z);                                                  \
    UNET_CHECK_ARG(has_nodata == 0 || has_nodata == 1, what ": has_nodata must be 0 or 1 (got %d)", has_nodata)

extern "C" int unet_zonal_absmax(const int32_t* zones, const float* values, int H, int W, int Z, int has_nodata, float nodata, long long* absmax,
                                 void* stream) {
    UNET_CHECK_ARG(zones && values && absmax, "zonal_absmax: null pointer");
    ZV_CHECK_PLANE("zonal_absmax");
    const long long n = (long long)H * W;
    hipStream_t st = (hipStream_t)stream;
    UNET_CHECK_HIP(hipMemsetAsync(absmax, 0, sizeof(long long), st));
    const long long groups = (n + 3) / 4;
    const int grid = groups > (long long)ZV_MAX_GRID * ZVT ? ZV_MAX_GRID : ew_grid(groups, ZVT);
    const int vec = aligned16(zones) && aligned16(values) ? 1 : 0;
    hipLaunchKernelGGL(zonal_absmax_kernel, dim3(grid), dim3(ZVT), 0, st, zones, values, n, Z, vec, has_nodata, nodata,
                       reinterpret_cast<unsigned*>(absmax));          // the low half of the little-endian word
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_zonal_values(const int32_t* zones, const float* values, int H, int W, int Z, int has_nodata, float nodata, int shift,
                                 long long* sums, float* minmax, long long* bad, void* stream) {
    UNET_CHECK_ARG(zones && values && sums && minmax && bad, "zonal_values: null pointer");
    ZV_CHECK_PLANE("zonal_values");
    UNET_CHECK_ARG(shift >= ZV_MIN_SHIFT && shift <= ZV_MAX_SHIFT, "zonal_values: shift must be in -98..178 (got %d)", shift);
    const long long n = (long long)H * W;
    hipStream_t st = (hipStream_t)stream;
    UNET_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(long long), st));
    unsigned long long* s = reinterpret_cast<unsigned long long*>(sums);
    unsigned* mm = reinterpret_cast<unsigned*>(minmax);
    const Tables t{s, s + Z, s + 2LL * Z, s + 3LL * Z, s + 4LL * Z, mm, mm + Z};
    const int zgrid = ew_grid(Z, ZVT);
    hipLaunchKernelGGL(zv_init_kernel, dim3(zgrid), dim3(ZVT), 0, st, t, Z);
    UNET_CHECK_LAUNCH();
    const long long groups = (n + 3) / 4;
    const int grid = groups > (long long)ZV_MAX_GRID * ZVT ? ZV_MAX_GRID : ew_grid(groups, ZVT);
    const long long waves = (long long)grid * ZVWAVES;
    const long long span = ((groups + waves - 1) / waves + 127) / 128 * 128;          // grid * ZVWAVES * span >= groups
    const int vec = aligned16(zones) && aligned16(values) ? 1 : 0;
    hipLaunchKernelGGL(zonal_values_kernel, dim3(grid), dim3(ZVT), 0, st, zones, values, n, span, Z, vec, has_nodata, nodata, ldexp(1.0, shift), t,
                       reinterpret_cast<unsigned long long*>(bad));
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(zv_decode_kernel, dim3(zgrid), dim3(ZVT), 0, st, t, Z);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
