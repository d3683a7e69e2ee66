// Zonal statistics: the joint histogram of a zone plane and a class mask (unet_amd/zonal.py).
//   unet_zonal_lds_bins   the largest Z * C that the LDS form takes
//   unet_zonal_counts     counts[z, c] += pixels with zone z and mask value c; objects[z, c] += anchors (labels[p] == p) among them
// The planes are one flat run of n = H * W pixels.  A lane owns 4 consecutive pixels per step: one 16-byte load of the zones, one 4-byte
// load of the mask, one 16-byte load of the labels when given, so a wavefront reads 1 KiB / 256 B / 1 KiB of contiguous memory per
// instruction.  A wavefront walks ONE contiguous span of the plane (not a grid stride), so that runs of one key last over many steps:
//   - if all lanes hold one and the same key on all their 4 pixels, the step adds 256 to a pending (key, count) pair that the wave carries in
//     registers, which is written out by one lane only when the key changes or the span ends -- a zone that covers the raster costs one
//     add per span, not one per pixel on one address;
//   - otherwise the keys form runs along the lanes (zones and class regions are coherent): a lane whose 4 pixels hold one key and whose left
//     neighbour holds the same is no head; the head of such a run (a ballot and a find-first-set give its length) adds the run at once,
//     and a lane with several keys merges equal neighbours among its 4 pixels and adds those.
// Z * C <= ZONAL_LDS_BINS: the adds go to a table of uint32 bins in LDS, private to the workgroup, whose non-zero bins are added to counts by
// 64-bit global atomics at the end; a workgroup sees fewer than 2^31 pixels (checked on the host), so a bin cannot wrap.  Anything larger:
// the adds are 64-bit global atomics into counts.  Anchors are rare and always go straight to objects.  Every accumulation is an integer
// add, so the tables do not depend on the order of arrival.  Where a base pointer is not aligned for the wide loads, and on the last
// n % 4 pixels, a lane loads its pixels one by one: no access touches a byte outside the n elements.
#include "common.h"

using namespace unet;

namespace {

constexpr int ZONAL_LDS_BINS = 8192;                  // 32 KiB of LDS per workgroup
constexpr int ZONAL_MAX_SIDE = 1 << 20;               // as the rasterizer
constexpr int ZONAL_MAX_ZONES = 1 << 23;              // as the rasterizer's feature limit
constexpr int ZT = 256, ZWAVES = ZT / 64;
constexpr long long ZONAL_WG_PIXELS = 1LL << 31;
constexpr int ZONAL_MAX_GRID = 1024;                 // 4 workgroups per CU: all of them resident at once in both forms (measured: DESIGN 3.22)

template <bool LDS>
__device__ __forceinline__ void zonal_add(unsigned* bins, unsigned long long* __restrict__ counts, int key, unsigned long long c) {
    if (LDS) atomicAdd(bins + key, (unsigned)c);
    else atomicAdd(counts + key, c);
}

struct Group {          // the 4 pixels of one lane
    int z[4], l[4];
    unsigned m[4];
    bool whole;          // all 4 inside the plane and inside the wavefront's span
};

__device__ __forceinline__ void zonal_load(const int* __restrict__ zones, const uint8_t* __restrict__ mask, const int* __restrict__ labels,
                                           long long g, long long last, long long n, int vec, Group& p) {
    const long long i0 = g * 4;
    p.whole = g < last && i0 + 4 <= n;
    for (int j = 0; j < 4; ++j) {
        p.z[j] = -1;
        p.l[j] = -1;
        p.m[j] = 0;
    }
    if (p.whole && vec) {
        const int4 zz = *reinterpret_cast<const int4*>(zones + i0);
        const unsigned mm = *reinterpret_cast<const unsigned*>(mask + i0);
        p.z[0] = zz.x; p.z[1] = zz.y; p.z[2] = zz.z; p.z[3] = zz.w;
        p.m[0] = mm & 255u; p.m[1] = (mm >> 8) & 255u; p.m[2] = (mm >> 16) & 255u; p.m[3] = mm >> 24;
        if (labels) {
            const int4 ll = *reinterpret_cast<const int4*>(labels + i0);
            p.l[0] = ll.x; p.l[1] = ll.y; p.l[2] = ll.z; p.l[3] = ll.w;
        }
    } else if (g < last) {
        for (int j = 0; j < 4; ++j)
            if (i0 + j < n) {
                p.z[j] = zones[i0 + j];
                p.m[j] = mask[i0 + j];
                if (labels) p.l[j] = labels[i0 + j];
            }
    }
}

// span: the groups of 4 pixels that one wavefront walks, a multiple of 128 (two groups per lane and step, 64 lanes apart, both loaded
// before either is counted)
template <bool LDS>
__global__ __launch_bounds__(ZT) void zonal_counts_kernel(const int* __restrict__ zones, const uint8_t* __restrict__ mask,
                                                          const int* __restrict__ labels, long long n, long long span, int Z, int C, int vec,
                                                          unsigned long long* __restrict__ counts, unsigned long long* __restrict__ objects,
                                                          unsigned long long* __restrict__ bad) {
    __shared__ unsigned bins[LDS ? ZONAL_LDS_BINS : 1];
    const int nb = Z * C;
    if (LDS) {
        for (int b = threadIdx.x; b < nb; b += ZT) bins[b] = 0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const long long groups = (n + 3) / 4;
    const long long wave = (long long)blockIdx.x * ZWAVES + (threadIdx.x >> 6);
    const long long first = wave * span;
    const long long last = first + span < groups ? first + span : groups;
    unsigned badbits = 0;
    int pend_key = -1;                                // the same in all lanes of the wave
    unsigned long long pend = 0;
    for (long long g0 = first; g0 < last; g0 += 128) {
        Group px[2];
        zonal_load(zones, mask, labels, g0 + lane, last, n, vec, px[0]);
        zonal_load(zones, mask, labels, g0 + 64 + lane, last, n, vec, px[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const Group& p = px[h];
            const long long g = g0 + 64 * h + lane, i0 = g * 4;
            int key[4];
            for (int j = 0; j < 4; ++j) {
                const bool inside = g < last && i0 + j < n;
                const bool zbad = inside && (p.z[j] < -1 || p.z[j] >= Z), mbad = inside && p.m[j] >= (unsigned)C;
                badbits |= (mbad ? 1u : 0u) | (zbad ? 2u : 0u);
                key[j] = (!inside || p.z[j] < 0 || zbad || mbad) ? -1 : p.z[j] * C + (int)p.m[j];
                if (labels && key[j] >= 0 && (long long)p.l[j] == i0 + j) atomicAdd(objects + key[j], 1ull);
            }
            // runs of one key along the lanes: a lane is the head of a run unless it and its left neighbour hold one and the same key on all
            // their pixels; the head of a run of such lanes adds the whole run, a lane with several keys adds its own pixels
            const bool same = p.whole && key[0] == key[1] && key[1] == key[2] && key[2] == key[3];
            const int left_key = __shfl_up(key[3], 1);
            const int left_same = __shfl_up((int)same, 1);
            const bool head = lane == 0 || !same || !left_same || left_key != key[0];
            const unsigned long long heads = __ballot(head);
            if (heads == 1ull && __shfl((int)same, 0)) {          // one run over the wavefront: it joins the pending pair
                const int k = __shfl(key[0], 0);
                if (k == pend_key) {
                    pend += 256;
                } else {
                    if (lane == 0 && pend_key >= 0) zonal_add<LDS>(bins, counts, pend_key, pend);
                    pend_key = k;
                    pend = 256;
                }
            } else if (head) {
                if (same) {
                    const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
                    const int len = after ? __ffsll((long long)after) : 64 - lane;          // lanes up to the next head
                    if (key[0] >= 0) zonal_add<LDS>(bins, counts, key[0], 4ull * len);
                } else {
                    int k = key[0];
                    unsigned c = 1;
                    for (int j = 1; j < 4; ++j) {
                        if (key[j] == k) {
                            ++c;
                        } else {
                            if (k >= 0) zonal_add<LDS>(bins, counts, k, c);
                            k = key[j];
                            c = 1;
                        }
                    }
                    if (k >= 0) zonal_add<LDS>(bins, counts, k, c);
                }
            }
        }
    }
    if (lane == 0 && pend_key >= 0) zonal_add<LDS>(bins, counts, pend_key, pend);
    if (badbits) atomicOr(bad, (unsigned long long)badbits);
    if (LDS) {
        __syncthreads();
        for (int b = threadIdx.x; b < nb; b += ZT) {
            const unsigned v = bins[b];
            if (v) atomicAdd(counts + b, (unsigned long long)v);
        }
    }
}

}  // namespace

extern "C" int unet_zonal_lds_bins(void) { return ZONAL_LDS_BINS; }

extern "C" int unet_zonal_counts(const int32_t* zones, const uint8_t* mask, const int32_t* labels, int H, int W, int Z, int C,
                                 long long* counts, long long* objects, long long* bad, void* stream) {
    UNET_CHECK_ARG(zones && mask && counts && bad, "zonal_counts: null pointer");
    UNET_CHECK_ARG((labels == nullptr) == (objects == nullptr), "zonal_counts: labels and objects are given together or not at all");
    UNET_CHECK_ARG(H >= 1 && W >= 1 && H < ZONAL_MAX_SIDE && W < ZONAL_MAX_SIDE, "zonal_counts: H, W must be in 1..2^20 - 1 (got %d x %d)", H, W);
    UNET_CHECK_ARG(Z >= 1 && Z < ZONAL_MAX_ZONES && C >= 1 && C <= 256 && (long long)Z * C < (1LL << 31),
                   "zonal_counts: Z must be in 1..2^23 - 1, C in 1..256 and Z * C under 2^31 (got %d, %d)", Z, C);
    const long long n = (long long)H * W;
    UNET_CHECK_ARG(labels == nullptr || n <= 2147483647LL, "zonal_counts: int32 labels index at most 2^31 - 1 pixels (got %lld)", n);
    hipStream_t st = (hipStream_t)stream;
    UNET_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(long long), st));
    const long long groups = (n + 3) / 4;
    const int grid = groups > (long long)ZONAL_MAX_GRID * ZT ? ZONAL_MAX_GRID : ew_grid(groups, ZT);
    const long long waves = (long long)grid * ZWAVES;
    const long long span = ((groups + waves - 1) / waves + 127) / 128 * 128;          // grid * ZWAVES * span >= groups
    UNET_CHECK_ARG(span * 4 * ZWAVES < ZONAL_WG_PIXELS, "zonal_counts: a workgroup would see 2^31 pixels or more");
    const int vec = aligned16(zones) && (((uintptr_t)mask) & 3) == 0 && (labels == nullptr || aligned16(labels)) ? 1 : 0;
    unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
    unsigned long long* o = reinterpret_cast<unsigned long long*>(objects);
    unsigned long long* b = reinterpret_cast<unsigned long long*>(bad);
    if ((long long)Z * C <= ZONAL_LDS_BINS)
        hipLaunchKernelGGL(zonal_counts_kernel<true>, dim3(grid), dim3(ZT), 0, st, zones, mask, labels, n, span, Z, C, vec, c, o, b);
    else
        hipLaunchKernelGGL(zonal_counts_kernel<false>, dim3(grid), dim3(ZT), 0, st, zones, mask, labels, n, span, Z, C, vec, c, o, b);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
