// Arc-based Douglas-Peucker simplification of the traced rings on the device (unet_amd/vectorize.py), in exact integer
// arithmetic.  The candidates of every ring (its corners and the nodes it passes) lie in ring order in arrays over C candidates; the
// placement, the scans and the coordinates come from the launchers of vectorize.hip.
//   unet_simp_marks        per edge: bit 0 = its end vertex is a candidate (corner or node), bit 4 = it is a node
//   unet_simp_gather       per candidate: the ring index and the node mark
//   unet_simp_closed       rings with fewer than two nodes: the anchor and the candidate farthest from it; then the keep marks (nodes,
//                          anchors, far points) and the cyclic neighbours that start the nearest-kept search
//   unet_simp_near_rounds  pointer doubling: lo / hi = the nearest kept candidate before / after, cyclic within the ring
//   unet_simp_dp_rounds    Douglas-Peucker rounds: |cross| against the chord, a segmented arg-max, the exact test of the winner
//   unet_simp_emit         the kept vertices of the surviving rings, and their ring index
//   unet_simp_area         twice the signed area of every ring of the result
// Atomics decide no position: they take a minimum, a maximum (which do not depend on the order of arrival) or an exact integer sum.
#include "common.h"

using namespace unet;

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ bool in_range(long long p, long long n) { return p >= 0 && p < n; }

__device__ __forceinline__ uint32_t vertex_index(int x, int y, int W) { return (uint32_t)((u64)y * (u64)(W + 1) + (u64)x); }

// ------------------------------------------------------------------------------------------------------------------ node marks

__global__ __launch_bounds__(256) void simp_marks_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ flags,
                                                         const int* __restrict__ offs, const uint8_t* __restrict__ corner, int H, int W,
                                                         long long E, uint8_t* __restrict__ cand) {
    const long long n = (long long)H * W;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const unsigned f = flags[p];
        if (f == 0) continue;
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        int e = offs[p];
        for (int s = 0; s < 4; ++s) {
            if (!((f >> s) & 1u)) continue;
            if (in_range(e, E)) {
                const int vx = x + (s >= 2 ? 1 : 0), vy = y + (s == 1 || s == 2 ? 1 : 0);          // the end vertex
                // the four pixels around it; outside the raster (decided by coordinates, never read) is the label -1
                const bool up = vy > 0, down = vy < H, left = vx > 0, right = vx < W;
                const long long q = (long long)vy * W + vx;
                const int nw = up && left ? labels[q - W - 1] : -1, ne = up && right ? labels[q - W] : -1;
                const int sw = down && left ? labels[q - 1] : -1, se = down && right ? labels[q] : -1;
                const int borders = (nw != ne) + (sw != se) + (nw != sw) + (ne != se);
                const bool node = borders >= 3 || ((vx == 0 || vx == W) && (vy == 0 || vy == H));
                cand[e] = (uint8_t)((corner[e] || node ? 1 : 0) | (node ? 16 : 0));
            }
            ++e;
        }
    }
}

__global__ __launch_bounds__(256) void simp_gather_kernel(const int* __restrict__ ring, const int* __restrict__ ridx, const int* __restrict__ pos,
                                                          const int* __restrict__ coff, const uint8_t* __restrict__ cand, long long E, long long R,
                                                          long long C, int* __restrict__ cring, uint8_t* __restrict__ cnode) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        const unsigned m = cand[e];
        if (!(m & 1u)) continue;
        const int lead = ring[e], at = pos[e];
        if (!in_range(lead, E) || !in_range(at, E)) continue;
        const long long r = ridx[lead], k = coff[at];
        if (!in_range(r, R) || !in_range(k, C)) continue;
        cring[k] = (int)r;
        cnode[k] = (uint8_t)(m >> 4);
    }
}

// ------------------------------------------------------------------------------------------------------------------ closed arcs

// anchor key: nodes first, then the smallest (y, x); the low 31 bits carry the candidate
__global__ __launch_bounds__(256) void simp_anchor_kernel(const int2* __restrict__ cxy, const int* __restrict__ cring, const uint8_t* __restrict__ cnode,
                                                          long long C, long long R, int W, int* __restrict__ nnodes, u64* __restrict__ akey) {
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < C; k += (long long)gridDim.x * 256) {
        const long long r = cring[k];
        if (!in_range(r, R)) continue;
        const int2 z = cxy[k];
        const bool node = cnode[k] != 0;
        if (node) atomicAdd(nnodes + r, 1);
        atomicMin(akey + r, ((u64)(node ? 0 : 1) << 63) | ((u64)vertex_index(z.x, z.y, W) << 31) | (u64)k);
    }
}

__device__ __forceinline__ u64 dist2(int2 a, int2 b) {
    const long long dx = (long long)a.x - b.x, dy = (long long)a.y - b.y;
    return (u64)(dx * dx) + (u64)(dy * dy);
}

__global__ __launch_bounds__(256) void simp_far_kernel(const int2* __restrict__ cxy, const int* __restrict__ cring, long long C, long long R, int W,
                                                       const int* __restrict__ nnodes, const u64* __restrict__ akey, u64* __restrict__ fard,
                                                       u64* __restrict__ fark, int second) {
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < C; k += (long long)gridDim.x * 256) {
        const long long r = cring[k];
        if (!in_range(r, R) || nnodes[r] > 1) continue;
        const long long a = (long long)(akey[r] & 0x7FFFFFFFull);
        if (!in_range(a, C) || a == k) continue;
        const int2 z = cxy[k];
        const u64 d = dist2(z, cxy[a]);
        if (!second) atomicMax(fard + r, d);
        else if (d == fard[r]) atomicMin(fark + r, ((u64)vertex_index(z.x, z.y, W) << 31) | (u64)k);          // ties: the smallest (y, x)
    }
}

__global__ __launch_bounds__(256) void simp_init_kernel(const int* __restrict__ cring, const uint8_t* __restrict__ cnode, const int* __restrict__ cs,
                                                        const int* __restrict__ cn, long long C, long long R, const int* __restrict__ nnodes,
                                                        const u64* __restrict__ akey, const u64* __restrict__ fark, uint8_t* __restrict__ keep,
                                                        int* __restrict__ lo, int* __restrict__ hi) {
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < C; k += (long long)gridDim.x * 256) {
        const long long r = cring[k];
        bool kp = true;          // (a candidate without a ring is never one; it is kept and points at itself)
        long long before = k, after = k;
        if (in_range(r, R)) {
            const long long s = cs[r], n = cn[r];
            kp = cnode[k] != 0;
            if (nnodes[r] <= 1) kp = kp || (long long)(akey[r] & 0x7FFFFFFFull) == k || (long long)(fark[r] & 0x7FFFFFFFull) == k;
            if (!kp && n > 0 && k >= s && k < s + n && s >= 0 && s + n <= C) {
                before = k == s ? s + n - 1 : k - 1;
                after = k == s + n - 1 ? s : k + 1;
            } else {
                kp = true;
            }
        }
        keep[k] = kp ? 1 : 0;
        lo[k] = (int)before;
        hi[k] = (int)after;
    }
}

__global__ __launch_bounds__(256) void simp_near_round_kernel(const int* __restrict__ lo, const int* __restrict__ hi, long long C, int* __restrict__ lo2,
                                                              int* __restrict__ hi2, int* __restrict__ changed) {
    bool any = false;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < C; k += (long long)gridDim.x * 256) {
        const int l = lo[k], h = hi[k];
        const int l2 = in_range(l, C) ? lo[l] : l, h2 = in_range(h, C) ? hi[h] : h;
        lo2[k] = l2;
        hi2[k] = h2;
        any |= l2 != l || h2 != h;
    }
    if (__any(any) && (threadIdx.x & 63) == 0) *changed = 1;
}

// ------------------------------------------------------------------------------------------------------------------ Douglas-Peucker rounds

// lo[k] < 0: k is kept or dropped for good.  Otherwise k is live in the segment lo[k] .. hi[k].  Only thread k reads or writes lo[k] / hi[k].
__global__ __launch_bounds__(256) void simp_key_kernel(const int2* __restrict__ cxy, const int* __restrict__ cring, const int* __restrict__ cn,
                                                       const uint8_t* __restrict__ keep, const int* __restrict__ win,
                                                       long long C, long long R, int W, int first, int* __restrict__ lo, int* __restrict__ hi,
                                                       u64* __restrict__ key, u64* __restrict__ slot) {
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < C; k += (long long)gridDim.x * 256) {
        int l = lo[k], h = hi[k];
        if (l < 0) continue;
        if (!in_range(l, C) || !in_range(h, C)) { lo[k] = -1; continue; }
        if (first) {
            if (keep[k]) { lo[k] = -1; continue; }
        } else {
            // the previous round's winner of this segment: kept (the segment splits there) or not (the whole interior is dropped)
            const int w = win[l];
            const long long r = cring[k];
            if (w < 0 || w == k || !in_range(w, C) || !in_range(r, R)) { lo[k] = -1; continue; }
            const int n = cn[r];
            int a = (int)k - l, b = w - l;
            if (a < 0) a += n;
            if (b < 0) b += n;
            if (a < b) hi[k] = h = w;
            else lo[k] = l = w;
        }
        const int2 p = cxy[l], q = cxy[h], z = cxy[k];
        long long c = ((long long)q.x - p.x) * ((long long)z.y - p.y) - ((long long)q.y - p.y) * ((long long)z.x - p.x);
        if (c < 0) c = -c;
        const u64 v = ((u64)c << 32) | (u64)(uint32_t)~vertex_index(z.x, z.y, W);          // |c| < 2^31 for H * W < 2^31; ties: the smallest (y, x)
        key[k] = v;
        atomicMax(slot + l, v);
    }
}

__global__ __launch_bounds__(256) void simp_test_kernel(const int2* __restrict__ cxy, const int* __restrict__ lo, const int* __restrict__ hi,
                                                        const u64* __restrict__ key, const u64* __restrict__ slot, long long C, u64 q2,
                                                        int* __restrict__ win, uint8_t* __restrict__ keep, int* __restrict__ changed) {
    bool any = false;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < C; k += (long long)gridDim.x * 256) {
        const int l = lo[k];
        if (!in_range(l, C)) continue;
        const u64 v = key[k];
        if (v != slot[l]) continue;          // the vertex index is unique within a ring: one winner per segment
        const int h = hi[k];
        if (!in_range(h, C)) continue;
        const u64 c = v >> 32;
        const unsigned __int128 lhs = (unsigned __int128)(c * c) * 256u;                                   // c^2 < 2^62
        const unsigned __int128 rhs = (unsigned __int128)q2 * (unsigned __int128)dist2(cxy[l], cxy[h]);    // q^2 <= 2^32, |Q - P|^2 < 2^63
        const bool kp = lhs > rhs;
        win[l] = kp ? (int)k : -1;
        if (kp) keep[k] = 1;
        any = true;          // the round had a live segment
    }
    if (__any(any) && (threadIdx.x & 63) == 0) *changed = 1;
}

// ------------------------------------------------------------------------------------------------------------------ result

__global__ __launch_bounds__(256) void simp_emit_kernel(const int2* __restrict__ cxy, const int* __restrict__ cring, const uint8_t* __restrict__ keep,
                                                        const int* __restrict__ koff, const int* __restrict__ kstart, const long long* __restrict__ vbase,
                                                        const int* __restrict__ newring, long long C, long long R, long long V, int2* __restrict__ xy,
                                                        int* __restrict__ vring) {
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < C; k += (long long)gridDim.x * 256) {
        if (!keep[k]) continue;
        const long long r = cring[k];
        if (!in_range(r, R)) continue;
        const int nr = newring[r];
        if (nr < 0) continue;          // a dropped ring
        const long long v = vbase[r] + ((long long)koff[k] - kstart[r]);
        if (!in_range(v, V)) continue;
        xy[v] = cxy[k];
        vring[v] = nr;
    }
}

__global__ __launch_bounds__(256) void simp_area_kernel(const int2* __restrict__ xy, const int* __restrict__ vring, const long long* __restrict__ ring_start,
                                                        long long V, long long R, long long* __restrict__ area2) {
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long long)gridDim.x * 256) {
        const long long r = vring[v];
        if (!in_range(r, R)) continue;
        const long long nx = v + 1 < ring_start[r + 1] ? v + 1 : ring_start[r];
        if (!in_range(nx, V)) continue;
        const int2 a = xy[v], b = xy[nx];
        const long long t = (long long)b.x * a.y - (long long)a.x * b.y;
        atomicAdd(reinterpret_cast<u64*>(area2 + r), (u64)t);          // an exact sum: the order of arrival does not show
    }
}

bool shape_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W <= 2147483647LL; }
bool count_ok(long long n) { return n > 0 && n <= 2147483647LL; }
bool al8(const void* p) { return (((uintptr_t)p) & 7) == 0; }

}  // namespace

extern "C" int unet_simp_marks(const int32_t* labels, const uint8_t* flags, const int32_t* offs, const uint8_t* corner, int H, int W, long long E,
                               uint8_t* cand, void* stream) {
    UNET_CHECK_ARG(labels && flags && offs && corner && cand, "simp_marks: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W) && count_ok(E), "simp_marks: H * W and E must be in 1..2^31 - 1 (got %d x %d, %lld)", H, W, E);
    hipLaunchKernelGGL(simp_marks_kernel, dim3(ew_grid((long long)H * W, 256)), dim3(256), 0, (hipStream_t)stream, labels, flags, offs, corner, H, W, E,
                       cand);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_simp_gather(const int32_t* ring, const int32_t* ridx, const int32_t* pos, const int32_t* coff, const uint8_t* cand, long long E,
                                long long R, long long C, int32_t* cring, uint8_t* cnode, void* stream) {
    UNET_CHECK_ARG(ring && ridx && pos && coff && cand && cring && cnode, "simp_gather: null pointer");
    UNET_CHECK_ARG(count_ok(E) && count_ok(R) && count_ok(C) && C <= E, "simp_gather: E, R and C <= E must be in 1..2^31 - 1 (got %lld, %lld, %lld)", E, R, C);
    hipLaunchKernelGGL(simp_gather_kernel, dim3(ew_grid(E, 256)), dim3(256), 0, (hipStream_t)stream, ring, ridx, pos, coff, cand, E, R, C, cring, cnode);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_simp_closed(const int32_t* cxy, const int32_t* cring, const uint8_t* cnode, const int32_t* cs, const int32_t* cn, long long C,
                                long long R, int W, int32_t* nnodes, unsigned long long* akey, unsigned long long* fard, unsigned long long* fark,
                                uint8_t* keep, int32_t* lo, int32_t* hi, void* stream) {
    UNET_CHECK_ARG(cxy && cring && cnode && cs && cn && nnodes && akey && fard && fark && keep && lo && hi, "simp_closed: null pointer");
    UNET_CHECK_ARG(count_ok(C) && count_ok(R) && R <= C && W > 0, "simp_closed: C, R <= C must be in 1..2^31 - 1 and W positive (got %lld, %lld, %d)", C, R, W);
    UNET_CHECK_ARG(al8(cxy) && al8(akey) && al8(fard) && al8(fark), "simp_closed: cxy and the key arrays must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int grid = ew_grid(C, 256);
    const int2* xy = reinterpret_cast<const int2*>(cxy);
    UNET_CHECK_HIP(hipMemsetAsync(nnodes, 0, (size_t)R * sizeof(int32_t), st));
    UNET_CHECK_HIP(hipMemsetAsync(akey, 0xFF, (size_t)R * sizeof(u64), st));
    UNET_CHECK_HIP(hipMemsetAsync(fard, 0, (size_t)R * sizeof(u64), st));
    UNET_CHECK_HIP(hipMemsetAsync(fark, 0xFF, (size_t)R * sizeof(u64), st));
    hipLaunchKernelGGL(simp_anchor_kernel, dim3(grid), dim3(256), 0, st, xy, cring, cnode, C, R, W, nnodes, akey);
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(simp_far_kernel, dim3(grid), dim3(256), 0, st, xy, cring, C, R, W, nnodes, akey, fard, fark, 0);
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(simp_far_kernel, dim3(grid), dim3(256), 0, st, xy, cring, C, R, W, nnodes, akey, fard, fark, 1);
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(simp_init_kernel, dim3(grid), dim3(256), 0, st, cring, cnode, cs, cn, C, R, nnodes, akey, fark, keep, lo, hi);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_simp_near_rounds(long long C, int32_t* lo_a, int32_t* hi_a, int32_t* lo_b, int32_t* hi_b, int rounds, int32_t* changed,
                                     void* stream) {
    UNET_CHECK_ARG(lo_a && hi_a && lo_b && hi_b && changed, "simp_near_rounds: null pointer");
    UNET_CHECK_ARG(count_ok(C) && rounds >= 0 && rounds <= 64, "simp_near_rounds: C must be in 1..2^31 - 1 and rounds in 0..64 (got %lld, %d)", C, rounds);
    UNET_CHECK_ARG(lo_a != lo_b && hi_a != hi_b && lo_a != hi_a && lo_b != hi_b && lo_a != hi_b && lo_b != hi_a, "simp_near_rounds: the four buffers must differ");
    hipStream_t st = (hipStream_t)stream;
    const int grid = ew_grid(C, 256);
    if (rounds > 0) UNET_CHECK_HIP(hipMemsetAsync(changed, 0, (size_t)rounds * sizeof(int32_t), st));
    for (int r = 0; r < rounds; ++r) {          // round r reads set a (r even) or b (r odd) and writes the other
        if (r % 2 == 0) hipLaunchKernelGGL(simp_near_round_kernel, dim3(grid), dim3(256), 0, st, lo_a, hi_a, C, lo_b, hi_b, changed + r);
        else hipLaunchKernelGGL(simp_near_round_kernel, dim3(grid), dim3(256), 0, st, lo_b, hi_b, C, lo_a, hi_a, changed + r);
        UNET_CHECK_LAUNCH();
    }
    return UNET_OK;
}

extern "C" int unet_simp_dp_rounds(const int32_t* cxy, const int32_t* cring, const int32_t* cn, long long C, long long R, int W, int q,
                                   int first, int rounds, uint8_t* keep, int32_t* lo, int32_t* hi, unsigned long long* key, unsigned long long* slot,
                                   int32_t* win, int32_t* changed, void* stream) {
    UNET_CHECK_ARG(cxy && cring && cn && keep && lo && hi && key && slot && win && changed, "simp_dp_rounds: null pointer");
    UNET_CHECK_ARG(count_ok(C) && count_ok(R) && W > 0 && rounds >= 0 && rounds <= 64,
                   "simp_dp_rounds: C, R must be in 1..2^31 - 1, W positive and rounds in 0..64 (got %lld, %lld, %d, %d)", C, R, W, rounds);
    UNET_CHECK_ARG(q >= 0 && q <= 65536, "simp_dp_rounds: q (sixteenths of a pixel) must be in 0..65536 (got %d)", q);
    UNET_CHECK_ARG(al8(cxy) && al8(key) && al8(slot) && key != slot && lo != hi && lo != win && hi != win,
                   "simp_dp_rounds: cxy, key and slot must be 8-byte aligned and the work buffers must differ");
    hipStream_t st = (hipStream_t)stream;
    const int grid = ew_grid(C, 256);
    const int2* xy = reinterpret_cast<const int2*>(cxy);
    if (rounds > 0) UNET_CHECK_HIP(hipMemsetAsync(changed, 0, (size_t)rounds * sizeof(int32_t), st));
    for (int r = 0; r < rounds; ++r) {
        UNET_CHECK_HIP(hipMemsetAsync(slot, 0, (size_t)C * sizeof(u64), st));
        hipLaunchKernelGGL(simp_key_kernel, dim3(grid), dim3(256), 0, st, xy, cring, cn, keep, win, C, R, W, (first && r == 0) ? 1 : 0, lo, hi, key, slot);
        UNET_CHECK_LAUNCH();
        hipLaunchKernelGGL(simp_test_kernel, dim3(grid), dim3(256), 0, st, xy, lo, hi, key, slot, C, (u64)q * (u64)q, win, keep, changed + r);
        UNET_CHECK_LAUNCH();
    }
    return UNET_OK;
}

extern "C" int unet_simp_emit(const int32_t* cxy, const int32_t* cring, const uint8_t* keep, const int32_t* koff, const int32_t* kstart,
                              const long long* vbase, const int32_t* newring, long long C, long long R, long long V, int32_t* xy, int32_t* vring,
                              void* stream) {
    UNET_CHECK_ARG(cxy && cring && keep && koff && kstart && vbase && newring && xy && vring, "simp_emit: null pointer");
    UNET_CHECK_ARG(count_ok(C) && count_ok(R) && count_ok(V) && V <= C, "simp_emit: C, R and V <= C must be in 1..2^31 - 1 (got %lld, %lld, %lld)", C, R, V);
    UNET_CHECK_ARG(al8(cxy) && al8(xy), "simp_emit: cxy and xy must be 8-byte aligned");
    hipLaunchKernelGGL(simp_emit_kernel, dim3(ew_grid(C, 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const int2*>(cxy), cring, keep, koff,
                       kstart, vbase, newring, C, R, V, reinterpret_cast<int2*>(xy), vring);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_simp_area(const int32_t* xy, const int32_t* vring, const long long* ring_start, long long V, long long R, long long* area2,
                              void* stream) {
    UNET_CHECK_ARG(xy && vring && ring_start && area2, "simp_area: null pointer");
    UNET_CHECK_ARG(count_ok(V) && count_ok(R) && R <= V, "simp_area: V and R <= V must be in 1..2^31 - 1 (got %lld, %lld)", V, R);
    UNET_CHECK_ARG(al8(xy) && al8(area2), "simp_area: xy and area2 must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    UNET_CHECK_HIP(hipMemsetAsync(area2, 0, (size_t)R * sizeof(long long), st));
    hipLaunchKernelGGL(simp_area_kernel, dim3(ew_grid(V, 256)), dim3(256), 0, st, reinterpret_cast<const int2*>(xy), vring, ring_start, V, R, area2);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
