// Ring tracing of a labelled class mask on the device (unet_amd/vectorize.py): boundary edges of 4-connected components,
// their successors, the rings as cycles of the successor array, and the corners of every ring in walk order.
//   unet_vec_flags        side flags (bit s = boundary edge on side s; N=0 W=1 S=2 E=3) per pixel, none for excluded classes
//   unet_vec_scan         exclusive scan of popcount(byte & 15) over a byte array: compact edge index, ring index, vertex index
//   unet_vec_succ         succ[e] = first existing of left / straight / right, and whether e ends in a corner
//   unet_vec_min_rounds   pointer doubling: m[e] = smallest edge of the 2^k edges from e on; settles at the cycle minimum = the ring leader
//   unet_vec_swap         at saddle vertices whose two incoming edges lie in ONE ring: swap their successors (the ring splits in two)
//   unet_vec_rank_init / unet_vec_rank_rounds   list ranking of every cycle cut at its leader: steps to the leader and twice the area on the way
//   unet_vec_ring_info    per ring: label, edge count, signed area
//   unet_vec_place        pos[e] = ring base + rank; the corner marks in ring order
//   unet_vec_emit         xy[vertex index of pos[e]] = end vertex of every corner edge
//   unet_vec_read         the host reads of a call: a few int64 words and a stream sync
// The compact index of edge (p, s) is offs[p] + popcount(flags[p] & ((1 << s) - 1)): monotone in the dense id 4 p + s, so the smallest
// compact index of a cycle is its smallest dense id.  Every output position is computed (scan + rank), no atomic decides one; the doubling
// rounds are Jacobi steps between two buffer sets, so every round's result is a function of the previous round alone.
#include "common.h"

using namespace unet;

namespace {

constexpr int SCAN_T = 256, SCAN_PER = 16, SCAN_CHUNK = SCAN_T * SCAN_PER;          // 4096 bytes per block: 16 per thread, one 16-byte load

struct ExcludeSet { uint32_t w[8]; };

__device__ __forceinline__ bool in_range(long long p, long long n) { return p >= 0 && p < n; }

// ------------------------------------------------------------------------------------------------------------------ side flags

__global__ __launch_bounds__(256) void vec_flags_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ labels, int H, int W,
                                                        ExcludeSet ex, uint8_t* __restrict__ flags) {
    const long long n = (long long)H * W;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        const int c = mask[p];
        unsigned f = 0;
        if (!((ex.w[c >> 5] >> (c & 31)) & 1u)) {
            const int l = labels[p];
            f |= (y == 0 || labels[p - W] != l) ? 1u : 0u;
            f |= (x == 0 || labels[p - 1] != l) ? 2u : 0u;
            f |= (y == H - 1 || labels[p + W] != l) ? 4u : 0u;
            f |= (x == W - 1 || labels[p + 1] != l) ? 8u : 0u;
        }
        flags[p] = (uint8_t)f;
    }
}

// ------------------------------------------------------------------------------------------------------------------ scan

// sum of popcount(b & 15) over the thread's 16 bytes [i0, i0 + 16) clipped to n; v[j] = the bytes (0 past the end)
__device__ __forceinline__ int scan_load(const uint8_t* __restrict__ in, long long i0, long long n, bool vec, uint32_t v[4]) {
    if (vec && i0 + 16 <= n) {
        const uint4 q = *reinterpret_cast<const uint4*>(in + i0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        for (int j = 0; j < 4; ++j) {
            uint32_t w = 0;
            for (int b = 0; b < 4; ++b) {
                const long long i = i0 + j * 4 + b;
                if (i < n) w |= (uint32_t)in[i] << (8 * b);
            }
            v[j] = w;
        }
    }
    int s = 0;
    for (int j = 0; j < 4; ++j) {
        v[j] &= 0x0F0F0F0Fu;
        s += __popc(v[j]);
    }
    return s;
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

__global__ __launch_bounds__(SCAN_T) void scan_reduce_kernel(const uint8_t* __restrict__ in, long long n, int vec, long long* __restrict__ bsum) {
    __shared__ int part[SCAN_T / 64];
    const long long i0 = (long long)blockIdx.x * SCAN_CHUNK + (long long)threadIdx.x * SCAN_PER;
    uint32_t v[4];
    int s = i0 < n ? scan_load(in, i0, n, vec != 0, v) : 0;
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = (long long)part[0] + part[1] + part[2] + part[3];
}

// one block: bsum[0 .. nb) becomes its exclusive scan, bsum[nb] the total
__global__ __launch_bounds__(1024) void scan_blocks_kernel(long long* __restrict__ bsum, int nb) {
    __shared__ long long sh[1024];
    __shared__ long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nb; base += 1024) {
        const int i = base + threadIdx.x;
        const long long own = i < nb ? bsum[i] : 0;
        sh[threadIdx.x] = own;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const long long add = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        const long long c = carry;
        if (i < nb) bsum[i] = c + sh[threadIdx.x] - own;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}

__global__ __launch_bounds__(SCAN_T) void scan_apply_kernel(const uint8_t* __restrict__ in, long long n, int vec, int vec_out,
                                                            const long long* __restrict__ bsum, int* __restrict__ out) {
    __shared__ int sh[SCAN_T];
    const long long i0 = (long long)blockIdx.x * SCAN_CHUNK + (long long)threadIdx.x * SCAN_PER;
    uint32_t v[4] = {0, 0, 0, 0};
    const int own = i0 < n ? scan_load(in, i0, n, vec != 0, v) : 0;
    sh[threadIdx.x] = own;
    __syncthreads();
    for (int d = 1; d < SCAN_T; d <<= 1) {
        const int add = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    if (i0 >= n) return;
    // a total above 2^31 - 1 is refused by the caller before any offset is used; the low 32 bits are stored either way
    unsigned run = (unsigned)(unsigned long long)(bsum[blockIdx.x] + (long long)(sh[threadIdx.x] - own));
    int o[SCAN_PER];
    for (int j = 0; j < 4; ++j)
        for (int b = 0; b < 4; ++b) {
            o[j * 4 + b] = (int)run;
            run += __popc((v[j] >> (8 * b)) & 0xFu);
        }
    if (vec_out && i0 + 16 <= n) {
        int4* q = reinterpret_cast<int4*>(out + i0);
        q[0] = make_int4(o[0], o[1], o[2], o[3]);
        q[1] = make_int4(o[4], o[5], o[6], o[7]);
        q[2] = make_int4(o[8], o[9], o[10], o[11]);
        q[3] = make_int4(o[12], o[13], o[14], o[15]);
    } else {
        for (int j = 0; j < SCAN_PER; ++j)
            if (i0 + j < n) out[i0 + j] = o[j];
    }
}

// ------------------------------------------------------------------------------------------------------------------ edges

__device__ __forceinline__ int edge_index(const uint8_t* __restrict__ flags, const int* __restrict__ offs, long long p, int s) {
    return offs[p] + __popc((unsigned)flags[p] & ((1u << s) - 1u));
}

// the pixel after p along the walk of side s, and from there the pixel on the outer side
__device__ __forceinline__ long long ahead(long long p, int s, int W) { return s == 0 ? p - 1 : s == 1 ? p + W : s == 2 ? p + 1 : p - W; }
__device__ __forceinline__ long long outer(long long q, int s, int W) { return s == 0 ? q - W : s == 1 ? q - 1 : s == 2 ? q + W : q + 1; }

// An edge whose left turn is no boundary edge has the same label across that side, which is the pixel ahead: it exists.  If that pixel's
// side s is no boundary edge either, the pixel beyond it on the outer side exists, has the label, and its side s - 1 faces the pixel
// across p's own side s: a boundary edge.  So the flags alone decide, and every index read here lies inside the raster.
__global__ __launch_bounds__(256) void vec_succ_kernel(const uint8_t* __restrict__ flags, const int* __restrict__ offs, int H, int W,
                                                       int* __restrict__ succ, uint8_t* __restrict__ corner) {
    const long long n = (long long)H * W;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const unsigned f = flags[p];
        if (f == 0) continue;
        const int base = offs[p];
        int k = 0;
        for (int s = 0; s < 4; ++s) {
            if (!((f >> s) & 1u)) continue;
            const int e = base + k++;
            const int left = (s + 1) & 3;
            int nx;
            bool turn = true;
            if ((f >> left) & 1u) {
                nx = base + __popc(f & ((1u << left) - 1u));
            } else {
                const long long q = ahead(p, s, W);
                if ((flags[q] >> s) & 1u) {
                    nx = edge_index(flags, offs, q, s);
                    turn = false;
                } else {
                    nx = edge_index(flags, offs, outer(q, s, W), (s + 3) & 3);
                }
            }
            succ[e] = nx;
            corner[e] = turn ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(256) void vec_min_init_kernel(const int* __restrict__ succ, long long E, int* __restrict__ m, int* __restrict__ nxt) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        const int j = succ[e];
        m[e] = (int)e;
        nxt[e] = in_range(j, E) ? j : (int)e;          // (a successor is always an edge; an index outside the arrays is never followed)
    }
}

__global__ __launch_bounds__(256) void vec_min_round_kernel(const int* __restrict__ m, const int* __restrict__ nxt, long long E,
                                                            int* __restrict__ m2, int* __restrict__ nxt2, int* __restrict__ changed) {
    bool any = false;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        const int j = nxt[e], a = m[e], b = m[j];
        m2[e] = b < a ? b : a;
        nxt2[e] = nxt[j];
        any |= b < a;
    }
    if (__any(any) && (threadIdx.x & 63) == 0) *changed = 1;          // a plain store of one value: nothing is counted
}

// vertex (vx, vy), 1 <= vx < W, 1 <= vy < H, with the pixels A = NW, B = NE, C = SW, D = SE.  Every edge ends in one vertex, so no two
// threads write one succ entry, and `ring` (the first identification) is only read.
__global__ __launch_bounds__(256) void vec_swap_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ flags, const int* __restrict__ offs,
                                                       int H, int W, const int* __restrict__ ring, int* __restrict__ succ) {
    const long long nv = (long long)(H - 1) * (W - 1);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
        const int vy = (int)(i / (W - 1)) + 1, vx = (int)(i % (W - 1)) + 1;
        const long long pd = (long long)vy * W + vx, pc = pd - 1, pb = pd - W, pa = pb - 1;
        const int a = labels[pa], b = labels[pb], c = labels[pc], d = labels[pd];
        if (a == d && b != a && c != a && (flags[pa] & 4u)) {          // flags are 0 for an excluded class
            const int ea = edge_index(flags, offs, pa, 2), ed = edge_index(flags, offs, pd, 0);          // A's S and D's N end here
            if (ring[ea] == ring[ed]) {
                succ[ea] = edge_index(flags, offs, pd, 1);
                succ[ed] = edge_index(flags, offs, pa, 3);
            }
        }
        if (b == c && a != b && d != b && (flags[pb] & 2u)) {
            const int eb = edge_index(flags, offs, pb, 1), ec = edge_index(flags, offs, pc, 3);          // B's W and C's E end here
            if (ring[eb] == ring[ec]) {
                succ[eb] = edge_index(flags, offs, pc, 0);
                succ[ec] = edge_index(flags, offs, pb, 2);
            }
        }
    }
}

// twice the signed area that edge (x, y, s) adds: x1 y0 - x0 y1 of its two end points
__device__ __forceinline__ long long area2_of(int x, int y, int s) { return s == 0 ? -(long long)y : s == 1 ? -(long long)x : s == 2 ? y + 1 : x + 1; }

// the cycle is cut AT its leader: the leader is the end of the list (nxt = itself, nothing to add), every other edge points at its
// successor.  After the rounds steps[e] = edges from e up to (not including) the leader, area[e] = their area terms.
__global__ __launch_bounds__(256) void vec_rank_init_kernel(const uint8_t* __restrict__ flags, const int* __restrict__ offs, int H, int W,
                                                            const int* __restrict__ succ, const int* __restrict__ ring, int* __restrict__ steps,
                                                            int* __restrict__ nxt, long long* __restrict__ area, uint8_t* __restrict__ mark, long long E) {
    const long long n = (long long)H * W;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const unsigned f = flags[p];
        if (f == 0) continue;
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        int e = offs[p];
        for (int s = 0; s < 4; ++s) {
            if (!((f >> s) & 1u)) continue;
            const int j = succ[e];
            const bool lead = ring[e] == e || !in_range(j, E);
            steps[e] = lead ? 0 : 1;
            nxt[e] = lead ? e : j;
            area[e] = lead ? 0 : area2_of(x, y, s);
            mark[e] = lead ? 1 : 0;
            ++e;
        }
    }
}

__global__ __launch_bounds__(256) void vec_rank_round_kernel(const int* __restrict__ steps, const int* __restrict__ nxt, const long long* __restrict__ area,
                                                             long long E, int* __restrict__ steps2, int* __restrict__ nxt2,
                                                             long long* __restrict__ area2, int* __restrict__ changed) {
    bool any = false;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        const int j = nxt[e], jj = nxt[j];
        steps2[e] = steps[e] + steps[j];
        area2[e] = area[e] + area[j];
        nxt2[e] = jj;
        any |= jj != j;
    }
    if (__any(any) && (threadIdx.x & 63) == 0) *changed = 1;
}

__global__ __launch_bounds__(256) void vec_ring_info_kernel(const uint8_t* __restrict__ flags, const int* __restrict__ offs, const int* __restrict__ labels,
                                                            int H, int W, const int* __restrict__ succ, const int* __restrict__ ring,
                                                            const int* __restrict__ ridx, const int* __restrict__ steps, const long long* __restrict__ area,
                                                            long long R, int* __restrict__ ring_label, long long* __restrict__ ring_len,
                                                            long long* __restrict__ ring_area) {
    const long long n = (long long)H * W;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const unsigned f = flags[p];
        if (f == 0) continue;
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        int e = offs[p];
        for (int s = 0; s < 4; ++s) {
            if (!((f >> s) & 1u)) continue;
            if (ring[e] == e) {
                const long long r = ridx[e];
                if (in_range(r, R)) {
                    const int first = succ[e];
                    ring_label[r] = labels[p];
                    ring_len[r] = (long long)steps[first] + 1;
                    ring_area[r] = (area[first] + area2_of(x, y, s)) / 2;          // even by construction
                }
            }
            ++e;
        }
    }
}

__global__ __launch_bounds__(256) void vec_place_kernel(const int* __restrict__ ring, const int* __restrict__ steps, const int* __restrict__ ridx,
                                                        const long long* __restrict__ ring_base, const long long* __restrict__ ring_len,
                                                        const uint8_t* __restrict__ corner, long long E, long long R, int* __restrict__ pos,
                                                        uint8_t* __restrict__ corner_ord) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        const int lead = ring[e];
        const long long r = ridx[lead];
        if (!in_range(r, R)) continue;
        const long long at = ring_base[r] + (lead == e ? 0 : ring_len[r] - steps[e]);
        if (!in_range(at, E)) continue;
        pos[e] = (int)at;
        corner_ord[at] = corner[e];
    }
}

__global__ __launch_bounds__(256) void vec_emit_kernel(const uint8_t* __restrict__ flags, const int* __restrict__ offs, int H, int W,
                                                       const uint8_t* __restrict__ corner, const int* __restrict__ pos, const int* __restrict__ voff,
                                                       long long E, long long V, int* __restrict__ xy) {
    const long long n = (long long)H * W;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const unsigned f = flags[p];
        if (f == 0) continue;
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        int e = offs[p];
        for (int s = 0; s < 4; ++s) {
            if (!((f >> s) & 1u)) continue;
            if (corner[e] && in_range(pos[e], E)) {
                const long long v = voff[pos[e]];
                if (in_range(v, V))
                    *reinterpret_cast<int2*>(xy + 2 * v) = make_int2(x + (s >= 2 ? 1 : 0), y + (s == 1 || s == 2 ? 1 : 0));
            }
            ++e;
        }
    }
}

bool shape_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W <= 2147483647LL; }
bool count_ok(long long n) { return n > 0 && n <= 2147483647LL; }

}  // namespace

extern "C" int unet_vec_flags(const uint8_t* mask, const int32_t* labels, int H, int W, const uint32_t* exclude8, uint8_t* flags, void* stream) {
    UNET_CHECK_ARG(mask && labels && flags, "vec_flags: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W), "vec_flags: H, W must be positive with H * W <= 2^31 - 1 (got %d x %d)", H, W);
    ExcludeSet ex;
    for (int i = 0; i < 8; ++i) ex.w[i] = exclude8 ? exclude8[i] : 0u;
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(vec_flags_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, mask, labels, H, W, ex, flags);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" long long unet_vec_scan_words(long long n) { return n < 1 ? 0 : (n + SCAN_CHUNK - 1) / SCAN_CHUNK + 1; }

extern "C" int unet_vec_scan(const uint8_t* in, long long n, int32_t* out, long long* blocks, void* stream) {
    UNET_CHECK_ARG(in && out && blocks, "vec_scan: null pointer");
    UNET_CHECK_ARG(count_ok(n), "vec_scan: n must be in 1..2^31 - 1 (got %lld)", n);
    UNET_CHECK_ARG((((uintptr_t)out) & 3) == 0 && (((uintptr_t)blocks) & 7) == 0, "vec_scan: out / blocks must be aligned to their element");
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)((n + SCAN_CHUNK - 1) / SCAN_CHUNK);
    const int vec = aligned16(in), vec_out = aligned16(out);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(nb), dim3(SCAN_T), 0, st, in, n, vec, blocks);
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(1024), 0, st, blocks, nb);
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(SCAN_T), 0, st, in, n, vec, vec_out, blocks, out);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_vec_read(const long long* dev, int count, long long* host, void* stream) {
    UNET_CHECK_ARG(dev && host && count >= 1 && count <= 64, "vec_read: null pointer, or count outside 1..64");
    hipStream_t st = (hipStream_t)stream;
    UNET_CHECK_HIP(hipMemcpyAsync(host, dev, (size_t)count * sizeof(long long), hipMemcpyDeviceToHost, st));
    UNET_CHECK_HIP(hipStreamSynchronize(st));
    return UNET_OK;
}

extern "C" int unet_vec_succ(const uint8_t* flags, const int32_t* offs, int H, int W, long long E, int32_t* succ, uint8_t* corner, void* stream) {
    UNET_CHECK_ARG(flags && offs && succ && corner, "vec_succ: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W) && count_ok(E), "vec_succ: H * W and E must be in 1..2^31 - 1 (got %d x %d, %lld)", H, W, E);
    hipLaunchKernelGGL(vec_succ_kernel, dim3(ew_grid((long long)H * W, 256)), dim3(256), 0, (hipStream_t)stream, flags, offs, H, W, succ, corner);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_vec_min_rounds(const int32_t* succ, long long E, int32_t* m_a, int32_t* nxt_a, int32_t* m_b, int32_t* nxt_b, int init, int rounds,
                                   int32_t* changed, void* stream) {
    UNET_CHECK_ARG(succ && m_a && nxt_a && m_b && nxt_b && changed, "vec_min_rounds: null pointer");
    UNET_CHECK_ARG(count_ok(E) && rounds >= 0 && rounds <= 64, "vec_min_rounds: E must be in 1..2^31 - 1 and rounds in 0..64 (got %lld, %d)", E, rounds);
    UNET_CHECK_ARG(m_a != m_b && nxt_a != nxt_b && m_a != nxt_a && m_b != nxt_b && m_a != nxt_b && m_b != nxt_a, "vec_min_rounds: the four buffers must differ");
    hipStream_t st = (hipStream_t)stream;
    const int grid = ew_grid(E, 256);
    if (init) {
        hipLaunchKernelGGL(vec_min_init_kernel, dim3(grid), dim3(256), 0, st, succ, E, m_a, nxt_a);
        UNET_CHECK_LAUNCH();
    }
    if (rounds > 0) UNET_CHECK_HIP(hipMemsetAsync(changed, 0, (size_t)rounds * sizeof(int32_t), st));
    for (int r = 0; r < rounds; ++r) {          // round r reads set a (r even) or b (r odd) and writes the other
        if (r % 2 == 0) hipLaunchKernelGGL(vec_min_round_kernel, dim3(grid), dim3(256), 0, st, m_a, nxt_a, E, m_b, nxt_b, changed + r);
        else hipLaunchKernelGGL(vec_min_round_kernel, dim3(grid), dim3(256), 0, st, m_b, nxt_b, E, m_a, nxt_a, changed + r);
        UNET_CHECK_LAUNCH();
    }
    return UNET_OK;
}

extern "C" int unet_vec_swap(const int32_t* labels, const uint8_t* flags, const int32_t* offs, int H, int W, const int32_t* ring, int32_t* succ,
                             void* stream) {
    UNET_CHECK_ARG(labels && flags && offs && ring && succ, "vec_swap: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W), "vec_swap: H, W must be positive with H * W <= 2^31 - 1 (got %d x %d)", H, W);
    if (H < 2 || W < 2) return UNET_OK;          // no interior vertex
    hipLaunchKernelGGL(vec_swap_kernel, dim3(ew_grid((long long)(H - 1) * (W - 1), 256)), dim3(256), 0, (hipStream_t)stream, labels, flags, offs, H, W,
                       ring, succ);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_vec_rank_init(const uint8_t* flags, const int32_t* offs, int H, int W, const int32_t* succ, const int32_t* ring, int32_t* steps,
                                  int32_t* nxt, long long* area, uint8_t* mark, long long E, void* stream) {
    UNET_CHECK_ARG(flags && offs && succ && ring && steps && nxt && area && mark, "vec_rank_init: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W) && count_ok(E), "vec_rank_init: H * W and E must be in 1..2^31 - 1 (got %d x %d, %lld)", H, W, E);
    hipLaunchKernelGGL(vec_rank_init_kernel, dim3(ew_grid((long long)H * W, 256)), dim3(256), 0, (hipStream_t)stream, flags, offs, H, W, succ, ring,
                       steps, nxt, area, mark, E);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_vec_rank_rounds(long long E, int32_t* steps_a, int32_t* nxt_a, long long* area_a, int32_t* steps_b, int32_t* nxt_b, long long* area_b,
                                    int rounds, int32_t* changed, void* stream) {
    UNET_CHECK_ARG(steps_a && nxt_a && area_a && steps_b && nxt_b && area_b && changed, "vec_rank_rounds: null pointer");
    UNET_CHECK_ARG(count_ok(E) && rounds >= 0 && rounds <= 64, "vec_rank_rounds: E must be in 1..2^31 - 1 and rounds in 0..64 (got %lld, %d)", E, rounds);
    UNET_CHECK_ARG(steps_a != steps_b && nxt_a != nxt_b && area_a != area_b && steps_a != nxt_a && steps_b != nxt_b && steps_a != nxt_b && steps_b != nxt_a,
                   "vec_rank_rounds: the buffers must differ");
    hipStream_t st = (hipStream_t)stream;
    const int grid = ew_grid(E, 256);
    if (rounds > 0) UNET_CHECK_HIP(hipMemsetAsync(changed, 0, (size_t)rounds * sizeof(int32_t), st));
    for (int r = 0; r < rounds; ++r) {
        if (r % 2 == 0) hipLaunchKernelGGL(vec_rank_round_kernel, dim3(grid), dim3(256), 0, st, steps_a, nxt_a, area_a, E, steps_b, nxt_b, area_b, changed + r);
        else hipLaunchKernelGGL(vec_rank_round_kernel, dim3(grid), dim3(256), 0, st, steps_b, nxt_b, area_b, E, steps_a, nxt_a, area_a, changed + r);
        UNET_CHECK_LAUNCH();
    }
    return UNET_OK;
}

extern "C" int unet_vec_ring_info(const uint8_t* flags, const int32_t* offs, const int32_t* labels, int H, int W, const int32_t* succ, const int32_t* ring,
                                  const int32_t* ridx, const int32_t* steps, const long long* area, long long R, int32_t* ring_label, long long* ring_len,
                                  long long* ring_area, void* stream) {
    UNET_CHECK_ARG(flags && offs && labels && succ && ring && ridx && steps && area && ring_label && ring_len && ring_area, "vec_ring_info: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W) && count_ok(R), "vec_ring_info: H * W and R must be in 1..2^31 - 1 (got %d x %d, %lld)", H, W, R);
    hipLaunchKernelGGL(vec_ring_info_kernel, dim3(ew_grid((long long)H * W, 256)), dim3(256), 0, (hipStream_t)stream, flags, offs, labels, H, W, succ,
                       ring, ridx, steps, area, R, ring_label, ring_len, ring_area);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_vec_place(const int32_t* ring, const int32_t* steps, const int32_t* ridx, const long long* ring_base, const long long* ring_len,
                              const uint8_t* corner, long long E, long long R, int32_t* pos, uint8_t* corner_ord, void* stream) {
    UNET_CHECK_ARG(ring && steps && ridx && ring_base && ring_len && corner && pos && corner_ord, "vec_place: null pointer");
    UNET_CHECK_ARG(count_ok(E) && count_ok(R) && R <= E, "vec_place: E and R <= E must be in 1..2^31 - 1 (got %lld, %lld)", E, R);
    hipLaunchKernelGGL(vec_place_kernel, dim3(ew_grid(E, 256)), dim3(256), 0, (hipStream_t)stream, ring, steps, ridx, ring_base, ring_len, corner, E, R,
                       pos, corner_ord);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_vec_emit(const uint8_t* flags, const int32_t* offs, int H, int W, const uint8_t* corner, const int32_t* pos, const int32_t* voff,
                             long long E, long long V, int32_t* xy, void* stream) {
    UNET_CHECK_ARG(flags && offs && corner && pos && voff && xy, "vec_emit: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W) && count_ok(E) && count_ok(V), "vec_emit: H * W, E and V must be in 1..2^31 - 1 (got %d x %d, %lld, %lld)", H, W, E, V);
    UNET_CHECK_ARG((((uintptr_t)xy) & 7) == 0, "vec_emit: xy must be 8-byte aligned");
    hipLaunchKernelGGL(vec_emit_kernel, dim3(ew_grid((long long)H * W, 256)), dim3(256), 0, (hipStream_t)stream, flags, offs, H, W, corner, pos, voff, E, V, xy);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
