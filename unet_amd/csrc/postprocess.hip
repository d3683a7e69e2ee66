// Post-processing of a merged uint8 class mask on the device (unet_amd/postprocess.py):
//   unet_cc_label         connected components of equal-class pixels (4- / 8-adjacency); label = smallest linear index of the component
//   unet_cc_label_keys    the same components of a 32-bit key image at 4-adjacency (the flat zones of unet_amd/instances.py)
//   unet_cc_sizes         pixel count of every component, stored at its root label
//   unet_sieve_round      one round of the small-region sieve: label, sizes, best neighbour per small component, simultaneous merges
//   unet_majority_filter  k x k majority vote (one Jacobi pass), window clipped to the raster
//   unet_postprocess_counters  the one host read per round: {merged, small not merged, give-up code, 0}
// Labelling is a union-find in three launches: (1) every 32 x 64 tile is labelled in LDS and written as parent[pixel] = the tile-local
// root's linear index, (2) the pixels on tile borders join the trees of neighbouring tiles with atomicMin on the parent array, (3) every
// pixel is flattened to its root.  A parent is always a SMALLER index of the same component, so every chain ends in the component's
// smallest index whatever the schedule was: the result is canonical.
// No workgroup waits for another one: inside launch (2) every access to the parent array is an agent-scope atomic, a stale parent only
// costs one more step (the value atomicMin returns is what counts), and every find / union loop gives up after H * W steps with a code in
// the counters' third word.
#include "common.h"

using namespace unet;

namespace {

constexpr int CC_TH = 32, CC_TW = 64, CC_TP = CC_TH * CC_TW;        // 2048 px: 8 KiB of labels + 2 KiB of classes in LDS, 8 blocks per CU
constexpr int GIVEUP_TILE = 1, GIVEUP_BORDER = 2, GIVEUP_FLATTEN = 4;

__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int agent_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of a in the tile's LDS forest.  Every move of a find / union makes one of the two cursors smaller and none ever grows, so a call
// makes fewer than a + b < 2 CC_TP moves (for the parent array: 2 H W; chains there are as long as the tiles they cross, far below H W)
__device__ __forceinline__ int tile_find(const int* L, int a, int& budget) {
    while (budget > 0) {
        const int p = lds_load(&L[a]);
        if (p == a) break;
        a = p;
        --budget;
    }
    return a;
}

__device__ __forceinline__ void tile_union(int* L, int a, int b, int& budget) {
    a = tile_find(L, a, budget);
    b = tile_find(L, b, budget);
    while (a != b && budget > 0) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(&L[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) break;                    // a was a root and hangs under b now
        a = tile_find(L, old, budget);          // a had the parent `old` (< a): old and b are what is left to join
        --budget;
    }
}

// K: uint8_t, the class mask, or uint32_t, the (class << 16 | height) keys whose components are the flat zones of unet_inst_distance
// (8 KiB of keys instead of 2 KiB of classes in LDS)
template <typename K>
__global__ __launch_bounds__(256) void cc_tile_kernel(const K* __restrict__ mask, int H, int W, int ntx, int conn8,
                                                     int* __restrict__ parent, int* __restrict__ counters) {
    __shared__ int L[CC_TP];
    __shared__ K cls[CC_TP];
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * CC_TH, x0 = tx * CC_TW;
    const int t = threadIdx.x;
    for (int i = t; i < CC_TP; i += 256) {
        const int ly = i / CC_TW, lx = i % CC_TW;
        const int gy = y0 + ly, gx = x0 + lx;
        L[i] = i;
        cls[i] = (gy < H && gx < W) ? mask[(long long)gy * W + gx] : 0;
    }
    __syncthreads();
    bool gave_up = false;
    int budget = 0;
    for (int i = t; i < CC_TP; i += 256) {
        const int ly = i / CC_TW, lx = i % CC_TW;
        if (y0 + ly >= H || x0 + lx >= W) continue;
        const K c = cls[i];
        budget = 8 * CC_TP;          // the at most four unions of one pixel
        if (lx > 0 && cls[i - 1] == c) tile_union(L, i, i - 1, budget);
        if (ly > 0) {
            if (cls[i - CC_TW] == c) tile_union(L, i, i - CC_TW, budget);
            if (conn8) {
                if (lx > 0 && cls[i - CC_TW - 1] == c) tile_union(L, i, i - CC_TW - 1, budget);
                if (lx < CC_TW - 1 && x0 + lx + 1 < W && cls[i - CC_TW + 1] == c) tile_union(L, i, i - CC_TW + 1, budget);
            }
        }
        gave_up |= budget <= 0;
    }
    __syncthreads();
    for (int i = t; i < CC_TP; i += 256) {
        const int ly = i / CC_TW, lx = i % CC_TW;
        if (y0 + ly >= H || x0 + lx >= W) continue;
        budget = CC_TP;
        const int r = tile_find(L, i, budget);
        gave_up |= budget <= 0;
        parent[(long long)(y0 + ly) * W + x0 + lx] = (int)((long long)(y0 + r / CC_TW) * W + x0 + r % CC_TW);
    }
    if (gave_up) atomicOr(&counters[2], GIVEUP_TILE);
}

__device__ __forceinline__ int global_find(const int* P, int a, long long& budget) {
    while (budget > 0) {
        const int p = agent_load(&P[a]);
        if (p == a) break;
        a = p;
        --budget;
    }
    return a;
}

__device__ __forceinline__ void global_union(int* P, int a, int b, long long& budget) {
    a = global_find(P, a, budget);
    b = global_find(P, b, budget);
    while (a != b && budget > 0) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(&P[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) break;
        a = global_find(P, old, budget);
        --budget;
    }
}

// one thread per pixel in the first column (rows: first row) of a tile that has a tile to its left (above it)
template <typename K>
__global__ __launch_bounds__(256) void cc_border_kernel(const K* __restrict__ mask, int H, int W, int ntx, int nty, int conn8,
                                                       int* __restrict__ parent, int* __restrict__ counters) {
    const long long n = (long long)H * W;
    const long long nv = (long long)(ntx - 1) * H, total = nv + (long long)(nty - 1) * W;
    bool gave_up = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long budget = n;
        int x, y;
        if (i < nv) {                 // vertical border: x is a multiple of CC_TW, the partners lie in column x - 1
            x = (int)(i / H + 1) * CC_TW;
            y = (int)(i % H);
            const long long g = (long long)y * W + x;
            const K c = mask[g];
            if (mask[g - 1] == c) global_union(parent, (int)g, (int)(g - 1), budget);
            if (conn8) {
                if (y > 0 && mask[g - W - 1] == c) global_union(parent, (int)g, (int)(g - W - 1), budget);
                if (y < H - 1 && mask[g + W - 1] == c) global_union(parent, (int)g, (int)(g + W - 1), budget);
            }
        } else {                      // horizontal border: y is a multiple of CC_TH, the partners lie in row y - 1
            const long long j = i - nv;
            y = (int)(j / W + 1) * CC_TH;
            x = (int)(j % W);
            const long long g = (long long)y * W + x;
            const K c = mask[g];
            if (mask[g - W] == c) global_union(parent, (int)g, (int)(g - W), budget);
            if (conn8) {
                if (x > 0 && mask[g - W - 1] == c) global_union(parent, (int)g, (int)(g - W - 1), budget);
                if (x < W - 1 && mask[g - W + 1] == c) global_union(parent, (int)g, (int)(g - W + 1), budget);
            }
        }
        gave_up |= budget <= 0;
    }
    if (gave_up) atomicOr(&counters[2], GIVEUP_BORDER);
}

// in place: a pixel that another thread has flattened already holds its root, one that it has not holds its old parent; both lie on the chain
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* __restrict__ parent, long long n, int* __restrict__ counters) {
    bool gave_up = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        int p = agent_load(&parent[i]);
        long long budget = n;
        while (budget > 0) {
            const int q = agent_load(&parent[p]);
            if (q == p) break;
            p = q;
            --budget;
        }
        gave_up |= budget <= 0;
        parent[i] = p;
    }
    if (gave_up) atomicOr(&counters[2], GIVEUP_FLATTEN);
}

// 4 consecutive pixels per thread.  A wave whose 256 pixels all carry one label adds nothing yet: it keeps (label, count) pending
// across its grid-stride steps and adds once when the label changes, so a component of millions of pixels costs a few thousand adds to its
// one address instead of one per thread.  Other waves add one run of equal neighbouring labels at a time.
__global__ __launch_bounds__(256) void cc_sizes_kernel(const int* __restrict__ labels, long long n, int* __restrict__ sizes) {
    const long long quads = (n + 3) / 4;
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (long long)gridDim.x * 4;
    int pend_label = -1, pend_count = 0;          // the same in every lane of the wave
    for (long long base = wave * 64; base < quads; base += nwaves * 64) {          // a wave-uniform trip count
        const long long q = base + lane, i0 = q * 4;
        int l[4] = {-1, -1, -1, -1};
        if (i0 + 4 <= n) {
            const int4 v = *reinterpret_cast<const int4*>(labels + i0);          // labels are 16-byte aligned (checked by the entry point)
            l[0] = v.x; l[1] = v.y; l[2] = v.z; l[3] = v.w;
        } else {
            for (int j = 0; j < 4; ++j) l[j] = i0 + j < n ? labels[i0 + j] : -1;
        }
        const int first = __shfl(l[0], 0);
        const bool same = l[0] == first && l[1] == first && l[2] == first && l[3] == first;
        if (first >= 0 && first < n && __all(same)) {
            if (first != pend_label) {
                if (pend_count > 0 && lane == 0) atomicAdd(&sizes[pend_label], pend_count);
                pend_label = first;
                pend_count = 0;
            }
            pend_count += 256;
            continue;
        }
        int run = 1;
        for (int j = 1; j <= 4; ++j) {
            if (j < 4 && l[j] == l[j - 1]) { ++run; continue; }
            if (l[j - 1] >= 0 && l[j - 1] < n) atomicAdd(&sizes[l[j - 1]], run);          // (labels of a caller: never outside sizes)
            run = 1;
        }
    }
    if (pend_count > 0 && lane == 0) atomicAdd(&sizes[pend_label], pend_count);
}

__device__ __forceinline__ unsigned long long pack_key(int size, int label) {
    return ((unsigned long long)(unsigned)size << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)label);
}

// best neighbour of every small component: the largest key (size, -label) over its edge-adjacent components of a class that is not frozen
__global__ __launch_bounds__(256) void sieve_best_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ labels,
                                                        const int* __restrict__ sizes, int H, int W, long long min_pixels, int frozen,
                                                        unsigned long long* __restrict__ keys) {
    const long long n = (long long)H * W;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const int c = mask[p];
        if (c == frozen) continue;
        const int l = labels[p];
        if ((long long)sizes[l] >= min_pixels) continue;
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        unsigned long long best = 0;
        const long long nb[4] = {p - 1, p + 1, p - W, p + W};
        const bool ok[4] = {x > 0, x < W - 1, y > 0, y < H - 1};
        for (int j = 0; j < 4; ++j) {
            if (!ok[j]) continue;
            const int lq = labels[nb[j]];
            if (lq == l || (int)mask[nb[j]] == frozen) continue;
            const unsigned long long k = pack_key(sizes[lq], lq);
            best = k > best ? k : best;
        }
        if (best != 0) atomicMax(&keys[l], best);
    }
}

// out = in with every merging small component recoloured; counters[0] += merging components, counters[1] += small ones that stay
__global__ __launch_bounds__(256) void sieve_apply_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const int* __restrict__ labels,
                                                         const int* __restrict__ sizes, const unsigned long long* __restrict__ keys, long long n,
                                                         long long min_pixels, int frozen, int* __restrict__ counters) {
    int merged = 0, left = 0;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const uint8_t c = in[p];
        uint8_t o = c;
        const int l = labels[p];
        const int s = sizes[l];
        if ((int)c != frozen && (long long)s < min_pixels) {
            const unsigned long long k = keys != nullptr ? keys[l] : 0;          // no keys: a counting pass (out == nullptr)
            const bool merge = k > pack_key(s, l);          // no neighbour: k = 0, smaller than every key of a component
            if (merge) o = in[0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull)];          // the best neighbour's label is one of its pixels
            if (p == l) { merged += merge; left += !merge; }
        }
        if (out != nullptr) out[p] = o;
    }
    for (int o = 32; o > 0; o >>= 1) {          // one add per wave
        merged += __shfl_down(merged, o);
        left += __shfl_down(left, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (merged) atomicAdd(&counters[0], merged);
        if (left) atomicAdd(&counters[1], left);
    }
}

// ---------------------------------------------------------------------------------------------------------------- majority filter
constexpr int MJ_TH = 32, MJ_TW = 128, MJ_HALO = 7;
constexpr int MJ_ROWS = MJ_TH + 2 * MJ_HALO, MJ_TS = 144 /* >= MJ_TW + 2 * MJ_HALO */, MJ_HS = MJ_TW + 16;
constexpr int MJ_NOVOTE = 0x100, MJ_OUTSIDE = 0x1FF;          // tile entries >= 0x100 do not vote: a frozen pixel keeps its class in the low byte

// Per class present in the tile: horizontal box counts of (pixel == class) into LDS, then their vertical sums per output pixel and a running
// best.  Classes are visited in ascending order and replace the best only with a HIGHER count, so the smallest id wins a tie, unless the
// centre's own class has the best count.
__global__ __launch_bounds__(256) void majority_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W, int ntx, int k,
                                                      int frozen, int vec) {
    __shared__ uint16_t tile[MJ_ROWS * MJ_TS];
    __shared__ __attribute__((aligned(16))) uint8_t hc[MJ_ROWS * MJ_HS];
    __shared__ unsigned present[8];
    const int t = threadIdx.x;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * MJ_TH, x0 = tx * MJ_TW;
    const int rad = k >> 1, off = MJ_HALO - rad;            // rows / columns [off, off + T + 2 rad) of the tile are in use
    const int rows = MJ_TH + 2 * rad, cols = MJ_TW + 2 * rad;
    if (t < 8) present[t] = 0;
    __syncthreads();
    auto put = [&](int r, int cx, int v) {
        if (v == frozen) v |= MJ_NOVOTE;
        else if (!(present[v >> 5] >> (v & 31) & 1u)) atomicOr(&present[v >> 5], 1u << (v & 31));
        tile[r * MJ_TS + cx] = (uint16_t)v;
    };
    const bool body16 = vec && x0 + MJ_TW <= W;              // the 128 centre columns of a row as 8 x 16 bytes
    if (body16) {
        for (int i = t; i < rows * 8; i += 256) {
            const int r = off + i / 8, part = i % 8;
            const int gy = y0 - MJ_HALO + r;
            const int cx = MJ_HALO + part * 16;
            if (gy < 0 || gy >= H) {
                for (int j = 0; j < 16; ++j) tile[r * MJ_TS + cx + j] = MJ_OUTSIDE;
                continue;
            }
            const uint4 v = *reinterpret_cast<const uint4*>(in + (long long)gy * W + x0 + part * 16);
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
            for (int j = 0; j < 16; ++j) put(r, cx + j, (int)(w[j >> 2] >> (8 * (j & 3)) & 0xFFu));
        }
    }
    const int side = body16 ? 2 * rad : cols;               // columns still to load bytewise: the two halos, or everything
    for (int i = t; i < rows * side; i += 256) {
        const int r = off + i / side;
        int cx = i % side;
        cx = body16 ? (cx < rad ? off + cx : MJ_HALO + MJ_TW + (cx - rad)) : off + cx;
        const int gy = y0 - MJ_HALO + r, gx = x0 - MJ_HALO + cx;
        if (gy < 0 || gy >= H || gx < 0 || gx >= W) tile[r * MJ_TS + cx] = MJ_OUTSIDE;
        else put(r, cx, in[(long long)gy * W + gx]);
    }
    __syncthreads();

    const int row = t >> 3, cg = t & 7;                      // this thread's 16 output pixels: row `row`, columns [16 cg, 16 cg + 16)
    int centre[16], best[16], cc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        centre[j] = tile[(MJ_HALO + row) * MJ_TS + MJ_HALO + cg * 16 + j];
        best[j] = 0;
        cc[j] = 0;
    }
    for (int w = 0; w < 8; ++w) {
        unsigned bits = present[w];
        while (bits) {
            const int b = __builtin_ctz(bits);
            bits &= bits - 1;
            const int c = w * 32 + b;
            for (int i = t; i < rows * MJ_TW; i += 256) {
                const int r = off + i / MJ_TW, x = i % MJ_TW;
                const uint16_t* src = &tile[r * MJ_TS + off + x];
                int cnt = 0;
                for (int dx = 0; dx < k; ++dx) cnt += src[dx] == c;
                hc[r * MJ_HS + x] = (uint8_t)cnt;
            }
            __syncthreads();
            unsigned acc[4] = {0, 0, 0, 0};                  // 16 byte lanes: at most 15 rows x 15 per byte, no carry
            for (int dy = 0; dy < k; ++dy) {
                const uint4 v = *reinterpret_cast<const uint4*>(&hc[(row + off + dy) * MJ_HS + cg * 16]);
                acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w;
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int cnt = (int)(acc[j >> 2] >> (8 * (j & 3)) & 0xFFu);
                if (cnt > (best[j] >> 8)) best[j] = cnt << 8 | c;
                if (c == centre[j]) cc[j] = cnt;
            }
            __syncthreads();
        }
    }
    const int gy = y0 + row, gx0 = x0 + cg * 16;
    if (gy >= H || gx0 >= W) return;
    uint8_t o[16];
#pragma unroll
    for (int j = 0; j < 16; ++j)
        o[j] = (uint8_t)((centre[j] >= MJ_NOVOTE || cc[j] == (best[j] >> 8)) ? (centre[j] & 0xFF) : (best[j] & 0xFF));
    uint8_t* dst = out + (long long)gy * W + gx0;
    if (vec && gx0 + 16 <= W) {
        uint4 v;
        unsigned* w = reinterpret_cast<unsigned*>(&v);
        for (int q = 0; q < 4; ++q) w[q] = o[4 * q] | o[4 * q + 1] << 8 | o[4 * q + 2] << 16 | (unsigned)o[4 * q + 3] << 24;
        *reinterpret_cast<uint4*>(dst) = v;
    } else {
        for (int j = 0; j < 16 && gx0 + j < W; ++j) dst[j] = o[j];
    }
}

bool shape_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W <= 2147483647ll; }

template <typename K>
int label_launches(const K* mask, int H, int W, int connectivity, int32_t* labels, int32_t* counters, hipStream_t st) {
    const int ntx = cdiv(W, CC_TW), nty = cdiv(H, CC_TH);
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(cc_tile_kernel<K>, dim3((unsigned)((long long)ntx * nty)), dim3(256), 0, st, mask, H, W, ntx, connectivity == 8, labels, counters);
    UNET_CHECK_LAUNCH();
    const long long border = (long long)(ntx - 1) * H + (long long)(nty - 1) * W;
    if (border > 0) {
        hipLaunchKernelGGL(cc_border_kernel<K>, dim3(ew_grid(border, 256)), dim3(256), 0, st, mask, H, W, ntx, nty, connectivity == 8, labels, counters);
        UNET_CHECK_LAUNCH();
        hipLaunchKernelGGL(cc_flatten_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, st, labels, n, counters);
        UNET_CHECK_LAUNCH();
    }
    return UNET_OK;
}

int sizes_launches(const int32_t* labels, long long n, int32_t* sizes, hipStream_t st) {
    UNET_CHECK_HIP(hipMemsetAsync(sizes, 0, (size_t)n * sizeof(int32_t), st));
    hipLaunchKernelGGL(cc_sizes_kernel, dim3(ew_grid((n + 3) / 4, 256)), dim3(256), 0, st, labels, n, sizes);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

}  // namespace

extern "C" void unet_cc_tile_shape(int* th, int* tw) {
    if (th) *th = CC_TH;
    if (tw) *tw = CC_TW;
}

extern "C" int unet_cc_label(const uint8_t* mask, int H, int W, int connectivity, int32_t* labels, int32_t* counters, void* stream) {
    UNET_CHECK_ARG(mask && labels && counters, "cc_label: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W), "cc_label: H, W must be positive with H * W <= 2^31 - 1 (got %d x %d)", H, W);
    UNET_CHECK_ARG(connectivity == 4 || connectivity == 8, "cc_label: connectivity must be 4 or 8 (got %d)", connectivity);
    UNET_CHECK_ARG(aligned16(labels), "cc_label: labels must be 16-byte aligned");
    UNET_CHECK_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(int32_t), (hipStream_t)stream));
    return label_launches(mask, H, W, connectivity, labels, counters, (hipStream_t)stream);
}

extern "C" int unet_cc_label_keys(const uint32_t* keys, int H, int W, int32_t* labels, int32_t* counters, void* stream) {
    UNET_CHECK_ARG(keys && labels && counters, "cc_label_keys: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W), "cc_label_keys: H, W must be positive with H * W <= 2^31 - 1 (got %d x %d)", H, W);
    UNET_CHECK_ARG(aligned16(labels) && (((uintptr_t)keys) & 3) == 0, "cc_label_keys: labels must be 16-byte aligned, keys 4-byte aligned");
    UNET_CHECK_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(int32_t), (hipStream_t)stream));
    return label_launches(keys, H, W, 4, labels, counters, (hipStream_t)stream);
}

extern "C" int unet_cc_sizes(const int32_t* labels, int H, int W, int32_t* sizes, void* stream) {
    UNET_CHECK_ARG(labels && sizes, "cc_sizes: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W), "cc_sizes: H, W must be positive with H * W <= 2^31 - 1 (got %d x %d)", H, W);
    UNET_CHECK_ARG(aligned16(labels), "cc_sizes: labels must be 16-byte aligned");
    return sizes_launches(labels, (long long)H * W, sizes, (hipStream_t)stream);
}

extern "C" int unet_sieve_round(const uint8_t* in, uint8_t* out, int H, int W, int connectivity, long long min_pixels, int frozen_class,
                                int32_t* labels, int32_t* sizes, unsigned long long* keys, int32_t* counters, void* stream) {
    UNET_CHECK_ARG(in && labels && sizes && counters && (keys || !out), "sieve_round: null pointer");
    UNET_CHECK_ARG(in != out, "sieve_round: the round reads `in` while it writes `out`: they must differ");
    UNET_CHECK_ARG(shape_ok(H, W), "sieve_round: H, W must be positive with H * W <= 2^31 - 1 (got %d x %d)", H, W);
    UNET_CHECK_ARG(connectivity == 4 || connectivity == 8, "sieve_round: connectivity must be 4 or 8 (got %d)", connectivity);
    UNET_CHECK_ARG(min_pixels >= 2, "sieve_round: min_pixels must be >= 2 (got %lld)", min_pixels);
    UNET_CHECK_ARG(frozen_class >= -1 && frozen_class <= 255, "sieve_round: frozen_class must be -1 (none) or 0..255 (got %d)", frozen_class);
    UNET_CHECK_ARG(aligned16(labels), "sieve_round: labels must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)H * W;
    UNET_CHECK_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(int32_t), st));
    int rc = label_launches(in, H, W, connectivity, labels, counters, st);
    if (rc != UNET_OK) return rc;
    rc = sizes_launches(labels, n, sizes, st);
    if (rc != UNET_OK) return rc;
    if (out != nullptr) {
        UNET_CHECK_HIP(hipMemsetAsync(keys, 0, (size_t)n * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(sieve_best_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, st, in, labels, sizes, H, W, min_pixels, frozen_class, keys);
        UNET_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(sieve_apply_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, st, in, out, labels, sizes, keys, n,
                       min_pixels, frozen_class, counters);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_majority_filter(const uint8_t* in, uint8_t* out, int H, int W, int k, int frozen_class, void* stream) {
    UNET_CHECK_ARG(in && out && in != out, "majority_filter: null pointer, or in == out (one Jacobi pass reads the input while it writes)");
    UNET_CHECK_ARG(shape_ok(H, W), "majority_filter: H, W must be positive with H * W <= 2^31 - 1 (got %d x %d)", H, W);
    UNET_CHECK_ARG(k >= 3 && k <= 2 * MJ_HALO + 1 && (k & 1), "majority_filter: k must be odd, 3..15 (got %d)", k);
    UNET_CHECK_ARG(frozen_class >= -1 && frozen_class <= 255, "majority_filter: frozen_class must be -1 (none) or 0..255 (got %d)", frozen_class);
    const int ntx = cdiv(W, MJ_TW), nty = cdiv(H, MJ_TH);
    const int vec = (W % 16 == 0) && aligned16(in) && aligned16(out);
    hipLaunchKernelGGL(majority_kernel, dim3((unsigned)((long long)ntx * nty)), dim3(256), 0, (hipStream_t)stream, in, out, H, W, ntx, k, frozen_class, vec);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_postprocess_counters(const int32_t* counters, int32_t* host4, void* stream) {
    UNET_CHECK_ARG(counters && host4, "postprocess_counters: null pointer");
    hipStream_t st = (hipStream_t)stream;
    UNET_CHECK_HIP(hipMemcpyAsync(host4, counters, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    UNET_CHECK_HIP(hipStreamSynchronize(st));
    if (host4[2] != 0) {
        set_error("connected components: a find / union loop gave up after H * W steps (code %d: 1 tile, 2 border merge, 4 flatten)", host4[2]);
        return UNET_E_HIP;
    }
    return UNET_OK;
}
