// Instance split of a merged uint8 class mask on the device (unet_amd/instances.py): touching objects of one class are
// separated along the ridges of a capped distance transform, shallow basins are merged back.
//   unet_inst_distance      keys[p] = class << 16 | h(p): the capped squared distance to the nearest pixel of another value (0 for a class
//                           that is not split), a row pass into a byte image and a column pass, both staged in LDS with a halo of R
//   unet_inst_check_labels  does a caller's label image name, per pixel, a root pixel of the same class at or before it?
//   unet_inst_ascent        per flat zone the highest 4-adjacent pixel of its class above it (64-bit atomic maximum of
//                           h(u) << 32 | ~index(u)); ptr = the zone of that pixel, or the zone itself: a seed
//   unet_inst_ptr_rounds    pointer doubling over the roots of a label image, Jacobi between two buffers, with the changed words of
//                           unet_vec_min_rounds
//   unet_inst_gather        out[p] = ptr[root[p]]
//   unet_inst_merge_round   one merge round on the segments: peak and best neighbour per segment (atomic maxima), the decision per
//                           segment, doubling rounds over the merge pointers (a fixed number of launches; those behind a round that
//                           moved nothing return at once), the gather
//   unet_inst_canonical     labels[p] = the smallest linear index of p's segment (atomic minimum, gather)
//   unet_inst_marks / unet_inst_ids   dense ids 1..N of the segments of the split classes in ascending label order, 0 elsewhere: root marks,
//                           unet_vec_scan of them, a gather
// The flat zones themselves are labelled by unet_cc_label_keys (postprocess.hip).  A zone / segment is named by the linear index of one
// of its pixels, its ROOT (root[p] == p there), so every per-zone and per-segment array is a pixel-sized array used at the roots only.
// Atomics take maxima and minima of integers: the order of arrival cannot show.  Counts (seeds, merges, segments) are block sums written
// to partial[blockIdx.x] (unet_inst_partials() words, zero where a block has nothing), added up by the caller.  No float arithmetic.
#include "common.h"

using namespace unet;

namespace {

constexpr int DR_TW = 256, DR_TH = 4;          // row pass: 4 rows x 256 columns per block; LDS 4 x (256 + 2 * 255) bytes = 3064 bytes
constexpr int DC_TW = 32, DC_TH = 64;          // column pass: 64 rows x 32 columns; LDS (64 + 2 R) x 32 x 2 bytes: 12 KiB at R = 64, 35.9 KiB at 255
constexpr int MAX_R = 255;
constexpr int PARTIALS = 2048;                 // = the largest ew_grid

struct ClassSet { uint32_t w[8]; };

__device__ __forceinline__ bool in_set(const ClassSet& s, int c) { return (s.w[c >> 5] >> (c & 31)) & 1u; }

// g[p] = the horizontal distance from p to the nearest pixel of another value in its row, R if there is none within R
__global__ __launch_bounds__(256) void inst_rows_kernel(const uint8_t* __restrict__ mask, int H, int W, int ntx, int R, uint8_t* __restrict__ g) {
    __shared__ uint8_t row[DR_TH][DR_TW + 2 * MAX_R];
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * DR_TH, x0 = tx * DR_TW;
    const int t = threadIdx.x, span = DR_TW + 2 * R;
    for (int r = 0; r < DR_TH; ++r) {
        const int gy = y0 + r;
        if (gy >= H) break;
        for (int i = t; i < span; i += 256) {
            const int gx = x0 - R + i;
            row[r][i] = (gx >= 0 && gx < W) ? mask[(long long)gy * W + gx] : 0;
        }
    }
    __syncthreads();
    const int x = x0 + t;
    if (x >= W) return;
    for (int r = 0; r < DR_TH; ++r) {
        const int gy = y0 + r;
        if (gy >= H) break;
        const uint8_t* c = &row[r][R + t];
        const uint8_t own = c[0];
        int d = 1;
        for (; d < R; ++d) {          // columns outside the raster hold no pixel
            if ((x - d >= 0 && c[-d] != own) || (x + d < W && c[d] != own)) break;
        }
        g[(long long)gy * W + x] = (uint8_t)d;
    }
}

// keys[p] = class << 16 | min(R^2, min over |dy| <= R of dy^2 + (another value in row y + dy ? 0 : g^2)) for the classes of `split`, class << 16
// for the others.  A direction ends at the first row of another value (the rows behind it are farther), and at the first dy with
// dy^2 >= the best so far.  The tile holds class << 8 | g per pixel; g >= 1 everywhere, so 0 marks a row outside the raster.
__global__ __launch_bounds__(256) void inst_cols_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ g, int H, int W, int ntx, int R,
                                                        ClassSet split, uint32_t* __restrict__ keys) {
    extern __shared__ uint16_t cg[];          // [DC_TH + 2 R][DC_TW]
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * DC_TH, x0 = tx * DC_TW;
    const int t = threadIdx.x, rows = DC_TH + 2 * R;
    for (int i = t; i < rows * DC_TW; i += 256) {
        const int r = i / DC_TW, lx = i % DC_TW;
        const long long gy = (long long)y0 - R + r;
        const int gx = x0 + lx;
        uint16_t v = 0;
        if (gy >= 0 && gy < H && gx < W) {
            const long long p = gy * W + gx;
            v = (uint16_t)((unsigned)mask[p] << 8 | g[p]);
        }
        cg[i] = v;
    }
    __syncthreads();
    const int lx = t % DC_TW, gx = x0 + lx;
    if (gx >= W) return;
    for (int ly = t / DC_TW; ly < DC_TH; ly += 256 / DC_TW) {
        const int gy = y0 + ly;
        if (gy >= H) break;
        const uint16_t* col = &cg[(ly + R) * DC_TW + lx];
        const unsigned own = col[0], c = own >> 8;
        unsigned h = 0;
        if (in_set(split, (int)c)) {
            h = (own & 255u) * (own & 255u);
            bool up = true, down = true;
            for (int dy = 1; dy <= R && (up || down) && (unsigned)(dy * dy) < h; ++dy) {
                const unsigned d2 = (unsigned)(dy * dy);
                if (up) {
                    const unsigned e = col[-dy * DC_TW];
                    if (e == 0) up = false;
                    else if ((e >> 8) != c) { h = min(h, d2); up = false; }
                    else h = min(h, d2 + (e & 255u) * (e & 255u));
                }
                if (down) {
                    const unsigned e = col[dy * DC_TW];
                    if (e == 0) down = false;
                    else if ((e >> 8) != c) { h = min(h, d2); down = false; }
                    else h = min(h, d2 + (e & 255u) * (e & 255u));
                }
            }
            h = min(h, (unsigned)(R * R));
        }
        keys[(long long)gy * W + gx] = c << 16 | h;
    }
}

__global__ __launch_bounds__(256) void inst_check_labels_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ labels, long long n,
                                                                long long* __restrict__ bad) {
    bool any = false;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const int l = labels[p];
        any |= l < 0 || l > p || labels[l] != l || mask[l] != mask[p];          // (|| does not evaluate what follows a true operand)
    }
    if (__any(any) && (threadIdx.x & 63) == 0) *bad = 1;          // a plain store of one value
}

__device__ __forceinline__ unsigned long long pack(unsigned hi, unsigned index) { return ((unsigned long long)hi << 32) | (unsigned long long)(~index); }
__device__ __forceinline__ int index_of(unsigned long long key) { return (int)(~(unsigned)(key & 0xFFFFFFFFull)); }

// a maximum: a stale read that is already at least the key makes the atomic unnecessary, one that is lower only costs the atomic
__device__ __forceinline__ void raise(unsigned long long* slot, unsigned long long key) {
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(slot, key);
}

__device__ __forceinline__ void block_count(int mine, long long* __restrict__ partial) {
    __shared__ int part[4];
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (long long)part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(256) void inst_zero_roots_kernel(const int* __restrict__ root, long long n, unsigned long long* __restrict__ best,
                                                              int* __restrict__ peak) {
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256)
        if (root[p] == p) {
            best[p] = 0;
            if (peak != nullptr) peak[p] = 0;
        }
}

// every pixel u offers itself to the zones of its lower 4-neighbours of the same class
__global__ __launch_bounds__(256) void inst_ascent_kernel(const uint32_t* __restrict__ keys, const int* __restrict__ zone, int H, int W,
                                                          unsigned long long* __restrict__ zkey) {
    const long long n = (long long)H * W;
    for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < n; u += (long long)gridDim.x * 256) {
        const unsigned ku = keys[u], hu = ku & 0xFFFFu;
        if (hu == 0) continue;
        const int y = (int)(u / W), x = (int)(u - (long long)y * W);
        const long long nb[4] = {u - 1, u + 1, u - W, u + W};
        const bool ok[4] = {x > 0, x < W - 1, y > 0, y < H - 1};
        const unsigned long long key = pack(hu, (unsigned)u);
        for (int j = 0; j < 4; ++j) {
            if (!ok[j]) continue;
            const unsigned kv = keys[nb[j]];
            if ((kv >> 16) == (ku >> 16) && (kv & 0xFFFFu) < hu) raise(&zkey[zone[nb[j]]], key);
        }
    }
}

__global__ __launch_bounds__(256) void inst_ascent_ptr_kernel(const int* __restrict__ zone, const unsigned long long* __restrict__ zkey, long long n,
                                                              int* __restrict__ ptr, long long* __restrict__ partial) {
    int seeds = 0;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        if (zone[p] != p) continue;
        const unsigned long long k = zkey[p];
        ptr[p] = k ? zone[index_of(k)] : (int)p;
        seeds += k == 0;
    }
    block_count(seeds, partial);
}

// the pointer of a root is a root, so only entries at roots are ever read or written.  prev: the changed word of the round before, written
// by an earlier launch; 0 there means that round moved nothing, so a and b agree at every root already and this round has nothing to do
// (its own word stays 0, which ends the rounds behind it the same way)
__global__ __launch_bounds__(256) void inst_ptr_round_kernel(const int* __restrict__ root, const int* __restrict__ a, long long n, int* __restrict__ b,
                                                             const int* prev, int* changed) {
    if (prev != nullptr && *prev == 0) return;
    bool any = false;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        if (root[p] != p) continue;
        const int j = a[p], jj = a[j];
        b[p] = jj;
        any |= jj != j;
    }
    if (__any(any) && (threadIdx.x & 63) == 0) *changed = 1;
}

// out may be root itself: every thread reads and writes its own pixel only
__global__ __launch_bounds__(256) void inst_gather_kernel(const int* root, const int* __restrict__ ptr, long long n, int* out) {
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) out[p] = ptr[root[p]];
}

// peak[A] = the largest h in A; best[A] = the largest (pass << 32 | ~id(B)) over the 4-adjacent pairs of equal class between A and another
// segment B, pass = the smaller of the two heights.  Every pair is seen once, from its left / upper pixel, and offered to both sides.
__global__ __launch_bounds__(256) void inst_peak_best_kernel(const uint32_t* __restrict__ keys, const int* __restrict__ seg, int H, int W,
                                                             int* __restrict__ peak, unsigned long long* __restrict__ best) {
    const long long n = (long long)H * W;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const unsigned kp = keys[p], hp = kp & 0xFFFFu;
        if (hp == 0) continue;          // a class that is not split: its segments are its components, they have no neighbour of their class
        const int a = seg[p];
        if (__hip_atomic_load(&peak[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (int)hp) atomicMax(&peak[a], (int)hp);
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        const long long nb[2] = {p + 1, p + W};
        const bool ok[2] = {x < W - 1, y < H - 1};
        for (int j = 0; j < 2; ++j) {
            if (!ok[j]) continue;
            const unsigned kr = keys[nb[j]];
            if ((kr >> 16) != (kp >> 16)) continue;
            const int b = seg[nb[j]];
            if (b == a) continue;
            const unsigned pass = min(hp, kr & 0xFFFFu);
            raise(&best[a], pack(pass, (unsigned)b));
            raise(&best[b], pack(pass, (unsigned)a));
        }
    }
}

// sqrt(peak) - sqrt(pass) < q / 16, exactly: with L = 256 (peak - pass) - q^2, L < 0 or L^2 < 1024 q^2 pass
__device__ __forceinline__ bool shallow(long long peak, long long pass, long long q) {
    const long long L = 256 * (peak - pass) - q * q;
    return L < 0 || L * L < 1024 * q * q * pass;
}

__global__ __launch_bounds__(256) void inst_decide_kernel(const int* __restrict__ seg, const int* __restrict__ peak, const unsigned long long* __restrict__ best,
                                                          long long n, int q, int* __restrict__ ptr, long long* __restrict__ partial) {
    int merged = 0;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        if (seg[p] != p) continue;
        const unsigned long long k = best[p];
        int to = (int)p;
        if (k != 0) {
            const int b = index_of(k);
            const int pa = peak[p], pb = peak[b];
            if (shallow(pa, (long long)(k >> 32), q) && (pa < pb || (pa == pb && p > b))) to = b;
        }
        ptr[p] = to;
        merged += to != p;
    }
    block_count(merged, partial);
}

__global__ __launch_bounds__(256) void inst_min_init_kernel(const int* __restrict__ seg, long long n, int* __restrict__ lowest) {
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256)
        if (seg[p] == p) lowest[p] = 0x7FFFFFFF;
}

__global__ __launch_bounds__(256) void inst_min_kernel(const int* __restrict__ seg, long long n, int* __restrict__ lowest) {
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        int* slot = &lowest[seg[p]];
        if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (int)p) atomicMin(slot, (int)p);
    }
}

__global__ __launch_bounds__(256) void inst_label_kernel(const int* __restrict__ seg, const int* __restrict__ lowest, long long n, int* __restrict__ labels,
                                                         long long* __restrict__ partial) {
    int segments = 0;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const int l = lowest[seg[p]];
        labels[p] = l;
        segments += l == p;
    }
    block_count(segments, partial);
}

// mark[p] = 1 at the root pixel of every segment of a class in `split` (vec_scan of the marks numbers them in ascending label order)
__global__ __launch_bounds__(256) void inst_marks_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ labels, long long n, ClassSet split,
                                                         uint8_t* __restrict__ mark) {
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256)
        mark[p] = (labels[p] == p && in_set(split, mask[p])) ? 1 : 0;
}

__global__ __launch_bounds__(256) void inst_ids_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ labels, const int* __restrict__ offs,
                                                       long long n, ClassSet split, uint32_t* __restrict__ ids) {
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const int l = labels[p];
        ids[p] = (in_set(split, mask[p]) && l >= 0 && l < n) ? (uint32_t)offs[l] + 1u : 0u;
    }
}

bool shape_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W <= 2147483647LL; }

}  // namespace

extern "C" void unet_inst_tile_shapes(int* row_th, int* row_tw, int* col_th, int* col_tw) {
    if (row_th) *row_th = DR_TH;
    if (row_tw) *row_tw = DR_TW;
    if (col_th) *col_th = DC_TH;
    if (col_tw) *col_tw = DC_TW;
}

extern "C" int unet_inst_partials(void) { return PARTIALS; }

extern "C" int unet_inst_distance(const uint8_t* mask, int H, int W, const uint32_t* split8, int radius, uint8_t* g, uint32_t* keys, void* stream) {
    UNET_CHECK_ARG(mask && split8 && g && keys, "inst_distance: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W), "inst_distance: H, W must be positive with H * W <= 2^31 - 1 (got %d x %d)", H, W);
    UNET_CHECK_ARG(radius >= 1 && radius <= MAX_R, "inst_distance: radius must be in 1..255 (got %d)", radius);
    UNET_CHECK_ARG((((uintptr_t)keys) & 3) == 0, "inst_distance: keys must be 4-byte aligned");
    ClassSet split;
    for (int i = 0; i < 8; ++i) split.w[i] = split8[i];
    hipStream_t st = (hipStream_t)stream;
    int ntx = cdiv(W, DR_TW);
    hipLaunchKernelGGL(inst_rows_kernel, dim3((unsigned)((long long)ntx * cdiv(H, DR_TH))), dim3(256), 0, st, mask, H, W, ntx, radius, g);
    UNET_CHECK_LAUNCH();
    ntx = cdiv(W, DC_TW);
    const size_t lds = (size_t)(DC_TH + 2 * radius) * DC_TW * sizeof(uint16_t);
    hipLaunchKernelGGL(inst_cols_kernel, dim3((unsigned)((long long)ntx * cdiv(H, DC_TH))), dim3(256), lds, st, mask, g, H, W, ntx, radius, split, keys);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_inst_check_labels(const uint8_t* mask, const int32_t* labels, int H, int W, long long* bad, void* stream) {
    UNET_CHECK_ARG(mask && labels && bad, "inst_check_labels: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W), "inst_check_labels: H, W must be positive with H * W <= 2^31 - 1 (got %d x %d)", H, W);
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)H * W;
    UNET_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(long long), st));
    hipLaunchKernelGGL(inst_check_labels_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, st, mask, labels, n, bad);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_inst_ascent(const uint32_t* keys, const int32_t* zone, int H, int W, unsigned long long* zkey, int32_t* ptr, long long* partial,
                                void* stream) {
    UNET_CHECK_ARG(keys && zone && zkey && ptr && partial, "inst_ascent: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W), "inst_ascent: H, W must be positive with H * W <= 2^31 - 1 (got %d x %d)", H, W);
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)H * W;
    const int grid = ew_grid(n, 256);
    UNET_CHECK_HIP(hipMemsetAsync(partial, 0, PARTIALS * sizeof(long long), st));
    hipLaunchKernelGGL(inst_zero_roots_kernel, dim3(grid), dim3(256), 0, st, zone, n, zkey, (int*)nullptr);
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(inst_ascent_kernel, dim3(grid), dim3(256), 0, st, keys, zone, H, W, zkey);
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(inst_ascent_ptr_kernel, dim3(grid), dim3(256), 0, st, zone, zkey, n, ptr, partial);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_inst_ptr_rounds(const int32_t* root, long long n, int32_t* ptr_a, int32_t* ptr_b, int rounds, int32_t* changed, void* stream) {
    UNET_CHECK_ARG(root && ptr_a && ptr_b && changed, "inst_ptr_rounds: null pointer");
    UNET_CHECK_ARG(n > 0 && n <= 2147483647LL && rounds >= 0 && rounds <= 64, "inst_ptr_rounds: n must be in 1..2^31 - 1 and rounds in 0..64 (got %lld, %d)",
                   n, rounds);
    UNET_CHECK_ARG(ptr_a != ptr_b && root != ptr_a && root != ptr_b, "inst_ptr_rounds: the buffers must differ");
    hipStream_t st = (hipStream_t)stream;
    const int grid = ew_grid(n, 256);
    if (rounds > 0) UNET_CHECK_HIP(hipMemsetAsync(changed, 0, (size_t)rounds * sizeof(int32_t), st));
    for (int r = 0; r < rounds; ++r) {          // round r reads a (r even) or b (r odd) and writes the other
        hipLaunchKernelGGL(inst_ptr_round_kernel, dim3(grid), dim3(256), 0, st, root, r % 2 == 0 ? ptr_a : ptr_b, n, r % 2 == 0 ? ptr_b : ptr_a,
                           r > 0 ? changed + r - 1 : (const int*)nullptr, changed + r);
        UNET_CHECK_LAUNCH();
    }
    return UNET_OK;
}

extern "C" int unet_inst_gather(const int32_t* root, const int32_t* ptr, long long n, int32_t* out, void* stream) {
    UNET_CHECK_ARG(root && ptr && out, "inst_gather: null pointer");
    UNET_CHECK_ARG(n > 0 && n <= 2147483647LL, "inst_gather: n must be in 1..2^31 - 1 (got %lld)", n);
    UNET_CHECK_ARG(ptr != out && ptr != root, "inst_gather: ptr must differ from root and out");
    hipLaunchKernelGGL(inst_gather_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, root, ptr, n, out);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_inst_merge_round(const uint32_t* keys, int32_t* seg, int H, int W, int q, int doublings, int32_t* peak, unsigned long long* best,
                                     int32_t* ptr_a, int32_t* ptr_b, int32_t* changed, long long* partial, void* stream) {
    UNET_CHECK_ARG(keys && seg && peak && best && ptr_a && ptr_b && changed && partial, "inst_merge_round: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W), "inst_merge_round: H, W must be positive with H * W <= 2^31 - 1 (got %d x %d)", H, W);
    UNET_CHECK_ARG(q >= 0 && q <= 16 * 255 && doublings >= 1 && doublings <= 32, "inst_merge_round: q must be in 0..4080, doublings in 1..32 (got %d, %d)",
                   q, doublings);
    UNET_CHECK_ARG(ptr_a != ptr_b && seg != ptr_a && seg != ptr_b && peak != ptr_a && peak != ptr_b && peak != seg, "inst_merge_round: the buffers must differ");
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)H * W;
    const int grid = ew_grid(n, 256);
    UNET_CHECK_HIP(hipMemsetAsync(partial, 0, PARTIALS * sizeof(long long), st));
    UNET_CHECK_HIP(hipMemsetAsync(changed, 0, (size_t)doublings * sizeof(int32_t), st));
    hipLaunchKernelGGL(inst_zero_roots_kernel, dim3(grid), dim3(256), 0, st, seg, n, best, peak);
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(inst_peak_best_kernel, dim3(grid), dim3(256), 0, st, keys, seg, H, W, peak, best);
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(inst_decide_kernel, dim3(grid), dim3(256), 0, st, seg, peak, best, n, q, ptr_a, partial);
    UNET_CHECK_LAUNCH();
    for (int r = 0; r < doublings; ++r) {
        hipLaunchKernelGGL(inst_ptr_round_kernel, dim3(grid), dim3(256), 0, st, seg, r % 2 == 0 ? ptr_a : ptr_b, n, r % 2 == 0 ? ptr_b : ptr_a,
                           r > 0 ? changed + r - 1 : (const int*)nullptr, changed + r);
        UNET_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(inst_gather_kernel, dim3(grid), dim3(256), 0, st, seg, doublings % 2 == 0 ? ptr_a : ptr_b, n, seg);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_inst_canonical(const int32_t* seg, long long n, int32_t* lowest, int32_t* labels, long long* partial, void* stream) {
    UNET_CHECK_ARG(seg && lowest && labels && partial, "inst_canonical: null pointer");
    UNET_CHECK_ARG(n > 0 && n <= 2147483647LL, "inst_canonical: n must be in 1..2^31 - 1 (got %lld)", n);
    UNET_CHECK_ARG(seg != lowest && seg != labels && lowest != labels, "inst_canonical: the buffers must differ");
    hipStream_t st = (hipStream_t)stream;
    const int grid = ew_grid(n, 256);
    UNET_CHECK_HIP(hipMemsetAsync(partial, 0, PARTIALS * sizeof(long long), st));
    hipLaunchKernelGGL(inst_min_init_kernel, dim3(grid), dim3(256), 0, st, seg, n, lowest);
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(inst_min_kernel, dim3(grid), dim3(256), 0, st, seg, n, lowest);
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(inst_label_kernel, dim3(grid), dim3(256), 0, st, seg, lowest, n, labels, partial);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_inst_marks(const uint8_t* mask, const int32_t* labels, long long n, const uint32_t* split8, uint8_t* mark, void* stream) {
    UNET_CHECK_ARG(mask && labels && split8 && mark, "inst_marks: null pointer");
    UNET_CHECK_ARG(n > 0 && n <= 2147483647LL, "inst_marks: n must be in 1..2^31 - 1 (got %lld)", n);
    ClassSet split;
    for (int i = 0; i < 8; ++i) split.w[i] = split8[i];
    hipLaunchKernelGGL(inst_marks_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, mask, labels, n, split, mark);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_inst_ids(const uint8_t* mask, const int32_t* labels, const int32_t* offs, long long n, const uint32_t* split8, uint32_t* ids,
                             void* stream) {
    UNET_CHECK_ARG(mask && labels && offs && split8 && ids, "inst_ids: null pointer");
    UNET_CHECK_ARG(n > 0 && n <= 2147483647LL, "inst_ids: n must be in 1..2^31 - 1 (got %lld)", n);
    ClassSet split;
    for (int i = 0; i < 8; ++i) split.w[i] = split8[i];
    hipLaunchKernelGGL(inst_ids_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, mask, labels, offs, n, split, ids);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
