// Border distance of a batch of class masks on the device (unet_amd/border.py):
//   unet_border_edt     int32 [B, H, W]: squared Euclidean distance to the nearest border pixel of the same image, INT32_MAX where the
//                       image has no border; masks are uint8 or int64
//   unet_border_weight  float [P]: class_w[y] + w0 * exp(-D^2 / (2 sigma^2)), the weight map of the U-Net paper
// The transform is the separable exact one, in two launches with a uint16 intermediate g [B, H, W]:
//   column pass  g(x, y) = vertical distance to the nearest border pixel of column x (EDT_INF = 16384 if the column has none).  The edge
//                test is fused.  A block owns 64 columns (lanes along x: coalesced rows) and cuts them into 16 row segments; every thread
//                sweeps its segment down, the segments exchange their last / first border row through LDS, and a sweep up finishes g.
//   row pass     D^2(x, y) = min over x' of (x - x')^2 + g(x', y)^2.  One wavefront per row, g of the row in LDS.  The argmin is monotone
//                in x (for a < b, cost(x, a) - cost(x, b) grows with x), so the row is solved by halving: the position in the middle of
//                two solved ones searches only between their argmins.  The positions of a level are dealt to groups of 16 lanes that
//                scan the range together; the range is also clipped to |x - x'| <= g(x, y), beyond which no x' can beat x' = x.  The
//                work of a row is at most (W + positions of the level) reads per level whatever the mask holds.
// Integer arithmetic throughout, no atomics, every pixel is written by exactly one thread: the result does not depend on the schedule.
#include <limits.h>

#include "common.h"

using namespace unet;

namespace {

constexpr int EDT_MAX = 8192;            // 2 * 8191^2 < 2^31
constexpr int EDT_INF = 16384;           // "no border in this column": EDT_INF^2 + 8191^2 < 2^31, and it fits the uint16 intermediate
constexpr int COL_SEGS = 16, COL_W = 64;
constexpr int ROW_GROUP = 16, ROW_GROUPS = 64 / ROW_GROUP;

template <typename M>
__device__ __forceinline__ bool is_edge(const M* __restrict__ img, int H, int W, int x, int y, long long excl) {
    const long long v = (long long)img[(size_t)y * W + x];
    if (v == excl) return false;
    bool e = false;
    if (x > 0) { const long long u = (long long)img[(size_t)y * W + x - 1]; e |= (u != v && u != excl); }
    if (x + 1 < W) { const long long u = (long long)img[(size_t)y * W + x + 1]; e |= (u != v && u != excl); }
    if (y > 0) { const long long u = (long long)img[(size_t)(y - 1) * W + x]; e |= (u != v && u != excl); }
    if (y + 1 < H) { const long long u = (long long)img[(size_t)(y + 1) * W + x]; e |= (u != v && u != excl); }
    return e;
}

template <typename M>
__global__ __launch_bounds__(COL_W * COL_SEGS) void edt_column_kernel(const M* __restrict__ mask, int H, int W, long long excl,
                                                                      uint16_t* __restrict__ g) {
    __shared__ int s_last[COL_SEGS][COL_W], s_first[COL_SEGS][COL_W];
    const int lx = threadIdx.x, s = threadIdx.y;
    const int x = blockIdx.x * COL_W + lx;
    const bool active = x < W;
    const size_t off = (size_t)blockIdx.y * H * W;
    const M* img = mask + off;
    uint16_t* gi = g + off;
    const int R = (H + COL_SEGS - 1) / COL_SEGS;
    const int y0 = min(s * R, H), y1 = min(y0 + R, H);
    int last = -1, first = -1;
    if (active) {
        for (int y = y0; y < y1; ++y) {          // down: distance to the last border row of this segment
            if (is_edge(img, H, W, x, y, excl)) {
                last = y;
                if (first < 0) first = y;
            }
            gi[(size_t)y * W + x] = (uint16_t)(last >= 0 ? y - last : EDT_INF);
        }
    }
    s_last[s][lx] = last;
    s_first[s][lx] = first;
    __syncthreads();
    if (!active) return;
    int above = -1, below = -1;
    for (int t = 0; t < s; ++t) above = max(above, s_last[t][lx]);
    for (int t = COL_SEGS - 1; t > s; --t) {
        const int f = s_first[t][lx];
        if (f >= 0) below = f;
    }
    for (int y = y1 - 1; y >= y0; --y) {         // up: the nearer of the border row above and the one below
        const int v = gi[(size_t)y * W + x];
        if (v == 0) below = y;
        const int down = v != EDT_INF ? v : (above >= 0 ? y - above : EDT_INF);
        const int up = below >= 0 ? below - y : EDT_INF;
        gi[(size_t)y * W + x] = (uint16_t)min(down, up);
    }
}

// dynamic LDS: per wavefront g of its row (uint16 [W]) and the argmin of every solved position (uint16 [W])
__global__ __launch_bounds__(256) void edt_row_kernel(const uint16_t* __restrict__ g, long long rows, int W, int levels,
                                                      int32_t* __restrict__ d2) {
    extern __shared__ uint16_t lds[];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + wv;
    const bool live = row < rows;
    uint16_t* G = lds + (size_t)wv * 2 * W;
    uint16_t* A = G + W;
    if (live)
        for (int x = lane; x < W; x += 64) G[x] = g[(size_t)row * W + x];
    __syncthreads();
    const int grp = lane / ROW_GROUP, gl = lane % ROW_GROUP;
    const int W2 = 1 << levels;                  // the power of two above W: positions p = x + 1 in 1..W, all below W2
    for (int l = 0; l < levels; ++l) {
        const int step = W2 >> (l + 1), n = 1 << l;
        for (int k0 = 0; k0 < n && (2 * k0 + 1) * step <= W; k0 += ROW_GROUPS) {
            const int k = k0 + grp, p = (2 * k + 1) * step;
            const bool valid = live && k < n && p <= W;
            unsigned long long key = ~0ull;
            const int x = p - 1;
            if (valid) {
                // the solved neighbours p - step and p + step bound the argmin; none beyond the row's ends
                int lo = p - step >= 1 ? (int)A[p - step - 1] : 0;
                int hi = p + step <= W ? (int)A[p + step - 1] : W - 1;
                const int gx = G[x];
                lo = max(lo, x - gx);
                hi = min(hi, x + gx);
                for (int xp = lo + gl; xp <= hi; xp += ROW_GROUP) {
                    const int gg = G[xp], d = x - xp;
                    const unsigned long long c = (unsigned long long)(unsigned)(d * d + gg * gg);
                    key = min(key, (c << 13) | (unsigned long long)xp);
                }
            }
            for (int o = ROW_GROUP / 2; o > 0; o >>= 1) {
                const unsigned long long other = __shfl_xor(key, o, ROW_GROUP);
                key = min(key, other);
            }
            // (the range always holds an argmin, so a key was found; x itself keeps every later index inside the row regardless)
            if (valid && gl == 0) A[x] = (uint16_t)(key != ~0ull ? (int)(key & 8191ull) : x);
        }
        __syncthreads();
    }
    if (!live) return;
    for (int x = lane; x < W; x += 64) {
        const int a = A[x], gg = G[a], d = x - a;
        d2[(size_t)row * W + x] = gg >= EDT_INF ? INT32_MAX : d * d + gg * gg;
    }
}

__global__ __launch_bounds__(256) void border_weight_kernel(const int32_t* __restrict__ d2, const int64_t* __restrict__ target,
                                                            const float* __restrict__ class_w, int C, float w0, double inv2s2,
                                                            long long P, float* __restrict__ pw) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
        const long long y = target[p];
        float w = 0.f;
        if (y >= 0 && y < C) {
            w = class_w ? class_w[y] : 1.f;
            const int32_t d = d2[p];
            // the exponent is rounded once (from fp64): its error stays below the fp32 spacing at the exponent's size
            if (d != INT32_MAX) w += w0 * expf((float)(-(double)d * inv2s2));
        }
        pw[p] = w;
    }
}

int row_levels(int W) {
    int l = 0;
    while ((1 << l) <= W) ++l;
    return l;
}

}  // namespace

extern "C" size_t unet_edt_workspace(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || H > EDT_MAX || W > EDT_MAX) return 0;
    return (size_t)B * H * W * sizeof(uint16_t);
}

extern "C" int unet_border_edt(const void* mask, int mask_is_int64, int B, int H, int W, int exclude, int32_t* d2, void* workspace,
                               void* stream) {
    UNET_CHECK_ARG(mask && d2 && workspace, "border_edt: null pointer");
    UNET_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && H <= EDT_MAX && W <= EDT_MAX, "border_edt: needs B >= 1 and 1 <= H, W <= 8192 (got %d x %d x %d)", B, H, W);
    UNET_CHECK_ARG(B <= 65535, "border_edt: at most 65535 images per call (got %d)", B);
    UNET_CHECK_ARG(exclude >= -1, "border_edt: exclude must be -1 (none) or a class id (got %d)", exclude);
    UNET_CHECK_ARG((((uintptr_t)workspace) & 1) == 0, "border_edt: the workspace must be 2-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    uint16_t* g = (uint16_t*)workspace;
    const long long excl = exclude < 0 ? LLONG_MIN : (long long)exclude;        // no mask value equals LLONG_MIN's stand-in for "none"
    const dim3 cgrid(cdiv(W, COL_W), B), cblock(COL_W, COL_SEGS);
    if (mask_is_int64)
        hipLaunchKernelGGL(edt_column_kernel<int64_t>, cgrid, cblock, 0, st, (const int64_t*)mask, H, W, excl, g);
    else
        hipLaunchKernelGGL(edt_column_kernel<uint8_t>, cgrid, cblock, 0, st, (const uint8_t*)mask, H, W, excl, g);
    UNET_CHECK_LAUNCH();
    // 4 W bytes of LDS per row: four rows per block up to W = 2048 (32 KiB), one row above (32 KiB at W = 8192)
    const int rpb = W <= 2048 ? 4 : 1;
    const long long rows = (long long)B * H;
    hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(64 * rpb), (size_t)rpb * 2 * W * sizeof(uint16_t), st,
                       g, rows, W, row_levels(W), d2);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_border_weight(const int32_t* d2, const int64_t* target, const float* class_w, int C, float w0, double sigma,
                                  long long P, float* pw, void* stream) {
    UNET_CHECK_ARG(d2 && target && pw && P > 0 && C > 0, "border_weight: bad args");
    UNET_CHECK_ARG(w0 >= 0.f && sigma > 0.0, "border_weight: needs w0 >= 0 and sigma > 0 (got %g, %g)", (double)w0, sigma);
    const double inv2s2 = 1.0 / (2.0 * sigma * sigma);
    hipLaunchKernelGGL(border_weight_kernel, dim3(ew_grid(P, 256)), dim3(256), 0, (hipStream_t)stream, d2, target, class_w, C, w0, inv2s2, P, pw);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
