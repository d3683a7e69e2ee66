// Pixel-level augmentations of a batch: the radiometric transforms of unet_amd/augment.py (RandomBrightnessContrast, CoarseDropout,
// RandomGamma, GaussNoise, ChannelDropout, ChannelShuffle, GaussianBlur, Blur) as albumentations applies them per image on the host.
//
// pixel_ops_kernel, in place: every fired image has a program of at most 8 pointwise ops in the kernel arguments (8 programs of 432
// bytes per launch); grid.y counts programs, so an image without one gets no block.  One thread owns a pixel -- four neighbouring
// pixels when W % 4 == 0, as one 16-byte access per channel -- across all channels: it loads every channel it needs, then computes,
// then stores, so a channel permutation is safe in place.  The only cross-channel op is the permutation; it is resolved before the
// loads by walking the program backwards (output channel c <- source channel s0, and the channel index each op sees on the way), so
// the gather happens in the load addresses and registers keep static indices.  Traffic: one read and one write of the fired images.
//
// blur_kernel, out of place: a block stages one plane's 32 x 64 output tile plus its halo of radius r (reflect-101, any distance) in
// LDS, filters rows into a second LDS tile and columns from there into memory, channel after channel.  LDS at r = 15: (62 x 94 + 62 x 64)
// floats = 38.3 KB, four blocks per CU in 160 KB.  Threads run x fastest and a 32-lane group never leaves a tile row (the tile is 64
// wide), so row taps (in[row][col + t]), column taps (mid[row + t][col]) and the staging stores (consecutive words) all touch 32
// consecutive banks: no conflicts in either pass, whatever the row stride.
//
// No atomics, no device allocation, no host wait; every load index is reflected or checked into the image, and the only stores are each
// thread's own output elements.
#include <cmath>

#include "border.h"
#include "common.h"
#include "philox.h"

using namespace unet;

namespace {

struct Progs {                // passed by value in the kernel arguments (3.4 KB)
    unet_pixel_prog p[UNET_PIXEL_MAX_PROGS];
};

struct RectSets {
    unet_rect_set s[UNET_PIXEL_MAX_PROGS];
};

struct Taps {                 // 2 KB
    int k[UNET_BLUR_MAX_IMAGES];
    float t[UNET_BLUR_MAX_IMAGES][UNET_BLUR_MAX_KSIZE];
};

// The Box-Muller pair of words (w0, w1): r cos(2 pi u1), r sin(2 pi u1), r = sqrt(-2 ln u0), u = ((w >> 8) + 0.5) 2^-24.  u has 25
// significant bits, one more than fp32 holds, so both functions get an argument that IS exact: ln u0 as log1p(-(1 - u0)) in the upper
// half (1 - u0 is exact there), and the angle reduced by half a turn (cos, sin change sign) when u1 >= 1/2.
__device__ __forceinline__ void box_muller(uint32_t w0, uint32_t w1, float& za, float& zb) {
    constexpr float S = 5.9604644775390625e-8f;        // 2^-24
    const uint32_t m0 = w0 >> 8, m1 = w1 >> 8;
    const float nl = m0 < (1u << 23) ? -logf(((float)m0 + 0.5f) * S) : -log1pf(-(((float)((1u << 24) - m0) - 0.5f) * S));
    const float r = sqrtf(2.0f * nl);
    float s, c;
    sincospif((float)(2u * (m1 & 0x7fffffu) + 1u) * S, &s, &c);       // 2 u1 minus 1 when u1 >= 1/2: at most 24 bits
    if (m1 >> 23) s = -s, c = -c;
    za = r * c;
    zb = r * s;
}

// ------------------------------------------------------------------------------------------------------------- pointwise programs
template <int V>
struct Px {                   // what a thread knows about its V pixels before the channel loop
    int x, y;
    uint32_t inrect;          // bit (4 i + l): pixel l lies in a rectangle of op i
};

template <int V>
__device__ __forceinline__ void apply_ops(const unet_pixel_prog& pr, const Px<V>& px, uint32_t chain, int direct, int H, int W, float v[V]) {
    for (uint32_t i = 0; i < pr.nops; ++i) {
        const unet_pixel_op& op = pr.ops[i];
        const uint32_t c = direct >= 0 ? (uint32_t)direct : (chain >> (4 * i)) & 15u;      // the channel this value sits in when op i runs
        switch (op.code & 0xffu) {
            case UNET_PIXEL_BRIGHTNESS_CONTRAST:
#pragma unroll
                for (int l = 0; l < V; ++l) {
                    float t = fmul_unfused(v[l], op.f0);             // the product rounded on its own (common.h): never an FMA with the sum
                    if (op.f1 != 0.0f) t = __fadd_rn(t, op.f1);
                    v[l] = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
                }
                break;
            case UNET_PIXEL_GAMMA:
#pragma unroll
                for (int l = 0; l < V; ++l) v[l] = powf(fmaxf(v[l], 0.0f), op.f0);
                break;
            case UNET_PIXEL_GAUSS_NOISE: {
                const uint32_t plane = (op.code & UNET_PIXEL_PER_CHANNEL) ? c : 0u;
                const uint32_t e = (plane * (uint32_t)H + (uint32_t)px.y) * (uint32_t)W + (uint32_t)px.x;
                uint32_t w[4];
                philox4x32_10(e >> 2, 0u, op.u0, op.u1, w);
                float z[4];
                if (V == 4) {                                        // W % 4 == 0 and x % 4 == 0: the four pixels are one counter
                    box_muller(w[0], w[1], z[0], z[1]);
                    box_muller(w[2], w[3], z[2], z[3]);
                } else {
                    float za, zb;
                    box_muller((e & 2u) ? w[2] : w[0], (e & 2u) ? w[3] : w[1], za, zb);
                    z[0] = (e & 1u) ? zb : za;
                }
#pragma unroll
                for (int l = 0; l < V; ++l) {
                    const float t = v[l] + op.f0 + op.f1 * z[l];
                    v[l] = fminf(fmaxf(t, 0.0f), 1.0f);
                }
                break;
            }
            case UNET_PIXEL_FILL_RECTS:
#pragma unroll
                for (int l = 0; l < V; ++l)
                    if ((px.inrect >> (4 * i + l)) & 1u) v[l] = op.f0;
                break;
            case UNET_PIXEL_CHANNEL_DROP:
                if ((op.u0 >> c) & 1u) {
#pragma unroll
                    for (int l = 0; l < V; ++l) v[l] = op.f0;
                }
                break;
            default:                                                 // UNET_PIXEL_CHANNEL_PERMUTE: done in the load addresses
                break;
        }
    }
}

// output channel c of the program: its source channel, and in `chain` (4 bits per op) the channel index every op sees on the way
__device__ __forceinline__ uint32_t source_channel(const unet_pixel_prog& pr, uint32_t c, uint32_t& chain) {
    uint32_t s = c;
    chain = 0;
    for (int i = (int)pr.nops - 1; i >= 0; --i) {
        const unet_pixel_op& op = pr.ops[i];
        if ((op.code & 0xffu) == UNET_PIXEL_CHANNEL_PERMUTE) s = ((s < 8u ? op.u0 >> (4u * s) : op.u1 >> (4u * (s - 8u)))) & 15u;
        chain |= s << (4 * i);
    }
    return s;
}

template <int V>
__device__ __forceinline__ void load_px(const float* p, float v[V]) {
    if (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        v[0] = *p;
    }
}

template <int V>
__device__ __forceinline__ void store_px(float* p, const float v[V]) {
    if (V == 4)
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else
        *p = v[0];
}

// CMAX > 0: C <= CMAX, all channels loaded (through the permutation) before the first store.  CMAX == 0: any C, channel after channel;
// the host refuses a permutation there.
template <int CMAX, int V>
__global__ __launch_bounds__(256) void pixel_ops_kernel(float* __restrict__ xb, int C, int H, int W, Progs progs) {
    const long long HW = (long long)H * W;
    const long long p = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (p >= HW) return;
    const unet_pixel_prog& pr = progs.p[blockIdx.y];
    Px<V> px;
    px.y = (int)(p / W);
    px.x = (int)(p - (long long)px.y * W);
    px.inrect = 0;
    for (uint32_t i = 0; i < pr.nops; ++i) {
        const unet_pixel_op& op = pr.ops[i];
        if ((op.code & 0xffu) != UNET_PIXEL_FILL_RECTS) continue;
        for (uint32_t k = op.u0; k < op.u0 + op.u1; ++k) {
            const int y0 = pr.rects[k][0], x0 = pr.rects[k][1], y1 = pr.rects[k][2], x1 = pr.rects[k][3];
            if (px.y < y0 || px.y >= y1) continue;
#pragma unroll
            for (int l = 0; l < V; ++l)
                if (px.x + l >= x0 && px.x + l < x1) px.inrect |= 1u << (4 * i + l);
        }
    }
    float* img = xb + (size_t)pr.image * C * HW + p;
    if (CMAX == 0) {
        for (int c = 0; c < C; ++c) {
            float v[V];
            load_px<V>(img + (size_t)c * HW, v);
            apply_ops<V>(pr, px, 0, c, H, W, v);
            store_px<V>(img + (size_t)c * HW, v);
        }
        return;
    }
    float v[CMAX > 0 ? CMAX : 1][V];
    uint32_t chain[CMAX > 0 ? CMAX : 1];
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (c < C) load_px<V>(img + (size_t)source_channel(pr, c, chain[c]) * HW, v[c]);
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
        if (c < C) {
            apply_ops<V>(pr, px, chain[c], -1, H, W, v[c]);
            store_px<V>(img + (size_t)c * HW, v[c]);
        }
}

template <typename T>
__global__ __launch_bounds__(256) void fill_rects_mask_kernel(T* __restrict__ mask, int H, int W, RectSets sets, T fill) {
    const long long HW = (long long)H * W;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    const unet_rect_set& s = sets.s[blockIdx.y];
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    bool in = false;
    for (uint32_t k = 0; k < s.nrects; ++k)
        in |= y >= s.rects[k][0] && y < s.rects[k][2] && x >= s.rects[k][1] && x < s.rects[k][3];
    if (in) mask[(size_t)s.image * HW + p] = fill;
}

// ------------------------------------------------------------------------------------------------------------------ separable blur
constexpr int BT_H = 32, BT_W = 64, BR_MAX = UNET_BLUR_MAX_KSIZE / 2;
constexpr int BS_W = BT_W + 2 * BR_MAX, BS_H = BT_H + 2 * BR_MAX;       // the staged tile: 62 rows of 94

__global__ __launch_bounds__(256) void blur_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int H, int W, Taps taps) {
    __shared__ float in[BS_H * BS_W];          // 23312 B
    __shared__ float mid[BS_H * BT_W];         // 15872 B
    const int j = blockIdx.z, k = taps.k[j], r = k >> 1;
    const float* tp = taps.t[j];
    const int x0 = blockIdx.x * BT_W, y0 = blockIdx.y * BT_H;
    const int tw = min(BT_W, W - x0), th = min(BT_H, H - y0);           // the part of the tile inside the image
    const int sw = tw + 2 * r, sh = th + 2 * r;
    const long long HW = (long long)H * W;
    const int tid = threadIdx.x;
    for (int c = 0; c < C; ++c) {
        const float* s = src + ((size_t)j * C + c) * HW;
        for (int idx = tid; idx < sh * BS_W; idx += 256) {             // stage: in[row][col] = plane at the reflected (y0 - r + row, x0 - r + col)
            const int row = idx / BS_W, col = idx - row * BS_W;
            if (col >= sw) continue;
            const int iy = border_index<B_REFLECT101>(y0 - r + row, H), ix = border_index<B_REFLECT101>(x0 - r + col, W);
            in[idx] = s[(size_t)iy * W + ix];
        }
        __syncthreads();
        for (int idx = tid; idx < sh * BT_W; idx += 256) {             // rows: mid[row][col] = sum_t tap[t] in[row][col + t]
            const int row = idx / BT_W, col = idx % BT_W;
            if (col >= tw) continue;
            const float* a = in + row * BS_W + col;
            float acc = tp[0] * a[0];
            for (int t = 1; t < k; ++t) acc = fmaf(tp[t], a[t], acc);
            mid[idx] = acc;
        }
        __syncthreads();
        float* d = dst + ((size_t)j * C + c) * HW;
        for (int idx = tid; idx < th * BT_W; idx += 256) {             // columns: out[row][col] = sum_t tap[t] mid[row + t][col]
            const int row = idx / BT_W, col = idx % BT_W;
            if (col >= tw) continue;
            const float* a = mid + idx;
            float acc = tp[0] * a[0];
            for (int t = 1; t < k; ++t) acc = fmaf(tp[t], a[t * BT_W], acc);
            d[(size_t)(y0 + row) * W + x0 + col] = acc;
        }
        __syncthreads();                                               // the next channel overwrites both tiles
    }
}

// H, W <= 65535 (rectangle corners are uint16) and C H W < 2^31 (the noise element index and every plane offset fit 32 bits)
bool sizes_ok(int n, int C, int H, int W) {
    return n >= 1 && C >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535 && (long long)C * H * W <= 0x7fffffffLL;
}

bool rects_ok(const uint16_t (*r)[4], uint32_t n, int H, int W) {
    for (uint32_t k = 0; k < n; ++k)
        if (!(r[k][0] < r[k][2] && r[k][1] < r[k][3] && r[k][2] <= H && r[k][3] <= W)) return false;
    return true;
}

// nullptr when the program is well formed, else what is wrong with it
const char* prog_error(const unet_pixel_prog& p, int C, int H, int W) {
    if (p.nops < 1 || p.nops > UNET_PIXEL_MAX_OPS) return "1..8 ops per program";
    if (p.nrects > UNET_PIXEL_MAX_RECTS || !rects_ok(p.rects, p.nrects, H, W)) return "a rectangle is empty or outside the image, or more than 32";
    for (uint32_t i = 0; i < p.nops; ++i) {
        const unet_pixel_op& op = p.ops[i];
        if (!std::isfinite(op.f0) || !std::isfinite(op.f1)) return "non-finite operand";
        if (op.code & ~(0xffu | UNET_PIXEL_PER_CHANNEL)) return "unknown opcode";
        switch (op.code & 0xffu) {
            case UNET_PIXEL_BRIGHTNESS_CONTRAST: case UNET_PIXEL_GAMMA: case UNET_PIXEL_GAUSS_NOISE: break;
            case UNET_PIXEL_FILL_RECTS:
                if (op.u0 > p.nrects || op.u1 > p.nrects - op.u0) return "FILL_RECTS names rectangles past nrects";
                break;
            case UNET_PIXEL_CHANNEL_DROP:
                if (C > 32) return "CHANNEL_DROP supports C <= 32";
                if (C < 32 && (op.u0 >> C)) return "CHANNEL_DROP names a channel >= C";
                break;
            case UNET_PIXEL_CHANNEL_PERMUTE: {
                if (C > 16) return "CHANNEL_PERMUTE supports C <= 16";
                const unsigned long long perm = (unsigned long long)op.u0 | ((unsigned long long)op.u1 << 32);
                uint32_t seen = 0;
                for (int c = 0; c < C; ++c) seen |= 1u << ((perm >> (4 * c)) & 15u);
                if (seen != (1u << C) - 1u) return "CHANNEL_PERMUTE is not a permutation of the C channels";
                break;
            }
            default: return "unknown opcode";
        }
    }
    return nullptr;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int unet_pixel_ops(float* x, int n, int C, int H, int W, const unet_pixel_prog* progs_host, int nprog, void* stream) {
    UNET_CHECK_ARG(x && progs_host, "pixel_ops: null pointer");
    UNET_CHECK_ARG(sizes_ok(n, C, H, W), "pixel_ops: bad sizes n=%d C=%d H=%d W=%d (H, W <= 65535, C H W < 2^31)", n, C, H, W);
    UNET_CHECK_ARG(nprog >= 1 && nprog <= UNET_PIXEL_MAX_PROGS, "pixel_ops: %d programs (1..%d per call)", nprog, UNET_PIXEL_MAX_PROGS);
    Progs progs;
    memset(&progs, 0, sizeof(progs));
    for (int j = 0; j < nprog; ++j) {
        const unet_pixel_prog& p = progs_host[j];
        UNET_CHECK_ARG(p.image < (uint32_t)n && (j == 0 || p.image > progs_host[j - 1].image),
                       "pixel_ops: program %d names image %u (indices strictly increasing, below n=%d)", j, p.image, n);
        const char* err = prog_error(p, C, H, W);
        UNET_CHECK_ARG(err == nullptr, "pixel_ops: program %d: %s", j, err);
        progs.p[j] = p;
    }
    // 16-byte accesses when every plane and row starts on 16 bytes; not with 9..16 channels held in registers at once (64 values per
    // thread: the compiler spills them)
    const bool vec = (W & 3) == 0 && aligned16(x) && (C <= 8 || C > 16);
    const dim3 grid(cdiv((long long)H * W, vec ? 1024 : 256), nprog);
#define PIXEL_LAUNCH(CMAX)                                                                                      \
    do {                                                                                                        \
        if (vec) hipLaunchKernelGGL((pixel_ops_kernel<CMAX, 4>), grid, dim3(256), 0, ST, x, C, H, W, progs);     \
        else hipLaunchKernelGGL((pixel_ops_kernel<CMAX, 1>), grid, dim3(256), 0, ST, x, C, H, W, progs);         \
    } while (0)
    if (C <= 4) PIXEL_LAUNCH(4);
    else if (C <= 8) PIXEL_LAUNCH(8);
    else if (C <= 16) hipLaunchKernelGGL((pixel_ops_kernel<16, 1>), grid, dim3(256), 0, ST, x, C, H, W, progs);
    else PIXEL_LAUNCH(0);                               // (prog_error has refused CHANNEL_PERMUTE for C > 16)
#undef PIXEL_LAUNCH
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_fill_rects_mask(void* mask, int dst_f32, int n, int H, int W, const unet_rect_set* sets_host, int nsets, double fill,
                                    void* stream) {
    UNET_CHECK_ARG(mask && sets_host, "fill_rects_mask: null pointer");
    UNET_CHECK_ARG(dst_f32 == 0 || dst_f32 == 1, "fill_rects_mask: dst_f32 must be 0 (int64) or 1 (fp32)");
    UNET_CHECK_ARG(sizes_ok(n, 1, H, W), "fill_rects_mask: bad sizes n=%d H=%d W=%d (H, W <= 65535)", n, H, W);
    UNET_CHECK_ARG(nsets >= 1 && nsets <= UNET_PIXEL_MAX_PROGS, "fill_rects_mask: %d rectangle sets (1..%d per call)", nsets, UNET_PIXEL_MAX_PROGS);
    UNET_CHECK_ARG(std::isfinite(fill) && (dst_f32 || fabs(fill) < 9.2e18), "fill_rects_mask: fill value %g is not finite / not an int64", fill);
    RectSets sets;
    memset(&sets, 0, sizeof(sets));
    for (int j = 0; j < nsets; ++j) {
        const unet_rect_set& s = sets_host[j];
        UNET_CHECK_ARG(s.image < (uint32_t)n && (j == 0 || s.image > sets_host[j - 1].image),
                       "fill_rects_mask: set %d names mask %u (indices strictly increasing, below n=%d)", j, s.image, n);
        UNET_CHECK_ARG(s.nrects >= 1 && s.nrects <= UNET_PIXEL_MAX_RECTS && rects_ok(s.rects, s.nrects, H, W),
                       "fill_rects_mask: set %d: a rectangle is empty or outside the mask, or not 1..32 of them", j);
        sets.s[j] = s;
    }
    const dim3 grid(cdiv((long long)H * W, 256), nsets);
    if (dst_f32)
        hipLaunchKernelGGL((fill_rects_mask_kernel<float>), grid, dim3(256), 0, ST, (float*)mask, H, W, sets, (float)fill);
    else
        hipLaunchKernelGGL((fill_rects_mask_kernel<long long>), grid, dim3(256), 0, ST, (long long*)mask, H, W, sets, (long long)fill);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_blur_separable(const float* src, float* dst, int n, int C, int H, int W, const int* ksize_host, const float* taps_host,
                                   void* stream) {
    UNET_CHECK_ARG(src && dst && ksize_host && taps_host, "blur_separable: null pointer");
    UNET_CHECK_ARG(src != dst, "blur_separable: src == dst (the blur is out of place)");
    UNET_CHECK_ARG(sizes_ok(n, C, H, W) && n <= UNET_BLUR_MAX_IMAGES, "blur_separable: bad sizes n=%d C=%d H=%d W=%d (1..%d images per call)",
                   n, C, H, W, UNET_BLUR_MAX_IMAGES);
    UNET_CHECK_ARG(cdiv(H, BT_H) <= 65535, "blur_separable: H=%d needs more than 65535 tile rows", H);
    Taps taps;
    memset(&taps, 0, sizeof(taps));
    for (int j = 0; j < n; ++j) {
        const int k = ksize_host[j];
        UNET_CHECK_ARG(k >= 1 && k <= UNET_BLUR_MAX_KSIZE && (k & 1), "blur_separable: kernel size %d of image %d (odd, 1..31)", k, j);
        for (int t = 0; t < k; ++t) {
            UNET_CHECK_ARG(std::isfinite(taps_host[j * UNET_BLUR_MAX_KSIZE + t]), "blur_separable: non-finite tap %d of image %d", t, j);
            taps.t[j][t] = taps_host[j * UNET_BLUR_MAX_KSIZE + t];
        }
        taps.k[j] = k;
    }
    hipLaunchKernelGGL(blur_kernel, dim3(cdiv(W, BT_W), cdiv(H, BT_H), n), dim3(256), 0, ST, src, dst, C, H, W, taps);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
