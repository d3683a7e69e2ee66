// Non-rigid warps of a batch: the field augmentations of unet_amd/augment.py (ElasticTransform, GridDistortion, OpticalDistortion) as
// albumentations / cv2.remap apply them per image on the host.
//
// warp_field_kernel / warp_field_mask_kernel, the remap: output pixel p of image j takes the source value at pre_j * (p + d_j(p)).  d_j is
// the displacement of the launch's kind -- a dense field [n, 2, H, W] in device memory (8 bytes per pixel next to the 32 the image
// moves at C = 4), or evaluated per pixel from the image's descriptor in the kernel arguments (grid: per-axis node values with the
// linspace between them; optical: k, dx, dy) -- and zero for an image that did not fire.  pre_j is the 2 x 3 inverse map of the D4
// transforms that share the segment: a permutation of the grid, applied to the tap indices (TapMap of warp_sample.h).  One thread per
// output pixel, x fastest; coordinates in fp64 clamped to +-2^24, then the sampler of csrc/warp_sample.h, the one csrc/warp.hip uses:
// taps and bilinear weights computed once for all planes.  Every tap index is mapped into the image by border_index or replaced by
// fill, and a checked D4 map keeps it
// there, so no field value -- NaN and infinity included -- reaches memory outside src.
//
// elastic_rows_kernel / elastic_cols_kernel, the displacement field of ElasticTransform: uniform noise in (-1, 1) smoothed by a separable
// Gaussian of up to 401 taps, times alpha.  The noise is a pure function of (key, plane, y W + x) (Philox4x32-10, include/unet_hip.h) and is
// generated into LDS by the row pass -- it never exists in memory.  A row block stages 4 rows of 256 + 2 r noise values (reflect-101 at
// any distance) and every thread runs the taps down 4 accumulators; LDS at r = 200: 4 x 656 floats = 10.3 KB.  The row result goes to the
// caller's workspace once.  A column block stages (64 + 2 r) reflected rows of 32 columns of it (128-byte row segments; 58 KB at
// r = 200, 14 KB at r = 24) and filters from LDS, so a row result is read from memory (64 + 2 r) / 64 times, not ksize times.  Lanes run
// along x in both passes: 32 consecutive words per row of lanes, no bank conflicts.  The taps are read from the kernel arguments with a
// uniform index (scalar loads).
//
// No atomics, no device allocation, no host wait; the only stores are each thread's own output elements.
#include "philox.h"
#include "warp_sample.h"

using namespace unet;

namespace {

struct Images {               // passed by value in the kernel arguments (2.75 KB)
    unet_field_image im[UNET_FIELD_MAX_IMAGES];
};

struct Elastic {              // 2.8 KB
    unet_elastic_image im[UNET_ELASTIC_MAX_IMAGES];
    float taps[UNET_ELASTIC_MAX_KSIZE];
};

// entry i of np.linspace over the cell of i: cells of `step` entries (the last one clipped at N), cell c from nodes[c] to nodes[c + 1],
// endpoint included; a cell of one entry gets its first node
__device__ __forceinline__ double grid_axis(const float* nodes, int i, int N, int step) {
    const int cell = i / step, a = cell * step, len = min(step, N - a), l = i - a;
    const double prev = (double)nodes[cell], cur = (double)nodes[cell + 1];
    if (l == 0) return prev;
    if (l == len - 1) return cur;
    return prev + (double)l * ((cur - prev) / (double)(len - 1));
}

// source coordinates of the output pixel (x, y) = element p of its plane; f = the image's two field planes (dense kind only)
template <int KIND>
__device__ __forceinline__ void src_coords(const unet_field_image& im, const float* __restrict__ f, long long p, long long HW, int x, int y,
                                           int H, int W, int step_x, int step_y, double& sx, double& sy) {
    constexpr double LIM = 16777216.0;
    double px = (double)x, py = (double)y;
    if (im.fired) {
        if (KIND == UNET_FIELD_DENSE) {
            px += (double)f[p];
            py += (double)f[HW + p];
        } else if (KIND == UNET_FIELD_GRID) {
            px = grid_axis(im.nodes[0], x, W, step_x);
            py = grid_axis(im.nodes[1], y, H, step_y);
        } else {                                       // x + (x - c) (kappa - 1) + shift: the identity, exactly, at k = 0 and shift 0
            const double ax = px - 0.5 * (double)(W - 1), ay = py - 0.5 * (double)(H - 1);
            const double u = ax / (double)W, v = ay / (double)H, r2 = u * u + v * v;
            const double g = (double)im.optical[0] * (r2 + r2 * r2);
            px = px + ax * g + (double)im.optical[1];
            py = py + ay * g + (double)im.optical[2];
        }
    }
    sx = fmin(fmax(px, -LIM), LIM);                    // (a NaN comes out as -2^24)
    sy = fmin(fmax(py, -LIM), LIM);
}

// pre = the image's D4 pre-map (load_images checks it), applied to the tap indices: TapMap of warp_sample.h
template <int KIND, int BORDER, int INTERP>
__global__ __launch_bounds__(256) void warp_field_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                         const float* __restrict__ field, int C, int H, int W, int step_x, int step_y,
                                                         Images images, float fill) {
    const long long HW = (long long)H * W;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    const int j = blockIdx.y;
    int x, y;
    pixel_xy(p, W, x, y);
    double sx, sy;
    src_coords<KIND>(images.im[j], KIND == UNET_FIELD_DENSE ? field + (size_t)j * 2 * HW : nullptr, p, HW, x, y, H, W, step_x, step_y, sx, sy);
    const TapMap at(images.im[j].pre, W);
    sample_planes<BORDER, INTERP>(src + (size_t)j * C * HW, dst + (size_t)j * C * HW + p, C, HW, H, W, sx, sy, at, fill);
}

template <typename T, int KIND, int BORDER>
__global__ __launch_bounds__(256) void warp_field_mask_kernel(const T* __restrict__ src, T* __restrict__ dst, const float* __restrict__ field,
                                                              int H, int W, int step_x, int step_y, Images images, T fill) {
    const long long HW = (long long)H * W;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    const int j = blockIdx.y;
    int x, y;
    pixel_xy(p, W, x, y);
    double sx, sy;
    src_coords<KIND>(images.im[j], KIND == UNET_FIELD_DENSE ? field + (size_t)j * 2 * HW : nullptr, p, HW, x, y, H, W, step_x, step_y, sx, sy);
    const TapMap at(images.im[j].pre, W);
    sample_mask<T, BORDER>(src, dst, j, HW, p, H, W, sx, sy, at, fill);
}

// ----------------------------------------------------------------------------------------------------------- the elastic field
// word e % 4 of Philox4x32-10 under (k0, k1) at counter (e / 4, plane, 0, 0), as 2 u - 1 with u = ((w >> 8) + 0.5) 2^-24: the odd integer
// 2 (w >> 8) + 1 - 2^24 (below 2^24 in magnitude: exact in fp32) times 2^-24
__device__ __forceinline__ float field_noise(uint32_t k0, uint32_t k1, uint32_t plane, uint32_t e) {
    uint32_t c[4];
    philox4x32_10(e >> 2, plane, k0, k1, c);
    const uint32_t w = (e & 2u) ? ((e & 1u) ? c[3] : c[2]) : ((e & 1u) ? c[1] : c[0]);
    return (float)((int)(2u * (w >> 8) + 1u) - (1 << 24)) * 5.9604644775390625e-8f;
}

constexpr int RT_W = 256, RT_H = 4;                    // row pass: outputs per block
constexpr int CT_W = 32, CT_H = 64, CT_G = 8;          // column pass: outputs per block; 256 threads = 32 columns x 8 row groups

size_t rows_lds(int ksize) { return sizeof(float) * RT_H * (RT_W + 2 * (ksize >> 1)); }
size_t cols_lds(int ksize) { return sizeof(float) * (CT_H + 2 * (ksize >> 1)) * CT_W; }

__global__ __launch_bounds__(256) void elastic_rows_kernel(float* __restrict__ ws, int H, int W, int ksize, Elastic a) {
    extern __shared__ float lds[];                     // RT_H rows of RT_W + 2 r noise values
    const int j = blockIdx.z >> 1, q = blockIdx.z & 1;
    const unet_elastic_image& im = a.im[j];
    if (!im.fired) return;                             // (the whole block: the column pass writes the zeros)
    const int r = ksize >> 1, stride = RT_W + 2 * r;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;
    const int tw = min(RT_W, W - x0), th = min(RT_H, H - y0), sw = tw + 2 * r;
    const uint32_t plane = im.same_dxdy ? 0u : (uint32_t)q;
    const int tid = threadIdx.x;
    for (int idx = tid; idx < RT_H * stride; idx += 256) {
        const int row = idx / stride, col = idx - row * stride;
        float v = 0.0f;
        if (row < th && col < sw) {
            const int ix = border_index<B_REFLECT101>(x0 - r + col, W);
            v = field_noise(im.key0, im.key1, plane, (uint32_t)(y0 + row) * (uint32_t)W + (uint32_t)ix);
        }
        lds[idx] = v;
    }
    __syncthreads();
    if (tid >= tw) return;
    float acc[RT_H];
#pragma unroll
    for (int rr = 0; rr < RT_H; ++rr) acc[rr] = 0.0f;
    const float* e = lds + tid;
    for (int t = 0; t < ksize; ++t) {
        const float g = a.taps[t];
#pragma unroll
        for (int rr = 0; rr < RT_H; ++rr) acc[rr] = fmaf(g, e[rr * stride + t], acc[rr]);
    }
    float* d = ws + ((size_t)blockIdx.z * H + y0) * W + x0 + tid;
#pragma unroll
    for (int rr = 0; rr < RT_H; ++rr)
        if (rr < th) d[(size_t)rr * W] = acc[rr];
}

__global__ __launch_bounds__(256) void elastic_cols_kernel(const float* __restrict__ ws, float* __restrict__ field, int H, int W, int ksize,
                                                           Elastic a) {
    extern __shared__ float lds[];                     // CT_H + 2 r rows of CT_W row-pass values
    const int j = blockIdx.z >> 1;
    const unet_elastic_image& im = a.im[j];
    const int r = ksize >> 1;
    const int x0 = blockIdx.x * CT_W, y0 = blockIdx.y * CT_H;
    const int tw = min(CT_W, W - x0), th = min(CT_H, H - y0), sh = th + 2 * r;
    const int tid = threadIdx.x, col = tid & (CT_W - 1), rg = tid / CT_W;
    float* d = field + ((size_t)blockIdx.z * H + y0) * W + x0 + col;
    if (!im.fired) {
        if (col < tw)
            for (int row = rg; row < th; row += CT_G) d[(size_t)row * W] = 0.0f;
        return;
    }
    const float* s = ws + (size_t)blockIdx.z * H * W + x0;
    for (int idx = tid; idx < (CT_H + 2 * r) * CT_W; idx += 256) {
        const int row = idx / CT_W, c = idx & (CT_W - 1);
        float v = 0.0f;
        if (row < sh && c < tw) v = s[(size_t)border_index<B_REFLECT101>(y0 - r + row, H) * W + c];
        lds[idx] = v;
    }
    __syncthreads();
    if (col >= tw) return;
    float acc[CT_H / CT_G];
#pragma unroll
    for (int i = 0; i < CT_H / CT_G; ++i) acc[i] = 0.0f;
    const float* m = lds + rg * CT_W + col;
    for (int t = 0; t < ksize; ++t) {
        const float g = a.taps[t];
#pragma unroll
        for (int i = 0; i < CT_H / CT_G; ++i) acc[i] = fmaf(g, m[(CT_G * i + t) * CT_W], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < CT_H / CT_G; ++i)
        if (rg + CT_G * i < th) d[(size_t)(rg + CT_G * i) * W] = im.alpha * acc[i];
}

// m maps the grid [0, W) x [0, H) onto itself as a flip, a transposition or a product of them: each row has one entry +-1 on its own
// axis (or, on a square grid, on the other one), offset 0 for +1 and N - 1 for -1
bool d4_map(const float* m, int H, int W) {
    const bool straight = m[1] == 0.0f && m[3] == 0.0f, swapped = m[0] == 0.0f && m[4] == 0.0f && H == W;
    if (!straight && !swapped) return false;
    const float sx = straight ? m[0] : m[1], sy = straight ? m[4] : m[3];
    if (sx != 1.0f && sx != -1.0f) return false;
    if (sy != 1.0f && sy != -1.0f) return false;
    return m[2] == (sx > 0 ? 0.0f : (float)(W - 1)) && m[5] == (sy > 0 ? 0.0f : (float)(H - 1));
}

// nullptr when the descriptors are well formed, else what is wrong with them; `images` gets the copy that goes into the arguments
const char* load_images(const unet_field_image* host, int n, int kind, const float* field, int H, int W, int step_x, int step_y, Images& images) {
    if (kind != UNET_FIELD_DENSE && kind != UNET_FIELD_GRID && kind != UNET_FIELD_OPTICAL) return "unknown kind (0 dense, 1 grid, 2 optical)";
    if (kind == UNET_FIELD_DENSE && !field) return "null field";
    int cells_x = 0, cells_y = 0;
    if (kind == UNET_FIELD_GRID) {
        if (step_x < 1 || step_y < 1) return "grid steps below 1";
        cells_x = cdiv(W, step_x), cells_y = cdiv(H, step_y);
        if (cells_x > UNET_FIELD_MAX_CELLS || cells_y > UNET_FIELD_MAX_CELLS) return "more than 16 grid cells on an axis";
    }
    memset(&images, 0, sizeof(images));
    for (int j = 0; j < n; ++j) {
        const unet_field_image& im = host[j];
        if (im.fired != 0 && im.fired != 1) return "fired must be 0 or 1";
        if (!all_finite(im.pre, 6)) return "non-finite pre-map entry";
        if (!d4_map(im.pre, H, W)) return "the pre-map is not a D4 map of the H x W grid";
        images.im[j].fired = im.fired;
        memcpy(images.im[j].pre, im.pre, sizeof(im.pre));
        if (kind == UNET_FIELD_OPTICAL) {
            if (!all_finite(im.optical, 3)) return "non-finite optical parameter";
            memcpy(images.im[j].optical, im.optical, sizeof(im.optical));
        } else if (kind == UNET_FIELD_GRID) {
            if (!all_finite(im.nodes[0], cells_x + 1) || !all_finite(im.nodes[1], cells_y + 1)) return "non-finite grid node";
            memcpy(images.im[j].nodes[0], im.nodes[0], sizeof(float) * (cells_x + 1));
            memcpy(images.im[j].nodes[1], im.nodes[1], sizeof(float) * (cells_y + 1));
        }
    }
    return nullptr;
}

}  // namespace

#define ST ((hipStream_t)stream)

#define KIND_DISPATCH(kind, CALL)                                              \
    switch (kind) {                                                            \
        case UNET_FIELD_DENSE: { constexpr int KD = UNET_FIELD_DENSE; CALL; break; }   \
        case UNET_FIELD_GRID: { constexpr int KD = UNET_FIELD_GRID; CALL; break; }     \
        default: { constexpr int KD = UNET_FIELD_OPTICAL; CALL; break; }               \
    }

extern "C" int unet_warp_field(const float* src, float* dst, int n, int C, int H, int W, int kind, const unet_field_image* images_host,
                               const float* field, int grid_step_x, int grid_step_y, int interp, int border, float fill, void* stream) {
    if (const int e = check_image_args("warp_field", src, dst, images_host, field, true, n, UNET_FIELD_MAX_IMAGES, C, H, W, interp, border, fill))
        return e;
    Images images;
    const char* err = load_images(images_host, n, kind, field, H, W, grid_step_x, grid_step_y, images);
    UNET_CHECK_ARG(err == nullptr, "warp_field: %s", err);
    const dim3 grid(cdiv((long long)H * W, 256), n);
#define FIELD_LAUNCH(IP)                                                                                                     \
    KIND_DISPATCH(kind, BORDER_DISPATCH(border, hipLaunchKernelGGL((warp_field_kernel<KD, BM, IP>), grid, dim3(256), 0, ST, src, dst, field, \
                                                                   C, H, W, grid_step_x, grid_step_y, images, fill)))
    if (interp == 0) {
        FIELD_LAUNCH(0);
    } else {
        FIELD_LAUNCH(1);
    }
#undef FIELD_LAUNCH
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_warp_field_mask(const void* src, void* dst, int dst_f32, int n, int H, int W, int kind, const unet_field_image* images_host,
                                    const float* field, int grid_step_x, int grid_step_y, int border, double fill, void* stream) {
    if (const int e = check_mask_args("warp_field_mask", src, dst, images_host, field, true, dst_f32, n, UNET_FIELD_MAX_IMAGES, H, W, border, fill))
        return e;
    Images images;
    const char* err = load_images(images_host, n, kind, field, H, W, grid_step_x, grid_step_y, images);
    UNET_CHECK_ARG(err == nullptr, "warp_field_mask: %s", err);
    const dim3 grid(cdiv((long long)H * W, 256), n);
    MASK_DISPATCH(dst_f32, KIND_DISPATCH(kind, BORDER_DISPATCH(border, hipLaunchKernelGGL((warp_field_mask_kernel<MT, KD, BM>), grid, dim3(256), 0,
                                                                                          ST, (const MT*)src, (MT*)dst, field, H, W, grid_step_x,
                                                                                          grid_step_y, images, (MT)fill))));
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_elastic_field(float* field, float* workspace, int n, int H, int W, const unet_elastic_image* images_host,
                                  const float* taps_host, int ksize, void* stream) {
    UNET_CHECK_ARG(field && workspace && images_host && taps_host, "elastic_field: null pointer");
    UNET_CHECK_ARG(field != workspace, "elastic_field: field == workspace (the column pass is out of place)");
    UNET_CHECK_ARG(sizes_ok(n, UNET_ELASTIC_MAX_IMAGES, H, W), "elastic_field: bad sizes n=%d H=%d W=%d (1..%d images per call)", n, H, W,
                   UNET_ELASTIC_MAX_IMAGES);
    UNET_CHECK_ARG(cdiv(H, RT_H) <= 65535, "elastic_field: H=%d needs more than 65535 row blocks", H);
    UNET_CHECK_ARG(ksize >= 1 && ksize <= UNET_ELASTIC_MAX_KSIZE && (ksize & 1), "elastic_field: kernel size %d (odd, 1..%d)", ksize,
                   UNET_ELASTIC_MAX_KSIZE);
    Elastic a;
    memset(&a, 0, sizeof(a));
    UNET_CHECK_ARG(all_finite(taps_host, ksize), "elastic_field: non-finite tap");
    memcpy(a.taps, taps_host, sizeof(float) * ksize);
    bool any = false;
    for (int j = 0; j < n; ++j) {
        const unet_elastic_image& im = images_host[j];
        UNET_CHECK_ARG((im.fired == 0 || im.fired == 1) && (im.same_dxdy == 0 || im.same_dxdy == 1),
                       "elastic_field: image %d: fired and same_dxdy must be 0 or 1", j);
        UNET_CHECK_ARG(std::isfinite(im.alpha), "elastic_field: image %d: non-finite alpha", j);
        a.im[j] = im;
        any |= im.fired != 0;
    }
    if (any)
        hipLaunchKernelGGL(elastic_rows_kernel, dim3(cdiv(W, RT_W), cdiv(H, RT_H), 2 * n), dim3(256), rows_lds(ksize), ST, workspace, H, W,
                           ksize, a);
    hipLaunchKernelGGL(elastic_cols_kernel, dim3(cdiv(W, CT_W), cdiv(H, CT_H), 2 * n), dim3(256), cols_lds(ksize), ST, workspace, field, H, W,
                       ksize, a);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
