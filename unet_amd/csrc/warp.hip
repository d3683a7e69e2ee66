// Affine warps of a batch: the geometric augmentations of unet_amd/augment.py (RandomRotate90, Transpose, Rotate, ShiftScaleRotate and
// the flips when a pipeline holds one of those) as albumentations / cv2.warpAffine apply them per image on the host.
//
// Output pixel p of image j takes the source value at M_j * p, M_j = the 2 x 3 INVERSE map of image j (row-major, fp32), read from the
// kernel arguments (n <= 64: no device buffer, no copy).  One thread per output pixel, x fastest (coalesced stores); the source
// coordinates, taps and bilinear weights are computed once and reused for every plane.  Every tap index is mapped into [0, W) x [0, H)
// by the border rule or replaced by the fill value, and the only store is the thread's own output pixel: no input reaches memory
// outside src / dst.  No atomics, no LDS: the result does not depend on launch order.
#include <cmath>

#include "border.h"
#include "common.h"

using namespace unet;

namespace {

constexpr int MAXMAPS = 64;

struct Maps {                 // passed by value in the kernel arguments (1.5 KB)
    float m[MAXMAPS][6];
};

// source coordinates of the output pixel (x, y) under map m, clamped to +-2^24 (floor and the int conversion stay exact).  fp64: a
// shifted, down-scaled map reaches coordinates of 10^4 - 10^5 pixels, where an fp32 coordinate is off by 10^-3 pixel and more; a few
// fp64 FMAs per pixel cost nothing next to the memory traffic.
__device__ __forceinline__ void src_coords(const float* m, int x, int y, double& sx, double& sy) {
    constexpr double LIM = 16777216.0;
    sx = fmin(fmax(fma((double)m[0], (double)x, fma((double)m[1], (double)y, (double)m[2])), -LIM), LIM);
    sy = fmin(fmax(fma((double)m[3], (double)x, fma((double)m[4], (double)y, (double)m[5])), -LIM), LIM);
}

// one tap of a plane: the value at offset o, or fill when the tap lies outside (constant border; o is 0 then).  The load is unconditional
// and always inside the plane, so the loads of several planes issue back to back.
__device__ __forceinline__ float tap(const float* __restrict__ plane, size_t o, bool ok, float fill) {
    const float v = plane[o];
    return ok ? v : fill;
}

template <int BORDER, int INTERP>
__global__ __launch_bounds__(256) void warp_affine_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int H, int W,
                                                          Maps maps, float fill) {
    const long long HW = (long long)H * W;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    const int j = blockIdx.y;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    double sx, sy;
    src_coords(maps.m[j], x, y, sx, sy);
    const float* s = src + (size_t)j * C * HW;
    float* d = dst + (size_t)j * C * HW + p;
    if (INTERP == 0) {
        const int ix = border_index<BORDER>((int)floor(sx + 0.5), W), iy = border_index<BORDER>((int)floor(sy + 0.5), H);
        const bool ok = ix >= 0 && iy >= 0;
        const size_t o = ok ? (size_t)iy * W + ix : 0;
#pragma unroll 4
        for (int c = 0; c < C; ++c) d[(size_t)c * HW] = tap(s + (size_t)c * HW, o, ok, fill);
        return;
    }
    const double fx0 = floor(sx), fy0 = floor(sy);
    const float fx = (float)(sx - fx0), fy = (float)(sy - fy0);           // fp32 weights
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int ix0 = border_index<BORDER>(x0, W), ix1 = border_index<BORDER>(x0 + 1, W);
    const int iy0 = border_index<BORDER>(y0, H), iy1 = border_index<BORDER>(y0 + 1, H);
    if (fx == 0.0f && fy == 0.0f) {                    // on a grid point (every D4 map): an exact copy of the tap, whatever its value
        const bool ok = ix0 >= 0 && iy0 >= 0;
        const size_t o = ok ? (size_t)iy0 * W + ix0 : 0;
#pragma unroll 4
        for (int c = 0; c < C; ++c) d[(size_t)c * HW] = tap(s + (size_t)c * HW, o, ok, fill);
        return;
    }
    const bool ok00 = ix0 >= 0 && iy0 >= 0, ok01 = ix1 >= 0 && iy0 >= 0, ok10 = ix0 >= 0 && iy1 >= 0, ok11 = ix1 >= 0 && iy1 >= 0;
    const size_t o00 = ok00 ? (size_t)iy0 * W + ix0 : 0, o01 = ok01 ? (size_t)iy0 * W + ix1 : 0;
    const size_t o10 = ok10 ? (size_t)iy1 * W + ix0 : 0, o11 = ok11 ? (size_t)iy1 * W + ix1 : 0;
    const float w00 = (1.0f - fx) * (1.0f - fy), w01 = fx * (1.0f - fy), w10 = (1.0f - fx) * fy, w11 = fx * fy;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
        const float* sc = s + (size_t)c * HW;
        const float v00 = tap(sc, o00, ok00, fill), v01 = tap(sc, o01, ok01, fill);
        const float v10 = tap(sc, o10, ok10, fill), v11 = tap(sc, o11, ok11, fill);
        d[(size_t)c * HW] = w00 * v00 + w01 * v01 + w10 * v10 + w11 * v11;
    }
}

// masks: nearest neighbour, floor(s + 0.5), whatever the image interpolation
template <typename T, int BORDER>
__global__ __launch_bounds__(256) void warp_mask_kernel(const T* __restrict__ src, T* __restrict__ dst, int H, int W, Maps maps, T fill) {
    const long long HW = (long long)H * W;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    const int j = blockIdx.y;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    double sx, sy;
    src_coords(maps.m[j], x, y, sx, sy);
    const int ix = border_index<BORDER>((int)floor(sx + 0.5), W), iy = border_index<BORDER>((int)floor(sy + 0.5), H);
    dst[(size_t)j * HW + p] = ix >= 0 && iy >= 0 ? src[(size_t)j * HW + (size_t)iy * W + ix] : fill;
}

bool load_maps(const float* host, int n, Maps& maps) {
    for (int k = 0; k < 6 * n; ++k)
        if (!std::isfinite(host[k])) return false;
    memset(&maps, 0, sizeof(maps));
    memcpy(maps.m, host, sizeof(float) * 6 * n);
    return true;
}

// H, W <= 2^24 keeps every index expression of border_index inside int
bool sizes_ok(int n, int H, int W) {
    return n >= 1 && n <= MAXMAPS && H > 0 && W > 0 && H <= (1 << 24) && W <= (1 << 24) && (long long)H * W <= 0x7fffffffLL;
}

bool known_border(int b) { return b == B_CONSTANT || b == B_REPLICATE || b == B_REFLECT || b == B_REFLECT101; }

}  // namespace

#define ST ((hipStream_t)stream)

#define BORDER_DISPATCH(border, CALL)                                 \
    switch (border) {                                                 \
        case B_CONSTANT: { constexpr int BM = B_CONSTANT; CALL; break; }     \
        case B_REPLICATE: { constexpr int BM = B_REPLICATE; CALL; break; }   \
        case B_REFLECT: { constexpr int BM = B_REFLECT; CALL; break; }       \
        default: { constexpr int BM = B_REFLECT101; CALL; break; }           \
    }

extern "C" int unet_warp_affine(const float* src, float* dst, int n, int C, int H, int W, const float* inv_maps_host, int interp, int border,
                                float fill, void* stream) {
    UNET_CHECK_ARG(src && dst && inv_maps_host, "warp_affine: null pointer");
    UNET_CHECK_ARG(src != dst, "warp_affine: src == dst (the warp is out of place)");
    UNET_CHECK_ARG(sizes_ok(n, H, W) && C > 0, "warp_affine: bad sizes n=%d C=%d H=%d W=%d (1..64 images per call)",
                   n, C, H, W);
    UNET_CHECK_ARG(interp == 0 || interp == 1, "warp_affine: unknown interpolation %d (0 nearest, 1 bilinear)", interp);
    UNET_CHECK_ARG(known_border(border), "warp_affine: unknown border mode %d (0 constant, 1 replicate, 2 reflect, 4 reflect-101)", border);
    UNET_CHECK_ARG(std::isfinite(fill), "warp_affine: non-finite fill value");
    Maps maps;
    UNET_CHECK_ARG(load_maps(inv_maps_host, n, maps), "warp_affine: non-finite map entry");
    const dim3 grid(cdiv((long long)H * W, 256), n);
    if (interp == 0) {
        BORDER_DISPATCH(border, hipLaunchKernelGGL((warp_affine_kernel<BM, 0>), grid, dim3(256), 0, ST, src, dst, C, H, W, maps, fill));
    } else {
        BORDER_DISPATCH(border, hipLaunchKernelGGL((warp_affine_kernel<BM, 1>), grid, dim3(256), 0, ST, src, dst, C, H, W, maps, fill));
    }
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_warp_affine_mask(const void* src, void* dst, int dst_f32, int n, int H, int W, const float* inv_maps_host, int border,
                                     double fill, void* stream) {
    UNET_CHECK_ARG(src && dst && inv_maps_host, "warp_affine_mask: null pointer");
    UNET_CHECK_ARG(src != dst, "warp_affine_mask: src == dst (the warp is out of place)");
    UNET_CHECK_ARG(dst_f32 == 0 || dst_f32 == 1, "warp_affine_mask: dst_f32 must be 0 (int64) or 1 (fp32)");
    UNET_CHECK_ARG(sizes_ok(n, H, W), "warp_affine_mask: bad sizes n=%d H=%d W=%d (1..64 masks per call)", n, H, W);
    UNET_CHECK_ARG(known_border(border), "warp_affine_mask: unknown border mode %d (0 constant, 1 replicate, 2 reflect, 4 reflect-101)",
                   border);
    UNET_CHECK_ARG(std::isfinite(fill) && (dst_f32 || fabs(fill) < 9.2e18), "warp_affine_mask: fill value %g is not finite / not an int64", fill);
    Maps maps;
    UNET_CHECK_ARG(load_maps(inv_maps_host, n, maps), "warp_affine_mask: non-finite map entry");
    const dim3 grid(cdiv((long long)H * W, 256), n);
    if (dst_f32) {
        BORDER_DISPATCH(border, hipLaunchKernelGGL((warp_mask_kernel<float, BM>), grid, dim3(256), 0, ST, (const float*)src, (float*)dst, H, W,
                                                   maps, (float)fill));
    } else {
        BORDER_DISPATCH(border, hipLaunchKernelGGL((warp_mask_kernel<long long, BM>), grid, dim3(256), 0, ST, (const long long*)src,
                                                   (long long*)dst, H, W, maps, (long long)fill));
    }
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
