// Affine warps of a batch: the geometric augmentations of unet_amd/augment.py (RandomRotate90, Transpose, Rotate, ShiftScaleRotate and
// the flips when a pipeline holds one of those) as albumentations / cv2.warpAffine apply them per image on the host.
//
// Output pixel p of image j takes the source value at M_j * p, M_j = the 2 x 3 INVERSE map of image j (row-major, fp32), read from the
// kernel arguments (n <= 64: no device buffer, no copy).  One thread per output pixel, x fastest (coalesced stores); the source
// coordinates are computed here and sampled by warp_sample.h, the sampler this file shares with warp_field.hip: taps and bilinear
// weights are computed once and reused for every plane, every tap index is mapped into [0, W) x [0, H) by the border rule or replaced
// by the fill value, and the only store is the thread's own output pixel: no input reaches memory outside src / dst.  No atomics, no
// LDS: the result does not depend on launch order.
#include "warp_sample.h"

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

template <int BORDER, int INTERP>
__global__ __launch_bounds__(256) void warp_affine_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int H, int W,
                                                          Maps maps, float fill) {
    const long long HW = (long long)H * W;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    const int j = blockIdx.y;
    int x, y;
    pixel_xy(p, W, x, y);
    double sx, sy;
    src_coords(maps.m[j], x, y, sx, sy);
    sample_planes<BORDER, INTERP>(src + (size_t)j * C * HW, dst + (size_t)j * C * HW + p, C, HW, H, W, sx, sy, RowMajor{W}, fill);
}

template <typename T, int BORDER>
__global__ __launch_bounds__(256) void warp_mask_kernel(const T* __restrict__ src, T* __restrict__ dst, int H, int W, Maps maps, T fill) {
    const long long HW = (long long)H * W;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    const int j = blockIdx.y;
    int x, y;
    pixel_xy(p, W, x, y);
    double sx, sy;
    src_coords(maps.m[j], x, y, sx, sy);
    sample_mask<T, BORDER>(src, dst, j, HW, p, H, W, sx, sy, RowMajor{W}, fill);
}

bool load_maps(const float* host, int n, Maps& maps) {
    if (!all_finite(host, 6 * n)) return false;
    memset(&maps, 0, sizeof(maps));
    memcpy(maps.m, host, sizeof(float) * 6 * n);
    return true;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int unet_warp_affine(const float* src, float* dst, int n, int C, int H, int W, const float* inv_maps_host, int interp, int border,
                                float fill, void* stream) {
    if (const int e = check_image_args("warp_affine", src, dst, inv_maps_host, nullptr, false, n, MAXMAPS, C, H, W, interp, border, fill))
        return e;
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
    if (const int e = check_mask_args("warp_affine_mask", src, dst, inv_maps_host, nullptr, false, dst_f32, n, MAXMAPS, H, W, border, fill))
        return e;
    Maps maps;
    UNET_CHECK_ARG(load_maps(inv_maps_host, n, maps), "warp_affine_mask: non-finite map entry");
    const dim3 grid(cdiv((long long)H * W, 256), n);
    MASK_DISPATCH(dst_f32, BORDER_DISPATCH(border, hipLaunchKernelGGL((warp_mask_kernel<MT, BM>), grid, dim3(256), 0, ST, (const MT*)src,
                                                                      (MT*)dst, H, W, maps, (MT)fill)));
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
