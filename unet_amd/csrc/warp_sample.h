// The one sampler of the warps: what the affine warp (warp.hip) and the field warp (warp_field.hip) do once they know the source
// coordinates (sx, sy) of an output pixel, and the argument checks their entry points share.  A warp kernel computes (sx, sy) its own
// way -- fp64, clamped to +-2^24 so that floor and the int conversion stay exact -- and hands them to sample_planes / sample_mask with
// an offset functor `at(ix, iy)` that turns a tap inside the grid into its offset in a plane.
//
// The rules: nearest is floor(s + 0.5); bilinear takes the 4 taps around s with fp32 weights, and on a grid point copies the tap bit
// for bit; every tap index is mapped into [0, W) x [0, H) by border_index or replaced by the fill value; masks are always nearest.
#pragma once

#include <cmath>

#include "border.h"
#include "common.h"

namespace unet {

// one tap of a plane: the value at offset o, or fill when the tap lies outside (constant border; o is 0 then).  The load is unconditional
// and always inside the plane, so the loads of several planes issue back to back.
__device__ __forceinline__ float tap(const float* __restrict__ plane, size_t o, bool ok, float fill) {
    const float v = plane[o];
    return ok ? v : fill;
}

// element p of a plane as the pixel (x, y): p = y W + x, x fastest
__device__ __forceinline__ void pixel_xy(long long p, int W, int& x, int& y) {
    y = (int)(p / W);
    x = (int)(p - (long long)y * W);
}

// the offset in a plane of tap (ix, iy), both inside the grid: row-major as it stands ...
struct RowMajor {
    int W;
    __device__ __forceinline__ size_t operator()(int ix, int iy) const { return (size_t)iy * W + ix; }
};

// ... or through a D4 map m of the H x W grid (d4_map of warp_field.hip checks it): integer entries, a permutation of the grid.
// Sampling the permuted image at s is sampling the image at the permuted taps of s with the same weights and the same border rule, so the
// map is applied to the tap indices -- exact, and bit for bit what permuting first would give.
struct TapMap {
    int a, b, c, d, e, f, W;
    __device__ __forceinline__ explicit TapMap(const float* m, int W_)
        : a((int)m[0]), b((int)m[1]), c((int)m[2]), d((int)m[3]), e((int)m[4]), f((int)m[5]), W(W_) {}
    __device__ __forceinline__ size_t operator()(int ix, int iy) const {
        return (size_t)(d * ix + e * iy + f) * W + (size_t)(a * ix + b * iy + c);
    }
};

// d[c HW] = plane c of s sampled at (sx, sy), c < C; taps and weights are computed once and reused for every plane
template <int BORDER, int INTERP, typename At>
__device__ __forceinline__ void sample_planes(const float* s, float* d, int C, long long HW, int H, int W,
                                              double sx, double sy, const At at, float fill) {
    if (INTERP == 0) {
        const int ix = border_index<BORDER>((int)floor(sx + 0.5), W), iy = border_index<BORDER>((int)floor(sy + 0.5), H);
        const bool ok = ix >= 0 && iy >= 0;
        const size_t o = ok ? at(ix, iy) : 0;
#pragma unroll 4
        for (int c = 0; c < C; ++c) d[(size_t)c * HW] = tap(s + (size_t)c * HW, o, ok, fill);
        return;
    }
    const double fx0 = floor(sx), fy0 = floor(sy);
    const float fx = (float)(sx - fx0), fy = (float)(sy - fy0);           // fp32 weights
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int ix0 = border_index<BORDER>(x0, W), ix1 = border_index<BORDER>(x0 + 1, W);
    const int iy0 = border_index<BORDER>(y0, H), iy1 = border_index<BORDER>(y0 + 1, H);
    if (fx == 0.0f && fy == 0.0f) {                    // on a grid point (a D4 map, an unfired image, a zero field): an exact copy of the tap
        const bool ok = ix0 >= 0 && iy0 >= 0;
        const size_t o = ok ? at(ix0, iy0) : 0;
#pragma unroll 4
        for (int c = 0; c < C; ++c) d[(size_t)c * HW] = tap(s + (size_t)c * HW, o, ok, fill);
        return;
    }
    const bool ok00 = ix0 >= 0 && iy0 >= 0, ok01 = ix1 >= 0 && iy0 >= 0, ok10 = ix0 >= 0 && iy1 >= 0, ok11 = ix1 >= 0 && iy1 >= 0;
    const size_t o00 = ok00 ? at(ix0, iy0) : 0, o01 = ok01 ? at(ix1, iy0) : 0;
    const size_t o10 = ok10 ? at(ix0, iy1) : 0, o11 = ok11 ? at(ix1, iy1) : 0;
    const float w00 = (1.0f - fx) * (1.0f - fy), w01 = fx * (1.0f - fy), w10 = (1.0f - fx) * fy, w11 = fx * fy;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
        const float* sc = s + (size_t)c * HW;
        const float v00 = tap(sc, o00, ok00, fill), v01 = tap(sc, o01, ok01, fill);
        const float v10 = tap(sc, o10, ok10, fill), v11 = tap(sc, o11, ok11, fill);
        d[(size_t)c * HW] = w00 * v00 + w01 * v01 + w10 * v10 + w11 * v11;
    }
}

// masks: nearest neighbour, floor(s + 0.5), whatever the image interpolation; element p of mask j of src / dst [n, H, W].  (It takes
// j and HW, not plane pointers: with the index formed here, j HW + at(...), the affine mask kernels compile to the code they had.)
template <typename T, int BORDER, typename At>
__device__ __forceinline__ void sample_mask(const T* src, T* dst, int j, long long HW, long long p, int H, int W, double sx,
                                            double sy, const At at, T fill) {
    const int ix = border_index<BORDER>((int)floor(sx + 0.5), W), iy = border_index<BORDER>((int)floor(sy + 0.5), H);
    dst[(size_t)j * HW + p] = ix >= 0 && iy >= 0 ? src[(size_t)j * HW + at(ix, iy)] : fill;
}

// ----------------------------------------------------------------------------------------------------------- the host side
// H, W <= 2^24 keeps every index expression of border_index inside int
inline bool sizes_ok(int n, int nmax, int H, int W) {
    return n >= 1 && n <= nmax && H > 0 && W > 0 && H <= (1 << 24) && W <= (1 << 24) && (long long)H * W <= 0x7fffffffLL;
}

inline bool known_border(int b) { return b == B_CONSTANT || b == B_REPLICATE || b == B_REFLECT || b == B_REFLECT101; }

inline bool all_finite(const float* v, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(v[k])) return false;
    return true;
}

// The arguments every image entry takes, checked under the entry's name `who`; params = its maps or descriptors.  An entry with a
// displacement field passes it and with_field (an entry without one passes null; dst is not null by then).
inline int check_image_args(const char* who, const void* src, const void* dst, const void* params, const void* field, bool with_field, int n,
                            int nmax, int C, int H, int W, int interp, int border, float fill) {
    UNET_CHECK_ARG(src && dst && params, "%s: null pointer", who);
    UNET_CHECK_ARG(src != dst && field != dst, "%s: src == dst%s (the warp is out of place)", who,
                   with_field ? " or field == dst" : "");
    UNET_CHECK_ARG(sizes_ok(n, nmax, H, W) && C > 0, "%s: bad sizes n=%d C=%d H=%d W=%d (1..%d images per call)", who, n, C, H, W, nmax);
    UNET_CHECK_ARG(interp == 0 || interp == 1, "%s: unknown interpolation %d (0 nearest, 1 bilinear)", who, interp);
    UNET_CHECK_ARG(known_border(border), "%s: unknown border mode %d (0 constant, 1 replicate, 2 reflect, 4 reflect-101)", who, border);
    UNET_CHECK_ARG(std::isfinite(fill), "%s: non-finite fill value", who);
    return UNET_OK;
}

inline int check_mask_args(const char* who, const void* src, const void* dst, const void* params, const void* field, bool with_field,
                           int dst_f32, int n, int nmax, int H, int W, int border, double fill) {
    UNET_CHECK_ARG(src && dst && params, "%s: null pointer", who);
    UNET_CHECK_ARG(src != dst && field != dst, "%s: src == dst%s (the warp is out of place)", who,
                   with_field ? " or field == dst" : "");
    UNET_CHECK_ARG(dst_f32 == 0 || dst_f32 == 1, "%s: dst_f32 must be 0 (int64) or 1 (fp32)", who);
    UNET_CHECK_ARG(sizes_ok(n, nmax, H, W), "%s: bad sizes n=%d H=%d W=%d (1..%d masks per call)", who, n, H, W, nmax);
    UNET_CHECK_ARG(known_border(border), "%s: unknown border mode %d (0 constant, 1 replicate, 2 reflect, 4 reflect-101)", who, border);
    UNET_CHECK_ARG(std::isfinite(fill) && (dst_f32 || fabs(fill) < 9.2e18), "%s: fill value %g is not finite / not an int64", who, fill);
    return UNET_OK;
}

}  // namespace unet

// CALL with BM = the border code as a constant
#define BORDER_DISPATCH(border, CALL)                                 \
    switch (border) {                                                 \
        case B_CONSTANT: { constexpr int BM = B_CONSTANT; CALL; break; }     \
        case B_REPLICATE: { constexpr int BM = B_REPLICATE; CALL; break; }   \
        case B_REFLECT: { constexpr int BM = B_REFLECT; CALL; break; }       \
        default: { constexpr int BM = B_REFLECT101; CALL; break; }           \
    }

// CALL with MT = the element type of a mask: float (regression targets) or long long (classes)
#define MASK_DISPATCH(dst_f32, CALL) \
    if (dst_f32) {                   \
        using MT = float;            \
        CALL;                        \
    } else {                         \
        using MT = long long;        \
        CALL;                        \
    }
