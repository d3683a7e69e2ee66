// The overview pyramid of a tiled GeoTIFF built on the device (unet_amd/tiffenc.py): one launch per level over all planes.
//   unet_tiff_reduce_level   [P, H, W] samples (row / plane strides free: level 0 is read where it lies) -> dense [P, ceil(H/2), ceil(W/2)]
// An output sample looks at the up-to-2x2 block of its parent, clipped at odd edges, in row-major order (TL, TR, BL, BR).  A sample is
// valid if no nodata was given or it differs from nodata (NaN nodata: valid = not NaN); a block without a valid sample gives nodata.
//   nearest  the top-left sample, valid or not
//   mode     the valid value with the highest count, ties to the value that occurs first
//   average  integers: floor((2 s + n) / (2 n)), s the exact sum of the n valid samples (round half up, also below zero);
//            float32: the valid samples summed one after the other in fp32 starting from +0, divided by float(n), correctly rounded
// A thread produces 16 bytes of one output row from 32 bytes of two parent rows: 16-byte loads and stores where the pointers, strides
// and row lengths allow (host flags + whole groups), sample by sample otherwise.  No atomics, no shared memory: every output sample depends
// on its own block alone.
#include "common.h"

using namespace unet;

namespace {

enum { RS_NEAREST = 0, RS_MODE = 1, RS_AVERAGE = 2 };

struct RedArgs {
    const void* src;
    void* dst;
    long long row_stride, plane_stride, total;          // strides in samples; total = P * h * groups threads
    int H, W, h, w, groups;                             // parent size, output size, 16-byte groups per output row
    int src_vec, dst_vec;                               // 16-byte accesses are aligned on every row
    int has_nodata, nan_nodata;
    double nodata;
};

template <typename T>
struct Rule {
    static constexpr bool is_float = false;
    T nd;
    int has, nan_nd;
    __device__ __forceinline__ bool valid(T v) const { return !has || v != nd; }
};
template <>
struct Rule<float> {
    static constexpr bool is_float = true;
    float nd;
    int has, nan_nd;
    __device__ __forceinline__ bool valid(float v) const { return !has || (nan_nd ? v == v : v != nd); }
};

// the rule for one block: v[0..3] in row-major order, in[k]: sample k lies inside the parent
template <typename T, int MODE>
__device__ __forceinline__ T reduce_block(const T (&v)[4], const bool (&in)[4], const Rule<T>& r) {
    if constexpr (MODE == RS_NEAREST) return v[0];
    bool ok[4];
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ok[k] = in[k] && r.valid(v[k]);
        n += ok[k];
    }
    if (n == 0) return r.nd;                            // (n == 0 needs a nodata: without one the top-left sample always counts)
    if constexpr (MODE == RS_AVERAGE) {
        if constexpr (Rule<T>::is_float) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) acc = acc + v[k];
            return __fdiv_rn(acc, (float)n);            // IEEE division: the build does not relax it (no fast-math, no approximate-div flag)
        } else {
            long long s = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) s += (long long)v[k];
            const long long num = 2 * s + n, den = 2 * n;
            long long q = num / den;
            if (num % den != 0 && num < 0) --q;         // floor
            return (T)q;
        }
    } else {
        T best = v[0];
        int best_n = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!ok[k]) continue;
            int c = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) c += (ok[j] && v[j] == v[k]);
            if (c > best_n) { best = v[k]; best_n = c; }          // strictly more: a tie stays with the earlier value
        }
        return best;
    }
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void reduce_level_kernel(RedArgs a) {
    constexpr int ES = (int)sizeof(T), VO = 16 / ES, VI = 2 * VO;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.total) return;
    const int g = (int)(idx % a.groups);
    const long long rest = idx / a.groups;
    const int y = (int)(rest % a.h);
    const long long p = rest / a.h;
    const int x0 = g * VO;                              // first output column of this thread; 2 * x0 < W
    const int ncols = min(VI, a.W - 2 * x0);            // parent columns that exist, >= 1
    const int nrows = min(2, a.H - 2 * y);              // parent rows that exist, >= 1
    const int nout = min(VO, a.w - x0);                 // output columns that exist, >= 1
    Rule<T> rule;
    rule.has = a.has_nodata;
    rule.nan_nd = a.nan_nodata;
    rule.nd = a.has_nodata ? (T)a.nodata : (T)0;

    T in[2][VI];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        if (rr < nrows) {
            const T* rowp = static_cast<const T*>(a.src) + p * a.plane_stride + (2ll * y + rr) * a.row_stride + 2 * x0;
            if (a.src_vec && ncols == VI) {
                const uint4 q0 = reinterpret_cast<const uint4*>(rowp)[0], q1 = reinterpret_cast<const uint4*>(rowp)[1];
                __builtin_memcpy(&in[rr][0], &q0, 16);
                __builtin_memcpy(&in[rr][VO], &q1, 16);
            } else {
#pragma unroll
                for (int c = 0; c < VI; ++c) in[rr][c] = c < ncols ? rowp[c] : (T)0;
            }
        } else {
#pragma unroll
            for (int c = 0; c < VI; ++c) in[rr][c] = (T)0;
        }
    }

    T out[VO];
#pragma unroll
    for (int o = 0; o < VO; ++o) {
        const T v[4] = {in[0][2 * o], in[0][2 * o + 1], in[1][2 * o], in[1][2 * o + 1]};
        const bool c0 = 2 * o < ncols, c1 = 2 * o + 1 < ncols, r1 = nrows == 2;
        const bool inside[4] = {c0, c1, c0 && r1, c1 && r1};
        out[o] = reduce_block<T, MODE>(v, inside, rule);
    }

    T* dstp = static_cast<T*>(a.dst) + (p * a.h + y) * (long long)a.w + x0;
    if (a.dst_vec && nout == VO) {
        uint4 q;
        __builtin_memcpy(&q, &out[0], 16);
        *reinterpret_cast<uint4*>(dstp) = q;
    } else {
#pragma unroll
        for (int o = 0; o < VO; ++o)
            if (o < nout) dstp[o] = out[o];
    }
}

template <typename T>
int launch_reduce(const RedArgs& a, int resampling, hipStream_t stream) {
    const dim3 grid((unsigned)((a.total + 255) / 256)), block(256);
    if (resampling == RS_NEAREST) hipLaunchKernelGGL((reduce_level_kernel<T, RS_NEAREST>), grid, block, 0, stream, a);
    else if (resampling == RS_MODE) hipLaunchKernelGGL((reduce_level_kernel<T, RS_MODE>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((reduce_level_kernel<T, RS_AVERAGE>), grid, block, 0, stream, a);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

}  // namespace

extern "C" int unet_tiff_reduce_level(const void* src, int elem_size, int kind, int P, int H, int W, long long row_stride, long long plane_stride,
                                      int resampling, int has_nodata, double nodata, void* dst, void* stream) {
    UNET_CHECK_ARG(src && dst && src != dst, "tiff_reduce_level: null pointer or dst == src");
    UNET_CHECK_ARG(elem_size == 1 || elem_size == 2 || elem_size == 4, "tiff_reduce_level: elem_size must be 1, 2 or 4 (got %d)", elem_size);
    UNET_CHECK_ARG(kind == 0 || kind == 1 || (kind == 2 && elem_size == 4),
                   "tiff_reduce_level: kind must be 0 (unsigned), 1 (signed) or 2 (float, 4 bytes) (got %d with %d bytes)", kind, elem_size);
    UNET_CHECK_ARG(resampling == RS_NEAREST || resampling == RS_AVERAGE || (resampling == RS_MODE && kind != 2),
                   "tiff_reduce_level: resampling must be 0 (nearest), 1 (mode, integers only) or 2 (average) (got %d, kind %d)", resampling, kind);
    UNET_CHECK_ARG(P >= 1 && H >= 1 && W >= 1 && (H > 1 || W > 1) && (long long)P * H * (long long)W <= (1ll << 38),
                   "tiff_reduce_level: bad image %d x %d x %d", P, H, W);
    UNET_CHECK_ARG(row_stride >= W && (P == 1 || plane_stride >= 1) && ((uintptr_t)src % elem_size) == 0 && ((uintptr_t)dst % elem_size) == 0,
                   "tiff_reduce_level: bad strides (%lld, %lld) or a misaligned pointer", row_stride, plane_stride);
    const bool nan_nd = has_nodata && nodata != nodata;
    UNET_CHECK_ARG(has_nodata == 0 || has_nodata == 1, "tiff_reduce_level: has_nodata must be 0 or 1 (got %d)", has_nodata);
    if (has_nodata && kind != 2) {
        const double lo = kind == 0 ? 0.0 : -(double)(1ll << (8 * elem_size - 1));
        const double hi = kind == 0 ? (double)((1ll << (8 * elem_size)) - 1) : (double)((1ll << (8 * elem_size - 1)) - 1);
        UNET_CHECK_ARG(!nan_nd && nodata >= lo && nodata <= hi && nodata == (double)(long long)nodata,
                       "tiff_reduce_level: nodata %g is no sample of this integer type (pass has_nodata = 0: every sample is valid)", nodata);
    }
    RedArgs a;
    a.src = src;
    a.dst = dst;
    a.row_stride = row_stride;
    a.plane_stride = P > 1 ? plane_stride : 0;
    a.H = H;
    a.W = W;
    a.h = (H + 1) / 2;
    a.w = (W + 1) / 2;
    const int vo = 16 / elem_size;
    a.groups = (a.w + vo - 1) / vo;
    a.total = (long long)P * a.h * a.groups;
    a.src_vec = aligned16(src) && (row_stride * elem_size) % 16 == 0 && (P == 1 || (plane_stride * elem_size) % 16 == 0);
    a.dst_vec = aligned16(dst) && ((long long)a.w * elem_size) % 16 == 0;
    a.has_nodata = has_nodata;
    a.nan_nodata = nan_nd ? 1 : 0;
    a.nodata = has_nodata ? nodata : 0.0;
    hipStream_t s = (hipStream_t)stream;
    if (kind == 2) return launch_reduce<float>(a, resampling, s);
    if (kind == 0) {
        if (elem_size == 1) return launch_reduce<uint8_t>(a, resampling, s);
        if (elem_size == 2) return launch_reduce<uint16_t>(a, resampling, s);
        return launch_reduce<uint32_t>(a, resampling, s);
    }
    if (elem_size == 1) return launch_reduce<int8_t>(a, resampling, s);
    if (elem_size == 2) return launch_reduce<int16_t>(a, resampling, s);
    return launch_reduce<int32_t>(a, resampling, s);
}
