// Distance to the two nearest distinct objects of a batch of class masks on the device, and the weight map of the U-Net paper in its own
// form, w0 * exp(-(d1 + d2)^2 / (2 sigma^2)) (unet_amd/border.py):
//   unet_object_edt  int32 [B, H, W] x 2: for a background pixel the smallest and the second smallest squared Euclidean distance to an
//                    object of the same image within `radius`, INT32_MAX where there is none and off the background; float [B, H, W]: the
//                    weight map.  Masks are uint8 or int64.
// Four steps on one stream, no host sync:
//   keys         int32 [B * H, W]: image << 8 | value on an object pixel, 0x80000000 | linear index on every other pixel (a key of its
//                own: such a pixel is a component by itself and costs the labelling nothing).
//   labels       unet_cc_label_keys on the stacked key image: label = smallest linear index of the object.  Images never join, their keys
//                differ.
//   column pass  per pixel the two nearest object pixels of its column with DISTINCT labels within `radius` rows of the same image, each as
//                a uint8 distance and an int32 label (-1: none), the pair of a pixel stored together.  A sweep down and a sweep up each
//                carry the last object pixel seen (A) and the last one seen with another label than A's (B); the four are merged to
//                two.  A column is cut into segments whose end states are exchanged through LDS (oe_column_kernel).  Two per column are
//                enough: if the nearest pixel of an object L in column x' is not among the column's two candidates for row y, the two
//                candidates belong to two other objects that are both at least as near to every pixel of row y as L is, so L is third
//                at best.
//   row pass     per BACKGROUND pixel a scan over x' in [x - radius, x + radius] of the two candidates per column, staged in LDS with the
//                halo, keeping the best and the best with another label of dx^2 + dy^2 <= radius^2; the scan ends once dx^2 exceeds the
//                second best.  D1, D2 and the weight are written from there.
// Integer arithmetic in the distances, no atomics (outside the labelling, whose result is canonical), every output is written by exactly
// one thread: the result does not depend on the schedule.
#include <limits.h>

#include "common.h"

using namespace unet;

namespace {

constexpr int OE_MAX = 8192, OE_MAX_R = 255;
constexpr int COL_W = 32, COL_SEGS = 32;                     // a block: 32 columns of one image in 32 row segments; 32 KiB of LDS
constexpr int ROW_W = 256, ROW_LDS = ROW_W + 2 * OE_MAX_R;    // a block: 256 pixels of one row; 766 x (8 + 2) bytes of LDS = 7.5 KiB
constexpr int OBJ = 0, BACKGROUND = 1, EXCLUDED = 2;

__device__ __forceinline__ int classify(long long v, int background, int exclude, int ncls) {
    if (v < 0 || v >= ncls || v == exclude) return EXCLUDED;
    return v == background ? BACKGROUND : OBJ;
}

// best = nearest, second = nearest with another label than best's; a label of -1 is "none".  The VALUES kept do not depend on the order
// of the offers.
struct Two {
    int d1 = INT32_MAX, l1 = -1, d2 = INT32_MAX, l2 = -1;
    __device__ __forceinline__ void offer(int d, int l) {
        if (l == l1) {
            d1 = min(d1, d);
        } else if (d < d1) {
            d2 = d1; l2 = l1;
            d1 = d; l1 = l;
        } else if (l == l2) {
            d2 = min(d2, d);
        } else if (d < d2) {
            d2 = d; l2 = l;
        }
    }
};

// the sweep's state: A = the last object pixel seen, B = the last one seen with another label than A's
struct Carry {
    int ay = -1, al = -1, by = -1, bl = -1;
    __device__ __forceinline__ void see(int y, int l) {
        if (l == al) {
            ay = y;
        } else {
            by = ay; bl = al;
            ay = y; al = l;
        }
    }
};

template <typename M>
__global__ __launch_bounds__(256) void oe_keys_kernel(const M* __restrict__ mask, long long N, long long HW, int background, int exclude,
                                                      int ncls, int32_t* __restrict__ keys) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (long long)gridDim.x * blockDim.x) {
        const long long v = (long long)mask[p];
        const unsigned k = classify(v, background, exclude, ncls) == OBJ ? ((unsigned)(p / HW) << 8) | (unsigned)v : 0x80000000u | (unsigned)p;
        keys[p] = (int32_t)k;
    }
}

// cl int2 [N], cd uint16 [N] (low byte: the first): the labels and distances of the two candidates of every pixel, nearest first.  A block owns COL_W columns of one image, cut into COL_SEGS
// row segments.  (1) Every thread reads its segment once and leaves two summaries in LDS: the state a sweep down ends in, and the state a
// sweep up ends in (the first object pixel from the top and the first with another label).  (2) The state a sweep enters a segment with is
// the fold of the summaries before it: replaying B, then A, of a segment leaves the state that replaying all of its pixels would.  (3) A
// sweep down writes the candidates from above, a sweep up merges them with those from below.
__global__ __launch_bounds__(COL_W * COL_SEGS) void oe_column_kernel(const int32_t* __restrict__ keys, const int32_t* __restrict__ labels,
                                                                     int H, int W, int R, int2* __restrict__ cl,
                                                                     uint16_t* __restrict__ cd) {
    __shared__ int4 s_down[COL_SEGS][COL_W], s_up[COL_SEGS][COL_W];
    const int lx = threadIdx.x, s = threadIdx.y;
    const int x = blockIdx.x * COL_W + lx;
    const bool active = x < W;
    const int seg = (H + COL_SEGS - 1) / COL_SEGS;
    const int y0 = min(s * seg, H), y1 = min(y0 + seg, H);
    const long long img = (long long)blockIdx.y * H * W;           // rows of other images are never read: no distance crosses a seam
    const int32_t* K = keys + img;
    const int32_t* L = labels + img;
    int2* CL = cl + img;
    uint16_t* CD = cd + img;
    Carry dn, up;
    if (active) {
#pragma unroll 4
        for (int y = y0; y < y1; ++y) {
            const long long q = (long long)y * W + x;
            if (K[q] >= 0) {
                const int l = L[q];
                dn.see(y, l);
                if (up.al < 0) {
                    up.ay = y; up.al = l;
                } else if (l != up.al && up.bl < 0) {
                    up.by = y; up.bl = l;
                }
            }
        }
    }
    s_down[s][lx] = make_int4(dn.ay, dn.al, dn.by, dn.bl);
    s_up[s][lx] = make_int4(up.ay, up.al, up.by, up.bl);
    __syncthreads();
    if (!active || y0 >= y1) return;
    Carry c;
    for (int t = 0; t < s; ++t) {
        const int4 v = s_down[t][lx];
        if (v.w >= 0) c.see(v.z, v.w);
        if (v.y >= 0) c.see(v.x, v.y);
    }
#pragma unroll 4
    for (int y = y0; y < y1; ++y) {                                // down: the candidates above and on the row
        const long long q = (long long)y * W + x;
        if (K[q] >= 0) c.see(y, L[q]);
        const bool a = c.ay >= 0 && y - c.ay <= R, b = c.by >= 0 && y - c.by <= R;
        CL[q] = make_int2(a ? c.al : -1, b ? c.bl : -1);
        CD[q] = (uint16_t)((a ? y - c.ay : 0) | (b ? y - c.by : 0) << 8);
    }
    c = Carry();
    for (int t = COL_SEGS - 1; t > s; --t) {
        const int4 v = s_up[t][lx];
        if (v.w >= 0) c.see(v.z, v.w);
        if (v.y >= 0) c.see(v.x, v.y);
    }
#pragma unroll 4
    for (int y = y1 - 1; y >= y0; --y) {                           // up: the candidates below, merged with this thread's own from above
        const long long q = (long long)y * W + x;
        if (K[q] >= 0) c.see(y, L[q]);
        Two t;
        const int2 l = CL[q];
        const int d = CD[q];
        if (l.x >= 0) t.offer(d & 255, l.x);
        if (l.y >= 0) t.offer(d >> 8, l.y);
        if (c.ay >= 0 && c.ay - y <= R) t.offer(c.ay - y, c.al);
        if (c.by >= 0 && c.by - y <= R) t.offer(c.by - y, c.bl);
        CL[q] = make_int2(t.l1, t.l2);
        CD[q] = (uint16_t)((t.l1 >= 0 ? t.d1 : 0) | (t.l2 >= 0 ? t.d2 : 0) << 8);
    }
}

template <typename M>
__global__ __launch_bounds__(ROW_W) void oe_row_kernel(const M* __restrict__ mask, const int2* __restrict__ cl, const uint16_t* __restrict__ cd,
                                                       int W, int ntx, int R, int background, int exclude, int ncls,
                                                       const float* __restrict__ class_w, float w0, double inv2s2, int32_t* __restrict__ out1,
                                                       int32_t* __restrict__ out2, float* __restrict__ pw) {
    __shared__ int2 s_l[ROW_LDS];
    __shared__ uint16_t s_d[ROW_LDS];
    const long long row = blockIdx.x / ntx;
    const int x0 = (int)(blockIdx.x % ntx) * ROW_W, x = x0 + threadIdx.x;
    const long long base = row * W;
    long long v = -1;
    int kind = EXCLUDED;
    if (x < W) {
        v = (long long)mask[base + x];
        kind = classify(v, background, exclude, ncls);
    }
    Two t;
    if (__syncthreads_or(kind == BACKGROUND)) {                    // a tile without a background pixel stages nothing
        const int n = min(ROW_W, W - x0) + 2 * R;
        for (int i = threadIdx.x; i < n; i += ROW_W) {
            const int xc = x0 - R + i;
            int2 l = make_int2(-1, -1);
            unsigned d = 0;
            if (xc >= 0 && xc < W) {
                l = cl[base + xc];
                d = cd[base + xc];
            }
            s_l[i] = l;
            s_d[i] = (uint16_t)d;
        }
        __syncthreads();
        if (kind == BACKGROUND) {
            const int R2 = R * R, c = R + threadIdx.x;
            for (int dx = 0; dx <= R; ++dx) {
                const int dx2 = dx * dx;
                if (dx2 > t.d2) break;                             // nothing farther left or right can enter the two
                for (int side = 0; side < (dx ? 2 : 1); ++side) {
                    const int i = side ? c + dx : c - dx;
                    const int2 l = s_l[i];
                    if (l.x < 0) continue;                         // no first candidate: no second one either
                    const int d = s_d[i], da = d & 255, db = d >> 8;
                    const int ea = dx2 + da * da, eb = dx2 + db * db;
                    if (ea <= R2) t.offer(ea, l.x);
                    if (l.y >= 0 && eb <= R2) t.offer(eb, l.y);
                }
            }
        }
    }
    if (x >= W) return;
    if (out1) {
        out1[base + x] = t.d1;
        out2[base + x] = t.d2;
    }
    if (pw) {
        float w = 0.f;
        if (v >= 0 && v < ncls) {
            w = class_w ? class_w[v] : 1.f;
            if (t.d2 != INT32_MAX) {
                // the exponent from the exact integers in fp64, rounded once: its error stays below the fp32 spacing at the exponent's size
                const double e = (double)(t.d1 + t.d2) + 2.0 * sqrt((double)t.d1 * (double)t.d2);
                w += w0 * expf((float)(-e * inv2s2));
            }
        }
        pw[base + x] = w;
    }
}

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

bool shape_ok(int B, int H, int W) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= OE_MAX && W <= OE_MAX && (long long)B * H * W <= 2147483647ll;
}

}  // namespace

extern "C" size_t unet_object_edt_workspace(int B, int H, int W) {
    if (!shape_ok(B, H, W)) return 0;
    const size_t N = (size_t)B * H * W;
    return 2 * up16(4 * N) + up16(8 * N) + up16(2 * N) + 16;      // keys, labels, candidate labels, candidate distances, counters
}

extern "C" int unet_object_edt(const void* mask, int mask_is_int64, int B, int H, int W, int background, int exclude, int n_classes, int radius,
                               void* workspace, int32_t* d1, int32_t* d2, const float* class_w, float w0, double sigma, float* pw,
                               void* stream) {
    UNET_CHECK_ARG(mask && workspace && (d1 || pw) && (d1 != nullptr) == (d2 != nullptr), "object_edt: null pointer (needs d1 and d2, pw, or all)");
    UNET_CHECK_ARG(shape_ok(B, H, W), "object_edt: needs 1 <= B <= 65535, 1 <= H, W <= 8192 and B * H * W <= 2^31 - 1 (got %d x %d x %d)", B, H, W);
    UNET_CHECK_ARG(n_classes >= 1 && n_classes <= 256, "object_edt: n_classes must be 1..256 (got %d)", n_classes);
    UNET_CHECK_ARG(background >= 0 && background <= 255, "object_edt: background must be a class id 0..255 (got %d)", background);
    UNET_CHECK_ARG(exclude >= -1 && exclude != background, "object_edt: exclude must be -1 (none) or a class id other than background (got %d)", exclude);
    UNET_CHECK_ARG(radius >= 1 && radius <= OE_MAX_R, "object_edt: radius must be 1..255 (got %d)", radius);
    UNET_CHECK_ARG(aligned16(workspace), "object_edt: the workspace must be 16-byte aligned");
    UNET_CHECK_ARG(!pw || (w0 >= 0.f && sigma > 0.0), "object_edt: needs w0 >= 0 and sigma > 0 (got %g, %g)", (double)w0, sigma);
    hipStream_t st = (hipStream_t)stream;
    const long long N = (long long)B * H * W;
    char* ws = (char*)workspace;
    int32_t* keys = (int32_t*)ws;
    int32_t* labels = (int32_t*)(ws + up16(4 * (size_t)N));
    int2* cl = (int2*)(ws + 2 * up16(4 * (size_t)N));
    uint16_t* cd = (uint16_t*)(ws + 2 * up16(4 * (size_t)N) + up16(8 * (size_t)N));
    int32_t* counters = (int32_t*)((char*)cd + up16(2 * (size_t)N));
    if (mask_is_int64)
        hipLaunchKernelGGL(oe_keys_kernel<int64_t>, dim3(ew_grid(N, 256)), dim3(256), 0, st, (const int64_t*)mask, N, (long long)H * W, background,
                           exclude, n_classes, keys);
    else
        hipLaunchKernelGGL(oe_keys_kernel<uint8_t>, dim3(ew_grid(N, 256)), dim3(256), 0, st, (const uint8_t*)mask, N, (long long)H * W, background,
                           exclude, n_classes, keys);
    UNET_CHECK_LAUNCH();
    const int rc = unet_cc_label_keys((const uint32_t*)keys, B * H, W, labels, counters, stream);
    if (rc != UNET_OK) return rc;
    hipLaunchKernelGGL(oe_column_kernel, dim3(cdiv(W, COL_W), B), dim3(COL_W, COL_SEGS), 0, st, keys, labels, H, W, radius, cl, cd);
    UNET_CHECK_LAUNCH();
    const int ntx = cdiv(W, ROW_W);
    const double inv2s2 = pw ? 1.0 / (2.0 * sigma * sigma) : 0.0;
    const dim3 rgrid((unsigned)((long long)ntx * B * H));
    if (mask_is_int64)
        hipLaunchKernelGGL(oe_row_kernel<int64_t>, rgrid, dim3(ROW_W), 0, st, (const int64_t*)mask, cl, cd, W, ntx, radius, background, exclude,
                           n_classes, class_w, w0, inv2s2, d1, d2, pw);
    else
        hipLaunchKernelGGL(oe_row_kernel<uint8_t>, rgrid, dim3(ROW_W), 0, st, (const uint8_t*)mask, cl, cd, W, ntx, radius, background, exclude,
                           n_classes, class_w, w0, inv2s2, d1, d2, pw);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
