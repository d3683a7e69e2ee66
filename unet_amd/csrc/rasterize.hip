// Polygon rings burnt into a class mask on the device (unet_amd/rasterize.py): the pixel centre decides, the fill is even-odd
// per feature, the feature with the highest index wins.  Vertices are int32 fixed point with 8 fractional bits.
//   unet_ras_count     per edge (vertex i -> the next vertex of its ring): the row centres it crosses after clipping to 0 .. H - 1
//   unet_ras_scan      exclusive scan of those counts in int64; the total goes to info[0]
//   unet_ras_emit      per edge: its crossings as keys feature << 40 | row << 20 | k, k = the first column whose centre lies at or right of it
//   unet_ras_spans     sorted keys 2j, 2j + 1 bound one span of one (feature, row): atomicMax of (feature + 1) << 8 | value into the plane
//   unet_ras_resolve   out = word ? word & 255 : (what out held, or fill)
//   unet_ras_resolve_ids  ids = word ? (word >> 8) - 1 : -1: the feature that owns the pixel (unet_amd/zonal.py)
// The sort between emit and spans is the caller's (one torch.sort).  Every position a kernel writes is computed (the scan) or clamped
// (rows to 0 .. H - 1, columns to 0 .. W) and compared with the size of its buffer; the only atomic is a maximum of integers, which does
// not depend on the order of arrival.
#include "common.h"

using namespace unet;

namespace {

constexpr int RAS_MAX_SIDE = 1 << 20;                 // H, W < 2^20: row and column fit the 20-bit fields of a key
constexpr int RAS_MAX_COORD = 1 << 29;                // |X|, |Y| <= 2^21 px in 1/256 px: every product below stays under 2^60
constexpr long long RAS_MAX_FEATURES = 1LL << 23;     // (feature + 1) << 8 fits the uint32 word of the plane
constexpr long long RAS_MAX_COUNT = 2147483647LL;
constexpr int SCAN_T = 256, SCAN_PER = 8, SCAN_CHUNK = SCAN_T * SCAN_PER;

struct Edge { int X0, Y0, X1, Y1, ring; };

// the edge that starts at vertex i: false for the vertices of rings with fewer than 3 vertices and wherever the CSR does not hold i
__device__ __forceinline__ bool edge_of(const int* __restrict__ xy, const long long* __restrict__ ring_start, const int* __restrict__ vring,
                                        long long i, long long V, long long R, Edge& e) {
    const int r = vring[i];
    if (r < 0 || r >= R) return false;
    const long long s = ring_start[r], t = ring_start[r + 1];
    if (s < 0 || t > V || i < s || i >= t || t - s < 3) return false;
    const long long j = i + 1 == t ? s : i + 1;
    const int2 a = reinterpret_cast<const int2*>(xy)[i], b = reinterpret_cast<const int2*>(xy)[j];
    e.X0 = a.x; e.Y0 = a.y; e.X1 = b.x; e.Y1 = b.y; e.ring = r;
    return true;
}

// the rows y with min(Y0, Y1) <= 256 y + 128 < max(Y0, Y1), clipped to 0 .. H - 1: [ylo, yhi), empty for horizontal edges
__device__ __forceinline__ void row_range(int Y0, int Y1, int H, int& ylo, int& yhi) {
    const long long lo = Y0 < Y1 ? Y0 : Y1, hi = Y0 < Y1 ? Y1 : Y0;
    const long long a = (lo + 127) >> 8, b = (hi + 127) >> 8;          // ceil((v - 128) / 256): >> is a floor division
    ylo = (int)(a < 0 ? 0 : a > H ? H : a);
    yhi = (int)(b < 0 ? 0 : b > H ? H : b);
}

__device__ __forceinline__ bool coord_ok(int v) { return v >= -RAS_MAX_COORD && v <= RAS_MAX_COORD; }

__global__ __launch_bounds__(256) void ras_count_kernel(const int* __restrict__ xy, const long long* __restrict__ ring_start,
                                                        const int* __restrict__ vring, long long V, long long R, int H,
                                                        int* __restrict__ counts, unsigned long long* __restrict__ info) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        const int2 own = reinterpret_cast<const int2*>(xy)[i];
        unsigned long long bad = (coord_ok(own.x) && coord_ok(own.y)) ? 0ull : 1ull;
        const int r = vring[i];
        if (r < 0 || r >= R) bad |= 2ull;
        else {
            const long long s = ring_start[r], t = ring_start[r + 1];
            if (s < 0 || t > V || i < s || i >= t) bad |= 2ull;
        }
        int c = 0;
        Edge e;
        if (!bad && edge_of(xy, ring_start, vring, i, V, R, e)) {
            int ylo, yhi;
            row_range(e.Y0, e.Y1, H, ylo, yhi);
            c = yhi > ylo ? yhi - ylo : 0;
        }
        counts[i] = c;
        if (bad) atomicOr(info + 1, bad);
    }
}

// ------------------------------------------------------------------------------------------------------------------ scan

__device__ __forceinline__ long long scan_load(const int* __restrict__ in, long long i0, long long n, bool vec, int v[SCAN_PER]) {
    if (vec && i0 + SCAN_PER <= n) {
        const int4 a = *reinterpret_cast<const int4*>(in + i0), b = *reinterpret_cast<const int4*>(in + i0 + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        for (int j = 0; j < SCAN_PER; ++j) v[j] = i0 + j < n ? in[i0 + j] : 0;
    }
    long long s = 0;
    for (int j = 0; j < SCAN_PER; ++j) s += v[j];
    return s;
}

// the inclusive scan of one value per thread over the block, in LDS
__device__ __forceinline__ long long block_scan(long long own, long long* sh) {
    sh[threadIdx.x] = own;
    __syncthreads();
    for (int d = 1; d < SCAN_T; d <<= 1) {
        const long long add = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    return sh[threadIdx.x];
}

__global__ __launch_bounds__(SCAN_T) void ras_scan_reduce_kernel(const int* __restrict__ in, long long n, int vec, long long* __restrict__ bsum) {
    __shared__ long long sh[SCAN_T];
    const long long i0 = (long long)blockIdx.x * SCAN_CHUNK + (long long)threadIdx.x * SCAN_PER;
    int v[SCAN_PER];
    const long long own = i0 < n ? scan_load(in, i0, n, vec != 0, v) : 0;
    block_scan(own, sh);
    if (threadIdx.x == 0) bsum[blockIdx.x] = sh[SCAN_T - 1];
}

// one block: bsum[0 .. nb) becomes its exclusive scan, *total the sum
__global__ __launch_bounds__(1024) void ras_scan_blocks_kernel(long long* __restrict__ bsum, int nb, long long* __restrict__ total) {
    __shared__ long long sh[1024];
    __shared__ long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nb; base += 1024) {
        const int i = base + threadIdx.x;
        const long long own = i < nb ? bsum[i] : 0;
        sh[threadIdx.x] = own;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const long long add = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        const long long c = carry;
        if (i < nb) bsum[i] = c + sh[threadIdx.x] - own;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(SCAN_T) void ras_scan_apply_kernel(const int* __restrict__ in, long long n, int vec, int vec_out,
                                                                const long long* __restrict__ bsum, long long* __restrict__ out) {
    __shared__ long long sh[SCAN_T];
    const long long i0 = (long long)blockIdx.x * SCAN_CHUNK + (long long)threadIdx.x * SCAN_PER;
    int v[SCAN_PER] = {0, 0, 0, 0, 0, 0, 0, 0};
    const long long own = i0 < n ? scan_load(in, i0, n, vec != 0, v) : 0;
    const long long incl = block_scan(own, sh);
    if (i0 >= n) return;
    long long run = bsum[blockIdx.x] + incl - own;
    long long o[SCAN_PER];
    for (int j = 0; j < SCAN_PER; ++j) {
        o[j] = run;
        run += v[j];
    }
    if (vec_out && i0 + SCAN_PER <= n) {
        longlong2* q = reinterpret_cast<longlong2*>(out + i0);
        for (int j = 0; j < SCAN_PER / 2; ++j) q[j] = make_longlong2(o[2 * j], o[2 * j + 1]);
    } else {
        for (int j = 0; j < SCAN_PER; ++j)
            if (i0 + j < n) out[i0 + j] = o[j];
    }
}

// ------------------------------------------------------------------------------------------------------------------ crossings

// k = ceil((X* - 128) / 256) for X* = X0 + (Yc - Y0)(X1 - X0) / (Y1 - Y0), clamped to 0 .. W: an int64 floor division on a positive
// denominator.  |Yc - Y0| <= |Y1 - Y0| <= 2^30 and |X1 - X0| <= 2^30, so the numerator stays under 2^61.
__device__ __forceinline__ long long crossing_column(const Edge& e, int y, int W) {
    long long k;
    if (e.X0 == e.X1) {
        k = ((long long)e.X0 + 127) >> 8;
    } else {
        long long d = (long long)e.Y1 - e.Y0;
        long long num = (256LL * y + 128 - e.Y0) * ((long long)e.X1 - e.X0);
        if (d < 0) {
            d = -d;
            num = -num;
        }
        const long long a = -(((long long)e.X0 - 128) * d + num), D = 256 * d;          // ceil(N / D) = -floor(-N / D)
        long long q = a / D;
        if (a % D < 0) --q;
        k = -q;
    }
    return k < 0 ? 0 : k > W ? W : k;
}

__global__ __launch_bounds__(256) void ras_emit_kernel(const int* __restrict__ xy, const long long* __restrict__ ring_start,
                                                       const int* __restrict__ vring, const int* __restrict__ ring_feature, long long V,
                                                       long long R, int H, int W, const long long* __restrict__ offs, long long M,
                                                       long long* __restrict__ keys) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        Edge e;
        if (!edge_of(xy, ring_start, vring, i, V, R, e)) continue;
        int ylo, yhi;
        row_range(e.Y0, e.Y1, H, ylo, yhi);
        if (yhi <= ylo) continue;
        const long long f = ring_feature[e.ring];
        const bool known = f >= 0 && f < RAS_MAX_FEATURES;          // else a negative key: it breaks the pairing, which the span pass reports
        long long o = offs[i];
        for (int y = ylo; y < yhi; ++y, ++o) {
            if (o < 0 || o >= M) continue;
            keys[o] = known ? (f << 40 | (long long)y << 20 | crossing_column(e, y, W)) : -1;
        }
    }
}

// one wavefront per pair of sorted keys
__global__ __launch_bounds__(256) void ras_spans_kernel(const long long* __restrict__ keys, long long pairs, const uint8_t* __restrict__ values,
                                                        long long F, int H, int W, unsigned* __restrict__ plane,
                                                        unsigned long long* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const long long nw = (long long)gridDim.x * 4;
    unsigned long long wrong = 0;
    for (long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); j < pairs; j += nw) {
        const longlong2 ab = reinterpret_cast<const longlong2*>(keys)[j];
        const long long a = ab.x, b = ab.y;
        const long long f = a >> 40;
        const int y = (int)((a >> 20) & 0xFFFFF), k0 = (int)(a & 0xFFFFF), k1 = (int)(b & 0xFFFFF);
        if (a < 0 || ((a ^ b) >> 20) != 0 || f >= F || y >= H || k1 > W || k0 > k1) {
            ++wrong;
            continue;
        }
        const unsigned word = (unsigned)(f + 1) << 8 | values[f];
        unsigned* row = plane + (long long)y * W;
        for (int x = k0 + lane; x < k1; x += 64) atomicMax(row + x, word);
    }
    if (lane == 0 && wrong) atomicAdd(bad, wrong);
}

__device__ __forceinline__ unsigned resolve4(uint4 p, unsigned old) {
    unsigned r = 0;
    r |= (p.x ? p.x & 255u : old & 255u);
    r |= (p.y ? p.y & 255u : (old >> 8) & 255u) << 8;
    r |= (p.z ? p.z & 255u : (old >> 16) & 255u) << 16;
    r |= (p.w ? p.w & 255u : (old >> 24) & 255u) << 24;
    return r;
}

// 16 pixels per thread: four 16-byte loads of the plane, one 16-byte load (keep) and one 16-byte store of out
__global__ __launch_bounds__(256) void ras_resolve_kernel(const unsigned* __restrict__ plane, long long n, unsigned fill, int keep, int vec,
                                                          uint8_t* __restrict__ out) {
    const long long groups = (n + 15) / 16;
    const unsigned fill4 = fill * 0x01010101u;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        const long long i0 = g * 16;
        if (vec && i0 + 16 <= n) {
            const uint4* p = reinterpret_cast<const uint4*>(plane + i0);
            uint4 old = make_uint4(fill4, fill4, fill4, fill4);
            if (keep) old = *reinterpret_cast<const uint4*>(out + i0);
            uint4 r;
            r.x = resolve4(p[0], old.x);
            r.y = resolve4(p[1], old.y);
            r.z = resolve4(p[2], old.z);
            r.w = resolve4(p[3], old.w);
            *reinterpret_cast<uint4*>(out + i0) = r;
        } else {
            for (long long i = i0; i < i0 + 16 && i < n; ++i) {
                const unsigned w = plane[i];
                out[i] = (uint8_t)(w ? w & 255u : keep ? out[i] : fill);
            }
        }
    }
}

__device__ __forceinline__ int id_of(unsigned w) { return w ? (int)(w >> 8) - 1 : -1; }

// 4 pixels per thread: one 16-byte load of the plane, one 16-byte store of ids
__global__ __launch_bounds__(256) void ras_resolve_ids_kernel(const unsigned* __restrict__ plane, long long n, int vec, int* __restrict__ ids) {
    const long long groups = (n + 3) / 4;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        const long long i0 = g * 4;
        if (vec && i0 + 4 <= n) {
            const uint4 p = *reinterpret_cast<const uint4*>(plane + i0);
            *reinterpret_cast<int4*>(ids + i0) = make_int4(id_of(p.x), id_of(p.y), id_of(p.z), id_of(p.w));
        } else {
            for (long long i = i0; i < i0 + 4 && i < n; ++i) ids[i] = id_of(plane[i]);
        }
    }
}

bool side_ok(int H, int W) { return H >= 1 && W >= 1 && H < RAS_MAX_SIDE && W < RAS_MAX_SIDE; }
bool count_ok(long long v) { return v >= 1 && v <= RAS_MAX_COUNT; }
bool aligned8(const void* p) { return (((uintptr_t)p) & 7) == 0; }

}  // namespace

extern "C" int unet_ras_count(const int32_t* xy, const long long* ring_start, const int32_t* vring, long long V, long long R, int H,
                              int32_t* counts, long long* info, void* stream) {
    UNET_CHECK_ARG(xy && ring_start && vring && counts && info, "ras_count: null pointer");
    UNET_CHECK_ARG(count_ok(V) && count_ok(R) && H >= 1 && H < RAS_MAX_SIDE, "ras_count: V, R must be in 1..2^31 - 1 and H in 1..2^20 - 1 (got %lld, %lld, %d)",
                   V, R, H);
    UNET_CHECK_ARG(aligned8(xy), "ras_count: xy must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    UNET_CHECK_HIP(hipMemsetAsync(info, 0, 2 * sizeof(long long), st));
    hipLaunchKernelGGL(ras_count_kernel, dim3(ew_grid(V, 256)), dim3(256), 0, st, xy, ring_start, vring, V, R, H, counts,
                       reinterpret_cast<unsigned long long*>(info));
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" long long unet_ras_scan_words(long long n) { return n < 1 ? 1 : (n + SCAN_CHUNK - 1) / SCAN_CHUNK; }

extern "C" int unet_ras_scan(const int32_t* counts, long long n, long long* offs, long long* blocks, long long* info, void* stream) {
    UNET_CHECK_ARG(counts && offs && blocks && info, "ras_scan: null pointer");
    UNET_CHECK_ARG(count_ok(n), "ras_scan: n must be in 1..2^31 - 1 (got %lld)", n);
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)unet_ras_scan_words(n);
    const int vec = aligned16(counts) ? 1 : 0, vec_out = aligned16(offs) ? 1 : 0;
    hipLaunchKernelGGL(ras_scan_reduce_kernel, dim3(nb), dim3(SCAN_T), 0, st, counts, n, vec, blocks);
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(ras_scan_blocks_kernel, dim3(1), dim3(1024), 0, st, blocks, nb, info);
    UNET_CHECK_LAUNCH();
    hipLaunchKernelGGL(ras_scan_apply_kernel, dim3(nb), dim3(SCAN_T), 0, st, counts, n, vec, vec_out, blocks, offs);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_ras_emit(const int32_t* xy, const long long* ring_start, const int32_t* vring, const int32_t* ring_feature, long long V,
                             long long R, int H, int W, const long long* offs, long long M, long long* keys, void* stream) {
    UNET_CHECK_ARG(xy && ring_start && vring && ring_feature && offs && keys, "ras_emit: null pointer");
    UNET_CHECK_ARG(count_ok(V) && count_ok(R) && count_ok(M) && side_ok(H, W),
                   "ras_emit: V, R, M must be in 1..2^31 - 1 and H, W in 1..2^20 - 1 (got %lld, %lld, %lld, %d x %d)", V, R, M, H, W);
    UNET_CHECK_ARG(aligned8(xy), "ras_emit: xy must be 8-byte aligned");
    hipLaunchKernelGGL(ras_emit_kernel, dim3(ew_grid(V, 256)), dim3(256), 0, (hipStream_t)stream, xy, ring_start, vring, ring_feature, V, R, H, W,
                       offs, M, keys);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_ras_spans(const long long* keys, long long M, const uint8_t* values, long long F, int H, int W, uint32_t* plane,
                              long long* bad, void* stream) {
    UNET_CHECK_ARG(plane && bad && (M == 0 || (keys && values)), "ras_spans: null pointer");
    UNET_CHECK_ARG(M >= 0 && M <= RAS_MAX_COUNT && M % 2 == 0 && F >= 0 && F < RAS_MAX_FEATURES && (M == 0 || F >= 1) && side_ok(H, W),
                   "ras_spans: M must be even in 0..2^31 - 1, F under 2^23 and H, W in 1..2^20 - 1 (got %lld, %lld, %d x %d)", M, F, H, W);
    UNET_CHECK_ARG(M == 0 || aligned16(keys), "ras_spans: keys must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    UNET_CHECK_HIP(hipMemsetAsync(plane, 0, (size_t)H * (size_t)W * sizeof(uint32_t), st));
    UNET_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(long long), st));
    if (M == 0) return UNET_OK;
    hipLaunchKernelGGL(ras_spans_kernel, dim3(ew_grid(M / 2 * 64, 256)), dim3(256), 0, st, keys, M / 2, values, F, H, W, plane,
                       reinterpret_cast<unsigned long long*>(bad));
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_ras_resolve(const uint32_t* plane, int H, int W, int fill, int keep, uint8_t* out, void* stream) {
    UNET_CHECK_ARG(plane && out, "ras_resolve: null pointer");
    UNET_CHECK_ARG(side_ok(H, W) && fill >= 0 && fill <= 255, "ras_resolve: H, W must be in 1..2^20 - 1 and fill in 0..255 (got %d x %d, %d)", H, W, fill);
    const long long n = (long long)H * W;
    const int vec = aligned16(plane) && aligned16(out) ? 1 : 0;
    hipLaunchKernelGGL(ras_resolve_kernel, dim3(ew_grid((n + 15) / 16, 256)), dim3(256), 0, (hipStream_t)stream, plane, n, (unsigned)fill, keep ? 1 : 0,
                       vec, out);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_ras_resolve_ids(const uint32_t* plane, int H, int W, int32_t* ids, void* stream) {
    UNET_CHECK_ARG(plane && ids, "ras_resolve_ids: null pointer");
    UNET_CHECK_ARG(side_ok(H, W), "ras_resolve_ids: H, W must be in 1..2^20 - 1 (got %d x %d)", H, W);
    const long long n = (long long)H * W;
    const int vec = aligned16(plane) && aligned16(ids) ? 1 : 0;
    hipLaunchKernelGGL(ras_resolve_ids_kernel, dim3(ew_grid((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, plane, n, vec, ids);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
