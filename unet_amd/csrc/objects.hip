// Per-object attributes of a label image (unet_amd/objects.py, DESIGN 3.23, where the rules are): a keyed reduction over the label plane.
//   unet_obj_point_packed  whether the representative pixel of an H x W raster is found in one pass (the key fits 64 bits)
//   unet_obj_compact       label[k], cls[k] of object k from the anchor marks and their exclusive scan
//   unet_obj_accumulate    sums[k] = (pixels, sum_x, sum_y, edges_v, edges_h), bbox[k] = (x0, y0, x1, y1) half open
//   unet_obj_point         point[k] = the pixel of object k nearest to its floored centroid, ties to the smallest index
// The planes are one flat run of n = H * W pixels.  A lane owns 4 consecutive pixels per step (one 16-byte load of the labels, one 4-byte
// load of the mask), a wavefront 256, and it walks ONE contiguous span of the plane.  The key of a pixel is (label, mask value); a run is a
// stretch of one key inside one row, and only the head of a run touches the tables:
//   - a lane whose 4 pixels hold one key in one row, and whose left neighbour lane does too with the same key in the same row, is no head;
//     the head of such a run of lanes (a ballot and a find-first-set give its length) owns 4 * len pixels from its own column on, so the
//     count, the column and row sums and the extent are closed forms, and the edge counts of the run come from one wave-wide inclusive scan;
//   - a lane with several keys, a row end, or the ragged end of the plane walks its pixels one by one and flushes every stretch;
//   - a step whose 256 pixels are one run joins a pending run that the wave carries in registers (the background: one address would
//     otherwise take every add).  The accumulation carries it across rows, the point passes only along one row.
// A flush of the accumulation reads labels[L], mask[L] and offs[L] at the run's label L (three independent loads) -- this is the check of
// the input: L outside 0 .. n - 1 (bit 0 of *bad), labels[L] != L (bit 1), mask[L] != the run's mask value (bit 2); such a run is dropped.
// offs[L], the object's index, is below P because L is an anchor of a kept class.  So nothing is stored outside the tables whatever the
// planes hold; the point passes read *bad first and do nothing when a bit is set.  Accumulation: five 64-bit adds and four 32-bit minima /
// maxima, the latter only where a plain read of the extent says they would change it (a stale read costs one atomic more, never one less:
// minima only fall); the point passes read the current key the same way and skip the minimum that cannot win.  Edges are per pixel: the left / right (edges_v) and upper / lower (edges_h) neighbour has
// another LABEL or lies outside the raster; the upper and lower labels are two more reads of the label plane one row away.
// The point: a run x0 .. x1 of row y offers the pixel (clamp(cx, x0, x1), y), its nearest to (cx, cy) = (sum_x / pixels, sum_y / pixels)
// and on a tie the smaller column cannot lie in the run without cx itself.  One pass takes the minimum of d2 << 31 | index where
// (H - 1)^2 + (W - 1)^2 < 2^33; otherwise one pass takes the minimum of d2 and a second the minimum index among the pixels that reach it.
// Where a base pointer is not aligned for the wide loads, and on the last n % 4 pixels, a lane loads its pixels one by one: no access
// touches a byte outside the n elements.  Every accumulation is an integer add, minimum or maximum: the tables do not depend on the order.
#include "common.h"

using namespace unet;

namespace {

constexpr int OBJ_MAX_SIDE = 1 << 20;
constexpr int OT = 256, OWAVES = OT / 64;
constexpr int OBJ_MAX_GRID = 1024;                    // 4 workgroups per CU, as zonal_counts
constexpr unsigned long long OBJ_PACKED_D2 = 1ull << 33;          // d2 << 31 | index fits 64 bits below this

enum { ACCUMULATE = 0, POINT_PACKED = 1, POINT_DIST = 2, POINT_INDEX = 3 };

struct ClassSet { uint32_t w[8]; };

__device__ __forceinline__ bool in_set(const ClassSet& s, unsigned c) { return (s.w[(c >> 5) & 7] >> (c & 31)) & 1u; }

struct Planes {
    const uint8_t* mask;
    const int* labels;
    const int* offs;
    long long n;
    int W, P;
    ClassSet exclude;
};

struct Tables {
    unsigned long long* sums;          // [P, 5]
    int* bbox;                         // [P, 4]
    unsigned long long* key64;         // [P]
    int* point;                        // [P]
};

struct Run {                           // a stretch of pixels of one key; the extent is inclusive
    int label;
    unsigned cls;
    unsigned long long cnt, sx, sy, ev, eh;
    int x0, x1, y0, y1;
};

template <int MODE>
__device__ void obj_flush(const Planes& pl, const Tables& tb, const Run& r, unsigned& badbits) {
    const long long L = r.label;
    if (L < 0 || L >= pl.n) { badbits |= 1u; return; }
    if (MODE == ACCUMULATE) {
        const int anchor = pl.labels[L];                  // three independent loads: one round trip
        const unsigned cls = pl.mask[L];
        const int k = pl.offs[L];
        if (anchor != r.label) { badbits |= 2u; return; }
        if (cls != r.cls) { badbits |= 4u; return; }
        if (in_set(pl.exclude, r.cls)) return;
        if ((unsigned)k >= (unsigned)pl.P) return;          // cannot happen: L is an anchor of a kept class
        int* b = tb.bbox + 4ll * k;
        const int b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];          // a stale value errs on the side of one atomic more: minima only fall
        unsigned long long* s = tb.sums + 5ll * k;
        atomicAdd(s, r.cnt);
        atomicAdd(s + 1, r.sx);
        atomicAdd(s + 2, r.sy);
        if (r.ev) atomicAdd(s + 3, r.ev);
        if (r.eh) atomicAdd(s + 4, r.eh);
        if (r.x0 < b0) atomicMin(b, r.x0);
        if (r.y0 < b1) atomicMin(b + 1, r.y0);
        if (r.x1 + 1 > b2) atomicMax(b + 2, r.x1 + 1);
        if (r.y1 + 1 > b3) atomicMax(b + 3, r.y1 + 1);
    } else {          // the input passed the check of the accumulation (the kernel returns otherwise); r is x0 .. x1 of row y0
        if (in_set(pl.exclude, r.cls)) return;
        const int k = pl.offs[L];
        if ((unsigned)k >= (unsigned)pl.P) return;
        const unsigned long long* s = tb.sums + 5ll * k;
        const unsigned long long px = s[0], sx = s[1], sy = s[2];
        const unsigned long long seen = tb.key64[k];          // stale at worst: it only falls
        const int seen_point = MODE == POINT_INDEX ? tb.point[k] : 0;
        if (px == 0) return;
        const long long cx = (long long)(sx / px), cy = (long long)(sy / px);
        const long long x = cx < r.x0 ? r.x0 : cx > r.x1 ? r.x1 : cx;
        const long long dx = x - cx, dy = r.y0 - cy;
        const unsigned long long d2 = (unsigned long long)(dx * dx + dy * dy);
        const unsigned long long p = (unsigned long long)((long long)r.y0 * pl.W + x);
        if (MODE == POINT_PACKED) {
            if ((d2 << 31 | p) < seen) atomicMin(tb.key64 + k, d2 << 31 | p);
        } else if (MODE == POINT_DIST) {
            if (d2 < seen) atomicMin(tb.key64 + k, d2);
        } else if (seen == d2 && (int)p < seen_point) {
            atomicMin(tb.point + k, (int)p);
        }
    }
}

// span: the groups of 4 pixels that one wavefront walks, a multiple of 64 (one group per lane and step)
template <int MODE>
__global__ __launch_bounds__(OT) void obj_walk_kernel(Planes pl, Tables tb, long long span, int vec, int vec_rows, unsigned long long* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const long long n = pl.n;
    const unsigned W = (unsigned)pl.W;
    const int* __restrict__ labels = pl.labels;
    const long long groups = (n + 3) / 4;
    const long long wave = (long long)blockIdx.x * OWAVES + (threadIdx.x >> 6);
    const long long first = wave * span;
    const long long last = first + span < groups ? first + span : groups;
    if (MODE != ACCUMULATE && *bad) return;           // the point passes rely on the check that the accumulation made
    unsigned badbits = 0;
    Run pend;                                         // the same in all lanes of the wave
    bool has_pend = false;
    for (long long g0 = first; g0 < last; g0 += 64) {
        const long long g = g0 + lane, i0 = g * 4;
        const bool active = g < last;                 // then i0 < n
        const bool whole = active && i0 + 4 <= n;
        int l[4] = {-1, -1, -1, -1};
        unsigned m[4] = {0, 0, 0, 0};
        if (whole && vec) {
            const int4 ll = *reinterpret_cast<const int4*>(labels + i0);
            const unsigned mm = *reinterpret_cast<const unsigned*>(pl.mask + i0);
            l[0] = ll.x; l[1] = ll.y; l[2] = ll.z; l[3] = ll.w;
            m[0] = mm & 255u; m[1] = (mm >> 8) & 255u; m[2] = (mm >> 16) & 255u; m[3] = mm >> 24;
        } else if (active) {
            for (int j = 0; j < 4; ++j)
                if (i0 + j < n) {
                    l[j] = labels[i0 + j];
                    m[j] = pl.mask[i0 + j];
                }
        }
        unsigned x0 = 0, y0 = 0;
        if (active) {
            y0 = (unsigned)i0 / W;
            x0 = (unsigned)i0 - y0 * W;
        }
        // the edges of every pixel, accumulation only
        unsigned ev[4] = {0, 0, 0, 0}, eh[4] = {0, 0, 0, 0};
        if (MODE == ACCUMULATE) {
            int leftn = __shfl_up(l[3], 1), rightn = __shfl_down(l[0], 1);
            if (lane == 0) leftn = (active && i0 > 0) ? labels[i0 - 1] : -1;
            if (lane == 63) rightn = (active && i0 + 4 < n) ? labels[i0 + 4] : -1;
            int up[4] = {-1, -1, -1, -1}, dn[4] = {-1, -1, -1, -1};
            if (whole && vec_rows) {                  // W % 4 == 0: the 4 pixels lie in one row, and so do the 4 above and the 4 below
                if (i0 >= (long long)W) {
                    const int4 u = *reinterpret_cast<const int4*>(labels + (i0 - W));
                    up[0] = u.x; up[1] = u.y; up[2] = u.z; up[3] = u.w;
                }
                if (i0 + W + 4 <= n) {
                    const int4 d = *reinterpret_cast<const int4*>(labels + (i0 + W));
                    dn[0] = d.x; dn[1] = d.y; dn[2] = d.z; dn[3] = d.w;
                }
            } else if (active) {
                for (int j = 0; j < 4; ++j) {
                    const long long p = i0 + j;
                    if (p < n && p >= (long long)W) up[j] = labels[p - W];
                    if (p + W < n) dn[j] = labels[p + W];
                }
            }
            unsigned x = x0;
            for (int j = 0; j < 4; ++j) {
                const long long p = i0 + j;
                if (active && p < n) {
                    const int lf = j == 0 ? leftn : l[j - 1], rt = j == 3 ? rightn : l[j + 1];
                    ev[j] = ((x == 0 || lf != l[j]) ? 1u : 0u) + ((x == W - 1 || rt != l[j]) ? 1u : 0u);
                    eh[j] = ((p < (long long)W || up[j] != l[j]) ? 1u : 0u) + ((p + W >= n || dn[j] != l[j]) ? 1u : 0u);
                }
                if (++x == W) x = 0;
            }
        }
        // runs along the lanes
        const bool same = whole && l[0] == l[1] && l[1] == l[2] && l[2] == l[3] && m[0] == m[1] && m[1] == m[2] && m[2] == m[3] && x0 + 4 <= W;
        const int left_l = __shfl_up(l[3], 1);
        const unsigned left_m = __shfl_up(m[3], 1);
        const int left_same = __shfl_up((int)same, 1);
        const bool head = lane == 0 || !same || !left_same || left_l != l[0] || left_m != m[0] || x0 == 0;
        const unsigned long long heads = __ballot(head);
        const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
        const int len = after ? __ffsll((long long)after) : 64 - lane;          // lanes up to the next head
        const unsigned mine = (ev[0] + ev[1] + ev[2] + ev[3]) | (eh[0] + eh[1] + eh[2] + eh[3]) << 16;
        unsigned scan = mine;                         // inclusive scan of (edges_v, edges_h) along the lanes: at most 512 each
        if (MODE == ACCUMULATE) {
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned t = __shfl_up(scan, d);
                if (lane >= d) scan += t;
            }
        }
        const unsigned run_edges = __shfl(scan, lane + len - 1) - scan + mine;
        if (heads == 1ull && __shfl((int)same, 0)) {          // one run over the wavefront: it joins the pending run
            const int k = __shfl(l[0], 0);
            const unsigned c = __shfl(m[0], 0);
            const unsigned X = __shfl(x0, 0), Y = __shfl(y0, 0);
            const unsigned tot = __shfl(scan, 63);
            const bool join = has_pend && pend.label == k && pend.cls == c && (MODE == ACCUMULATE || (pend.y0 == (int)Y && pend.x1 + 1 == (int)X));
            if (has_pend && !join && lane == 0) obj_flush<MODE>(pl, tb, pend, badbits);
            if (!join) {
                pend.label = k; pend.cls = c;
                pend.cnt = pend.sx = pend.sy = pend.ev = pend.eh = 0;
                pend.x0 = (int)X; pend.x1 = (int)X + 255; pend.y0 = pend.y1 = (int)Y;
                has_pend = true;
            }
            pend.cnt += 256;
            pend.sx += 256ull * X + 256ull * 255 / 2;
            pend.sy += 256ull * Y;
            pend.ev += tot & 0xffffu;
            pend.eh += tot >> 16;
            pend.x0 = min(pend.x0, (int)X); pend.x1 = max(pend.x1, (int)X + 255);
            pend.y0 = min(pend.y0, (int)Y); pend.y1 = max(pend.y1, (int)Y);
            continue;
        }
        if (MODE != ACCUMULATE && has_pend) {         // a point run is one unbroken stretch of a row
            if (lane == 0) obj_flush<MODE>(pl, tb, pend, badbits);
            has_pend = false;
        }
        if (!head || !active) continue;
        if (same) {
            Run r;
            const unsigned long long c = 4ull * len;
            r.label = l[0]; r.cls = m[0];
            r.cnt = c; r.sx = c * x0 + c * (c - 1) / 2; r.sy = c * y0;
            r.ev = run_edges & 0xffffu; r.eh = run_edges >> 16;
            r.x0 = (int)x0; r.x1 = (int)(x0 + c - 1); r.y0 = r.y1 = (int)y0;
            obj_flush<MODE>(pl, tb, r, badbits);
        } else {
            Run r;
            bool open = false;
            unsigned x = x0, y = y0;
            for (int j = 0; j < 4; ++j) {
                if (i0 + j < n) {
                    if (open && (r.label != l[j] || r.cls != m[j] || x == 0)) {
                        obj_flush<MODE>(pl, tb, r, badbits);
                        open = false;
                    }
                    if (!open) {
                        r.label = l[j]; r.cls = m[j];
                        r.cnt = r.sx = r.sy = r.ev = r.eh = 0;
                        r.x0 = (int)x; r.y0 = r.y1 = (int)y;
                        open = true;
                    }
                    r.cnt += 1; r.sx += x; r.sy += y; r.ev += ev[j]; r.eh += eh[j];
                    r.x1 = (int)x;
                }
                if (++x == W) { x = 0; ++y; }
            }
            if (open) obj_flush<MODE>(pl, tb, r, badbits);
        }
    }
    if (has_pend && lane == 0) obj_flush<MODE>(pl, tb, pend, badbits);
    if (MODE == ACCUMULATE && badbits) atomicOr(bad, (unsigned long long)badbits);
}

__global__ __launch_bounds__(OT) void obj_compact_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ mark, const int* __restrict__ offs,
                                                         long long n, long long P, int* __restrict__ label, uint8_t* __restrict__ cls) {
    for (long long p = (long long)blockIdx.x * OT + threadIdx.x; p < n; p += (long long)gridDim.x * OT)
        if (mark[p]) {
            const long long k = offs[p];
            if (k >= 0 && k < P) {
                label[k] = (int)p;
                cls[k] = mask[p];
            }
        }
}

__global__ __launch_bounds__(OT) void obj_init_tables_kernel(long long P, unsigned long long* __restrict__ sums, int* __restrict__ bbox) {
    for (long long k = (long long)blockIdx.x * OT + threadIdx.x; k < P; k += (long long)gridDim.x * OT) {
        for (int j = 0; j < 5; ++j) sums[5 * k + j] = 0;
        bbox[4 * k] = bbox[4 * k + 1] = 2147483647;
        bbox[4 * k + 2] = bbox[4 * k + 3] = 0;
    }
}

__global__ __launch_bounds__(OT) void obj_init_point_kernel(long long P, unsigned long long* __restrict__ key64, int* __restrict__ point) {
    for (long long k = (long long)blockIdx.x * OT + threadIdx.x; k < P; k += (long long)gridDim.x * OT) {
        key64[k] = ~0ull;
        point[k] = 2147483647;
    }
}

__global__ __launch_bounds__(OT) void obj_unpack_point_kernel(long long P, const unsigned long long* __restrict__ key64, int* __restrict__ point) {
    for (long long k = (long long)blockIdx.x * OT + threadIdx.x; k < P; k += (long long)gridDim.x * OT)
        point[k] = (int)(key64[k] & 0x7fffffffull);
}

struct Walk {
    int grid, vec, vec_rows;
    long long span;
};

Walk plan_walk(const uint8_t* mask, const int32_t* labels, long long n, int W) {
    Walk w;
    const long long groups = (n + 3) / 4;
    w.grid = groups > (long long)OBJ_MAX_GRID * OT ? OBJ_MAX_GRID : ew_grid(groups, OT);
    const long long waves = (long long)w.grid * OWAVES;
    w.span = ((groups + waves - 1) / waves + 63) / 64 * 64;          // grid * OWAVES * span >= groups
    w.vec = aligned16(labels) && (((uintptr_t)mask) & 3) == 0 ? 1 : 0;
    w.vec_rows = w.vec && W % 4 == 0 ? 1 : 0;
    return w;
}

bool shape_ok(int H, int W) { return H >= 1 && W >= 1 && H < OBJ_MAX_SIDE && W < OBJ_MAX_SIDE && (long long)H * W <= 2147483647LL; }

}  // namespace

extern "C" int unet_obj_point_packed(int H, int W) {
    const unsigned long long h = (unsigned long long)(H > 0 ? H - 1 : 0), w = (unsigned long long)(W > 0 ? W - 1 : 0);
    return h * h + w * w < OBJ_PACKED_D2 ? 1 : 0;
}

extern "C" int unet_obj_compact(const uint8_t* mask, const uint8_t* mark, const int32_t* offs, long long n, long long P, int32_t* label,
                                uint8_t* cls, void* stream) {
    UNET_CHECK_ARG(mask && mark && offs && label && cls, "obj_compact: null pointer");
    UNET_CHECK_ARG(n >= 1 && n <= 2147483647LL && P >= 1 && P <= n, "obj_compact: n must be in 1..2^31 - 1 and P in 1..n (got %lld, %lld)", n, P);
    hipLaunchKernelGGL(obj_compact_kernel, dim3(ew_grid(n, OT)), dim3(OT), 0, (hipStream_t)stream, mask, mark, offs, n, P, label, cls);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_obj_accumulate(const uint8_t* mask, const int32_t* labels, const int32_t* offs, int H, int W, const uint32_t* exclude8,
                                   long long P, long long* sums, int32_t* bbox, long long* bad, void* stream) {
    UNET_CHECK_ARG(mask && labels && offs && exclude8 && bad, "obj_accumulate: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W), "obj_accumulate: H, W must be in 1..2^20 - 1 and H * W at most 2^31 - 1 (got %d x %d)", H, W);
    const long long n = (long long)H * W;
    UNET_CHECK_ARG(P >= 0 && P <= n && (P == 0 || (sums && bbox)), "obj_accumulate: P must be in 0..H * W, with tables unless it is 0 (got %lld)", P);
    hipStream_t st = (hipStream_t)stream;
    UNET_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(long long), st));
    Planes pl;
    pl.mask = mask; pl.labels = labels; pl.offs = offs; pl.n = n; pl.W = W; pl.P = (int)P;
    for (int i = 0; i < 8; ++i) pl.exclude.w[i] = exclude8[i];
    Tables tb;
    tb.sums = reinterpret_cast<unsigned long long*>(sums); tb.bbox = bbox; tb.key64 = nullptr; tb.point = nullptr;
    if (P) {
        hipLaunchKernelGGL(obj_init_tables_kernel, dim3(ew_grid(P, OT)), dim3(OT), 0, st, P, tb.sums, bbox);
        UNET_CHECK_LAUNCH();
    }
    const Walk w = plan_walk(mask, labels, n, W);
    hipLaunchKernelGGL(obj_walk_kernel<ACCUMULATE>, dim3(w.grid), dim3(OT), 0, st, pl, tb, w.span, w.vec, w.vec_rows,
                       reinterpret_cast<unsigned long long*>(bad));
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_obj_point(const uint8_t* mask, const int32_t* labels, const int32_t* offs, int H, int W, const uint32_t* exclude8,
                              long long P, const long long* sums, const long long* bad, long long* key64, int32_t* point, void* stream) {
    UNET_CHECK_ARG(mask && labels && offs && exclude8 && sums && bad && key64 && point, "obj_point: null pointer");
    UNET_CHECK_ARG(shape_ok(H, W), "obj_point: H, W must be in 1..2^20 - 1 and H * W at most 2^31 - 1 (got %d x %d)", H, W);
    const long long n = (long long)H * W;
    UNET_CHECK_ARG(P >= 1 && P <= n, "obj_point: P must be in 1..H * W (got %lld)", P);
    hipStream_t st = (hipStream_t)stream;
    Planes pl;
    pl.mask = mask; pl.labels = labels; pl.offs = offs; pl.n = n; pl.W = W; pl.P = (int)P;
    for (int i = 0; i < 8; ++i) pl.exclude.w[i] = exclude8[i];
    Tables tb;
    tb.sums = reinterpret_cast<unsigned long long*>(const_cast<long long*>(sums)); tb.bbox = nullptr;
    tb.key64 = reinterpret_cast<unsigned long long*>(key64); tb.point = point;
    const Walk w = plan_walk(mask, labels, n, W);
    const dim3 pg(ew_grid(P, OT)), bt(OT);
    unsigned long long* word = reinterpret_cast<unsigned long long*>(const_cast<long long*>(bad));          // read only
    hipLaunchKernelGGL(obj_init_point_kernel, pg, bt, 0, st, P, tb.key64, point);
    UNET_CHECK_LAUNCH();
    if (unet_obj_point_packed(H, W)) {
        hipLaunchKernelGGL(obj_walk_kernel<POINT_PACKED>, dim3(w.grid), bt, 0, st, pl, tb, w.span, w.vec, 0, word);
        UNET_CHECK_LAUNCH();
        hipLaunchKernelGGL(obj_unpack_point_kernel, pg, bt, 0, st, P, tb.key64, point);
    } else {
        hipLaunchKernelGGL(obj_walk_kernel<POINT_DIST>, dim3(w.grid), bt, 0, st, pl, tb, w.span, w.vec, 0, word);
        UNET_CHECK_LAUNCH();
        hipLaunchKernelGGL(obj_walk_kernel<POINT_INDEX>, dim3(w.grid), bt, 0, st, pl, tb, w.span, w.vec, 0, word);
    }
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
