// Shared by the fp32 (conv_igemm.hip) and bf16 (conv_bf16.hip) implicit-GEMM convolution kernels of libunet_hip.so and their dispatcher
// (conv_dispatch.hip): tap tables, kernel arguments, the launch plan, the inline-asm global-load helpers of the direct-operand main loop,
// the host-side launch ladder and the launch functions of the kernel families.
// Both kernels move the SAME bytes per stage -- a reduction chunk is 64 bytes per pixel (16 fp32 or 32 bf16 channels), an LDS halo row
// is 64 + 16 pad bytes, a filter tile is 16 columns x 64 bytes = 1 KiB in MFMA operand order -- so the geometry code is common.
#pragma once
#include "common.h"

namespace unetconv {

constexpr int KC = 16;   // fp32: reduction channels per chunk
constexpr int LDK = 20;  // LDS halo row length in dwords: 64 bytes of channels + 16 bytes pad (conflict-free ds_read_b128 lane groups)
constexpr int KCB = 32;  // bf16: reduction channels per chunk (64 bytes of bf16)
// bf16 LDS halo row length in dwords: 64 bytes of channels + 32 bytes pad.  With 96-byte rows the 16 lanes of every ds_read_b128 lane group
// ({0-3,12-15,20-27}, ...: pixel rows r, 16-byte slot (6 r + kq) mod 16) hit 16 different slots -- conflict free; the 80-byte rows of
// the fp32 kernel are 2-way conflicted on 3 of 16 slots (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.5), which that MFMA-bound
// kernel hides and the bf16 one (27 % MFMA busy) does not.
constexpr int LDKB = 24;

struct TapSet {
    int n;              // number of taps
    int min_dy, min_dx; // halo origin offset (input coords relative to tile origin * S)
    int ext_y, ext_x;   // halo extent beyond (T-1)*S
    int py, px;         // output parity offsets (OS == 2)
    signed char dy[9], dx[9], widx[9];
    // the same tables packed 4 bits per tap for scalar decoding (16x16x4 kernel): dpack nibble t = (dy - min_dy) | (dx - min_dx) << 2,
    // wpack nibble t = widx
    unsigned long long dpack, wpack;
};

struct KArgs {
    const float* x; const float* wp; const float* bias; const float* res; const float* mask;
    float* y; float* colsum; float* colsumsq;
    int x_cs, x_co, res_cs, res_co, mask_cs, mask_co, y_cs, y_co;
    int N, IH, IW, Cin, Cin4;
    int OH, OW, Cout;
    int S, OS, TSH, TSW, tiles_y, tiles_x, ntn;
    int nchunks, coutPad, flags, mtiles;
    int n_base, n_end;   // produced-channel range of this launch (unet_conv_desc.cout_begin / cout_count); n_end <= Cout
    int fold;            // bf16 kernel: the reduction tail runs tap-folded (bf16_fold_tail below)
    int sliver;          // fp32 16x16x4 kernel: the last 1..4 output channels run on v_mfma_f32_4x4x1 (f32_sliver below)
    const float* wsl;    // its filter image [tap][chunk16][4][16]
    long long wp_stride; // floats between the packed filter images of consecutive batch images (0: one image for all)
    int cps;             // split-K: reduction chunks per split (blockIdx.y = split index); 0 = the whole reduction in one workgroup
    long long slab;      // split-K: elements between the partial-sum slabs of consecutive splits (y then points at slab 0)
    TapSet taps[4];
};

// ---- the fp32 packed filter image --------------------------------------------------------------------------------
// wp[tap][chunk16][outPad][16] (a reduction tail stored channel-transposed, see pack_weights_kernel), and for an output width that
// leaves 1..4 channels beyond a multiple of 16 (100 = 6 * 16 + 4) a SLIVER image behind it: wsl[tap][chunk16][4][16] holds the
// filters of those channels, position p of a 16-float row = reduction channel p of the chunk (tail chunk: the same transposition
// as the main image, channel 4 (p % 4) + p / 4).  conv_igemm16_kernel<.,2,2,2,2,4> multiplies them with v_mfma_f32_4x4x1_16B_f32
// (64 pixels x 4 channels per instruction at the FLOP rate of the 16x16x4 form) instead of paying a seventh 16-wide tile for 4 of
// its 16 columns.
__host__ __device__ inline bool f32_sliver(int out) { return out >= 16 && (out & 15) != 0 && (out & 15) <= 4; }
__host__ __device__ inline size_t f32_image_elems(int red, int out, int T) {
    const int nchunks = (red + 15) / 16, outPad = (out + 127) / 128 * 128;
    return (size_t)T * nchunks * outPad * 16 + (f32_sliver(out) ? (size_t)T * nchunks * 64 : 0);
}
// element i of the sliver image (i counted from its start); same (w, Cout, Cin, T, mode) convention as bf16_image_value
__device__ inline float f32_sliver_value(const float* __restrict__ w, int Cout, int Cin, int T, int mode, int nchunks, size_t i) {
    const int pos = (int)(i & 15), j = (int)((i >> 4) & 3);
    const int chunk = (int)((i >> 6) % nchunks), tap = (int)((i >> 6) / nchunks);
    const int red = mode == 0 ? Cin : Cout, out = mode == 0 ? Cout : Cin;
    const bool tail = (red & 15) != 0 && chunk == nchunks - 1;
    const int r = chunk * 16 + (tail ? (4 * (pos & 3) + (pos >> 2)) : pos);
    const int o = (out & ~15) + j;
    if (r >= red || o >= out) return 0.f;
    return mode == 0 ? w[((size_t)o * Cin + r) * T + tap] : w[((size_t)r * Cin + o) * T + tap];
}

// ---- the bf16 packed filter image ------------------------------------------------------------------------------
// wp[tap][chunk32][outPad][32], and for a 3x3 filter whose reduction leaves a tail of 1..8 channels (100 = 3 * 32 + 4) three more
// slabs fold[j][outPad][32]: k-slot (kq, c) of fold slab j = tail channel c of filter tap 4 j + kq.  One 16x16x32 MFMA then
// multiplies the tail channels of FOUR taps (each 8-channel lane group reads its own tap's pixel): the tail chunk costs 3 stages
// instead of 9 (30 instead of 36 for 100 channels).  Only single-tap-set launches use it (everything but the stride-2 input
// gradient, which reads the unfolded tail chunk that is still part of the image).
__host__ __device__ inline bool bf16_fold_tail(int red, int T) { return T == 9 && (red & 31) != 0 && (red & 31) <= 8; }
__host__ __device__ inline size_t bf16_image_elems(int red, int out_pad, int T) {
    return (size_t)(T * ((red + 31) / 32) + (bf16_fold_tail(red, T) ? 3 : 0)) * out_pad * 32;
}
// mode 2 = mode 0 with the image columns in pixel-shuffle order: column q = ij * (Cout / 4) + c holds filter 4 c + ij
__host__ __device__ inline int ps_filter_of(int q, int Cout) { const int nf = Cout >> 2; return 4 * (q % nf) + q / nf; }
// element i of the image of the fp32 master parameter w[Cout][Cin][T]; mode 0: out = cout, reduction = cin; mode 1: the reverse
__device__ inline float bf16_image_value(const float* __restrict__ w, int Cout, int Cin, int T, int mode, int nchunks, int outPad, size_t i) {
    const int rr = (int)(i & 31);
    size_t j = i >> 5;
    const int o = (int)(j % outPad);
    const int slab = (int)(j / outPad);
    const int red = mode == 1 ? Cout : Cin;
    int tap, r;
    if (slab < T * nchunks) {
        tap = slab / nchunks;
        r = (slab % nchunks) * 32 + rr;
    } else {
        tap = 4 * (slab - T * nchunks) + (rr >> 3);
        r = (nchunks - 1) * 32 + (rr & 7);
        if (tap >= T) return 0.f;
    }
    if (r >= red) return 0.f;
    if (mode == 2) return o < Cout ? w[((size_t)ps_filter_of(o, Cout) * Cin + r) * T + tap] : 0.f;
    if (mode == 0) return o < Cout ? w[((size_t)o * Cin + r) * T + tap] : 0.f;
    return o < Cin ? w[((size_t)r * Cin + o) * T + tap] : 0.f;
}

// ---- explicitly scheduled global loads for the 16x16x4 kernel -------------------------------------------------
// The compiler's s_waitcnt insertion merges the wait state of conditional loads conservatively (it drained vmcnt to 0 in
// the middle of the MFMA stream: a full L2 round trip per stage).  The main loop therefore issues its loads as inline asm
// (SGPR base + 32-bit lane offset) and places the vmcnt waits itself; vmcnt counts in issue order, and every path issues a
// fixed number of loads per stage (invalid items load from a clamped, always addressable offset and are zeroed later).
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;
// wave-uniform pointer -> SGPR pair for the saddr form.  The leading s_nop 4 of every load group covers the "VALU writes
// SGPR -> VMEM reads it" hazard (5 wait states): the compiler's hazard recognizer does not look inside inline asm.
__device__ __forceinline__ u64 sgpr_ptr(const void* p) {
    const u64 b = reinterpret_cast<u64>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return ((u64)hi << 32) | lo;
}
// operand-B tiles of one stage: tiles 0/1 at p + {0, TSTR}, tiles 2/3 at p + 2*TSTR + {0, TSTR}; one lane offset
template <int TSTR, int N>
__device__ __forceinline__ void gld_b(v4f (&d)[N], unsigned voff, const char* p) {
    static_assert(N == 2 || N == 4, "operand-B tiles per wave");
    const u64 s0 = sgpr_ptr(p);
    if constexpr (N == 2) {
        asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %2, %3\n\tglobal_load_dwordx4 %1, %2, %3 offset:%4"
                     : "=&v"(d[0]), "=&v"(d[1]) : "v"(voff), "s"(s0), "n"(TSTR));
    } else {
        const u64 s1 = sgpr_ptr(p + 2 * TSTR);
        asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %4, %5\n\tglobal_load_dwordx4 %1, %4, %5 offset:%7\n\t"
                     "global_load_dwordx4 %2, %4, %6\n\tglobal_load_dwordx4 %3, %4, %6 offset:%7"
                     : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]) : "v"(voff), "s"(s0), "s"(s1), "n"(TSTR));
    }
}
// The same with a lane offset of its own for the LAST tile: the kernels that share an odd last output tile between the two waves of a
// pixel row (see `nsplit` in conv_igemm16_kernel) address that tile out of the regular stride.
template <int TSTR, int N>
__device__ __forceinline__ void gld_bl(v4f (&d)[N], unsigned voff, unsigned voff_last, const char* p) {
    static_assert(N == 2 || N == 4, "operand-B tiles per wave");
    const u64 s0 = sgpr_ptr(p);
    if constexpr (N == 2) {
        asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %2, %4\n\tglobal_load_dwordx4 %1, %3, %4 offset:%5"
                     : "=&v"(d[0]), "=&v"(d[1]) : "v"(voff), "v"(voff_last), "s"(s0), "n"(TSTR));
    } else {
        const u64 s1 = sgpr_ptr(p + 2 * TSTR);
        asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %4, %6\n\tglobal_load_dwordx4 %1, %4, %6 offset:%8\n\t"
                     "global_load_dwordx4 %2, %4, %7\n\tglobal_load_dwordx4 %3, %5, %7 offset:%8"
                     : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]) : "v"(voff), "v"(voff_last), "s"(s0), "s"(s1), "n"(TSTR));
    }
}
// The halo items of one chunk: one base, one lane offset per item.  Executed in EVERY stage with `on` = all ones (fetch) or
// 0 (EXEC is cleared around the loads: nothing is fetched, the registers keep their values).  For the compiler the halo
// registers are thus one unbroken chain of tied asm operands -- no conditional definition, no phi, hence no register copy
// it could schedule between a load and its wait.
template <int N>
__device__ __forceinline__ void gld_halo(v4f (&h)[N], const unsigned (&vo)[N], const void* p, bool fetch) {
    static_assert(N == 4 || N == 6 || N == 10, "halo items per thread");
    const u64 sb = sgpr_ptr(p);
    const u64 on = sgpr_ptr(reinterpret_cast<const void*>(fetch ? ~0ull : 0ull));
    u64 sv;
    if constexpr (N == 4) {
        asm volatile("s_and_saveexec_b64 %[sv], %[on]\n\ts_nop 4\n\t"
                     "global_load_dwordx4 %[h0], %[o0], %[sb]\n\tglobal_load_dwordx4 %[h1], %[o1], %[sb]\n\t"
                     "global_load_dwordx4 %[h2], %[o2], %[sb]\n\tglobal_load_dwordx4 %[h3], %[o3], %[sb]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [h0] "+v"(h[0]), [h1] "+v"(h[1]), [h2] "+v"(h[2]), [h3] "+v"(h[3]), [sv] "=&s"(sv)
                     : [o0] "v"(vo[0]), [o1] "v"(vo[1]), [o2] "v"(vo[2]), [o3] "v"(vo[3]), [sb] "s"(sb), [on] "s"(on)
                     : "scc");   // s_and_saveexec writes SCC
    } else if constexpr (N == 6) {
        asm volatile("s_and_saveexec_b64 %[sv], %[on]\n\ts_nop 4\n\t"
                     "global_load_dwordx4 %[h0], %[o0], %[sb]\n\tglobal_load_dwordx4 %[h1], %[o1], %[sb]\n\t"
                     "global_load_dwordx4 %[h2], %[o2], %[sb]\n\tglobal_load_dwordx4 %[h3], %[o3], %[sb]\n\t"
                     "global_load_dwordx4 %[h4], %[o4], %[sb]\n\tglobal_load_dwordx4 %[h5], %[o5], %[sb]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [h0] "+v"(h[0]), [h1] "+v"(h[1]), [h2] "+v"(h[2]), [h3] "+v"(h[3]), [h4] "+v"(h[4]), [h5] "+v"(h[5]), [sv] "=&s"(sv)
                     : [o0] "v"(vo[0]), [o1] "v"(vo[1]), [o2] "v"(vo[2]), [o3] "v"(vo[3]), [o4] "v"(vo[4]), [o5] "v"(vo[5]), [sb] "s"(sb), [on] "s"(on)
                     : "scc");   // s_and_saveexec writes SCC
    } else {
        asm volatile("s_and_saveexec_b64 %[sv], %[on]\n\ts_nop 4\n\t"
                     "global_load_dwordx4 %[h0], %[o0], %[sb]\n\tglobal_load_dwordx4 %[h1], %[o1], %[sb]\n\t"
                     "global_load_dwordx4 %[h2], %[o2], %[sb]\n\tglobal_load_dwordx4 %[h3], %[o3], %[sb]\n\t"
                     "global_load_dwordx4 %[h4], %[o4], %[sb]\n\tglobal_load_dwordx4 %[h5], %[o5], %[sb]\n\t"
                     "global_load_dwordx4 %[h6], %[o6], %[sb]\n\tglobal_load_dwordx4 %[h7], %[o7], %[sb]\n\t"
                     "global_load_dwordx4 %[h8], %[o8], %[sb]\n\tglobal_load_dwordx4 %[h9], %[o9], %[sb]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [h0] "+v"(h[0]), [h1] "+v"(h[1]), [h2] "+v"(h[2]), [h3] "+v"(h[3]), [h4] "+v"(h[4]), [h5] "+v"(h[5]),
                       [h6] "+v"(h[6]), [h7] "+v"(h[7]), [h8] "+v"(h[8]), [h9] "+v"(h[9]), [sv] "=&s"(sv)
                     : [o0] "v"(vo[0]), [o1] "v"(vo[1]), [o2] "v"(vo[2]), [o3] "v"(vo[3]), [o4] "v"(vo[4]), [o5] "v"(vo[5]),
                       [o6] "v"(vo[6]), [o7] "v"(vo[7]), [o8] "v"(vo[8]), [o9] "v"(vo[9]), [sb] "s"(sb), [on] "s"(on)
                     : "scc");   // s_and_saveexec writes SCC
    }
}
// The four halo items of a chunk plus ONE item of the chunk's sliver filters (base of its own; lanes selected by `msl`, which is zero
// outside sliver launches).  Same contract as gld_halo: executed in every stage, EXEC-masked.
__device__ __forceinline__ void gld_halo4_sl(v4f (&h)[4], const unsigned (&vo)[4], const void* p, bool fetch, v4f& sl, unsigned vosl,
                                             const void* psl, u64 msl) {
    const u64 sb = sgpr_ptr(p), sbl = sgpr_ptr(psl);
    const u64 on = sgpr_ptr(reinterpret_cast<const void*>(fetch ? ~0ull : 0ull));
    const u64 ms = sgpr_ptr(reinterpret_cast<const void*>(msl));
    u64 sv;
    asm volatile("s_and_saveexec_b64 %[sv], %[on]\n\ts_nop 4\n\t"
                 "global_load_dwordx4 %[h0], %[o0], %[sb]\n\tglobal_load_dwordx4 %[h1], %[o1], %[sb]\n\t"
                 "global_load_dwordx4 %[h2], %[o2], %[sb]\n\tglobal_load_dwordx4 %[h3], %[o3], %[sb]\n\t"
                 "s_and_b64 exec, exec, %[ms]\n\ts_nop 0\n\t"
                 "global_load_dwordx4 %[sl], %[osl], %[sbl]\n\t"
                 "s_mov_b64 exec, %[sv]"
                 : [h0] "+v"(h[0]), [h1] "+v"(h[1]), [h2] "+v"(h[2]), [h3] "+v"(h[3]), [sl] "+v"(sl), [sv] "=&s"(sv)
                 : [o0] "v"(vo[0]), [o1] "v"(vo[1]), [o2] "v"(vo[2]), [o3] "v"(vo[3]), [osl] "v"(vosl), [sb] "s"(sb), [sbl] "s"(sbl),
                   [on] "s"(on), [ms] "s"(ms)
                 : "scc");
}
__device__ __forceinline__ void wait_loads_sl(v4f (&b)[4], v4f (&h)[4], v4f& sl) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(h[0]), "+v"(h[1]), "+v"(h[2]), "+v"(h[3]), "+v"(sl));
}
// s_waitcnt vmcnt(0) that also "defines" every register the outstanding loads write (operand-B tiles and halo items), so
// that no consumer is scheduled above it
template <int NB, int NH>
__device__ __forceinline__ void wait_loads(v4f (&b)[NB], v4f (&h)[NH]) {
    static_assert((NB == 2 || NB == 4) && (NH == 4 || NH == 6 || NH == 10), "register groups");
    // ONE statement (a tied operand's input copy, if the compiler ever made one, must not be able to slip in front of the
    // s_waitcnt of a sibling statement); 14 tied operands = 28 of the 30 asm operands allowed
#define UNET_H4 "+v"(h[0]), "+v"(h[1]), "+v"(h[2]), "+v"(h[3])
#define UNET_H6 UNET_H4, "+v"(h[4]), "+v"(h[5])
#define UNET_H10 UNET_H4, "+v"(h[4]), "+v"(h[5]), "+v"(h[6]), "+v"(h[7]), "+v"(h[8]), "+v"(h[9])
    if constexpr (NB == 4 && NH == 6) asm volatile("s_waitcnt vmcnt(0)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), UNET_H6);
    else if constexpr (NB == 2 && NH == 6) asm volatile("s_waitcnt vmcnt(0)" : "+v"(b[0]), "+v"(b[1]), UNET_H6);
    else if constexpr (NB == 2 && NH == 4) asm volatile("s_waitcnt vmcnt(0)" : "+v"(b[0]), "+v"(b[1]), UNET_H4);
    else if constexpr (NB == 2) asm volatile("s_waitcnt vmcnt(0)" : "+v"(b[0]), "+v"(b[1]), UNET_H10);
    else if constexpr (NH == 4) asm volatile("s_waitcnt vmcnt(0)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), UNET_H4);
    else asm volatile("s_waitcnt vmcnt(0)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), UNET_H10);
#undef UNET_H4
#undef UNET_H6
#undef UNET_H10
}

struct Plan {
    KArgs k;
    int tw, bm, bn, hit, nparity, mf, max_hpix;
    size_t lds_bytes;
    dim3 grid;
    // split-K (small grids with a long reduction): `splits` workgroups share one output tile, each reduces cps chunks into an fp32
    // slab [split][pixel][cp] of the caller's workspace; splitk_reduce_kernel adds the slabs in split order and applies the epilogue
    int splits, cp;
    size_t ws_floats;
    unet_tuning tune;        // the switches of this launch (a copy: the descriptor's or the defaults)
};


// one element of an activation tensor of either storage type (fp32 | bf16 bit pattern)
__device__ __forceinline__ float ld_act(const float* p) { return *p; }
__device__ __forceinline__ float ld_act(const unsigned short* p) { return __uint_as_float((unsigned)*p << 16); }
__device__ __forceinline__ void st_act(float* p, float v) { *p = v; }
__device__ __forceinline__ void st_act(unsigned short* p, float v) { *p = __builtin_bit_cast(unsigned short, (__bf16)v); }

// ---- host side: from a plan to a launch ------------------------------------------------------------------------
// Kernels that take more than 64 KiB of dynamic LDS: the attribute once per device (hipFuncSetAttribute is per device; the mask is a
// static of this template, so one per kernel instantiation, one bit per device ordinal), then the launch, then its check.
template <auto Kern, typename... Args>
int launch_big_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Args&... args) {
    static unsigned long long configured = 0;
    if (unet::first_use_on_device(&configured))
        UNET_CHECK_HIP(hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(Kern, grid, block, lds_bytes, st, args...);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

// The tile-shape ladder of the generic kernels of both storage types: tw, then bm / bn, then <TW, MT, NT, WM, WN, HIT>.  K supplies the
// kernel: K::launch<TW, MT, NT, WM, WN, HIT>(plan, y_f32, stream).
template <typename K, int TW, int HIT>
int launch_bn(const Plan& p, int y_f32, hipStream_t st) {
    if (p.bm == 64) {
        if (p.bn == 64) return K::template launch<TW, 1, 1, 2, 2, HIT>(p, y_f32, st);
        return K::template launch<TW, 1, 2, 2, 2, HIT>(p, y_f32, st);
    }
    switch (p.bn) {
        case 32: return K::template launch<TW, 1, 1, 4, 1, HIT>(p, y_f32, st);
        case 64: return K::template launch<TW, 2, 1, 2, 2, HIT>(p, y_f32, st);
        default: return K::template launch<TW, 2, 2, 2, 2, HIT>(p, y_f32, st);
    }
}
template <typename K, int HIT>
int launch_tw(const Plan& p, int y_f32, hipStream_t st) {
    switch (p.tw) {
        case 32: return launch_bn<K, 32, HIT>(p, y_f32, st);
        case 16: return launch_bn<K, 16, HIT>(p, y_f32, st);
        default: return launch_bn<K, 8, HIT>(p, y_f32, st);
    }
}
template <typename K>
int launch_generic(const Plan& p, int y_f32, hipStream_t st) {
    if (p.bm == 256 || p.hit == 6) {          // (the dispatcher hands these plans to conv_t256)
        unet::set_error("conv: inconsistent plan (the 256-pixel tile / halo item count 6 on the generic kernels)");
        return UNET_E_UNSUPPORTED;
    }
    return p.hit == 10 ? launch_tw<K, 10>(p, y_f32, st) : launch_tw<K, 4>(p, y_f32, st);
}

// ---- the launch functions of the kernel families (chosen by conv_dispatch.hip; each takes both storage types unless it says otherwise) ----
// the generic 128- / 64-pixel tiles: conv_igemm.hip (fp32: conv_igemm16_kernel / conv_igemm_kernel) and conv_bf16.hip (conv_bf16_kernel;
// y_f32: the output is fp32 although the activations are bf16)
int conv_generic_f32(const Plan& p, hipStream_t st);
int conv_generic_bf16(const Plan& p, int y_f32, hipStream_t st);
// the 256-pixel tile (conv_bf16.hip: conv_bf16_t256_kernel in its bf16 and its float form); an fp32 launch stores fp32 whatever y_f32 says
int conv_t256(const Plan& p, int dtype, int y_f32, hipStream_t st);
// epilogue of a split launch (conv_igemm.hip): y = act(sum_s slab[s] + bias + res) masked, in split order
int splitk_reduce(const unet_conv_desc* d, const Plan& p, hipStream_t st);
// 1x1 convolutions with a reduction of at most 8 channels (conv_igemm.hip: conv1x1_smallk_kernel)
bool conv_smallk_applies(const unet_conv_desc* d);
int conv_smallk(const unet_conv_desc* d, hipStream_t st);
// 3x3 forward convolutions of at most 8 input channels (the stem's first conv; conv_igemm.hip: conv3x3_smallcin_kernel)
bool conv_smallcin_applies(const unet_conv_desc* d);
int conv_smallcin(const unet_conv_desc* d, hipStream_t st);
// 1x1 forward convolutions with at most 16 produced channels (the segmentation head; conv1x1.hip: conv1x1_head_kernel)
bool conv_head1x1_applies(const unet_conv_desc* d);
int conv_head1x1(const unet_conv_desc* d, hipStream_t st);
// 1x1 / stride-1 convolutions of whole reduction chunks on the flat-pixel GEMM kernel (conv1x1.hip: conv1x1_gemm_kernel)
bool conv_gemm1x1_applies(const unet_conv_desc* d);
int conv_gemm1x1(const unet_conv_desc* d, hipStream_t st);
// validation of a unet_conv_desc.pixel_shuffle descriptor (UNET_OK: conv_gemm1x1 takes it)
int conv_gemm1x1_ps_check(const unet_conv_desc* d);

}  // namespace unetconv
