// The conv dispatcher of libunet_hip.so (host code only: no kernel lives here).  unet_conv2d, unet_conv2d_variant and
// unet_conv2d_splitk_workspace are behind every forward conv and input-gradient launch, and each has to know which kernel family takes a
// descriptor and with which plan: `choose` answers that ONCE, for both storage types -- validate and plan (make_plan), redirect a split plan
// into the caller's workspace (splitk_redirect), then walk the family ladder -- and `variant_id` names the choice for benchmarks and tests.
// The kernels and what each of them can take stay with their files (conv_igemm.hip, conv_bf16.hip, conv1x1.hip); conv_common.h declares
// their launch functions.
#include <stdlib.h>

#include "conv_common.h"

// The defaults of unet_tuning: constants, with environment overrides read ONCE when the library is loaded (A/B runs of whole programs).
// Nothing writes them afterwards: the library has no mutable process state.
namespace unetconv {
static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return (e != nullptr && e[0] != 0) ? atoi(e) : dflt;
}
const unet_tuning& tuning_defaults() {
    static const unet_tuning t = [] {
        unet_tuning v;
        v.conv_splitk = env_int("UNET_CONV_SPLITK", 1);
        v.mfma_shape = 16;
        v.f32_big_tile = 1;
        v.bf16_big_tile = 1;
        v.t256_tiles_per_wg = 0;
        v.t256_sliver = env_int("UNET_T256_SLIVER", 1);
        v.conv1x1_gemm = env_int("UNET_CONV1X1_GEMM", 0);
        v.wgrad_mfma_shape = 32;
        v.wgrad_bf16_k4 = 1;
        v.wgrad_1x1 = 1;
        v.wgrad_narrow = 1;
        v.plan_batch = 0;
        v.wgrad_wgs = env_int("UNET_WGRAD_WGS", 0);
        v.conv_smallcin = env_int("UNET_CONV_SMALLCIN", 1);
        v.conv_head1x1 = env_int("UNET_CONV_HEAD1X1", 1);
        return v;
    }();
    return t;
}
}  // namespace unetconv

extern "C" void unet_tuning_default(unet_tuning* t) {
    if (t != nullptr) *t = unetconv::tuning_defaults();
}

namespace {

using namespace unetconv;

// kc: reduction channels per chunk (16 fp32 / 32 bf16 = 64 bytes); vec: channels per 16-byte access (4 fp32 / 8 bf16): channel
// strides, offsets and the zero-padded channel count of a slice are multiples of vec; mf: MFMA shape of the fp32 kernels (16 | 32)
// big_tile: allow the 256-pixel workgroup tile (bf16 kernel: the math is 16x cheaper, so halving the filter-operand loads per MFMA pays)
// splitk: unet_tuning.conv_splitk of this plan (0: never split; callers that must not split pass 0)
// plan_batch: unet_tuning.plan_batch (0: the descriptor's N decides tile sizes / splits; n: as if the batch were n images)
int make_plan(const unet_conv_desc* d, Plan* p, int kc, int vec, int mf, int big_tile, int splitk, int plan_batch) {
    UNET_CHECK_ARG(d != nullptr, "conv: null desc");
    UNET_CHECK_ARG(d->x && d->wp && d->y, "conv: null tensor pointer");
    UNET_CHECK_ARG(d->ks == 1 || d->ks == 3, "conv: ks must be 1 or 3 (got %d)", d->ks);
    UNET_CHECK_ARG(d->stride == 1 || d->stride == 2, "conv: stride must be 1 or 2 (got %d)", d->stride);
    UNET_CHECK_ARG(!(d->ks == 1 && d->stride != 1), "conv: 1x1 stride 2 unsupported");
    UNET_CHECK_ARG(d->N > 0 && d->IH > 0 && d->IW > 0 && d->OH > 0 && d->OW > 0 && d->Cin > 0 && d->Cout > 0, "conv: bad dims");
    UNET_CHECK_ARG(unet::slice_ok_v(d->x_cs, d->x_co, d->Cin, vec), "conv: bad x slice cs=%d co=%d C=%d", d->x_cs, d->x_co, d->Cin);
    UNET_CHECK_ARG(unet::slice_ok_v(d->y_cs, d->y_co, d->Cout, d->y_f32 ? 4 : vec), "conv: bad y slice cs=%d co=%d C=%d", d->y_cs, d->y_co, d->Cout);
    UNET_CHECK_ARG(unet::aligned16(d->x) && unet::aligned16(d->wp), "conv: x/wp must be 16-byte aligned");
    if (d->res) UNET_CHECK_ARG(unet::slice_ok_v(d->res_cs, d->res_co, d->Cout, vec), "conv: bad res slice");
    if (d->flags & UNET_CONV_MASK) UNET_CHECK_ARG(d->mask && unet::slice_ok_v(d->mask_cs, d->mask_co, d->Cout, vec), "conv: bad mask slice");
    const int pad = (d->ks - 1) / 2;
    if (d->kind == UNET_CONV_FWD) {
        UNET_CHECK_ARG(d->OH == (d->IH + 2 * pad - d->ks) / d->stride + 1 && d->OW == (d->IW + 2 * pad - d->ks) / d->stride + 1,
                       "conv fwd: output dims %dx%d inconsistent with input %dx%d ks %d stride %d", d->OH, d->OW, d->IH, d->IW, d->ks, d->stride);
    } else if (d->kind == UNET_CONV_DGRAD) {
        // here I* = dims of the forward OUTPUT gradient, O* = dims of the forward INPUT
        UNET_CHECK_ARG(d->IH == (d->OH + 2 * pad - d->ks) / d->stride + 1 && d->IW == (d->OW + 2 * pad - d->ks) / d->stride + 1,
                       "conv dgrad: grad dims %dx%d inconsistent with input dims %dx%d", d->IH, d->IW, d->OH, d->OW);
    } else {
        UNET_CHECK_ARG(false, "conv: bad kind %d", d->kind);
    }
    // the image-local offsets are 32-bit
    UNET_CHECK_ARG((long long)d->IH * d->IW * d->x_cs < (1ll << 31) && (long long)d->OH * d->OW * d->y_cs < (1ll << 31) &&
                       (long long)d->OH * d->OW * (d->res ? d->res_cs : 1) < (1ll << 31) &&
                       (long long)d->OH * d->OW * ((d->flags & UNET_CONV_MASK) ? d->mask_cs : 1) < (1ll << 31),
                   "conv: image too large for 32-bit in-image offsets");

    KArgs& k = p->k;
    memset(&k, 0, sizeof(k));
    k.x = d->x; k.wp = d->wp; k.bias = d->bias; k.res = d->res; k.mask = (d->flags & UNET_CONV_MASK) ? d->mask : nullptr;
    k.y = d->y; k.colsum = d->colsum; k.colsumsq = d->colsumsq;
    k.x_cs = d->x_cs; k.x_co = d->x_co; k.res_cs = d->res_cs; k.res_co = d->res_co;
    k.mask_cs = d->mask_cs; k.mask_co = d->mask_co; k.y_cs = d->y_cs; k.y_co = d->y_co;
    k.N = d->N; k.IH = d->IH; k.IW = d->IW; k.Cin = d->Cin; k.Cin4 = unet::roundup(d->Cin, vec);
    k.OH = d->OH; k.OW = d->OW; k.Cout = d->Cout;
    // optional produced-channel range (a wide layer can be issued as several launches with different channel-block widths)
    const int cols = d->cout_count > 0 ? d->cout_count : d->Cout;
    UNET_CHECK_ARG(d->cout_begin >= 0 && (d->cout_begin & 15) == 0 && d->cout_begin + cols <= d->Cout, "conv: bad cout range [%d,+%d) of %d",
                   d->cout_begin, cols, d->Cout);
    k.n_base = d->cout_begin; k.n_end = d->cout_begin + cols;
    UNET_CHECK_ARG(d->wp_img_stride >= 0 && (d->wp_img_stride & 3) == 0, "conv: bad wp_img_stride");
    k.wp_stride = d->wp_img_stride;
    k.flags = d->flags;
    k.nchunks = unet::cdiv(d->Cin, kc);
    k.coutPad = unet::roundup(d->Cout, 128);
    p->nparity = 1;
    k.S = 1; k.OS = 1; k.TSH = d->OH; k.TSW = d->OW;

    const int T = d->ks * d->ks;
    if (d->kind == UNET_CONV_FWD) {
        k.S = d->stride;
        TapSet& t = k.taps[0];
        t.n = T; t.min_dy = -pad; t.min_dx = -pad; t.ext_y = d->ks; t.ext_x = d->ks; t.py = t.px = 0;
        for (int r = 0; r < d->ks; ++r)
            for (int s = 0; s < d->ks; ++s) {
                const int i = r * d->ks + s;
                t.dy[i] = (signed char)(r - pad); t.dx[i] = (signed char)(s - pad); t.widx[i] = (signed char)i;
            }
    } else if (d->stride == 1) {
        TapSet& t = k.taps[0];
        t.n = T; t.min_dy = -pad; t.min_dx = -pad; t.ext_y = d->ks; t.ext_x = d->ks; t.py = t.px = 0;
        for (int r = 0; r < d->ks; ++r)
            for (int s = 0; s < d->ks; ++s) {
                const int i = r * d->ks + s;
                t.dy[i] = (signed char)(pad - r); t.dx[i] = (signed char)(pad - s); t.widx[i] = (signed char)i;
            }
    } else {
        // stride-2 3x3 pad-1 dgrad: 4 output parity classes.  Output row 2*o+py receives
        //   py = 0: r = 1 from grad row o        py = 1: r = 0 from grad row o+1, r = 2 from grad row o
        k.OS = 2; k.TSH = (d->OH + 1) / 2; k.TSW = (d->OW + 1) / 2;
        p->nparity = 4;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                TapSet& t = k.taps[py * 2 + px];
                int rs[2], rdy[2], nr, ss[2], sdx[2], ns;
                if (py == 0) { nr = 1; rs[0] = 1; rdy[0] = 0; } else { nr = 2; rs[0] = 0; rdy[0] = 1; rs[1] = 2; rdy[1] = 0; }
                if (px == 0) { ns = 1; ss[0] = 1; sdx[0] = 0; } else { ns = 2; ss[0] = 0; sdx[0] = 1; ss[1] = 2; sdx[1] = 0; }
                t.n = nr * ns; t.min_dy = 0; t.min_dx = 0; t.ext_y = (py == 0) ? 1 : 2; t.ext_x = (px == 0) ? 1 : 2;
                t.py = py; t.px = px;
                int i = 0;
                for (int a = 0; a < nr; ++a)
                    for (int b = 0; b < ns; ++b, ++i) {
                        t.dy[i] = (signed char)rdy[a]; t.dx[i] = (signed char)sdx[b]; t.widx[i] = (signed char)(rs[a] * 3 + ss[b]);
                    }
            }
    }

    for (int z = 0; z < p->nparity; ++z) {
        TapSet& t = k.taps[z];
        t.dpack = 0; t.wpack = 0;
        for (int i = 0; i < t.n; ++i) {
            const int dyi = t.dy[i] - t.min_dy, dxi = t.dx[i] - t.min_dx;
            UNET_CHECK_ARG(dyi >= 0 && dyi < 4 && dxi >= 0 && dxi < 4 && t.widx[i] >= 0 && t.widx[i] < 16, "conv: tap table out of range");
            t.dpack |= (unsigned long long)(dyi | (dxi << 2)) << (4 * i);
            t.wpack |= (unsigned long long)t.widx[i] << (4 * i);
        }
    }

    p->tw = k.TSW >= 32 ? 32 : (k.TSW >= 16 ? 16 : 8);
    p->bn = cols <= 32 ? 32 : (cols <= 64 ? 64 : 128);
    p->bm = 128;
    p->hit = (k.S == 2) ? 10 : 4;
    p->mf = mf;
    // small problems (deep 16x16 / 32x32 stages): shrink the tile until the grid can fill 256 CUs x 2
    auto blocks = [&](int bm, int bn) {
        const int th_ = bm / p->tw;
        return (long long)(plan_batch > 0 ? plan_batch : d->N) * unet::cdiv(k.TSH, th_) * unet::cdiv(k.TSW, p->tw) * unet::cdiv(cols, bn) * p->nparity;
    };
    // Split-K first: a grid that cannot fill the chip with full-size tiles although the reduction is long (deep low-resolution stages,
    // small batches: BASELINE configs[0], predict at batch 1).  Instead of shrinking the tile -- fewer MACs per operand byte and still one
    // long serial reduction per workgroup -- `splits` workgroups per output tile each take a contiguous range of reduction chunks.
    // Partial sums meet in fixed order in the reduce kernel: deterministic, and the accumulation chain of an output element becomes
    // `splits` chains of K / splits products (the fp32 MFMA sums one k-ordered chain: its rounding error grows like sqrt(K)).
    p->splits = 1; p->cp = 0; p->ws_floats = 0;
    bool split = false;
    // fp32 on a small grid: narrower channel blocks (64, then 32) of the 256-pixel kernel put a workgroup on every CU.  Preferred to a split
    // reduction of the generic kernel (isolated launches, scripts/conv_f32_bias.py: 16 x 16 512 -> 512 0.207 -> 0.153 ms, 1024 -> 512 0.393 -> 0.299,
    // 32 x 32 128 -> 128 0.070 -> 0.045) and to the 64-pixel tile (32 x 32 256 -> 256 0.171 -> 0.147)
    int nb_first = 0;
    if (kc == 16 && big_tile && big_tile != 2 && d->ks == 3 && k.S == 1 && p->nparity == 1 && mf == 16 && d->colsum == nullptr && d->colsumsq == nullptr &&
        (p->tw == 32 || p->tw == 16) && p->bn == 128 && blocks(256, 128) < 256)
        nb_first = blocks(256, 64) >= 256 ? 64 : (blocks(256, 32) >= 256 ? 32 : 0);
    if (nb_first) p->bn = nb_first;
    if (!nb_first && splitk && mf == 16 && p->nparity == 1 && d->colsum == nullptr && d->colsumsq == nullptr && k.nchunks >= 8 && blocks(128, p->bn) < (splitk > 1 ? splitk : (kc == 32 ? 400 : 256))) {      // (bf16: measured +1.2 % on the step at 400; fp32 indifferent)
        // at least two chunks per split; when even the deepest split of full-size tiles leaves most CUs idle (a handful of pixel tiles:
        // 8 x 8 stages at batch 2), the tile shrinks as well
        const int smax = k.nchunks / 2 < 32 ? k.nchunks / 2 : 32;
        if (p->bn >= 64 && blocks(128, p->bn) * smax < 384) {
            p->bm = 64;
            if (p->bn == 128 && blocks(64, 128) * smax < 384) p->bn = 64;
        }
        const long long b = blocks(p->bm, p->bn);
        int sp = (int)((384 + b - 1) / b);
        if (sp > smax) sp = smax;
        if (sp >= 2) {
            split = true;
            k.cps = unet::cdiv(k.nchunks, sp);
            p->splits = unet::cdiv(k.nchunks, k.cps);
            p->cp = unet::roundup(cols, 4);
            k.slab = (long long)d->N * d->OH * d->OW * p->cp;
            p->ws_floats = (size_t)p->splits * k.slab;
        } else {
            p->bm = 128;
            p->bn = cols <= 32 ? 32 : (cols <= 64 ? 64 : 128);
        }
    }
    // bf16: the 256-pixel x 128-channel tile (conv_bf16_t256_kernel) for 3x3 / stride-1 launches from 64 blocks up -- on the deep 32 x 32
    // stages (a quarter of the chip's workgroup slots) it still beats the generic 128- / 64-pixel tiles by 1.2-1.7x, 512 -> 512: 109 -> 65 us,
    // with or without a split reduction on top (scripts/conv_mid_ab.py).  big_tile == 2: the order of round 3's first half (shrink first).
    // fp32 (kc == 16): the same kernel in its float form (a reduction tail runs transposed with its spare MFMA steps skipped; an output width of
    // 16 n + 1..4 takes a whole channel tile there instead of the 4-channel sliver of conv_igemm16_kernel); not for launches that emit column sums
    const bool f32_fit = kc != 16 || (mf == 16 && d->colsum == nullptr && d->colsumsq == nullptr);
    const bool big_ok = big_tile && f32_fit && d->ks == 3 && p->bm == 128 && (p->bn == 128 || big_tile != 2) && (p->tw == 32 || (p->tw == 16 && big_tile != 2)) && k.S == 1 && p->nparity == 1 &&
                        blocks(256, p->bn) >= (big_tile >= 3 ? 64 * (big_tile - 2) : (big_tile == 2 ? 512 : (kc == 16 ? 256 : 64))) &&        // (fp32 is MFMA-bound either way: it wants every CU busy)
                        (long long)d->IH * d->IW * d->x_cs * (kc == 16 ? 4 : 2) < (1ll << 31) - 65536 &&        // (bytes of ONE image at the storage width: the buffer descriptor's num_records, and the OOB offset 0x80000000 must stay outside it)
                        (long long)d->OH * d->OW * d->y_cs * 4 < (1ll << 31) - 65536;       // (its halo items and result stores go through buffer descriptors: one image within 2 GiB)
    if (!split && !(big_ok && big_tile != 2) && p->bn >= 64 && blocks(128, p->bn) < 400) {
        p->bm = 64;
        if (p->bn == 128 && blocks(64, 128) < 400) p->bn = 64;
    }
    if (big_ok && p->bm == 128) {
        p->bm = 256;          // 8 x 32 pixel patch per workgroup, each wave 128 pixels x 64 channels
        p->hit = 6;
    }
    const int th = p->bm / p->tw;
    k.tiles_y = unet::cdiv(k.TSH, th);
    k.tiles_x = unet::cdiv(k.TSW, p->tw);
    k.ntn = unet::cdiv(cols, p->bn);
    UNET_CHECK_ARG(k.n_base + k.ntn * p->bn <= k.coutPad, "conv: cout range leaves the packed filter image");
    // in-image element offsets are 32-bit inside the kernels (the image index is applied in 64 bits)
    UNET_CHECK_ARG((long long)d->IH * d->IW * d->x_cs < (1ll << 31) && (long long)d->OH * d->OW * d->y_cs < (1ll << 31) &&
                   (d->res == nullptr || (long long)d->OH * d->OW * d->res_cs < (1ll << 31)) &&
                   (d->mask == nullptr || (long long)d->OH * d->OW * d->mask_cs < (1ll << 31)),
                   "conv: one image of a tensor exceeds 2^31 elements");
    const long long mtiles_ll = (long long)d->N * k.tiles_y * k.tiles_x;
    UNET_CHECK_ARG(mtiles_ll * k.ntn < (1ll << 31) - 8, "conv: grid too large (%lld pixel tiles x %d channel blocks)", mtiles_ll, k.ntn);
    k.mtiles = (int)mtiles_ll;
    int max_hpix = 0;
    for (int z = 0; z < p->nparity; ++z) {
        const int hh = (th - 1) * k.S + k.taps[z].ext_y, hw = (p->tw - 1) * k.S + k.taps[z].ext_x;
        if (hh * hw > max_hpix) max_hpix = hh * hw;
    }
    UNET_CHECK_ARG(max_hpix * 4 <= p->hit * 256, "conv: halo tile too large (%d pixels)", max_hpix);
    p->max_hpix = max_hpix;
    // the 16x16x4 kernel keeps no filter slab in LDS (operand B goes global -> VGPR)
    p->lds_bytes = (size_t)(32 + 2 * max_hpix * LDK + (p->mf == 16 ? 0 : 2 * p->bn * LDK)) * sizeof(float);
    // fp32 sliver (kc == 16 only): the 128 x 128 tile of the 16x16x4 kernel, single tap set, the launch that produces the last channels,
    // one filter image for all batch images, no column sums
    k.sliver = 0; k.wsl = nullptr;
    if (kc == 16 && p->mf == 16 && p->bm == 128 && p->bn == 128 && p->hit == 4 && p->nparity == 1 && f32_sliver(d->Cout) && k.n_end == d->Cout &&
        d->wp_img_stride == 0 && d->colsum == nullptr && d->colsumsq == nullptr && p->splits == 1) {
        k.sliver = 1;
        k.wsl = d->wp + (size_t)T * k.nchunks * k.coutPad * 16;
        p->lds_bytes += (size_t)2 * 9 * 64 * sizeof(float);      // two chunk buffers at the kernel's fixed stride of 9 taps (a 1x1 filter uses one tap of each)
    }
    // (the 16x16x4 kernel remaps block ids XCD-aware and needs a multiple of 8; the surplus workgroups exit at once)
    p->grid = dim3((unsigned)unet::roundup((int)((long long)k.mtiles * k.ntn), p->mf == 16 ? 8 : 1), (unsigned)p->splits, (unsigned)p->nparity);
    UNET_CHECK_ARG((long long)k.mtiles * k.ntn < (1ll << 31), "conv: grid too large");
    return UNET_OK;
}

// Split-K launches: the kernels write plain partial sums (no bias / residual / activation / mask) into the workspace slabs.
// Returns false when the plan splits but the caller's workspace is missing or too small
// (the planner then has to be re-run without splitting).
bool splitk_redirect(const unet_conv_desc* d, Plan* p) {
    if (p->splits <= 1) return true;
    if (d->splitk_ws == nullptr || d->splitk_ws_floats < p->ws_floats) return false;
    KArgs& k = p->k;
    k.bias = nullptr; k.res = nullptr; k.mask = nullptr; k.flags = 0;
    k.y = d->splitk_ws - k.n_base;          // the kernels address channel c of a pixel as y[pixel * y_cs + y_co + c]: slab column 0 = n_base
    k.y_cs = p->cp; k.y_co = 0;
    return true;
}

// The planner of each storage type.  splitk < 0: the tuning's own value; 0: a plan that must not split (column-sum launches, a caller
// without a workspace)
int plan_f32(const unet_conv_desc* d, Plan* p, int splitk = -1) {
    UNET_CHECK_ARG(d != nullptr, "conv: null desc");
    const unet_tuning t = tuning_of(d->tuning);
    UNET_CHECK_ARG(t.mfma_shape == 16 || t.mfma_shape == 32, "conv: unet_tuning.mfma_shape must be 16 or 32 (start from unet_tuning_default())");
    const int rc = make_plan(d, p, KC, 4, t.mfma_shape, t.f32_big_tile ? 1 : 0, splitk < 0 ? t.conv_splitk : splitk, t.plan_batch);
    p->tune = t;
    return rc;
}
int plan_bf16(const unet_conv_desc* d, Plan* p, int splitk = -1) {
    UNET_CHECK_ARG(d != nullptr, "conv: null desc");
    const unet_tuning t = tuning_of(d->tuning);
    int rc = make_plan(d, p, KCB, 8, 16, t.bf16_big_tile, splitk < 0 ? t.conv_splitk : splitk, t.plan_batch);
    p->tune = t;
    if (rc != UNET_OK) return rc;
    UNET_CHECK_ARG(d->colsum == nullptr && d->colsumsq == nullptr, "conv bf16: column sums are not available in the bf16 kernel");
    p->lds_bytes = (size_t)(32 + 2 * p->max_hpix * LDKB) * sizeof(float);
    p->k.fold = (p->nparity == 1 && p->splits == 1 && bf16_fold_tail(d->Cin, d->ks * d->ks)) ? 1 : 0;
    UNET_CHECK_ARG(d->Cout % 4 == 0 || d->y_co + unet::roundup(d->Cout, 4) <= d->y_cs, "conv bf16: the output slice must own its 4-channel padding");
    UNET_CHECK_ARG(unet::aligned16(d->y) && (!d->res || unet::aligned16(d->res)) && (!d->mask || unet::aligned16(d->mask)),
                   "conv bf16: y/res/mask must be 16-byte aligned");
    return UNET_OK;
}
// (a null descriptor and every dtype but UNET_BF16 get the fp32 planner and its message; unet_conv2d refuses unknown dtypes itself)
int plan(const unet_conv_desc* d, Plan* p, int splitk = -1) {
    return d != nullptr && d->dtype == UNET_BF16 ? plan_bf16(d, p, splitk) : plan_f32(d, p, splitk);
}

enum class Family { PixelShuffle, SmallK, SmallCin, Head1x1, Gemm1x1, T256, Generic };

// THE selection: UNET_OK with the family that takes the descriptor and (all but PixelShuffle) its plan -- made with split-K when the caller
// brought a workspace for it, else without, the redirect into the workspace already applied -- or the error code of the validation that
// refused it.  Every descriptor that is not pixel-shuffle is planned, and so validated, before a special family is considered.
int choose(const unet_conv_desc* d, Family* f, Plan* p) {
    if (d != nullptr && d->pixel_shuffle) {          // 1x1 conv + activation + PixelShuffle(2) store: conv1x1_gemm_kernel only, validated there
        *f = Family::PixelShuffle;
        return conv_gemm1x1_ps_check(d);
    }
    int rc = plan(d, p);
    if (rc == UNET_OK && !splitk_redirect(d, p)) rc = plan(d, p, 0);
    if (rc != UNET_OK) return rc;
    if (conv_smallk_applies(d)) *f = Family::SmallK;
    else if (conv_smallcin_applies(d)) *f = Family::SmallCin;
    else if (conv_head1x1_applies(d)) *f = Family::Head1x1;
    else if (conv_gemm1x1_applies(d)) *f = Family::Gemm1x1;
    else *f = p->hit == 6 ? Family::T256 : Family::Generic;
    return UNET_OK;
}

// The id unet_conv2d_variant reports: 8 conv1x1_gemm_kernel (pixel-shuffle or not), 9 conv1x1_smallk_kernel, 10 conv3x3_smallcin_kernel,
// 11 conv1x1_head_kernel; the tiled kernels tw * 10000 + bn * 10 + last digit + 1000000 * splits (when split), last digit 0 = the 128-pixel
// tile, 1 = its stride-2 form (10 halo items), 5 = the 64-pixel tile, and for the 256-pixel tile 7 = the large layers (128-wide blocks, 32-pixel
// patches, >= 512 blocks: the launches bench.py's roofline follows), 6 = its narrow-block / 16-pixel-patch / small-grid launches
int variant_id(Family f, const Plan& p) {
    switch (f) {
        case Family::PixelShuffle: case Family::Gemm1x1: return 8;
        case Family::SmallK: return 9;
        case Family::SmallCin: return 10;
        case Family::Head1x1: return 11;
        default: break;
    }
    const bool large = p.bm == 256 && p.bn == 128 && p.tw == 32 && (long long)p.k.mtiles * p.k.ntn >= 512;
    return p.tw * 10000 + p.bn * 10 + (p.hit == 10 ? 1 : 0) + (p.bm == 64 ? 5 : 0) + (p.bm == 256 ? (large ? 7 : 6) : 0) + (p.splits > 1 ? 1000000 * p.splits : 0);
}

}  // namespace

extern "C" int unet_conv2d(const unet_conv_desc* d, void* stream) {
    UNET_CHECK_ARG(d == nullptr || d->pixel_shuffle || d->dtype == UNET_F32 || d->dtype == UNET_BF16, "conv: unknown dtype %d", d->dtype);
    Family f;
    Plan p;
    int rc = choose(d, &f, &p);
    if (rc != UNET_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool bf = d->dtype == UNET_BF16;
    const int y_f32 = p.splits > 1 ? 1 : d->y_f32;        // (bf16 kernels: partial sums are fp32 slabs)
    switch (f) {
        case Family::PixelShuffle: case Family::Gemm1x1: return conv_gemm1x1(d, st);
        case Family::SmallK: return conv_smallk(d, st);
        case Family::SmallCin: return conv_smallcin(d, st);
        case Family::Head1x1: return conv_head1x1(d, st);
        case Family::T256: rc = conv_t256(p, d->dtype, y_f32, st); break;
        case Family::Generic: rc = bf ? conv_generic_bf16(p, y_f32, st) : conv_generic_f32(p, st); break;
    }
    if (rc != UNET_OK || p.splits <= 1) return rc;
    return splitk_reduce(d, p, st);
}

extern "C" int unet_conv2d_variant(const unet_conv_desc* d) {
    Family f;
    Plan p;
    const int rc = choose(d, &f, &p);
    return rc == UNET_OK ? variant_id(f, p) : rc;
}

// the workspace the plan made with the tuning's own split setting asks for (what a caller has to bring for the launch to split)
extern "C" size_t unet_conv2d_splitk_workspace(const unet_conv_desc* d) {
    Plan p;
    if (d == nullptr || d->pixel_shuffle) return 0;
    return plan(d, &p) == UNET_OK ? p.ws_floats : 0;
}

extern "C" int unet_conv2d_colsum_rows(const unet_conv_desc* d) {
    Plan p;
    // the plan of the launch that WILL carry the column-sum pointers (they may still be null in this query): an fp32 launch, never split
    const int rc = plan_f32(d, &p, 0);
    if (rc != UNET_OK) return rc;
    const int wm = (p.bn == 32 && p.bm == 128) ? 4 : 2;
    return p.nparity * p.k.mtiles * wm;
}
