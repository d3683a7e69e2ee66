/*
 * unet_hip.h -- C ABI of libunet_hip.so: the MI355X (gfx950) hot path of the
 * U-Net segmentation train / predict step.
 *
 * The reference (LUP-LuftbildUmweltPlanung/UNet) has no FFI of its own: its hot
 * path is two Python lines -- model construction (train.py:128-144) and
 * learn.fit_one_cycle / learn.predict (train.py:247-250, predict.py:193) -- whose
 * arithmetic is executed by fastai 2.5.1 + ATen.  Each entry point below replaces
 * the ATen operator family that graph issues; the
 * comment on each names the fastai module / reference call site it stands for.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch allocates);
 *     the library never allocates, frees or synchronises;
 *   - all tensors are fp32 NHWC; a tensor argument is (ptr, cs, co): base
 *     pointer of the [N,H,W,cs] buffer, physical channel stride cs (multiple of
 *     4) and channel offset co (multiple of 4) -- this is how torch.cat is
 *     eliminated: producers write channel slices of one buffer;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued
 *     asynchronously on it;
 *   - return value: 0 = OK, <0 = UNET_E_*; unet_last_error() gives the text.
 */
#ifndef UNET_HIP_H
#define UNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNET_OK 0
#define UNET_E_BADARG (-1)
#define UNET_E_UNSUPPORTED (-2)
#define UNET_E_HIP (-3)

#define UNET_ABI_VERSION 8

int unet_abi_version(void);
const char* unet_last_error(void);

/* Storage type of activations / activation gradients / packed filter images.  UNET_F32 is the parity path (the reference computes in
 * fp32: train.py:141-144 has no to_fp16()).  UNET_BF16 is the bf16-storage variant of BASELINE.json configs[1]: tensors are bfloat16
 * bit patterns (unet_bf16), channel strides / offsets are multiples of 8 (16-byte vectors), every product is accumulated in fp32
 * (v_mfma_f32_16x16x32_bf16), per-channel vectors (bias, BatchNorm coefficients), losses, master weights and optimizer state stay
 * fp32.  Entry points with a _bf16 suffix take bf16 tensors where the fp32 entry point takes float tensors. */
#define UNET_F32 0
#define UNET_BF16 1
typedef uint16_t unet_bf16;

/* ---------------------------------------------------------------- tuning --
 * Kernel-selection switches of ONE launch (A/B measurements, cross-checks between independently written kernel families in the tests).
 * A descriptor's `tuning` pointer may be NULL: the defaults.  The library keeps NO mutable process state: the switches
 * travel with the descriptor, two callers -- threads, models -- with different tunings do not see each other, every entry point is
 * re-entrant.  Always start from unet_tuning_default(): a zeroed struct is NOT the default.  Every alternative computes the same result up
 * to summation order.  Environment overrides of the DEFAULTS, read once at load: UNET_CONV_SPLITK, UNET_T256_SLIVER, UNET_CONV1X1_GEMM. */
typedef struct {
    int conv_splitk;        /* 1: the planner may split the reduction of small-grid launches (default); 0: never; n > 1: split launches of
                               fewer than n full-size tiles */
    int mfma_shape;         /* fp32 conv: 16 = v_mfma_f32_16x16x4_f32 (default), 32 = v_mfma_f32_32x32x2_f32 with an LDS filter slab */
    int f32_big_tile;       /* 1: eligible fp32 3x3 launches run on conv_bf16_t256_kernel<.., float> (default); 0: conv_igemm16_kernel */
    int bf16_big_tile;      /* bf16 conv: 1 = the 256-pixel tile for 3x3 / stride-1 launches from 64 blocks up (default), 0 = off,
                               2 = the planner order of round 3's first half, 3.. = from 64 (n - 2) blocks up */
    int t256_tiles_per_wg;  /* consecutive tiles per workgroup of conv_bf16_t256_kernel; 0 = the launcher's choice (default) */
    int t256_sliver;        /* 1: a 7-tile fp32 block whose last tile holds 1..4 channels multiplies them as a 4x4x1 sliver (default) */
    int conv1x1_gemm;       /* plain 1x1 / stride-1 convs of whole chunks on conv1x1_gemm_kernel (the flat-pixel GEMM, csrc/conv1x1.hip):
                               0 = auto (default): its LDS-staged form for bf16 storage, the implicit-GEMM kernels for fp32 (measured);
                               1 = its direct form, 2 = its staged form (both storage types), -1 = never.  pixel_shuffle descriptors always use it */
    int wgrad_mfma_shape;   /* fp32 weight gradient: 32 (default) | 16 (opt-in: loses to wave imbalance) */
    int wgrad_bf16_k4;      /* 1: bf16 3x3 / 1x1 stride-1 weight gradients on wgrad_bf16_k4_kernel (default); 0: wgrad_bf16_kernel */
    int wgrad_1x1;          /* 1: the 128x128-tiled GEMM kernel (and the small-output FMA kernel) for fp32 1x1 weight gradients (default; launches of
                               <= 64 input / output channels or < 3 GFLOP stay on the 64x64-blocked general kernel); 2: the GEMM kernel for all; 0: never */
    int wgrad_narrow;       /* 1: the narrow-output (80 < Cout <= 112) flattened-tap fp32 weight-gradient kernel (default); 2: the same without the
                               4-row v_mfma_f32_4x4x1 sliver for 97..100 output channels (seven 16-row tiles: A/B, cross-check); 3: as 1, and the
                               general fp32 kernel without the pixel sub-splits of layers with <= 32 input / output channels (A/B); 4: as 1,
                               and every launch of the narrow-output kernel stages its tiles through registers (A/B, cross-check: same bits).
                               With 1, 2 and 3 a launch whose column blocks each read at most two of the three tap rows loads its tiles by
                               LDS-DMA (buffer loads straight to LDS); unet_conv2d_wgrad_dma tells which form a descriptor gets */
    int plan_batch;         /* 0 (default): the conv planner sizes tiles / split reductions for the batch of the descriptor.  n > 0: it plans as
                               if the batch were n images, whatever N is -- with 1, every image of a batch runs exactly the kernels, tiles and split
                               chains it would run alone: predictions become bit-identical ACROSS batch sizes (the reference predicts tile by
                               tile, predict.py:191-193), at the price of batch-1 plans on full grids (predict.predict_raster(batch_invariant=True)) */
    int wgrad_wgs;          /* workgroups a weight-gradient launch is split into (split-K over pixel tiles).  0 (default): ~512 (two per CU); bf16
                               storage, 3x3 layers up to ~175 GFLOP: ~256 (one per CU: half the partial filter images to write and read back,
                               measured faster).  n > 0: ~n workgroups (A/B) */
    int conv_smallcin;      /* 1 (default): forward 3x3 convs of <= 8 input channels (the stem's first conv) on the direct HBM-bound kernel; 0: the
                               implicit-GEMM kernels (A/B, cross-check) */
    int conv_head1x1;       /* 1 (default): 1x1 forward convs with <= 16 produced channels (the segmentation head) on the streaming kernel that keeps
                               the filter in registers; 0: the implicit-GEMM kernels (A/B, cross-check: same bits); 2: the other pixel-tile count per trip (A/B) */
} unet_tuning;
void unet_tuning_default(unet_tuning* t);

/* ------------------------------------------------------------------ conv --
 * Implicit-GEMM convolution on fp32 MFMA, NHWC, no im2col.  Default instruction v_mfma_f32_16x16x4_f32: LDS-staged input halo
 * tile, packed filter tiles global -> VGPR (MFMA operand order); v_mfma_f32_32x32x2_f32 with an LDS filter slab is kept
 * behind unet_tuning.mfma_shape = 32.
 * Replaces: every nn.Conv2d of fastai ConvLayer (layers.py) in XResNet
 * (vision/models/xresnet.py), DynamicUnet.middle_conv / UnetBlock.conv1,conv2 /
 * PixelShuffle_ICNR 1x1 / final ResBlock / head (vision/models/unet.py), as
 * built by train.py:128-144, and their autograd input-gradients.
 */

/* flags for unet_conv2d */
#define UNET_CONV_RELU 1          /* y = max(y, 0) after bias/residual */
#define UNET_CONV_MASK 4          /* y = (maskref > 0) ? y : 0 (ReLU backward fused in dgrad) */

/* kind */
#define UNET_CONV_FWD 0           /* y = conv(x, W) stride S pad (ks-1)/2 */
#define UNET_CONV_DGRAD 1         /* y = dL/dx given x := dL/d(conv out); wp packed by unet_pack_weights(mode DGRAD) */

typedef struct {
    const float* x; int x_cs, x_co;      /* input: FWD: activations [N,IH,IW]; DGRAD: output-gradient [N,IH,IW] */
    const float* wp;                     /* packed weights (unet_pack_weights) */
    const float* bias;                   /* [Cout] or NULL */
    const float* res; int res_cs, res_co;      /* optional residual added before activation, same geometry as y */
    const float* mask; int mask_cs, mask_co;   /* UNET_CONV_MASK reference, same geometry as y */
    float* y; int y_cs, y_co;            /* output [N,OH,OW] */
    int N, IH, IW, Cin;                  /* Cin = reduction channels of this launch */
    int OH, OW, Cout;                    /* Cout = produced channels of this launch */
    int ks, stride;                      /* kernel size 1|3, stride 1|2 of the FORWARD convolution */
    int kind, flags;
    float* colsum;                       /* optional [rows][Cout] per-wave partial column sums of y (bias-grad / BN stats), or NULL */
    float* colsumsq;                     /* optional same shape, sums of y*y */
    int cout_begin, cout_count;          /* produce only channels [cout_begin, cout_begin + cout_count) of the Cout-wide problem
                                            (cout_begin % 16 == 0); 0, 0 = all.  Lets a caller issue e.g. 192 channels as 128 + 64
                                            with a channel-block width that fits each part. */
    long long wp_img_stride;             /* elements between the packed filter images of consecutive batch images; 0 = one image for all.
                                            Per-image "filters" are activations: the attention products of SelfAttention run as ONE
                                            launch over the batch (unet_pack_weights_strided once per image into one buffer). */
    int dtype;                           /* UNET_F32 (default 0) | UNET_BF16: storage type of x, res, mask, y and wp (cast the pointers);
                                            bias stays fp32.  bf16: wp from unet_pack_weights_bf16, colsum / colsumsq unsupported */
    int y_f32;                           /* dtype UNET_BF16 only: y is an fp32 buffer (the logits head feeds the fp32 loss kernels) */
    float* splitk_ws;                    /* optional scratch for split-K launches (small grid, long reduction): fp32, 16-byte aligned, */
    size_t splitk_ws_floats;             /*   >= unet_conv2d_splitk_workspace(desc) floats; NULL / too small = never split this launch */
    const unet_tuning* tuning;           /* NULL = defaults */
    int pixel_shuffle;                   /* 1: a 1x1 FWD conv of Cout = 4 nf channels that stores PixelShuffle(2)(act(conv)) directly: y is a Cout / 4 wide
                                            slice of a [N, 2 OH, 2 OW] tensor, produced channel q = ij * nf + c of pixel (h, w) lands at channel c of pixel
                                            (2 h + ij / 2, 2 w + ij % 2); wp must be the mode-2 image (columns in that order), bias stays in the filter's own
                                            order.  The PixelShuffle_ICNR without blur in front of the dense merge (reference train.py:141: blur_final applies
                                            to the LAST UnetBlock, the final upsample has none) then needs no un-shuffled copy of the conv output at all.
                                            Only descriptors unet_conv2d_variant answers 8 for are taken (UNET_E_UNSUPPORTED otherwise) */
    /* pixel_shuffle only, optional (ps_tail = NULL: none): an NHWC tensor [N, 2 OH, 2 OW] of y's storage type whose channels [ps_tail_co,
       ps_tail_co + ps_tail_c) are copied to channels [ps_tail_at, ..) of y's BUFFER (counted from the buffer, not from y_co) by the lane that
       stores the last four shuffled channels of the same pixel: the network-input half of DynamicUnet's final concat (reference train.py:141,
       last_cross: cat([up, x])) without a second pass of 8-byte writes at 208-byte stride over the buffer (158 us alone at 16 x 512^2; measured
       with bf16 storage: 490 + 158 us -> 598 us in one launch; with fp32 storage the appended stores cost more than the pass: 1021 + 155 -> 1229,
       so the model uses it for bf16 only).  Whole quads are copied (ps_tail_c rounded up to 4: pad lanes of the source are zeros);
       ps_tail_cs, ps_tail_co and ps_tail_at are multiples of 4, ps_tail_at + roundup(ps_tail_c, 4) <= y_cs */
    const void* ps_tail;
    int ps_tail_cs, ps_tail_co;
    int ps_tail_c, ps_tail_at;
} unet_conv_desc;

/* number of partial rows the colsum buffers must hold for this desc */
int unet_conv2d_colsum_rows(const unet_conv_desc* d);
int unet_conv2d(const unet_conv_desc* d, void* stream);
/* floats of split-K scratch the planner would use for this desc (0: it does not split).  A launch whose output grid cannot fill the chip
 * although its reduction is long (deep low-resolution stages, small batches) is cut into `splits` contiguous ranges of reduction chunks;
 * partial sums are added in split order by a second kernel that applies bias / residual / ReLU / mask: deterministic, and shorter
 * accumulation chains.  unet_tuning.conv_splitk = 0 switches it off for a launch (A/B). */
size_t unet_conv2d_splitk_workspace(const unet_conv_desc* d);
/* which kernel instantiation serves this desc: TW*10000 + BN*10 + (stride-2 halo variant) + 1000000 * splits -- for profilers / bench.py;
 * ...7 / ...6: the 256-pixel tile of the bf16 path (3x3 stride 1: conv_bf16_t256_kernel; 7 = 128-wide blocks, 32-pixel patches, >= 512 blocks,
 * 6 = its narrow-block / 16-pixel-patch / small-grid launches); 9: conv1x1_smallk_kernel (1x1, reduction of <= 8 channels);
 * 8: conv1x1_gemm_kernel (1x1 stride 1, whole reduction chunks, >= 256 blocks: the flat-pixel GEMM without LDS staging) */
int unet_conv2d_variant(const unet_conv_desc* d);
/* weight packing.  w is the torch-layout master parameter [Cout,Cin,ks,ks].
 * mode 0 (FWD):   wp[tap][chunk][coutPad][16]  reduction over Cin
 * mode 1 (DGRAD): wp[tap][chunk][cinPad][16]   reduction over Cout
 * mode 2 (FWD, pixel-shuffle order; ks = 1, Cout % 64 == 0): mode 0 with image column q = ij * (Cout / 4) + c holding filter 4 c + ij
 *                 (what unet_conv_desc.pixel_shuffle stores from)
 * pads are zero filled; chunk = 16 reduction channels; *Pad = roundup(.,128). */
size_t unet_pack_weights_size(int Cout, int Cin, int ks, int mode); /* floats */
int unet_pack_weights(const float* w, float* wp, int Cout, int Cin, int ks, int mode, void* stream);
/* 1x1 "weights" that are themselves activations (self-attention operands): element (out o, reduction r) = w[o*so + r*sr];
 * produces the same packed image as mode 0 with ks = 1 (size unet_pack_weights_size(O, R, 1, 0), the sliver block of a 16 n + 1..4 wide
 * output included). */
int unet_pack_weights_strided(const float* w, long long so, long long sr, float* wp, int O, int R, void* stream);
/* bf16 images from the fp32 master parameter: wp[tap][chunk][outPad][32] with chunk = 32 reduction channels (64 bytes, as in fp32);
 * a 3x3 filter whose reduction leaves a tail of 1..8 channels gets three more slabs fold[j][outPad][32] (k-slot (kq, c) = tail
 * channel c of tap 4 j + kq) that single-tap-set launches read instead of the nine tail chunks.  The size function includes them. */
size_t unet_pack_weights_size_bf16(int Cout, int Cin, int ks, int mode); /* elements */
int unet_pack_weights_bf16(const float* w, unet_bf16* wp, int Cout, int Cin, int ks, int mode, void* stream);
/* All filter images of a model in one launch (the parameters change every step, so every image is rebuilt every step).
 * unet_pack_batch_build fills a HOST table (unet_pack_batch_table_bytes(njobs) bytes) from the job list -- same layouts as
 * unet_pack_weights (dtype UNET_F32) / unet_pack_weights_bf16 (UNET_BF16) -- and returns the grid size; the caller uploads the table
 * once (addresses are static) and calls unet_pack_batch_run on it whenever the parameters have changed. */
typedef struct {
    const float* w;                      /* master parameter [Cout,Cin,ks,ks] (device) */
    void* wp;                            /* packed image (device), unet_pack_weights_size[_bf16] elements */
    int Cout, Cin, ks, mode;             /* mode 0 = forward image, 1 = input-gradient image */
    const float* out_scale;              /* optional [Cout] (device), mode 0: image of w * out_scale[cout] -- eval-mode BatchNorm folded into
                                            the filter (y = conv(x, w * scale) + shift, the conv epilogue adds shift as its bias) */
} unet_pack_job;
size_t unet_pack_batch_table_bytes(int njobs);
int unet_pack_batch_build(const unet_pack_job* jobs, int njobs, int dtype, void* table_host, unsigned* total_blocks);
int unet_pack_batch_run(const void* table_dev, int njobs, unsigned total_blocks, int dtype, void* stream);
/* weight gradient dW[Cout,Cin,ks,ks] (torch layout) = sum_pixels dy (x) x.
 * Replaces the autograd weight-gradient of the same nn.Conv2d modules.
 * workspace holds split-K partials; query its size (floats) first. */
typedef struct {
    const float* x; int x_cs, x_co;      /* forward input  [N,IH,IW,Cin] */
    const float* dy; int dy_cs, dy_co;   /* output grad    [N,OH,OW,Cout] */
    float* dw;                           /* [Cout,Cin,ks,ks] */
    float* dbias;                        /* [Cout] or NULL: also produce sum_pixels dy */
    int N, IH, IW, Cin, OH, OW, Cout, ks, stride;
    float* workspace; size_t workspace_floats;
    int accumulate;                      /* 0: dw = result, 1: dw += result */
    int dtype;                           /* UNET_F32 (default 0) | UNET_BF16: storage type of x and dy; dw, dbias and the workspace are fp32 */
    const unet_tuning* tuning;           /* NULL = defaults */
} unet_wgrad_desc;
size_t unet_conv2d_wgrad_workspace(const unet_wgrad_desc* d);
/* 1: the launch loads its tiles by LDS-DMA (see unet_tuning.wgrad_narrow), 0: through registers or on another kernel, -1: bad descriptor */
int unet_conv2d_wgrad_dma(const unet_wgrad_desc* d);
int unet_conv2d_wgrad(const unet_wgrad_desc* d, void* stream);

/* ----------------------------------------------------------- batch norm --
 * Replaces nn.BatchNorm2d(eps 1e-5, momentum 0.1) of fastai BatchNorm
 * (layers.py) in train mode (batch statistics, wavefront reductions) and eval
 * mode (running statistics), fused with residual add + ReLU of ResBlock.forward.
 */
/* per-channel partial sums of x and x*x over P pixels -> two planes partial[0:rows][C] (sums) and
 * partial[rows:2*rows][C] (sums of squares); rows = unet_bn_stats_rows(P) */
int unet_bn_stats_rows(long long P);
int unet_bn_stats(const float* x, int x_cs, int x_co, long long P, int C, float* partial, void* stream);
/* train-mode finalize: from partial sums psum[rows][C], psumsq[rows][C] (unet_bn_stats planes or the
 * colsum/colsumsq of a conv epilogue) compute mean / invstd, scale = gamma*invstd, shift = beta - mean*scale,
 * and update running stats (unbiased var, momentum); batches_tracked (BatchNorm2d.num_batches_tracked, int64, or NULL) += 1. */
int unet_bn_finalize(const float* psum, const float* psumsq, int rows, long long count, int C,
                     const float* gamma, const float* beta, float* running_mean, float* running_var,
                     float momentum, float eps,
                     float* scale, float* shift, float* save_mean, float* save_invstd, long long* batches_tracked, void* stream);
/* eval-mode: scale/shift from running stats */
int unet_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                        float eps, int C, float* scale, float* shift, void* stream);
/* y = act(x*scale+shift [+ x2*scale2+shift2 | + x2]) ; scale2 NULL with x2 != NULL means plain add */
int unet_affine_act(const float* x, int x_cs, int x_co, const float* scale, const float* shift,
                    const float* x2, int x2_cs, int x2_co, const float* scale2, const float* shift2,
                    float* y, int y_cs, int y_co, long long P, int C, int relu, void* stream);
/* BN backward, train mode.  g = dout * (out > 0 if out != NULL).
 * reduce: planes partial[0:rows][C] = sum g, partial[rows:2*rows][C] = sum g*xhat; rows = unet_bn_stats_rows(P) */
int unet_bn_bwd_reduce(const float* dout, int d_cs, int d_co, const float* out, int o_cs, int o_co,
                       const float* x, int x_cs, int x_co, const float* mean, const float* invstd,
                       long long P, int C, float* partial, void* stream);
/* finalize: dgamma, dbeta and coefficient vectors c1 = sum g / count, c2 = sum g xhat / count */
int unet_bn_bwd_finalize(const float* partial, int rows, long long count, int C,
                         float* dgamma, float* dbeta, float* c1, float* c2, void* stream);
/* apply: dx = gamma*invstd*(g - c1 - xhat*c2) ; optionally also writes g to gout (for the residual branch) */
int unet_bn_bwd_apply(const float* dout, int d_cs, int d_co, const float* out, int o_cs, int o_co,
                      const float* x, int x_cs, int x_co, const float* mean, const float* invstd,
                      const float* gamma, const float* c1, const float* c2,
                      float* dx, int dx_cs, int dx_co, float* gout, int g_cs, int g_co, int g_accumulate,
                      long long P, int C, void* stream);

/* -------------------------------------------------------------- pooling --
 * MaxPool2d(3,2,1) after the stem and AvgPool2d(2, ceil_mode=True) on strided
 * identity paths (fastai xresnet.py / layers.py ResBlock). */
int unet_maxpool3x3s2(const float* x, int x_cs, int x_co, float* y, int y_cs, int y_co, uint8_t* idx,
                      int N, int IH, int IW, int C, int OH, int OW, void* stream);
int unet_maxpool3x3s2_bwd(const float* dy, int dy_cs, int dy_co, const uint8_t* idx, float* dx, int dx_cs, int dx_co,
                          int N, int IH, int IW, int C, int OH, int OW, int accumulate, void* stream);
int unet_avgpool2_ceil(const float* x, int x_cs, int x_co, float* y, int y_cs, int y_co,
                       int N, int IH, int IW, int C, int OH, int OW, void* stream);
int unet_avgpool2_ceil_bwd(const float* dy, int dy_cs, int dy_co, float* dx, int dx_cs, int dx_co,
                           int N, int IH, int IW, int C, int OH, int OW, int accumulate, void* stream);

/* -------------------------------------------------- decoder data movement --
 * PixelShuffle_ICNR (layers.py) tail and UnetBlock.forward (vision/models/unet.py):
 *   up = [blur](PixelShuffle(2)(yc)),  yc = relu(conv1x1(x)) of shape [N,h,w,4*Cu]
 *   PixelShuffle: P[2h+i, 2w+j, c] = yc[h, w, 4c+2i+j]
 *   blur = ReplicationPad2d((1,0,1,0)) + AvgPool2d(2, stride=1)
 * writes X[N,2h,2w][X_co : X_co+Cu]; the skip half of torch.cat is written by
 * unet_affine_act (relu(bn(skip))) into the neighbouring channel slice. */
int unet_shuffle_blur(const float* yc, int yc_cs, int yc_co, float* X, int X_cs, int X_co,
                      int N, int h, int w, int Cu, int do_blur, void* stream);
/* adjoint incl. the ReLU of the 1x1 conv: dyc = (yc > 0) * shuffle^T(blur^T(dX)) */
int unet_shuffle_blur_bwd(const float* dX, int dX_cs, int dX_co, const float* yc, int yc_cs, int yc_co,
                          float* dyc, int dyc_cs, int dyc_co, int N, int h, int w, int Cu, int do_blur, void* stream);
/* the same adjoint without blur when the forward stored the shuffled activation only (unet_conv_desc.pixel_shuffle): the ReLU mask is read
 * from X, the [N,2h,2w] forward output, at the address of dX: dyc[h,w,4c+2i+j] = X[2h+i,2w+j,c] > 0 ? dX[2h+i,2w+j,c] : 0 */
int unet_shuffle_bwd_xmask(const float* dX, int dX_cs, int dX_co, const float* X, int X_cs, int X_co,
                           float* dyc, int dyc_cs, int dyc_co, int N, int h, int w, int Cu, void* stream);
/* F.interpolate(mode='nearest') and its adjoint (UnetBlock / ResizeToOrig when sizes differ) */
int unet_resize_nearest(const float* x, int x_cs, int x_co, float* y, int y_cs, int y_co,
                        int N, int IH, int IW, int OH, int OW, int C, void* stream);
int unet_resize_nearest_bwd(const float* dy, int dy_cs, int dy_co, float* dx, int dx_cs, int dx_co,
                            int N, int IH, int IW, int OH, int OW, int C, void* stream);
/* layout conversion at the seam (torch side is NCHW): */
int unet_nchw_to_nhwc(const float* x, float* y, int y_cs, int y_co, int N, int C, int H, int W, void* stream);
int unet_nhwc_to_nchw(const float* x, int x_cs, int x_co, float* y, int N, int C, int H, int W, void* stream);
/* elementwise helpers on NHWC slices */
int unet_copy_slice(const float* x, int x_cs, int x_co, float* y, int y_cs, int y_co, long long P, int C,
                    int accumulate, void* stream);
int unet_relu_mask(const float* g, int g_cs, int g_co, const float* ref, int r_cs, int r_co,
                   float* y, int y_cs, int y_co, long long P, int C, void* stream);
int unet_colsum(const float* x, int x_cs, int x_co, long long P, int C, float* out, float* workspace, void* stream);
size_t unet_colsum_workspace(long long P, int C);
/* out[0] = sum over pixels and channels of x * y (fp64 second stage); workspace = unet_colsum_workspace(P, C) floats.
 * SelfAttention.gamma gradient: sum(O * dout) (fastai layers.py SelfAttention: o = gamma * (h beta) + x). */
int unet_dot(const float* x, int x_cs, int x_co, const float* y, int y_cs, int y_co, long long P, int C, float* out,
             float* workspace, void* stream);

/* ----------------------------------------------------------------- loss --
 * CrossEntropyLossFlat(axis=1, weight=w) (fastai losses.py; train.py:195,211):
 * loss = sum w[y] * -log softmax(z)[y] / sum w[y]; activation softmax(dim=1),
 * decodes argmax(dim=1) (predict.py:193,232).
 * logits NHWC [P,C] (cs/co), targets int64 [P]. */
size_t unet_ce_workspace(long long P);   /* floats */
int unet_ce_fwd(const float* z, int z_cs, int z_co, const int64_t* target, const float* weight, long long P, int C,
                float* loss /*[1]*/, float* denom /*[1]*/, float* workspace, void* stream);
/* the same sums, not divided: numden[0] = sum w[y] * nll, numden[1] = sum w[y].  Tile-DDP all-reduces these two floats between the loss
 * forward and backward kernels (one cross-entropy over the global batch); a rank whose tiles carry only zero-weight classes contributes
 * 0 and 0 instead of a 0/0 quotient. */
int unet_ce_fwd_parts(const float* z, int z_cs, int z_co, const int64_t* target, const float* weight, long long P, int C,
                      float* numden /*[2]*/, float* workspace, void* stream);
/* dz = gscale * w[y] * (softmax(z) - onehot(y)) / denom ; gscale multiplies (loss scaling / DDP averaging) */
int unet_ce_bwd(const float* z, int z_cs, int z_co, const int64_t* target, const float* weight, long long P, int C,
                const float* denom, float gscale, float* dz, int dz_cs, int dz_co, void* stream);
/* The same three with ONE WEIGHT PER PIXEL, pixel_weight float [P] (never NULL), in place of the class weights: loss = sum pw * nll / sum pw,
 * parts = the two sums, dz = gscale * pw * (softmax(z) - onehot(y)) / denom.  A target outside [0, C) is ignored whatever its weight is.
 * Same kernels, reduction order and workspace (unet_ce_workspace): pw[p] == w[y(p)] reproduces the class-weighted results bit for bit. */
int unet_ce_fwd_pw(const float* z, int z_cs, int z_co, const int64_t* target, const float* pixel_weight, long long P, int C,
                   float* loss /*[1]*/, float* denom /*[1]*/, float* workspace, void* stream);
int unet_ce_fwd_parts_pw(const float* z, int z_cs, int z_co, const int64_t* target, const float* pixel_weight, long long P, int C,
                         float* numden /*[2]*/, float* workspace, void* stream);
int unet_ce_bwd_pw(const float* z, int z_cs, int z_co, const int64_t* target, const float* pixel_weight, long long P, int C,
                   const float* denom, float gscale, float* dz, int dz_cs, int dz_co, void* stream);
/* FocalLossFlat(gamma, axis=1): the alternative classification loss the reference's configuration names (params_and_main.py:87-89).  fastai 2.5.1
 * losses.FocalLoss: ce = w[y] * nll per pixel (F.cross_entropy(weight, reduction="none"); train.py:211 assigns the class weights to every
 * loss), loss = mean over ALL P pixels of (1 - exp(-ce))^gamma * ce.  dz = gscale * d loss / d z.  workspace = unet_ce_workspace(P) floats.
 * Where ce == 0 exactly and gamma < 1, torch's autograd returns NaN (0 * inf); these kernels return the limit, 0. */
int unet_focal_fwd(const float* z, int z_cs, int z_co, const int64_t* target, const float* weight, long long P, int C, float gamma,
                   float* loss /*[1]*/, float* workspace, void* stream);
int unet_focal_bwd(const float* z, int z_cs, int z_co, const int64_t* target, const float* weight, long long P, int C, float gamma,
                   float gscale, float* dz, int dz_cs, int dz_co, void* stream);
/* DiceLoss(axis=1, smooth, reduction, square_in_union): the fifth loss of the reference's configuration (params_and_main.py:16), fastai
 * losses.DiceLoss.  Logits z = B samples of HW pixels each (NHWC [B*HW, z_cs], slice z_co..z_co+C), targets int64 [B*HW]; per sample b
 * and class c, with p = softmax(z) and t = onehot(y) (a target outside [0, C) is an all-zero row):
 *   I = sum_hw p t,  U = sum_hw (p + t)  (square_in_union: sum_hw (p^2 + t)),  loss = sum_{b,c} 1 - (2 I + smooth) / (U + smooth),
 * divided by mean_div when mean_div > 0 (reduction 'mean': B * C; tile-DDP: the global count of the terms), mean_div = 0: 'sum'.
 * unet_dice_fwd writes loss[0] and coef [B][C][2] = (d loss / dI, d loss / dU) = (-2 / (U + s), (2 I + s) / (U + s)^2) / mean_div, which
 * unet_dice_bwd reads: dz = gscale * d loss / d z (gscale multiplies: loss scaling).  workspace = unet_dice_workspace(B, HW, C) floats.
 * C <= 64.  Deterministic: block partials per sample, summed in a fixed order in fp64. */
size_t unet_dice_workspace(int B, long long HW, int C);   /* floats */
int unet_dice_fwd(const float* z, int z_cs, int z_co, const int64_t* target, int B, long long HW, int C, float smooth, int square_in_union,
                  long long mean_div, float* loss /*[1]*/, float* coef /*[B*C*2]*/, float* workspace, void* stream);
int unet_dice_bwd(const float* z, int z_cs, int z_co, const int64_t* target, int B, long long HW, int C, int square_in_union,
                  const float* coef, float gscale, float* dz, int dz_cs, int dz_co, void* stream);
/* CombinedLoss(axis=1, smooth, alpha, gamma, reduction, square_in_union, weight) = FocalLossFlat(gamma, weight) + alpha * DiceLoss(smooth,
 * reduction, square_in_union), the compound loss fastai's documentation of DiceLoss ends with (gamma = 0: Dice + CE).  Both terms as defined
 * above, in one pass over the logits per direction with one softmax per pixel.  unet_combined_fwd writes the terms SEPARATELY:
 *   terms[0] = focal mean over all B * HW pixels,  terms[1] = Dice sum (divided by mean_div when mean_div > 0),
 * and the Dice coefficients coef [B][C][2] exactly as unet_dice_fwd; the caller forms terms[0] + alpha * terms[1] (under tile-DDP after
 * normalising each term in its own way).  unet_combined_bwd writes dz = fscale * d focal / d z + dscale * d dice / d z (fscale: loss scale /
 * world, dscale: loss scale * alpha).  A target outside [0, C) adds 0 to the focal sum, counts in its mean and has no focal gradient; it
 * is an all-zero one-hot row of the Dice term, whose gradient it keeps.  weight [C] or NULL feeds the focal term only.
 * workspace = unet_combined_workspace(B, HW, C) floats.  C <= 64.  Deterministic (no atomics, fixed-order fp64 sums). */
size_t unet_combined_workspace(int B, long long HW, int C);   /* floats */
int unet_combined_fwd(const float* z, int z_cs, int z_co, const int64_t* target, const float* weight, int B, long long HW, int C, float gamma,
                      float smooth, int square_in_union, long long mean_div, float* terms /*[2]*/, float* coef /*[B*C*2]*/, float* workspace,
                      void* stream);
int unet_combined_bwd(const float* z, int z_cs, int z_co, const int64_t* target, const float* weight, int B, long long HW, int C, float gamma,
                      int square_in_union, const float* coef, float fscale, float dscale, float* dz, int dz_cs, int dz_co, void* stream);
/* Regression mode (enable_regression, reference train.py:137-138,189-193; utils.py:145-147): n_out = 1, the loss is the mean over all
 * pixels of kind 0 = (z - t)^2 (MSELossFlat), 1 = |z - t| (L1LossFlat), 2 = SmoothL1(beta) (Smoothl1: beta 0.5).  z = channel z_co of
 * the NHWC output [P,z_cs], float targets [P]; workspace = unet_ce_workspace(P) floats.
 * dz = gscale * d loss / d z. */
int unet_regloss_fwd(const float* z, int z_cs, int z_co, const float* target, long long P, int kind, float beta,
                     float* loss /*[1]*/, float* workspace, void* stream);
int unet_regloss_bwd(const float* z, int z_cs, int z_co, const float* target, long long P, int kind, float beta, float gscale,
                     float* dz, int dz_cs, int dz_co, void* stream);
/* probs NCHW [N,C,H,W] (what Learner.predict returns, predict.py:196-203) and argmax uint8/int64 mask */
int unet_softmax_argmax(const float* z, int z_cs, int z_co, int N, int H, int W, int C,
                        float* probs_nchw /*or NULL*/, int64_t* argmax /*or NULL*/, void* stream);

/* ------------------------------------------------------- self-attention --
 * fastai SelfAttention (layers.py; DynamicUnet(self_attention=True), params_and_main.py:81-83): beta = softmax(f^T g, dim=1),
 * o = gamma * h beta + x.  The matrix products run on unet_conv2d / unet_conv2d_wgrad with per-image operands packed by
 * unet_pack_weights_strided; these two kernels are the softmax over one attention row (all key positions) and its adjoint. */
int unet_row_softmax(const float* x, int x_cs, int x_co, float* y, int y_cs, int y_co, long long P, int C, void* stream);
int unet_row_softmax_bwd(const float* y, int y_cs, int y_co, const float* dy, int dy_cs, int dy_co,
                         float* dx, int dx_cs, int dx_co, long long P, int C, void* stream);

/* ------------------------------------------------------------ optimiser --
 * fastai Adam (optimizer.py: weight_decay, average_grad(dampening), average_sqr_grad,
 * step_stat, adam_step) with decoupled wd, per-group lr (train.py:78-80, 247-250).
 * code[i] = group_id (bits 0-1) | do_wd << 2.  grad_scale multiplies g first. */
int unet_adam_step(float* p, const float* g, float* m, float* v, const uint8_t* code, long long n,
                   const float* lr /*[4] host*/, float mom, float sqr_mom, float eps, float wd, int step,
                   float grad_scale, void* stream);

/* hipGraph-friendly form: the hyper-parameter block (unet_adam_hyper_floats() floats, filled on the host by
 * unet_adam_fill_hyper and copied to the device by the caller before each replay) is read from device memory, so a captured
 * step can be replayed with a new lr / momentum / step count. */
int unet_adam_hyper_floats(void);
int unet_adam_fill_hyper(float* hyper_host, const float* lr /*[4]*/, float mom, float sqr_mom, float eps, float wd, int step,
                         float grad_scale);
int unet_adam_step_dev(float* p, const float* g, float* m, float* v, const uint8_t* code, long long n,
                       const float* hyper_dev, void* stream);

/* ------------------------------------------------- overlap-merge (predict) --
 * predict.py:284-326: sum softmax probabilities of overlapping tiles into a
 * mosaic + hit counter, divide, argmax. */
int unet_mosaic_accumulate(const float* probs_nchw, int C, int th, int tw, float* mosaic /*[C,MH,MW]*/,
                           int32_t* count /*[MH,MW]*/, int MH, int MW, int y0, int x0, void* stream);
int unet_mosaic_finalize(float* mosaic, const int32_t* count, int C, int MH, int MW, uint8_t* argmax, void* stream);
/* Gaussian-blended form of unet_mosaic_accumulate (the slab add of an N-rank merge): probs [C, th, tw] is added as fl(w * p) with
 * w = fl(wy[ty] * wx[tx]) (fp32 profile tables of th / tw entries on the device; a slab of the top th rows of a window passes the first
 * th entries of its vertical profile), w is added to wsum [MH, MW] and the hit counter is incremented.  C <= 64. */
int unet_mosaic_accumulate_weighted(const float* probs_nchw, int C, int th, int tw, const float* wy, const float* wx, float* mosaic,
                                    int32_t* count, float* wsum, int MH, int MW, int y0, int x0, void* stream);

/* --------------------------------------- sliding-window predict over a raster --
 * BASELINE.json configs[4]: the raster stays in HBM as the integers it was read as; windows are cut, scaled and merged on the device.
 * Replaces, with identical results, the host round trip create_tiles_unet.split_raster (create_tiles_unet.py:252-434) -> tile files
 * -> predict.save_predictions(merge=True) (predict.py:191-222, 257-334).
 * A source is band-sequential: sample (band c, row y, column x) of source s is src[s * src_stride + c * band_stride + y * row_stride + x].
 * A window table is int32 [n][4] on the device: {y0, x0, source index, unused}. */
#define UNET_RASTER_U8 0
#define UNET_RASTER_U16 1
#define UNET_RASTER_I16 2
#define UNET_RASTER_I32 3
#define UNET_RASTER_F32 4          /* cast through int32 like every tile the reference opens (data.py:24) */
/* create_tiles_unet.py:344-352: every band of a pixel becomes 0 where ANY band equals the raster's nodata value (in place) */
int unet_raster_nodata_zero(void* raster, int rtype, int bands, long long pixels, double nodata, void* stream);
/* create_tiles_unet.py:379: counts[j] = number of non-zero samples (all bands) of window j; the host drops windows with
 * counts[j] < bands * th * tw * (1 - max_empty) */
int unet_window_nonzero(const void* raster, int rtype, int bands, long long band_stride, int row_stride, const int32_t* windows, int n,
                        int th, int tw, unsigned long long* counts, void* stream);
/* x[j, y, x, x_co + c] = float(int32(sample)) / 255 (and / 255 once more when div255_twice: the reference's int16 rasters, utils.py:248-249
 * + IntToFloatTensor); x is an NHWC activation buffer [n, th, tw, x_cs] of storage type dtype (UNET_F32 | UNET_BF16).  Equals
 * open_npy + the transform + unet_nchw_to_nhwc of the same window bit for bit. */
int unet_window_gather(const void* src, int rtype, int bands, long long src_stride, long long band_stride, int row_stride,
                       const int32_t* windows, int n, int th, int tw, int div255_twice, void* x, int x_cs, int x_co, int dtype, void* stream);
/* predict.py:193-203 + 284-292 for a batch: window j's softmax probabilities (mode 0; the arithmetic of unet_softmax_argmax) or raw
 * values (mode 1, regression) of the fp32 NHWC logits z [n, th, tw, z_cs] are added to mosaic [C, MH, MW] at (y0 - origin_y,
 * x0 - origin_x) and the hit counter is incremented; only mosaic rows [row_lo, row_hi) are touched.  Contributions to one pixel are
 * added in window order (stream order across calls), so the result equals n successive unet_mosaic_accumulate calls bit for bit. */
int unet_mosaic_accumulate_windows(const float* z, int z_cs, int z_co, int C, int th, int tw, const int32_t* windows, int n, int origin_y,
                                   int origin_x, int mode, float* mosaic, int32_t* count, int MH, int MW, int row_lo, int row_hi,
                                   void* stream);
/* predict.py:306-334 on rows [row0, row0 + nrows): mosaic /= count where count > 0 (in place); argmax (uint8 [nrows, MW], may be NULL);
 * fill_host != NULL: pixels without a hit become *fill_host (regression nodata -9999, predict.py:312-315) */
int unet_mosaic_finalize_rows(float* mosaic, const int32_t* count, int C, int MH, int MW, int row0, int nrows, uint8_t* argmax,
                              const float* fill_host, void* stream);
/* Gaussian blending (predict.py blend="gaussian"): unet_mosaic_accumulate_windows where window k adds fl(w * p) for each value p it
 * adds there, w = fl(wy[Y - y0_k] * wx[X - x0_k]) from fp32 profile tables wy [th], wx [tw] on the device, and w is added to wsum
 * [MH, MW] (fp32, zero-initialised by the caller) in the same window order; the hit counter still counts windows. */
int unet_mosaic_accumulate_windows_weighted(const float* z, int z_cs, int z_co, int C, int th, int tw, const int32_t* windows, int n,
                                            int origin_y, int origin_x, int mode, float* mosaic, int32_t* count, int MH, int MW, int row_lo,
                                            int row_hi, const float* wy, const float* wx, float* wsum, void* stream);
/* unet_mosaic_finalize_rows with the weight sum as divisor: mosaic /= wsum where count > 0 (IEEE fp32 division), fill / argmax as there */
int unet_mosaic_finalize_rows_weighted(float* mosaic, const int32_t* count, const float* wsum, int C, int MH, int MW, int row0, int nrows,
                                       uint8_t* argmax, const float* fill_host, void* stream);

/* Test-time augmentation (TTA).  A D4 code g names one of the 8 symmetries of the square, by its action on the last two axes
 * [..., H, W] of a tensor: 0 x, 1 flip(x, [-1]), 2 flip(x, [-2]), 3 flip(x, [-2, -1]), 4 x^T, 5 rot90(x, 1, (-2, -1)),
 * 6 rot90(x, -1, (-2, -1)), 7 flip(x^T, [-2, -1]); the inverse of 5 is 6 and vice versa, every other code is its own inverse.  Codes
 * 4..7 need square windows / images (else UNET_E_BADARG).  Every map is an exact index permutation. */
/* unet_window_gather with window j written as g(window j) (same casts and divisions bit for bit) */
int unet_window_gather_oriented(const void* src, int rtype, int bands, long long src_stride, long long band_stride, int row_stride,
                                const int32_t* windows, int n, int th, int tw, int div255_twice, void* x, int x_cs, int x_co, int dtype,
                                int orient, void* stream);
/* unet_nchw_to_nhwc (dtype UNET_F32 | UNET_BF16 storage of y) with image n written as g(x[n]) */
int unet_nchw_to_nhwc_oriented(const float* x, void* y, int y_cs, int y_co, int N, int C, int H, int W, int dtype, int orient, void* stream);
/* acc [n, th, tw, acc_cs] (fp32, channels [0, C)) = (first ? 0 : acc) + g^-1(softmax(z)) (mode 0, the arithmetic of unet_softmax_argmax)
 * or + g^-1(z) (mode 1, regression), z the fp32 NHWC logits [n, th, tw, z_cs] of windows produced under code g = orient.  One thread per
 * acc pixel: the codes of a set add in launch order (no atomics).  finalize_k > 0 (the last code of a set of k): acc /= k (one rounded
 * division) in place, and probs (NCHW [n, C, th, tw], may be NULL) and argmax (int64 [n, th, tw], first maximum, may be NULL) are
 * written; with finalize_k == 0 both must be NULL. */
int unet_tta_accumulate(const float* z, int z_cs, int z_co, int n, int C, int th, int tw, int orient, int mode, int first, float* acc,
                        int acc_cs, int finalize_k, float* probs, int64_t* argmax, void* stream);

/* ------------------------------------------------------- training feed --
 * What learn.fit_one_cycle's loader does per batch on the host in the reference (train.py:345 -> data.py:18-28 open_npy: tile -> int32 ->
 * float; utils.py:239-295 SegmentationAlbumentationsTransform: / 255 for int8 data, / 255 twice for int16 data, flips on the first
 * ceil(B * n_transform_imgs) - B images; MaskBlock: int64 masks), done on the device on the INTEGERS of the tile files: the batch crosses
 * PCIe as uint8 / uint16 samples (1 / 2 bytes instead of 4 + 8 per pixel).  src = n staged tiles [n, bands, H, W] (masks: [n, H, W]) of
 * sample type rtype (UNET_RASTER_*), n <= 64 per call; image j is mirrored along x when bit j of hflip is set and along y for vflip.
 * unet_tiles_stage: dst_nchw [n, bands, H, W] fp32 = float(int32(sample)) / 255 [/ 255], bit-equal to the host arithmetic.
 * unet_mask_stage: dst [n, H, W] int64 (dst_f32 = 0, classification) or float (dst_f32 = 1, regression targets, data.py:98-99). */
int unet_tiles_stage(const void* src, int rtype, int n, int bands, int H, int W, int div255_twice, unsigned long long hflip,
                     unsigned long long vflip, float* dst_nchw, void* stream);
int unet_mask_stage(const void* src, int rtype, int n, int H, int W, unsigned long long hflip, unsigned long long vflip, void* dst, int dst_f32,
                    void* stream);
/* DiceMulti counters of a validation batch (fastai metrics.py DiceMulti; reference train.py:196), ACCUMULATED into counts [3][C] (uint64,
 * zeroed by the caller at the start of a validation pass): [0][c] += #(pred == c and targ == c), [1][c] += #(pred == c),
 * [2][c] += #(clamp(targ, 0, C - 1) == c).  C <= 64. */
int unet_dice_counts(const int64_t* pred, const int64_t* targ, long long P, int C, unsigned long long* counts, void* stream);

/* ---------------------------------------------------- geometric augmentation --
 * The rotate / transpose / shift-scale-rotate augmentations of unet_amd.augment (albumentations RandomRotate90, Transpose, Rotate,
 * ShiftScaleRotate: cv2.warpAffine per image on the host in the reference's pipeline, params_and_main.py:105-115) on a device batch.
 * Output pixel (x, y) of image j takes the source value at (m[0] x + m[1] y + m[2], m[3] x + m[4] y + m[5]), m = inv_maps_host + 6 j:
 * the INVERSE affine map, n x 6 fp32 in host memory, read at call time and passed in the kernel arguments (n <= 64).  Out of place
 * (src == dst is refused); the output has the input's size.  interp: 0 nearest (floor(s + 0.5)), 1 bilinear (fp32 weights, without cv2's
 * 1/32-pixel quantisation).  border: cv2 codes 0 constant (fill), 1 replicate, 2 reflect, 4 reflect-101, for coordinates any distance
 * outside the image.  Every tap is mapped into the image or replaced by fill; nothing is read or written outside src / dst.
 * unet_warp_affine: src / dst [n, C, H, W] fp32.
 * unet_warp_affine_mask: nearest always; src / dst [n, H, W] int64 (dst_f32 = 0, classification) or fp32 (dst_f32 = 1, regression).
 * Both return -1 before any launch on a null pointer, n outside 1..64, a size outside 1..2^24, an unknown interp / border, or a
 * non-finite map entry or fill. */
int unet_warp_affine(const float* src, float* dst, int n, int C, int H, int W, const float* inv_maps_host, int interp, int border, float fill,
                     void* stream);
int unet_warp_affine_mask(const void* src, void* dst, int dst_f32, int n, int H, int W, const float* inv_maps_host, int border, double fill,
                          void* stream);

/* -------------------------------------------------- non-rigid augmentation --
 * The field augmentations of unet_amd.augment (albumentations ElasticTransform, GridDistortion, OpticalDistortion: cv2.remap per image on
 * the host) on a device batch (csrc/warp_field.hip).  Output pixel p = (x, y) of image j takes the source value at pre_j * (p + d_j(p)):
 * d_j is the displacement of the launch-wide kind, zero where images[j].fired == 0, and pre_j the 2 x 3 inverse map of the D4 transforms
 * in front of the field transform (the identity 1 0 0 0 1 0 otherwise).  pre_j must be a D4 map of the H x W grid -- entries 0 / +-1,
 * offsets 0 or N - 1, x and y swapped only when H == W; anything else is refused.  Sampling commutes with such a map, so the kernel
 * applies it to the tap indices of p + d_j(p): bit for bit what permuting the image first and warping then gives.  images_host: n
 * descriptors in host memory, read at call time and passed in the kernel arguments (n <= UNET_FIELD_MAX_IMAGES).
 *   UNET_FIELD_DENSE    d = (field[j][0][y][x], field[j][1][y][x]); field [n, 2, H, W] fp32 on the device (not read for unfired images)
 *   UNET_FIELD_GRID     p + d = (xx[x], yy[y]): an axis of N entries is cut into cells of grid_step entries (the last one clipped at N, at
 *                       most UNET_FIELD_MAX_CELLS of them), and cell c runs from nodes[axis][c] to nodes[axis][c + 1] as
 *                       np.linspace(prev, cur, len) does, endpoint included (a cell of one entry gets prev); axis 0 is x
 *   UNET_FIELD_OPTICAL  with c = ((W - 1) / 2, (H - 1) / 2), u = (x - c_x) / W, v = (y - c_y) / H, r2 = u u + v v and k, dx, dy =
 *                       optical[0..2]: p + d = (x + (x - c_x) k (r2 + r2 r2) + dx, y + (y - c_y) k (r2 + r2 r2) + dy), which is
 *                       (W u kappa + c_x + dx, H v kappa + c_y + dy) for kappa = 1 + k r2 + k r2 r2
 * Coordinates are evaluated in fp64 and clamped to +-2^24 (a NaN of the field becomes -2^24); interp, border, fill, the exact copy of a
 * source on a grid point and the mask rule are those of unet_warp_affine / unet_warp_affine_mask.  Out of place.
 * unet_elastic_field writes the dense field [n, 2, H, W] of ElasticTransform: plane q (0 = dx, 1 = dy; plane 0 twice with same_dxdy) at
 * element e = y W + x starts as the noise 2 u - 1, u = ((w >> 8) + 0.5) 2^-24, w = word e % 4 of Philox4x32-10 under (key0, key1) at
 * counter (e / 4, q, 0, 0); it is filtered along rows, then along columns with the ksize (odd, 1..UNET_ELASTIC_MAX_KSIZE) taps of
 * taps_host, border reflect-101 repeated as often as the radius needs, and multiplied by alpha.  Unfired images get zeros.  workspace:
 * n 2 H W floats for the row-pass result (contents on return unspecified).  n <= UNET_ELASTIC_MAX_IMAGES per call; the field of an
 * image does not depend on the other images of the call.
 * All return -1 before any launch on a null pointer, sizes or counts out of range, an unknown kind / interp / border, a non-finite
 * parameter, a pre-map that is not a D4 map, or src == dst (field == dst, field == workspace). */
#define UNET_FIELD_MAX_IMAGES 16
#define UNET_FIELD_MAX_CELLS 16
#define UNET_ELASTIC_MAX_IMAGES 64
#define UNET_ELASTIC_MAX_KSIZE 401
enum { UNET_FIELD_DENSE = 0, UNET_FIELD_GRID = 1, UNET_FIELD_OPTICAL = 2 };
typedef struct unet_field_image {
    int32_t fired;
    float pre[6];
    float optical[3];                                  /* k, dx, dy (pixels) */
    float nodes[2][UNET_FIELD_MAX_CELLS + 1];          /* [0] x, [1] y */
} unet_field_image;
typedef struct unet_elastic_image {
    uint32_t key0, key1;
    float alpha;
    int32_t fired, same_dxdy;
} unet_elastic_image;
int unet_warp_field(const float* src, float* dst, int n, int C, int H, int W, int kind, const unet_field_image* images_host,
                    const float* field, int grid_step_x, int grid_step_y, int interp, int border, float fill, void* stream);
int unet_warp_field_mask(const void* src, void* dst, int dst_f32, int n, int H, int W, int kind, const unet_field_image* images_host,
                         const float* field, int grid_step_x, int grid_step_y, int border, double fill, void* stream);
int unet_elastic_field(float* field, float* workspace, int n, int H, int W, const unet_elastic_image* images_host, const float* taps_host,
                       int ksize, void* stream);

/* -------------------------------------------------- pixel-level augmentation --
 * The radiometric augmentations of unet_amd.augment (albumentations RandomBrightnessContrast, CoarseDropout, RandomGamma, GaussNoise,
 * ChannelDropout, ChannelShuffle, GaussianBlur, Blur) on a device batch [n, C, H, W] fp32 (csrc/pixel_aug.hip).  Per-image parameters
 * are read at call time from host memory and passed in the kernel arguments; no device allocation, no host wait, no atomics; each
 * thread stores only its own output elements.
 *
 * unet_pixel_ops, IN PLACE: image progs[j].image gets the program progs[j].ops[0 .. nops), applied in order to every pixel; images
 * without an entry are not touched (no block is launched for them).  nprog <= UNET_PIXEL_MAX_PROGS per call, image indices strictly
 * increasing.  Operands of an op (code & 0xff; f0, f1 fp32; u0, u1 uint32):
 *   BRIGHTNESS_CONTRAST  x = clamp(x * f0 [+ f1], 0, 1): product and sum rounded separately, the sum skipped when f1 == 0
 *   GAMMA                x = powf(fmaxf(x, 0), f0)
 *   GAUSS_NOISE          x = clamp(x + f0 + f1 z, 0, 1); z = the normal deviate of element e under the Philox4x32-10 key (u0, u1):
 *                        counter (e / 4, 0, 0, 0); word w -> u = ((w >> 8) + 0.5) 2^-24; words (0, 1) give r cos(2 pi u1), r sin(2 pi u1)
 *                        with r = sqrt(-2 ln u0) for elements 4q, 4q + 1, words (2, 3) the same for 4q + 2, 4q + 3.
 *                        e = (c H + y) W + x with UNET_PIXEL_PER_CHANNEL set in code, else y W + x (one deviate for all channels)
 *   FILL_RECTS           x = f0 inside any of rects[u0 .. u0 + u1): rows [y0, y1) x columns [x0, x1), every channel
 *   CHANNEL_DROP         x = f0 in the channels whose bit is set in u0
 *   CHANNEL_PERMUTE      channel c takes the value of channel (u0 | u1 << 32) >> 4 c & 15; C <= 16
 * unet_fill_rects_mask: the rectangles of sets[j] of mask sets[j].image set to fill; mask [n, H, W] int64 (dst_f32 = 0) or fp32 (1).
 * unet_blur_separable, OUT OF PLACE: dst[j] = src[j] filtered along rows and columns with the ksize[j] (odd, 1..31) taps
 * taps_host[31 j ..], border cv2 reflect-101 repeated as often as the radius needs (any H, W >= 1); ksize 1 with tap 1 copies bit for
 * bit.  n <= UNET_BLUR_MAX_IMAGES per call.
 * All return -1 before any launch on a null pointer, sizes or counts out of range, an unknown opcode, a non-finite operand, a
 * channel index >= C, or src == dst (blur). */
#define UNET_PIXEL_MAX_PROGS 8
#define UNET_PIXEL_MAX_OPS 8
#define UNET_PIXEL_MAX_RECTS 32
#define UNET_BLUR_MAX_IMAGES 16
#define UNET_BLUR_MAX_KSIZE 31
enum { UNET_PIXEL_BRIGHTNESS_CONTRAST = 1, UNET_PIXEL_GAMMA = 2, UNET_PIXEL_GAUSS_NOISE = 3, UNET_PIXEL_FILL_RECTS = 4,
       UNET_PIXEL_CHANNEL_DROP = 5, UNET_PIXEL_CHANNEL_PERMUTE = 6, UNET_PIXEL_PER_CHANNEL = 0x100 };
typedef struct unet_pixel_op {
    uint32_t code, u0, u1;
    float f0, f1;
} unet_pixel_op;
typedef struct unet_pixel_prog {
    uint32_t image, nops, nrects, reserved;
    unet_pixel_op ops[UNET_PIXEL_MAX_OPS];
    uint16_t rects[UNET_PIXEL_MAX_RECTS][4];           /* y0, x0, y1, x1 */
} unet_pixel_prog;
typedef struct unet_rect_set {
    uint32_t image, nrects;
    uint16_t rects[UNET_PIXEL_MAX_RECTS][4];
} unet_rect_set;
int unet_pixel_ops(float* x, int n, int C, int H, int W, const unet_pixel_prog* progs_host, int nprog, void* stream);
int unet_fill_rects_mask(void* mask, int dst_f32, int n, int H, int W, const unet_rect_set* sets_host, int nsets, double fill, void* stream);
int unet_blur_separable(const float* src, float* dst, int n, int C, int H, int W, const int* ksize_host, const float* taps_host,
                        void* stream);

/* ---------------------------------------------------- bf16-storage twins --
 * The HBM-bound kernels of the step with bf16 activation / gradient tensors (per-channel vectors, statistics, indices, losses stay
 * as in the fp32 entry point of the same name; arithmetic is fp32 per element, one rounding to bf16 at the store).  Used by
 * HipDynamicUnet(act_dtype="bf16"): BASELINE.json configs[1] "bf16" variant.  The logits head writes fp32 (unet_conv_desc.y_f32), so
 * unet_ce_fwd / unet_softmax_argmax are shared; unet_ce_bwd_bf16 writes the bf16 logit gradient. */
int unet_bn_stats_bf16(const unet_bf16* x, int x_cs, int x_co, long long P, int C, float* partial, void* stream);
int unet_affine_act_bf16(const unet_bf16* x, int x_cs, int x_co, const float* scale, const float* shift, const unet_bf16* x2, int x2_cs, int x2_co, const float* scale2, const float* shift2, unet_bf16* y, int y_cs, int y_co, long long P, int C, int relu, void* stream);
int unet_bn_bwd_reduce_bf16(const unet_bf16* dout, int d_cs, int d_co, const unet_bf16* out, int o_cs, int o_co, const unet_bf16* x, int x_cs, int x_co, const float* mean, const float* invstd, long long P, int C, float* partial, void* stream);
int unet_bn_bwd_apply_bf16(const unet_bf16* dout, int d_cs, int d_co, const unet_bf16* out, int o_cs, int o_co, const unet_bf16* x, int x_cs, int x_co, const float* mean, const float* invstd, const float* gamma, const float* c1, const float* c2, unet_bf16* dx, int dx_cs, int dx_co, unet_bf16* gout, int g_cs, int g_co, int g_accumulate, long long P, int C, void* stream);
int unet_maxpool3x3s2_bf16(const unet_bf16* x, int x_cs, int x_co, unet_bf16* y, int y_cs, int y_co, uint8_t* idx, int N, int IH, int IW, int C, int OH, int OW, void* stream);
int unet_maxpool3x3s2_bwd_bf16(const unet_bf16* dy, int dy_cs, int dy_co, const uint8_t* idx, unet_bf16* dx, int dx_cs, int dx_co, int N, int IH, int IW, int C, int OH, int OW, int accumulate, void* stream);
int unet_avgpool2_ceil_bf16(const unet_bf16* x, int x_cs, int x_co, unet_bf16* y, int y_cs, int y_co, int N, int IH, int IW, int C, int OH, int OW, void* stream);
int unet_avgpool2_ceil_bwd_bf16(const unet_bf16* dy, int dy_cs, int dy_co, unet_bf16* dx, int dx_cs, int dx_co, int N, int IH, int IW, int C, int OH, int OW, int accumulate, void* stream);
int unet_shuffle_blur_bf16(const unet_bf16* yc, int yc_cs, int yc_co, unet_bf16* X, int X_cs, int X_co, int N, int h, int w, int Cu, int do_blur, void* stream);
int unet_shuffle_bwd_xmask_bf16(const unet_bf16* dX, int dX_cs, int dX_co, const unet_bf16* X, int X_cs, int X_co, unet_bf16* dyc, int dyc_cs, int dyc_co, int N, int h, int w, int Cu, void* stream);
int unet_shuffle_blur_bwd_bf16(const unet_bf16* dX, int dX_cs, int dX_co, const unet_bf16* yc, int yc_cs, int yc_co, unet_bf16* dyc, int dyc_cs, int dyc_co, int N, int h, int w, int Cu, int do_blur, void* stream);
int unet_resize_nearest_bf16(const unet_bf16* x, int x_cs, int x_co, unet_bf16* y, int y_cs, int y_co, int N, int IH, int IW, int OH, int OW, int C, void* stream);
int unet_resize_nearest_bwd_bf16(const unet_bf16* dy, int dy_cs, int dy_co, unet_bf16* dx, int dx_cs, int dx_co, int N, int IH, int IW, int OH, int OW, int C, void* stream);
int unet_nchw_to_nhwc_bf16(const float* x, unet_bf16* y, int y_cs, int y_co, int N, int C, int H, int W, void* stream);
int unet_copy_slice_bf16(const unet_bf16* x, int x_cs, int x_co, unet_bf16* y, int y_cs, int y_co, long long P, int C, int accumulate, void* stream);
int unet_ce_bwd_bf16(const float* z, int z_cs, int z_co, const int64_t* target, const float* weight, long long P, int C, const float* denom, float gscale, unet_bf16* dz, int dz_cs, int dz_co, void* stream);
int unet_focal_bwd_bf16(const float* z, int z_cs, int z_co, const int64_t* target, const float* weight, long long P, int C, float gamma, float gscale, unet_bf16* dz, int dz_cs, int dz_co, void* stream);
int unet_ce_bwd_pw_bf16(const float* z, int z_cs, int z_co, const int64_t* target, const float* pixel_weight, long long P, int C, const float* denom, float gscale, unet_bf16* dz, int dz_cs, int dz_co, void* stream);
int unet_dice_bwd_bf16(const float* z, int z_cs, int z_co, const int64_t* target, int B, long long HW, int C, int square_in_union, const float* coef, float gscale, unet_bf16* dz, int dz_cs, int dz_co, void* stream);
int unet_combined_bwd_bf16(const float* z, int z_cs, int z_co, const int64_t* target, const float* weight, int B, long long HW, int C, float gamma, int square_in_union, const float* coef, float fscale, float dscale, unet_bf16* dz, int dz_cs, int dz_co, void* stream);
/* bf16 SelfAttention (round 3): the attention logits and the gradient of the attention weights stay fp32 (the products that make them write
 * fp32: unet_conv_desc.y_f32), the weights themselves and every other tensor are bf16 */
int unet_pack_weights_strided_bf16(const unet_bf16* w, long long so, long long sr, unet_bf16* wp, int O, int R, void* stream);
int unet_row_softmax_bf16(const float* x, int x_cs, int x_co, unet_bf16* y, int y_cs, int y_co, long long P, int C, void* stream);
int unet_row_softmax_bwd_bf16(const unet_bf16* y, int y_cs, int y_co, const float* dy, int dy_cs, int dy_co, unet_bf16* dx, int dx_cs, int dx_co, long long P, int C, void* stream);
/* Fused SelfAttention for bf16 storage (round 5; csrc/attention.hip): beta = softmax(f^T g, dim=1), o = h beta of fastai layers.py
 * SelfAttention (params_and_main.py:81-83, train.py:141-144) without the N x N matrix in HBM.  qkv: [B][N][cq] rows with F (query conv) at
 * channel 0, G (key conv) at dp, H (value conv) at 2 dp; dp <= 64, C <= 512, both multiples of 8 (unet_sa_fused_supported; other shapes run
 * the blockwise products above).  Rows are positions h * W + w of the NHWC tensors.
 *   unet_sa_pack_bf16   image of a channel slice blocked by 64 positions with positions innermost (unet_sa_pack_elems(N, cc) elements per
 *                       image): the operand of the products that sum over positions (H for O = P H; dO, G, F in the backward pass)
 *   unet_sa_fwd_bf16    O[j] = sum_i softmax_i(G_j . F_i) H_i (bf16) and lse[b][j] = log sum_i exp(G_j . F_i) (fp32), vpack = pack of H.
 *                       lse and D are [B][Np] with Np = 64 ceil(N / 64): the rows past N are written as 1e30 (their recomputed weight is 0)
 *   unet_sa_rowdot_bf16 D[b][j] = sum_c a[b][j][c] o[b][j][c] (fp32): the softmax-adjoint term dO_j . O_j (rows past N untouched: keep them finite)
 *   unet_sa_bwd_bf16    dqkv (all three slices: dF, dG, dH) from dO, lse, D; dopack / gpack / fpack = packs of dO, G, F.  Weights are
 *                       recomputed from lse; no atomics (run-to-run identical bits) */
int unet_sa_fused_supported(int dp, int C);
size_t unet_sa_pack_elems(int N, int cc);
int unet_sa_pack_bf16(const unet_bf16* x, int x_cs, int x_co, int cc, int B, int N, unet_bf16* out, void* stream);
int unet_sa_fwd_bf16(const unet_bf16* qkv, int cq, int dp, int C, int B, int N, const unet_bf16* vpack, unet_bf16* O, int o_cs, int o_co, float* lse, void* stream);
int unet_sa_rowdot_bf16(const unet_bf16* a, int a_cs, int a_co, const unet_bf16* o, int o_cs, int o_co, int B, int N, int C, float* D, void* stream);
int unet_sa_bwd_bf16(const unet_bf16* qkv, int cq, int dp, int C, int B, int N, const unet_bf16* dO, int do_cs, int do_co, const unet_bf16* dopack,
                     const unet_bf16* gpack, const unet_bf16* fpack, const float* lse, const float* D, unet_bf16* dqkv, void* stream);
int unet_relu_mask_bf16(const unet_bf16* g, int g_cs, int g_co, const unet_bf16* ref, int r_cs, int r_co, unet_bf16* y, int y_cs, int y_co, long long P, int C, void* stream);
int unet_dot_bf16(const unet_bf16* x, int x_cs, int x_co, const unet_bf16* y, int y_cs, int y_co, long long P, int C, float* out, float* workspace, void* stream);
int unet_cast_slice_bf16(const float* x, int x_cs, int x_co, unet_bf16* y, int y_cs, int y_co, long long P, int C, void* stream);

/* ------------------------------------------------- class-mask post-processing --
 * csrc/postprocess.hip (unet_amd/postprocess.py).  Masks are contiguous uint8 [H, W], H * W <= 2^31 - 1; labels / sizes are
 * int32 [H, W] (labels 16-byte aligned), keys uint64 [H, W]; counters is int32[4] on the device: {components merged, small components
 * not merged, give-up code, 0}.  frozen_class: -1 (none) or 0..255.  All workspace belongs to the caller.
 * unet_cc_label: labels[p] = the smallest linear index y * W + x of p's component (equal class, 4- / 8-adjacency); resets counters.
 *   Launches: tiles of unet_cc_tile_shape in LDS, border merge (atomicMin on the parent array = labels), flatten.
 * unet_cc_label_keys: the same labelling, by the same kernels, of a contiguous uint32 [H, W] key image at 4-adjacency (a component = equal
 *   keys): the flat zones of the instance split below.
 * unet_cc_sizes: sizes[l] = pixel count of the component with root label l, 0 at every other index.
 * unet_sieve_round: one round on `in`: label + sizes + per small component (size < min_pixels, class != frozen_class) the edge-adjacent
 *   component with the largest key (size << 32 | 0xFFFFFFFF - label), class != frozen_class, by a 64-bit atomicMax; a small component
 *   whose best key exceeds its own takes that neighbour's class in `out` (!= in).  counters[0] / [1] = components that merged / stayed
 *   small.  out == NULL: a counting pass (label, sizes, counters[1] = small components; keys may be NULL).  min_pixels >= 2.
 * unet_majority_filter: out (!= in) = the class with the highest count in the k x k window (k odd, 3..15) clipped to the raster; ties: the
 *   centre's class if tied, else the smallest id; frozen_class pixels neither vote nor change.
 * unet_postprocess_counters: copies counters to host4 and waits for the stream; a give-up code (a find / union loop that ran H * W
 *   steps) returns UNET_E_HIP with unet_last_error set.
 * Bad arguments return -1 before any launch. */
void unet_cc_tile_shape(int* th, int* tw);
int unet_cc_label(const uint8_t* mask, int H, int W, int connectivity, int32_t* labels, int32_t* counters, void* stream);
int unet_cc_label_keys(const uint32_t* keys, int H, int W, int32_t* labels, int32_t* counters, void* stream);
int unet_cc_sizes(const int32_t* labels, int H, int W, int32_t* sizes, void* stream);
int unet_sieve_round(const uint8_t* in, uint8_t* out, int H, int W, int connectivity, long long min_pixels, int frozen_class,
                     int32_t* labels, int32_t* sizes, unsigned long long* keys, int32_t* counters, void* stream);
int unet_majority_filter(const uint8_t* in, uint8_t* out, int H, int W, int k, int frozen_class, void* stream);
int unet_postprocess_counters(const int32_t* counters, int32_t* host4, void* stream);

/* ------------------------------------------------------- border distance --
 * csrc/edt.hip (unet_amd/border.py).  Masks are contiguous [B, H, W], uint8 or int64 (mask_is_int64), 1 <= H, W <= 8192.
 * A pixel is a BORDER pixel when one of its 4-neighbours inside the image has another value; with exclude >= 0 a pair in which either
 * value equals exclude does not count (-1: none).
 * unet_border_edt: d2 int32 [B, H, W] = the squared Euclidean distance to the nearest border pixel of the same image (0 on a border
 *   pixel), INT32_MAX in an image without one.  Exact and independent of the schedule (integers, no atomics).  Two launches: a column
 *   pass into the uint16 workspace (unet_edt_workspace BYTES, 2-byte aligned, the caller's), a row pass with the row in LDS.
 * unet_border_weight: pw[p] = class_w[y] + w0 * exp(-d2[p] / (2 sigma^2)), the weight map of the U-Net paper; class_w [C] or NULL (ones);
 *   a target outside [0, C) gives 0; d2 == INT32_MAX gives a border term of exactly 0.  One launch.
 * Bad arguments return -1 before any launch. */
size_t unet_edt_workspace(int B, int H, int W);   /* bytes; 0 for a shape outside the limits */
int unet_border_edt(const void* mask, int mask_is_int64, int B, int H, int W, int exclude, int32_t* d2, void* workspace, void* stream);
int unet_border_weight(const int32_t* d2, const int64_t* target, const float* class_w, int C, float w0, double sigma, long long P,
                       float* pw, void* stream);

/* ------------------------------------------- distance to the two nearest objects --
 * csrc/object_edt.hip (unet_amd/border.py).  Masks as above, with B * H * W <= 2^31 - 1.  A pixel is EXCLUDED when its value
 * equals exclude (-1: none) or lies outside [0, n_classes) (n_classes 1..256), BACKGROUND when it is not excluded and equals background
 * (0..255, != exclude), and an OBJECT pixel otherwise; an object is a 4-connected component of object pixels of one value in one image.
 * unet_object_edt: for a background pixel p, d1 / d2 int32 [B, H, W] = the smallest and the second smallest of delta(p, L) = min over the
 *   pixels q of object L of |p - q|^2 over the distinct objects L with delta <= radius^2 (radius 1..255); INT32_MAX where there is no
 *   such object and at object and excluded pixels.  pw float [B, H, W] = class_w[y] + w0 * exp(-(sqrt d1 + sqrt d2)^2 / (2 sigma^2)) with
 *   the exponent formed in fp64 as d1 + d2 + 2 sqrt(d1 d2) and rounded to fp32 once; class_w [n_classes] or NULL (ones); the second term
 *   is exactly 0 where d2 is INT32_MAX; a value outside [0, n_classes) gives 0.  d1 and d2 (both or neither) and pw may be NULL, not all.
 *   Launches: the key image (image << 8 | value for object pixels, a key of its own for every other pixel), unet_cc_label_keys on the
 *   stacked [B * H, W] key image, a column pass (per pixel the two nearest object pixels of its column with distinct labels within
 *   radius rows of the same image) and a row pass with the candidates of radius columns either side in LDS.  Integers only in the
 *   distances, no atomics outside the labelling, one thread per output: independent of the schedule.  No host sync; capturable.
 *   The workspace (unet_object_edt_workspace BYTES, 16-byte aligned, the caller's) holds keys, labels, candidates and the labelling's
 *   counters: 18 bytes per pixel.
 * Bad arguments return -1 before any launch. */
size_t unet_object_edt_workspace(int B, int H, int W);   /* bytes; 0 for a shape outside the limits */
int unet_object_edt(const void* mask, int mask_is_int64, int B, int H, int W, int background, int exclude, int n_classes, int radius,
                    void* workspace, int32_t* d1, int32_t* d2, const float* class_w, float w0, double sigma, float* pw, void* stream);

/* ------------------------------------------------------ GeoTIFF codecs --
 * Host-side (no device code) strip / tile decoders of unet_amd/tiffio.py.  Replaces what GDAL / rasterio do when the reference opens a
 * compressed raster (create_tiles_unet.py:252-434: gdal.Open / ReadAsArray; data.py:18-28: rasterio.open().read()).  Deflate is zlib.
 * Return the number of bytes written to dst (capacity cap), -1 on a malformed stream or overflow. */
long long unet_tiff_lzw_decode(const unsigned char* src, long long n, unsigned char* dst, long long cap);      /* TIFF 6.0 LZW (compression 5) */
long long unet_tiff_packbits_decode(const unsigned char* src, long long n, unsigned char* dst, long long cap); /* PackBits (compression 32773) */
/* The LZW encoder of the writer (same file, host-side): one strip of n bytes -> dst, the number of bytes written, or -1 instead of writing
 * past dst + cap.  The code stream is the one rule of DESIGN 3.16 (Clear first, early change, Clear when the next code would be 4094,
 * EOI, zero padding); unet_tiff_lzw_cap(n) = (3 * (n + n / 3836 + 4) + 1) / 2 bytes always suffice. */
long long unet_tiff_lzw_cap(long long n);
long long unet_tiff_lzw_encode(const unsigned char* src, long long n, unsigned char* dst, long long cap);

/* ---------------------------------------------------- GeoTIFF encoding on the device --
 * csrc/tiff_encode.hip (unet_amd/tiffenc.py): LZW strips of a device image, byte for byte what unet_tiff_lzw_encode writes.
 * The image is [P, H, W] samples of elem_size 1, 2 or 4 bytes; row_stride / plane_stride are in samples (W contiguous samples per row).
 * Strips hold rows_per_strip rows (the last one of a plane fewer); strip k = p * strips_per_plane + s is strip s of plane p.
 * unet_tiff_encode_strips: strips [first, first + count) -> scratch + j * slot_bytes for j = k - first, sizes[j] = encoded bytes.
 *   predictor 2: horizontal differencing per sample modulo 2^bits, applied while the input is staged.  slot_bytes: a multiple of 4, at
 *   least unet_tiff_lzw_cap(rows_per_strip * W * elem_size) -- the kernel never writes outside a slot; a slot that would overflow (it
 *   cannot, by the capacity rule) reports sizes[j] = 0xFFFFFFFF.  One wavefront per strip; deterministic, no atomics.
 * unet_tiff_compact_strips: out[offsets[j], offsets[j] + sizes[j]) = slot j, for count slots; offsets = exclusive prefix sum of sizes.
 * Bad arguments return -1 before any launch. */
int unet_tiff_encode_strips(const void* src, int elem_size, int P, int H, int W, long long row_stride, long long plane_stride,
                            int rows_per_strip, int predictor, long long first, int count, unsigned char* scratch, long long slot_bytes,
                            uint32_t* sizes, void* stream);
int unet_tiff_compact_strips(const unsigned char* scratch, long long slot_bytes, const uint32_t* sizes, const long long* offsets, int count,
                             unsigned char* out, long long out_bytes, void* stream);

/* -------------------------------------------- tiled GeoTIFFs with overviews on the device --
 * DESIGN 3.17.  unet_tiff_encode_tiles (csrc/tiff_encode.hip): the encoder of unet_tiff_encode_strips over square tiles of `tile` samples a
 *   side (a multiple of 16 in 16..1024).  Tile k = (p * tiles_down + j) * tiles_across + i, the TIFF order; tiles [first, first + count) ->
 *   scratch + j * slot_bytes, sizes[j].  Samples beyond the right / bottom edge of the image are zero; predictor 2 runs along the whole
 *   padded tile row.  slot_bytes: a multiple of 4, at least unet_tiff_lzw_cap(tile * tile * elem_size).  unet_tiff_compact_strips packs
 *   the slots as it packs strips.  unet_tiff_encode_tile_levels: one launch over the tiles of up to UNET_TIFF_MAX_LEVELS images of the same
 *   sample type and plane count, one image after the other in the order given (a writer passes the pyramid smallest level first), so
 *   that the small levels of a pyramid do not cost a launch -- one tile's latency -- each; unet_tiff_encode_tiles is its one-image form.
 * unet_tiff_reduce_level (csrc/tiff_pyramid.hip): the next overview level of [P, H, W] samples (strides in samples, W contiguous samples per
 *   row) -> dst, dense [P, ceil(H / 2), ceil(W / 2)].  kind: 0 unsigned, 1 signed, 2 float (4 bytes); resampling: 0 nearest, 1 mode
 *   (integers only), 2 average; the rule per clipped 2 x 2 block is stated at the top of csrc/tiff_pyramid.hip.  has_nodata / nodata: samples
 *   equal to nodata (NaN: NaN samples) do not count, a block without a valid sample gives nodata; an integer nodata must be a sample of the
 *   type.  H x W must be larger than 1 x 1.  Deterministic, no atomics.
 * Bad arguments return -1 before any launch. */
#define UNET_TIFF_MAX_LEVELS 32
typedef struct unet_tiff_level {
    const void* src;
    long long row_stride, plane_stride; /* in samples */
    int H, W;
} unet_tiff_level;
int unet_tiff_encode_tiles(const void* src, int elem_size, int P, int H, int W, long long row_stride, long long plane_stride, int tile,
                           int predictor, long long first, int count, unsigned char* scratch, long long slot_bytes, uint32_t* sizes,
                           void* stream);
int unet_tiff_encode_tile_levels(const unet_tiff_level* levels, int nlevels, int elem_size, int P, int tile, int predictor, long long first,
                                 int count, unsigned char* scratch, long long slot_bytes, uint32_t* sizes, void* stream);
int unet_tiff_reduce_level(const void* src, int elem_size, int kind, int P, int H, int W, long long row_stride, long long plane_stride,
                           int resampling, int has_nodata, double nodata, void* dst, void* stream);

/* --------------------------------------------------------- polygon rings --
 * Ring tracing of a labelled class mask (csrc/vectorize.hip, unet_amd/vectorize.py).  mask / labels are contiguous [H, W] with
 * H * W <= 2^31 - 1; labels are those of unet_cc_label at connectivity 4, or any other image in which every segment is 4-connected, of
 * one class and labelled by the smallest linear index of its pixels (unet_inst_canonical writes such an image).  Sides: N=0 W=1 S=2 E=3; the dense id of an edge is 4 p + s, its
 * compact index offs[p] + popcount(flags[p] & ((1 << s) - 1)).  E edges, R rings, V vertices, all in 1..2^31 - 1.
 * vec_flags: flags[p] bit s = side s of pixel p is a boundary edge (the neighbour is outside or has another label); 0 where the
 *   pixel's class has its bit set in exclude8 (256 bits as 8 words, NULL: none).
 * vec_scan: out[i] = sum over j < i of popcount(in[j] & 15); blocks holds vec_scan_words(n) words, the last one receives the total.
 * vec_read: copies `count` (1..64) int64 words to the host and waits for the stream: the host reads of a call.
 * vec_succ: succ[e] = the first existing of left (same pixel, side s + 1), straight (pixel ahead, side s), right (pixel diagonally
 *   ahead on the outer side, side s - 1); corner[e] = 1 unless it went straight.
 * vec_min_rounds: init != 0: m_a = e, nxt_a = succ.  Then `rounds` Jacobi doubling rounds m'[e] = min(m[e], m[nxt[e]]),
 *   nxt'[e] = nxt[nxt[e]]: round r reads set a (r even) or b (r odd), writes the other, and sets changed[r] = 1 if any m fell.  A round
 *   that changed nothing has every m at its cycle's minimum; ceil(log2 E) rounds always reach that.
 * vec_swap: at every interior vertex whose diagonal pixels share a label that the other two do not have: if the two edges of that label
 *   that END there have one `ring` value, their successors are exchanged.
 * vec_rank_init / vec_rank_rounds: every cycle cut at its leader (ring[e] == e): steps / area = edges, and twice the signed area, from e
 *   up to the leader, by the same doubling and the same changed words; mark[e] = 1 at leaders.
 * vec_ring_info: per ring r = ridx[leader]: its label, edge count and signed area.
 * vec_place: pos[e] = ring_base[r] + rank of e in its ring (leader = 0), corner_ord[pos[e]] = corner[e].
 * vec_emit: xy[voff[pos[e]]] = the end vertex (x, y) of every corner edge e.
 * No atomic decides a position.  Bad arguments return -1 before any launch. */
int unet_vec_flags(const uint8_t* mask, const int32_t* labels, int H, int W, const uint32_t* exclude8, uint8_t* flags, void* stream);
long long unet_vec_scan_words(long long n);
int unet_vec_scan(const uint8_t* in, long long n, int32_t* out, long long* blocks, void* stream);
int unet_vec_read(const long long* dev, int count, long long* host, void* stream);
int unet_vec_succ(const uint8_t* flags, const int32_t* offs, int H, int W, long long E, int32_t* succ, uint8_t* corner, void* stream);
int unet_vec_min_rounds(const int32_t* succ, long long E, int32_t* m_a, int32_t* nxt_a, int32_t* m_b, int32_t* nxt_b, int init, int rounds,
                        int32_t* changed, void* stream);
int unet_vec_swap(const int32_t* labels, const uint8_t* flags, const int32_t* offs, int H, int W, const int32_t* ring, int32_t* succ,
                  void* stream);
int unet_vec_rank_init(const uint8_t* flags, const int32_t* offs, int H, int W, const int32_t* succ, const int32_t* ring, int32_t* steps,
                       int32_t* nxt, long long* area, uint8_t* mark, long long E, void* stream);
int unet_vec_rank_rounds(long long E, int32_t* steps_a, int32_t* nxt_a, long long* area_a, int32_t* steps_b, int32_t* nxt_b, long long* area_b,
                         int rounds, int32_t* changed, void* stream);
int unet_vec_ring_info(const uint8_t* flags, const int32_t* offs, const int32_t* labels, int H, int W, const int32_t* succ, const int32_t* ring,
                       const int32_t* ridx, const int32_t* steps, const long long* area, long long R, int32_t* ring_label, long long* ring_len,
                       long long* ring_area, void* stream);
int unet_vec_place(const int32_t* ring, const int32_t* steps, const int32_t* ridx, const long long* ring_base, const long long* ring_len,
                   const uint8_t* corner, long long E, long long R, int32_t* pos, uint8_t* corner_ord, void* stream);
int unet_vec_emit(const uint8_t* flags, const int32_t* offs, int H, int W, const uint8_t* corner, const int32_t* pos, const int32_t* voff,
                  long long E, long long V, int32_t* xy, void* stream);

/* ---------------------------------------------------- ring simplification --
 * Arc-based Douglas-Peucker on the traced rings (csrc/simplify.hip, unet_amd/vectorize.py).  C candidates (corners and the
 * nodes a ring passes) lie in ring order: vec_place / vec_scan / vec_emit run on the marks of simp_marks give their coordinates cxy.
 * simp_marks: cand[e] bit 0 = the end vertex of edge e is a candidate, bit 4 = it is a node (at least 3 of its 4 unit segments are
 *   borders between labels, outside the raster being one label, or it is a raster corner).
 * simp_gather: cring[k] = ring index, cnode[k] = node mark of candidate k = coff[pos[e]].
 * simp_closed: per ring the node count and the anchor (its first node by (y, x), else its candidate with the smallest (y, x)); for rings
 *   with fewer than 2 nodes the candidate farthest from the anchor (squared distance, ties to the smallest (y, x)).  Then keep[k] = node,
 *   anchor or far point, and lo / hi = k for kept candidates, else the cyclic neighbours within the ring (cs = first candidate, cn =
 *   candidate count per ring).  nnodes, akey, fard, fark are R-entry work arrays.
 * simp_near_rounds: Jacobi doubling lo' = lo[lo], hi' = hi[hi] between two buffer sets, changed[r] as in vec_min_rounds; settles at the
 *   nearest kept candidate before / after.
 * simp_dp_rounds: `rounds` rounds.  Each: every live candidate takes |c|, c = (Q - P) x (Z - P) against its segment lo .. hi; the segment's
 *   maximum of (|c|, smallest (y, x)) is kept iff 256 c^2 > q^2 |Q - P|^2 (128-bit, q in sixteenths of a pixel, 0..65536); its segment
 *   splits there, or its whole interior is dropped.  first != 0 on the first call.  changed[r] = 1 if round r still had a live segment.
 *   key, slot (C words each) and win (C) are work arrays.
 * simp_emit: xy[vbase[r] + koff[k] - kstart[r]] = cxy[k], vring = newring[r], for kept candidates of rings with newring[r] >= 0.
 * simp_area: area2[r] = sum of x1 y0 - x0 y1 over the ring's consecutive vertices (twice the signed area).
 * Atomics take minima, maxima and exact integer sums only.  Bad arguments return -1 before any launch. */
int unet_simp_marks(const int32_t* labels, const uint8_t* flags, const int32_t* offs, const uint8_t* corner, int H, int W, long long E,
                    uint8_t* cand, void* stream);
int unet_simp_gather(const int32_t* ring, const int32_t* ridx, const int32_t* pos, const int32_t* coff, const uint8_t* cand, long long E,
                     long long R, long long C, int32_t* cring, uint8_t* cnode, void* stream);
int unet_simp_closed(const int32_t* cxy, const int32_t* cring, const uint8_t* cnode, const int32_t* cs, const int32_t* cn, long long C,
                     long long R, int W, int32_t* nnodes, unsigned long long* akey, unsigned long long* fard, unsigned long long* fark,
                     uint8_t* keep, int32_t* lo, int32_t* hi, void* stream);
int unet_simp_near_rounds(long long C, int32_t* lo_a, int32_t* hi_a, int32_t* lo_b, int32_t* hi_b, int rounds, int32_t* changed, void* stream);
int unet_simp_dp_rounds(const int32_t* cxy, const int32_t* cring, const int32_t* cn, long long C, long long R, int W, int q, int first, int rounds,
                        uint8_t* keep, int32_t* lo, int32_t* hi, unsigned long long* key, unsigned long long* slot, int32_t* win,
                        int32_t* changed, void* stream);
int unet_simp_emit(const int32_t* cxy, const int32_t* cring, const uint8_t* keep, const int32_t* koff, const int32_t* kstart,
                   const long long* vbase, const int32_t* newring, long long C, long long R, long long V, int32_t* xy, int32_t* vring,
                   void* stream);
int unet_simp_area(const int32_t* xy, const int32_t* vring, const long long* ring_start, long long V, long long R, long long* area2,
                   void* stream);

/* --------------------------------------------------------- instance split --
 * Touching objects of one class split along the ridges of a capped distance transform (csrc/instances.hip, unet_amd/instances.py, DESIGN
 * 3.20, where the rules are).  mask is a contiguous uint8 [H, W], H * W <= 2^31 - 1 = n; every other image is [H, W] of the type given.
 * A zone / segment is named by the linear index of one of its pixels, its root (root[p] == p there); per-zone and per-segment arrays are
 * pixel-sized and used at the roots only.  partial: unet_inst_partials() int64 words; their sum is the count the call reports.
 * inst_distance: keys[p] = class << 16 | h(p), h = min(R^2, squared distance to the nearest pixel of another value inside the raster) for
 *   the classes of split8 (256 bits as 8 words), 0 for the others.  Two launches: g (uint8 workspace) = the horizontal distance capped at R
 *   = radius (1..255), 4 x 256 px per block with 4 x (256 + 510) bytes of LDS; then columns, 64 x 32 px per block with (64 + 2 R) x 32 x 2
 *   bytes of dynamic LDS.  unet_inst_tile_shapes gives those tile sizes.
 * inst_check_labels: *bad = 1 unless for every p: 0 <= labels[p] <= p, labels[labels[p]] == labels[p], mask[labels[p]] == mask[p].
 * inst_ascent: zone = unet_cc_label_keys(keys).  zkey[Z] = max over the pixels u 4-adjacent to a pixel of Z, of Z's class and higher than Z,
 *   of (h(u) << 32 | ~u); ptr[Z] = zone[u] of that maximum, or Z for a zone without one (a seed).  partial: seeds.
 * inst_ptr_rounds: `rounds` (0..64) Jacobi rounds b[r] = a[a[r]] at the roots r of `root`, reading ptr_a in even rounds and ptr_b in odd ones;
 *   changed[k] = 1 if round k moved a pointer (the words of vec_min_rounds).  A round behind one that moved nothing returns at once: both
 *   buffers hold the settled pointers then, and its own word stays 0.
 * inst_gather: out[p] = ptr[root[p]]; out may be root.
 * inst_merge_round: on the segments seg (updated in place): peak[A] = max h; best[A] = max over the 4-adjacent pairs (p in A, r in B != A) of
 *   equal class of (min(h(p), h(r)) << 32 | ~B); A points to B = best(A) iff 256 (peak - pass) - q^2 = L gives L < 0 or L^2 < 1024 q^2 pass
 *   (int64; q = depth in sixteenths of a pixel, 0..4080) and (peak(A), -A) < (peak(B), -B); `doublings` (1..32, at least log2 of the segment
 *   count) rounds of inst_ptr_rounds, with their words in changed (`doublings` words), follow every chain to its end, then
 *   seg[p] = ptr[seg[p]].  partial: the segments that merged.
 * inst_canonical: lowest[A] = the smallest p in A (atomic minimum), labels[p] = lowest[seg[p]].  partial: segments.
 * inst_marks / inst_ids: mark[p] = 1 where labels[p] == p and the class is in split8; with offs = unet_vec_scan(mark), ids[p] = offs[labels[p]]
 *   + 1 for the classes of split8 and 0 for the others: dense ids in ascending label order.
 * Atomics take maxima and minima of integers only.  Bad arguments return -1 before any launch. */
void unet_inst_tile_shapes(int* row_th, int* row_tw, int* col_th, int* col_tw);
int unet_inst_partials(void);
int unet_inst_distance(const uint8_t* mask, int H, int W, const uint32_t* split8, int radius, uint8_t* g, uint32_t* keys, void* stream);
int unet_inst_check_labels(const uint8_t* mask, const int32_t* labels, int H, int W, long long* bad, void* stream);
int unet_inst_ascent(const uint32_t* keys, const int32_t* zone, int H, int W, unsigned long long* zkey, int32_t* ptr, long long* partial,
                     void* stream);
int unet_inst_ptr_rounds(const int32_t* root, long long n, int32_t* ptr_a, int32_t* ptr_b, int rounds, int32_t* changed, void* stream);
int unet_inst_gather(const int32_t* root, const int32_t* ptr, long long n, int32_t* out, void* stream);
int unet_inst_merge_round(const uint32_t* keys, int32_t* seg, int H, int W, int q, int doublings, int32_t* peak, unsigned long long* best,
                          int32_t* ptr_a, int32_t* ptr_b, int32_t* changed, long long* partial, void* stream);
int unet_inst_canonical(const int32_t* seg, long long n, int32_t* lowest, int32_t* labels, long long* partial, void* stream);
int unet_inst_marks(const uint8_t* mask, const int32_t* labels, long long n, const uint32_t* split8, uint8_t* mark, void* stream);
int unet_inst_ids(const uint8_t* mask, const int32_t* labels, const int32_t* offs, long long n, const uint32_t* split8, uint32_t* ids,
                  void* stream);

/* ------------------------------------------------------- polygon burning --
 * Rings burnt into a uint8 [H, W] class mask (csrc/rasterize.hip, unet_amd/rasterize.py, DESIGN 3.21, where the rules are): the pixel
 * centre decides, the fill is even-odd over the rings of a feature, the feature with the highest index wins.  xy holds V vertices (x, y) as
 * int32 fixed point with 8 fractional bits, |x|, |y| <= 2^29; ring_start (R + 1 words) is the CSR of the rings over the vertices;
 * vring[i] = the ring of vertex i; ring_feature[r] = the feature of ring r; values[f] = the burn value of feature f, F < 2^23 features.
 * 1 <= H, W < 2^20; V, R and the number of crossings M are in 1..2^31 - 1.  Edge i runs from vertex i to the next vertex of its ring (the
 * first one behind the last); rings of fewer than 3 vertices have no edges.
 * ras_count: counts[i] = the rows y of 0 .. H - 1 with min(Y0, Y1) <= 256 y + 128 < max(Y0, Y1) of edge i.  info (2 words) is reset;
 *   info[1] gains bit 0 if a coordinate is outside +-2^29 and bit 1 if ring_start / vring do not hold a vertex (such vertices count 0).
 * ras_scan: offs = the exclusive scan of counts in int64, info[0] = the total; blocks holds unet_ras_scan_words(n) words.
 * ras_emit: keys[offs[i] + t] = ring_feature << 40 | y << 20 | k for the t-th row y of edge i, k = ceil((X* - 128) / 256) clamped to 0 .. W,
 *   X* = X0 + (256 y + 128 - Y0)(X1 - X0) / (Y1 - Y0) exactly (int64 floor division); positions outside 0 .. M - 1 are not written.
 * ras_spans: the plane ([H, W] uint32) and *bad are zeroed; then for the sorted keys every pair 2j, 2j + 1 of one (feature, row) takes the
 *   maximum of (feature + 1) << 8 | values[feature] into plane[row, k0 .. k1 - 1], one wavefront per pair.  Pairs whose keys differ above
 *   bit 20, or name a feature, row or column outside F, H, W, are counted in *bad and burn nothing.  M = 0: the two resets only.
 * ras_resolve: out[p] = plane[p] ? plane[p] & 255 : (keep ? out[p] : fill), in 16-byte accesses where plane and out are 16-byte aligned.
 * The one atomic is a maximum of integers.  Bad arguments return -1 before any launch. */
int unet_ras_count(const int32_t* xy, const long long* ring_start, const int32_t* vring, long long V, long long R, int H, int32_t* counts,
                   long long* info, void* stream);
long long unet_ras_scan_words(long long n);
int unet_ras_scan(const int32_t* counts, long long n, long long* offs, long long* blocks, long long* info, void* stream);
int unet_ras_emit(const int32_t* xy, const long long* ring_start, const int32_t* vring, const int32_t* ring_feature, long long V, long long R,
                  int H, int W, const long long* offs, long long M, long long* keys, void* stream);
int unet_ras_spans(const long long* keys, long long M, const uint8_t* values, long long F, int H, int W, uint32_t* plane, long long* bad,
                   void* stream);
int unet_ras_resolve(const uint32_t* plane, int H, int W, int fill, int keep, uint8_t* out, void* stream);
/* ras_resolve_ids: ids[p] = plane[p] ? (plane[p] >> 8) - 1 : -1 (int32 [H, W]): the feature that owns each pixel, in 16-byte accesses where
 * plane and ids are 16-byte aligned. */
int unet_ras_resolve_ids(const uint32_t* plane, int H, int W, int32_t* ids, void* stream);

/* ------------------------------------------------------ zonal statistics --
 * The joint histogram of a zone plane and a class mask (csrc/zonal.hip, unet_amd/zonal.py, DESIGN 3.22, where the rules are).  zones is
 * int32 [H, W] (-1 = no zone, else 0 .. Z - 1), mask uint8 [H, W] (values 0 .. C - 1), labels int32 [H, W] or null (labels[p] = the smallest
 * linear index of the object of pixel p; p is an anchor iff labels[p] == p; with labels H * W <= 2^31 - 1).  1 <= H, W < 2^20, 1 <= Z < 2^23,
 * 1 <= C <= 256, Z * C < 2^31.  counts and objects are uint64 [Z, C] and ZEROED BY THE CALLER; objects is null exactly when labels is.
 * zonal_counts: counts[z, c] += the pixels with zone z and mask value c; objects[z, c] += the anchors among them.  A pixel whose mask value
 *   is >= C (bit 0) or whose zone lies outside -1 .. Z - 1 (bit 1) is counted nowhere and sets that bit in *bad, which is reset first.
 *   Z * C <= unet_zonal_lds_bins(): every workgroup counts into a private table of uint32 bins in LDS (it sees fewer than 2^31 pixels) and
 *   adds its non-zero bins to counts; otherwise the adds go to counts directly.  Every add is an integer atomic add, so the result does
 *   not depend on the order of arrival.  16-byte accesses where zones and labels are 16-byte and mask 4-byte aligned; no access outside the
 *   H * W elements.  Bad arguments return -1 before any launch. */
int unet_zonal_lds_bins(void);
int unet_zonal_counts(const int32_t* zones, const uint8_t* mask, const int32_t* labels, int H, int W, int Z, int C, long long* counts,
                      long long* objects, long long* bad, void* stream);

/* ------------------------------------------------------ zonal statistics of a float plane --
 * Count, sum, sum of squares, minimum and maximum of a float32 plane per zone (csrc/zonal_values.hip, unet_amd/zonal.py, DESIGN 3.25, where
 * the rules are).  zones as above, values float32 [H, W]; 1 <= H, W < 2^20, H * W <= 2^31 - 1, 1 <= Z < 2^23.  A pixel is valid iff its zone
 * lies in 0 .. Z - 1, its value is finite and, with has_nodata = 1, differs from nodata.
 * zonal_absmax: *absmax (one 64-bit word, reset first) = the largest bit pattern of |v| over the valid pixels, 0 where there is none: a maximum per
 *   wavefront, then one unsigned atomic maximum each.
 * zonal_values: sums (uint64 [5, Z]: pixels, valid, sum_q, sq_lo, sq_hi; sum_q in two's complement) and minmax (float32 [2, Z]: min, max),
 *   both initialised here.  pixels counts every pixel of a zone, the others its valid pixels: q = rint(double(v) * 2^shift), half to even,
 *   -98 <= shift <= 178, and q^2 = hi * 2^30 + lo with 0 <= lo < 2^30, split before anything is summed, so that with |q| <= 2^30 every sum
 *   stays within 2^61.  min and max are the exact float32 extremes (unsigned atomics on the order-preserving image of the bits, decoded in
 *   place by a last launch); a zone without a valid pixel holds +inf and -inf.  *bad is reset and gains bit 1 for a zone outside
 *   -1 .. Z - 1 (counted nowhere) and bit 2 for a valid pixel with |q| > 2^30 (left out of the sums).  Every accumulation is an integer
 *   atomic add, minimum or maximum, so the result does not depend on the order of arrival.  16-byte accesses where zones and values are
 *   16-byte aligned; no access outside the H * W elements.  Bad arguments return -1 before any launch. */
int unet_zonal_absmax(const int32_t* zones, const float* values, int H, int W, int Z, int has_nodata, float nodata, long long* absmax,
                      void* stream);
int unet_zonal_values(const int32_t* zones, const float* values, int H, int W, int Z, int has_nodata, float nodata, int shift,
                      long long* sums, float* minmax, long long* bad, void* stream);

/* ------------------------------------------------------ object attributes --
 * A keyed reduction per object over a label image (csrc/objects.hip, unet_amd/objects.py, DESIGN 3.23, where the rules are).  mask is uint8
 * [H, W], labels int32 [H, W] (labels[p] = the smallest linear index of the object of pixel p; p is an anchor iff labels[p] == p), 1 <= H, W
 * < 2^20, H * W <= 2^31 - 1.  exclude8: the excluded classes, 256 bits as 8 words.  The P objects are the anchors of the other classes in
 * ascending order; offs = unet_vec_scan of their marks (unet_inst_marks with the kept classes), so offs[L] is the index of the object with
 * anchor L.
 * obj_compact: label[offs[p]] = p and cls[offs[p]] = mask[p] at every marked p; indices outside 0 .. P - 1 are not written.
 * obj_accumulate: sums (uint64 [P, 5]) = pixels, sum of columns, sum of rows, edges_v, edges_h of every object, bbox (int32 [P, 4]) = x0, y0,
 *   x1, y1 half open; both are initialised here.  *bad is reset and gains bit 0 for a label outside 0 .. H * W - 1, bit 1 for
 *   labels[labels[p]] != labels[p], bit 2 for mask[labels[p]] != mask[p]; such pixels are counted nowhere and nothing is stored outside the
 *   tables.  P = 0 (sums, bbox may be null): the check alone.
 * obj_point: point[k] = the pixel of object k that minimises ((x - cx)^2 + (y - cy)^2, y W + x), cx = sum_x / pixels, cy = sum_y / pixels
 *   (floored), from the complete sums; key64 (uint64 [P]) is workspace; bad is the word of obj_accumulate on the same planes, which made
 *   the check of the input: with a bit set the passes do nothing.  One pass where unet_obj_point_packed(H, W) (the squared distance
 *   stays below 2^33 and packs with the index into 64 bits), two minimum passes otherwise.
 * Every accumulation is an integer atomic add, minimum or maximum.  16-byte accesses where labels is 16-byte and mask 4-byte aligned; no
 * access outside the H * W elements.  Bad arguments return -1 before any launch. */
int unet_obj_point_packed(int H, int W);
int unet_obj_compact(const uint8_t* mask, const uint8_t* mark, const int32_t* offs, long long n, long long P, int32_t* label, uint8_t* cls,
                     void* stream);
int unet_obj_accumulate(const uint8_t* mask, const int32_t* labels, const int32_t* offs, int H, int W, const uint32_t* exclude8, long long P,
                        long long* sums, int32_t* bbox, long long* bad, void* stream);
int unet_obj_point(const uint8_t* mask, const int32_t* labels, const int32_t* offs, int H, int W, const uint32_t* exclude8, long long P,
                   const long long* sums, const long long* bad, long long* key64, int32_t* point, void* stream);

/* ------------------------------------------- float statistics per object --
 * Count, sum, sum of squares, minimum and maximum of a float32 plane per object, with the pixel of each extreme (csrc/object_values.hip,
 * unet_amd/objects.py, DESIGN 3.26, where the rules are).  mask, labels, offs, exclude8 and P are those of obj_accumulate; values is float32
 * [H, W].  A pixel is valid iff its class is not excluded, its value is finite and, with has_nodata, differs from nodata.
 * obj_absmax: *absmax (one 64-bit word, reset first) = the largest bit pattern of |v| over the valid pixels, 0 where there is none.  It reads the
 *   mask and the values only.
 * obj_values: table (uint64 [6, P], initialised here): rows 0 .. 3 are valid, sum_q (two's complement), sq_lo and sq_hi of every object under
 *   q = rint(double(v) * 2^shift), half to even, -98 <= shift <= 178, q^2 = hi * 2^30 + lo; rows 4 and 5 are min and max: while the pass runs
 *   key(v) << 32 | p under an unsigned atomic minimum and key(v) << 32 | (0xFFFFFFFF - p) under an unsigned atomic maximum (key: the
 *   order-preserving image of the float bits, p the linear index), so each extreme comes with the smallest index that attains it; a last
 *   launch decodes them in place to the float32 bits in the low half of the word and the int32 index in the high half (+inf, -inf and -1
 *   for an object without a valid pixel).  *bad is reset and gains the three bits of obj_accumulate (such runs are dropped) and bit 3 for a
 *   valid pixel with |q| > 2^30 (left out of every table).  P = 0 (table may be null): the check alone.
 * Every accumulation is an integer atomic add, minimum or maximum.  16-byte accesses where labels and values are 16-byte and mask 4-byte
 * aligned; no access outside the H * W elements, no store outside the table.  Bad arguments return -1 before any launch. */
int unet_obj_absmax(const uint8_t* mask, const float* values, int H, int W, const uint32_t* exclude8, int has_nodata, float nodata,
                    long long* absmax, void* stream);
int unet_obj_values(const uint8_t* mask, const int32_t* labels, const float* values, const int32_t* offs, int H, int W, const uint32_t* exclude8,
                    long long P, int has_nodata, float nodata, int shift, long long* table, long long* bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNET_HIP_H */
