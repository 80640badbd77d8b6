/*
 * mi355x_gan.h -- C ABI of libmi355x_gan.so: the MI355X (gfx950) GAN training inner loop.
 *
 * The reference (Cameronr11/GAN-Variant-Research) has no FFI of its own: its operator API is
 * torch.nn -> ATen.  Each entry point below replaces the ATen ops one reference call site dispatches
 * (cited as file:line relative to the reference root).  All pointers are DEVICE pointers unless a
 * parameter says "host"; `stream` is a hipStream_t passed as void* (NULL = default stream).  The library
 * never allocates, frees or synchronises; workspaces are supplied by the caller.  Every function returns
 * 0 on success or a negative error code; gan_last_error() describes the last failure of this thread.
 *
 * Data layout in HBM ("halo-NHWC"): an activation is [B][Hp][Wp][C] with C a multiple of 8 (zero-filled
 * pad channels) and an optional spatial halo already materialised by the producer (reflect or zero), so
 * every convolution is a bounds-check-free "valid" implicit GEMM over 16-byte channel chunks.
 */
#ifndef MI355X_GAN_H
#define MI355X_GAN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* GAN_FP8: OCP e4m3 ("e4m3fn": no infinities, max 448), one byte per element.  Only operand COPIES of the bottleneck convolutions are
 * fp8 (BASELINE.json configs[4]): gan_quantize_fp8 writes activations / output gradients, gan_pack_weight the weights; every result,
 * statistic and master weight stays bf16 / fp32.  An fp8 view has C % 16 == 0.
 * Every producer of e4m3 bytes (gan_quantize_fp8, gan_quantize_fp8_pow2, the y8 copy of gan_in_apply_parts_fp8, gan_pack_weight_batch
 * with dtype GAN_FP8) converts the same way: the value, divided by its scale, is clamped to +-448 (+-inf included), then rounded to
 * nearest, ties to even, the sign of zero kept; a NaN element becomes an e4m3 NaN byte (0x7F / 0xFF), never a finite one, so the operand
 * copy of a poisoned buffer is poisoned too. */
enum { GAN_F32 = 0, GAN_BF16 = 1, GAN_FP8 = 2 };
enum { GAN_ACT_NONE = 0, GAN_ACT_RELU = 1, GAN_ACT_LRELU = 2, GAN_ACT_TANH = 3 };
#define GAN_TAP_PAD (1 << 30)   /* gan_conv_desc.tapoff entry of a padded tap (see there) */
/* GAN_HALO_REPLICATE (nn.ReplicationPad2d, generator_resnet_attn.py:26-27,45-46: an option the shipped configs do not use): accepted by
 * gan_nchw_to_view only; its gradient is gan_pad_fold */
enum { GAN_HALO_NONE = 0, GAN_HALO_ZERO = 1, GAN_HALO_REFLECT = 2, GAN_HALO_REPLICATE = 3 };

/* A halo-NHWC activation: `ptr` addresses element [0][0][0][0] of the allocation; the logical HxW image
 * starts at (y0,x0).  dtype: GAN_F32 or GAN_BF16. */
typedef struct gan_view {
  void* ptr;
  int32_t B, Hp, Wp, C;
  int32_t y0, x0, H, W;
  int32_t dtype;
  int32_t _pad;
} gan_view;

/* Generalised tap convolution (implicit GEMM on MFMA).  Row m=(b,ho,wo) of the GEMM reads, for tap t and
 * channel c, in[((b*in_Hp + ho*in_sy + in_y0)*in_Wp + wo*in_sx + in_x0)*Cin + tapoff[t] + c] and the result
 * for output channel n is act(sum + bias[n]) [* lrelu'(mask)] stored at
 * out[((b*out_Hp + ho*out_sy + out_y0)*out_Wp + wo*out_sx + out_x0)*out_C + n].
 * One descriptor covers nn.Conv2d forward, its input-gradient (flipped taps over a zero-haloed dY), the
 * four sub-pixel phases of nn.ConvTranspose2d and their gradients, and the four phases of a stride-2
 * nn.Conv2d's input gradient (out_sy = out_sx = 2, out_y0 / out_x0 = the phase).  Phase (ry, rx) of an H x W
 * destination has Ho = (H - ry + 1) / 2 and Wo = (W - rx + 1) / 2: on an odd destination the phases differ in
 * extent, and a phase without pixels (the odd ones of a 1-pixel axis) has no launch. */
typedef struct gan_conv_desc {
  int32_t dtype;                 /* operand/out dtype */
  int32_t B, Ho, Wo;             /* GEMM rows */
  int32_t Cin;                   /* padded channels per tap: power of two >= 8 */
  int32_t ntaps;                 /* padded so that ntaps*Cin is a multiple of 128 bytes of operand */
  int32_t Nw;                    /* rows of the packed weight [Nw][ntaps][Cin]; multiple of the N tile */
  int32_t Nst;                   /* channels stored (<= out_C, multiple of 4) */
  const void* in;
  int32_t in_Hp, in_Wp, in_y0, in_x0, in_sy, in_sx;
  const int32_t* tapoff;         /* device [ntaps]: (dy*in_Wp + dx)*Cin; an entry >= GAN_TAP_PAD (2^30: a multiple of every Cin, beyond any
                                    real tap) marks a padded tap: the generic kernel reads zeros for it, never a pixel (0 x Inf must
                                    not enter a sum), so w[n][t][*] MUST be zero for such a t; the host cannot check device entries,
                                    and only the generic kernel (w_layout 0) accepts them */
  const void* w;
  const float* bias;             /* device fp32 [>= Nst] or NULL */
  void* out;
  int32_t out_Hp, out_Wp, out_C, out_y0, out_x0, out_sy, out_sx;
  int32_t act;                   /* GAN_ACT_* applied after bias */
  const void* mask;              /* optional LeakyReLU-derivative mask: result *= (mask>0 ? 1 : 0.2); element
                                    ((b*mask_Hp + ho*out_sy + mask_y0)*mask_Wp + wo*out_sx + mask_x0)*out_C + n */
  int32_t mask_Hp, mask_Wp, mask_y0, mask_x0;
  float* stats;                  /* optional InstanceNorm partials fp32 [B][P][out_C][2], P = gan_conv_stats_parts(desc) > 0: per
                                    (image, pixel tile, channel) sum and sum of squares of the result (bias included, before its
                                    rounding to the output type), written with plain stores (deterministic); act must be none */
  int32_t max_tapoff;            /* largest value in tapoff[] (needed by the range-patch kernel's span check) */
  int32_t w_layout;              /* 0: w is [Nw][ntaps][Cin] (generic kernel); 1: fragment-major [Nw/16][ntaps*Cin/32][64][8]
                                    for the range-patch kernel (the descriptor must satisfy gan_conv_patch_ok); 2: w as for 0, run
                                    by the 7x7 window kernel (the descriptor must satisfy gan_conv_win7_ok) */
  int32_t win_ty0, win_tx0;      /* w_layout 2: tapoff[t] = ((win_ty0 + t/7) * in_Wp + win_tx0 + t%7) * Cin, t = 0..48 */
  int32_t tile_rows;             /* w_layout 1: output pixels per tile (256 or 288), fixed by the planner with gan_conv_patch_tile_rows so
                                    that the launch and the partial count of `stats` (gan_conv_stats_parts) agree; 0: chosen at launch */
  int32_t tile_cols;             /* w_layout 1: output channels per tile (128 or 256), fixed by the planner with gan_conv_patch_tile_cols
                                    AFTER tile_rows is set; 0: chosen at launch */
  /* dtype GAN_FP8 (range-patch kernel only, w_layout 1): `in` and `w` hold e4m3 bytes, `out` / `mask` / `bias` are as for GAN_BF16
   * (the result is bf16).  result = act(acc * w_scale[0] * (in_scale ? in_scale[b] : 1) + bias): the dequantisation scales of the
   * weight copy (gan_weight_scale_batch) and of image b of the input copy (gan_quantize_fp8), both device pointers. */
  const float* w_scale;
  const float* in_scale;
  /* Backward chain of a residual block (range-patch kernel only, w_layout 1, bf16, act none, no bias; generator_resnet_attn.py:56,64):
   * stats_mode 0: `stats` receives (sum t, sum t^2), the forward statistics of the result, and `mask` is the LeakyReLU' mask (as before);
   * stats_mode 1: `stats` receives (sum t [m > 0], sum t m) -- the two sums the InstanceNorm backward behind a ReLU needs of its incoming
   *   gradient t (this launch's result, an input gradient on the reflect-padded domain) -- with m = relu(xhat) = the activation the
   *   forward saved WITH its reflect halo, named by `mask` and the mask_* geometry and read at the output pixel's own position; the mask
   *   is then NOT applied to the result.  Summing on the padded domain equals summing the folded gradient because the halo of m is a copy
   *   of its pre-image.  Same partial layout as mode 0 ([B][P][out_C][2], P = gan_conv_stats_parts); consumer: gan_in_bwd_parts. */
  int32_t stats_mode;
  int32_t _pad2;
} gan_conv_desc;

/* Weight-gradient GEMM: part[s][n][t][c] = sum over the rows m of split s of
 * g[g_off(m) + n] * x[x_off(m) + tapoff[t] + c], with g_off/x_off as in gan_conv_desc.  nsplit slabs.
 * dtype GAN_FP8 (variant 1 only; variants 0 and 2 answer with an error): x and g hold e4m3 bytes -- x with unit scale (an e4m3 copy of
 * the layer input, halo >= 1), g the e4m3 copy of the output gradient with one dequantisation scale per image, g_scale[b] -- and
 *   part[s][n][t][c] = g_scale[b(s)] * sum over the pixels m of split s of g8[m][n] * x8[pix(m) + tapoff[t]][c]
 * in fp32 on v_mfma_scale_f32_16x16x128_f8f6f4; a split never crosses an image, the scale is applied when its sums are stored.  part keeps
 * the slab layout, so gan_wgrad_reduce follows unchanged.  With g_scale_pow2 (every g_scale[b] a power of two: gan_quantize_fp8_pow2) a
 * split may cover k whole images, part[s] = sum over the images b of split s of g_scale[b] * (image b's sum): the scale's exponent byte
 * is the E8M0 block scale of the MFMA's g operand, one 128-pixel k-step never leaves an image.  In fp8 mode it replaces the weight-gradient half of the backward() of the
 * residual blocks' nn.Conv2d(256, 256, 3) under autocast (GAN_Variant1/models/generator_resnet_attn.py:33,48). */
typedef struct gan_wgrad_desc {
  int32_t dtype;
  int32_t B, Ho, Wo;
  int32_t Cx;                    /* channels of x per tap (multiple of 8) */
  int32_t ntaps;                 /* real taps */
  int32_t N;                     /* channels of g used (multiple of 8) */
  int32_t nsplit;
  const void* x;
  int32_t x_Hp, x_Wp, x_y0, x_x0, x_sy, x_sx;
  const int32_t* tapoff;         /* device [ntaps]: (dy*x_Wp + dx)*Cx */
  const void* g;
  int32_t g_Hp, g_Wp, g_C, g_y0, g_x0, g_sy, g_sx;
  float* part;                   /* device fp32 [nsplit][N][ntaps][Cx] */
  int32_t max_tapoff;            /* largest value in tapoff[] (range-patch variant's span check) */
  int32_t variant;               /* 0: generic kernel, any nsplit; 1: range-patch kernel, nsplit = B * gan_wgrad_patch_splits() (or B / -that);
                                    2: 7x7 window kernel, nsplit = gan_wgrad_win7_splits() */
  const float* g_scale;          /* dtype GAN_FP8: device float[B], per-image scale of g (NULL = 1); other dtypes: ignored */
  int32_t g_scale_pow2;          /* dtype GAN_FP8, variant 1: the caller promises that every g_scale[b] is a normal power of two (0: no
                                    promise, one image per split); then nsplit may be B / k as gan_wgrad_patch_splits answers */
  int32_t _pad;
} gan_wgrad_desc;

/* Non-finite data in a gan_conv_igemm launch (tests/conv_cases.py).  A NaN or +-Inf in a real channel of one input pixel reaches the
 * output pixels of ITS image whose taps read it and no other: every other image, and its partials in `stats`, keep the bits of a clean
 * run.  Inside that footprint an element is non-finite wherever the float64 statement is, and a NaN stays a NaN through every
 * activation (ReLU is t < 0 ? 0 : t, as torch.relu: never fmaxf) and through the mask factor; where the statement is finite behind an
 * Inf (relu(-Inf) = 0, tanh(+-Inf) = +-1) so is the result.  Zero weights never widen the footprint, with ONE exception: a paired-phase
 * launch (convplan._PairPack: both x-phases of a phase row as one 128-channel launch, for transposed forwards and strided input
 * gradients with 64 output channels) multiplies the zero weights of one phase by the pixels the other phase reads, so both pixels of a
 * 128-channel super-pixel are poisoned when one is (a 6x10 input of the 128 -> 64 layer: 12 output pixels for the reference's 9); the
 * extra pixels are unspecified.  Pad channels (n >= the real Cout) of a poisoned output pixel are unspecified; elsewhere they are 0.
 * The partial sums of a poisoned (image, channel) are non-finite. */
const char* gan_last_error(void);
int gan_version(void);

/* ---- convolution family: replaces nn.Conv2d / nn.ConvTranspose2d forward+backward
 *      (GAN_Variant1/models/generator_resnet_attn.py:33,48,113,125,146-149,160; discriminator_patchgan.py:27,38,45,51;
 *       Basic_GAN/src/models.py:12,16,29,37,50-51,59,81,88,96,103) */
int gan_conv_igemm(const gan_conv_desc* d, void* stream);
/* 1 if the descriptor qualifies for the range-patch kernel (bf16, Cin % 64 == 0, Nw % 128 == 0, one tile's pixel span fits
 * the LDS slab); pure host-side predicate used by the planner to choose the weight layout */
int gan_conv_patch_ok(const gan_conv_desc* d);
/* pixels per tile the range-patch kernel would choose for this descriptor (256 or 288: the one with the fewest CU-rounds x rows; the
 * tuning variable GAN_PATCH_BM is read HERE, at planning time, never at launch); 0 if the descriptor does not qualify */
int gan_conv_patch_tile_rows(const gan_conv_desc* d);
/* output channels per tile for the descriptor's tile_rows: 256 (the whole Cout of the residual 256 -> 256 layers: one slab staging and
 * one epilogue per pixel tile, 32-36 MFMAs per k-step and wave) when Nst % 256 == 0, the layer has >= 4 taps, its maps are at most 64
 * pixels wide and the 256-wide tiles still fill the chip (>= 192 of them), else 128.  GAN_PATCH_BN = 128 | 256 (read here, at planning
 * time) forces one wherever the layer is eligible; 0 if the descriptor does not qualify for the range-patch kernel */
int gan_conv_patch_tile_cols(const gan_conv_desc* d);
/* the instantiation gan_conv_igemm runs a qualifying descriptor on (0: it does not qualify): tile rows | tile columns << 12 | LDS
 * slices (7 or 9: pixels a tile's taps span, / 64) << 24 | e4m3 operands << 28 | static 3x3 schedule << 29 | other static tap
 * schedules << 30 (1: 4 taps, 2: 2 taps, 3: 16 taps -- the sub-pixel phases and the discriminator's 4x4 windows).  The value uses bit 31:
 * read it as unsigned.  Pure host-side query: tests assert with it that a case really reaches the kernel it is meant to cover. */
int gan_conv_patch_variant(const gan_conv_desc* d);
/* the tiling of the launch gan_conv_igemm makes for the descriptor, by its w_layout: info[0] = pixels per tile, info[1] = output channels
 * per tile, info[2] = tiles (generic kernel: virtual tiles, the M tiles rounded up to a multiple of 8 times the N tiles), info[3] = blocks
 * launched.  A block of the generic kernel (w_layout 0, grid <= 512) and of the range-patch kernel (1, grid <= 256) walks tiles
 * b, b + grid, ...; the 7x7 window kernel (2) launches one block per 16x16 tile.  Returns 0, or non-zero (gan_last_error) if the
 * descriptor does not qualify for its w_layout.  Pure host-side query: the launch reads the same plan. */
int gan_conv_igemm_variant(const gan_conv_desc* d, int32_t* info);
/* 1 if the descriptor qualifies for a 7x7 window kernel (bf16, stride 1, 49 row-major taps located by win_ty0/win_tx0, act none or
 * tanh, no mask / stats): Cin = 64, Nw = 16, Nst = out_C = 8 (the 64 -> 3 channel layers) or Cin = 8, Nw = Nst = out_C = 64 with the
 * tap list padded to >= 52 (the 3 -> 64 channel layers) */
int gan_conv_win7_ok(const gan_conv_desc* d);
/* pixel tiles per image for which the descriptor's launch writes InstanceNorm partials to d->stats; 0: it cannot (then use gan_in_stats) */
int gan_conv_stats_parts(const gan_conv_desc* d);
int gan_conv_wgrad(const gan_wgrad_desc* d, void* stream);
/* splits per image the range-patch weight-gradient kernel wants (0: the descriptor does not qualify: bf16, 9 taps, stride 1,
 * Cx % 64 == 0, N % 128 == 0, one 128-pixel stage's window span fits LDS); pure host-side predicate for the planner.
 * A NEGATIVE value -k means k whole images per split (many small maps, e.g. 16x16 at batch 256): nsplit = B / k.
 * dtype GAN_FP8: the same question for the e4m3 kernel (e4m3 x and g, 9 taps, stride 1, Cx % 64 == 0, N % 128 == 0); without
 * g_scale_pow2 never negative -- where the bf16 answer would be, it is 0 and the planner keeps the bf16 kernel for that launch; with
 * g_scale_pow2 the bf16 query's negative answer for the same geometry. */
int gan_wgrad_patch_splits(const gan_wgrad_desc* d);
/* grad[(a*I2 + b)*KK + khw[t]] (+)= sum_s part[s][n][t][c], (a,b) = swap ? (c,n) : (n,c), for n<N_real, c<C_real, khw[t]>=0 */
/* slabs the 7x7 window weight-gradient kernels write (0: the descriptor does not qualify: bf16, 49 row-major taps, stride 1, and
 * Cx = 64, N = g_C = 8 -- the generator's 64 -> 3 channel output convolution -- or Cx = 8, N = g_C = 64 -- its 3 -> 64 first one) */
int gan_wgrad_win7_splits(const gan_wgrad_desc* d);
/* lanes G (1, 2 ... 32) gan_wgrad_reduce lets share one output quad for these arguments; pure query */
int gan_wgrad_reduce_lanes(int nsplit, int N_real, int ntaps, int Cx);
int gan_wgrad_reduce(const float* part, int nsplit, int N, int ntaps, int Cx, int N_real, int C_real, int swap, int I2,
                     int KK, const int32_t* khw, float* grad, int accumulate, void* stream);
/* dst[n][t][c] = src[(a*I2 + b)*KK + khw[t]] (0 where n>=N_real, c>=C_real or khw[t]<0); dst dtype GAN_*.
 * layout 0: row-major [Nw][ntaps][Cin]; layout 1: fragment-major, element (n, k=t*Cin+c) at
 * (((n/16)*(ntaps*Cin/32) + k/32)*64 + ((k%32)/8)*16 + n%16)*8 + k%8 (one MFMA operand fragment = 1 KB contiguous) */
int gan_pack_weight(const float* src, void* dst, int dtype, int Nw, int ntaps, int Cin, int N_real, int C_real, int swap,
                    int I2, int KK, const int32_t* khw, int layout, void* stream);
/* gan_pack_weight for many operand copies in one launch.  `descs` is a DEVICE array of n descriptors (fields as the arguments
 * of gan_pack_weight); the caller assigns each a contiguous block range: first_block = running sum of nblocks (256 threads per
 * block, any nblocks >= 1), total_blocks = their sum.  Validation of each descriptor is the caller's (same rules). */
typedef struct gan_pack_desc {
  const float* src; void* dst; const int32_t* khw;
  int32_t dtype, Nw, ntaps, Cin, N_real, C_real, swap, I2, KK, layout, first_block, nblocks;
  float* scale;                  /* dtype GAN_FP8: device float, dst = e4m3(src / *scale); written by gan_weight_scale_batch.  GAN_BF16 /
                                    GAN_F32: NULL, or a device float and dst = src / *scale (spectral norm: scale = sigma, so the
                                    copy is W_sn's, packed from weight_orig; discriminator_patchgan.py:21-23) */
} gan_pack_desc;
int gan_pack_weight_batch(const gan_pack_desc* descs, int n, int total_blocks, void* stream);
/* For every descriptor with dtype GAN_FP8: *scale = max|src| / 448 over the whole master weight ((swap ? C_real : N_real) * I2 * KK
 * floats), 1 if the weight is all zero, never below 2^-126 (as gan_quantize_fp8's scales: the reciprocal stays finite) -- the per-tensor
 * dequantisation scale of the e4m3 operand copy.  One launch for the batch
 * (same DEVICE descriptor array as gan_pack_weight_batch, which it precedes). */
int gan_weight_scale_batch(const gan_pack_desc* descs, int n, void* stream);
/* e4m3 operand copy of an activation / gradient buffer: dst (GAN_FP8) has exactly src's (GAN_BF16 / GAN_F32) geometry (B, Hp, Wp, C,
 * halo) and the WHOLE allocation is converted, halo included (the producer already materialised it).  amax == NULL: dst = e4m3(src)
 * (unit scale: InstanceNorm outputs are O(1)).  amax != NULL: device float[B] holding max|src| per image (gan_in_bwd_amax); then
 * scale_out[b] = amax[b] / 448 (1 if zero) and dst = e4m3(src / scale_out[b]).  Values are clamped to +-448 before conversion.
 * The scale is never below 2^-126: for 0 < amax[b] < 448 * 2^-126 the quotient would be subnormal and its reciprocal infinite, so it is
 * clamped to 2^-126 (what gan_quantize_fp8_pow2's exponent clamp gives) and the image's bytes are finite, small ones.  Only amax[0 .. B)
 * and scale_out[0 .. B) are read / written.  A NaN INSIDE amax is outside this contract. */
int gan_quantize_fp8(const gan_view* src, const gan_view* dst, const float* amax, float* scale_out, void* stream);
/* gan_quantize_fp8 with power-of-two scales (amax and scale_out required): scale_out[b] = 2^ceil(log2(amax[b] / 448)), computed on the bit
 * pattern of amax[b] (biased exponent e, mantissa field m: e - 8, plus 1 if m > 0x600000 i.e. 1.m > 1.75; clamped to 1 .. 254 so the
 * scale is a normal float), 1 for amax[b] == 0; dst = e4m3(src / scale_out[b]), clamped to +-448 first.  amax / 448 <= scale < 2 amax / 448:
 * at most one of e4m3's bits of range is given up, and the scale's exponent byte is an E8M0 block scale (gan_wgrad_desc.g_scale_pow2).
 * The e4m3 copies of the residual blocks' output gradients in the fused CycleGAN trainer's fp8 mode: the operand copies that
 * torch.autocast would make for the backward() of Basic_GAN/src/models.py:12,16 (nn.Conv2d(dim, dim, 3) of ResnetBlock), were it e4m3. */
int gan_quantize_fp8_pow2(const gan_view* src, const gan_view* dst, const float* amax, float* scale_out, void* stream);
/* bias gradient: grad[n] (+)= sum over logical pixels of g[...,n], n < N_real (column sums of dY) */
int gan_bias_grad(const gan_view* g, int N_real, float* grad, int accumulate, float* ws, void* stream);

/* ---- InstanceNorm2d (+ReLU/LeakyReLU, + residual add, + halo fill): replaces nn.InstanceNorm2d, nn.ReLU,
 *      nn.ReflectionPad2d and the residual add (generator_resnet_attn.py:25,43,56,64,71,111,114-115,126-127,150-151,158;
 *      Basic_GAN/src/models.py:10-18,30-31,38-39,52-53,91-92,99-100).  stats = fp32 [B][C][2] (mean, rstd).
 *
 * Conditioning of the statistics (every producer: gan_in_stats, gan_in_partial + gan_in_stats_from_parts / gan_in_apply_parts, the
 * convolution epilogue's partials, gan_in_finalize).  The biased variance is evaluated as E[x^2] - mean^2: sum and sum of squares are
 * accumulated in fp32 per lane and chunk, combined in fp64, var is clamped at 0 and rstd = 1 / sqrt(var + eps).  With
 *     dS = 4 sqrt(HW) 2^-24 sum|x|,   dQ = 4 sqrt(HW) 2^-24 sum x^2
 * the results satisfy   |mean - mean_exact| <= dS / HW + 2^-24 |mean|,
 *                       |var - var_exact|   <= tol_var = dQ / HW + 2 |mean| dS / HW + (dS / HW)^2,
 *                       rstd in [ (var_exact + tol_var + eps)^-1/2, (max(var_exact - tol_var, 0) + eps)^-1/2 ] widened by 2^-23 relative,
 * which for tol_var << var + eps is 1/2 rstd^3 tol_var.  The relative error of the variance therefore grows with
 * kappa = (mean^2 + var) / var: about 1e-5 on centred data, 1e-3 at |mean| / sigma = 100, and no digits are left around
 * |mean| / sigma = 1000 (has the measured figures).  torch's float32 instance_norm subtracts the mean before squaring
 * and is better conditioned (1e-7 on all of these); callers whose activations carry a mean far above their spread must centre them first.
 * With H * W = 1, var is the fp32 rounding error of x^2 (0 where x^2 is exact in fp32), mean is x and y is exactly 0 (+ residual).
 *
 * What each entry point writes.  stats: floats [0, B*C*2).  gan_in_stats' ws: floats [0, B*nchunks*C*2), nchunks <= 96.  gan_in_partial:
 * parts [0, B*gan_in_partial_count(x)*C*2).  gan_in_apply / gan_in_apply_parts: the interior of y, and with GAN_HALO_REFLECT also the
 * y0 / x0 halo pixels around it (each a bit copy of the value at its reflect pre-image); every other halo_mode (NONE, ZERO, REPLICATE)
 * leaves the halo as it is -- a zero halo is the caller's, zeroed once at allocation.  gan_in_bwd*, gan_fold_add, gan_pad_fold,
 * gan_act_bwd: the interior of dx / out only.  Bias: bias_grad[0, bias_n), bias_part [0, gan_in_bwd_bias_parts(x)*C) (row 0 of each image
 * holds the closed-form value, the other rows 0), gan_bias_finalize_batch: grad[0, N_real) of each descriptor.
 * Widths: C a multiple of 8 (both dtypes) with C/8 (bf16) or C/4 (fp32) a power of two <= 256; gan_in_apply_parts C <= 1024; the
 * backward entry points C <= 512.  Every entry point is deterministic: a repeated call gives the same bits. */
int gan_in_stats(const gan_view* x, float eps, float* stats, float* ws, void* stream);
/* (mean, rstd) from the per-tile partials a convolution epilogue wrote to gan_conv_desc.stats (parts = [B][nparts][C][2]) */
int gan_in_stats_from_parts(const float* parts, int nparts, int B, int C, int HW, float eps, float* stats, void* stream);
/* turns whole-image sums (sum, sum of squares) into (mean, rstd) in place */
int gan_in_finalize(float* stats, int BC, int HW, float eps, void* stream);
int gan_in_apply(const gan_view* x, const float* stats, int act, const gan_view* residual, const gan_view* y,
                 int halo_mode, void* stream);
/* The same pass with the statistics taken from per-chunk partial sums, parts = fp32 [B][nparts][C][2] (sum, sum of squares),
 * 1 <= nparts <= 16: each block adds the partials of its image up itself (fp64, fixed order), so no separate statistics launch sits
 * between the producing convolution and this pass; (mean, rstd) are also written to `stats` for the backward pass.  The partials come
 * from a convolution epilogue (gan_conv_desc.stats with gan_conv_stats_parts(desc) <= 16) or from gan_in_partial, which writes
 * gan_in_partial_count(x) of them per image. */
int gan_in_partial_count(const gan_view* x);
int gan_in_partial(const gan_view* x, float* parts, void* stream);
int gan_in_apply_parts(const gan_view* x, const float* parts, int nparts, float eps, float* stats, int act, const gan_view* residual,
                       const gan_view* y, int halo_mode, void* stream);
/* gan_in_apply_parts that also writes y8, an e4m3 copy of y (GAN_FP8 view of y's geometry, unit scale, halo included): the operand of the
 * next convolution on the fp8 path without a separate gan_quantize_fp8 pass */
int gan_in_apply_parts_fp8(const gan_view* x, const float* parts, int nparts, float eps, float* stats, int act, const gan_view* residual,
                           const gan_view* y, const gan_view* y8, int halo_mode, void* stream);
/* backward: g = (fold of `gy` over its reflect halo if fold) [+ g2], masked by act'(xhat) (relu / lrelu);
 * dx = rstd*(g - mean(g) - xhat*mean(g*xhat)) written to the interior of `dx` (halo untouched).
 * ws: fp32 >= B*96*C*2 + B*C*2 floats (gan_in_stats: B*96*C*2). */
int gan_in_bwd(const gan_view* x, const float* stats, int act, const gan_view* gy, int fold, const gan_view* g2,
               const gan_view* dx, float* ws, void* stream);
/* gan_in_bwd that also produces the gradient of the convolution bias in front of the norm (column sums of dx) in the same
 * pass: bias_grad[n] (+)= sum_pixels dx[..,n], n < bias_n.  ws: fp32 >= B*96*C*2 + B*C*2 + (B*1024+32)*C floats. */
int gan_in_bwd_bias(const gan_view* x, const float* stats, int act, const gan_view* gy, int fold, const gan_view* g2,
                    const gan_view* dx, float* ws, float* bias_grad, int bias_n, int bias_accumulate, void* stream);
/* out = a + fold(b): gradient of a residual block input (skip path + reflect-padded conv path) */
/* gan_in_bwd_bias with the bias-gradient sum deferred: the per-block column sums go to `bias_part`
 * ([gan_in_bwd_bias_parts(x)][x->C] floats, caller-owned) and gan_bias_finalize_batch adds them up for many layers in one launch
 * (descs on the device; first_block = running sum of ceil(C/32); total_blocks = that sum over all descriptors). */
typedef struct gan_bias_part_desc {
  const float* part; float* grad;
  int32_t nparts, C, N_real, accumulate, first_block, _pad;
} gan_bias_part_desc;
int gan_in_bwd_bias_parts(const gan_view* x);
/* The apply half of gan_in_bwd_bias_deferred alone, for a gradient whose two per-(image, channel) sums were already produced by the launch
 * that wrote it: parts = fp32 [B][nparts][C][2], 1 <= nparts <= 96, summed here in fp64 and in part order.
 * parts_mode 1: (sum g', sum g' xhat), second sum in normalised units (gan_conv_desc.stats_mode 1: m = relu(xhat); act must be relu);
 * parts_mode 2: (sum g', sum g' x) against the raw x (what gan_in_bwd's own first pass computes: for a producer that has x at hand).
 * bias_part may be NULL. */
int gan_in_bwd_parts(const gan_view* x, const float* stats, int act, const gan_view* gy, int fold, const gan_view* dx, const float* parts,
                     int nparts, int parts_mode, float* bias_part, void* stream);
int gan_in_bwd_bias_deferred(const gan_view* x, const float* stats, int act, const gan_view* gy, int fold, const gan_view* g2,
                             const gan_view* dx, float* ws, float* bias_part, void* stream);
int gan_bias_finalize_batch(const gan_bias_part_desc* descs, int n, int total_blocks, void* stream);
/* gan_in_bwd_bias_deferred (bias_part may be NULL: no bias gradient) that also leaves max|dx| per image in amax[B] (device floats,
 * combined with atomic max on the bit patterns -- order-independent, hence deterministic): the scale of dx's e4m3 copy.
 * amax[b] is the maximum over the INTERIOR of image b (the halo of dx is neither written nor read) of the fp32 values BEFORE the store
 * rounds them to dx's dtype: for GAN_F32 it is exactly max|dx[b]|, for GAN_BF16 it may differ from the maximum of the stored dx by one bf16
 * rounding (2^-8 relative).  Every call overwrites amax[0 .. B) (the reset is part of the op); dx and bias_part are bit for bit what
 * gan_in_bwd_bias_deferred / gan_in_bwd write.  What amax holds when dx contains a NaN is not specified. */
int gan_in_bwd_amax(const gan_view* x, const float* stats, int act, const gan_view* gy, int fold, const gan_view* dx, float* ws,
                    float* bias_part, float* amax, void* stream);
int gan_fold_add(const gan_view* a, const gan_view* b, int fold, const gan_view* out, void* stream);
/* gradient of a padding layer: out[b][y][x] = sum of g over the padded positions (g carries a halo of y0/x0 pixels) that the padding
 * copies from (y,x); mode GAN_HALO_REPLICATE (nn.ReplicationPad2d: an edge pixel collects its whole halo run) or GAN_HALO_REFLECT */
int gan_pad_fold(const gan_view* g, int mode, const gan_view* out, void* stream);
/* dx = g * act'(y) (tanh: 1-y^2, lrelu: y>0?1:0.2), g optionally folded; written to the interior of dx */
int gan_act_bwd(const gan_view* y, int act, const gan_view* g, int fold, const gan_view* g2, const gan_view* dx, void* stream);

/* ---- layout boundary: NCHW fp32 (the reference's tensors) <-> halo-NHWC */
int gan_nchw_to_view(const float* src, int C, const gan_view* dst, int halo_mode, void* stream);
int gan_view_to_nchw(const gan_view* src, int C, float* dst, void* stream);
int gan_view_copy(const gan_view* src, const gan_view* dst, int halo_mode, void* stream);   /* interior copy + halo fill */
/* The three are exact: every value is rounded once to the destination type (a NaN stays a NaN in exactly the copies that read it).
 * gan_nchw_to_view writes 0 to channels C .. dst->C of every pixel it writes; GAN_HALO_NONE writes the interior only, GAN_HALO_REFLECT
 * (both calls; needs y0 < H and x0 < W) and GAN_HALO_REPLICATE (gan_nchw_to_view) the padded extent of y0 / x0 pixels as well. */
/* Output epilogue of inference (GAN_Variant1/generate_folder.py:183-185 fused with the NCHW -> HWC turn): dst is packed [B][H][W][C]
 * uint8, 1 <= C <= 4, C <= src->C, src fp32 or bf16;  dst[b][y][x][c] = (uint8) rint(((clamp(v, -1, 1) * 0.5f) + 0.5f) * 255.f) with v
 * the interior value as fp32, every operation rounded to fp32 on its own, rint half to even: bit-identical to
 * y.clamp(-1, 1).mul(0.5).add(0.5).mul(255).round().byte() of what the fp32 NCHW conversion above writes, permuted to HWC.
 * A NaN gives 0 (torch leaves that conversion undefined); +-inf clamp like any other value.  Halo pixels are never read and the
 * values of the pad channels C .. src->C never reach dst.  C == 3 with W % 4 == 0 and a four-byte aligned dst (the generator's case)
 * is written as dwords, anything else as bytes. */
int gan_view_to_u8_hwc(const gan_view* src, int C, uint8_t* dst, void* stream);

/* ---- AvgPool2d(kernel 3, stride 2, padding 1, count_include_pad=False): the downsampling between the scales of
 *      MultiscaleDiscriminator (GAN_Variant1/models/discriminator_patchgan.py:100, 110-112; get_intermediate_features :125-127).
 *      y is ((H-1)/2+1) x ((W-1)/2+1); only interiors are written (zero halos stay zero).  bwd: gx (+)= pool^T gy.
 *      A NaN reaches exactly the outputs whose window reads it; the halo of x is never read. */
int gan_avgpool_fwd(const gan_view* x, const gan_view* y, void* stream);
int gan_avgpool_bwd(const gan_view* gy, const gan_view* gx, int accumulate, void* stream);

/* ---- Spectral normalisation of a convolution weight: torch.nn.utils.spectral_norm as applied by
 *      GAN_Variant1/models/discriminator_patchgan.py:21-23 and Basic_GAN/src/models.py:68-69 (n_power_iterations 1, eps 1e-12).
 *      W = weight_orig as an h x w row-major matrix (h = Cout, w = Cin*kh*kw: the OIHW tensor itself); u [h], v [w] are the
 *      module's weight_u / weight_v buffers.  fwd: if power_iter, v <- normalize(W^T u), u <- normalize(W v) in place; then
 *      *sigma = u . (W v) and Wsn = W / sigma.  bwd: dW = (G - <G, Wsn> u v^T) / sigma with G = dL/dWsn (u, v, sigma: the values
 *      the forward left).  ws: fp32, >= gan_spectral_norm_ws_floats(h, w) = h + w + 272 floats; nothing past it is written.
 *      Range: the squares of t = W^T u and s = W v stay normal and their sums finite for 2^-63 <= |t_j|, ||t|| < 2^64 (the same for s);
 *      smaller elements add at most 2^-126 each.  Below ||t|| < eps the divisor is eps (v = t / eps, not a unit vector): with the
 *      reference's eps = 1e-12 a W scaled by 1e-15 is there, and an all-zero W gives u = v = 0, sigma = 0 and W_sn = 0 / 0 = NaN.
 *      Non-finite, power_iter = 1: a NaN in W or u makes every element of u, v, sigma and W_sn NaN (the max with eps keeps a NaN
 *      norm, as F.normalize's clamp_min does); v is overwritten without being read.  power_iter = 0: u and v are not written, and a
 *      NaN in W, u or v makes sigma and every element of W_sn NaN.  bwd: a NaN in G makes every element of dW NaN (it enters
 *      <G, W_sn>), and so does the NaN sigma and W_sn that such a forward leaves.  Refused: a NULL pointer, h <= 0 or w <= 0. */
int64_t gan_spectral_norm_ws_floats(int h, int w);
int gan_spectral_norm_fwd(const float* W, int h, int w, float* u, float* v, int power_iter, float eps, float* sigma, float* Wsn,
                          float* ws, void* stream);
int gan_spectral_norm_bwd(const float* G, const float* Wsn, const float* u, const float* v, const float* sigma, int h, int w,
                          float* dW, float* ws, void* stream);
/* Batched spectral norm: every spectral-norm convolution of a discriminator (all scales) in a fixed number of launches, for the
 * fused trainer.  `descs` is a DEVICE array of n descriptors; each covers gan_spectral_norm_batch_blocks(h, w) blocks, first_block =
 * running sum of nblocks, total_blocks = their sum.
 *   fwd (3 launches; 2 without power_iter): if power_iter, v <- normalize(W^T u), u <- normalize(W v) in place (normalize(x) =
 *        x / max(||x||, eps)); then *sigma = u . (W v) and u_snap, v_snap <- (u, v).  W_sn is not written: the operand copies are
 *        packed from W with gan_pack_desc.scale = sigma.  Semantics of gan_spectral_norm_fwd.
 *   bwd (2 launches): dW (+)= (G - (<G, W> / sigma) u_snap v_snap^T) / sigma, G = dL/dW_sn as the weight-gradient kernels leave it;
 *        accumulate lets the real and fake halves of a D-step add into one weight_orig gradient.
 * Reductions run in a fixed order without atomics: repeated calls are bit-identical.
 * Extents: h <= 512 x w <= 8192 is what the trainers use; h and w are otherwise only limited by int32 tile counts.  Per descriptor
 *   ws >= gan_spectral_norm_batch_ws_floats(h, w) = R w + w + Cb + Cb h + R Cb floats (R = ceil(h / 32) row tiles, Cb = ceil(w / 256)
 *   column tiles); nothing past it is written, and nothing past u[h), v[w), the snapshots, sigma[1) and dW[h w).
 * Range and eps branch: as gan_spectral_norm_fwd.  Non-finite: a NaN in W, u or G of one descriptor reaches only that descriptor's
 *   outputs (with power_iter = 1, W or u: u, v, sigma, the snapshots and dW all NaN; G: dW all NaN); every other descriptor keeps
 *   its bits.
 * Refused: descs NULL, n <= 0, total_blocks <= 0 (the descriptors themselves live on the device and are not validated). */
typedef struct gan_sn_desc {
  const float* W;                /* weight_orig as an h x w row-major matrix */
  float* u; float* v;            /* the module's weight_u [h], weight_v [w] */
  float* sigma;                  /* [1] */
  float* u_snap; float* v_snap;  /* [h], [w]: the (u, v) of the last forward, read by the backward */
  const float* G;                /* bwd: dL/dW_sn [h x w] */
  float* dW;                     /* bwd: dL/dweight_orig [h x w] */
  float* ws;                     /* fp32 >= gan_spectral_norm_batch_ws_floats(h, w), private to the descriptor */
  int32_t h, w, first_block, nblocks;
} gan_sn_desc;
int64_t gan_spectral_norm_batch_ws_floats(int h, int w);
int gan_spectral_norm_batch_blocks(int h, int w);
int gan_spectral_norm_batch_fwd(const gan_sn_desc* descs, int n, int total_blocks, int power_iter, float eps, void* stream);
int gan_spectral_norm_batch_bwd(const gan_sn_desc* descs, int n, int total_blocks, int accumulate, void* stream);

/* ---- DiffAugment (GAN_Variant1/training/diffaugment.py:6-60,94-106), per-sample parameters injected.
 *      prm = device fp32 [B][12]: brightness add, saturation factor, contrast factor, tx, ty,
 *      cut_lo_h, cut_hi_h, cut_lo_w, cut_hi_w (inclusive; lo>hi = no cutout), 3 spare.  C = real channels (1..4; the views have C = 8).
 *      y[b][h][w] = 0 where (h, w) is cut or (h + tx, w + ty) lies outside the image, else the value of x[b][h + tx][w + ty] after
 *      brightness, saturation about the pixel's channel mean and contrast about the image's mean over (c, h, w); channels C..7 of
 *      every interior pixel of the output are written as 0, halos are not written.  ws: fp32, [0 .. B) is written (fwd: the images'
 *      sums over the real channels; bwd: the sums of gy over the pixels that took a value), nothing past it.
 *      Accuracy: the contrast line (s - mu) * con + mu carries the fp32 image mean: its error is about 4 sqrt(C H W) 2^-24 |mean|
 *      whatever the spread of the image, so relative to the spread it grows with |mean| / spread.
 *      Non-finite data: a NaN in a real channel of a pixel reaches, through the image mean, every output pixel of that image that
 *      takes a value (bwd: a NaN in a gy pixel that took a value reaches all of gx of that image); pixels that take no value stay
 *      exactly 0, other images are unaffected, and pad channels, halos and (bwd) cut or shifted-out pixels of gy are never read. */
int gan_diffaug_fwd(const gan_view* x, int C, const float* prm, const gan_view* y, float* ws, void* stream);
int gan_diffaug_bwd(const gan_view* gy, int C, const float* prm, const gan_view* gx, float* ws, void* stream);

/* ---- Device-side input pipeline: what the reference's dataset workers do per image with PIL, bit for bit --
 *      GAN_Variant1/dataio/transforms.py:10-49 (RandomCropResize = crop + BICUBIC resize, RandomHorizontalFlip,
 *      ColorJitter(0.05,0.05,0.05,0.02), ToTensor, Normalize(0.5,0.5); eval: Resize) and Basic_GAN/src/data.py:8-26
 *      (Resize(load_size, BICUBIC), RandomCrop/CenterCrop, flip, ToTensor, Normalize).  One job per image; the random draws are
 *      made by the caller (dataio.py reproduces the reference's draw order) so the kernels are deterministic. */
typedef struct gan_input_job {
  const uint8_t* src;            /* device: decoded RGB, HWC, 3 bytes per pixel */
  int32_t src_stride;            /* bytes per source row */
  int32_t crop_y, crop_x, crop_h, crop_w;   /* TF.crop box in the source (whole image: 0,0,H,W) */
  int32_t res_h, res_w;          /* size the box is resized to (Image.resize, BICUBIC) */
  int32_t win_y, win_x;          /* S x S window taken from the resized image (RandomCrop / CenterCrop; 0,0 when res == S) */
  int32_t flip;                  /* RandomHorizontalFlip */
  int32_t order[4];              /* ColorJitter: op applied in slot 0..3 (0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none) */
  float factor[4];               /* brightness, contrast, saturation factors (indexed by op); [3] unused */
  int32_t hue_shift;             /* uint8(hue_factor * 255): added to the H channel with wrap-around */
  int32_t hb_off, hk_off, hksize;  /* horizontal taps in the tables block (int32 units): bounds [res_w][2], taps [res_w][hksize] */
  int32_t vb_off, vk_off, vksize;  /* vertical taps: bounds [res_h][2], taps [res_h][vksize] */
} gan_input_job;
/* Pillow's taps for resizing in_size -> out_size (Resample.c precompute_coeffs + normalize_coeffs_8bpc, 22-bit fixed point).  Host-only,
 * no GPU.  The filter ids are Pillow's: BILINEAR is Resample.c bilinear_filter (1 - |x| for |x| < 1, support 1), BICUBIC its
 * bicubic_filter (Keys, a = -0.5, support 2); ksize = ceil(support * max(in / out, 1)) * 2 + 1.  Any other id is an error.  The two
 * entries without a filter argument are the BICUBIC case. */
enum { GAN_RESIZE_BILINEAR = 2, GAN_RESIZE_BICUBIC = 3 };
int gan_resize_ksize_filter(int in_size, int out_size, int filter);
int gan_resize_coeffs_filter(int in_size, int out_size, int filter, int32_t* bounds /* [out][2]: first index, count */,
                             int32_t* kk /* [out][ksize] */, int ksize);
int gan_resize_ksize(int in_size, int out_size);
int gan_resize_coeffs(int in_size, int out_size, int32_t* bounds /* [out][2]: first index, count */, int32_t* kk /* [out][ksize] */, int ksize);
/* jobs_dev/tables_dev: device copies; jobs_host: the same jobs readable by the host (validation, launch shapes).
 * tmp: >= B*tmp_rows*S*4 bytes (tmp_rows >= max crop_h); img: B*S*S*4 bytes; mean_ws: B int32; out: fp32 [B][3][S][S] in [-1,1]. */
int gan_input_pipeline(const gan_input_job* jobs_dev, const gan_input_job* jobs_host, int B, const int32_t* tables_dev, int S,
                       uint8_t* tmp, int tmp_rows, uint8_t* img, int32_t* mean_ws, float* out, void* stream);
/* The same with the jobs' tap counts validated against `filter` (one filter per call; the tables in the block are that filter's).
 * The resize kernels read tables, so nothing else differs; the entry above is the BICUBIC case. */
int gan_input_pipeline_filter(const gan_input_job* jobs_dev, const gan_input_job* jobs_host, int B, const int32_t* tables_dev, int S,
                              int filter, uint8_t* tmp, int tmp_rows, uint8_t* img, int32_t* mean_ws, float* out, void* stream);
/* The same launches with another finish: out is uint8 [B][3][S][S], the bytes of the transformed image (what the reference's evaluation
 * loader, EVAL/eval/datasets.py:52-66, hands the feature extractor after Image.resize and ToTensor * 255). */
int gan_input_pipeline_u8(const gan_input_job* jobs_dev, const gan_input_job* jobs_host, int B, const int32_t* tables_dev, int S,
                          int filter, uint8_t* tmp, int tmp_rows, uint8_t* img, int32_t* mean_ws, uint8_t* out, void* stream);

/* ---- Baseline JPEG encoder on the device: the file the reference writes with pil.save(..., format="JPEG", quality=95, subsampling=0,
 *      optimize=True) (GAN_Variant1/generate_folder.py:252), byte for byte -- libjpeg's 8-bit JDCT_ISLOW path, 4:4:4, one interleaved
 *      scan, optimal Huffman tables, no restart markers.  Integer arithmetic only; histogram adds and the ORs that pack the stream are
 *      integer atomics, so repeated calls give identical bytes.  The caller writes the header (SOI, JFIF APP0, two DQT, SOF0 with the
 *      true H and W, four DHT in the order DC0 AC0 DC1 AC1, SOS) from the tables these entries return, then the scan bytes, then EOI.
 *      Blocks are in scan order: MCU-major (row-major 8x8 tiles), Y then Cb then Cr; nblk = 3 ceil(H/8) ceil(W/8).
 *      Refused with a message, before any launch: a NULL pointer, B, H or W outside 1 .. 65535, quality outside 1 .. 100, an image of
 *      more than 2^32 / 1728 blocks (bit offsets inside one image are 32-bit; 4096 x 4096 passes), B nblk >= 2^28, a workspace or an
 *      output buffer smaller than gan_jpeg_bounds asks, a workspace that is not 16-byte aligned. */
/* Host only: bytes of workspace and of scan output that (B, H, W) needs.  out_bytes = 2 B nblk 216: a block codes to at most
 * 16 + 11 + 63 (16 + 10) = 1665 <= 1728 bits, and stuffing can at most double a stream. */
int gan_jpeg_bounds(int B, int H, int W, int64_t* ws_bytes, int64_t* out_bytes);
/* rgb: packed uint8 [B][H][W][3] (what gan_view_to_u8_hwc leaves).  Two launches.
 *   colour (jccolor.c):  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,  Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
 *     Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16, each minus 128; the last column / row is replicated to a multiple of 8.
 *   DCT (jfdctint.c, CONST_BITS 13, PASS1_BITS 2): rows, outputs 0/4 << 2, the others DESCALE(., 11); columns, outputs 0/4 DESCALE(., 2),
 *     the others DESCALE(., 15); DESCALE(x, n) = (x + (1 << (n - 1))) >> n, arithmetic shift.
 *   quantisation: q[k] = clamp((base[k] s + 50) / 100, 1, 255), s = quality < 50 ? 5000 / quality : 200 - 2 quality, base = the standard
 *     luminance (Y) / chrominance (Cb, Cr) table; coefficient = sign(c) ((|c| + 4 q) / (8 q)); stored in zig-zag order in the workspace.
 *   symbols (jchuff.c): DC = bit length of the difference to the same component's block of the previous MCU (0 at the start); AC =
 *     run << 4 | bit length, 0xF0 per 16 zeros, 0x00 when the block ends in zeros.
 * hist: uint32 [B][4][256], overwritten: symbol counts of the tables DC-Y, AC-Y, DC-C, AC-C of every image. */
int gan_jpeg_blocks(const uint8_t* rgb, int B, int H, int W, int quality, void* ws, int64_t ws_bytes, uint32_t* hist, void* stream);
/* jpeg_gen_optimal_table for n histograms (uint32 [n][256], each below 10^9 in sum), one wave each: a 257th pseudo-symbol of frequency 1;
 * merge the two least frequent non-zero entries until one is left, the larger index first on ties; lengths above 16 folded down with
 * libjpeg's bits[i] -= 2, bits[i-1]++, bits[j+1] += 2, bits[j]-- loop (lengths above 32, which libjpeg refuses, are counted as 32); the
 * pseudo-symbol leaves the longest length; symbols ordered by (length before folding, value); canonical codes.
 * dht: uint8 [n][272] = the DHT segment's 16 counts, then its symbols (zero past the last); codes: uint32 [n][256] = length << 16 | code,
 * 0 for a symbol without a code. */
int gan_jpeg_tables(const uint32_t* hist, int n, uint8_t* dht, uint32_t* codes, void* stream);
/* The entropy-coded scan of the coefficients gan_jpeg_blocks left in ws, with codes uint32 [B][4][256] from gan_jpeg_tables.  Six
 * launches: bits per block; exclusive scan per image; every block ORs its bits into the zeroed stream at its offset (most significant
 * bit first), the last byte padded with 1-bits; 0xFF bytes counted, scanned and scattered with a 0x00 after each (the padded last
 * byte included).  out: the streams of images 0 .. B-1 back to back; offsets: int64 [B + 1] on the device, image b is
 * out[offsets[b] .. offsets[b + 1]).  Nothing past out[out_bytes) is written. */
int gan_jpeg_scan(void* ws, int64_t ws_bytes, int B, int H, int W, const uint32_t* codes, uint8_t* out, int64_t out_bytes, int64_t* offsets,
                  void* stream);

/* ---- What a stored ZIP entry needs beside its name, made on the device: the bytes of the file and their CRC-32 (csrc/zip.hip).
 *      The CRC-32 is zlib's: reflected polynomial 0xEDB88320, register all ones at the start, complemented at the end; an empty range
 *      gives 0.  Integer arithmetic only and no atomic whose order matters (the only one ORs a constant into `flag`), so repeated
 *      calls give identical words.  Refused with a message, before any launch: a NULL pointer, a negative count or byte size, B outside
 *      1 .. 65535, a head outside 2 .. 65535 or an SOS outside 4 .. 65535 bytes, an image size gan_jpeg_bounds refuses. */
/* CRC-32 of n byte ranges of one device buffer; range i is buf[offsets[i] .. offsets[i + 1]).  offsets: int64 [n + 1] on the device (what
 * gan_jpeg_scan and gan_jpeg_files leave there); crc: uint32 [n] on the device; flag: one uint32 on the device, zeroed by the caller.
 * One launch, one workgroup of 256 lanes per range: the range is cut into 256 pieces at addresses that are multiples of 16, a lane
 * runs its piece through four slice tables in LDS (16-byte loads), multiplies its register by x^(8 bytes after its piece) modulo the
 * polynomial (32-step carry-less multiply, x^(2^k) from a table) and the workgroup XORs the products.  Every load is clamped to
 * [0, buf_bytes).  An inconsistent pair (negative, decreasing, or past buf_bytes) reads nothing, writes 0 for that range and ORs 1 into
 * *flag; the other ranges are not affected.  n == 0 succeeds and launches nothing. */
int gan_crc32_ranges(const uint8_t* buf, int64_t buf_bytes, const int64_t* offsets, int n, uint32_t* crc, uint32_t* flag, void* stream);
/* Host only: bytes of `files` that B images of H x W can need: out_bytes of gan_jpeg_bounds + B (head_bytes + 4 (5 + 16 + 256) +
 * sos_bytes + 2). */
int gan_jpeg_files_bounds(int B, int H, int W, int head_bytes, int sos_bytes, int64_t* files_bytes);
/* Complete JPEG files back to back on the device.  head: the constant bytes SOI .. SOF0; sos: the constant SOS segment; dht: uint8
 * [B][4][272] from gan_jpeg_tables (tables DC-Y, AC-Y, DC-C, AC-C); scan / scan_offsets (int64 [B + 1]): what gan_jpeg_scan left.
 * File b = head | four DHT segments in the order DC0 AC0 DC1 AC1 (class / id bytes 0x00 0x10 0x01 0x11), each FF C4, the big-endian
 * length 2 + 1 + 16 + n_t, the class byte, the 16 counts and n_t = min(sum of the counts, 256) symbols | sos | scan bytes of image b |
 * FF D9.  Three launches with no host round trip between them: sizes and their exclusive scan (one workgroup), the copy (one workgroup
 * per file; correct for every byte alignment of source and destination), the CRC-32 of every file (the kernel of gan_crc32_ranges).
 * files: file b is files[file_offsets[b] .. file_offsets[b + 1]); file_offsets: int64 [B + 1] on the device; crc: uint32 [B]; flag: one
 * uint32, overwritten: bit 0 = a pair of scan_offsets is inconsistent (negative, decreasing or past scan_bytes; that file gets an empty
 * scan), bit 1 = files_bytes is too small (the offsets are clamped to it and the files that do not fit are cut short).  Nothing past
 * files[files_bytes) is written. */
int gan_jpeg_files(const uint8_t* head, int head_bytes, const uint8_t* sos, int sos_bytes, const uint8_t* dht, const uint8_t* scan,
                   int64_t scan_bytes, const int64_t* scan_offsets, int B, uint8_t* files, int64_t files_bytes, int64_t* file_offsets,
                   uint32_t* crc, uint32_t* flag, void* stream);

/* ---- Baseline JPEG decoder on the device: the pixels Image.open(p).convert("RGB") gives (libjpeg-turbo's 8-bit path: Huffman decode,
 *      jidctint.c's jpeg_idct_islow, jdsample.c's fancy h2v1 / h2v2 upsampling, jdcolor.c's YCbCr -> RGB), for the files a host parser
 *      accepted: SOF0, 8 bit, one interleaved scan, 1 component (1x1) or 3 components with chroma 1x1 and luma 1x1 / 2x1 / 2x2, no Adobe
 *      marker; restart markers are supported.  Integer arithmetic only.  The scan is untrusted: every loop of the kernels is bounded by
 *      a count from the descriptors, every load is clamped to its segment, every store goes to an address computed from counters, and
 *      an irregularity sets bits of the image's error word (GAN_JPEGDEC_ERR_*) and ends that lane's work; the caller sends such a file
 *      to the host decoder.
 *
 *      One upload block carries everything (all offsets from its start, n images, nseg segments):
 *        gan_jpegdec_image [n] | gan_jpegdec_segment [nseg] | uint8 dht [n][4][272] | uint16 qt [n][4][64] | scan bytes
 *      dht[i][t]: 16 counts then the symbols of table t = DC0, DC1, AC0, AC1 (zeros when absent); qt[i][s]: quantisation table s in
 *      natural (row-major) order.  gan_jpegdec_block_offsets gives the byte offsets; qt and the scan bytes start at multiples of 16.
 *      Workspace (16-byte aligned, gan_jpegdec_bounds bytes): decode tables [n][4] | error words int32 [n] | int16 coefficients in
 *      natural order, component after component, blocks row-major over the MCU-padded component | uint8 component planes, padded alike.
 *      Refused with a message, before any launch: a NULL pointer, n or nseg below 1, n above 65535, H or W outside 1 .. 65535, a
 *      component layout outside the class above, MCU counts that do not belong to H and W, table slots outside 0 .. 3, a workspace that
 *      is too small or not 16-byte aligned, coefficient / plane / output offsets that leave their buffers, a segment that names no image,
 *      MCUs beyond its image or bytes outside the block's scan area. */
typedef struct gan_jpegdec_image {
  int32_t ncomp, H, W, hmax, vmax;   /* components 1 | 3; luma sampling factors 1x1, 2x1 or 2x2 (chroma is 1x1) */
  int32_t mcux, mcuy;                /* MCUs across and down: ceil(W / (8 hmax)), ceil(H / (8 vmax)) */
  int32_t seg_first, seg_count;      /* its restart segments in the segment table */
  int32_t dc_tab[3], ac_tab[3];      /* per component: index into dht[i] (DC: 0 | 1, AC: 2 | 3) */
  int32_t q_tab[3];                  /* per component: index into qt[i] */
  int32_t reserved[2];
  int64_t coef_off, plane_off;      /* bytes into the workspace (filled by gan_jpegdec_bounds) */
  int64_t out_off;                   /* bytes into `out` of gan_jpegdec_pixels: where the packed (H, W, 3) image goes */
} gan_jpegdec_image;
typedef struct gan_jpegdec_segment {
  int32_t image, mcu_first, mcu_count;   /* MCUs mcu_first .. mcu_first + mcu_count - 1 of the image, raster order */
  int32_t byte_begin, byte_end;          /* its entropy-coded bytes in the block, the RSTn / EOI marker after them excluded */
} gan_jpegdec_segment;
#define GAN_JPEGDEC_ERR_CODE 1       /* no Huffman code within 16 bits, or a DC category above 15 */
#define GAN_JPEGDEC_ERR_RUN 2        /* a run past coefficient 63 */
#define GAN_JPEGDEC_ERR_END 4        /* bits needed beyond the segment's end */
#define GAN_JPEGDEC_ERR_DC 8         /* a DC value outside int16 */
#define GAN_JPEGDEC_ERR_LEFT 16      /* whole bytes left over at the end of a segment */
#define GAN_JPEGDEC_ERR_RST 32       /* the marker in front of a segment is not the RSTn its number asks */
#define GAN_JPEGDEC_ERR_MARKER 64    /* a 0xFF inside a segment that no 0x00 follows */
#define GAN_JPEGDEC_ERR_RANGE 128    /* IDCT intermediates beyond what libjpeg's C and SIMD code agree on (see gan_jpegdec_idct) */
/* Host only.  Byte offsets of the block's parts for n images and nseg segments: off[0] segments, off[1] dht, off[2] qt, off[3] scan. */
int gan_jpegdec_block_offsets(int n, int nseg, int64_t* off);
/* Host only.  Fills coef_off and plane_off of imgs[0 .. n-1] (host memory) and gives the workspace size. */
int gan_jpegdec_bounds(gan_jpegdec_image* imgs, int n, int64_t* ws_bytes);
/* One wave per DHT table: the 9-bit lookahead table (next 9 bits -> length << 8 | symbol, 0 when the code is longer) and the canonical
 * maxcode / value-offset arrays for the longer codes.  Also zeroes the error words and the coefficient area.  blk_host: the host copy
 * of the block's descriptors (images and segments), which every entry validates. */
int gan_jpegdec_tables(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nseg, void* ws, int64_t ws_bytes, void* stream);
/* One 64-lane workgroup per image with the image's four tables in LDS; lane s decodes restart segments s, s + 64, ..: DC prediction
 * per component from 0, the block index from the MCU counter, 0xFF 0x00 read as 0xFF. */
int gan_jpegdec_entropy(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nseg, void* ws, int64_t ws_bytes, void* stream);
/* One thread per 8x8 block: dequantise in int32, jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2: columns DESCALE(., 11), rows
 * DESCALE(., 18)), + 128, clamp to 0 .. 255.  Sets GAN_JPEGDEC_ERR_RANGE when a dequantised product or a pass-1 value leaves int16
 * or a descaled row value leaves -512 .. 511. */
int gan_jpegdec_idct(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nseg, void* ws, int64_t ws_bytes, void* stream);
/* One thread per pixel: fancy upsampling of the chroma planes (h2v1: (3 cur + prev + 1) >> 2, (3 cur + next + 2) >> 2; h2v2: 3 cur +
 * above / below, then (3 cur + prev + 8) >> 4, (3 cur + next + 7) >> 4; the edges repeat the sample; plain replication when the
 * downsampled width is at most 2, as libjpeg chooses), then R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
 * G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), clamped; R = G = B = Y for one component.  Image i goes to out + out_off, packed
 * (H, W, 3).  err (may be NULL): int32 [n] on the device, receives a copy of the error words. */
int gan_jpegdec_pixels(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nseg, void* ws, int64_t ws_bytes, uint8_t* out,
                       int64_t out_bytes, int32_t* err, void* stream);

/* ---- Progressive JPEG decoder on the device (SOF2, Huffman): the same pixels, for the files a host parser accepted: the component
 *      classes of the baseline decoder, and a scan script that libjpeg decodes without a warning and that brings every coefficient of
 *      every component to its last bit (nothing is left to libjpeg's block smoothing).  A DC scan (Ss = Se = 0) holds all components
 *      interleaved or one component; an AC scan (1 <= Ss <= Se <= 63) holds one component; Al <= 13.  The scans are untrusted in the
 *      same way as the baseline decoder's, and an irregularity sets bits of the image's error word.
 *
 *      One upload block (all offsets from its start; n images, nscan scans, nseg restart segments, nver Huffman table versions):
 *        gan_jpegdec_image [n] | gan_jpegprog_image [n] | gan_jpegprog_scan [nscan] | gan_jpegprog_segment [nseg] | uint8 dht [nver][272]
 *        | uint16 qt [n][4][64] | scan bytes
 *      The gan_jpegdec_image of a file carries its geometry, q_tab, coef_off / plane_off / out_off exactly as for the baseline decoder
 *      (seg_first, seg_count, dc_tab and ac_tab are not read), so the stages behind the coefficients are the baseline decoder's own code
 *      over the same workspace layout.  A DHT that a file redefines is a new version: scans name versions (counted inside their file),
 *      not slots.  gan_jpegprog_block_offsets gives the byte offsets; every part starts at a multiple of 16.
 *      Workspace (16-byte aligned, gan_jpegprog_bounds bytes): decode tables [nver] | error words int32 [n] | int16 coefficients |
 *      uint8 component planes, the last two as in the baseline decoder.
 *      A single-component scan walks the component's real blocks in raster order, ceil(cw / 8) x ceil(ch / 8) with
 *      cw = ceil(W h_c / hmax), ch = ceil(H v_c / vmax), and its restart interval counts those blocks; an interleaved DC scan walks
 *      the MCUs.  Both store into the MCU-padded grid.
 *      Refused with a message, before any launch: everything the baseline entries refuse; counts below 1; more than
 *      GAN_JPEGPROG_MAX_SCANS scans or GAN_JPEGPROG_MAX_TABLES table versions in one file; scan, segment or version ranges outside
 *      their tables; a scan whose component, band, Ah / Al, table versions, dependency index or level is out of range; an earlier scan
 *      of the same file that touches one of its coefficients on the same or a later level; a segment that names no scan of its
 *      image, units beyond its scan or bytes outside the block's scan area; segments of a scan that are out of order, overlap or do
 *      not cover all of its units. */
#define GAN_JPEGPROG_MAX_SCANS 64
#define GAN_JPEGPROG_MAX_TABLES 64
typedef struct gan_jpegprog_image {
  int32_t scan_first, scan_count;    /* its scans in the scan table, file order */
  int32_t seg_first, seg_count;      /* its restart segments in the segment table, ordered by the level of their scan */
  int32_t ver_first, ver_count;      /* its Huffman table versions in dht */
  int32_t nlevel;                    /* 1 + the largest level of its scans */
  int32_t reserved;
} gan_jpegprog_image;
typedef struct gan_jpegprog_scan {
  int32_t image;
  int32_t comp;                      /* 0 .. ncomp - 1: that component alone; -1: all components interleaved (DC scans only) */
  int32_t Ss, Se, Ah, Al;
  int32_t tab[3];                    /* per component: the table version its symbols are coded with, counted inside the file; -1: none
                                        (components outside the scan; DC refinement reads raw bits) */
  int32_t dep;                       /* the latest earlier scan of the file (counted inside the file) that touches one of this scan's
                                        (component, coefficient) pairs, -1: none */
  int32_t level;                     /* scans of one level run side by side: larger than the level of every earlier scan that touches
                                        one of this scan's pairs */
  int32_t reserved[5];
} gan_jpegprog_scan;
typedef struct gan_jpegprog_segment {
  int32_t image, scan;               /* scan: index into the block's scan table */
  int32_t index;                     /* its number inside the scan: RST((index - 1) & 7) stands in front of it when index > 0 */
  int32_t unit_first, unit_count;    /* MCUs (interleaved scan) or real blocks of the component, raster order */
  int32_t byte_begin, byte_end;      /* its entropy-coded bytes in the block, the marker after them excluded */
  int32_t reserved;
} gan_jpegprog_segment;
#define GAN_JPEGPROG_ERR_REFINE 256  /* a refinement scan's symbol with a size other than 0 or 1 */
#define GAN_JPEGPROG_ERR_EOBRUN 512  /* an end-of-band run that outlasts the blocks of its segment */
#define GAN_JPEGPROG_ERR_COEF 1024   /* a coefficient outside int16 */
/* Host only.  off[0] gan_jpegprog_image, off[1] scans, off[2] segments, off[3] dht, off[4] qt, off[5] scan bytes. */
int gan_jpegprog_block_offsets(int n, int nscan, int nseg, int nver, int64_t* off);
/* Host only.  Fills coef_off and plane_off of imgs[0 .. n-1] (host memory) and gives the workspace size. */
int gan_jpegprog_bounds(gan_jpegdec_image* imgs, int n, int nver, int64_t* ws_bytes);
/* One wave per table version: the decode tables of gan_jpegdec_tables.  Also zeroes the error words and the coefficient area with one
 * memset.  blk_host: the host copy of the block's descriptors, which every entry validates. */
int gan_jpegprog_tables(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nscan, int nseg, int nver, void* ws, int64_t ws_bytes,
                        void* stream);
/* One 64-lane workgroup per image; a lane takes one (scan, restart segment).  The levels run one after the other with a workgroup
 * barrier between them; the segments of one level, which touch disjoint int16 slots, run on different lanes at the same time.  The
 * file's first 16 table versions are held in LDS, later ones are read from the workspace.  ITU-T T.81 Annex G as libjpeg reads it. */
int gan_jpegprog_entropy(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nscan, int nseg, int nver, void* ws, int64_t ws_bytes,
                         void* stream);
/* gan_jpegdec_idct and gan_jpegdec_pixels over this block. */
int gan_jpegprog_idct(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nscan, int nseg, int nver, void* ws, int64_t ws_bytes,
                      void* stream);
int gan_jpegprog_pixels(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nscan, int nseg, int nver, void* ws, int64_t ws_bytes,
                        uint8_t* out, int64_t out_bytes, int32_t* err, void* stream);

/* ---- PNG decoder on the device: the pixels Image.open(p).convert("RGB") gives, for the files a host parser accepted: no interlace,
 *      compression and filter method 0, colour type 0, 2, 4 or 6 at 8 bits (grey is replicated, alpha dropped, no compositing) or colour
 *      type 3 at 1, 2, 4 or 8 bits with a PLTE that covers every index its depth can give (a plain lookup; tRNS changes nothing).  The
 *      parser has checked every chunk's CRC, concatenated the IDAT payloads to one zlib stream and checked its two header bytes.
 *      Integer arithmetic only.  The stream is untrusted: every loop of the kernels is bounded by the stream's bit count or by the raw
 *      byte count H (1 + rowbytes) of the descriptor, every load lies inside the file's 16-byte-padded stream, every store address comes
 *      from counters clamped to the descriptor's extent, and an irregularity sets bits of the file's error word (GAN_PNGDEC_ERR_*) and
 *      ends that file's work; the caller sends such a file to the host decoder.  No atomics: the same bytes come out every time.
 *
 *      One upload block carries everything (all offsets from its start, n files):
 *        gan_pngdec_image [n] | uint8 palettes [n][768] (R, G, B per entry, zeros behind pal_count) | zlib streams, each at a multiple of 16
 *      gan_pngdec_block_offsets gives the byte offsets.  Workspace (16-byte aligned, gan_pngdec_bounds bytes): error words int32 [n] |
 *      per file the inflated bytes (the filtered scanlines: H rows of one filter byte and rowbytes bytes), each area at a multiple of 256.
 *      GAN_PNGDEC_MAX_ROWBYTES: the longest row the unfilter kernel's two LDS rows hold, 4096 pixels of RGBA.
 *      Refused with a message, before any launch: a NULL pointer, n outside 1 .. 65535, H or W below 1, a colour type / depth outside
 *      the class above, bpp or rowbytes that do not belong to them, rowbytes above GAN_PNGDEC_MAX_ROWBYTES, H (1 + rowbytes) or H W 3
 *      at or above 2^31, a palette of fewer entries than 1 << depth or more than 256, window bits outside 8 .. 15, a stream that is
 *      shorter than 7 bytes, not at a multiple of 16 or not inside the block, a block of 2^31 bytes or more, a workspace that is too
 *      small or not 16-byte aligned, raw or output offsets that leave their buffers. */
#define GAN_PNGDEC_MAX_ROWBYTES 16384
typedef struct gan_pngdec_image {
  int32_t H, W;
  int32_t color, depth;              /* PNG colour type 0 | 2 | 3 | 4 | 6 and bit depth (8; 1 | 2 | 4 | 8 for colour type 3) */
  int32_t bpp, rowbytes;             /* the filters' pixel step in bytes, max(1, channels depth / 8); ceil(W channels depth / 8) */
  int32_t pal_count;                 /* PLTE entries (colour type 3), else 0 */
  int32_t wbits;                     /* CINFO + 8 of the zlib header: no distance may exceed 1 << wbits */
  int32_t stream_off, stream_len;    /* the whole zlib stream in the block: 2 header bytes, deflate data, Adler-32 */
  int32_t reserved[2];
  int64_t raw_off;                   /* bytes into the workspace (filled by gan_pngdec_bounds) */
  int64_t out_off;                   /* bytes into `out` of gan_pngdec_pixels: where the packed (H, W, 3) image goes */
} gan_pngdec_image;
#define GAN_PNGDEC_ERR_BTYPE 1       /* block type 3 */
#define GAN_PNGDEC_ERR_STORED 2      /* a stored block whose LEN is not ~NLEN */
#define GAN_PNGDEC_ERR_COUNTS 4      /* more than 286 literal/length or more than 30 distance code lengths */
#define GAN_PNGDEC_ERR_REPEAT 8      /* a code-length repeat with no previous length, or one that runs past HLIT + HDIST */
#define GAN_PNGDEC_ERR_OVER 16       /* an over-subscribed set of code lengths */
#define GAN_PNGDEC_ERR_INCOMPLETE 32 /* an incomplete set, other than a single literal/length or distance code of length 1 */
#define GAN_PNGDEC_ERR_NOEOB 64      /* no end-of-block code */
#define GAN_PNGDEC_ERR_SYMBOL 128    /* literal/length symbol 286 | 287, distance symbol 30 | 31, or bits that are no code at all */
#define GAN_PNGDEC_ERR_DIST 256      /* a distance beyond the bytes produced so far, or beyond the window the header declares */
#define GAN_PNGDEC_ERR_END 512       /* bits needed beyond the stream */
#define GAN_PNGDEC_ERR_MORE 1024     /* more output than H (1 + rowbytes) */
#define GAN_PNGDEC_ERR_LESS 2048     /* less output than that at the final block */
#define GAN_PNGDEC_ERR_LEFT 4096     /* bytes between the final block and the Adler-32 */
#define GAN_PNGDEC_ERR_FILTER 8192   /* a filter byte above 4 */
#define GAN_PNGDEC_ERR_ADLER 16384   /* the Adler-32 of the inflated bytes is not the stream's */
/* Host only.  Byte offsets of the block's parts for n files: off[0] palettes, off[1] the first stream. */
int gan_pngdec_block_offsets(int n, int64_t* off);
/* Host only.  Fills raw_off of imgs[0 .. n-1] (host memory) and gives the workspace size. */
int gan_pngdec_bounds(gan_pngdec_image* imgs, int n, int64_t* ws_bytes);
/* One 64-lane workgroup per file: RFC 1951 inflate of stored, fixed and dynamic blocks.  The tables of the current block (a 9-bit
 * lookahead table plus canonical max-code / offset arrays and the symbols in code order) and the 32 KiB window live in LDS; the
 * wave builds the tables together.  Every lane carries the same 64-bit bit buffer, refilled from aligned 8-byte chunks with the next
 * chunk already requested, so a symbol, a length and a distance are wave-uniform without an exchange, and the whole wave copies a
 * match inside the window (byte k of a match comes from k mod distance: an overlapping match reads only bytes that were there before
 * it).  The window is written to the file's raw area 16 KiB at a time, 16 bytes per lane; nothing is read back from there.
 * Overwrites the file's error word.  blk_host: the host copy of the block's descriptors, which every entry validates. */
int gan_pngdec_inflate(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, void* ws, int64_t ws_bytes, void* stream);
/* One 64-lane workgroup per file, the previous and the current row in LDS, rows in order: filter 0 None, 1 Sub, 2 Up, 3 Average
 * ((left + up) >> 1 in 9 bits), 4 Paeth (ties: left, then up); the row above the first is zero, and so is the pixel left of the
 * first.  None and Up run over all bytes at once; Sub is a prefix sum per byte of the pixel (every lane sums its own stretch of pixels, then adds what the
 * stretches in front of it came to); Average and Paeth walk the row with one lane per byte of the pixel.  Then 1, 2
 * and 4-bit indices are unpacked most significant bit first (the padding bits of a row are not looked at), and palette lookup, grey
 * replication or alpha drop give image i packed (H, W, 3) at out + out_off.  The Adler-32 is summed row by row over the bytes as they
 * are read.  A file whose error word is set is left alone.  err (may be NULL): int32 [n] on the device, receives the error words. */
int gan_pngdec_pixels(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, void* ws, int64_t ws_bytes, uint8_t* out,
                      int64_t out_bytes, int32_t* err, void* stream);

/* ---- Evaluation (csrc/mifid.hip): the float64 work of FID / MiFID over feature matrices (the reference's EVAL/eval/mifid.py does it
 *      with numpy on the host and a float32 torch loop).  A feature matrix is row-major GAN_FEAT_F32 or GAN_FEAT_F64 with a row stride
 *      ld >= cols, in elements.  Values are promoted to float64 when loaded, every sum is float64 and runs in a fixed order, nothing
 *      uses a floating-point atomic: a repeated call repeats its bits.  Outputs are float64 unless stated.  Nothing past an output's
 *      extent (or inside the padding of its rows) is written.  Every entry validates first and launches nothing when it refuses. */
enum { GAN_FEAT_F32 = 0, GAN_FEAT_F64 = 1 };
/* X (n x D) -> mean [D] (column means), colcss [D] (sum_i (x_ij - mean_j)^2, from a second pass over the data, never sum x^2 - n mean^2),
 * norm [n] (row L2 norms), rowsum [n], css [1] (the sum of colcss: the centred sum of squares, (n - 1) tr cov), flag (int32 [1]):
 * non-zero when any element is NaN or Inf. */
int gan_feat_moments(const void* X, int dtype, int64_t n, int64_t D, int64_t ld, double* mean, double* colcss, double* norm, double* rowsum,
                     double* css, int32_t* flag, void* stream);
/* One contraction on v_mfma_f64_16x16x4_f64, 64 x 64 output tiles, any positive extents up to INT_MAX - 64 (M at most 65535 tiles):
 *   trans = 0: A is M x K, B is N x K:  C[i][j] = alpha * sum_k ((A[i][k] - ca[k]) ra[i]) ((B[j][k] - cb[k]) rb[j])
 *   trans = 1: A is K x M, B is K x N:  C[a][b] = alpha * sum_i (A[i][a] - ca[a]) (B[i][b] - cb[b])        (ra, rb must be NULL)
 * ca / cb NULL: no centring; ra / rb NULL: scale 1.  Centring, scaling and the conversion to float64 happen on the way into LDS.
 * C is M x N float64 with row stride ldc >= N.  A and B may be the same matrix. */
int gan_gram_f64(const void* A, int a_dtype, int64_t lda, const void* B, int b_dtype, int64_t ldb, int trans, int M, int N, int K,
                 const double* ca, const double* cb, const double* ra, const double* rb, double alpha, double* C, int64_t ldc, void* stream);
/* For every row i of A: dmin[i] = min_j d_ij and imin[i] (int32) = the lowest j that attains it, d_ij = 1 - s_ij (absolute = 1:
 * 1 - |s_ij|), s the trans = 0 product above.  Rows and columns whose scale is exactly 0 are left out: such a row, or a row with no
 * column left, gets +inf and -1.  The M x N matrix is never written: every workgroup reduces its tile to per-row (min, index) pairs in
 * ws ([column tiles][M] float64, then the same as int32, gan_cos_rowmin_bounds bytes, 16-byte aligned) and a second launch folds the
 * column tiles in ascending order. */
int gan_cos_rowmin_bounds(int M, int N, int64_t* ws_bytes);
int gan_cos_rowmin(const void* A, int a_dtype, int64_t lda, const void* B, int b_dtype, int64_t ldb, int M, int N, int K, const double* ca,
                   const double* cb, const double* ra, const double* rb, double alpha, int absolute, void* ws, int64_t ws_bytes, double* dmin,
                   int32_t* imin, void* stream);
/* The selection step (the reference's EVAL/scripts/select_7k.py).  Column transform: an element x of column k becomes (x - c[k]) * s[k]
 * on its way into LDS or into a sum, two rounded float64 operations in that order; c and s are float64 [K], each may be NULL (no
 * centre, scale 1), per operand.
 * For every row i of A (M x K): dmin[i] = min_j d_ij and imin[i] (int32) = the lowest j that attains it,
 *   d_ij = max(0, na_i + nb_j - 2 a'_i . b'_j),  a' / b' the transformed rows of A / B (N x K), na / nb their squared norms,
 * the norms from a row kernel (one wave per row, fixed order) into the head of ws, the products on the contraction tile above.  No row
 * or column is left out.  The M x N matrix is never written: ws holds na [M], nb [N], then per-tile (min, index) pairs as for
 * gan_cos_rowmin (gan_sqdist_rowmin_bounds bytes, 16-byte aligned); a last launch folds the column tiles in ascending order.
 * Extents as for gan_cos_rowmin. */
int gan_sqdist_rowmin_bounds(int M, int N, int64_t* ws_bytes);
int gan_sqdist_rowmin(const void* A, int a_dtype, int64_t lda, const void* B, int b_dtype, int64_t ldb, int M, int N, int K, const double* ca,
                      const double* sa, const double* cb, const double* sb, void* ws, int64_t ws_bytes, double* dmin, int32_t* imin,
                      void* stream);
/* k-means update: sums[j][d] = sum over the rows i with labels[i] == j, in ascending i, of the transformed x'_id (float64 [k][D], row
 * stride lds >= D; a cluster without rows gets exact zeros), counts[j] (int32 [k]) their number, *err (int32) non-zero when a label
 * lies outside [0, k); such rows are skipped.  One workgroup per (cluster, 256 columns); the member rows are compacted in order into
 * 1 KiB of LDS whatever k is, so k is bounded only by INT_MAX - 64 and D by 65535 strips of 256 columns. */
int gan_kmeans_update(const void* X, int dtype, int64_t n, int64_t D, int64_t ld, const double* c, const double* s, const int32_t* labels,
                      int k, double* sums, int64_t lds, int32_t* counts, int32_t* err, void* stream);

/* ---- losses. Every loss writes its value to *loss (device fp32, overwritten) and the gradient wrt its input.
 *      hinge: adv_hinge.py:6-62 (mode 0: mean relu(1-x), 1: mean relu(1+x), 2: -mean x), scaled by `scale`;
 *      lsgan/bce: Basic_GAN/src/losses.py:5-22 (mode 3: mse vs target, 4: bce-with-logits vs target in {0,1});
 *      l1: identity_l1.py:18-20 and Basic_GAN/src/losses.py:24-30 (target given as NCHW fp32).
 *      gan_patch_loss reads channel 0 of the logits: *loss = scale * mean f, grad = scale / n * f' in channel 0 and 0 in channels 1..7
 *      (grad->C must be 8); the hinge derivative at the kink (x == 1 for mode 0, x == -1 for mode 1) is 0, as relu' is in torch.
 *      gan_l1_loss: sign(0) = 0.  The gradient views' halos are never written; channels C..7 of their interior pixels are written as 0.
 *      ws of gan_l1_loss and gan_r1_reduce: fp32, [0 .. 512) is written, nothing past it.  Repeated calls repeat their bits.
 *      Non-finite data: one NaN in an element that is read (channel 0 of a logit; a real channel of x, target_nchw or g) makes *loss
 *      NaN in every mode of gan_patch_loss, in gan_l1_loss and in gan_r1_reduce; one +-Inf makes it what the formula gives in IEEE
 *      arithmetic -- not finite, except for a hinge on its flat side (relu(1 - Inf) = 0).  Pad channels and halos are never read: a NaN
 *      or Inf there changes nothing.  The gradient of a NaN or Inf element itself (0 or NaN) is unspecified; the gradients of
 *      the other elements are unaffected. */
int gan_patch_loss(const gan_view* logits, int mode, float target, float scale, float* loss, const gan_view* grad, void* stream);
int gan_l1_loss(const gan_view* x, int C, const float* target_nchw, float scale, const float* dev_grad_scale, float* loss,
                const gan_view* grad, float* ws, void* stream);   /* grad additionally * (*dev_grad_scale) if non-NULL */
/* r1 = (1/B) sum_b sum_chw g^2 (train_cutpp.py:201) and u = scale * 2 g / B into `u` (interior) */
int gan_r1_reduce(const gan_view* g, int C, float scale, float* loss, const gan_view* u, float* ws, void* stream);

/* ---- palette prior: low-frequency CIE-Lab statistics (GAN_Variant1/dataio/transforms.py:52-54 denormalize, :57-96 rgb_to_lab,
 *      :99-119 get_low_freq_stats), a loss against a running prior and its gradient wrt the image.  The reference's file that combined
 *      them (losses/palette_prior_lab.py) is gone; the loss below is this project's statement (DESIGN.md "Palette prior").
 *      x: fp32 or bf16 view, C = 8, channels 0..2 real, values in [-1, 1] (clamped like the reference); any halo.  T = low_freq_size
 *      in [2, 1024] (T = 1: error; the unbiased std of one cell is NaN).
 *      gan_palette_stats: cells[B][T*T][3] fp32 = adaptive_avg_pool2d of Lab to T x T (cell i covers rows floor(i H / T) ..
 *      ceil((i + 1) H / T) - 1, columns likewise), then stats[B][3][2] fp32 = (mean of the T*T cells, their unbiased std) per image and
 *      channel (L, a, b), taken in two fp64 passes over the stored cells.  Two launches.
 *      gan_palette_batch_mean: batch[3][2] = mean over the B images of stats.
 *      gan_palette_prior_update: v = batch * batch_scale (batch_scale = 1 / ranks after a summing all-reduce of `batch`);
 *      prior[3][2] = v if !use_ema or *steps == 0, else decay * prior + (1 - decay) * v; then ++*steps (device int32).
 *      gan_palette_loss: *loss = scale / (3B) * sum_{b,c} (|m - m_prior| + |s - s_prior|) / 100 (overwritten);
 *      gstats[B][3][2] (may be NULL) = the derivative of the UNSCALED loss wrt stats, sign(0) = 0.
 *      gan_palette_bwd: channels 0..2 of gx's interior pixels = (accumulate: +=) scale * dLoss/dx, with cells / stats / gstats of the
 *      calls above for the same x: per cell gm / N + gs (cell - m) / ((N - 1) s) (the gs term is 0 where s == 0), spread over the
 *      cell's pixels, then the transposed Jacobian of the Lab chain recomputed from x -- at every `where` the derivative of the branch the
 *      forward took, clamp passing the gradient on [0, 1] inclusive.  Every value is finite for every finite x.  accumulate = 0 writes
 *      channels 3..7 of interior pixels as 0; accumulate = 1 leaves their bits.  Halos of gx are never written.
 *      Halos and pad channels of x are never read: a NaN there changes nothing.  A NaN in a real channel makes that image's cells and
 *      stats, and through them *loss, NaN; the statistics and gradients of the other images are unaffected.
 *      Fixed-order reductions (fp32 per lane, fp64 across lanes), no atomics: repeated calls repeat their bits. */
int gan_palette_stats(const gan_view* x, int T, float* cells, float* stats, void* stream);
int gan_palette_batch_mean(const float* stats, int B, float* batch, void* stream);
int gan_palette_prior_update(const float* batch, float batch_scale, float* prior, int32_t* steps, int use_ema, float decay, void* stream);
int gan_palette_loss(const float* stats, const float* prior, int B, float scale, float* loss, float* gstats, void* stream);
int gan_palette_bwd(const gan_view* x, int T, const float* cells, const float* stats, const float* gstats, float scale,
                    const gan_view* gx, int accumulate, void* stream);

/* ---- feature matching between two discriminator feature maps (csrc/featmatch.hip): the term behind loss_weights.featmatch, over what
 *      MultiscaleDiscriminator.get_intermediate_features returns (GAN_Variant1/models/discriminator_patchgan.py:65-72, 118-128).  The
 *      reference's file that made a loss of them (losses/feat_matching.py) is gone; the statement is this project's.
 *      f (fake), r (real) and g share B, H, W and dtype (GAN_F32 or GAN_BF16); each has its own halo and its own C >= the C of the
 *      call (the real channels).  With n = B*H*W*C, over the interior elements of channels [0, C):
 *        *loss += (float)(S * ((double)loss_scale / (double)n)),   S = sum |f - r|      (one fp32 `+=` onto the slot, as gan_patchnce_fwd:
 *                                                                                        one slot collects every layer after one fill)
 *        g (accumulate: +=) v,   v = +m where f - r > 0, -m where f - r < 0, else 0 (sign(0) = 0; a NaN difference gives 0),
 *                                m = act == GAN_ACT_LRELU and not f > 0 ? inv02 : inv   (gan_act_bwd's convention: factor 0.2 at f == 0)
 *        in fp32, exactly:  inv = grad_scale / (float)n  (n converted to fp32, round to nearest; one division),  inv02 = 0.2f * inv  (one
 *        product);  f - r is one fp32 subtraction of the stored values;  accumulate = 0: g = round_to_dtype(v);  accumulate = 1:
 *        g = round_to_dtype((float)g + v), one fp32 addition.  Nothing else rounds: tests hold g to this bit for bit.
 *      g may be NULL (loss only).  act: GAN_ACT_NONE or GAN_ACT_LRELU.  Halos and channels >= C of f and r have no effect on any result and
 *      those of g keep their bits (g's zero halo is what the next input gradient relies on).  Mismatched geometry, another dtype or act,
 *      C outside (0, min C of the views], B*H*W*ceil(C/N) >= 2^31 or a workspace that is not 8-byte aligned: error, nothing is launched.
 *      Accumulation of S (N = 8 bf16 or 4 fp32 elements per 16-byte chunk): the chunks of the interior, items = B*H*W*ceil(C/N) in
 *      (b, y, x, chunk) order, are dealt round-robin to nblocks * 256 lanes, nblocks = min(2048, ceil(items / 256)).  A lane adds |f - r| of
 *      its chunks' real elements to ONE fp32 sum in that order: a chain of at most L = N * ceil(items / (256 nblocks)) terms.  Lanes are
 *      added in fp64 (fixed tree) to one fp64 partial per block in ws (2 floats each: gan_featmatch_ws_floats(f) = 2 * nblocks at C = f->C,
 *      enough for every C), and a one-block second launch adds the partials in fp64 in a fixed order.  No atomics: a repeated call repeats
 *      its bits.  Error bound that follows: every term takes one rounding in its subtraction and every fp32 partial sum of non-negative
 *      terms one more, so |S_computed - S| <= L * 2^-24 * S (first order; the fp64 stages add 2^-53 per step); the value added to the
 *      slot is then rounded to fp32 once and the `+=` rounds once:
 *        |*loss_after - (*loss_before + loss_scale S / n)| <= (L + 1) * 2^-24 * loss_scale S / n + 2^-24 * |*loss_after|.
 *      Non-finite data, as gan_l1_loss: one NaN in a real, interior element of f or r makes *loss NaN; the gradient of that element is
 *      unspecified, the gradients of the other elements are unaffected. */
int64_t gan_featmatch_ws_floats(const gan_view* f);
int gan_featmatch(const gan_view* f, const gan_view* r, int C, float loss_scale, float* loss, float grad_scale, int act,
                  const gan_view* g, int accumulate, float* ws, void* stream);

/* ---- PatchNCE (GAN_Variant1/losses/patchnce_cut.py:42-110) for one feature layer.
 *      ids: device int32 [P] positions in [0,H*W).  ws: fp32 workspace >= gan_patchnce_ws_floats(B,P,C).
 *      fwd: *loss += weight * mean_b CE.  bwd: grad rows of tgt (scaled by weight) are ADDED into `gtgt`
 *      (duplicates in ids accumulate); channels >= C and halos of `gtgt` are never written.
 *      Non-finite data: an image whose mean CE is not finite (an Inf or NaN in one of its sampled rows; the
 *      clamp to +-50 passes a NaN on, as torch.clamp does) counts as the constant 0: it adds nothing to the
 *      loss, its flag is 0, its rows of dX are exactly 0 and its part of `gtgt` keeps its bits.  The other
 *      images are unaffected; values outside the sampled rows are never read.
 *      Range: the row norm sqrt(sum_c x^2) is evaluated in fp32, so sampled rows must have ||x|| < 1.8e19
 *      (sum x^2 below FLT_MAX; beyond it the norm is Inf and the row normalises to zeros).  Rows below
 *      about 1e-19, whose squares underflow, fall to the eps branch x / 1e-6 like every row of norm
 *      <= 1e-6, in agreement with the reference.
 *      Workspace layout (floats, in this order; tests read it):
 *        Sn[B][P][C] | Tn[B][P][C]   normalised source / target rows, x / max(||x||, 1e-6)
 *        tnorm[B][P]                 max(||target row||, 1e-6)
 *        lse[B][P] | rowloss[B][P]   log-sum-exp of the clamped logits of row i; lse - logit(i, i)
 *        flag[(B+3)/4*4]             1 where the image's mean CE is finite, else 0 (entries >= B unused)
 *        dX[B][P][C]                 gradient rows before the scatter (written by bwd)
 *      followed by 64 unused floats: gan_patchnce_ws_floats = 3 B P C + 3 B P + (B+3)/4*4 + 64. */
int64_t gan_patchnce_ws_floats(int B, int P, int C);
int gan_patchnce_fwd(const gan_view* src, const gan_view* tgt, const int32_t* ids, int P, int C, float temperature,
                     float weight, float* loss, float* ws, void* stream);
int gan_patchnce_bwd(const gan_view* tgt, const int32_t* ids, int P, int C, float temperature, float weight,
                     const gan_view* gtgt, float* ws, void* stream);

/* ---- PatchNCE with negatives from the whole minibatch (patchnce.nce_includes_all_negatives_from_minibatch; the reference holds only
 *      the key, so the statement is this project's: the per-image statement above with the batch loop removed).
 *      One call scores the Q = B*P normalised target rows (queries; row b*P + i) against K = segs*Q normalised source rows (keys): segment
 *      s is keys + s*seg_stride, Q rows of C floats; segment `self` holds the keys of the call's own rows, and the positive of query i is
 *      key self*Q + i.  Single rank: keys = ws (the workspace's own Sn), segs 1, seg_stride 0, self 0.  Data parallel, rank r of W: every
 *      rank's Sn in rank order, segs = W, self = r.
 *        raw_ij    = <Tn_i, Key_j> / T;   lg = clamp(raw, -50, 50)   (a NaN stays a NaN)
 *        rowloss_i = logsumexp_j lg_ij - lg_{i, self*Q+i}
 *        call      = mean_i rowloss_i;   flag = isfinite(call);   *loss += weight * (flag ? call : 0)
 *        dlg_ij    = weight * flag * (softmax_ij - [j = self*Q+i]) / Q,   0 where raw is outside [-50, 50]
 *        dTn = dlg . Key / T;   dX_i = (dTn_i - Tn_i <Tn_i, dTn_i>) / ||x_i||  where ||x_i|| > 1e-6, else dTn_i / 1e-6
 *      With B = 1, segs = 1 this is gan_patchnce_fwd / bwd's statement.  One non-finite key row anywhere, or one non-finite target row,
 *      makes the call's flag 0: nothing is added to the loss, every row of dX is exactly 0 and `gtgt` keeps its bits.
 *      gan_patchnce_all_gather writes Sn, Tn, tnorm (and nothing else); gan_patchnce_all_fwd reads Tn and the keys and writes lse, rowloss
 *      and all B entries of flag (each the call's flag); gan_patchnce_all_bwd reads Tn, tnorm, lse, flag and the keys, writes dX and ADDS
 *      its rows into `gtgt` (duplicates in ids accumulate; channels >= C and halos are never written).  The keys are only read.
 *      Workspace: gan_patchnce_all_ws_floats = gan_patchnce_ws_floats, the same layout in the same order (tests read it), rows indexed
 *      b*P + i; no logit is ever stored and the kernels need no further scratch.  Q rows in tiles of 16, keys in trips of 256, channels
 *      in chunks of 64 on v_mfma_f32_16x16x4_f32 where C % 64 == 0, C <= 256 and Q % 16 == 0; a scalar path takes every other shape
 *      (1 <= P <= 256, 1 <= C <= 512 as above).  Fixed-order sums, no atomics: repeated calls repeat their bits.
 *      Refused arguments (also: keys NULL, self outside 0..segs-1, segs > 1 with seg_stride < Q*C) return their error and write nothing. */
int64_t gan_patchnce_all_ws_floats(int B, int P, int C);
int gan_patchnce_all_gather(const gan_view* src, const gan_view* tgt, const int32_t* ids, int P, int C, float* ws, void* stream);
int gan_patchnce_all_fwd(const gan_view* tgt, int P, int C, float temperature, float weight, const float* keys, int segs,
                         int64_t seg_stride, int self, float* loss, float* ws, void* stream);
int gan_patchnce_all_bwd(const gan_view* tgt, const int32_t* ids, int P, int C, float temperature, float weight, const float* keys,
                         int segs, int64_t seg_stride, int self, const gan_view* gtgt, float* ws, void* stream);

/* ---- fused clip_grad_norm_ + Adam + EMA (amp_utils.py:29-41, sched_optim.py:5-27, io_ckpt.py:23-29) over a
 *      tensor list.  The table is a device array of gan_adam_tensor; tensors with g == NULL are skipped. */
typedef struct gan_adam_tensor {
  float* p; const float* g; float* m; float* v; float* ema;   /* ema may be NULL */
  int64_t numel;
  int32_t* step;                                               /* device per-tensor step counter (incremented) */
  int64_t _pad;
} gan_adam_tensor;
/* norm_out: device fp32 [3] = (total L2 norm before clipping, clip coefficient, found_inf).  max_norm <= 0: no clipping.
 * grad_scale multiplies every gradient first (1/world_size after a sum all-reduce).
 * lr_dev (optional device float): the learning rate is read from it instead of `lr` -- a scheduler (Basic_GAN/src/train.py:27-31,54-58,125:
 *   LambdaLR with lambda_rule) rewrites one device float and the prebuilt launch stays valid.
 * inv_scale_dev (optional device float) and skip_nonfinite: torch.amp.GradScaler's unscale_ / step (amp_utils.py:29-41): gradients are
 *   multiplied by *inv_scale_dev, and with skip_nonfinite a non-finite total norm skips the update AND the step counters; found_inf is
 *   written to norm_out[2] either way (gan_scaler_update consumes it).
 * Extents: ws >= nchunks floats, all of them written; norm_out 3 floats; chunk k is the slice [chunk_off[k], chunk_off[k] + 16384) of
 *   tensor chunk_tensor[k], cut at numel; the table has to cover every element of every tensor once.  Slices need no alignment.
 * Scalars: beta1, beta2 and ema_decay are fp32, and 1 - beta is formed in fp32 from them; for beta2 = 0.999 that is 1.3e-5 (relative)
 *   away from the 1 - 0.999 torch forms in double.  The bias corrections 1 - beta^t are evaluated in fp64 from the fp32 betas and the
 *   device step counters (int32), then rounded once.  norm_out[1] is the coefficient applied; every element is the fp32 evaluation of
 *   torch's single-tensor expression with that coefficient (tests/optim_cases.py counts its roundings).
 * Range: the squares of the scaled gradients stay normal and their sum finite for 2^-63 <= |g * scale| < 2^64 / sqrt(number of live
 *   elements); smaller gradients add at most 2^-126 each to the sum of squares, larger ones give an Inf norm (below).
 * Non-finite gradients (skipped tensors are never read: a NaN in their p, m, v stays where it is and touches nothing):
 *   skip_nonfinite = 1: norm_out[0] holds the NaN / Inf norm, norm_out[2] = 1, nothing else is written and no counter moves.
 *   skip_nonfinite = 0, as torch.nn.utils.clip_grad_norm_ + Adam.step behave: with clipping on, a NaN gives the coefficient NaN
 *     (clamp keeps it) and p, m, v of EVERY live tensor go NaN; an Inf gives the coefficient 0, the Inf element goes NaN (Inf * 0) and
 *     all others take a zero gradient.  Without clipping only the non-finite elements go non-finite.  The counters move.
 * Refused arguments (NULL table / chunk arrays / norm_out / ws, ntensors or nchunks <= 0) return -1 and launch nothing. */
int gan_adam_step(const gan_adam_tensor* table, int ntensors, const int32_t* chunk_tensor, const int64_t* chunk_off,
                  int nchunks, float lr, float beta1, float beta2, float eps, float max_norm, float grad_scale,
                  float ema_decay, const float* lr_dev, const float* inv_scale_dev, int skip_nonfinite, float* norm_out, float* ws, void* stream);
/* gan_adam_step with torch's weight decay (sched_optim.py:16-25 hands optim.{G,D}.weight_decay to torch.optim.Adam).  The arguments are
 * gan_adam_step's in order, with weight_decay and decoupled in front of norm_out; everything said above holds, and in addition:
 * weight_decay == 0: the kernels of gan_adam_step are launched, so every result equals gan_adam_step's bit for bit.
 * decoupled = 0, torch.optim.Adam(weight_decay) (torch/optim/adam.py: grad = grad.add(param, alpha = weight_decay)).  The reference runs
 *   unscale_ -> clip_grad_norm_ -> step, so the decay meets the gradient after scaling and clipping:
 *   g_eff = g * (grad_scale * *inv_scale_dev * coef) + weight_decay * p_old, and m, v and p are gan_adam_step's expressions on g_eff.
 * decoupled = 1, torch.optim.AdamW / Adam(decoupled_weight_decay = True): p' = p_old * (1 - rate * weight_decay), rate = *lr_dev when
 *   given, else lr; m and v come from the undecayed gradient; p_new = p' - (rate / bc1) * m / denom.
 * Both: the decay is NOT part of norm_out[0] (the norm), norm_out[1] (the coefficient) or norm_out[2] (found_inf): the norm is that of
 *   the scaled gradients alone.  The EMA shadow reads p_new.  A tensor with g == NULL is not touched and not decayed (torch skips a
 *   parameter without a gradient entirely).  p is read anyway: no load or store is added, 28 B/param (36 with EMA).
 * Roundings, all fp32: decoupled = 0 adds the product weight_decay * p_old and its sum with the scaled gradient (or one fma) in front of
 *   gan_adam_step's chain; decoupled = 1 adds rate * weight_decay, 1 - that (both once per block) and the product with p_old in front
 *   of the final subtraction.
 * Non-finite gradients: skip_nonfinite = 1: as gan_adam_step -- nothing but norm_out is written, so nothing is decayed either.
 *   skip_nonfinite = 0: gan_adam_step's table with g_eff in place of g: a NaN coefficient makes p, m, v of every live tensor NaN; the
 *   coefficient 0 after an Inf leaves g_eff = weight_decay * p (decoupled = 0) or 0 (decoupled = 1) for the finite elements and NaN at the Inf one.
 * Refused, with -1 and nothing launched: gan_adam_step's cases, weight_decay < 0 or NaN, decoupled outside {0, 1}. */
int gan_adam_step_wd(const gan_adam_tensor* table, int ntensors, const int32_t* chunk_tensor, const int64_t* chunk_off,
                     int nchunks, float lr, float beta1, float beta2, float eps, float max_norm, float grad_scale,
                     float ema_decay, const float* lr_dev, const float* inv_scale_dev, int skip_nonfinite, float weight_decay, int decoupled,
                     float* norm_out, float* ws, void* stream);
/* torch.amp.GradScaler.update on the device (amp_utils.py:22,41): scale *= backoff_factor after an overflow (found_inf != 0, e.g.
 * norm_out + 2 of gan_adam_step), *= growth_factor after growth_interval clean steps; inv_scale = 1 / scale; no host synchronisation.
 * One rounding for the product, one for the reciprocal.  A scale backed off below 2^-126 goes subnormal and 1 / scale overflows to Inf
 * below 2^-128, as the fp32 expressions do: there is no floor.  Refused: a NULL pointer, growth_factor < 1, backoff_factor outside
 * (0, 1], growth_interval <= 0. */
int gan_scaler_update(float* scale, float* inv_scale, int32_t* growth_tracker, const float* found_inf, float growth_factor,
                      float backoff_factor, int growth_interval, void* stream);

/* small helpers: p[0 .. n) = v bit for bit (-0.0, NaN, Inf included); y[0 .. n) += a * x within one rounding of the multiply-add
 * (contracted or not).  n = 0 does nothing; a NULL pointer or n < 0 returns -1 and writes nothing. */
int gan_fill_f32(float* p, int64_t n, float v, void* stream);
int gan_axpy_f32(float* y, const float* x, float a, int64_t n, void* stream);   /* y += a*x */

#ifdef __cplusplus
}
#endif
#endif
