// e4m3 "range-patch" weight gradient: wgrad_patch.hip's kernel on OCP e4m3 operands (fp8 mode, the residual 3x3 256->256 layers).
//
//   part[s][n][t][c] = scale_g[b(s)] * sum over the pixels m of split s of  g8[m][n] * x8[pix(m) + tapoff[t]][c]
//
// x8 is an e4m3 view with unit scale (GPass.in8 / mid8), g8 the e4m3 copy of the output gradient with one scale per image; both already
// exist in fp8 mode (the forward and the input gradient read them), so this launch adds no quantisation pass.  The per-image scale is
// applied in fp32 when a split's accumulators are stored, so a split never crosses an image -- unless the caller promises power-of-two
// scales (gan_wgrad_desc.g_scale_pow2, gan_quantize_fp8_pow2): the MULTI instantiation then sums a split over several whole images, as
// the bf16 kernel does on many small maps, with the image's scale inside the MFMA.  The exponent field of a power-of-two float IS the E8M0
// byte of the instruction's block scale (result x 2^(byte - 127), probed with exact integer data: tools/probe/fp8_mfma_scale.hip); a stage
// of 128 pixels is one k-step inside one image, so its g operand carries exponent_byte(g_scale[b]) in all four bytes of a wave-uniform
// register (lane / byte layout of the scale operand irrelevant), x keeps 0x7f, and one fp32 accumulator set sums over the images.
//
// Same decomposition as the bf16 kernel: a block owns 128 n x 64 c x all 9 taps and walks its pixel range in stages of 128 pixels; the
// g tile (128 pixels x 128 B) and the x window (128/Wo + 2 image rows x 64 B per pixel) are staged once per stage by LDS-DMA.  A stage is
// ONE k-step of v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 both sides, scale byte 0x7f = 1): 36 MFMAs per wave and barrier, at twice the
// bf16 rate, on half the bytes.  Both operands are pixel-major in memory, so the fragments come from ds_read_b64_tr_b8:
//  * per group of 16 lanes it reads a block of 8 rows x 16 byte columns; lane 2q+p of the group supplies the address of row q, columns
//    8p..8p+7, and lane i receives column i, row q in its byte q (probed with exact integer data: tools/probe/ds_read_tr8.hip).
//  * the MFMA's k index is permuted identically for both operands: byte j = 8r + q of lane group fg is pixel 32r + 8fg + q (r: which of
//    the lane's four reads), so one instruction reads 32 CONSECUTIVE pixels and a 32-lane half 16 consecutive rows of the LDS image.
//  * the 16-byte piece index is XOR-ed by row bits (g, 128-byte rows: (row >> 1) & 7; x, 64-byte rows: (row >> 2) & 3): 16 consecutive
//    rows then fall into 16 different 16-byte slots of the 256-byte bank period at ANY pixel shift -- conflict-free transposed reads.
//  * the x window's row pitch is padded to a multiple of 16 pixels: image-row steps (the vertical tap offset, the k offset of narrow
//    maps) never change the swizzle bits and are plain byte offsets; only the three horizontal shifts have their own swizzled base.
//  * 8 waves = 2 (n) x 4 (c); a wave owns 4 n-tiles x 1 c-tile x 9 taps = 36 accumulator tiles (144 registers), as the bf16 kernel.
#include <stdlib.h>
#include <atomic>
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) int v8i_t;
typedef __attribute__((ext_vector_type(2))) int v2i_t;

constexpr int KM = 128;            // pixels per stage = one MFMA k-step
constexpr int NB = 128, CB = 64;   // output tile: g channels x x channels (x all taps)
constexpr int RX = 320;            // x window rows (pixels incl. pitch padding) per stage buffer
constexpr int GT_BYTES = KM * NB, XP_BYTES = RX * CB, STAGE_BYTES = GT_BYTES + XP_BYTES;
constexpr int LDS_BYTES = 2 * STAGE_BYTES;
constexpr int NT = 9;
// RING variant (maps exactly 128 pixels wide: 512x512 images), as in the bf16 kernel: a stage is one image row, the three rows of its
// window live in a ring of four slots (image row y -> slot y & 3) and every stage fetches only its newest row.
constexpr int RING_SLOTS = 4, RING_PITCH = 144;
constexpr int LDS_BYTES_RING = 2 * GT_BYTES + RING_SLOTS * RING_PITCH * CB;

struct Wp8Args {
  const char* x; const char* g; float* part; const float* g_scale;
  int B, HoWo, Wo, lgWo, spi, per;   // spi: splits per image, per: pixels per split (multiple of KM)
  int Cx, N, pitch, nrows;           // pitch: padded window row pitch (pixels, multiple of 16); nrows: image rows per window
  int x_Hp, x_Wp, x_y0, x_x0;
  int g_Hp, g_Wp, g_C, g_y0, g_x0;
  int NBLK, CBLK;
  int ipb;                           // MULTI: whole images per split (spi = 1, HoWo % KM == 0)
};

__device__ __forceinline__ void glds16q(const char* gbase, uint32_t goff, char* lds) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gbase + goff),
                                   (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}
__device__ __forceinline__ v2i_t tr8(const char* p) {
  return __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) v2i_t*)p);
}

template <bool RING, bool MULTI = false>
__global__ __launch_bounds__(512) void wgrad_patch_fp8_kernel(Wp8Args a) {
  static_assert(!(RING && MULTI), "the row-ring variant takes one image per split");
  extern __shared__ __attribute__((aligned(1024))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // XCD-aware block order, as the bf16 kernel: the blocks of one split share its operands in one L2
  int bid = (gridDim.x & 7) == 0 ? (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  const int cb = bid % a.CBLK; bid /= a.CBLK;
  const int nb = bid % a.NBLK; bid /= a.NBLK;
  const int sp = bid;                                  // split index: image b = sp / spi, sub-range sp % spi -- MULTI: ipb whole images from sp * ipb
  const int b = MULTI ? sp * a.ipb : sp / a.spi, sub = MULTI ? 0 : sp - b * a.spi;
  const int m_begin = sub * a.per, m_end = min(a.HoWo, m_begin + a.per);
  const int nst_img = (m_end - m_begin + KM - 1) / KM;   // stages per image
  const int nstage = MULTI ? nst_img * a.ipb : nst_img;  // MULTI: the stage pipeline runs across the images of the split
  const int n0 = nb * NB, c0 = cb * CB;

  // ---- staging roles (LDS-DMA, lane-linear images, XOR applied on the SOURCE chunk)
  // g tile: 128 rows x 128 B; row gr + 64*i (i<2); position gp holds source chunk gp ^ ((row >> 1) & 7)
  const int gr = tid >> 3, gp = tid & 7;
  const uint32_t gsrc = (uint32_t)(n0 + ((gp ^ ((gr >> 1) & 7)) << 4));
  // x window: RX rows x 64 B; row xr + 128*i (i<3); position xp holds source chunk xp ^ ((row >> 2) & 3)
  const int xr = tid >> 2, xp = tid & 3;
  const uint32_t xsrc = (uint32_t)(c0 + ((xp ^ ((xr >> 2) & 3)) << 4));
  const uint32_t x_pixb = (uint32_t)a.Cx, g_pixb = (uint32_t)a.g_C;

  char* const ring = lds + 2 * GT_BYTES;                 // RING: [RING_SLOTS][pitch][64 B] behind the two g tiles
  const uint32_t ring_rowb = (uint32_t)(a.pitch * CB);
  auto load_row = [&](int iy) {                          // RING: one padded image row -> its slot
    char* slot = ring + (uint32_t)(iy & (RING_SLOTS - 1)) * ring_rowb;
    const int iyc = iy < a.x_Hp ? iy : a.x_Hp - 1;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = xr + 128 * i;
      if (row < a.pitch) {                                 // pitch = 144: the second instruction runs in wave 0 only (rows 128..143)
        int ix = row + a.x_x0;
        ix = ix < a.x_Wp ? ix : a.x_Wp - 1;
        glds16q(a.x, (uint32_t)((b * a.x_Hp + iyc) * a.x_Wp + ix) * x_pixb + xsrc, slot + wave * 1024 + i * 8192);
      }
    }
  };
  const int b_first = b;
  auto stage = [&](int st, int buf) {
    char* gt = lds + buf * (RING ? GT_BYTES : STAGE_BYTES);
    char* xw = gt + GT_BYTES;
    const int img = MULTI ? st / nst_img : 0, b = b_first + img;      // MULTI: the image of this stage
    const int m0 = m_begin + (st - img * nst_img) * KM, ho0 = m0 >> a.lgWo;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int m = m0 + gr + 64 * i;
      m = m < a.HoWo ? m : a.HoWo - 1;   // rows past the split end are zeroed after landing
      const int ho = m >> a.lgWo, wo = m & (a.Wo - 1);
      glds16q(a.g, (uint32_t)((b * a.g_Hp + ho + a.g_y0) * a.g_Wp + wo + a.g_x0) * g_pixb + gsrc, gt + wave * 1024 + i * 8192);
    }
    if constexpr (RING) { load_row(ho0 + 2 + a.x_y0); return; }     // the newest of the stage's three rows
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int row = xr + 128 * i;                     // window row = image row wr, column wcol; a wave covers 16 rows, nrows * pitch is a multiple of 16
      if (row < a.nrows * a.pitch) {
        const int wr = row / a.pitch, wcol = row - wr * a.pitch;
        int iy = ho0 + wr + a.x_y0, ix = wcol + a.x_x0;   // pitch padding and rows past the image read a valid (unused) pixel
        iy = iy < a.x_Hp ? iy : a.x_Hp - 1;
        ix = ix < a.x_Wp ? ix : a.x_Wp - 1;
        glds16q(a.x, (uint32_t)((b * a.x_Hp + iy) * a.x_Wp + ix) * x_pixb + xsrc, xw + wave * 1024 + i * 8192);
      }
    }
  };

  const int wn = wave >> 2, wc = wave & 3;
  const int fr = lane & 15, fg = lane >> 4, q = fr >> 1, p = fr & 1;
  // transposed-read geometry: read r of the k-step delivers, to lane group fg, pixels 32r + 8fg + q (q = 0..7 in the lane's bytes)
  const int kl = 8 * fg + q;
  // Per-lane base addresses (read 0).  Read r adds a wave-uniform byte offset: 32r pixels are a multiple of 16 rows (swizzle bits
  // unchanged) and, for Wo >= 16, land on whole image rows or on a multiple of 32 columns, so they never carry into the lane's part.
  uint32_t gbase[4], xbase[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) gbase[i] = (uint32_t)(kl * NB) + ((uint32_t)((wn * 4 + i) * 16 + p * 8) ^ (uint32_t)(((kl >> 1) & 7) << 4));
  const int klrow = (kl >> a.lgWo) * a.pitch + (kl & (a.Wo - 1));   // the lane's pixel inside the window (16-pixel maps: kl spans two image rows)
#pragma unroll
  for (int dx = 0; dx < 3; ++dx) {
    const int r = klrow + dx;
    xbase[dx] = (uint32_t)(r * CB) + ((uint32_t)(wc * 16 + p * 8) ^ (uint32_t)(((r >> 2) & 3) << 4));
  }
  const uint32_t rowb = (uint32_t)(a.pitch * CB);   // bytes per window image row: a multiple of 1024, never touches the swizzle bits
  uint32_t xoff[4];                                 // wave-uniform byte offset of read r inside the window
#pragma unroll
  for (int r = 0; r < 4; ++r) xoff[r] = RING ? (uint32_t)(32 * r * CB) : (uint32_t)((((32 * r) >> a.lgWo) * a.pitch + ((32 * r) & (a.Wo - 1))) * CB);

  f32x4_t acc[4][NT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[i][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  if constexpr (RING) { const int iy0 = (m_begin >> a.lgWo) + a.x_y0; load_row(iy0); load_row(iy0 + 1); }
  stage(0, 0);
  for (int st = 0; st < nstage; ++st) {
    __syncthreads();   // stage st landed (LDS-DMA drained + barrier); everyone is done with the other buffer
    char* gt = lds + (st & 1) * (RING ? GT_BYTES : STAGE_BYTES);
    const char* xw = RING ? ring : gt + GT_BYTES;
    const int img = MULTI ? st / nst_img : 0;
    const int m0 = m_begin + (st - img * nst_img) * KM;
    // MULTI: the g operand's block scale = the exponent byte of this stage's image scale (a power of two), wave-uniform, in all four bytes
    int gsc = 0x7f7f7f7f;
    if constexpr (MULTI) {
      if (a.g_scale) gsc = (int)(((__builtin_bit_cast(uint32_t, a.g_scale[b + img]) >> 23) & 0xffu) * 0x01010101u);
    }
    uint32_t so[3] = {0u, rowb, 2u * rowb};              // byte offset of tap row dy (RING: of its slot)
    if constexpr (RING) {
      const int iy0 = (m0 >> a.lgWo) + a.x_y0;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) so[dy] = (uint32_t)((iy0 + dy) & (RING_SLOTS - 1)) * ring_rowb;
    }
    if (m0 + KM > m_end) {   // tail: pixels past the split end must not contribute -> zero their g rows
      for (int c = tid; c < KM * (NB / 16); c += 512)
        if (m0 + (c >> 3) >= m_end) *reinterpret_cast<u32x4_t*>(gt + c * 16) = u32x4_t{0, 0, 0, 0};
      __syncthreads();
    }
    if (st + 1 < nstage) stage(st + 1, (st + 1) & 1);
    // keep the seven base addresses opaque so that the derived addresses are recomputed (1 add each), not hoisted and spilled
    asm volatile("" : "+v"(gbase[0]), "+v"(gbase[1]), "+v"(gbase[2]), "+v"(gbase[3]), "+v"(xbase[0]), "+v"(xbase[1]), "+v"(xbase[2]));
    v8i_t av[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v2i_t f[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) f[r] = tr8(gt + gbase[i] + (uint32_t)(r * 32 * NB));
      av[i] = v8i_t{f[0][0], f[0][1], f[1][0], f[1][1], f[2][0], f[2][1], f[3][0], f[3][1]};
    }
    // 9 taps: a 3-deep ring of x operands, read two taps ahead of their MFMAs; tap t = (dy, dx) = (t / 3, t % 3)
    v8i_t xv[3];
    auto x_read = [&](int t) {
      v2i_t f[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) f[r] = tr8(xw + xbase[t % 3] + xoff[r] + so[t / 3]);
      xv[t % 3] = v8i_t{f[0][0], f[0][1], f[1][0], f[1][1], f[2][0], f[2][1], f[3][0], f[3][1]};
    };
    x_read(0);
    x_read(1);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t + 2 < NT) x_read(t + 2);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[i][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av[i], xv[t % 3], acc[i][t], 0, 0, 0, MULTI ? gsc : 0x7f7f7f7f, 0, 0x7f7f7f7f);
    }
  }

  // D[row = n (fg*4+e)][col = c (fr)], times the image's dequantisation scale (MULTI: already applied, image by image, in the MFMAs)
  const float sc = (!MULTI && a.g_scale) ? a.g_scale[b] : 1.f;
  float* part = a.part + (int64_t)sp * a.N * NT * a.Cx;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = n0 + (wn * 4 + i) * 16 + fg * 4 + e;
        part[((int64_t)n * NT + t) * a.Cx + c0 + wc * 16 + fr] = acc[i][t][e] * sc;
      }
}

}  // namespace

// gan_wgrad_patch_splits for GAN_FP8 descriptors: splits per image (> 0), or 0 where the e4m3 kernel does not qualify -- also where the
// bf16 query answers negative (several whole images per split): the per-image scale forbids a split that crosses images, unless the
// caller promises power-of-two scales (g_scale_pow2): then the bf16 query's answer, -(images per split), for the MULTI instantiation.
int gan_wgrad_patch_fp8_splits(const gan_wgrad_desc* d) {
  if (d->dtype != GAN_FP8 || d->ntaps != NT || d->Cx % CB != 0 || d->N % NB != 0 || d->N != d->g_C) return 0;
  if (d->x_sy != 1 || d->x_sx != 1 || d->g_sy != 1 || d->g_sx != 1) return 0;
  if (d->Wo < 16 || (d->Wo & (d->Wo - 1)) != 0 || KM % d->Wo != 0 || d->max_tapoff != (2 * d->x_Wp + 2) * d->Cx) return 0;
  const int HoWo = d->Ho * d->Wo;
  if (HoWo < KM) return 0;
  const int pitch = (d->Wo + 2 + 15) / 16 * 16, nrows = KM / d->Wo + 2;
  if (nrows * pitch > RX && !(d->Wo == KM && pitch == RING_PITCH)) return 0;     // 128-wide maps: the row-ring variant
  const int blocks_per_split = (d->N / NB) * (d->Cx / CB);
  if (HoWo < 8 * KM && d->B * blocks_per_split > 256 && HoWo % KM == 0 && nrows * pitch <= RX) {
    int ipb = d->B * blocks_per_split / 256;
    while (ipb > 1 && d->B % ipb != 0) --ipb;
    if (ipb > 1) return d->g_scale_pow2 ? -ipb : 0;
  }
  if (HoWo < 8 * KM && d->B > 64) return 0;
  int spi = (256 + d->B * blocks_per_split - 1) / (d->B * blocks_per_split);   // ~one block per CU
  const int max_spi = HoWo / (2 * KM) > 0 ? HoWo / (2 * KM) : 1;
  if (spi > max_spi) spi = max_spi;
  if (spi < 1) spi = 1;
  return spi;
}

int gan_wgrad_patch_fp8_launch(const gan_wgrad_desc* d, hipStream_t s) {
  const int spi_want = gan_wgrad_patch_fp8_splits(d);
  GAN_CHECK(spi_want != 0, "wgrad: variant=1, dtype GAN_FP8, but the descriptor does not qualify for the e4m3 range-patch kernel");
  const int spi = spi_want > 0 ? spi_want : 1, ipb = spi_want > 0 ? 1 : -spi_want;
  GAN_CHECK(d->x && d->g && d->part, "wgrad_patch_fp8: null pointer");
  GAN_CHECK(((uintptr_t)d->x % 16) == 0 && ((uintptr_t)d->g % 16) == 0, "wgrad_patch_fp8: operand pointers must be 16-byte aligned");
  // the planner's split count must be the one gan_wgrad_patch_splits answered (the kernel indexes partial slabs and images by it)
  // (several images per split only under g_scale_pow2: without the promise the query never answers negative)
  GAN_CHECK(d->nsplit > 0 && (spi_want > 0 ? d->nsplit == d->B * spi : d->nsplit * ipb == d->B),
            "wgrad_patch_fp8: nsplit=%d is not what gan_wgrad_patch_splits implies (B=%d, answer %d)", d->nsplit, d->B, spi_want);
  Wp8Args a;
  a.x = (const char*)d->x; a.g = (const char*)d->g; a.part = d->part; a.g_scale = d->g_scale;
  a.B = d->B; a.HoWo = d->Ho * d->Wo; a.Wo = d->Wo; a.lgWo = __builtin_ctz(d->Wo);
  a.spi = spi; a.ipb = ipb;
  int per = (a.HoWo + a.spi - 1) / a.spi;
  per = (per + KM - 1) / KM * KM;
  a.per = per;
  GAN_CHECK((a.spi - 1) * per < a.HoWo, "wgrad_patch_fp8: nsplit=%d leaves empty splits", d->nsplit);
  a.Cx = d->Cx; a.N = d->N; a.pitch = (d->Wo + 2 + 15) / 16 * 16; a.nrows = KM / d->Wo + 2;
  a.x_Hp = d->x_Hp; a.x_Wp = d->x_Wp; a.x_y0 = d->x_y0; a.x_x0 = d->x_x0;
  a.g_Hp = d->g_Hp; a.g_Wp = d->g_Wp; a.g_C = d->g_C; a.g_y0 = d->g_y0; a.g_x0 = d->g_x0;
  a.NBLK = d->N / NB; a.CBLK = d->Cx / CB;
  // every pixel the window touches lies inside the x allocation: the taps of the last output pixel end at (Ho + 1 + y0, Wo + 1 + x0)
  GAN_CHECK(d->x_y0 >= 0 && d->x_x0 >= 0 && d->Ho + 2 + d->x_y0 <= d->x_Hp && d->Wo + 2 + d->x_x0 <= d->x_Wp,
            "wgrad_patch_fp8: the 3x3 window leaves the x view (halo too small)");
  GAN_CHECK(d->g_y0 >= 0 && d->g_x0 >= 0 && d->Ho + d->g_y0 <= d->g_Hp && d->Wo + d->g_x0 <= d->g_Wp, "wgrad_patch_fp8: g view too small");
  // the staging addresses are 32-bit byte offsets from the tensor bases
  GAN_CHECK((int64_t)d->B * d->x_Hp * d->x_Wp * d->Cx < (1ll << 32) && (int64_t)d->B * d->g_Hp * d->g_Wp * d->g_C < (1ll << 32),
            "wgrad_patch_fp8: an operand tensor exceeds the kernel's 32-bit byte offsets (4 GiB): split the batch");
  static std::atomic<uint64_t> attr_devs{0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return gan_set_error(-2, "wgrad_patch_fp8: hipGetDevice failed");
  const uint64_t dev_bit = 1ull << (dev & 63);
  if (!(attr_devs.load(std::memory_order_acquire) & dev_bit)) {
    if (hipFuncSetAttribute((const void*)wgrad_patch_fp8_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess ||
        hipFuncSetAttribute((const void*)wgrad_patch_fp8_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES_RING) != hipSuccess ||
        hipFuncSetAttribute((const void*)wgrad_patch_fp8_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess)
      return gan_set_error(-2, "wgrad_patch_fp8: cannot raise the dynamic LDS limit to %d bytes", LDS_BYTES);
    attr_devs.fetch_or(dev_bit, std::memory_order_release);
  }
  const bool ring = a.nrows * a.pitch > RX;
  GAN_CHECK(!(ipb > 1 && (ring || a.HoWo % KM != 0)), "wgrad_patch_fp8: several images per split need whole 128-pixel stages and the window variant");
  if (ipb > 1) hipLaunchKernelGGL((wgrad_patch_fp8_kernel<false, true>), dim3(a.NBLK * a.CBLK * d->nsplit), dim3(512), LDS_BYTES, s, a);
  else if (ring) hipLaunchKernelGGL(wgrad_patch_fp8_kernel<true>, dim3(a.NBLK * a.CBLK * d->nsplit), dim3(512), LDS_BYTES_RING, s, a);
  else hipLaunchKernelGGL(wgrad_patch_fp8_kernel<false>, dim3(a.NBLK * a.CBLK * d->nsplit), dim3(512), LDS_BYTES, s, a);
  if (hipGetLastError() != hipSuccess) return gan_set_error(-2, "wgrad_patch_fp8: launch failed");
  return 0;
}
