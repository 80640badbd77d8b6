// "Range-patch" weight gradient for stride-1 3x3 windows on maps whose width divides 128 (the 18 residual 3x3 256->256
// convolutions: 54 of the 76 weight-gradient launches of a CUT step).
//
//   part[s][n][t][c] = sum over the pixels m of split s of  g[m][n] * x[pix(m) + tapoff[t]][c]
//
// Same lesson as conv_patch.hip: the generic kernel (conv_wgrad.hip) pays one block-wide barrier per 64-pixel K-step and
// re-stages x once per tap.  Here a block owns an output tile of 128 n x 64 c x ALL 9 taps and walks its pixel range in
// stages of whole image rows; both operands are staged by LDS-DMA and every tap reads its x fragments from the staged image
// rows at a shifted position.  Both operands are reduction-major in memory, so fragments come from ds_read_b64_tr_b16.
//  * The MFMA k index is permuted (k = 16h + 4*lanegroup + q, identically for both operands) so that the eight rows a
//    half-wave reads are CONSECUTIVE pixels; the 32-byte piece index is XOR-ed by row bits (g: row&7, x: (column>>1)&3), which
//    makes the transposed reads bank-conflict free at ANY pixel shift.
//  * x is stored as image rows whose pitch is padded to a multiple of 8 pixels: the vertical part of a tap offset then never
//    changes the swizzle bits and is a wave-uniform offset; only the three horizontal shifts need their own (precomputed)
//    swizzled address -> ~1 vector ALU op per transposed read.
//  * 8 waves = 2 (n) x 4 (c); a wave owns 4 n-tiles x 1 c-tile x 9 taps = 36 accumulator tiles (144 registers).
//
// THE STAGE RING (wgrad_patch_kernel<LGWO>, Wo = 16 ... 128).  A stage is KS pixels = R = KS/Wo whole image rows.  Its g tile (KS pixels
// x 128 n) goes into one of DEPTH + 1 tile buffers and its R NEW x rows into a ring of row slots (tap row v of the split -> slot v mod
// SLOTS): the two rows a stage shares with its predecessor are already there -- at Wo = 64 a 128-pixel stage fetches two rows where a
// self-contained window fetched four.  The first stage of an image also fetches that image's two leading rows, and a split over several
// images (many small maps) runs the ring across the image boundaries, which is what the ring's spare slots are for.
//  * hipcc waits vmcnt(0) for every LDS-DMA it knows of at a __syncthreads() AND in front of the first transposed read after the next
//    stage's DMAs were issued: the stage just requested was waited for before the stage at hand was computed, one exposed memory
//    latency per stage.  So the DMAs are inline assembly that hipcc does not count, and the kernel counts them: every wave issues exactly
//    DMA_PER_STAGE instructions per stage (chunk indices past the end are clamped and rewrite the last chunk with the same bytes; the
//    leading rows' extra instructions only make a counted wait retire more than it must), a stage is retired by
//    `s_waitcnt vmcnt(DMA_PER_STAGE * stages still in flight) lgkmcnt(0)` + a raw s_barrier, and read only behind that barrier.  The same
//    barrier orders the reads of stage st - 1 before the DMAs of stage st + DEPTH, which overwrite its tile and its dead rows.
//  * Stage size and depth are measured, not derived (profiles/wgrad_ring.txt; B = 16 / 32, 64x64, 256 -> 256, us per launch, the kernel
//    before the ring 80.1 / 142.5): KS = 64 with DEPTH = 2 or 3 (counted vmcnt(4) / vmcnt(8), no drain anywhere) 77.3 / 135.0 and 76.8 /
//    135.7; KS = 128 with DEPTH = 1 (the wait at the barrier is a vmcnt(0), of DMAs issued a whole stage earlier) 73.7 / 128.1.  What
//    paid is the wait that no longer stands between a stage's DMAs and the reads of the stage before; a second barrier per 144 MFMAs
//    costs more than deeper prefetch returns, and KS = 128 with DEPTH = 2 does not fit 160 KiB at Wo = 64.
//  * The sums and their order (stages in pixel order, k-steps of 32 pixels in order, one k permutation) do not depend on KS or DEPTH:
//    `part` is bit-identical for every setting, and to the kernel before the ring (tests/test_wgrad_patch_ring_gpu.py).
#include <stdlib.h>
#include <atomic>
#include "common.h"

namespace {

constexpr int KM = 128;            // pixel granularity of a split (gan_wgrad_patch_splits)
constexpr int NB = 128, CB = 64;   // output tile: g channels x x channels (x all taps)
constexpr int NT = 9;
constexpr int KS = 128;            // pixels per stage: divides KM, so no split changes
constexpr int DEPTH = 1;           // stages in flight while one computes
constexpr int NGT = DEPTH + 1;     // g tile buffers
constexpr int GS_BYTES = KS * 256;
template <int LGWO> struct Ring {
  static constexpr int WO = 1 << LGWO, R = KS / WO;              // R: image rows per stage
  static constexpr bool MULTI = WO < KM;                          // splits may run over several images (gan_wgrad_patch_splits: never on 128-wide maps)
  static constexpr int PITCH = (WO + 2 + 7) / 8 * 8, ROWB = PITCH * 128, CPR = PITCH / 8;   // CPR: chunks per row
  // rows alive while stage st computes and st + DEPTH lands: R + 2 read, DEPTH * R on their way, and 2 leading rows for every image boundary
  // between them (an image is at least KM / KS stages)
  static constexpr int SLOTS = (R + 2) + DEPTH * R + (MULTI ? 2 * ((DEPTH * KS + KM - 1) / KM) : 0);
  // a chunk is 1 KB = one wave instruction; per wave and stage: G_DMA of the g tile's chunks + X_DMA of the new rows' (LEAD_DMA more for an image's first)
  static constexpr int X_CHUNKS = R * CPR, LEAD_CHUNKS = 2 * CPR, G_DMA = KS / 32, X_DMA = (X_CHUNKS + 7) / 8, LEAD_DMA = (LEAD_CHUNKS + 7) / 8;
  static constexpr int DMA_PER_STAGE = G_DMA + X_DMA;
  static constexpr int LDS = NGT * GS_BYTES + SLOTS * ROWB;
  static_assert(KS % WO == 0 && KM % KS == 0, "a stage is whole image rows and a split is whole stages");
  static_assert(DMA_PER_STAGE * (DEPTH - 1) < 64, "vmcnt is a 6-bit counter");
  static_assert(R + 2 <= SLOTS && LDS <= 160 * 1024, "the ring does not fit the CU's 160 KiB of LDS");
};

struct WpArgs {
  const char* x; const char* g; float* part;
  int HoWo, spi, per;                // spi: splits per image, per: pixels per split (multiple of KM)
  int ipb;                           // images per split (> 1: small maps, spi = 1 -- a block accumulates over ipb whole images)
  int Cx, N;
  int x_Hp, x_Wp, x_y0, x_x0;        // x_y0/x_x0: position of tap (0,0) of output pixel (0,0) inside the padded image
  int g_Hp, g_Wp, g_C, g_y0, g_x0;
  int NBLK, CBLK;
};

// 16-byte-per-lane LDS-DMA as an instruction hipcc does not count: lds_dst is the wave-uniform LDS byte address (M0), goff each
// lane's byte offset from the wave-uniform base.  M0 is the compiler's, so it is saved and restored inside the statement.
__device__ __forceinline__ void dma16(const char* gbase, uint32_t goff, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(goff), "s"(gbase), "s"(__builtin_amdgcn_readfirstlane(lds_dst)) : "memory");
}
// retire all but the newest `K` stages' DMAs of this wave and the wave's LDS reads, then meet the block: after it the retired stage may be
// read and the buffers read before it may be overwritten
template <int K, int DMA_PER_STAGE> __device__ __forceinline__ void retire_and_barrier(int in_flight) {
  if constexpr (K == 0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else if (in_flight >= K) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" :: "n"(K * DMA_PER_STAGE) : "memory");
  else retire_and_barrier<K - 1, DMA_PER_STAGE>(in_flight);
}

template <int LGWO>
__global__ __launch_bounds__(512) void wgrad_patch_kernel(WpArgs a) {
  using G = Ring<LGWO>;
  extern __shared__ __attribute__((aligned(1024))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // XCD-aware: the NBLK*CBLK blocks of one pixel split share its dY tile / x rows; workgroups b and b+8 share an XCD, so
  // hand consecutive ids to one XCD (the split's operands are then fetched into one L2 once)
  int bid = (gridDim.x & 7) == 0 ? (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  const int cb = bid % a.CBLK; bid /= a.CBLK;
  const int nb = bid % a.NBLK; bid /= a.NBLK;
  const int sp = bid;                                  // split index: image b0 = sp / spi, sub-range sp % spi -- or ipb whole images from sp * ipb
  const int b0 = a.ipb > 1 ? sp * a.ipb : sp / a.spi, sub = a.ipb > 1 ? 0 : sp - b0 * a.spi;
  const int m_begin = sub * a.per, m_end = min(a.HoWo, m_begin + a.per);
  const int nst_img = (m_end - m_begin + KM - 1) / KM * (KM / KS);   // stages per image: the KM-pixel ranges of the split, cut in KS
  const int nstage = nst_img * a.ipb;                                // the ring runs across the images of the split
  const int n0 = nb * NB, c0 = cb * CB, ho0 = m_begin >> LGWO;

  // ---- staging roles (LDS-DMA, lane-linear images, XOR applied on the SOURCE chunk)
  // g tile: KS rows x 256 B; row gr + 32*i (i < KS/32); position gp holds source chunk gp ^ ((row & 7) << 1)
  const int gr = tid >> 4, gp = tid & 15;
  const uint32_t gsrc = (uint32_t)((n0 + ((gp ^ ((gr & 7) << 1)) << 3)) * 2);
  // x row: PITCH pixels x 128 B in chunks of 8 pixels; position xp of pixel column col holds the source chunk with piece (xp>>1) ^ ((col>>1)&3)
  const int xr = lane >> 3, xp = lane & 7;
  const uint32_t xsrc = (uint32_t)((c0 + ((((xp >> 1) ^ ((xr >> 1) & 3)) << 1 | (xp & 1)) << 3)) * 2);
  const uint32_t x_pixb = (uint32_t)a.Cx * 2u, g_pixb = (uint32_t)a.g_C * 2u;

  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
  constexpr uint32_t XRING = NGT * GS_BYTES;           // [SLOTS][PITCH][128 B] behind the g tiles
  auto wrap = [](int s) { return s >= G::SLOTS ? s - G::SLOTS : s; };

  // image row `lr` (counted from the split's first tap row) of image b, chunk cc -> slot
  auto x_chunk = [&](int b, int lr, int cc, int slot) {
    int iy = ho0 + lr + a.x_y0, ix = cc * 8 + xr + a.x_x0;       // pitch padding and rows past the image read a valid (unused) pixel
    iy = iy < a.x_Hp ? iy : a.x_Hp - 1;
    ix = ix < a.x_Wp ? ix : a.x_Wp - 1;
    dma16(a.x, (uint32_t)((b * a.x_Hp + iy) * a.x_Wp + ix) * x_pixb + xsrc, lds0 + XRING + (uint32_t)(slot * G::ROWB + cc * 1024));
  };
  // loader state: the next stage to issue (image l_img, stage l_ls of it), its g tile buffer and the slot of its first tap row
  int l_img = 0, l_ls = 0, l_buf = 0, l_slot = 0;
  auto issue = [&]() {
    const int b = b0 + l_img, m0 = m_begin + l_ls * KS;
#pragma unroll
    for (int i = 0; i < G::G_DMA; ++i) {
      int m = m0 + gr + 32 * i;
      m = m < a.HoWo ? m : a.HoWo - 1;   // rows past the split end are zeroed after landing
      const int ho = m >> LGWO, wo = m & (G::WO - 1);
      dma16(a.g, (uint32_t)((b * a.g_Hp + ho + a.g_y0) * a.g_Wp + wo + a.g_x0) * g_pixb + gsrc,
            lds0 + (uint32_t)(l_buf * GS_BYTES + wave * 1024 + i * 8192));
    }
#pragma unroll
    for (int i = 0; i < G::X_DMA; ++i) { // the stage's R new rows: tap rows l_ls * R + 2 ...
      const int c = min(wave + 8 * i, G::X_CHUNKS - 1), r = c / G::CPR;
      x_chunk(b, l_ls * G::R + 2 + r, c - r * G::CPR, wrap(l_slot + 2 + r));
    }
    if (l_ls == 0) {                     // first stage of an image: its two leading rows as well
#pragma unroll
      for (int i = 0; i < G::LEAD_DMA; ++i) {
        const int c = min(wave + 8 * i, G::LEAD_CHUNKS - 1), r = c / G::CPR;
        x_chunk(b, r, c - r * G::CPR, wrap(l_slot + r));
      }
    }
    l_buf = l_buf + 1 == NGT ? 0 : l_buf + 1;
    l_slot += G::R;
    if (++l_ls == nst_img) { l_ls = 0; ++l_img; l_slot += 2; }
    l_slot = wrap(l_slot);
  };

  const int wn = wave >> 2, wc = wave & 3;
  const int fr = lane & 15, fg = lane >> 4, q = fr >> 2, p4 = fr & 3;
  // transposed-read geometry: instruction h of k-step ks reads, for lane group fg, pixels ks*32 + 16h + 4fg + q
  uint32_t gcol[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) gcol[i] = (uint32_t)(((wn * 4 + i) * 16 + p4 * 4) * 2);
  const uint32_t xcol = (uint32_t)((wc * 16 + p4 * 4) * 2);
  // Per-lane base addresses (k-step 0, h = 0).  Every other (k-step, h) adds a wave-uniform byte offset: 16h + 32ks is a
  // multiple of 8 pixels (swizzle bits unchanged) and, for Wo >= 16, never carries into the lane's 4fg+q part.
  const int kl = 4 * fg + q;
  uint32_t gbase[4], xbase[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) gbase[i] = (uint32_t)(kl * 256) + (gcol[i] ^ (uint32_t)((kl & 7) << 5));
#pragma unroll
  for (int dx = 0; dx < 3; ++dx) {
    const int r = kl + dx;
    xbase[dx] = XRING + (uint32_t)(r * 128) + (xcol ^ (uint32_t)((r & 6) << 4));
  }

  f32x4_t acc[4][NT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[i][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  for (int s = 0; s < DEPTH && s < nstage; ++s) issue();
  int r_ls = 0, r_buf = 0, r_slot = 0;                      // reader state: stage st is stage r_ls of its image
  for (int st = 0; st < nstage; ++st) {
    retire_and_barrier<DEPTH - 1, G::DMA_PER_STAGE>(nstage - 1 - st);         // stage st landed in every wave; everyone is done reading stage st - 1
    char* gt = lds + r_buf * GS_BYTES;
    const int m0 = m_begin + r_ls * KS;
    uint32_t so[G::R + 2];                                  // byte offset of the slot of tap row j of the stage
#pragma unroll
    for (int j = 0; j < G::R + 2; ++j) so[j] = (uint32_t)(wrap(r_slot + j) * G::ROWB);
    if (m0 + KS > m_end) {   // tail: pixels past the split end must not contribute -> zero their g rows
      for (int c = tid; c < KS * 16; c += 512)
        if (m0 + (c >> 4) >= m_end) *reinterpret_cast<u32x4_t*>(gt + c * 16) = u32x4_t{0, 0, 0, 0};
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    if (st + DEPTH < nstage) issue();                       // into the tile and the rows stage st - 1 was read from
#pragma unroll
    for (int ks = 0; ks < KS / 32; ++ks) {
      // keep the seven base addresses opaque so that the derived addresses are recomputed (1 add each), not hoisted and spilled
      asm volatile("" : "+v"(gbase[0]), "+v"(gbase[1]), "+v"(gbase[2]), "+v"(gbase[3]), "+v"(xbase[0]), "+v"(xbase[1]), "+v"(xbase[2]));
      s16x4_t gf[4][2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t goff = (uint32_t)((ks * 32 + 16 * h) * 256);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          gf[i][h] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(gt + gbase[i] + goff));
      }
      bf16x8_t av[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        av[i] = bf16x8_t{gf[i][0][0], gf[i][0][1], gf[i][0][2], gf[i][0][3], gf[i][1][0], gf[i][1][1], gf[i][1][2], gf[i][1][3]};
      // 9 taps: a 3-deep ring of x fragments, read two taps ahead of their MFMAs; tap t = (dy, dx) = (t / 3, t % 3)
      s16x4_t xf[3][2];
      auto x_read = [&](int t) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int ku = ks * 32 + 16 * h;                  // wave-uniform part of the pixel index: stage row ku >> LGWO, column ku & (Wo - 1)
          xf[t % 3][h] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4_t*)(lds + (xbase[t % 3] + so[(ku >> LGWO) + t / 3]) + (ku & (G::WO - 1)) * 128));
        }
      };
      x_read(0);
      x_read(1);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (t + 2 < NT) x_read(t + 2);
        const bf16x8_t bv = {xf[t % 3][0][0], xf[t % 3][0][1], xf[t % 3][0][2], xf[t % 3][0][3],
                             xf[t % 3][1][0], xf[t % 3][1][1], xf[t % 3][1][2], xf[t % 3][1][3]};
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bv, acc[i][t], 0, 0, 0);
      }
    }
    r_buf = r_buf + 1 == NGT ? 0 : r_buf + 1;
    r_slot += G::R;
    if (++r_ls == nst_img) { r_ls = 0; r_slot += 2; }
    r_slot = wrap(r_slot);
  }

  // D[row = n (fg*4+e)][col = c (fr)]
  float* part = a.part + (int64_t)sp * a.N * NT * a.Cx;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = n0 + (wn * 4 + i) * 16 + fg * 4 + e;
        part[((int64_t)n * NT + t) * a.Cx + c0 + wc * 16 + fr] = acc[i][t][e];
      }
}

template <int LGWO> int launch_ring(const WpArgs& a, int nsplit, hipStream_t s) {
  static std::atomic<uint64_t> attr_devs{0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return gan_set_error(-2, "wgrad_patch: hipGetDevice failed");
  const uint64_t dev_bit = 1ull << (dev & 63);
  if (!(attr_devs.load(std::memory_order_acquire) & dev_bit)) {
    if (hipFuncSetAttribute((const void*)wgrad_patch_kernel<LGWO>, hipFuncAttributeMaxDynamicSharedMemorySize, Ring<LGWO>::LDS) != hipSuccess)
      return gan_set_error(-2, "wgrad_patch: cannot raise the dynamic LDS limit to %d bytes", Ring<LGWO>::LDS);
    attr_devs.fetch_or(dev_bit, std::memory_order_release);
  }
  hipLaunchKernelGGL(wgrad_patch_kernel<LGWO>, dim3(a.NBLK * a.CBLK * nsplit), dim3(512), Ring<LGWO>::LDS, s, a);
  return 0;
}

}  // namespace

// the e4m3 kernel of the same decomposition (wgrad_patch_fp8.hip): dtype GAN_FP8 descriptors are its
int gan_wgrad_patch_fp8_splits(const gan_wgrad_desc* d);
int gan_wgrad_patch_fp8_launch(const gan_wgrad_desc* d, hipStream_t s);

// splits per image the range-patch weight-gradient kernel wants for this problem (0 = descriptor does not qualify).
// The planner sizes `part` for B * spi slabs and sets nsplit = B * spi, variant = 1.
extern "C" int gan_wgrad_patch_splits(const gan_wgrad_desc* d) {
  if (!d) return 0;
  if (d->dtype == GAN_FP8) return gan_wgrad_patch_fp8_splits(d);
  if (d->dtype != GAN_BF16 || d->ntaps != NT || d->Cx % CB != 0 || d->N % NB != 0 || d->N != d->g_C) return 0;
  if (d->x_sy != 1 || d->x_sx != 1 || d->g_sy != 1 || d->g_sx != 1) return 0;
  // 3x3 window in row-major tap order over a map whose width is a power of two dividing the stage
  if (d->Wo < 16 || (d->Wo & (d->Wo - 1)) != 0 || KM % d->Wo != 0 || d->max_tapoff != (2 * d->x_Wp + 2) * d->Cx) return 0;
  const int HoWo = d->Ho * d->Wo;
  if (HoWo < KM) return 0;
  const int blocks_per_split = (d->N / NB) * (d->Cx / CB);
  // Many small images (Basic_GAN: 16x16 maps at batch 256): with one split per image a block runs two stages between a full prologue and
  // a 300 KB partial store, and the reduction reads B slabs (0.77x of the generic kernel, measured).  A split then covers SEVERAL whole
  // images -- the negative return value: -(images per split), the largest divisor of B that still leaves one block per CU.
  // (not on 128-wide maps, whose row ring has no slots for an image boundary)
  if (HoWo < 8 * KM && d->B * blocks_per_split > 256 && HoWo % KM == 0 && d->Wo < KM) {
    int ipb = d->B * blocks_per_split / 256;
    while (ipb > 1 && d->B % ipb != 0) --ipb;
    if (ipb > 1) return -ipb;
  }
  if (HoWo < 8 * KM && d->B > 64) return 0;
  int spi = (256 + d->B * blocks_per_split - 1) / (d->B * blocks_per_split);   // ~one block per CU
  const int max_spi = HoWo / (2 * KM) > 0 ? HoWo / (2 * KM) : 1;
  if (spi > max_spi) spi = max_spi;
  if (spi < 1) spi = 1;
  return spi;
}

int gan_wgrad_patch_launch(const gan_wgrad_desc* d, hipStream_t s) {
  if (d->dtype == GAN_FP8) return gan_wgrad_patch_fp8_launch(d, s);
  const int spi_want = gan_wgrad_patch_splits(d);
  GAN_CHECK(spi_want != 0 && d->nsplit > 0 && (d->nsplit % d->B == 0 || (d->B % d->nsplit == 0 && (d->Ho * d->Wo) % KM == 0)),
            "wgrad: variant=1 but the descriptor does not qualify for the range-patch kernel");
  WpArgs a;
  a.x = (const char*)d->x; a.g = (const char*)d->g; a.part = d->part;
  a.HoWo = d->Ho * d->Wo;
  a.ipb = d->nsplit < d->B ? d->B / d->nsplit : 1;      // fewer splits than images: whole images per split
  a.spi = a.ipb > 1 ? 1 : d->nsplit / d->B;
  int per = (a.HoWo + a.spi - 1) / a.spi;
  per = (per + KM - 1) / KM * KM;
  a.per = per;
  GAN_CHECK((a.spi - 1) * per < a.HoWo, "wgrad_patch: nsplit=%d leaves empty splits", d->nsplit);
  a.Cx = d->Cx; a.N = d->N;
  a.x_Hp = d->x_Hp; a.x_Wp = d->x_Wp; a.x_y0 = d->x_y0; a.x_x0 = d->x_x0;
  a.g_Hp = d->g_Hp; a.g_Wp = d->g_Wp; a.g_C = d->g_C; a.g_y0 = d->g_y0; a.g_x0 = d->g_x0;
  a.NBLK = d->N / NB; a.CBLK = d->Cx / CB;
  // the planner's split count must be the one gan_wgrad_patch_splits answered (the kernel indexes partial slabs and images by it), and on
  // 128-wide maps a split stays inside ONE image
  GAN_CHECK(spi_want > 0 ? d->nsplit == d->B * spi_want : d->nsplit * -spi_want == d->B, "wgrad_patch: nsplit=%d is not what gan_wgrad_patch_splits implies (%d)",
            d->nsplit, spi_want);
  GAN_CHECK(!(d->Wo == KM && a.ipb > 1), "wgrad_patch: 128-pixel-wide maps take one image per split");
  // the staging addresses are 32-bit byte offsets from the tensor bases
  GAN_CHECK((int64_t)d->B * d->x_Hp * d->x_Wp * d->Cx * 2 < (1ll << 32) && (int64_t)d->B * d->g_Hp * d->g_Wp * d->g_C * 2 < (1ll << 32),
            "wgrad_patch: an operand tensor exceeds the kernel's 32-bit byte offsets (4 GiB): split the batch");
  const int lgWo = __builtin_ctz(d->Wo);
  const int rc = lgWo == 4 ? launch_ring<4>(a, d->nsplit, s) : lgWo == 5 ? launch_ring<5>(a, d->nsplit, s)
               : lgWo == 6 ? launch_ring<6>(a, d->nsplit, s) : launch_ring<7>(a, d->nsplit, s);
  if (rc != 0) return rc;
  if (hipGetLastError() != hipSuccess) return gan_set_error(-2, "wgrad_patch: launch failed");
  return 0;
}
