// Baseline JPEG encoder on the device, byte-identical to what the reference writes with PIL:
// pil.save(..., format="JPEG", quality=95, subsampling=0, optimize=True) (GAN_Variant1/generate_folder.py:252), i.e. libjpeg's
// 8-bit JDCT_ISLOW path, 4:4:4, one interleaved scan, optimal Huffman tables, no restart markers.  Integer arithmetic throughout.
//
//   gan_jpeg_blocks : colour conversion + forward DCT + quantisation (one thread per 8x8 block of one component), then the symbol
//                     histograms of the four tables of every image (LDS atomics per workgroup, integer global atomics across them)
//   gan_jpeg_tables : jpeg_gen_optimal_table, one wave per table; the two-smallest search is a wave butterfly
//   gan_jpeg_scan   : bits per block, exclusive scan per image, every block ORs its bits into the zeroed stream, 0xFF stuffing as
//                     count / scan / scatter, streams compacted over the batch
#include "common.h"

namespace {

constexpr int JPEG_BLOCK_BITS = 1728;        // bound on one block's code: DC 16 + 11, 63 x (16 + 10) = 1665, rounded to 27 * 64
constexpr int STUFF_CHUNK = 4096;            // raw bytes per workgroup of the stuffing passes: 256 threads x 16 bytes

struct JpegPlan {
  int nbx, nby, nblk;                        // blocks across, down; blocks per image in scan order (3 per MCU)
  int64_t raw_words, raw_bound, nchunks;     // per image: words of the unstuffed stream, its byte bound, stuffing chunks
  int64_t off_coef, off_bits, off_tot, off_raw, off_ff, ws_bytes, out_bytes;
};

int jpeg_plan(int B, int H, int W, JpegPlan* p) {
  GAN_CHECK(B >= 1 && B <= 65535 && H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "jpeg: B=%d H=%d W=%d outside 1 <= B, H, W <= 65535", B, H, W);   // B is grid.y
  p->nbx = (W + 7) / 8; p->nby = (H + 7) / 8;
  const int64_t nblk = 3ll * p->nbx * p->nby;
  GAN_CHECK(nblk * JPEG_BLOCK_BITS < (1ll << 32), "jpeg: %dx%d: bit offsets of one image are 32-bit (%lld blocks x %d bits); refused",
            H, W, (long long)nblk, JPEG_BLOCK_BITS);
  GAN_CHECK(B * nblk < (1ll << 28), "jpeg: B=%d x %lld blocks: batch too large", B, (long long)nblk);
  p->nblk = (int)nblk;
  p->raw_words = (nblk * JPEG_BLOCK_BITS + 31) / 32 + 1;
  p->raw_bound = nblk * (JPEG_BLOCK_BITS / 8);
  p->nchunks = (p->raw_bound + STUFF_CHUNK - 1) / STUFF_CHUNK;
  auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
  int64_t o = 0;
  p->off_coef = o; o += up(B * nblk * 64 * 2);
  p->off_bits = o; o += up(B * nblk * 4);
  p->off_tot = o;  o += up(B * 8);
  p->off_raw = o;  o += up(B * p->raw_words * 4);
  p->off_ff = o;   o += up(B * p->nchunks * 4);
  p->ws_bytes = o;
  p->out_bytes = 2 * B * p->raw_bound;
  return 0;
}

// zig-zag position -> natural index.  The callers index it from fully unrolled loops, so it folds to constants.
__device__ __forceinline__ constexpr int zig_nat(int k) {
  constexpr int t[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                         35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return t[k];
}
__device__ __forceinline__ constexpr int base_luma(int i) {
  constexpr int t[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
  return t[i];
}
__device__ __forceinline__ constexpr int base_chroma(int i) {
  constexpr int t[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
  return t[i];
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One pass of jfdctint.c over d[0], d[S], .. d[7 S].  FIRST: the row pass (outputs 0/4 << 2, others DESCALE 11); else the column pass
// (outputs 0/4 DESCALE 2, others DESCALE 15).
template <bool FIRST, int S> __device__ __forceinline__ void fdct_pass(int* d) {
  const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
  const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int N = FIRST ? 11 : 15;
  d[0] = FIRST ? (t10 + t11) << 2 : descale(t10 + t11, 2);
  d[4 * S] = FIRST ? (t10 - t11) << 2 : descale(t10 - t11, 2);
  int z1 = (t12 + t13) * 4433;
  d[2 * S] = descale(z1 + t13 * 6270, N);
  d[6 * S] = descale(z1 - t12 * 15137, N);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7 * S] = descale(u4 + z1 + z3, N);
  d[5 * S] = descale(u5 + z2 + z4, N);
  d[3 * S] = descale(u6 + z2 + z3, N);
  d[S] = descale(u7 + z1 + z4, N);
}

// Stages a-c.  Thread = one 8x8 block of one component, in scan order (block = 3 * mcu + component); grid.y = image.
// coef: int16 [B][nblk][64], quantised, zig-zag order; coefficient 0 is the DC value itself (the difference is taken by the readers).
__global__ __launch_bounds__(256) void jpeg_dct_kernel(const uint8_t* __restrict__ rgb, int H, int W, int nbx, int nblk, int qscale,
                                                       int16_t* __restrict__ coef) {
  const int gid = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (gid >= nblk) return;
  const int mcu = gid / 3, comp = gid - 3 * mcu, by = mcu / nbx, bx = mcu - by * nbx;
  // jccolor.c: 16-bit fixed point, one multiplier set per component
  const int kr = comp == 0 ? 19595 : comp == 1 ? -11059 : 32768;
  const int kg = comp == 0 ? 38470 : comp == 1 ? -21709 : -27439;
  const int kb = comp == 0 ? 7471 : comp == 1 ? 32768 : -5329;
  const int k0 = comp == 0 ? 32768 : (128 << 16) + 32767;
  const uint8_t* img = rgb + (int64_t)b * H * W * 3;
  int d[64];
  const bool whole = bx * 8 + 8 <= W && W % 4 == 0 && ((uintptr_t)rgb & 3) == 0;     // a row of the block is six aligned dwords
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int y = min(by * 8 + r, H - 1);                                             // edge replication
    const uint8_t* row = img + (int64_t)y * W * 3;
    if (whole) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(row + bx * 24);
      uint32_t w[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) w[i] = p[i];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int R = (w[(3 * c) >> 2] >> (8 * ((3 * c) & 3))) & 255, G = (w[(3 * c + 1) >> 2] >> (8 * ((3 * c + 1) & 3))) & 255;
        const int Bv = (w[(3 * c + 2) >> 2] >> (8 * ((3 * c + 2) & 3))) & 255;
        d[r * 8 + c] = ((kr * R + kg * G + kb * Bv + k0) >> 16) - 128;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint8_t* p = row + min(bx * 8 + c, W - 1) * 3;
        d[r * 8 + c] = ((kr * p[0] + kg * p[1] + kb * p[2] + k0) >> 16) - 128;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) fdct_pass<true, 1>(d + 8 * r);
#pragma unroll
  for (int c = 0; c < 8; ++c) fdct_pass<false, 8>(d + c);
  // quantise: divisor 8 q, round half away from zero; q = clamp((base * s + 50) / 100, 1, 255)
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const int base = comp == 0 ? base_luma(i) : base_chroma(i);
    const int q = min(max((base * qscale + 50) / 100, 1), 255), dv = 8 * q;
    const int a = d[i] < 0 ? -d[i] : d[i];
    const int r = (int)((unsigned)(a + (dv >> 1)) / (unsigned)dv);
    d[i] = d[i] < 0 ? -r : r;
  }
  u32x4_t* o = reinterpret_cast<u32x4_t*>(coef + ((int64_t)b * nblk + gid) * 64);
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    u32x4_t t;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      t[j] = ((uint32_t)d[zig_nat(8 * v + 2 * j)] & 0xffffu) | ((uint32_t)d[zig_nat(8 * v + 2 * j + 1)] << 16);
    o[v] = t;
  }
}

__device__ __forceinline__ int bit_length(int a) { return 32 - __clz(a); }      // a >= 0; 0 for a == 0

// jchuff.c encode_one_block over the block `gid` of image-relative coefficients `c` (int16 [nblk][64]): calls
// emit(table, symbol, extra bits, extra bit count) for every symbol; table 0 DC-Y, 1 AC-Y, 2 DC-C, 3 AC-C.
template <typename F> __device__ __forceinline__ void walk_block(const int16_t* __restrict__ c, int gid, F emit) {
  const u32x4_t* p = reinterpret_cast<const u32x4_t*>(c + (int64_t)gid * 64);
  uint32_t w[32];
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const u32x4_t t = p[v];
    w[4 * v] = t[0]; w[4 * v + 1] = t[1]; w[4 * v + 2] = t[2]; w[4 * v + 3] = t[3];
  }
  const int tb = (gid % 3) == 0 ? 0 : 2;
  const int prev = gid >= 3 ? (int)c[(int64_t)(gid - 3) * 64] : 0;               // the same component's block of the previous MCU
  {
    const int diff = (int)(int16_t)(w[0] & 0xffffu) - prev;
    const int a = diff < 0 ? -diff : diff, n = bit_length(a);
    emit(tb, n, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);
  }
  int run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    const int v = (k & 1) ? (int)w[k >> 1] >> 16 : (int)(int16_t)(w[k >> 1] & 0xffffu);
    if (v == 0) { ++run; continue; }
    while (run > 15) { emit(tb + 1, 0xF0, 0u, 0); run -= 16; }
    const int a = v < 0 ? -v : v, n = bit_length(a);
    emit(tb + 1, (run << 4) | n, (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u), n);
    run = 0;
  }
  if (run > 0) emit(tb + 1, 0, 0u, 0);
}

// Stage d: hist uint32 [B][4][256], zeroed by the caller.  A workgroup lies inside one image, counts in LDS, adds its non-zero bins.
__global__ __launch_bounds__(256) void jpeg_hist_kernel(const int16_t* __restrict__ coef, int nblk, uint32_t* __restrict__ hist) {
  __shared__ uint32_t sh[1024];
  const int gid = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  for (int i = threadIdx.x; i < 1024; i += 256) sh[i] = 0;
  __syncthreads();
  if (gid < nblk)
    walk_block(coef + (int64_t)b * nblk * 64, gid, [&](int tb, int sym, uint32_t, int) { atomicAdd(&sh[tb * 256 + sym], 1u); });
  __syncthreads();
  for (int i = threadIdx.x; i < 1024; i += 256)
    if (sh[i]) atomicAdd(&hist[(int64_t)b * 1024 + i], sh[i]);
}

// Stage e: jpeg_gen_optimal_table.  One wave per table; lane l holds entries l, l + 64, .. l + 256 (entry 256 is the pseudo-symbol).
// Instead of libjpeg's codesize / others chains every entry carries the head of its group: merging c2 into c1 lengthens the code of
// every member of both groups by one, which is what walking the two chains does.
// dht: uint8 [n][272] = bits[16] then huffval[256] (zero past the last symbol); codes: uint32 [n][256] = size << 16 | code, 0 = unused.
__global__ __launch_bounds__(64) void jpeg_tables_kernel(const uint32_t* __restrict__ hist, uint8_t* __restrict__ dht, uint32_t* __restrict__ codes) {
  __shared__ int cs_sh[257];
  __shared__ int bits[33], first_pos[17], first_code[17];
  const int t = blockIdx.x, lane = threadIdx.x;
  const unsigned long long NONE = ~0ull;
  uint32_t f[5];
  int grp[5], cs[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int i = lane + 64 * j;
    f[j] = i < 256 ? hist[(int64_t)t * 256 + i] : i == 256 ? 1u : 0u;
    grp[j] = i; cs[j] = 0;
  }
  for (int i = lane; i < 272; i += 64) dht[(int64_t)t * 272 + i] = 0;
  if (lane < 33) bits[lane] = 0;
  for (;;) {
    // the two smallest non-zero frequencies, the larger index first on ties (libjpeg scans upwards with <=)
    unsigned long long m1 = NONE, m2 = NONE;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      if (!f[j]) continue;
      const unsigned long long key = ((unsigned long long)f[j] << 32) | (0xffffffffu - (uint32_t)(lane + 64 * j));
      if (key < m1) { m2 = m1; m1 = key; }
      else if (key < m2) m2 = key;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                 // the two halves of every exchange hold disjoint entries
      const unsigned long long a1 = __shfl_xor(m1, o, 64), a2 = __shfl_xor(m2, o, 64);
      const unsigned long long lo = m1 < a1 ? m1 : a1, hi = m1 < a1 ? a1 : m1, s2 = m2 < a2 ? m2 : a2;
      m1 = lo; m2 = hi < s2 ? hi : s2;
    }
    if (m2 == NONE) break;
    const int c1 = (int)(0xffffffffu - (uint32_t)m1), c2 = (int)(0xffffffffu - (uint32_t)m2);
    const uint32_t fsum = (uint32_t)(m1 >> 32) + (uint32_t)(m2 >> 32);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int i = lane + 64 * j;
      if (i == c1) f[j] = fsum;
      if (i == c2) f[j] = 0;
      if (grp[j] == c1 || grp[j] == c2) { ++cs[j]; grp[j] = c1; }
    }
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int i = lane + 64 * j;
    if (i <= 256) cs_sh[i] = cs[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 5; ++j)
    if (lane + 64 * j <= 256 && cs[j] > 0) atomicAdd(&bits[min(cs[j], 32)], 1);   // libjpeg refuses lengths above 32; kept in range here
  __syncthreads();
  if (lane == 0) {
    for (int i = 32; i > 16; --i) {
      while (bits[i] > 0) {
        int j = i - 2;
        while (j > 0 && bits[j] == 0) --j;
        bits[i] -= 2; bits[i - 1] += 1; bits[j + 1] += 2; bits[j] -= 1;
      }
    }
    int i = 16;
    while (i > 0 && bits[i] == 0) --i;
    if (i > 0) bits[i] -= 1;                                                      // the pseudo-symbol leaves the longest length
    int p = 0, code = 0;
    for (int L = 1; L <= 16; ++L) {
      first_pos[L] = p; first_code[L] = code;
      p += bits[L]; code = (code + bits[L]) << 1;
    }
  }
  __syncthreads();
  if (lane < 16) dht[(int64_t)t * 272 + lane] = (uint8_t)bits[lane + 1];
  // symbols ordered by (length before limiting, value); the position in that order gives the limited length and the canonical code
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = lane + 64 * j, mine = cs[j];
    uint32_t out = 0;
    if (mine > 0) {
      int rank = 0;
      for (int k = 0; k < 256; ++k) {
        const int o = cs_sh[k];
        rank += (o > 0 && (o < mine || (o == mine && k < i))) ? 1 : 0;
      }
      int L = 16;
      for (int l = 1; l <= 16; ++l)
        if (rank >= first_pos[l] && rank < first_pos[l] + bits[l]) L = l;
      dht[(int64_t)t * 272 + 16 + rank] = (uint8_t)i;
      out = ((uint32_t)L << 16) | (uint32_t)(first_code[L] + rank - first_pos[L]);
    }
    codes[(int64_t)t * 256 + i] = out;
  }
}

// Stage f, 1: bits per block.  The image's four code tables sit in LDS.
__global__ __launch_bounds__(256) void jpeg_blockbits_kernel(const int16_t* __restrict__ coef, int nblk, const uint32_t* __restrict__ codes,
                                                             uint32_t* __restrict__ blkbits) {
  __shared__ uint32_t tab[1024];
  const int gid = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  for (int i = threadIdx.x; i < 1024; i += 256) tab[i] = codes[(int64_t)b * 1024 + i];
  __syncthreads();
  if (gid >= nblk) return;
  uint32_t n = 0;
  walk_block(coef + (int64_t)b * nblk * 64, gid, [&](int tb, int sym, uint32_t, int ne) { n += (tab[tb * 256 + sym] >> 16) + (uint32_t)ne; });
  blkbits[(int64_t)b * nblk + gid] = n;
}

// exclusive scan over a workgroup of NW waves; *total = the sum.  sh: NW entries.
template <int NW> __device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* sh, uint32_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  __syncthreads();
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const uint32_t s = sh[i];
    if (i < w) before += s;
    all += s;
  }
  *total = all;
  return before + inc - v;
}

// Stage f, 2: one workgroup per image turns blkbits into exclusive bit offsets, records (total bits, raw bytes), zeroes the words the
// stream will be ORed into and sets the 1-bits that pad the last byte.
__global__ __launch_bounds__(1024) void jpeg_scan_kernel(uint32_t* __restrict__ blkbits, int nblk, uint32_t* __restrict__ tot,
                                                         uint32_t* __restrict__ raw, int64_t raw_words) {
  __shared__ uint32_t sh[16];
  const int b = blockIdx.x;
  uint32_t* v = blkbits + (int64_t)b * nblk;
  uint32_t carry = 0;
  for (int base = 0; base < nblk; base += 1024) {
    const int i = base + threadIdx.x;
    const uint32_t x = i < nblk ? v[i] : 0u;
    uint32_t sum;
    const uint32_t e = block_scan_excl<16>(x, sh, &sum);
    if (i < nblk) v[i] = carry + e;
    carry += sum;
  }
  const uint32_t T = carry, nbytes = (T + 7) >> 3;
  uint32_t* r = raw + (int64_t)b * raw_words;
  const int64_t nz = min((int64_t)((T + 31) >> 5) + 1, raw_words);
  for (int64_t i = threadIdx.x; i < nz; i += 1024) r[i] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    tot[2 * b] = T; tot[2 * b + 1] = nbytes;
    const uint32_t pad = (8u - (T & 7u)) & 7u;
    if (pad) r[T >> 5] = ((1u << pad) - 1u) << (32u - (T & 31u) - pad);
  }
}

// Stage f, 3: every block writes its code at its bit offset.  Words hold the stream most significant bit first; neighbouring blocks
// share words, so everything is ORed into the zeroed buffer (integer OR: the result does not depend on the order).
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const int16_t* __restrict__ coef, int nblk, const uint32_t* __restrict__ codes,
                                                        const uint32_t* __restrict__ blkoff, uint32_t* __restrict__ raw, int64_t raw_words) {
  __shared__ uint32_t tab[1024];
  const int gid = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  for (int i = threadIdx.x; i < 1024; i += 256) tab[i] = codes[(int64_t)b * 1024 + i];
  __syncthreads();
  if (gid >= nblk) return;
  const uint32_t off = blkoff[(int64_t)b * nblk + gid];
  uint32_t* r = raw + (int64_t)b * raw_words;
  int64_t w = off >> 5;
  int n = (int)(off & 31u);                   // the bits of the first word that belong to earlier blocks count as zeros of ours
  unsigned long long acc = 0;
  walk_block(coef + (int64_t)b * nblk * 64, gid, [&](int tb, int sym, uint32_t extra, int ne) {
    const uint32_t e = tab[tb * 256 + sym];
    const int len = (int)(e >> 16) + ne;       // <= 16 + 11
    acc = (acc << len) | (unsigned long long)(((e & 0xffffu) << ne) | extra);
    n += len;
    if (n >= 32) {
      if (w < raw_words) atomicOr(&r[w], (uint32_t)(acc >> (n - 32)));
      ++w; n -= 32;
    }
  });
  if (n > 0 && w < raw_words) atomicOr(&r[w], (uint32_t)(acc << (32 - n)));
}

__device__ __forceinline__ uint32_t stream_byte(const uint32_t* r, int64_t i) { return (r[i >> 2] >> (24 - 8 * (int)(i & 3))) & 255u; }

__device__ __forceinline__ uint32_t count_ff16(const uint32_t* r, int64_t first, int64_t nbytes) {
  uint32_t n = 0;
  for (int k = 0; k < 4; ++k) {
    if (first + 4 * k >= nbytes) break;
    const uint32_t w = r[(first >> 2) + k];
#pragma unroll
    for (int j = 0; j < 4; ++j) n += (first + 4 * k + j < nbytes && ((w >> (24 - 8 * j)) & 255u) == 255u) ? 1u : 0u;
  }
  return n;
}

// Stuffing, 1: 0xFF bytes per chunk of STUFF_CHUNK raw bytes.  chunk_ff: uint32 [B][nchunks]; chunks past the stream are not written.
__global__ __launch_bounds__(256) void jpeg_ffcount_kernel(const uint32_t* __restrict__ raw, int64_t raw_words, const uint32_t* __restrict__ tot,
                                                           uint32_t* __restrict__ chunk_ff, int64_t nchunks) {
  __shared__ uint32_t sh[4];
  const int b = blockIdx.y;
  const int64_t nbytes = tot[2 * b + 1], first = (int64_t)blockIdx.x * STUFF_CHUNK + threadIdx.x * 16;
  if ((int64_t)blockIdx.x * STUFF_CHUNK >= nbytes) return;
  uint32_t sum;
  block_scan_excl<4>(count_ff16(raw + (int64_t)b * raw_words, first, nbytes), sh, &sum);
  if (threadIdx.x == 0) chunk_ff[(int64_t)b * nchunks + blockIdx.x] = sum;
}

// Stuffing, 2: one workgroup.  Per image the chunk counts become exclusive prefixes; offsets[b] = first output byte of image b,
// offsets[B] = total.  The images are walked one after the other: a few scan steps each at the batch sizes inference uses (16 images of
// 256 x 256: 17 us); a batch of thousands of images would want one workgroup per image and a scan over their totals.
__global__ __launch_bounds__(1024) void jpeg_offsets_kernel(uint32_t* __restrict__ chunk_ff, int64_t nchunks, const uint32_t* __restrict__ tot, int B,
                                                            int64_t* __restrict__ offsets) {
  __shared__ uint32_t sh[16];
  int64_t run = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t nbytes = tot[2 * b + 1], nc = (nbytes + STUFF_CHUNK - 1) / STUFF_CHUNK;
    uint32_t* v = chunk_ff + (int64_t)b * nchunks;
    uint32_t carry = 0;
    for (int64_t base = 0; base < nc; base += 1024) {
      const int64_t i = base + threadIdx.x;
      const uint32_t x = i < nc ? v[i] : 0u;
      uint32_t sum;
      const uint32_t e = block_scan_excl<16>(x, sh, &sum);
      if (i < nc) v[i] = carry + e;
      carry += sum;
    }
    if (threadIdx.x == 0) offsets[b] = run;
    run += nbytes + carry;
  }
  if (threadIdx.x == 0) offsets[B] = run;
}

// Stuffing, 3: scatter with a 0x00 after every 0xFF (the padded last byte included).
__global__ __launch_bounds__(256) void jpeg_stuff_kernel(const uint32_t* __restrict__ raw, int64_t raw_words, const uint32_t* __restrict__ tot,
                                                         const uint32_t* __restrict__ chunk_ff, int64_t nchunks, const int64_t* __restrict__ offsets,
                                                         uint8_t* __restrict__ out, int64_t out_bytes) {
  __shared__ uint32_t sh[4];
  const int b = blockIdx.y;
  const int64_t nbytes = tot[2 * b + 1], first = (int64_t)blockIdx.x * STUFF_CHUNK + threadIdx.x * 16;
  if ((int64_t)blockIdx.x * STUFF_CHUNK >= nbytes) return;
  const uint32_t* r = raw + (int64_t)b * raw_words;
  uint32_t sum;
  const uint32_t e = block_scan_excl<4>(count_ff16(r, first, nbytes), sh, &sum);
  int64_t p = offsets[b] + first + chunk_ff[(int64_t)b * nchunks + blockIdx.x] + e;
  for (int k = 0; k < 16; ++k) {
    if (first + k >= nbytes) break;
    const uint32_t v = stream_byte(r, first + k);
    if (p < out_bytes) out[p] = (uint8_t)v;
    ++p;
    if (v == 255u) {
      if (p < out_bytes) out[p] = 0;
      ++p;
    }
  }
}

}  // namespace

extern "C" int gan_jpeg_bounds(int B, int H, int W, int64_t* ws_bytes, int64_t* out_bytes) {
  JpegPlan p;
  if (jpeg_plan(B, H, W, &p)) return -1;
  GAN_CHECK(ws_bytes && out_bytes, "jpeg_bounds: null pointer");
  *ws_bytes = p.ws_bytes; *out_bytes = p.out_bytes;
  return 0;
}

extern "C" int gan_jpeg_blocks(const uint8_t* rgb, int B, int H, int W, int quality, void* ws, int64_t ws_bytes, uint32_t* hist, void* stream) {
  JpegPlan p;
  if (jpeg_plan(B, H, W, &p)) return -1;
  GAN_CHECK(quality >= 1 && quality <= 100, "jpeg_blocks: quality %d outside 1 .. 100", quality);
  GAN_CHECK(rgb && ws && hist, "jpeg_blocks: null pointer");
  GAN_CHECK(ws_bytes >= p.ws_bytes && (uintptr_t)ws % 16 == 0, "jpeg_blocks: workspace of %lld bytes, gan_jpeg_bounds asks %lld (16-byte aligned)",
            (long long)ws_bytes, (long long)p.ws_bytes);
  hipStream_t s = (hipStream_t)stream;
  int16_t* coef = reinterpret_cast<int16_t*>((char*)ws + p.off_coef);
  const int qscale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  if (hipMemsetAsync(hist, 0, (size_t)B * 1024 * sizeof(uint32_t), s) != hipSuccess) return gan_set_error(-2, "jpeg_blocks: hipMemsetAsync failed");
  const dim3 grid((p.nblk + 255) / 256, B);
  hipLaunchKernelGGL(jpeg_dct_kernel, grid, dim3(256), 0, s, rgb, H, W, p.nbx, p.nblk, qscale, coef);
  hipLaunchKernelGGL(jpeg_hist_kernel, grid, dim3(256), 0, s, coef, p.nblk, hist);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_jpeg_tables(const uint32_t* hist, int n, uint8_t* dht, uint32_t* codes, void* stream) {
  GAN_CHECK(hist && dht && codes, "jpeg_tables: null pointer");
  GAN_CHECK(n >= 1 && n <= (1 << 20), "jpeg_tables: n=%d tables outside 1 .. 2^20", n);
  hipLaunchKernelGGL(jpeg_tables_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, hist, dht, codes);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_jpeg_scan(void* ws, int64_t ws_bytes, int B, int H, int W, const uint32_t* codes, uint8_t* out, int64_t out_bytes,
                             int64_t* offsets, void* stream) {
  JpegPlan p;
  if (jpeg_plan(B, H, W, &p)) return -1;
  GAN_CHECK(ws && codes && out && offsets, "jpeg_scan: null pointer");
  GAN_CHECK(ws_bytes >= p.ws_bytes && (uintptr_t)ws % 16 == 0, "jpeg_scan: workspace of %lld bytes, gan_jpeg_bounds asks %lld (16-byte aligned)",
            (long long)ws_bytes, (long long)p.ws_bytes);
  GAN_CHECK(out_bytes >= p.out_bytes, "jpeg_scan: output of %lld bytes, gan_jpeg_bounds asks %lld", (long long)out_bytes, (long long)p.out_bytes);
  GAN_CHECK(p.nchunks <= 0x7fffffff, "jpeg_scan: too many stuffing chunks");
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  int16_t* coef = reinterpret_cast<int16_t*>(base + p.off_coef);
  uint32_t* blkbits = reinterpret_cast<uint32_t*>(base + p.off_bits);
  uint32_t* tot = reinterpret_cast<uint32_t*>(base + p.off_tot);
  uint32_t* raw = reinterpret_cast<uint32_t*>(base + p.off_raw);
  uint32_t* chunk_ff = reinterpret_cast<uint32_t*>(base + p.off_ff);
  const dim3 grid((p.nblk + 255) / 256, B), cgrid((unsigned)p.nchunks, B);
  hipLaunchKernelGGL(jpeg_blockbits_kernel, grid, dim3(256), 0, s, coef, p.nblk, codes, blkbits);
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(B), dim3(1024), 0, s, blkbits, p.nblk, tot, raw, p.raw_words);
  hipLaunchKernelGGL(jpeg_pack_kernel, grid, dim3(256), 0, s, coef, p.nblk, codes, blkbits, raw, p.raw_words);
  hipLaunchKernelGGL(jpeg_ffcount_kernel, cgrid, dim3(256), 0, s, raw, p.raw_words, tot, chunk_ff, p.nchunks);
  hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(1024), 0, s, chunk_ff, p.nchunks, tot, B, offsets);
  hipLaunchKernelGGL(jpeg_stuff_kernel, cgrid, dim3(256), 0, s, raw, p.raw_words, tot, chunk_ff, p.nchunks, offsets, out, out_bytes);
  GAN_LAUNCH_CHECK();
  return 0;
}
