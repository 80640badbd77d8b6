// The arithmetic of the device JPEG decoder as plain functions: the table builder, the per-segment entropy decode, the 8x8 inverse DCT
// and the upsampling + colour conversion of one pixel.  jpegdec.hip wraps them in kernels; jpegdec_host.cpp includes the same text and
// runs it on the CPU under AddressSanitizer over the golden and the corrupted files, before a GPU sees them.
// Every loop is bounded by a count known before the data is read, every load is clamped to [begin, end), every store index comes from
// counters (the caller has validated the descriptors), and an irregularity returns GAN_JPEGDEC_ERR_* bits.
#pragma once
#include <stdint.h>
#include "../../include/mi355x_gan.h"

#if defined(__HIPCC__)
#define JD_FN __device__ __forceinline__
#define JD_HD __host__ __device__ __forceinline__     // geometry only: the launchers size their grids with it
#define JD_CONST static __device__ const
#else
#define JD_FN static inline
#define JD_HD static inline
#define JD_CONST static const
#endif

constexpr int JD_LOOK = 9;                       // lookahead width, libjpeg's HUFF_LOOKAHEAD + 1

struct JdTable {                                 // 1424 bytes
  uint16_t look[1 << JD_LOOK];                   // next 9 bits -> length << 8 | symbol; 0: the code is longer (or there is none)
  int32_t maxcode[18];                           // [l], l = 1 .. 16: the largest code of length l, -1 when there is none
  int32_t valoff[17];                            // [l]: index of the first symbol of length l, minus its code
  uint8_t val[256];
  uint8_t pad[4];
};
static_assert(sizeof(JdTable) == 1424 && sizeof(JdTable) % 16 == 0, "JdTable layout");
static_assert(sizeof(gan_jpegdec_image) == 104 && sizeof(gan_jpegdec_segment) == 20, "descriptor layout");

JD_CONST uint8_t jd_zigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- tables.  raw: 16 counts, then up to 256 symbols (the caller's buffer holds 272 bytes whatever the counts say).
JD_FN void jd_table_head(const uint8_t* raw, JdTable* t) {
  int code = 0, p = 0;
  t->maxcode[0] = -1; t->valoff[0] = 0; t->maxcode[17] = 0xFFFFF;
  for (int l = 1; l <= 16; ++l) {
    const int n = raw[l - 1];
    t->valoff[l] = p - code;
    t->maxcode[l] = n ? code + n - 1 : -1;
    p += n; code = (code + n) << 1;
  }
}
// entry i of the lookahead table (and, for i < 256, symbol i); needs jd_table_head's arrays
JD_FN void jd_table_entry(const uint8_t* raw, JdTable* t, int i) {
  if (i < 256) t->val[i] = raw[16 + i];
  uint16_t e = 0;
  for (int l = JD_LOOK; l >= 1; --l) {           // downwards: the shortest matching length is written last and wins
    const int c = i >> (JD_LOOK - l);
    if (c <= t->maxcode[l]) e = (uint16_t)((l << 8) | raw[16 + ((t->valoff[l] + c) & 255)]);
  }
  t->look[i] = e;
}

// ---- bit reader over data[pos .. end): most significant bit first, the 0x00 after a 0xFF skipped; `buf` holds the next `n` bits at its top.
// Memory is read as aligned 8-byte chunks, chunk k + 1 requested when chunk k is taken into use, so a refill does not wait for a load
// it has just issued.  The chunks lie between the segment's first and last byte rounded out to multiples of 8 -- inside the block,
// whose start and length are multiples of 16 -- and the bytes outside [pos, end) that they bring are never looked at.
struct JdBits {
  const uint8_t* data;
  int64_t pos, end, idx, last;                   // idx: the chunk `cur` holds; last: the segment's last chunk
  uint64_t buf, cur, nxt;
  int n, err;
};
JD_FN uint64_t jd_load8(const uint8_t* data, int64_t idx) {
#if defined(__HIPCC__)
  return *reinterpret_cast<const uint64_t*>(data + idx * 8);
#else
  uint64_t v;
  __builtin_memcpy(&v, data + idx * 8, 8);
  return v;
#endif
}
JD_FN void jd_open(JdBits* b, const uint8_t* data, int64_t begin, int64_t end) {
  b->data = data; b->pos = begin; b->end = end; b->buf = 0; b->n = 0; b->err = 0;
  b->idx = begin >> 3; b->last = b->idx; b->cur = b->nxt = 0;
  if (begin < end) {
    b->last = (end - 1) >> 3;
    b->cur = jd_load8(data, b->idx);
    b->nxt = jd_load8(data, b->idx < b->last ? b->idx + 1 : b->last);
  }
}
JD_FN uint32_t jd_byte(JdBits* b, int64_t pos) {          // pos in [begin, end), never below an earlier call's
  const int64_t i = pos >> 3;
  if (i != b->idx) {                                     // bytes are taken one after the other: this is chunk idx + 1
    b->cur = b->nxt; b->idx = i;
    b->nxt = jd_load8(b->data, i < b->last ? i + 1 : b->last);
  }
  return (uint32_t)(b->cur >> (8 * (int)(pos & 7))) & 255u;
}
JD_FN void jd_fill(JdBits* b) {
  while (b->n <= 56 && b->pos < b->end) {        // at most 8 rounds
    const uint32_t v = jd_byte(b, b->pos++);
    if (v == 0xFFu) {
      if (b->pos < b->end && jd_byte(b, b->pos) == 0) ++b->pos;
      else b->err |= GAN_JPEGDEC_ERR_MARKER;
    }
    b->buf |= (uint64_t)v << (56 - b->n);
    b->n += 8;
  }
}
JD_FN uint32_t jd_peek(const JdBits* b, int k) { return (uint32_t)(b->buf >> (64 - k)); }      // 1 <= k <= 32; zeros past the end
JD_FN void jd_skip(JdBits* b, int k) {
  if (k > b->n) { b->err |= GAN_JPEGDEC_ERR_END; k = b->n; }
  b->buf = k >= 64 ? 0 : b->buf << k;
  b->n -= k;
}
// one Huffman symbol; the caller keeps at least 32 bits in the buffer while the segment has them (a symbol and its extra bits take at most 31)
JD_FN int jd_symbol(JdBits* b, const JdTable* t) {
  const uint32_t e = t->look[jd_peek(b, JD_LOOK)];
  int l = (int)(e >> 8), sym = (int)(e & 255u);
  if (e == 0) {
    uint32_t code = 0;
    for (l = JD_LOOK + 1; l <= 16; ++l) {
      code = jd_peek(b, l);
      if ((int)code <= t->maxcode[l]) break;
    }
    if (l > 16) { b->err |= GAN_JPEGDEC_ERR_CODE; return 0; }
    sym = t->val[(t->valoff[l] + (int)code) & 255];
  }
  jd_skip(b, l);
  return sym;
}
JD_FN int jd_extend(JdBits* b, int s) {          // s bits -> the signed value of category s, 0 <= s <= 15
  if (s == 0) return 0;
  const int v = (int)jd_peek(b, s);
  jd_skip(b, s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// Component c of an image: blocks across, blocks per MCU across / down, first block.
struct JdComp { int bw, h, v, first; };
JD_HD JdComp jd_comp(const gan_jpegdec_image* im, int c) {
  JdComp r;
  r.h = c == 0 ? im->hmax : 1; r.v = c == 0 ? im->vmax : 1;
  r.bw = im->mcux * r.h;
  const int n0 = im->mcux * im->mcuy * im->hmax * im->vmax, n1 = im->mcux * im->mcuy;
  r.first = c == 0 ? 0 : c == 1 ? n0 : n0 + n1;
  return r;
}
JD_HD int jd_blocks(const gan_jpegdec_image* im) {
  return im->mcux * im->mcuy * (im->hmax * im->vmax + (im->ncomp == 3 ? 2 : 0));
}
JD_HD int64_t jd_plane_bytes(const gan_jpegdec_image* im) { return (int64_t)jd_blocks(im) * 64; }

// ---- one restart segment `j` (counted inside its image) into the image's zeroed coefficients.  tabs: the image's four tables.
// zz: jd_zigzag, or a copy of it in faster memory.
JD_FN int jd_decode_segment(const gan_jpegdec_image* im, const gan_jpegdec_segment* sg, int j, const uint8_t* data, const JdTable* tabs,
                            const uint8_t* zz, int16_t* coef) {
  JdBits b;
  jd_open(&b, data, sg->byte_begin, sg->byte_end);
  if (j > 0 && (data[sg->byte_begin - 2] != 0xFF || data[sg->byte_begin - 1] != 0xD0 + ((j - 1) & 7))) return GAN_JPEGDEC_ERR_RST;
  int pred[3] = {0, 0, 0};
  for (int m = 0; m < sg->mcu_count; ++m) {
    const int mcu = sg->mcu_first + m, my = mcu / im->mcux, mx = mcu - my * im->mcux;
    for (int c = 0; c < im->ncomp; ++c) {
      const JdComp cp = jd_comp(im, c);
      const JdTable* dc = tabs + im->dc_tab[c];
      const JdTable* ac = tabs + im->ac_tab[c];
      for (int u = 0; u < cp.h * cp.v; ++u) {
        const int v = u / cp.h, h = u - v * cp.h;
        int16_t* blk = coef + (int64_t)(cp.first + (my * cp.v + v) * cp.bw + mx * cp.h + h) * 64;
        if (b.n < 32) jd_fill(&b);
        const int s = jd_symbol(&b, dc);
        if (s > 15) b.err |= GAN_JPEGDEC_ERR_CODE;
        if (b.err) return b.err;
        pred[c] += jd_extend(&b, s);
        if (pred[c] < -32768 || pred[c] > 32767) b.err |= GAN_JPEGDEC_ERR_DC;
        if (b.err) return b.err;
        blk[0] = (int16_t)pred[c];
        for (int k = 1; k < 64; ++k) {
          if (b.n < 32) jd_fill(&b);
          const int rs = jd_symbol(&b, ac), r = rs >> 4, n = rs & 15;
          if (b.err) return b.err;
          if (n == 0) {
            if (r != 15) break;                  // end of block
            k += 15;                             // ZRL; past 63 it only ends the block, as in libjpeg
            continue;
          }
          k += r;
          if (k > 63) return b.err | GAN_JPEGDEC_ERR_RUN;
          const int val = jd_extend(&b, n);
          if (b.err) return b.err;
          blk[zz[k]] = (int16_t)val;
        }
      }
    }
  }
  jd_fill(&b);
  if (b.pos < b.end || b.n >= 8) b.err |= GAN_JPEGDEC_ERR_LEFT;
  return b.err;
}

// ---- jidctint.c jpeg_idct_islow on one block: coef natural order, q natural order; out: 8 rows of 8 bytes, `stride` apart.
JD_FN int jd_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// one 1-D pass over d[0], d[S] .. d[7 S]; SHIFT = 11 for the columns, 18 for the rows
template <int S, int SHIFT> JD_FN void jd_idct_pass(int* d) {
  int z2 = d[2 * S], z3 = d[6 * S];
  int z1 = (z2 + z3) * 4433;
  int tmp2 = z1 + z3 * -15137, tmp3 = z1 + z2 * 6270;
  z2 = d[0]; z3 = d[4 * S];
  int tmp0 = (int)((unsigned)(z2 + z3) << 13), tmp1 = (int)((unsigned)(z2 - z3) << 13);
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = d[7 * S]; tmp1 = d[5 * S]; tmp2 = d[3 * S]; tmp3 = d[S];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * 9633;
  tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  d[0] = jd_descale(tmp10 + tmp3, SHIFT); d[7 * S] = jd_descale(tmp10 - tmp3, SHIFT);
  d[S] = jd_descale(tmp11 + tmp2, SHIFT); d[6 * S] = jd_descale(tmp11 - tmp2, SHIFT);
  d[2 * S] = jd_descale(tmp12 + tmp1, SHIFT); d[5 * S] = jd_descale(tmp12 - tmp1, SHIFT);
  d[3 * S] = jd_descale(tmp13 + tmp0, SHIFT); d[4 * S] = jd_descale(tmp13 - tmp0, SHIFT);
}
// d: the 64 coefficients, replaced by the samples 0 .. 255.  Returns GAN_JPEGDEC_ERR_RANGE where libjpeg's C and SIMD code part.
JD_FN int jd_idct(int* d, const uint16_t* q) {
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    d[i] *= (int)q[i];                           // |coefficient| < 2^15, q < 2^8 (the parser refuses 16-bit tables)
    bad |= d[i] < -32768 || d[i] > 32767;
  }
  if (bad) {                                     // keep the products small enough for the int32 passes; the file goes to the host decoder
#pragma unroll
    for (int i = 0; i < 64; ++i) d[i] = 0;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) jd_idct_pass<8, 11>(d + c);
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    if (d[i] < -32768 || d[i] > 32767) { bad = true; d[i] = 0; }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) jd_idct_pass<1, 18>(d + 8 * r);
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    bad |= d[i] < -512 || d[i] > 511;
    const int v = d[i] + 128;
    d[i] = v < 0 ? 0 : v > 255 ? 255 : v;
  }
  return bad ? GAN_JPEGDEC_ERR_RANGE : 0;
}

// ---- pixel (y, x) of an image from its component planes (plane c: jd_comp(im, c).bw * 8 bytes wide, first byte at planes + 64 first)
JD_FN int jd_chroma(const gan_jpegdec_image* im, const uint8_t* pl, int stride, int y, int x) {
  if (im->hmax == 1) return pl[(int64_t)y * stride + x];
  const int cw = (im->W + 1) >> 1, cx = x >> 1;
  if (im->vmax == 1) {
    const uint8_t* row = pl + (int64_t)y * stride;
    const int cur = row[cx];
    if (cw <= 2) return cur;                     // libjpeg takes the plain replicating upsampler for such widths
    if (x & 1) return cx == cw - 1 ? cur : (3 * cur + row[cx + 1] + 2) >> 2;
    return cx == 0 ? cur : (3 * cur + row[cx - 1] + 1) >> 2;
  }
  const int ch = (im->H + 1) >> 1, cy = y >> 1;
  if (cw <= 2) return pl[(int64_t)cy * stride + cx];
  int ny = (y & 1) ? cy + 1 : cy - 1;
  ny = ny < 0 ? 0 : ny > ch - 1 ? ch - 1 : ny;   // above the first row is the first row, below the last real row is that row
  const uint8_t* r0 = pl + (int64_t)cy * stride;
  const uint8_t* r1 = pl + (int64_t)ny * stride;
  const int cur = 3 * r0[cx] + r1[cx];
  if (x & 1) return cx == cw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * r0[cx + 1] + r1[cx + 1] + 7) >> 4;
  return cx == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * r0[cx - 1] + r1[cx - 1] + 8) >> 4;
}
JD_FN int jd_clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
JD_FN void jd_pixel(const gan_jpegdec_image* im, const uint8_t* planes, int y, int x, uint8_t* rgb) {
  const JdComp c0 = jd_comp(im, 0);
  const int Y = planes[(int64_t)y * (c0.bw * 8) + x];
  if (im->ncomp == 1) { rgb[0] = rgb[1] = rgb[2] = (uint8_t)Y; return; }
  const JdComp c1 = jd_comp(im, 1), c2 = jd_comp(im, 2);
  const int cb = jd_chroma(im, planes + (int64_t)c1.first * 64, c1.bw * 8, y, x) - 128;
  const int cr = jd_chroma(im, planes + (int64_t)c2.first * 64, c2.bw * 8, y, x) - 128;
  rgb[0] = (uint8_t)jd_clamp8(Y + ((91881 * cr + 32768) >> 16));
  rgb[1] = (uint8_t)jd_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  rgb[2] = (uint8_t)jd_clamp8(Y + ((116130 * cb + 32768) >> 16));
}

// ---- the bodies of the back-end kernels of jpegdec.hip, which both decoders launch (both upload blocks begin with
// gan_jpegdec_image [n] and both workspaces lay out coefficients and planes alike).  Device only; the includer has common.h.
#if defined(__HIPCC__)
constexpr int JD_DHT_BYTES = 272;

// workgroup b of 64 lanes: raw table b -> decode table b.  t: one JdTable in LDS.
__device__ __forceinline__ void jd_tables_body(const uint8_t* __restrict__ dht, JdTable* __restrict__ tabs, JdTable* t) {
  const uint8_t* raw = dht + (int64_t)blockIdx.x * JD_DHT_BYTES;
  if (threadIdx.x == 0) jd_table_head(raw, t);
  __syncthreads();
  for (int i = threadIdx.x; i < (1 << JD_LOOK); i += 64) jd_table_entry(raw, t, i);
  __syncthreads();
  const uint32_t* s = reinterpret_cast<const uint32_t*>(t);
  uint32_t* d = reinterpret_cast<uint32_t*>(tabs + blockIdx.x);
  for (int i = threadIdx.x; i < (int)(sizeof(JdTable) / 4); i += 64) d[i] = s[i];
}

// one thread per 8x8 block of image blockIdx.y (workgroups of 256)
__device__ __forceinline__ void jd_idct_body(const uint8_t* __restrict__ blk, int64_t off_qt, char* __restrict__ ws, int32_t* __restrict__ errw) {
  const int b = blockIdx.y, g = blockIdx.x * 256 + threadIdx.x;
  const gan_jpegdec_image& im = reinterpret_cast<const gan_jpegdec_image*>(blk)[b];      // uniform over the workgroup: scalar loads
  if (g >= jd_blocks(&im)) return;
  const JdComp c1 = jd_comp(&im, 1), c2 = jd_comp(&im, 2);
  const int c = im.ncomp == 1 || g < c1.first ? 0 : g < c2.first ? 1 : 2;
  const JdComp cp = jd_comp(&im, c);
  const int r = g - cp.first, by = r / cp.bw, bx = r - by * cp.bw;
  const uint16_t* q = reinterpret_cast<const uint16_t*>(blk + off_qt) + ((int64_t)b * 4 + im.q_tab[c]) * 64;
  const u32x4_t* p = reinterpret_cast<const u32x4_t*>(ws + im.coef_off + (int64_t)g * 128);
  int d[64];
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const u32x4_t w = p[v];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      d[8 * v + 2 * j] = (int)(int16_t)(w[j] & 0xffffu);
      d[8 * v + 2 * j + 1] = (int)w[j] >> 16;
    }
  }
  const int e = jd_idct(d, q);
  if (e) atomicOr(&errw[b], e);
  const int stride = cp.bw * 8;
  char* o = ws + im.plane_off + (int64_t)cp.first * 64 + (int64_t)by * 8 * stride + bx * 8;
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    u32x2_t w;
    w[0] = (uint32_t)d[8 * y] | (uint32_t)d[8 * y + 1] << 8 | (uint32_t)d[8 * y + 2] << 16 | (uint32_t)d[8 * y + 3] << 24;
    w[1] = (uint32_t)d[8 * y + 4] | (uint32_t)d[8 * y + 5] << 8 | (uint32_t)d[8 * y + 6] << 16 | (uint32_t)d[8 * y + 7] << 24;
    *reinterpret_cast<u32x2_t*>(o + (int64_t)y * stride) = w;
  }
}

// one thread per pixel of image blockIdx.y (workgroups of 256)
__device__ __forceinline__ void jd_pixels_body(const uint8_t* __restrict__ blk, const char* __restrict__ ws, uint8_t* __restrict__ out,
                                               const int32_t* __restrict__ errw, int32_t* __restrict__ err) {
  const int b = blockIdx.y;
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  const gan_jpegdec_image& im = reinterpret_cast<const gan_jpegdec_image*>(blk)[b];
  if (g == 0 && err) err[b] = errw[b];
  if (g >= (uint32_t)im.H * (uint32_t)im.W) return;
  const int y = (int)(g / (uint32_t)im.W), x = (int)(g - (uint32_t)y * (uint32_t)im.W);
  uint8_t rgb[3];
  jd_pixel(&im, reinterpret_cast<const uint8_t*>(ws + im.plane_off), y, x, rgb);
  uint8_t* o = out + im.out_off + (int64_t)g * 3;
  o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
}
#else
// ---- the host programs' walk behind the coefficients of one image: dequantise + jd_idct into the planes, then jd_pixel per pixel.
// qt: the image's four quantisation tables; ws, out: the whole workspace and output.  Returns the GAN_JPEGDEC_ERR_* bits.
static inline int jd_host_back(const gan_jpegdec_image* im, const uint16_t* qt, uint8_t* ws, uint8_t* out) {
  const int16_t* coef = (const int16_t*)(ws + im->coef_off);
  uint8_t* planes = ws + im->plane_off;
  int err = 0;
  for (int c = 0; c < im->ncomp; ++c) {
    const JdComp cp = jd_comp(im, c);
    const int nb = c == 0 ? im->mcux * im->mcuy * im->hmax * im->vmax : im->mcux * im->mcuy;
    for (int r = 0; r < nb; ++r) {
      int d[64];
      for (int i = 0; i < 64; ++i) d[i] = coef[(int64_t)(cp.first + r) * 64 + i];
      err |= jd_idct(d, qt + im->q_tab[c] * 64);
      const int by = r / cp.bw, bx = r - by * cp.bw, stride = cp.bw * 8;
      for (int y = 0; y < 8; ++y)
        for (int x = 0; x < 8; ++x) planes[(int64_t)cp.first * 64 + (int64_t)(by * 8 + y) * stride + bx * 8 + x] = (uint8_t)d[8 * y + x];
    }
  }
  for (int y = 0; y < im->H; ++y)
    for (int x = 0; x < im->W; ++x) jd_pixel(im, planes, y, x, out + im->out_off + ((int64_t)y * im->W + x) * 3);
  return err;
}
#endif
