// The arithmetic of the device PNG decoder as plain functions: the bit reader, the code-table builder, the inflate of one zlib stream
// and the unfiltering + conversion of one image.  pngdec.hip wraps them in kernels; pngdec_host.cpp includes the same text and runs it
// on the CPU under AddressSanitizer over the golden and the corrupted files, before a GPU sees them.
// The functions are written for the `nl` lanes of ONE wave that run them together on shared state (`lane` = 0 .. nl - 1, nl <= PD_MAX_LANES
// = the wave size; PD_SYNC between a phase that writes the shared state and one that reads it); every value that steers control flow is
// the same in all lanes.  The barriers are placed for lanes that issue their loads and stores in one instruction stream; a workgroup of
// several waves has not been reasoned through and is refused by a static_assert beside the launches.  The host runs them with one lane.
// Every loop is bounded by the stream's bit count or by a byte count of the validated descriptor, every load lies in
// [begin, end) of the stream rounded out to 8-byte chunks (inside its 16-byte padding), every store index comes from counters checked
// against the descriptor's extent, and an irregularity returns GAN_PNGDEC_ERR_* bits.
#pragma once
#include <stdint.h>
#include "../../include/mi355x_gan.h"

#if defined(__HIPCC__)
#define PD_FN __device__ __forceinline__
#define PD_SYNC() __syncthreads()
#define PD_CONST static __device__ const
#else
#define PD_FN static inline
#define PD_CONST static const
#define PD_SYNC() ((void)0)
#endif

constexpr int PD_LOOK = 9;                       // lookahead width of the code tables
constexpr int PD_WINDOW = 32768;                 // the ring that holds the last 32 KiB of output
constexpr int PD_FLUSH = 16384;                  // bytes of the ring that go to memory at a time
constexpr int PD_MAX_LANES = 64;                 // one wave: see above
static_assert(sizeof(gan_pngdec_image) == 64, "descriptor layout");

// ---- bit reader over data[begin .. end): least significant bit first; `buf` holds the next `n` bits at its bottom, zeros above.
// Memory is read as aligned 8-byte chunks, chunk k + 1 requested when chunk k is taken into use.
struct PdBits {
  const uint8_t* data;
  int64_t end, idx, last, left;                  // idx: the chunk `cur` holds; last: the stream's last chunk; left: bits not yet in buf
  uint64_t buf, cur, nxt;
  int n, used, err;                              // used: bits of `cur` already moved into buf
};
PD_FN uint64_t pd_load8(const uint8_t* data, int64_t idx) {
#if defined(__HIPCC__)
  return *reinterpret_cast<const uint64_t*>(data + idx * 8);
#else
  uint64_t v;
  __builtin_memcpy(&v, data + idx * 8, 8);
  return v;
#endif
}
PD_FN void pd_open(PdBits* b, const uint8_t* data, int64_t begin, int64_t end) {      // keeps b->err
  b->data = data; b->end = end; b->buf = 0; b->n = 0; b->left = begin < end ? (end - begin) * 8 : 0;
  b->idx = begin >> 3; b->last = b->idx; b->used = (int)(begin & 7) * 8; b->cur = b->nxt = 0;
  if (begin < end) {
    b->last = (end - 1) >> 3;
    b->cur = pd_load8(data, b->idx);
    b->nxt = pd_load8(data, b->idx < b->last ? b->idx + 1 : b->last);
  }
}
PD_FN void pd_fill(PdBits* b) {                  // afterwards n = 64, or every bit of the stream is in buf
  for (int r = 0; r < 2; ++r) {
    int take = 64 - b->n;
    if (take > 64 - b->used) take = 64 - b->used;
    if ((int64_t)take > b->left) take = (int)b->left;
    if (take <= 0) break;
    uint64_t v = b->cur >> b->used;
    if (take < 64) v &= ((uint64_t)1 << take) - 1;
    b->buf |= v << b->n;
    b->n += take; b->used += take; b->left -= take;
    if (b->used == 64) {
      b->cur = b->nxt; ++b->idx; b->used = 0;
      b->nxt = pd_load8(b->data, b->idx < b->last ? b->idx + 1 : b->last);
    }
  }
}
PD_FN uint32_t pd_peek(const PdBits* b, int k) { return (uint32_t)b->buf & ((1u << k) - 1u); }      // 0 <= k <= 16; zeros past the end
PD_FN void pd_skip(PdBits* b, int k) {
  if (k > b->n) { b->err |= GAN_PNGDEC_ERR_END; k = b->n; }
  b->buf = k >= 64 ? 0 : b->buf >> k;
  b->n -= k;
}
PD_FN uint32_t pd_take(PdBits* b, int k) {
  const uint32_t v = pd_peek(b, k);
  pd_skip(b, k);
  return v;
}
PD_FN int64_t pd_bytepos(const PdBits* b) { return b->end - (b->left + b->n) / 8; }      // of the next whole byte not yet touched

PD_FN uint32_t pd_rev16(uint32_t v) {
  v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
  v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
  v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
  return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu);
}

// ---- one canonical code (RFC 1951 3.2.2) over symbols 0 .. nsym - 1, nsym <= 288
struct PdTable {
  uint16_t look[1 << PD_LOOK];                   // next 9 bits of the stream -> length << 9 | symbol; 0: the code is longer (or there is none)
  int32_t count[16];                             // [l]: codes of length l
  int32_t maxcode[16];                           // [l], l = 1 .. 15: the largest code of length l, -1 when there is none
  int32_t valoff[16];                            // [l]: index in `sym` of the first symbol of length l, minus its code
  int32_t first[16];                             // [l]: that index itself
  uint16_t sym[288];                             // the symbols in code order
};
PD_FN int pd_sym_at(const PdTable* t, int i) { return t->sym[i < 0 ? 0 : i > 287 ? 287 : i]; }
// lens[0 .. nsym): code lengths 0 .. 15.  codes: the code-length code, which may not be incomplete in any way.
PD_FN int pd_build(PdTable* t, const uint8_t* lens, int nsym, bool codes, int lane, int nl) {
  for (int l = lane; l <= 15; l += nl) {
    int c = 0;
    for (int s = 0; s < nsym; ++s) c += lens[s] == l;
    t->count[l] = c;
  }
  PD_SYNC();
  int left = 1, code = 0, p = 0, maxlen = 0;
  for (int l = 1; l <= 15; ++l) {
    const int n = t->count[l];
    left = (left << 1) - n;
    if (left < 0) return GAN_PNGDEC_ERR_OVER;
    if (lane == 0) { t->valoff[l] = p - code; t->maxcode[l] = n ? code + n - 1 : -1; t->first[l] = p; }
    p += n; code = (code + n) << 1;
    if (n) maxlen = l;
  }
  if (left > 0 && (codes ? true : maxlen > 1)) return GAN_PNGDEC_ERR_INCOMPLETE;      // no code at all (a block of literals has no distance code) and one code of length 1 pass
  PD_SYNC();
  for (int l = 1 + lane; l <= 15; l += nl) {
    int k = t->first[l];
    for (int s = 0; s < nsym; ++s)
      if (lens[s] == l && k < 288) t->sym[k++] = (uint16_t)s;
  }
  PD_SYNC();
  for (int i = lane; i < (1 << PD_LOOK); i += nl) {
    const int c = (int)(pd_rev16((uint32_t)i) >> (16 - PD_LOOK));      // the 9 bits, first bit of the stream on top
    uint16_t e = 0;
    for (int l = 1; l <= PD_LOOK; ++l) {                              // upwards: a prefix that is no code of a shorter length is not below the first code of this one
      const int cd = c >> (PD_LOOK - l);
      if (cd <= t->maxcode[l]) { e = (uint16_t)((l << PD_LOOK) | pd_sym_at(t, t->valoff[l] + cd)); break; }
    }
    t->look[i] = e;
  }
  PD_SYNC();
  return 0;
}
// one symbol; the caller keeps at least 15 bits in the buffer while the stream has them
PD_FN int pd_symbol(PdBits* b, const PdTable* t) {
  const uint32_t e = t->look[pd_peek(b, PD_LOOK)];
  if (e) { pd_skip(b, (int)(e >> PD_LOOK)); return (int)(e & ((1u << PD_LOOK) - 1u)); }
  const int r = (int)(pd_rev16(pd_peek(b, 15)) >> 1);
  int l, cd = 0;
  for (l = PD_LOOK + 1; l <= 15; ++l) {
    cd = r >> (15 - l);
    if (cd <= t->maxcode[l]) break;
  }
  if (l > 15) { b->err |= GAN_PNGDEC_ERR_SYMBOL; return 0; }
  pd_skip(b, l);
  return pd_sym_at(t, t->valoff[l] + cd);
}

PD_CONST uint8_t pd_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};      // of the code-length code's lengths

// ---- inflate.  The shared state of one stream: the window ring, the three code tables (code-length code, literal/length, distance)
// and the code lengths being read.
struct PdInflate {
  alignas(16) uint8_t win[PD_WINDOW];
  PdTable tab[3];
  uint8_t lens[320];
  uint8_t clens[32];
};
// the ring's bytes [from, from + bytes) of the output, from and bytes multiples of 16, to raw
PD_FN void pd_flush(const PdInflate* S, uint8_t* raw, int64_t from, int bytes, int lane, int nl) {
  for (int i = lane * 16; i < bytes; i += nl * 16) {
    const uint8_t* s = S->win + ((from + i) & (PD_WINDOW - 1));
#if defined(__HIPCC__)
    typedef __attribute__((ext_vector_type(4))) uint32_t pd_u32x4;
    *reinterpret_cast<pd_u32x4*>(raw + from + i) = *reinterpret_cast<const pd_u32x4*>(s);
#else
    __builtin_memcpy(raw + from + i, s, 16);
#endif
  }
}
// The zlib stream of `im` in the block `blk` -> its raw_bytes = H (1 + rowbytes) bytes at `raw` (an area of raw_bytes rounded up to a
// multiple of 16 at least).  Returns the error bits, the same in every lane.
PD_FN int pd_inflate(const gan_pngdec_image* im, const uint8_t* blk, PdInflate* S, uint8_t* raw, int lane, int nl) {
  const int64_t raw_bytes = (int64_t)im->H * (1 + im->rowbytes);
  const int64_t begin = (int64_t)im->stream_off + 2, end = (int64_t)im->stream_off + im->stream_len - 4;
  const int64_t dmax = (int64_t)1 << im->wbits;
  int64_t produced = 0, flushed = 0;
  bool fixed_built = false;
  PdBits b;
  b.err = 0;
  pd_open(&b, blk, begin, end);
  for (;;) {                                     // one block per round; a block takes at least 3 bits
    pd_fill(&b);
    const int final_block = (int)pd_take(&b, 1), type = (int)pd_take(&b, 2);
    if (b.err) return b.err;
    if (type == 3) return GAN_PNGDEC_ERR_BTYPE;
    if (type == 0) {
      pd_skip(&b, (int)((b.left + b.n) & 7));      // to the next byte of the stream
      pd_fill(&b);
      const uint32_t len = pd_take(&b, 16), nlen = pd_take(&b, 16);
      if (b.err) return b.err;
      if (len != (~nlen & 0xffffu)) return GAN_PNGDEC_ERR_STORED;
      int64_t pos = pd_bytepos(&b);
      if (pos + len > end) return GAN_PNGDEC_ERR_END;
      if (produced + len > raw_bytes) return GAN_PNGDEC_ERR_MORE;
      for (uint32_t done = 0; done < len;) {     // in pieces the ring can take before it is written out
        const int piece = (int)(len - done < (uint32_t)PD_FLUSH ? len - done : (uint32_t)PD_FLUSH);
        PD_SYNC();
        for (int k = lane; k < piece; k += nl) S->win[(produced + k) & (PD_WINDOW - 1)] = blk[pos + k];
        PD_SYNC();
        produced += piece; pos += piece; done += (uint32_t)piece;
        if (produced - flushed >= PD_FLUSH) { pd_flush(S, raw, flushed, PD_FLUSH, lane, nl); flushed += PD_FLUSH; }
      }
      pd_open(&b, blk, pos, end);
    } else {
      if (type == 1) {
        if (!fixed_built) {
          PD_SYNC();
          for (int s = lane; s < 320; s += nl) S->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
          PD_SYNC();
          pd_build(&S->tab[1], S->lens, 288, false, lane, nl);
          pd_build(&S->tab[2], S->lens + 288, 32, false, lane, nl);
          fixed_built = true;
        }
      } else {
        fixed_built = false;
        const int hlit = (int)pd_take(&b, 5) + 257, hdist = (int)pd_take(&b, 5) + 1, hclen = (int)pd_take(&b, 4) + 4;
        if (b.err) return b.err;
        if (hlit > 286 || hdist > 30) return GAN_PNGDEC_ERR_COUNTS;
        PD_SYNC();
        for (int k = lane; k < 19; k += nl) S->clens[k] = 0;
        PD_SYNC();
        for (int k = 0; k < hclen; ++k) {
          if (b.n < 3) pd_fill(&b);
          const uint32_t v = pd_take(&b, 3);
          if (lane == 0) S->clens[pd_order[k]] = (uint8_t)v;
        }
        if (b.err) return b.err;
        PD_SYNC();
        int e = pd_build(&S->tab[0], S->clens, 19, true, lane, nl);
        if (e) return e;
        const int total = hlit + hdist;
        int have = 0, prev = 0;
        while (have < total) {                   // a round takes at least one bit
          if (b.n < 32) pd_fill(&b);
          const int s = pd_symbol(&b, &S->tab[0]);
          if (b.err) return b.err;
          int rep = 1, v = s;
          if (s == 16) {
            if (have == 0) return GAN_PNGDEC_ERR_REPEAT;
            v = prev; rep = 3 + (int)pd_take(&b, 2);
          } else if (s == 17) {
            v = 0; rep = 3 + (int)pd_take(&b, 3);
          } else if (s == 18) {
            v = 0; rep = 11 + (int)pd_take(&b, 7);
          }
          if (b.err) return b.err;
          if (have + rep > total) return GAN_PNGDEC_ERR_REPEAT;
          for (int k = lane; k < rep; k += nl) S->lens[have + k] = (uint8_t)v;
          have += rep; prev = v;
        }
        PD_SYNC();
        if (S->lens[256] == 0) return GAN_PNGDEC_ERR_NOEOB;
        e = pd_build(&S->tab[1], S->lens, hlit, false, lane, nl);
        if (e) return e;
        e = pd_build(&S->tab[2], S->lens + hlit, hdist, false, lane, nl);
        if (e) return e;
      }
      for (;;) {                                 // one symbol per round, at most 48 bits, at least one
        if (b.n < 48) pd_fill(&b);
        const int s = pd_symbol(&b, &S->tab[1]);
        if (b.err) return b.err;
        if (s == 256) break;
        if (s < 256) {
          if (produced >= raw_bytes) return GAN_PNGDEC_ERR_MORE;
          if (lane == 0) S->win[produced & (PD_WINDOW - 1)] = (uint8_t)s;
          ++produced;
        } else {
          if (s > 285) return GAN_PNGDEC_ERR_SYMBOL;
          int len;
          if (s < 265) len = s - 254;
          else if (s == 285) len = 258;
          else {
            const int x = (s - 261) >> 2;
            len = ((4 + ((s - 265) & 3)) << x) + 3 + (int)pd_take(&b, x);
            if (b.err) return b.err;
          }
          const int ds = pd_symbol(&b, &S->tab[2]);
          if (b.err) return b.err;
          if (ds > 29) return GAN_PNGDEC_ERR_SYMBOL;
          int64_t dist;
          if (ds < 4) dist = ds + 1;
          else {
            const int x = (ds >> 1) - 1;
            dist = ((2 + (ds & 1)) << x) + 1 + (int)pd_take(&b, x);
          }
          if (b.err) return b.err;
          if (dist > produced || dist > dmax) return GAN_PNGDEC_ERR_DIST;
          if (produced + len > raw_bytes) return GAN_PNGDEC_ERR_MORE;
          PD_SYNC();
          const int64_t from = produced - dist;  // every source byte lies in [from, produced): there before this match
          for (int k = lane; k < len; k += nl) {
            const int64_t src = from + (dist >= len ? k : k % (int)dist);
            S->win[(produced + k) & (PD_WINDOW - 1)] = S->win[src & (PD_WINDOW - 1)];
          }
          PD_SYNC();
          produced += len;
        }
        if (produced - flushed >= PD_FLUSH) {
          PD_SYNC();
          pd_flush(S, raw, flushed, PD_FLUSH, lane, nl);
          flushed += PD_FLUSH;
        }
      }
    }
    if (final_block) break;
  }
  if (produced < raw_bytes) return GAN_PNGDEC_ERR_LESS;
  if (b.left + b.n >= 8) return GAN_PNGDEC_ERR_LEFT;
  PD_SYNC();
  pd_flush(S, raw, flushed, (int)((produced - flushed + 15) / 16 * 16), lane, nl);
  return 0;
}

// ---- unfilter and convert.  The shared state of one image: two rows, its palette, the lanes' Adler-32 parts.
struct PdRows {
  alignas(16) uint8_t row[2][GAN_PNGDEC_MAX_ROWBYTES];
  uint8_t pal[768];
  uint32_t red[2][PD_MAX_LANES];
};
constexpr uint32_t PD_ADLER = 65521;
// raw: the image's H (1 + rowbytes) inflated bytes -> packed (H, W, 3) at out.  nl: a power of two, at most PD_MAX_LANES.
PD_FN int pd_pixels(const gan_pngdec_image* im, const uint8_t* blk, int64_t off_pal_i, const uint8_t* raw, PdRows* S, uint8_t* out, int lane, int nl) {
  const int H = im->H, W = im->W, rb = im->rowbytes, bpp = im->bpp, color = im->color, depth = im->depth, m = 1 + rb;
  const int64_t N = (int64_t)H * m;
  for (int i = lane; i < rb; i += nl) S->row[1][i] = 0;
  for (int i = lane; i < 768; i += nl) S->pal[i] = blk[off_pal_i + i];
  uint32_t S1 = 0, S2 = 0;                       // this lane's part of sum d[i] and sum (N - i) d[i], mod 65521
  for (int y = 0; y < H; ++y) {
    uint8_t* cur = S->row[y & 1];
    const uint8_t* prev = S->row[(y & 1) ^ 1];
    const uint8_t* src = raw + (int64_t)y * m;
    const int ft = src[0];
    if (ft > 4) return GAN_PNGDEC_ERR_FILTER;
    uint32_t s1 = 0, w = (uint32_t)((N - ((int64_t)y * m + (lane < m ? lane : 0))) % PD_ADLER);      // the weight of this lane's first byte of the row
    uint64_t s2 = 0;
    for (int j = lane; j < m; j += nl) {
      const uint32_t v = src[j];
      if (j > 0) cur[j - 1] = (uint8_t)v;
      s1 += v; s2 += (uint64_t)w * v;
      w = w >= (uint32_t)nl ? w - (uint32_t)nl : w + PD_ADLER - (uint32_t)nl;
    }
    S1 = (S1 + s1) % PD_ADLER; S2 = (uint32_t)((S2 + s2) % PD_ADLER);
    PD_SYNC();
    if (ft == 2) {
      for (int i = lane; i < rb; i += nl) cur[i] = (uint8_t)(cur[i] + prev[i]);
    } else if (ft == 1) {                        // Sub: a prefix sum per byte of the pixel (rb is a whole number of pixels; bpp = 1 for packed indices)
      const int npx = rb / bpp, seg = (npx + nl - 1) / nl;      // every lane takes `seg` pixels in a row
      const int p0 = lane * seg < npx ? lane * seg : npx, p1 = p0 + seg < npx ? p0 + seg : npx;
      for (int ch = 0; ch < bpp; ++ch) {         // the sums inside the lane's own stretch
        int a = 0;
        for (int p = p0; p < p1; ++p) {
          a = (a + cur[p * bpp + ch]) & 255;
          cur[p * bpp + ch] = (uint8_t)a;
        }
      }
      PD_SYNC();
      int off[4] = {0, 0, 0, 0};                 // what the stretches in front of this one add up to: their last pixels
      for (int l = 0; l < lane; ++l) {
        const int e = (l + 1) * seg < npx ? (l + 1) * seg : npx;
        if (e <= l * seg) break;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
          if (ch < bpp) off[ch] += cur[(e - 1) * bpp + ch];
      }
      PD_SYNC();
      for (int p = p0; p < p1; ++p) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
          if (ch < bpp) cur[p * bpp + ch] = (uint8_t)(cur[p * bpp + ch] + off[ch]);
      }
    } else if (ft != 0) {
      for (int ch = lane; ch < bpp; ch += nl) {  // Average and Paeth: one lane per byte of the pixel walks the row; left of the first pixel is zero
        int a = 0, c = 0;
        for (int i = ch; i < rb; i += bpp) {
          const int bb = prev[i];
          int pred;
          if (ft == 3) pred = (a + bb) >> 1;
          else {
            const int pa = bb > c ? bb - c : c - bb, pb = a > c ? a - c : c - a, t = a + bb - 2 * c, pc = t < 0 ? -t : t;
            pred = pa <= pb && pa <= pc ? a : pb <= pc ? bb : c;
          }
          a = (cur[i] + pred) & 255;
          cur[i] = (uint8_t)a;
          c = bb;
        }
      }
    }
    PD_SYNC();
    uint8_t* o = out + (int64_t)y * W * 3;
    for (int x = lane; x < W; x += nl) {
      int r, g, bl;
      if (color == 3) {
        const int bit = x * depth, idx = (cur[bit >> 3] >> (8 - depth - (bit & 7))) & ((1 << depth) - 1);
        r = S->pal[3 * idx]; g = S->pal[3 * idx + 1]; bl = S->pal[3 * idx + 2];
      } else if (color == 2 || color == 6) {
        r = cur[x * bpp]; g = cur[x * bpp + 1]; bl = cur[x * bpp + 2];
      } else {
        r = g = bl = cur[x * bpp];
      }
      o[3 * x] = (uint8_t)r; o[3 * x + 1] = (uint8_t)g; o[3 * x + 2] = (uint8_t)bl;
    }
  }
  PD_SYNC();
  S->red[0][lane] = S1; S->red[1][lane] = S2;
  PD_SYNC();
  for (int s = nl >> 1; s > 0; s >>= 1) {
    if (lane < s) { S->red[0][lane] += S->red[0][lane + s]; S->red[1][lane] += S->red[1][lane + s]; }
    PD_SYNC();
  }
  const uint32_t a = (1u + S->red[0][0]) % PD_ADLER, bsum = (uint32_t)((N + S->red[1][0]) % PD_ADLER);
  const uint8_t* t = blk + (int64_t)im->stream_off + im->stream_len - 4;
  const uint32_t want = (uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | (uint32_t)t[3];
  return (bsum << 16 | a) == want ? 0 : GAN_PNGDEC_ERR_ADLER;
}
