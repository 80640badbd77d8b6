// CRC-32 (zlib's: reflected polynomial 0xEDB88320, register all ones at the start, complemented at the end; an empty range gives 0) as
// plain integer functions: the slice tables, the register over a span of a buffer, the 32-step carry-less multiply modulo the polynomial,
// x^(8 n) from the table of x^(2^k), and the split of a range into pieces whose registers are combined by that multiply.  zip.hip wraps
// them in kernels; crc32_host.cpp includes the same text and runs it on the CPU under AddressSanitizer and UBSan.
// A word holds a polynomial with the coefficient of x^0 in bit 31 (the reflected convention), so x^0 = 0x80000000 and x^1 = 0x40000000.
// Every load of crc32_span is clamped to [0, buf_bytes); crc32_range_ok is the test that decides whether a pair of offsets is read at all.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CRC_FN __host__ __device__ __forceinline__
#else
#define CRC_FN static inline
#endif

constexpr uint32_t CRC32_POLY = 0xEDB88320u;
constexpr int CRC32_TABLE_WORDS = 1024;          // four slice tables of 256 words: table s advances the register over a byte and s zero bytes

// One bit of the register: divide by x (a right shift in this convention), reduce when a coefficient falls out.
CRC_FN uint32_t crc32_shift1(uint32_t r) { return (r >> 1) ^ ((0u - (r & 1u)) & CRC32_POLY); }

// Entries i = lane, lane + nl, .. of the four tables.  tab[s * 256 + i] = the register i after 8 (s + 1) single-bit steps.
CRC_FN void crc32_fill_tables(uint32_t* tab, int lane, int nl) {
  for (int i = lane; i < 256; i += nl) {
    uint32_t r = (uint32_t)i;
    for (int s = 0; s < 4; ++s) {
      for (int k = 0; k < 8; ++k) r = crc32_shift1(r);
      tab[s * 256 + i] = r;
    }
  }
}

CRC_FN uint32_t crc32_step_byte(uint32_t c, uint32_t byte, const uint32_t* tab) { return (c >> 8) ^ tab[(c ^ byte) & 255u]; }
// Four bytes at once; w holds them with the first byte lowest.
CRC_FN uint32_t crc32_step_word(uint32_t c, uint32_t w, const uint32_t* tab) {
  c ^= w;
  return tab[768 + (c & 255u)] ^ tab[512 + ((c >> 8) & 255u)] ^ tab[256 + ((c >> 16) & 255u)] ^ tab[c >> 24];
}

// a(x) b(x) mod P(x): 32 steps, each adds b where a has a coefficient and multiplies b by x.  No branch depends on the data.
CRC_FN uint32_t crc32_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= (0u - ((a >> (31 - i)) & 1u)) & b;
    b = crc32_shift1(b);
  }
  return p;
}

// x^(2^k) mod P for k = 0 .. 31, by repeated squaring at compile time.  x has an order that divides 2^32 - 1, so x^(2^32) = x and the
// table is read with k mod 32.
struct Crc32Pow { uint32_t v[32]; };
constexpr uint32_t crc32_mulmod_const(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= (0u - ((a >> (31 - i)) & 1u)) & b;
    b = (b >> 1) ^ ((0u - (b & 1u)) & CRC32_POLY);
  }
  return p;
}
constexpr Crc32Pow crc32_make_pow() {
  Crc32Pow t{};
  uint32_t p = 0x40000000u;
  for (int k = 0; k < 32; ++k) { t.v[k] = p; p = crc32_mulmod_const(p, p); }
  return t;
}
CRC_FN uint32_t crc32_xpow2k(int k) {
  constexpr Crc32Pow t = crc32_make_pow();
  return t.v[k & 31];
}

// x^(8 n) mod P, n >= 0, from pw[k] = x^(2^k) (32 words: crc32_xpow2k, or a copy of it): one multiply per set bit of n.
CRC_FN uint32_t crc32_xpow8n(int64_t n, const uint32_t* pw) {
  uint32_t p = 0x80000000u;
  for (int k = 3; n > 0; n >>= 1, ++k)
    if (n & 1) p = crc32_mulmod(pw[k & 31], p);
  return p;
}

// CRC-32 of A followed by B from the CRC-32 of each and the length of B: crc(A) x^(8 |B|) + crc(B).
CRC_FN uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, int64_t len_b, const uint32_t* pw) {
  return crc32_mulmod(crc32_xpow8n(len_b, pw), crc_a) ^ crc_b;
}

// A pair of offsets names a range of buf[0 .. buf_bytes) exactly when 0 <= lo <= hi <= buf_bytes.
CRC_FN bool crc32_range_ok(int64_t lo, int64_t hi, int64_t buf_bytes) { return lo >= 0 && lo <= hi && hi <= buf_bytes; }

CRC_FN uint32_t crc32_load_byte(const uint8_t* buf, int64_t buf_bytes, int64_t i) {
  i = i < 0 ? 0 : i;
  i = i >= buf_bytes ? buf_bytes - 1 : i;
  return buf[i];
}

// CRC-32 of buf[lo .. hi), 0 when the span is empty.  Bytes up to the first address that is a multiple of 16, then 16-byte loads
// (sixteen at a time while 256 bytes are left, then four, then one), then bytes; a 16-byte load is issued only when it lies inside
// [0, buf_bytes), and every byte load is clamped to it.
CRC_FN uint32_t crc32_span(const uint8_t* buf, int64_t buf_bytes, int64_t lo, int64_t hi, const uint32_t* tab) {
  if (hi <= lo || buf_bytes <= 0) return 0u;
  uint32_t c = ~0u;
  int64_t i = lo;
  for (; i < hi && (((uintptr_t)buf + (uintptr_t)i) & 15u) != 0; ++i) c = crc32_step_byte(c, crc32_load_byte(buf, buf_bytes, i), tab);
  for (; i + 256 <= hi && i >= 0 && i + 256 <= buf_bytes; i += 256) {                    // sixteen loads in flight before the first is used:
    uint32_t w[64];                                                                      // a load that misses the cache costs more than its steps
    __builtin_memcpy(w, __builtin_assume_aligned(buf + i, 16), 256);
    for (int j = 0; j < 64; ++j) c = crc32_step_word(c, w[j], tab);
  }
  for (; i + 64 <= hi && i >= 0 && i + 64 <= buf_bytes; i += 64) {                       // four
    uint32_t w[16];
    __builtin_memcpy(w, __builtin_assume_aligned(buf + i, 16), 64);
    for (int j = 0; j < 16; ++j) c = crc32_step_word(c, w[j], tab);
  }
  for (; i + 16 <= hi && i >= 0 && i + 16 <= buf_bytes; i += 16) {
    uint32_t w[4];
    __builtin_memcpy(w, __builtin_assume_aligned(buf + i, 16), 16);
    for (int j = 0; j < 4; ++j) c = crc32_step_word(c, w[j], tab);
  }
  for (; i < hi; ++i) c = crc32_step_byte(c, crc32_load_byte(buf, buf_bytes, i), tab);
  return ~c;
}

// The range [lo, hi) of buf cut into np pieces, piece p = [crc32_piece_edge(p), crc32_piece_edge(p + 1)): every inner edge lies at an
// address that is a multiple of 16 (so only the first piece starts with single bytes), edge 0 is lo and edge np is hi.  Pieces at the end
// of a short range are empty.
CRC_FN int64_t crc32_piece_edge(const uint8_t* buf, int64_t lo, int64_t hi, int p, int np) {
  const int64_t a0 = lo - (int64_t)(((uintptr_t)buf + (uintptr_t)lo) & 15u);            // the 16-byte line lo lies in; a0 <= lo
  const int64_t per = ((hi - a0 + np - 1) / np + 15) / 16 * 16;              // a0 + np per >= hi
  const int64_t e = a0 + (int64_t)p * per;
  return p <= 0 ? lo : p >= np ? hi : e < lo ? lo : e > hi ? hi : e;
}

// What piece p of np adds to the CRC-32 of [lo, hi): its own CRC-32 times x^(8 (bytes after it)).  The CRC-32 of the range is the XOR
// of the np contributions, in any order.
CRC_FN uint32_t crc32_piece(const uint8_t* buf, int64_t buf_bytes, int64_t lo, int64_t hi, int p, int np, const uint32_t* tab, const uint32_t* pw) {
  const int64_t a = crc32_piece_edge(buf, lo, hi, p, np), b = crc32_piece_edge(buf, lo, hi, p + 1, np);
  if (b <= a) return 0u;
  return crc32_mulmod(crc32_xpow8n(hi - b, pw), crc32_span(buf, buf_bytes, a, b, tab));
}
