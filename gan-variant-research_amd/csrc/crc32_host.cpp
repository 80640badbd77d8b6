// Stand-alone host run of the CRC-32 arithmetic (crc32_core.h, the text the kernels of zip.hip compile), meant to be built with
// -fsanitize=address,undefined:
//   crc32_host
// It holds crc32_core.h to a bit-by-bit CRC written here, in three ways: every length 0 .. 300 at every residue of the start address
// modulo 16, as one span and as the pieces a workgroup cuts a range into (1024, and other counts); the combine identity on random
// splits; and the range clamp (offsets negative, decreasing, past the end), on a heap buffer of exactly the size the functions are
// told, so that a load one byte outside is reported.  Exit status 0 when everything agrees.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "crc32_core.h"

static uint32_t bitwise_crc(const uint8_t* p, int64_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (int64_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
  }
  return n > 0 ? ~c : 0u;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); if (++failures > 20) exit(1); } } while (0)

// The range as a workgroup of np lanes computes it.
static uint32_t by_pieces(const uint8_t* buf, int64_t buf_bytes, int64_t lo, int64_t hi, int np, const uint32_t* tab, const uint32_t* pw) {
  uint32_t v = 0;
  int64_t covered = lo;
  for (int p = 0; p < np; ++p) {
    const int64_t a = crc32_piece_edge(buf, lo, hi, p, np), b = crc32_piece_edge(buf, lo, hi, p + 1, np);
    EXPECT(a == covered && b >= a && b <= hi, "pieces of [%lld, %lld): piece %d = [%lld, %lld) after %lld", (long long)lo, (long long)hi, p, (long long)a, (long long)b, (long long)covered);
    EXPECT(p == 0 || a == hi || ((uintptr_t)(buf + a) & 15u) == 0, "piece %d of [%lld, %lld) starts off a 16-byte line", p, (long long)lo, (long long)hi);
    covered = b;
    v ^= crc32_piece(buf, buf_bytes, lo, hi, p, np, tab, pw);
  }
  EXPECT(covered == hi, "pieces of [%lld, %lld) end at %lld", (long long)lo, (long long)hi, (long long)covered);
  return v;
}

int main() {
  std::vector<uint32_t> tab(CRC32_TABLE_WORDS), tab3(CRC32_TABLE_WORDS);
  crc32_fill_tables(tab.data(), 0, 1);
  for (int lane = 0; lane < 3; ++lane) crc32_fill_tables(tab3.data(), lane, 3);                 // the lanes' shares make the same tables
  EXPECT(tab == tab3, "tables depend on the lane count");
  uint32_t pw[32];
  for (int k = 0; k < 32; ++k) pw[k] = crc32_xpow2k(k);
  {                                                                                            // x^(2^k) by single steps, k <= 12
    uint32_t p = 0x80000000u;
    int64_t e = 0;
    for (int k = 0; k <= 12; ++k) {
      for (; e < (1ll << k); ++e) p = crc32_shift1(p);
      EXPECT(p == pw[k], "x^(2^%d) = %08x, table %08x", k, p, pw[k]);
    }
    EXPECT(crc32_mulmod(pw[31], pw[31]) == pw[0] && crc32_xpow2k(32) == pw[0], "x^(2^32) != x");
    EXPECT(crc32_mulmod(0x80000000u, 0x12345678u) == 0x12345678u && crc32_mulmod(0x12345678u, 0x80000000u) == 0x12345678u, "1 is not the unit");
    EXPECT(crc32_xpow8n(0, pw) == 0x80000000u, "x^0");
  }
  const uint8_t check[9] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
  EXPECT(bitwise_crc(check, 9) == 0xCBF43926u, "the bit-by-bit CRC misses the check value");

  // 1. every length 0 .. 300 at every residue; contents random, zeros, 0xFF
  for (int fill = 0; fill < 3; ++fill)
    for (int res = 0; res < 16; ++res)
      for (int len = 0; len <= 300; ++len) {
        const int64_t total = res + len + 1;                                                   // one byte after the range, inside the buffer
        uint8_t* buf = (uint8_t*)aligned_alloc(16, (total + 15) / 16 * 16);
        uint8_t* exact = (uint8_t*)malloc(total);                                              // exactly `total` bytes: ASan guards the rest
        for (int64_t i = 0; i < total; ++i) buf[i] = fill == 0 ? (uint8_t)rnd() : fill == 1 ? 0 : 0xFF;
        memcpy(exact, buf, total);
        const uint32_t want = bitwise_crc(buf + res, len);
        const uint32_t a = crc32_span(buf, total, res, res + len, tab.data());
        const uint32_t b = crc32_span(exact, total, res, res + len, tab.data());
        const uint32_t c = by_pieces(buf, total, res, res + len, 256, tab.data(), pw);
        const uint32_t d = by_pieces(exact, total, res, res + len, 7, tab.data(), pw);
        const uint32_t e = by_pieces(exact, total, res, res + len, 1024, tab.data(), pw);
        EXPECT(a == want && b == want && c == want && d == want && e == want, "fill %d residue %d length %d: span %08x %08x, pieces %08x %08x %08x, bit by bit %08x", fill, res,
               len, a, b, c, d, e, want);
        free(buf); free(exact);
      }

  // 2. the combine identity on random splits, and the pieces of longer ranges
  {
    const int64_t N = 70001;
    uint8_t* buf = (uint8_t*)malloc(N);
    for (int64_t i = 0; i < N; ++i) buf[i] = (uint8_t)rnd();
    for (int it = 0; it < 200; ++it) {
      int64_t lo = rnd() % N, hi = rnd() % (N + 1);
      if (lo > hi) { const int64_t t = lo; lo = hi; hi = t; }
      const int64_t mid = lo + rnd() % (hi - lo + 1);
      const uint32_t whole = bitwise_crc(buf + lo, hi - lo), left = bitwise_crc(buf + lo, mid - lo), right = bitwise_crc(buf + mid, hi - mid);
      EXPECT(crc32_combine(left, right, hi - mid, pw) == whole, "combine [%lld, %lld) + [%lld, %lld)", (long long)lo, (long long)mid, (long long)mid, (long long)hi);
      EXPECT(by_pieces(buf, N, lo, hi, 1024, tab.data(), pw) == whole && by_pieces(buf, N, lo, hi, 3, tab.data(), pw) == whole, "pieces of [%lld, %lld)", (long long)lo,
             (long long)hi);
    }
    EXPECT(crc32_combine(0x12345678u, 0u, 0, pw) == 0x12345678u, "combine with an empty tail");
    free(buf);
  }

  // 3. the clamp: pairs that are no range are refused; whatever crc32_span is handed, no load leaves [0, buf_bytes)
  {
    const int64_t N = 100;
    uint8_t* buf = (uint8_t*)malloc(N);
    for (int64_t i = 0; i < N; ++i) buf[i] = (uint8_t)rnd();
    const int64_t bad[][2] = {{-1, 10}, {-20, -10}, {10, 5}, {0, 101}, {90, 1000}, {101, 101}, {-5, 200}, {INT64_MIN, INT64_MAX}, {50, INT64_MAX}, {INT64_MIN, 50}};
    for (const auto& r : bad) EXPECT(!crc32_range_ok(r[0], r[1], N), "the pair (%lld, %lld) passes for a buffer of %lld bytes", (long long)r[0], (long long)r[1], (long long)N);
    const int64_t good[][2] = {{0, 0}, {0, 100}, {100, 100}, {37, 38}};
    for (const auto& r : good) EXPECT(crc32_range_ok(r[0], r[1], N), "the pair (%lld, %lld) is refused", (long long)r[0], (long long)r[1]);
    EXPECT(crc32_range_ok(0, 0, 0) && !crc32_range_ok(0, 1, 0), "the empty buffer");
    const int64_t wild[][2] = {{-40, 10}, {90, 140}, {-3, 103}, {10, 5}, {100, 130}, {-30, -10}};
    for (const auto& r : wild) (void)crc32_span(buf, N, r[0], r[1], tab.data());               // values are not defined; the loads must stay inside
    EXPECT(crc32_span(buf, 0, 0, 10, tab.data()) == 0u, "an empty buffer is read");
    free(buf);
  }
  if (failures) { fprintf(stderr, "crc32_host: %d checks failed\n", failures); return 1; }
  printf("crc32_host: crc32_core.h agrees with the bit-by-bit CRC\n");
  return 0;
}
