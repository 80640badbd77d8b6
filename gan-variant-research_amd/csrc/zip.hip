// What a stored ZIP entry needs beside its name, made on the device: the bytes of the complete file and their CRC-32.
//
//   gan_crc32_ranges : CRC-32 of n byte ranges of one buffer, one workgroup per range.  The lanes take pieces of the range (crc32_core.h:
//                      16-byte loads, four slice tables in LDS); every lane multiplies its register by x^(8 bytes after its piece) modulo
//                      the polynomial and the workgroup XORs the products.  Integer code only, no order-dependent atomics.
//   gan_jpeg_files   : complete JPEG files back to back from what the encoder holds (constant head, four DHT segments from the table
//                      kernel's rows, constant SOS, the image's scan bytes, EOI).  Three launches, no host round trip: sizes and their
//                      exclusive scan (one workgroup), the copy (one workgroup per file), the CRC-32 of every file (the kernel above).
#include "common.h"
#include "crc32_core.h"

namespace {

constexpr int ZIP_THREADS = 256;                 // the sizes kernel
constexpr int CRC_THREADS = 256;                 // lanes, and so pieces, per range.  One wave per SIMD: the multiplies of the combine cost a wave
                                                 // the same whatever its lanes hold, and with 1024 lanes they took longer than the loads they saved
constexpr int COPY_THREADS = 1024;               // a lane's loads follow one another: more lanes wait less
constexpr int DHT_ROW = 272;                     // gan_jpeg_tables: 16 counts, then up to 256 symbols

__global__ __launch_bounds__(CRC_THREADS) void crc32_ranges_kernel(const uint8_t* __restrict__ buf, int64_t buf_bytes, const int64_t* __restrict__ offsets,
                                                                   uint32_t* __restrict__ crc, uint32_t* __restrict__ flag) {
  __shared__ uint32_t tab[CRC32_TABLE_WORDS];
  __shared__ uint32_t pw[32];
  __shared__ uint32_t part[CRC_THREADS / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int64_t lo = offsets[r], hi = offsets[r + 1];
  if (!crc32_range_ok(lo, hi, buf_bytes)) {      // the same in every lane: nothing is read
    if (tid == 0) { crc[r] = 0u; atomicOr(flag, 1u); }
    return;
  }
  crc32_fill_tables(tab, tid, CRC_THREADS);
  if (tid < 32) pw[tid] = crc32_xpow2k(tid);
  __syncthreads();
  uint32_t v = crc32_piece(buf, buf_bytes, lo, hi, tid, CRC_THREADS, tab, pw);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o, 64);
  if ((tid & 63) == 0) part[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    uint32_t all = 0;
#pragma unroll
    for (int w = 0; w < CRC_THREADS / 64; ++w) all ^= part[w];
    crc[r] = all;
  }
}

struct FilesArgs {
  const uint8_t *head, *sos, *dht, *scan;
  const int64_t* scan_offsets;
  int head_bytes, sos_bytes, B;
  int64_t scan_bytes, files_bytes;
};

// Symbols of table t of image b: the sum of the row's 16 counts, at most 256.
__device__ __forceinline__ int dht_symbols(const uint8_t* __restrict__ dht, int b, int t) {
  const uint8_t* row = dht + ((int64_t)b * 4 + t) * DHT_ROW;
  int n = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) n += row[i];
  return min(n, 256);
}

// The scan bytes of image b as (first byte, length); an inconsistent pair of offsets gives an empty scan and *bad = true.
__device__ __forceinline__ int64_t scan_range(const FilesArgs& a, int b, int64_t* len, bool* bad) {
  const int64_t lo = a.scan_offsets[b], hi = a.scan_offsets[b + 1];
  *bad = !crc32_range_ok(lo, hi, a.scan_bytes);
  *len = *bad ? 0 : hi - lo;
  return *bad ? 0 : lo;
}

// Sizes and their exclusive scan.  One workgroup walks the batch ZIP_THREADS files at a time.  Offsets are clamped to files_bytes, so
// whatever reads them stays inside the buffer; *flag is overwritten: bit 0 an inconsistent pair of scan offsets, bit 1 files too small.
__global__ __launch_bounds__(ZIP_THREADS) void jpeg_file_sizes_kernel(FilesArgs a, int64_t* __restrict__ file_offsets, uint32_t* __restrict__ flag) {
  __shared__ int64_t wsum[ZIP_THREADS / 64];
  __shared__ uint32_t bits;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) bits = 0u;
  __syncthreads();
  int64_t carry = 0;
  uint32_t mine = 0;
  for (int base = 0; base < a.B; base += ZIP_THREADS) {
    const int b = base + tid;
    int64_t size = 0;
    if (b < a.B) {
      bool bad;
      int64_t slen;
      scan_range(a, b, &slen, &bad);
      mine |= bad ? 1u : 0u;
      size = (int64_t)a.head_bytes + a.sos_bytes + 2 + slen;
      for (int t = 0; t < 4; ++t) size += 5 + 16 + dht_symbols(a.dht, b, t);
    }
    int64_t inc = size;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int64_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < ZIP_THREADS / 64; ++i) {
      const int64_t s = wsum[i];
      if (i < w) before += s;
      all += s;
    }
    if (b < a.B) {
      const int64_t first = carry + before + inc - size;
      mine |= first + size > a.files_bytes ? 2u : 0u;
      file_offsets[b] = min(first, a.files_bytes);
      if (b == a.B - 1) file_offsets[a.B] = min(first + size, a.files_bytes);
    }
    carry += all;
  }
  if (mine) atomicOr(&bits, mine);               // LDS
  __syncthreads();
  if (tid == 0) *flag = bits;
}

// Byte `rel` of file b.  seg_dht[t] = first byte of DHT segment t, seg_dht[4] = of SOS; seg_scan, seg_eoi = of the scan bytes, of EOI.
__device__ __forceinline__ uint32_t file_byte(const FilesArgs& a, int b, const int* seg_dht, int64_t seg_scan, int64_t seg_eoi, int64_t scan_lo, int64_t rel) {
  if (rel < a.head_bytes) return a.head[rel];
  if (rel < seg_dht[4]) {
    int t = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i) t += rel >= seg_dht[i] ? 1 : 0;
    const int r = (int)rel - seg_dht[t], len = seg_dht[t + 1] - seg_dht[t] - 2;           // the length field counts itself, not the marker
    if (r == 0) return 0xFFu;
    if (r == 1) return 0xC4u;
    if (r == 2) return (uint32_t)len >> 8;
    if (r == 3) return (uint32_t)len & 255u;
    if (r == 4) return (uint32_t)((t & 1) << 4 | (t >> 1));                               // DC0, AC0, DC1, AC1 = 0x00, 0x10, 0x01, 0x11
    return a.dht[((int64_t)b * 4 + t) * DHT_ROW + (r - 5)];                               // r - 5 < 16 + symbols <= DHT_ROW
  }
  if (rel < seg_scan) return a.sos[rel - seg_dht[4]];
  if (rel < seg_eoi) return a.scan[scan_lo + (rel - seg_scan)];
  return rel == seg_eoi ? 0xFFu : 0xD9u;
}

// The copy.  One workgroup per file; a thread takes one aligned 16-byte line of `files` at a time.  A line that lies wholly inside the
// file's scan bytes is one 16-byte store, made of the five aligned source words that hold its bytes (whatever the residues of source
// and destination) when they lie inside the scan block, of sixteen byte loads otherwise; the lines at the file's ends and everything
// before the scan are written byte by byte.  Nothing at or past file_offsets[b + 1] <= files_bytes is written.
__global__ __launch_bounds__(COPY_THREADS) void jpeg_file_copy_kernel(FilesArgs a, const int64_t* __restrict__ file_offsets, uint8_t* __restrict__ files) {
  __shared__ int seg_dht[5];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    int p = a.head_bytes;
    for (int t = 0; t < 4; ++t) { seg_dht[t] = p; p += 5 + 16 + dht_symbols(a.dht, b, t); }
    seg_dht[4] = p;
  }
  __syncthreads();
  bool bad;
  int64_t slen;
  const int64_t scan_lo = scan_range(a, b, &slen, &bad);
  const int64_t seg_scan = (int64_t)seg_dht[4] + a.sos_bytes, seg_eoi = seg_scan + slen;
  const int64_t f0 = file_offsets[b], f1 = min(min(file_offsets[b + 1], f0 + seg_eoi + 2), a.files_bytes);
  if (f0 < 0 || f1 <= f0) return;
  const uintptr_t base = (uintptr_t)files, sbase = (uintptr_t)a.scan;
  const int64_t l0 = (int64_t)((base + (uintptr_t)f0) >> 4), l1 = (int64_t)((base + (uintptr_t)f1 + 15) >> 4);     // lines that overlap the file
  for (int64_t l = l0 + tid; l < l1; l += COPY_THREADS) {
    const int64_t p = (int64_t)(((uintptr_t)l << 4) - base);                              // offset of the line's first byte in files; may be < f0
    const int64_t rel = p - f0;
    if (p >= f0 && p + 16 <= f1 && rel >= seg_scan && rel + 16 <= seg_eoi) {
      const int64_t s = scan_lo + (rel - seg_scan);                                       // source bytes scan[s .. s + 16), inside the image's scan
      const uintptr_t sa = sbase + (uintptr_t)s, al = sa & ~(uintptr_t)3;
      const int sh = (int)(sa & 3u) * 8;
      u32x4_t v;
      if (al >= sbase && al + 20 <= sbase + (uintptr_t)a.scan_bytes) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(al);
        uint32_t w[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) w[j] = q[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (uint32_t)((((uint64_t)w[j + 1] << 32) | w[j]) >> sh);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          v[j] = (uint32_t)a.scan[s + 4 * j] | (uint32_t)a.scan[s + 4 * j + 1] << 8 | (uint32_t)a.scan[s + 4 * j + 2] << 16 | (uint32_t)a.scan[s + 4 * j + 3] << 24;
      }
      *reinterpret_cast<u32x4_t*>(files + p) = v;
    } else {
      for (int j = 0; j < 16; ++j)
        if (p + j >= f0 && p + j < f1) files[p + j] = (uint8_t)file_byte(a, b, seg_dht, seg_scan, seg_eoi, scan_lo, rel + j);
    }
  }
}

int files_check(const char* who, int B, int head_bytes, int sos_bytes) {
  GAN_CHECK(B >= 1 && B <= 65535, "%s: B=%d outside 1 .. 65535", who, B);
  GAN_CHECK(head_bytes >= 2 && head_bytes <= 65535 && sos_bytes >= 4 && sos_bytes <= 65535, "%s: head of %d bytes (2 .. 65535), SOS of %d bytes (4 .. 65535)",
            who, head_bytes, sos_bytes);
  return 0;
}

}  // namespace

extern "C" int gan_crc32_ranges(const uint8_t* buf, int64_t buf_bytes, const int64_t* offsets, int n, uint32_t* crc, uint32_t* flag, void* stream) {
  GAN_CHECK(buf && offsets && crc && flag, "crc32_ranges: null pointer");
  GAN_CHECK(n >= 0, "crc32_ranges: n=%d ranges: negative", n);
  GAN_CHECK(buf_bytes >= 0, "crc32_ranges: buffer of %lld bytes: negative", (long long)buf_bytes);
  if (n == 0) return 0;
  hipLaunchKernelGGL(crc32_ranges_kernel, dim3(n), dim3(CRC_THREADS), 0, (hipStream_t)stream, buf, buf_bytes, offsets, crc, flag);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_jpeg_files_bounds(int B, int H, int W, int head_bytes, int sos_bytes, int64_t* files_bytes) {
  GAN_CHECK(files_bytes, "jpeg_files_bounds: null pointer");
  if (files_check("jpeg_files_bounds", B, head_bytes, sos_bytes)) return -1;
  int64_t ws = 0, out = 0;
  if (gan_jpeg_bounds(B, H, W, &ws, &out)) return -1;
  *files_bytes = out + (int64_t)B * (head_bytes + 4 * (5 + 16 + 256) + sos_bytes + 2);
  return 0;
}

extern "C" int gan_jpeg_files(const uint8_t* head, int head_bytes, const uint8_t* sos, int sos_bytes, const uint8_t* dht, const uint8_t* scan,
                              int64_t scan_bytes, const int64_t* scan_offsets, int B, uint8_t* files, int64_t files_bytes, int64_t* file_offsets,
                              uint32_t* crc, uint32_t* flag, void* stream) {
  GAN_CHECK(head && sos && dht && scan && scan_offsets && files && file_offsets && crc && flag, "jpeg_files: null pointer");
  if (files_check("jpeg_files", B, head_bytes, sos_bytes)) return -1;
  GAN_CHECK(scan_bytes >= 0 && files_bytes >= 0, "jpeg_files: scan block of %lld bytes, files of %lld bytes: negative", (long long)scan_bytes, (long long)files_bytes);
  hipStream_t s = (hipStream_t)stream;
  FilesArgs a;
  a.head = head; a.sos = sos; a.dht = dht; a.scan = scan; a.scan_offsets = scan_offsets;
  a.head_bytes = head_bytes; a.sos_bytes = sos_bytes; a.B = B; a.scan_bytes = scan_bytes; a.files_bytes = files_bytes;
  hipLaunchKernelGGL(jpeg_file_sizes_kernel, dim3(1), dim3(ZIP_THREADS), 0, s, a, file_offsets, flag);
  hipLaunchKernelGGL(jpeg_file_copy_kernel, dim3(B), dim3(COPY_THREADS), 0, s, a, file_offsets, files);
  hipLaunchKernelGGL(crc32_ranges_kernel, dim3(B), dim3(CRC_THREADS), 0, s, (const uint8_t*)files, files_bytes, (const int64_t*)file_offsets, crc, flag);
  GAN_LAUNCH_CHECK();
  return 0;
}
