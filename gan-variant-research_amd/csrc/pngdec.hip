// PNG decoder on the device, pixel-identical to Image.open(p).convert("RGB") for the files dataio.PngDecoder's parser accepts; the
// arithmetic lives in pngdec_core.h, which a host program runs under a sanitizer over the same inputs.
//
//   gan_pngdec_inflate : one 64-lane workgroup per file, code tables and the 32 KiB window in LDS -> the filtered scanlines
//   gan_pngdec_pixels  : one 64-lane workgroup per file, two rows in LDS: unfilter, unpack, palette / grey / alpha -> packed HWC
#include "common.h"
#include "pngdec_core.h"

namespace {

constexpr int PAL_BYTES = 768;
constexpr int LANES = 64;                          // one workgroup is one wave: pngdec_core.h places its barriers for that
static_assert(LANES == PD_MAX_LANES && LANES == 64, "the PNG kernels run one wave64 per file");

struct PngLayout {
  int64_t off_pal, off_streams;                    // upload block
  int64_t off_raw;                                 // workspace; error words at 0
};

int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }

int block_offsets(int n, PngLayout* L) {
  GAN_CHECK(n >= 1 && n <= 65535, "pngdec: n=%d files outside 1 .. 65535", n);
  L->off_pal = (int64_t)n * sizeof(gan_pngdec_image);
  L->off_streams = L->off_pal + (int64_t)n * PAL_BYTES;
  L->off_raw = up256((int64_t)n * 4);
  return 0;
}

int check_geometry(const gan_pngdec_image& im, int i) {
  GAN_CHECK(im.H >= 1 && im.W >= 1, "pngdec: file %d: H=%d W=%d below 1", i, im.H, im.W);
  const bool pal = im.color == 3 && (im.depth == 1 || im.depth == 2 || im.depth == 4 || im.depth == 8);
  GAN_CHECK(pal || ((im.color == 0 || im.color == 2 || im.color == 4 || im.color == 6) && im.depth == 8),
            "pngdec: file %d: colour type %d at depth %d is outside the supported class", i, im.color, im.depth);
  const int channels = im.color == 2 ? 3 : im.color == 6 ? 4 : im.color == 4 ? 2 : 1;
  const int64_t bits = (int64_t)im.W * channels * im.depth;
  GAN_CHECK(im.bpp == (channels * im.depth + 7) / 8 && (int64_t)im.rowbytes == (bits + 7) / 8,
            "pngdec: file %d: bpp=%d rowbytes=%d do not belong to W=%d, colour type %d, depth %d", i, im.bpp, im.rowbytes, im.W, im.color, im.depth);
  GAN_CHECK(im.rowbytes <= GAN_PNGDEC_MAX_ROWBYTES, "pngdec: file %d: rowbytes=%d above the %d the unfilter kernel's rows hold", i, im.rowbytes,
            GAN_PNGDEC_MAX_ROWBYTES);
  GAN_CHECK((int64_t)im.H * (1 + im.rowbytes) < (1ll << 31) && (int64_t)im.H * im.W * 3 < (1ll << 31),
            "pngdec: file %d: H=%d W=%d: raw or output bytes at or above 2^31: too large", i, im.H, im.W);
  GAN_CHECK(pal ? im.pal_count >= (1 << im.depth) && im.pal_count <= 256 : im.pal_count == 0,
            "pngdec: file %d: palette of %d entries for colour type %d at depth %d", i, im.pal_count, im.color, im.depth);
  GAN_CHECK(im.wbits >= 8 && im.wbits <= 15, "pngdec: file %d: window bits %d outside 8 .. 15", i, im.wbits);
  return 0;
}

// Everything the kernels index with, checked on the host copy of the descriptors.
int check_block(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, const void* ws, int64_t ws_bytes, PngLayout* L) {
  if (block_offsets(n, L)) return -1;
  GAN_CHECK(blk_dev && blk_host && ws, "pngdec: null pointer");
  GAN_CHECK(blk_bytes >= L->off_streams && blk_bytes < (1ll << 31) && blk_bytes % 16 == 0,
            "pngdec: block of %lld bytes: %lld are descriptors and palettes, it ends at a multiple of 16, and byte offsets are 32-bit", (long long)blk_bytes,
            (long long)L->off_streams);
  GAN_CHECK((uintptr_t)blk_dev % 16 == 0 && (uintptr_t)ws % 16 == 0, "pngdec: block and workspace must be 16-byte aligned");
  GAN_CHECK(ws_bytes >= L->off_raw, "pngdec: workspace of %lld bytes is too small for %d error words", (long long)ws_bytes, n);
  const gan_pngdec_image* im = (const gan_pngdec_image*)blk_host;
  for (int i = 0; i < n; ++i) {
    if (check_geometry(im[i], i)) return -1;
    GAN_CHECK(im[i].stream_len >= 7 && im[i].stream_off >= L->off_streams && im[i].stream_off % 16 == 0 &&
                  ((int64_t)im[i].stream_off + im[i].stream_len + 15) / 16 * 16 <= blk_bytes,
              "pngdec: file %d: stream %d .. +%d is shorter than 7 bytes, not at a multiple of 16 or outside the block's stream area %lld .. %lld", i,
              im[i].stream_off, im[i].stream_len, (long long)L->off_streams, (long long)blk_bytes);
    const int64_t raw = ((int64_t)im[i].H * (1 + im[i].rowbytes) + 15) / 16 * 16;
    GAN_CHECK(im[i].raw_off >= L->off_raw && im[i].raw_off % 256 == 0 && im[i].raw_off + raw <= ws_bytes,
              "pngdec: file %d: raw offset %lld leaves the workspace of %lld bytes", i, (long long)im[i].raw_off, (long long)ws_bytes);
  }
  return 0;
}

__device__ __forceinline__ void load_descriptor(const uint8_t* blk, int b, gan_pngdec_image* im) {
  const uint32_t* si = reinterpret_cast<const uint32_t*>(blk + (int64_t)b * sizeof(gan_pngdec_image));
  if (threadIdx.x < (int)(sizeof(gan_pngdec_image) / 4)) reinterpret_cast<uint32_t*>(im)[threadIdx.x] = si[threadIdx.x];
  __syncthreads();
}

__global__ __launch_bounds__(LANES) void pngdec_inflate_kernel(const uint8_t* __restrict__ blk, char* __restrict__ ws) {
  __shared__ PdInflate S;
  __shared__ gan_pngdec_image im;
  const int b = blockIdx.x;
  load_descriptor(blk, b, &im);
  const int e = pd_inflate(&im, blk, &S, reinterpret_cast<uint8_t*>(ws + im.raw_off), (int)threadIdx.x, LANES);
  if (threadIdx.x == 0) reinterpret_cast<int32_t*>(ws)[b] = e;
}

__global__ __launch_bounds__(LANES) void pngdec_pixels_kernel(const uint8_t* __restrict__ blk, int64_t off_pal, char* __restrict__ ws, uint8_t* __restrict__ out,
                                                           int32_t* __restrict__ err) {
  __shared__ PdRows S;
  __shared__ gan_pngdec_image im;
  const int b = blockIdx.x;
  load_descriptor(blk, b, &im);
  int32_t* errw = reinterpret_cast<int32_t*>(ws);
  int e = errw[b];                                 // the same in every lane: a flagged file is left alone
  if (e == 0) {
    e = pd_pixels(&im, blk, off_pal + (int64_t)b * PAL_BYTES, reinterpret_cast<const uint8_t*>(ws + im.raw_off), &S, out + im.out_off, (int)threadIdx.x, LANES);
    if (threadIdx.x == 0) errw[b] = e;
  }
  if (threadIdx.x == 0 && err) err[b] = e;
}

}  // namespace

extern "C" int gan_pngdec_block_offsets(int n, int64_t* off) {
  PngLayout L;
  if (block_offsets(n, &L)) return -1;
  GAN_CHECK(off, "pngdec_block_offsets: null pointer");
  off[0] = L.off_pal; off[1] = L.off_streams;
  return 0;
}

extern "C" int gan_pngdec_bounds(gan_pngdec_image* imgs, int n, int64_t* ws_bytes) {
  PngLayout L;
  if (block_offsets(n, &L)) return -1;
  GAN_CHECK(imgs && ws_bytes, "pngdec_bounds: null pointer");
  int64_t o = L.off_raw;
  for (int i = 0; i < n; ++i) {
    if (check_geometry(imgs[i], i)) return -1;
    imgs[i].raw_off = o;
    o += up256((int64_t)imgs[i].H * (1 + imgs[i].rowbytes));
  }
  *ws_bytes = o;
  return 0;
}

extern "C" int gan_pngdec_inflate(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, void* ws, int64_t ws_bytes, void* stream) {
  PngLayout L;
  if (check_block(blk_dev, blk_host, blk_bytes, n, ws, ws_bytes, &L)) return -1;
  hipLaunchKernelGGL(pngdec_inflate_kernel, dim3(n), dim3(LANES), 0, (hipStream_t)stream, (const uint8_t*)blk_dev, (char*)ws);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_pngdec_pixels(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, void* ws, int64_t ws_bytes, uint8_t* out,
                                 int64_t out_bytes, int32_t* err, void* stream) {
  PngLayout L;
  if (check_block(blk_dev, blk_host, blk_bytes, n, ws, ws_bytes, &L)) return -1;
  GAN_CHECK(out, "pngdec_pixels: null pointer");
  const gan_pngdec_image* im = (const gan_pngdec_image*)blk_host;
  for (int i = 0; i < n; ++i)
    GAN_CHECK(im[i].out_off >= 0 && im[i].out_off + (int64_t)im[i].H * im[i].W * 3 <= out_bytes, "pngdec_pixels: file %d: output offset %lld leaves the output of %lld bytes",
              i, (long long)im[i].out_off, (long long)out_bytes);
  hipLaunchKernelGGL(pngdec_pixels_kernel, dim3(n), dim3(LANES), 0, (hipStream_t)stream, (const uint8_t*)blk_dev, L.off_pal, (char*)ws, out, err);
  GAN_LAUNCH_CHECK();
  return 0;
}
