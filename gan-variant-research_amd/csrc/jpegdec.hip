// Baseline JPEG decoder on the device, pixel-identical to Image.open(p).convert("RGB") (libjpeg-turbo) for the files dataio.JpegDecoder's
// parser accepts; the arithmetic lives in jpegdec_core.h, which a host program runs under a sanitizer over the same inputs.
//
//   gan_jpegdec_tables  : one wave per DHT table -> 9-bit lookahead + maxcode / value offsets; error words and coefficients zeroed
//   gan_jpegdec_entropy : one 64-lane workgroup per image, tables in LDS, lane s decodes restart segments s, s + 64, ..
//   gan_jpegdec_idct    : one thread per 8x8 block, dequantise + jpeg_idct_islow -> uint8 component planes
//   gan_jpegdec_pixels  : one thread per pixel, fancy upsampling + YCbCr -> RGB, packed HWC at the image's offset of the destination
//
// Tables, idct and pixels are the back end of jpegdec_back.h, which the progressive decoder (jpegprog.hip) launches too: a progressive
// decode shows jpegdec_tables_kernel, jpegdec_idct_kernel and jpegdec_pixels_kernel in a trace, beside jpegprog_entropy_kernel.
#include "common.h"
#include "jpegdec_core.h"
#include "jpegdec_back.h"

// ------------------------------------------------------------------------------------------------ the back end of both decoders
namespace {

__global__ __launch_bounds__(64) void jpegdec_tables_kernel(const uint8_t* __restrict__ dht, JdTable* __restrict__ tabs) {
  __shared__ JdTable t;
  jd_tables_body(dht, tabs, &t);
}

__global__ __launch_bounds__(256) void jpegdec_idct_kernel(const uint8_t* __restrict__ blk, int64_t off_qt, char* __restrict__ ws,
                                                           int32_t* __restrict__ errw) {
  jd_idct_body(blk, off_qt, ws, errw);
}

__global__ __launch_bounds__(256) void jpegdec_pixels_kernel(const uint8_t* __restrict__ blk, const char* __restrict__ ws, uint8_t* __restrict__ out,
                                                             const int32_t* __restrict__ errw, int32_t* __restrict__ err) {
  jd_pixels_body(blk, ws, out, errw, err);
}

}  // namespace

int64_t jd_up256(int64_t v) { return (v + 255) / 256 * 256; }

int jd_check_geometry(const char* who, const gan_jpegdec_image& im, int i) {
  GAN_CHECK(im.H >= 1 && im.H <= 65535 && im.W >= 1 && im.W <= 65535, "%s: image %d: H=%d W=%d outside 1 .. 65535", who, i, im.H, im.W);
  const bool gray = im.ncomp == 1 && im.hmax == 1 && im.vmax == 1;
  const bool colour = im.ncomp == 3 && (im.hmax == 1 || im.hmax == 2) && (im.vmax == 1 || im.vmax == 2) && !(im.hmax == 1 && im.vmax == 2);
  GAN_CHECK(gray || colour, "%s: image %d: %d components with luma sampling %dx%d is outside the supported class", who, i, im.ncomp, im.hmax, im.vmax);
  GAN_CHECK(im.mcux == (im.W + 8 * im.hmax - 1) / (8 * im.hmax) && im.mcuy == (im.H + 8 * im.vmax - 1) / (8 * im.vmax),
            "%s: image %d: %dx%d MCUs do not belong to H=%d W=%d", who, i, im.mcuy, im.mcux, im.H, im.W);
  return 0;
}

int jd_check_images(const char* who, const gan_jpegdec_image* im, int n, int64_t ws_bytes, int64_t off_coef, JdBack* B) {
  int64_t coef_end = off_coef, max_blocks = 0, max_pixels = 0;
  for (int i = 0; i < n; ++i) {
    if (jd_check_geometry(who, im[i], i)) return -1;
    for (int c = 0; c < 3; ++c)
      GAN_CHECK(im[i].q_tab[c] >= 0 && im[i].q_tab[c] <= 3, "%s: image %d: table slots: quantisation slot of component %d outside 0 .. 3", who, i, c);
    const int64_t nb = jd_blocks(&im[i]);
    GAN_CHECK(nb < (1 << 24), "%s: image %d: %lld blocks: too large", who, i, (long long)nb);
    GAN_CHECK(im[i].coef_off >= off_coef && im[i].coef_off % 16 == 0 && im[i].coef_off + nb * 128 <= ws_bytes,
              "%s: image %d: coefficient offset %lld leaves the workspace of %lld bytes", who, i, (long long)im[i].coef_off, (long long)ws_bytes);
    coef_end = im[i].coef_off + nb * 128 > coef_end ? im[i].coef_off + nb * 128 : coef_end;
    max_blocks = nb > max_blocks ? nb : max_blocks;
    max_pixels = (int64_t)im[i].H * im[i].W > max_pixels ? (int64_t)im[i].H * im[i].W : max_pixels;
  }
  B->off_planes = coef_end;
  for (int i = 0; i < n; ++i)                      // the planes lie behind every coefficient area (tables zeroes that span with one memset)
    GAN_CHECK(im[i].plane_off >= coef_end && im[i].plane_off % 16 == 0 && im[i].plane_off + jd_plane_bytes(&im[i]) <= ws_bytes,
              "%s: image %d: plane offset %lld leaves the workspace of %lld bytes", who, i, (long long)im[i].plane_off, (long long)ws_bytes);
  B->max_blocks = (int)max_blocks;
  GAN_CHECK(max_pixels < (1ll << 32), "%s: image too large", who);
  B->max_pixels = (int)((max_pixels + 255) / 256);   // in workgroups of 256
  return 0;
}

int jd_place(const char* who, gan_jpegdec_image* imgs, int n, int64_t off_coef, int64_t* ws_bytes) {
  GAN_CHECK(imgs && ws_bytes, "%s_bounds: null pointer", who);
  int64_t o = off_coef;
  for (int i = 0; i < n; ++i) {
    if (jd_check_geometry(who, imgs[i], i)) return -1;
    imgs[i].coef_off = o;
    o += jd_up256((int64_t)jd_blocks(&imgs[i]) * 128);
  }
  for (int i = 0; i < n; ++i) {
    imgs[i].plane_off = o;
    o += jd_up256(jd_plane_bytes(&imgs[i]));
  }
  *ws_bytes = o;
  return 0;
}

int jd_launch_tables(const char* who, const uint8_t* dht, int ntab, void* ws, int64_t off_err, int64_t off_planes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync((char*)ws + off_err, 0, (size_t)(off_planes - off_err), s) != hipSuccess) return gan_set_error(-2, "%s_tables: hipMemsetAsync failed", who);
  hipLaunchKernelGGL(jpegdec_tables_kernel, dim3(ntab), dim3(64), 0, s, dht, (JdTable*)ws);
  GAN_LAUNCH_CHECK();
  return 0;
}

int jd_launch_idct(const void* blk_dev, int n, int64_t off_qt, void* ws, int64_t off_err, int max_blocks, void* stream) {
  hipLaunchKernelGGL(jpegdec_idct_kernel, dim3((max_blocks + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)blk_dev, off_qt, (char*)ws,
                     (int32_t*)((char*)ws + off_err));
  GAN_LAUNCH_CHECK();
  return 0;
}

int jd_launch_pixels(const char* who, const void* blk_dev, const gan_jpegdec_image* im, int n, const void* ws, int64_t off_err, int max_pixels, uint8_t* out,
                     int64_t out_bytes, int32_t* err, void* stream) {
  GAN_CHECK(out, "%s_pixels: null pointer", who);
  for (int i = 0; i < n; ++i)
    GAN_CHECK(im[i].out_off >= 0 && im[i].out_off + (int64_t)im[i].H * im[i].W * 3 <= out_bytes, "%s_pixels: image %d: output offset %lld leaves the output of %lld bytes",
              who, i, (long long)im[i].out_off, (long long)out_bytes);
  hipLaunchKernelGGL(jpegdec_pixels_kernel, dim3(max_pixels, n), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)blk_dev, (const char*)ws, out,
                     (const int32_t*)((const char*)ws + off_err), err);
  GAN_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------ what is baseline about it
namespace {

constexpr int DHT_BYTES = JD_DHT_BYTES, QT_BYTES = 4 * 64 * 2;

struct DecLayout {
  int64_t off_seg, off_dht, off_qt, off_scan;      // upload block
  int64_t off_err, off_coef;                       // workspace; tables at 0
  JdBack back;
};

int block_offsets(int n, int nseg, DecLayout* L) {
  GAN_CHECK(n >= 1 && n <= 65535 && nseg >= 1 && nseg <= (1 << 24), "jpegdec: n=%d images, nseg=%d segments outside 1 <= n <= 65535, 1 <= nseg <= 2^24", n, nseg);
  L->off_seg = (int64_t)n * sizeof(gan_jpegdec_image);
  L->off_dht = L->off_seg + (int64_t)nseg * sizeof(gan_jpegdec_segment);
  L->off_qt = (L->off_dht + (int64_t)n * 4 * DHT_BYTES + 15) / 16 * 16;
  L->off_scan = (L->off_qt + (int64_t)n * QT_BYTES + 15) / 16 * 16;
  L->off_err = jd_up256((int64_t)n * 4 * sizeof(JdTable));
  L->off_coef = L->off_err + jd_up256((int64_t)n * 4);
  return 0;
}

// Everything the kernels index with, checked on the host copy of the descriptors.
int check_block(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nseg, const void* ws, int64_t ws_bytes, DecLayout* L) {
  if (block_offsets(n, nseg, L)) return -1;
  GAN_CHECK(blk_dev && blk_host && ws, "jpegdec: null pointer");
  GAN_CHECK(blk_bytes >= L->off_scan && blk_bytes < (1ll << 31), "jpegdec: block of %lld bytes: %lld are descriptors and tables, and byte offsets are 32-bit",
            (long long)blk_bytes, (long long)L->off_scan);
  GAN_CHECK((uintptr_t)blk_dev % 16 == 0 && (uintptr_t)ws % 16 == 0, "jpegdec: block and workspace must be 16-byte aligned");
  const gan_jpegdec_image* im = (const gan_jpegdec_image*)blk_host;
  const gan_jpegdec_segment* sg = (const gan_jpegdec_segment*)((const char*)blk_host + L->off_seg);
  if (jd_check_images("jpegdec", im, n, ws_bytes, L->off_coef, &L->back)) return -1;
  for (int i = 0; i < n; ++i) {
    for (int c = 0; c < 3; ++c)
      GAN_CHECK((im[i].dc_tab[c] | 1) == 1 && (im[i].ac_tab[c] | 1) == 3, "jpegdec: image %d: table slots of component %d outside DC 0 | 1, AC 2 | 3", i, c);
    GAN_CHECK(im[i].seg_first >= 0 && im[i].seg_count >= 1 && (int64_t)im[i].seg_first + im[i].seg_count <= nseg,
              "jpegdec: image %d: segments %d .. +%d outside the table of %d", i, im[i].seg_first, im[i].seg_count, nseg);
    for (int j = 0; j < im[i].seg_count; ++j) {
      const gan_jpegdec_segment& s = sg[im[i].seg_first + j];
      GAN_CHECK(s.image == i, "jpegdec: segment %d of image %d names image %d", j, i, s.image);
      GAN_CHECK(s.mcu_first >= 0 && s.mcu_count >= 1 && (int64_t)s.mcu_first + s.mcu_count <= (int64_t)im[i].mcux * im[i].mcuy,
                "jpegdec: segment %d of image %d: MCUs %d .. +%d outside the image", j, i, s.mcu_first, s.mcu_count);
      GAN_CHECK(s.byte_begin >= L->off_scan + (j > 0 ? 2 : 0) && s.byte_begin <= s.byte_end && s.byte_end <= blk_bytes,
                "jpegdec: segment %d of image %d: bytes %d .. %d outside the block's scan area %lld .. %lld", j, i, s.byte_begin, s.byte_end,
                (long long)L->off_scan, (long long)blk_bytes);
    }
  }
  return 0;
}

__global__ __launch_bounds__(64) void jpegdec_entropy_kernel(const uint8_t* __restrict__ blk, int64_t off_seg, const JdTable* __restrict__ tabs,
                                                             char* __restrict__ ws, int32_t* __restrict__ errw) {
  __shared__ JdTable t[4];
  __shared__ gan_jpegdec_image im;
  __shared__ uint8_t zz[64];
  const int b = blockIdx.x;
  zz[threadIdx.x] = jd_zigzag[threadIdx.x];
  {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(tabs + 4 * (int64_t)b);
    uint32_t* d = reinterpret_cast<uint32_t*>(t);
    for (int i = threadIdx.x; i < (int)(4 * sizeof(JdTable) / 4); i += 64) d[i] = s[i];
    const uint32_t* si = reinterpret_cast<const uint32_t*>(blk + (int64_t)b * sizeof(gan_jpegdec_image));
    if (threadIdx.x < (int)(sizeof(gan_jpegdec_image) / 4)) reinterpret_cast<uint32_t*>(&im)[threadIdx.x] = si[threadIdx.x];
  }
  __syncthreads();
  const gan_jpegdec_segment* segs = reinterpret_cast<const gan_jpegdec_segment*>(blk + off_seg) + im.seg_first;
  int16_t* coef = reinterpret_cast<int16_t*>(ws + im.coef_off);
  int err = 0;
  for (int j = threadIdx.x; j < im.seg_count; j += 64) {
    const gan_jpegdec_segment sg = segs[j];
    err |= jd_decode_segment(&im, &sg, j, blk, t, zz, coef);
  }
  if (err) atomicOr(&errw[b], err);
}

}  // namespace

extern "C" int gan_jpegdec_block_offsets(int n, int nseg, int64_t* off) {
  DecLayout L;
  if (block_offsets(n, nseg, &L)) return -1;
  GAN_CHECK(off, "jpegdec_block_offsets: null pointer");
  off[0] = L.off_seg; off[1] = L.off_dht; off[2] = L.off_qt; off[3] = L.off_scan;
  return 0;
}

extern "C" int gan_jpegdec_bounds(gan_jpegdec_image* imgs, int n, int64_t* ws_bytes) {
  DecLayout L;
  if (block_offsets(n, 1, &L)) return -1;
  return jd_place("jpegdec", imgs, n, L.off_coef, ws_bytes);
}

extern "C" int gan_jpegdec_tables(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nseg, void* ws, int64_t ws_bytes, void* stream) {
  DecLayout L;
  if (check_block(blk_dev, blk_host, blk_bytes, n, nseg, ws, ws_bytes, &L)) return -1;
  return jd_launch_tables("jpegdec", (const uint8_t*)blk_dev + L.off_dht, 4 * n, ws, L.off_err, L.back.off_planes, stream);
}

extern "C" int gan_jpegdec_entropy(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nseg, void* ws, int64_t ws_bytes, void* stream) {
  DecLayout L;
  if (check_block(blk_dev, blk_host, blk_bytes, n, nseg, ws, ws_bytes, &L)) return -1;
  hipLaunchKernelGGL(jpegdec_entropy_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)blk_dev, L.off_seg, (const JdTable*)ws, (char*)ws,
                     (int32_t*)((char*)ws + L.off_err));
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_jpegdec_idct(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nseg, void* ws, int64_t ws_bytes, void* stream) {
  DecLayout L;
  if (check_block(blk_dev, blk_host, blk_bytes, n, nseg, ws, ws_bytes, &L)) return -1;
  return jd_launch_idct(blk_dev, n, L.off_qt, ws, L.off_err, L.back.max_blocks, stream);
}

extern "C" int gan_jpegdec_pixels(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nseg, void* ws, int64_t ws_bytes, uint8_t* out,
                                  int64_t out_bytes, int32_t* err, void* stream) {
  DecLayout L;
  if (check_block(blk_dev, blk_host, blk_bytes, n, nseg, ws, ws_bytes, &L)) return -1;
  return jd_launch_pixels("jpegdec", blk_dev, (const gan_jpegdec_image*)blk_host, n, ws, L.off_err, L.back.max_pixels, out, out_bytes, err, stream);
}
