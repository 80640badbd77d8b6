// Progressive JPEG decoder on the device, pixel-identical to Image.open(p).convert("RGB") (libjpeg-turbo) for the files
// dataio.parse_jpeg_progressive accepts.  The entropy stage is jpegprog_core.h; everything behind the coefficients is the back end of
// jpegdec.hip (jpegdec_back.h) over a block that begins with the same gan_jpegdec_image descriptors, so this file holds only what is
// progressive: a progressive decode shows jpegdec_tables_kernel, jpegdec_idct_kernel and jpegdec_pixels_kernel in a trace, beside
// jpegprog_entropy_kernel.
//
//   gan_jpegprog_tables  : one wave per DHT version -> decode tables; error words and coefficients zeroed by one memset
//   gan_jpegprog_entropy : one 64-lane workgroup per image; a lane takes one (scan, restart segment); the scans' levels run one after
//                          the other with a barrier between them, the independent scans of a level side by side
//   gan_jpegprog_idct / gan_jpegprog_pixels : the back end's launches
#include "common.h"
#include "jpegprog_core.h"
#include "jpegdec_back.h"

namespace {

constexpr int QT_BYTES = 4 * 64 * 2;
constexpr int LDS_TABLES = 16;                     // table versions of a file held in LDS: 16 x 1424 = 22784 bytes (Pillow's script makes 10, 5 for grey)

struct ProgLayout {
  int64_t off_pimg, off_scan, off_seg, off_dht, off_qt, off_data;      // upload block
  int64_t off_err, off_coef;                                            // workspace; tables at 0
  JdBack back;
};

int64_t up16(int64_t v) { return (v + 15) / 16 * 16; }

int block_offsets(int n, int nscan, int nseg, int nver, ProgLayout* L) {
  GAN_CHECK(n >= 1 && n <= 65535 && nscan >= 1 && nscan <= n * GAN_JPEGPROG_MAX_SCANS && nseg >= 1 && nseg <= (1 << 24) && nver >= 1 &&
                nver <= n * GAN_JPEGPROG_MAX_TABLES,
            "jpegprog: n=%d images, nscan=%d scans, nseg=%d segments, nver=%d table versions outside 1 <= n <= 65535, 1 <= nscan <= %d n, 1 <= nseg <= 2^24, "
            "1 <= nver <= %d n", n, nscan, nseg, nver, GAN_JPEGPROG_MAX_SCANS, GAN_JPEGPROG_MAX_TABLES);
  L->off_pimg = up16((int64_t)n * sizeof(gan_jpegdec_image));
  L->off_scan = L->off_pimg + (int64_t)n * sizeof(gan_jpegprog_image);
  L->off_seg = L->off_scan + (int64_t)nscan * sizeof(gan_jpegprog_scan);
  L->off_dht = L->off_seg + (int64_t)nseg * sizeof(gan_jpegprog_segment);
  L->off_qt = up16(L->off_dht + (int64_t)nver * JD_DHT_BYTES);
  L->off_data = up16(L->off_qt + (int64_t)n * QT_BYTES);
  L->off_err = jd_up256((int64_t)nver * sizeof(JdTable));
  L->off_coef = L->off_err + jd_up256((int64_t)n * 4);
  return 0;
}

// Everything the kernels index with, checked on the host copy of the descriptors.
int check_block(const void* blk_dev, const void* blk_host, int64_t blk_bytes, int n, int nscan, int nseg, int nver, const void* ws, int64_t ws_bytes,
                ProgLayout* L) {
  if (block_offsets(n, nscan, nseg, nver, L)) return -1;
  GAN_CHECK(blk_dev && blk_host && ws, "jpegprog: null pointer");
  GAN_CHECK(blk_bytes >= L->off_data && blk_bytes < (1ll << 31), "jpegprog: block of %lld bytes: %lld are descriptors and tables, and byte offsets are 32-bit",
            (long long)blk_bytes, (long long)L->off_data);
  GAN_CHECK((uintptr_t)blk_dev % 16 == 0 && (uintptr_t)ws % 16 == 0, "jpegprog: block and workspace must be 16-byte aligned");
  const char* h = (const char*)blk_host;
  const gan_jpegdec_image* im = (const gan_jpegdec_image*)h;
  const gan_jpegprog_image* pi = (const gan_jpegprog_image*)(h + L->off_pimg);
  const gan_jpegprog_scan* sc = (const gan_jpegprog_scan*)(h + L->off_scan);
  const gan_jpegprog_segment* sg = (const gan_jpegprog_segment*)(h + L->off_seg);
  if (jd_check_images("jpegprog", im, n, ws_bytes, L->off_coef, &L->back)) return -1;
  for (int i = 0; i < n; ++i) {
    const gan_jpegprog_image& p = pi[i];
    GAN_CHECK(p.scan_count >= 1 && p.scan_count <= GAN_JPEGPROG_MAX_SCANS && p.scan_first >= 0 && (int64_t)p.scan_first + p.scan_count <= nscan,
              "jpegprog: image %d: scans %d .. +%d outside the table of %d, or more than %d scans", i, p.scan_first, p.scan_count, nscan, GAN_JPEGPROG_MAX_SCANS);
    GAN_CHECK(p.ver_count >= 1 && p.ver_count <= GAN_JPEGPROG_MAX_TABLES && p.ver_first >= 0 && (int64_t)p.ver_first + p.ver_count <= nver,
              "jpegprog: image %d: table versions %d .. +%d outside the table of %d, or more than %d versions", i, p.ver_first, p.ver_count, nver,
              GAN_JPEGPROG_MAX_TABLES);
    GAN_CHECK(p.seg_first >= 0 && p.seg_count >= 1 && (int64_t)p.seg_first + p.seg_count <= nseg, "jpegprog: image %d: segments %d .. +%d outside the table of %d",
              i, p.seg_first, p.seg_count, nseg);
    GAN_CHECK(p.nlevel >= 1 && p.nlevel <= p.scan_count, "jpegprog: image %d: %d levels for %d scans", i, p.nlevel, p.scan_count);
    for (int s = 0; s < p.scan_count; ++s) {
      const gan_jpegprog_scan& a = sc[p.scan_first + s];
      GAN_CHECK(a.image == i, "jpegprog: scan %d of image %d names image %d", s, i, a.image);
      GAN_CHECK(a.comp >= -1 && a.comp < im[i].ncomp && !(a.comp < 0 && a.Ss != 0), "jpegprog: scan %d of image %d: component %d (an AC scan holds one component)",
                s, i, a.comp);
      GAN_CHECK((a.Ss == 0 && a.Se == 0) || (a.Ss >= 1 && a.Ss <= a.Se && a.Se <= 63), "jpegprog: scan %d of image %d: band %d .. %d", s, i, a.Ss, a.Se);
      GAN_CHECK(a.Al >= 0 && a.Al <= 13 && (a.Ah == 0 || a.Ah == a.Al + 1), "jpegprog: scan %d of image %d: successive approximation Ah=%d Al=%d", s, i, a.Ah, a.Al);
      for (int c = 0; c < im[i].ncomp; ++c) {
        const bool needs = (a.comp < 0 || a.comp == c) && !(a.Ss == 0 && a.Ah != 0);
        GAN_CHECK(needs ? a.tab[c] >= 0 && a.tab[c] < p.ver_count : a.tab[c] >= -1 && a.tab[c] < p.ver_count,
                  "jpegprog: scan %d of image %d: table version %d of component %d outside the file's %d", s, i, a.tab[c], c, p.ver_count);
      }
      GAN_CHECK(a.dep >= -1 && a.dep < s, "jpegprog: scan %d of image %d: dependency index %d is not an earlier scan", s, i, a.dep);
      GAN_CHECK(a.level >= 0 && a.level < p.nlevel, "jpegprog: scan %d of image %d: level %d outside the image's %d", s, i, a.level, p.nlevel);
      for (int t = 0; t < s; ++t) {                // scans of one level must touch disjoint coefficients: that is what keeps the lanes apart
        const gan_jpegprog_scan& e = sc[p.scan_first + t];
        const bool overlap = (a.comp < 0 || e.comp < 0 || a.comp == e.comp) && a.Ss <= e.Se && e.Ss <= a.Se;
        GAN_CHECK(!overlap || e.level < a.level, "jpegprog: scan %d of image %d (level %d) touches coefficients of the earlier scan %d (level %d): its dependency level is not later",
                  s, i, a.level, t, e.level);
      }
    }
    int level = 0;
    int next_index[GAN_JPEGPROG_MAX_SCANS] = {0}, next_unit[GAN_JPEGPROG_MAX_SCANS] = {0};      // per scan: its segments so far
    for (int j = 0; j < p.seg_count; ++j) {
      const gan_jpegprog_segment& s = sg[p.seg_first + j];
      GAN_CHECK(s.image == i, "jpegprog: segment %d of image %d names image %d", j, i, s.image);
      GAN_CHECK(s.scan >= p.scan_first && s.scan < p.scan_first + p.scan_count, "jpegprog: segment %d of image %d names scan %d, not one of the image's", j, i, s.scan);
      const gan_jpegprog_scan& a = sc[s.scan];
      GAN_CHECK(a.level >= level, "jpegprog: segment %d of image %d: the segments are not ordered by the level of their scan", j, i);
      level = a.level;
      GAN_CHECK(s.index >= 0 && s.unit_first >= 0 && s.unit_count >= 1 && (int64_t)s.unit_first + s.unit_count <= jp_units(&im[i], a.comp),
                "jpegprog: segment %d of image %d: units %d .. +%d outside its scan", j, i, s.unit_first, s.unit_count);
      GAN_CHECK(s.byte_begin >= L->off_data + (s.index > 0 ? 2 : 0) && s.byte_begin <= s.byte_end && s.byte_end <= blk_bytes,
                "jpegprog: segment %d of image %d: bytes %d .. %d outside the block's scan area %lld .. %lld", j, i, s.byte_begin, s.byte_end,
                (long long)L->off_data, (long long)blk_bytes);
      const int k = s.scan - p.scan_first;         // a scan's segments come in order and tile its units: no unit twice, none left out
      GAN_CHECK(s.index == next_index[k] && s.unit_first == next_unit[k], "jpegprog: segment %d of image %d (number %d, from unit %d) does not continue its scan at number %d, unit %d",
                j, i, s.index, s.unit_first, next_index[k], next_unit[k]);
      next_index[k] += 1;
      next_unit[k] += s.unit_count;
    }
    for (int s = 0; s < p.scan_count; ++s)
      GAN_CHECK(next_unit[s] == jp_units(&im[i], sc[p.scan_first + s].comp), "jpegprog: scan %d of image %d: its segments cover %d of its %d units", s, i, next_unit[s],
                jp_units(&im[i], sc[p.scan_first + s].comp));
  }
  return 0;
}

__global__ __launch_bounds__(64) void jpegprog_entropy_kernel(const uint8_t* __restrict__ blk, int64_t off_pimg, int64_t off_scan, int64_t off_seg,
                                                              const JdTable* __restrict__ tabs, char* __restrict__ ws, int32_t* __restrict__ errw) {
  __shared__ JdTable t[LDS_TABLES];
  __shared__ gan_jpegdec_image im;
  __shared__ gan_jpegprog_image pi;
  __shared__ uint8_t zz[64];
  const int b = blockIdx.x;
  zz[threadIdx.x] = jd_zigzag[threadIdx.x];
  {
    const uint32_t* si = reinterpret_cast<const uint32_t*>(blk + (int64_t)b * sizeof(gan_jpegdec_image));
    if (threadIdx.x < (int)(sizeof(gan_jpegdec_image) / 4)) reinterpret_cast<uint32_t*>(&im)[threadIdx.x] = si[threadIdx.x];
    const uint32_t* sp = reinterpret_cast<const uint32_t*>(blk + off_pimg + (int64_t)b * sizeof(gan_jpegprog_image));
    if (threadIdx.x < (int)(sizeof(gan_jpegprog_image) / 4)) reinterpret_cast<uint32_t*>(&pi)[threadIdx.x] = sp[threadIdx.x];
  }
  __syncthreads();
  const JdTable* mine = tabs + pi.ver_first;
  {
    const int held = pi.ver_count < LDS_TABLES ? pi.ver_count : LDS_TABLES;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(mine);
    uint32_t* d = reinterpret_cast<uint32_t*>(t);
    for (int i = threadIdx.x; i < held * (int)(sizeof(JdTable) / 4); i += 64) d[i] = s[i];
  }
  __syncthreads();
  const gan_jpegprog_scan* scans = reinterpret_cast<const gan_jpegprog_scan*>(blk + off_scan);
  const gan_jpegprog_segment* segs = reinterpret_cast<const gan_jpegprog_segment*>(blk + off_seg) + pi.seg_first;
  int16_t* coef = reinterpret_cast<int16_t*>(ws + im.coef_off);
  int err = 0, first = 0;
  for (int level = 0; level < pi.nlevel; ++level) {          // uniform over the workgroup: every lane meets every barrier
    int end = first;
    while (end < pi.seg_count && scans[segs[end].scan].level == level) ++end;
    for (int j = first + threadIdx.x; j < end; j += 64) {
      const gan_jpegprog_segment sg = segs[j];
      const gan_jpegprog_scan sc = scans[sg.scan];
      const JdTable* tab[3];                       // LDS or workspace behind one pointer: the lookups are flat loads either way
#pragma unroll
      for (int c = 0; c < 3; ++c) tab[c] = sc.tab[c] < 0 ? nullptr : sc.tab[c] < LDS_TABLES ? t + sc.tab[c] : mine + sc.tab[c];
      err |= jp_decode_segment(&im, &sc, &sg, blk, tab, zz, coef);
    }
    first = end;
    __syncthreads();                                         // the next level reads what this one stored
  }
  if (err) atomicOr(&errw[b], err);
}

}  // namespace

extern "C" int gan_jpegprog_block_offsets(int n, int nscan, int nseg, int nver, int64_t* off) {
  ProgLayout L;
  if (block_offsets(n, nscan, nseg, nver, &L)) return -1;
  GAN_CHECK(off, "jpegprog_block_offsets: null pointer");
  off[0] = L.off_pimg; off[1] = L.off_scan; off[2] = L.off_seg; off[3] = L.off_dht; off[4] = L.off_qt; off[5] = L.off_data;
  return 0;
}

extern "C" int gan_jpegprog_bounds(gan_jpegdec_image* imgs, int n, int nver, int64_t* ws_bytes) {
  ProgLayout L;
  if (block_offsets(n, 1, 1, nver, &L)) return -1;
  return jd_place("jpegprog", imgs, n, L.off_coef, ws_bytes);
}

#define PROG_ARGS const void *blk_dev, const void *blk_host, int64_t blk_bytes, int n, int nscan, int nseg, int nver, void *ws, int64_t ws_bytes
#define PROG_CHECK()  \
  ProgLayout L;       \
  if (check_block(blk_dev, blk_host, blk_bytes, n, nscan, nseg, nver, ws, ws_bytes, &L)) return -1

extern "C" int gan_jpegprog_tables(PROG_ARGS, void* stream) {
  PROG_CHECK();
  return jd_launch_tables("jpegprog", (const uint8_t*)blk_dev + L.off_dht, nver, ws, L.off_err, L.back.off_planes, stream);
}

extern "C" int gan_jpegprog_entropy(PROG_ARGS, void* stream) {
  PROG_CHECK();
  hipLaunchKernelGGL(jpegprog_entropy_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)blk_dev, L.off_pimg, L.off_scan, L.off_seg,
                     (const JdTable*)ws, (char*)ws, (int32_t*)((char*)ws + L.off_err));
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_jpegprog_idct(PROG_ARGS, void* stream) {
  PROG_CHECK();
  return jd_launch_idct(blk_dev, n, L.off_qt, ws, L.off_err, L.back.max_blocks, stream);
}

extern "C" int gan_jpegprog_pixels(PROG_ARGS, uint8_t* out, int64_t out_bytes, int32_t* err, void* stream) {
  PROG_CHECK();
  return jd_launch_pixels("jpegprog", blk_dev, (const gan_jpegdec_image*)blk_host, n, ws, L.off_err, L.back.max_pixels, out, out_bytes, err, stream);
}
