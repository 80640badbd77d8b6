// Stand-alone host run of the progressive decoder's arithmetic (jpegprog_core.h and jpegdec_core.h, the text the kernels compile), meant
// to be built with -fsanitize=address,undefined and run over the golden files and their corrupted variants before a GPU sees them:
//   jpegprog_host IN OUT
// IN : int64 [12] = block bytes, images, scans, segments, table versions, workspace bytes, output bytes, offsets of the progressive image
//      descriptors / scans / segments / dht / qt in the block; then the upload block exactly as dataio.JpegDecoder packs it.
// OUT: int32 error word per image, then the output buffer.
// Every buffer is a heap allocation of exactly the size the device gets, so a load or store one byte outside is reported.  The scans
// run in file order, which is one of the orders the device's levels allow.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "jpegprog_core.h"

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int64_t hd[12];
  if (fread(hd, 8, 12, f) != 12) { fprintf(stderr, "short header\n"); return 2; }
  const int64_t total = hd[0], n = hd[1], nscan = hd[2], nseg = hd[3], nver = hd[4], ws_bytes = hd[5], out_bytes = hd[6];
  const int64_t o_pimg = hd[7], o_scan = hd[8], o_seg = hd[9], o_dht = hd[10], o_qt = hd[11];
  if (total < 1 || n < 1 || nscan < 1 || nseg < 1 || nver < 1 || ws_bytes < 1 || out_bytes < 1) { fprintf(stderr, "bad header\n"); return 2; }
  uint8_t* blk = (uint8_t*)malloc(total);
  if (fread(blk, 1, total, f) != (size_t)total) { fprintf(stderr, "short block\n"); return 2; }
  fclose(f);
  uint8_t* ws = (uint8_t*)calloc(ws_bytes, 1);
  uint8_t* out = (uint8_t*)calloc(out_bytes, 1);
  const gan_jpegdec_image* imgs = (const gan_jpegdec_image*)blk;
  const gan_jpegprog_image* pimgs = (const gan_jpegprog_image*)(blk + o_pimg);
  const gan_jpegprog_scan* scans = (const gan_jpegprog_scan*)(blk + o_scan);
  const gan_jpegprog_segment* segs = (const gan_jpegprog_segment*)(blk + o_seg);
  std::vector<JdTable> tabs(nver);
  std::vector<int32_t> err(n, 0);
  for (int64_t t = 0; t < nver; ++t) {
    const uint8_t* raw = blk + o_dht + t * 272;
    jd_table_head(raw, &tabs[t]);
    for (int i = 0; i < (1 << JD_LOOK); ++i) jd_table_entry(raw, &tabs[t], i);
  }
  for (int64_t b = 0; b < n; ++b) {
    const gan_jpegdec_image* im = imgs + b;
    const gan_jpegprog_image* pi = pimgs + b;
    int16_t* coef = (int16_t*)(ws + im->coef_off);
    for (int s = 0; s < pi->scan_count; ++s) {
      const gan_jpegprog_scan* sc = scans + pi->scan_first + s;
      const JdTable* tab[3];
      for (int c = 0; c < 3; ++c) tab[c] = sc->tab[c] < 0 ? nullptr : &tabs[pi->ver_first + sc->tab[c]];
      for (int j = 0; j < pi->seg_count; ++j) {
        const gan_jpegprog_segment* sg = segs + pi->seg_first + j;
        if (sg->scan == pi->scan_first + s) err[b] |= jp_decode_segment(im, sc, sg, blk, tab, jd_zigzag, coef);
      }
    }
    err[b] |= jd_host_back(im, (const uint16_t*)(blk + o_qt) + b * 4 * 64, ws, out);
  }
  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  fwrite(err.data(), 4, n, f);
  fwrite(out, 1, out_bytes, f);
  fclose(f);
  free(blk); free(ws); free(out);
  return 0;
}
