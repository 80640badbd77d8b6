// Stand-alone host run of the decoder's arithmetic (jpegdec_core.h, the text the kernels compile), meant to be built with
// -fsanitize=address,undefined and run over the golden files and their corrupted variants before a GPU sees them:
//   jpegdec_host IN OUT
// IN : int64 [8] = block bytes, images, segments, workspace bytes, output bytes, offsets of segments / dht / qt in the block; then the
//      upload block exactly as dataio.JpegDecoder packs it (descriptors filled by gan_jpegdec_bounds).
// OUT: int32 error word per image, then the output buffer.
// Every buffer is a heap allocation of exactly the size the device gets, so a load or store one byte outside is reported.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "jpegdec_core.h"

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int64_t hd[8];
  if (fread(hd, 8, 8, f) != 8) { fprintf(stderr, "short header\n"); return 2; }
  const int64_t total = hd[0], n = hd[1], nseg = hd[2], ws_bytes = hd[3], out_bytes = hd[4], o_seg = hd[5], o_dht = hd[6], o_qt = hd[7];
  if (total < 1 || n < 1 || nseg < 1 || ws_bytes < 1 || out_bytes < 1) { fprintf(stderr, "bad header\n"); return 2; }
  uint8_t* blk = (uint8_t*)malloc(total);
  if (fread(blk, 1, total, f) != (size_t)total) { fprintf(stderr, "short block\n"); return 2; }
  fclose(f);
  uint8_t* ws = (uint8_t*)calloc(ws_bytes, 1);
  uint8_t* out = (uint8_t*)calloc(out_bytes, 1);
  const gan_jpegdec_image* imgs = (const gan_jpegdec_image*)blk;
  const gan_jpegdec_segment* segs = (const gan_jpegdec_segment*)(blk + o_seg);
  std::vector<JdTable> tabs(4 * n);
  std::vector<int32_t> err(n, 0);
  for (int64_t t = 0; t < 4 * n; ++t) {
    const uint8_t* raw = blk + o_dht + t * 272;
    jd_table_head(raw, &tabs[t]);
    for (int i = 0; i < (1 << JD_LOOK); ++i) jd_table_entry(raw, &tabs[t], i);
  }
  for (int64_t b = 0; b < n; ++b) {
    const gan_jpegdec_image* im = imgs + b;
    int16_t* coef = (int16_t*)(ws + im->coef_off);
    for (int j = 0; j < im->seg_count; ++j) err[b] |= jd_decode_segment(im, segs + im->seg_first + j, j, blk, &tabs[4 * b], jd_zigzag, coef);
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
