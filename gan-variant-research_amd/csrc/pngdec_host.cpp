// Stand-alone host run of the PNG decoder's arithmetic (pngdec_core.h, the text the kernels compile), meant to be built with
// -fsanitize=address,undefined and run over the golden files and their corrupted variants before a GPU sees them:
//   pngdec_host IN OUT
// IN : int64 [5] = block bytes, files, workspace bytes, output bytes, offset of the palettes in the block; then the upload block
//      exactly as dataio.PngDecoder packs it (descriptors filled by gan_pngdec_bounds).
// OUT: int32 error word per file, then the output buffer.
// Every buffer is a heap allocation of exactly the size the device gets, so a load or store one byte outside is reported.  The
// functions run with one lane, which takes every lane's share of the work in turn.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pngdec_core.h"

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int64_t hd[5];
  if (fread(hd, 8, 5, f) != 5) { fprintf(stderr, "short header\n"); return 2; }
  const int64_t total = hd[0], n = hd[1], ws_bytes = hd[2], out_bytes = hd[3], o_pal = hd[4];
  if (total < 1 || n < 1 || ws_bytes < 1 || out_bytes < 1) { fprintf(stderr, "bad header\n"); return 2; }
  uint8_t* blk = (uint8_t*)malloc(total);
  if (fread(blk, 1, total, f) != (size_t)total) { fprintf(stderr, "short block\n"); return 2; }
  fclose(f);
  uint8_t* ws = (uint8_t*)calloc(ws_bytes, 1);
  uint8_t* out = (uint8_t*)calloc(out_bytes, 1);
  const gan_pngdec_image* imgs = (const gan_pngdec_image*)blk;
  std::vector<int32_t> err(n, 0);
  PdInflate* I = (PdInflate*)calloc(1, sizeof(PdInflate));
  PdRows* R = (PdRows*)calloc(1, sizeof(PdRows));
  for (int64_t b = 0; b < n; ++b) {
    const gan_pngdec_image* im = imgs + b;
    err[b] = pd_inflate(im, blk, I, ws + im->raw_off, 0, 1);
    if (err[b] == 0) err[b] = pd_pixels(im, blk, o_pal + b * 768, ws + im->raw_off, R, out + im->out_off, 0, 1);
  }
  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  fwrite(err.data(), 4, n, f);
  fwrite(out, 1, out_bytes, f);
  fclose(f);
  free(blk); free(ws); free(out); free(I); free(R);
  return 0;
}
