// The entropy stage of the progressive JPEG decoder as plain functions: one restart segment of one scan into the image's coefficients,
// ITU-T T.81 Annex G as libjpeg's jdphuff.c reads it.  jpegprog.hip wraps it in a kernel; jpegprog_host.cpp includes the same text and
// runs it on the CPU under AddressSanitizer over the golden and the corrupted files, before a GPU sees them.  The bit reader, the
// tables and everything behind the coefficients are jpegdec_core.h's.
// As there: every loop is bounded by a count known before the data is read, every load is clamped to the segment, every store index
// comes from counters and validated descriptors, and an irregularity returns error bits.  Whatever libjpeg would decode with a warning,
// or store somewhere this code does not, is an irregularity: the file then goes to the host decoder.
#pragma once
#include "jpegdec_core.h"

static_assert(sizeof(gan_jpegprog_image) == 32 && sizeof(gan_jpegprog_scan) == 64 && sizeof(gan_jpegprog_segment) == 32, "descriptor layout");

// The real (unpadded) block grid of component c: what a single-component scan walks.
struct JpGrid { int bw, bh; };
JD_HD JpGrid jp_grid(const gan_jpegdec_image* im, int c) {
  const int h = c == 0 ? im->hmax : 1, v = c == 0 ? im->vmax : 1;
  const int cw = (im->W * h + im->hmax - 1) / im->hmax, ch = (im->H * v + im->vmax - 1) / im->vmax;
  JpGrid g;
  g.bw = (cw + 7) / 8; g.bh = (ch + 7) / 8;
  return g;
}
// MCUs of an interleaved scan (comp < 0), real blocks of a single-component one: what its restart interval counts.
JD_HD int jp_units(const gan_jpegdec_image* im, int comp) {
  if (comp < 0) return im->mcux * im->mcuy;
  const JpGrid g = jp_grid(im, comp);
  return g.bw * g.bh;
}

JD_FN int jp_bit(JdBits* b) {
  if (b->n < 1) jd_fill(b);
  const int v = (int)jd_peek(b, 1);
  jd_skip(b, 1);
  return v;
}
JD_FN int jp_receive(JdBits* b, int k) {         // 0 <= k <= 15 raw bits
  if (k == 0) return 0;
  const int v = (int)jd_peek(b, k);
  jd_skip(b, k);
  return v;
}
JD_FN bool jp_int16(int v) { return v >= -32768 && v <= 32767; }

// first DC scan: the difference to the predictor, stored shifted
JD_FN void jp_dc_first(JdBits* b, const JdTable* t, int* pred, int Al, int16_t* blk) {
  if (b->n < 32) jd_fill(b);
  const int s = jd_symbol(b, t);
  if (s > 15) b->err |= GAN_JPEGDEC_ERR_CODE;
  if (b->err) return;
  *pred += jd_extend(b, s);
  if (!jp_int16(*pred)) b->err |= GAN_JPEGDEC_ERR_DC;
  if (b->err) return;
  const int v = *pred * (1 << Al);
  if (!jp_int16(v)) { b->err |= GAN_JPEGPROG_ERR_COEF; return; }
  blk[0] = (int16_t)v;
}

// the correction bit of an already-nonzero coefficient
JD_FN void jp_correct(JdBits* b, int16_t* t, int p1) {
  if (!jp_bit(b)) return;
  const int c = *t;
  if ((c & p1) != 0) return;
  const int v = c >= 0 ? c + p1 : c - p1;
  if (!jp_int16(v)) { b->err |= GAN_JPEGPROG_ERR_COEF; return; }
  *t = (int16_t)v;
}

// first AC scan of one block
JD_FN void jp_ac_first(JdBits* b, const JdTable* t, int Ss, int Se, int Al, int* eobrun, const uint8_t* zz, int16_t* blk) {
  if (*eobrun > 0) { --*eobrun; return; }
  for (int k = Ss; k <= Se; ++k) {
    if (b->n < 32) jd_fill(b);
    const int rs = jd_symbol(b, t), r = rs >> 4, s = rs & 15;
    if (b->err) return;
    if (s) {
      k += r;
      if (k > Se) { b->err |= GAN_JPEGDEC_ERR_RUN; return; }
      const int v = jd_extend(b, s) * (1 << Al);
      if (b->err) return;
      if (!jp_int16(v)) { b->err |= GAN_JPEGPROG_ERR_COEF; return; }
      blk[zz[k]] = (int16_t)v;
    } else if (r == 15) {
      k += 15;                                   // ZRL; past Se it only ends the block, as in libjpeg
    } else {
      *eobrun = (1 << r) + jp_receive(b, r) - 1; // this block is the run's first
      return;
    }
  }
}

// AC refinement of one block
JD_FN void jp_ac_refine(JdBits* b, const JdTable* t, int Ss, int Se, int Al, int* eobrun, const uint8_t* zz, int16_t* blk) {
  const int p1 = 1 << Al;
  int k = Ss;
  if (*eobrun == 0) {
    for (; k <= Se; ++k) {
      if (b->n < 32) jd_fill(b);
      const int rs = jd_symbol(b, t), s = rs & 15;
      int r = rs >> 4, nv = 0;
      if (b->err) return;
      if (s) {
        if (s != 1) { b->err |= GAN_JPEGPROG_ERR_REFINE; return; }
        nv = jp_bit(b) ? p1 : -p1;
      } else if (r != 15) {
        *eobrun = (1 << r) + jp_receive(b, r);   // the rest of this block belongs to the run
        break;
      }
      do {                                       // over the nonzero coefficients (a correction bit each) and r zero ones
        int16_t* c = blk + zz[k];
        if (*c != 0) jp_correct(b, c, p1);
        else if (--r < 0) break;
        ++k;
      } while (k <= Se);
      if (b->err) return;
      if (nv) {
        if (k > Se) { b->err |= GAN_JPEGDEC_ERR_RUN; return; }      // libjpeg would store it past the band without a word
        blk[zz[k]] = (int16_t)nv;
      }
    }
    if (b->err) return;
  }
  if (*eobrun > 0) {
    for (; k <= Se; ++k) {
      int16_t* c = blk + zz[k];
      if (*c != 0) jp_correct(b, c, p1);
    }
    --*eobrun;
  }
}

// ---- one restart segment of scan `sc` into the image's coefficients (zeroed before the first scan).  tab[c]: the decode table of
// component c in this scan, or null.  zz: jd_zigzag, or a copy of it in faster memory.
JD_FN int jp_decode_segment(const gan_jpegdec_image* im, const gan_jpegprog_scan* sc, const gan_jpegprog_segment* sg, const uint8_t* data,
                            const JdTable* const* tab, const uint8_t* zz, int16_t* coef) {
  JdBits b;
  jd_open(&b, data, sg->byte_begin, sg->byte_end);
  if (sg->index > 0 && (data[sg->byte_begin - 2] != 0xFF || data[sg->byte_begin - 1] != 0xD0 + ((sg->index - 1) & 7))) return GAN_JPEGDEC_ERR_RST;
  const int Ss = sc->Ss, Se = sc->Se, Al = sc->Al;
  const bool refine = sc->Ah != 0;
  if (sc->comp < 0) {                            // all components interleaved: DC only, MCU after MCU as in a baseline scan
    int pred[3] = {0, 0, 0};
    for (int m = 0; m < sg->unit_count; ++m) {
      const int mcu = sg->unit_first + m, my = mcu / im->mcux, mx = mcu - my * im->mcux;
      for (int c = 0; c < im->ncomp; ++c) {
        const JdComp cp = jd_comp(im, c);
        for (int u = 0; u < cp.h * cp.v; ++u) {
          const int v = u / cp.h, h = u - v * cp.h;
          int16_t* blk = coef + (int64_t)(cp.first + (my * cp.v + v) * cp.bw + mx * cp.h + h) * 64;
          if (refine) { if (jp_bit(&b)) blk[0] = (int16_t)(blk[0] | (1 << Al)); }
          else jp_dc_first(&b, tab[c], &pred[c], Al, blk);
          if (b.err) return b.err;
        }
      }
    }
  } else {                                       // one component: its real blocks in raster order, stored at the padded stride
    const int c = sc->comp;
    const JdComp cp = jd_comp(im, c);
    const JpGrid g = jp_grid(im, c);
    int pred = 0, eobrun = 0;
    for (int m = 0; m < sg->unit_count; ++m) {
      const int n = sg->unit_first + m, by = n / g.bw, bx = n - by * g.bw;
      int16_t* blk = coef + (int64_t)(cp.first + by * cp.bw + bx) * 64;
      if (Ss == 0) {
        if (refine) { if (jp_bit(&b)) blk[0] = (int16_t)(blk[0] | (1 << Al)); }
        else jp_dc_first(&b, tab[c], &pred, Al, blk);
      } else if (refine) {
        jp_ac_refine(&b, tab[c], Ss, Se, Al, &eobrun, zz, blk);
      } else {
        jp_ac_first(&b, tab[c], Ss, Se, Al, &eobrun, zz, blk);
      }
      if (b.err) return b.err;
    }
    if (eobrun > 0) return b.err | GAN_JPEGPROG_ERR_EOBRUN;
  }
  jd_fill(&b);
  if (b.pos < b.end || b.n >= 8) b.err |= GAN_JPEGDEC_ERR_LEFT;
  return b.err;
}
