// The JPEG decoders' back end: everything behind the coefficient area, defined once in jpegdec.hip and called by the baseline entries
// there and by the progressive ones in jpegprog.hip as ordinary host functions.  Both upload blocks begin with gan_jpegdec_image [n]
// and both workspaces hold decode tables at 0, error words at off_err, then coefficients and, behind every coefficient area, planes.
// `who` is the caller's prefix of the refusal texts, "jpegdec" or "jpegprog".  Internal: not installed, not extern "C".
#pragma once
#include <stdint.h>
#include "../../include/mi355x_gan.h"

struct JdBack {
  int64_t off_planes;                              // the end of the last coefficient area
  int max_blocks, max_pixels;                      // the largest image's 8x8 blocks; its pixels in workgroups of 256
};

int64_t jd_up256(int64_t v);
int jd_check_geometry(const char* who, const gan_jpegdec_image& im, int i);
// Everything the back-end kernels index with, checked on the host copy of the descriptors; coefficients may begin at off_coef.
int jd_check_images(const char* who, const gan_jpegdec_image* im, int n, int64_t ws_bytes, int64_t off_coef, JdBack* B);
// coef_off / plane_off of every image from off_coef on -> *ws_bytes
int jd_place(const char* who, gan_jpegdec_image* imgs, int n, int64_t off_coef, int64_t* ws_bytes);
// ntab raw tables at dht -> decode tables at the head of ws; error words and coefficients (off_err .. off_planes) zeroed by one memset
int jd_launch_tables(const char* who, const uint8_t* dht, int ntab, void* ws, int64_t off_err, int64_t off_planes, void* stream);
int jd_launch_idct(const void* blk_dev, int n, int64_t off_qt, void* ws, int64_t off_err, int max_blocks, void* stream);
int jd_launch_pixels(const char* who, const void* blk_dev, const gan_jpegdec_image* im, int n, const void* ws, int64_t off_err, int max_pixels, uint8_t* out,
                     int64_t out_bytes, int32_t* err, void* stream);
