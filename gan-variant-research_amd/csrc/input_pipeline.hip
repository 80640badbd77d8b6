// Device-side input pipeline: decoded uint8 RGB images -> the (B,3,S,S) fp32 batch in [-1,1] the trainers consume.
//
// Replaces, per image, the PIL chain the reference's datasets run on CPU workers
//   GAN_Variant1/dataio/transforms.py:10-49   RandomCropResize (crop + BICUBIC resize), RandomHorizontalFlip,
//                                             ColorJitter(0.05, 0.05, 0.05, 0.02), ToTensor, Normalize(0.5, 0.5); eval: Resize
//   Basic_GAN/src/data.py:8-26                Resize(load_size, BICUBIC), RandomCrop / CenterCrop, flip, ToTensor, Normalize
// bit for bit: Pillow's resize is integer (22-bit fixed-point taps, uint8 between the two passes), its ImageEnhance blends are
// float32 with truncation, its RGB<->HSV conversions mix float32 variables with double constants.  The arithmetic below follows
// Pillow 12.2 operation by operation (oracle/input_ref.py is the numpy restatement, pinned against Pillow itself), so floating-point
// contraction is off for this file and every rounding is the one the C code performs.
// All kernels are HBM-/latency-bound byte work: one pixel per lane, one image per blockIdx.y.
// The same file holds the other end of inference: view_to_u8_hwc_kernel turns the generator's last activation into the packed uint8
// HWC image PIL encodes (four pixels per lane), held to torch's float32 operation order for the same reason.
#include "common.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Pillow 12.2 Image.resize makes the vertical pass first when the source is more than 100 times taller than wide and the target is
// lower than the source (`size[1] > size[0] * 100 and new_height < size[1]`, either filter).  The bytes between the passes are rounded,
// so the order shows in the result.
__device__ __forceinline__ bool vertical_first(const gan_input_job& j) { return j.crop_h > (int64_t)100 * j.crop_w && j.res_h < j.crop_h; }

// ---- first pass, horizontal: source rows of the crop box -> tmp [B][tmp_rows][S][4] (uint8 RGBX), only the window's columns
__global__ __launch_bounds__(256) void input_resize_h_kernel(const gan_input_job* __restrict__ jobs, const int32_t* __restrict__ tables,
                                                             uint8_t* __restrict__ tmp, int tmp_rows, int S) {
  const gan_input_job j = jobs[blockIdx.y];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (vertical_first(j)) {              // the vertical pass comes first: the window's rows of every crop column -> tmp [S][crop_w]
    if (idx >= S * j.crop_w) return;    // crop_w < crop_h / 100 <= tmp_rows: fits the image's tmp_rows * S pixels
    const int y = idx / j.crop_w, x = idx - y * j.crop_w;
    const int32_t* b = tables + j.vb_off + 2 * (j.win_y + y);
    const int32_t* k = tables + j.vk_off + (int64_t)(j.win_y + y) * j.vksize;
    const int ymin = b[0], n = b[1];
    const uint8_t* col = j.src + (int64_t)(j.crop_y + ymin) * j.src_stride + (int64_t)(j.crop_x + x) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < n; ++t) {
      const int w = k[t];
      const uint8_t* p = col + (int64_t)t * j.src_stride;
      s0 += p[0] * w; s1 += p[1] * w; s2 += p[2] * w;
    }
    uchar4 o = make_uchar4((unsigned char)clip8(s0 >> PRECISION_BITS), (unsigned char)clip8(s1 >> PRECISION_BITS), (unsigned char)clip8(s2 >> PRECISION_BITS), 255);
    reinterpret_cast<uchar4*>(tmp)[(int64_t)blockIdx.y * tmp_rows * S + idx] = o;
    return;
  }
  if (idx >= j.crop_h * S) return;
  const int y = idx / S, x = idx - y * S;
  const int32_t* b = tables + j.hb_off + 2 * (j.win_x + x);
  const int32_t* k = tables + j.hk_off + (int64_t)(j.win_x + x) * j.hksize;
  const int xmin = b[0], n = b[1];
  const uint8_t* row = j.src + (int64_t)(j.crop_y + y) * j.src_stride + (int64_t)(j.crop_x + xmin) * 3;
  int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < n; ++t) {
    const int w = k[t];
    s0 += row[3 * t] * w; s1 += row[3 * t + 1] * w; s2 += row[3 * t + 2] * w;
  }
  uchar4 o = make_uchar4((unsigned char)clip8(s0 >> PRECISION_BITS), (unsigned char)clip8(s1 >> PRECISION_BITS), (unsigned char)clip8(s2 >> PRECISION_BITS), 255);
  reinterpret_cast<uchar4*>(tmp)[((int64_t)blockIdx.y * tmp_rows + y) * S + x] = o;
}

// ---- second pass, vertical: tmp -> img [B][S][S][4], only the window's rows
__global__ __launch_bounds__(256) void input_resize_v_kernel(const gan_input_job* __restrict__ jobs, const int32_t* __restrict__ tables,
                                                             const uint8_t* __restrict__ tmp, int tmp_rows, int S, uint8_t* __restrict__ img) {
  const gan_input_job j = jobs[blockIdx.y];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= S * S) return;
  const int y = idx / S, x = idx - y * S;
  if (vertical_first(j)) {              // tmp holds the vertical pass [S][crop_w]: this is the horizontal one
    const int32_t* b = tables + j.hb_off + 2 * (j.win_x + x);
    const int32_t* k = tables + j.hk_off + (int64_t)(j.win_x + x) * j.hksize;
    const int xmin = b[0], n = b[1];
    const uchar4* row = reinterpret_cast<const uchar4*>(tmp) + (int64_t)blockIdx.y * tmp_rows * S + (int64_t)y * j.crop_w + xmin;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < n; ++t) {
      const int w = k[t];
      const uchar4 p = row[t];
      s0 += p.x * w; s1 += p.y * w; s2 += p.z * w;
    }
    uchar4 o = make_uchar4((unsigned char)clip8(s0 >> PRECISION_BITS), (unsigned char)clip8(s1 >> PRECISION_BITS), (unsigned char)clip8(s2 >> PRECISION_BITS), 255);
    reinterpret_cast<uchar4*>(img)[((int64_t)blockIdx.y * S + y) * S + x] = o;
    return;
  }
  const int32_t* b = tables + j.vb_off + 2 * (j.win_y + y);
  const int32_t* k = tables + j.vk_off + (int64_t)(j.win_y + y) * j.vksize;
  const int ymin = b[0], n = b[1];
  const uchar4* col = reinterpret_cast<const uchar4*>(tmp) + ((int64_t)blockIdx.y * tmp_rows + ymin) * S + x;
  int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < n; ++t) {
    const int w = k[t];
    const uchar4 p = col[(int64_t)t * S];
    s0 += p.x * w; s1 += p.y * w; s2 += p.z * w;
  }
  uchar4 o = make_uchar4((unsigned char)clip8(s0 >> PRECISION_BITS), (unsigned char)clip8(s1 >> PRECISION_BITS), (unsigned char)clip8(s2 >> PRECISION_BITS), 255);
  reinterpret_cast<uchar4*>(img)[((int64_t)blockIdx.y * S + y) * S + x] = o;
}

// Convert.c rgb2l
__device__ __forceinline__ int luma(uchar4 p) { return (p.x * 19595 + p.y * 38470 + p.z * 7471 + 0x8000) >> 16; }

// ---- per-image grey mean of the current image state: int(sum / n + 0.5) (ImageEnhance.Contrast); one block per image
__global__ __launch_bounds__(1024) void input_gray_mean_kernel(const uint8_t* __restrict__ img, int S, int32_t* __restrict__ mean) {
  __shared__ unsigned long long sh[16];
  const uchar4* p = reinterpret_cast<const uchar4*>(img) + (int64_t)blockIdx.x * S * S;
  unsigned long long s = 0;
  for (int i = threadIdx.x; i < S * S; i += 1024) s += (unsigned)luma(p[i]);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int i = 0; i < 16; ++i) t += sh[i];
    const unsigned long long n = (unsigned long long)S * S;
    mean[blockIdx.x] = (int32_t)((2 * t + n) / (2 * n));       // == int(t / n + 0.5): the quotient is never within 1/(2n) of a half below it
  }
}

// Blend.c ImagingBlend: float32 in1 + alpha * (in2 - in1); alpha in [0,1] truncates, otherwise clip first
__device__ __forceinline__ int blend1(int in1, int in2, float alpha, bool inside) {
  // Two roundings, as the C code's: plain operators, so that this file's `fp contract(off)` governs them.  __fmul_rn and __fadd_rn
  // are header inlines compiled under the default contraction: a pair of them fuses into one v_fma_f32 (one rounding), which changes
  // bytes for factors next to a fraction k / (in2 - in1), 1 + 2^-23 among them.
  const float prod = alpha * (float)(in2 - in1);
  const float t = (float)in1 + prod;
  if (inside) return (int)t & 255;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// Convert.c rgb2hsv_row / hsv2rgb with the H channel shifted in between (torchvision _functional_pil.adjust_hue)
__device__ __forceinline__ uchar4 hue_rotate(uchar4 px, int shift) {
  const int r = px.x, g = px.y, b = px.z;
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  int uh = 0, us = 0;
  const int uv = maxc;
  if (minc != maxc) {
    const float cr = (float)(maxc - minc);
    const float s = __fdiv_rn(cr, (float)maxc);
    const float rc = __fdiv_rn((float)(maxc - r), cr), gc = __fdiv_rn((float)(maxc - g), cr), bc = __fdiv_rn((float)(maxc - b), cr);
    float h;
    if (r == maxc) h = __fsub_rn(bc, gc);
    else if (g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
    else h = (float)((4.0 + (double)gc) - (double)rc);
    const double t = (double)h / 6.0 + 1.0;
    h = (float)(t - trunc(t));                                   // fmod(t, 1.0), t > 0
    uh = clip8((int)((double)h * 255.0));
    us = clip8((int)((double)s * 255.0));
  }
  uh = (uh + shift) & 255;
  if (us == 0) return make_uchar4((unsigned char)uv, (unsigned char)uv, (unsigned char)uv, px.w);
  const double hf = (double)(float)uh * 6.0 / 255.0;
  const int i = (int)floor(hf);
  const double f = (double)(float)(hf - (double)(float)i);
  const double fs = (double)(float)((double)(float)us / 255.0);
  const double vf = (double)(float)uv;
  const int p = clip8((int)round(vf * (1.0 - fs)));
  const int q = clip8((int)round(vf * (1.0 - fs * f)));
  const int t2 = clip8((int)round(vf * (1.0 - fs * (1.0 - f))));
  int R, G, B;
  switch (i % 6) {
    case 0: R = uv; G = t2; B = p; break;
    case 1: R = q; G = uv; B = p; break;
    case 2: R = p; G = uv; B = t2; break;
    case 3: R = p; G = q; B = uv; break;
    case 4: R = t2; G = p; B = uv; break;
    default: R = uv; G = p; B = q; break;
  }
  return make_uchar4((unsigned char)R, (unsigned char)G, (unsigned char)B, px.w);
}

// ---- one ColorJitter slot: image b applies its op order[slot] in place
__global__ __launch_bounds__(256) void input_jitter_kernel(const gan_input_job* __restrict__ jobs, uint8_t* __restrict__ img, int S, int slot,
                                                           const int32_t* __restrict__ mean) {
  const gan_input_job& j = jobs[blockIdx.y];
  const int op = j.order[slot];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (op < 0 || idx >= S * S) return;
  uchar4* p = reinterpret_cast<uchar4*>(img) + (int64_t)blockIdx.y * S * S + idx;
  uchar4 v = *p;
  if (op == 3) { *p = hue_rotate(v, j.hue_shift); return; }
  const float a = j.factor[op];
  const bool inside = a >= 0.f && a <= 1.f;
  int d0, d1, d2;                       // the degenerate image: black, mean grey, own grey
  if (op == 0) d0 = d1 = d2 = 0;
  else if (op == 1) d0 = d1 = d2 = mean[blockIdx.y];
  else d0 = d1 = d2 = luma(v);
  v.x = (unsigned char)blend1(d0, v.x, a, inside);
  v.y = (unsigned char)blend1(d1, v.y, a, inside);
  v.z = (unsigned char)blend1(d2, v.z, a, inside);
  *p = v;
}

// ---- flip + ToTensor + Normalize(0.5, 0.5): img [B][S][S][4] -> out fp32 [B][3][S][S]
__global__ __launch_bounds__(256) void input_finish_kernel(const gan_input_job* __restrict__ jobs, const uint8_t* __restrict__ img, int S, float* __restrict__ out) {
  const int flip = jobs[blockIdx.y].flip;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= S * S) return;
  const int y = idx / S, x = idx - y * S;
  const uchar4 v = reinterpret_cast<const uchar4*>(img)[((int64_t)blockIdx.y * S + y) * S + (flip ? S - 1 - x : x)];
  float* o = out + (int64_t)blockIdx.y * 3 * S * S + idx;
  const int c[3] = {v.x, v.y, v.z};
#pragma unroll
  for (int k = 0; k < 3; ++k) o[(int64_t)k * S * S] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)c[k], 255.f), 0.5f), 0.5f);
}

// ---- the same flip, no normalisation: img [B][S][S][4] -> out uint8 [B][3][S][S] (what a feature extractor takes)
__global__ __launch_bounds__(256) void input_finish_u8_kernel(const gan_input_job* __restrict__ jobs, const uint8_t* __restrict__ img, int S, uint8_t* __restrict__ out) {
  const int flip = jobs[blockIdx.y].flip;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= S * S) return;
  const int y = idx / S, x = idx - y * S;
  const uchar4 v = reinterpret_cast<const uchar4*>(img)[((int64_t)blockIdx.y * S + y) * S + (flip ? S - 1 - x : x)];
  uint8_t* o = out + (int64_t)blockIdx.y * 3 * S * S + idx;
  o[0] = v.x; o[(int64_t)S * S] = v.y; o[(int64_t)2 * S * S] = v.z;
}

// ---- output epilogue: view interior -> packed [B][H][W][C] uint8, the reference's _to_uint8 (generate_folder.py:183-185) fused with the
// NCHW -> HWC turn PIL needs.  Each lane takes a run of four pixels of one row: four 16-byte loads issued back to back (a whole bf16
// pixel of 8 channels, or the first four fp32 channels; C <= 4, so nothing past them is needed), then PACKED (C == 3, W % 4 == 0, dst
// four-byte aligned: every run starts on a dword) twelve bytes as three dword stores, otherwise byte stores with a row tail.
__device__ __forceinline__ uint32_t unit_to_u8(float v) {
  if (!(v >= -1.f)) v = -1.f;            // clamp(-1, 1); a NaN takes this branch and becomes byte 0
  if (v > 1.f) v = 1.f;
  const float unit = v * 0.5f + 0.5f;     // plain operators under this file's contract(off) (v * 0.5 is exact: one rounding either way)
  return (uint32_t)rintf(unit * 255.f);   // rintf: half to even, as torch.round
}

template <typename T, bool PACKED>
__global__ __launch_bounds__(256) void view_to_u8_hwc_kernel(DView src, int C, uint8_t* __restrict__ dst) {
  const int gw = (src.W + 3) >> 2;
  const int64_t total = (int64_t)src.B * src.H * gw;
  const T* sp = reinterpret_cast<const T*>(src.ptr);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int g = (int)(i % gw);
    const int64_t r = i / gw;
    const int y = (int)(r % src.H), b = (int)(r / src.H);
    const int x = 4 * g;
    const int n = PACKED ? 4 : min(4, src.W - x);
    const T* p = sp + src.pix(b, y, x);
    Raw<T> raw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) raw[k] = ldraw<T>(p + (int64_t)(k < n ? k : 0) * src.C);     // a tail lane re-reads its first pixel: no load past the row
    uint32_t q[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float v[Chunk<T>::N];
      cvtraw<T>(raw[k], v);
#pragma unroll
      for (int c = 0; c < 4; ++c) q[k][c] = unit_to_u8(v[c]);
    }
    uint8_t* o = dst + (((int64_t)b * src.H + y) * src.W + x) * C;
    if (PACKED) {
      uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
      o4[0] = q[0][0] | (q[0][1] << 8) | (q[0][2] << 16) | (q[1][0] << 24);
      o4[1] = q[1][1] | (q[1][2] << 8) | (q[2][0] << 16) | (q[2][1] << 24);
      o4[2] = q[2][2] | (q[3][0] << 8) | (q[3][1] << 16) | (q[3][2] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (k < n && c < C) o[k * C + c] = (uint8_t)q[k][c];
      }
    }
  }
}
}  // namespace

// ---- host: Pillow's taps (Resample.c precompute_coeffs + normalize_coeffs_8bpc), double arithmetic, no GPU involved.  The filter ids
// are Pillow's (Image.BILINEAR = 2, Image.BICUBIC = 3); each filter is its Resample.c function and support.
static double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}

static double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

struct ResizeFilter { double (*fn)(double); double support; };
static bool resize_filter(int filter, ResizeFilter* f) {
  if (filter == GAN_RESIZE_BILINEAR) { f->fn = bilinear_filter; f->support = 1.0; return true; }
  if (filter == GAN_RESIZE_BICUBIC) { f->fn = bicubic_filter; f->support = 2.0; return true; }
  return false;
}

extern "C" int gan_resize_ksize_filter(int in_size, int out_size, int filter) {
  ResizeFilter f;
  if (!resize_filter(filter, &f)) return gan_set_error(-1, "resize_ksize: unknown filter %d (BILINEAR = 2, BICUBIC = 3)", filter);
  if (in_size <= 0 || out_size <= 0) return gan_set_error(-1, "resize_ksize: sizes must be positive (%d -> %d)", in_size, out_size);
  double filterscale = (double)in_size / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  return (int)ceil(f.support * filterscale) * 2 + 1;
}

extern "C" int gan_resize_coeffs_filter(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk, int ksize) {
  ResizeFilter f;
  GAN_CHECK(resize_filter(filter, &f), "resize_coeffs: unknown filter %d (BILINEAR = 2, BICUBIC = 3)", filter);
  GAN_CHECK(in_size > 0 && out_size > 0 && bounds && kk, "resize_coeffs: bad arguments (%d -> %d)", in_size, out_size);
  GAN_CHECK(ksize == gan_resize_ksize_filter(in_size, out_size, filter), "resize_coeffs: ksize must be gan_resize_ksize(in, out) = %d, got %d",
            gan_resize_ksize_filter(in_size, out_size, filter), ksize);
  const double in0 = 0.0, in1 = (double)in_size;
  double scale = (in1 - in0) / out_size, filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = f.support * filterscale, ss = 1.0 / filterscale;
  double w[1024];
  GAN_CHECK(ksize <= 1024, "resize_coeffs: downscale factor too large (ksize %d)", ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = in0 + (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) { w[x] = f.fn((x + xmin - center + 0.5) * ss); ww += w[x]; }
    int32_t* k = kk + (int64_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
      if (x >= xmax) { k[x] = 0; continue; }
      const double p = ww != 0.0 ? w[x] / ww : w[x];
      k[x] = p < 0 ? (int32_t)(-0.5 + p * (1 << PRECISION_BITS)) : (int32_t)(0.5 + p * (1 << PRECISION_BITS));
    }
    bounds[2 * xx] = xmin; bounds[2 * xx + 1] = xmax;
  }
  return 0;
}

extern "C" int gan_resize_ksize(int in_size, int out_size) { return gan_resize_ksize_filter(in_size, out_size, GAN_RESIZE_BICUBIC); }

extern "C" int gan_resize_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* kk, int ksize) {
  return gan_resize_coeffs_filter(in_size, out_size, GAN_RESIZE_BICUBIC, bounds, kk, ksize);
}

// The launch sequence of both entries below: `out` (fp32, normalised) or `out_u8` (the bytes), whichever is given.
static int input_pipeline_launch(const gan_input_job* jobs_dev, const gan_input_job* jobs_host, int B, const int32_t* tables_dev, int S,
                                 int filter, uint8_t* tmp, int tmp_rows, uint8_t* img, int32_t* mean_ws, float* out, uint8_t* out_u8, void* stream) {
  GAN_CHECK(filter == GAN_RESIZE_BILINEAR || filter == GAN_RESIZE_BICUBIC, "input_pipeline: unknown filter %d (BILINEAR = 2, BICUBIC = 3)", filter);
  GAN_CHECK(jobs_dev && jobs_host && tables_dev && tmp && img && mean_ws && (out || out_u8) && B > 0 && S > 0, "input_pipeline: null pointer or empty batch");
  int max_rows = 0;
  bool slot_used[4] = {false, false, false, false}, slot_mean[4] = {false, false, false, false};
  for (int b = 0; b < B; ++b) {
    const gan_input_job& j = jobs_host[b];
    GAN_CHECK(j.src && j.crop_h > 0 && j.crop_w > 0 && j.crop_y >= 0 && j.crop_x >= 0 && j.src_stride >= 3 * (j.crop_x + j.crop_w),
              "input_pipeline: image %d: crop box (%d,%d,%d,%d) outside a row of %d bytes", b, j.crop_y, j.crop_x, j.crop_h, j.crop_w, j.src_stride);
    GAN_CHECK(j.win_y >= 0 && j.win_x >= 0 && j.win_y + S <= j.res_h && j.win_x + S <= j.res_w,
              "input_pipeline: image %d: %dx%d window at (%d,%d) outside the %dx%d resized image", b, S, S, j.win_y, j.win_x, j.res_h, j.res_w);
    GAN_CHECK(j.hksize == gan_resize_ksize_filter(j.crop_w, j.res_w, filter) && j.vksize == gan_resize_ksize_filter(j.crop_h, j.res_h, filter),
              "input_pipeline: image %d: tap counts do not match its sizes", b);
    GAN_CHECK(j.crop_h <= tmp_rows, "input_pipeline: image %d: %d source rows > tmp_rows %d", b, j.crop_h, tmp_rows);
    if (j.crop_h > max_rows) max_rows = j.crop_h;
    for (int s = 0; s < 4; ++s) {
      GAN_CHECK(j.order[s] >= -1 && j.order[s] <= 3, "input_pipeline: image %d: jitter op %d", b, j.order[s]);
      if (j.order[s] >= 0) slot_used[s] = true;
      if (j.order[s] == 1) slot_mean[s] = true;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(input_resize_h_kernel, dim3((max_rows * S + 255) / 256, B), dim3(256), 0, s, jobs_dev, tables_dev, tmp, tmp_rows, S);
  const int gp = (S * S + 255) / 256;
  hipLaunchKernelGGL(input_resize_v_kernel, dim3(gp, B), dim3(256), 0, s, jobs_dev, tables_dev, tmp, tmp_rows, S, img);
  for (int slot = 0; slot < 4; ++slot) {
    if (!slot_used[slot]) continue;
    if (slot_mean[slot]) hipLaunchKernelGGL(input_gray_mean_kernel, dim3(B), dim3(1024), 0, s, img, S, mean_ws);
    hipLaunchKernelGGL(input_jitter_kernel, dim3(gp, B), dim3(256), 0, s, jobs_dev, img, S, slot, mean_ws);
  }
  if (out) hipLaunchKernelGGL(input_finish_kernel, dim3(gp, B), dim3(256), 0, s, jobs_dev, img, S, out);
  else hipLaunchKernelGGL(input_finish_u8_kernel, dim3(gp, B), dim3(256), 0, s, jobs_dev, img, S, out_u8);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_input_pipeline_filter(const gan_input_job* jobs_dev, const gan_input_job* jobs_host, int B, const int32_t* tables_dev, int S,
                                         int filter, uint8_t* tmp, int tmp_rows, uint8_t* img, int32_t* mean_ws, float* out, void* stream) {
  return input_pipeline_launch(jobs_dev, jobs_host, B, tables_dev, S, filter, tmp, tmp_rows, img, mean_ws, out, nullptr, stream);
}

extern "C" int gan_input_pipeline_u8(const gan_input_job* jobs_dev, const gan_input_job* jobs_host, int B, const int32_t* tables_dev, int S,
                                     int filter, uint8_t* tmp, int tmp_rows, uint8_t* img, int32_t* mean_ws, uint8_t* out, void* stream) {
  return input_pipeline_launch(jobs_dev, jobs_host, B, tables_dev, S, filter, tmp, tmp_rows, img, mean_ws, nullptr, out, stream);
}

extern "C" int gan_input_pipeline(const gan_input_job* jobs_dev, const gan_input_job* jobs_host, int B, const int32_t* tables_dev, int S,
                                  uint8_t* tmp, int tmp_rows, uint8_t* img, int32_t* mean_ws, float* out, void* stream) {
  return gan_input_pipeline_filter(jobs_dev, jobs_host, B, tables_dev, S, GAN_RESIZE_BICUBIC, tmp, tmp_rows, img, mean_ws, out, stream);
}

extern "C" int gan_view_to_u8_hwc(const gan_view* src, int C, uint8_t* dst, void* stream) {
  if (gan_check_view(src, "view_to_u8_hwc.src")) return -1;
  GAN_CHECK(src->dtype == GAN_F32 || src->dtype == GAN_BF16, "view_to_u8_hwc: the view must be fp32 or bf16 (dtype %d)", src->dtype);
  GAN_CHECK(dst && C >= 1 && C <= 4 && C <= src->C, "view_to_u8_hwc: bad C=%d (1 .. 4 channels)", C);
  const int64_t total = (int64_t)src->B * src->H * ((src->W + 3) / 4);
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  const bool packed = C == 3 && src->W % 4 == 0 && (uintptr_t)dst % 4 == 0;
  DView sv = to_dview(src);
  GAN_DISPATCH_DTYPE(src->dtype,
    if (packed) hipLaunchKernelGGL((view_to_u8_hwc_kernel<T, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, sv, C, dst);
    else hipLaunchKernelGGL((view_to_u8_hwc_kernel<T, false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, sv, C, dst);)
  GAN_LAUNCH_CHECK();
  return 0;
}
