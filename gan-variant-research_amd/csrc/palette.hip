// Palette prior: low-frequency CIE-Lab statistics of an image batch, their loss against a running prior, and the gradient of that
// loss with respect to the image.
//
// Replaces GAN_Variant1/dataio/transforms.py:52-54 (denormalize), :57-96 (rgb_to_lab) and :99-119 (get_low_freq_stats:
// adaptive_avg_pool2d to T x T, then mean and unbiased std of the T*T cells per image and channel) fused into one pass over the
// image, and the autograd backward of that chain.  The loss that combines them (losses/palette_prior_lab.py) no longer exists in
// the reference: its statement is this project's (DESIGN.md "Palette prior").
//
// The backward differentiates the branch the forward took at every `where` (never 0 * inf: an autograd backward of the reference's
// functions multiplies the infinite derivative of pow(0, 1/3) by the zero of the branch mask), so every gradient is finite for every
// finite input.  Reductions run in a fixed order, fp32 per lane and fp64 across lanes; no atomics: repeated calls repeat their bits.
#include "common.h"

namespace {

struct Lab { float L, a, b; };

// reference constants (transforms.py:69-92); the z row is the reference's 0.0193, 0.1192, 0.9505
#define PAL_XR 0.4124f
#define PAL_XG 0.3576f
#define PAL_XB 0.1805f
#define PAL_YR 0.2126f
#define PAL_YG 0.7152f
#define PAL_YB 0.0722f
#define PAL_ZR 0.0193f
#define PAL_ZG 0.1192f
#define PAL_ZB 0.9505f
#define PAL_WX 0.95047f
#define PAL_WZ 1.08883f
#define PAL_EPS 0.008856f
#define PAL_KAPPA 903.3f

// torch.clamp(v, 0, 1): a NaN stays a NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float pal_clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// sRGB linearisation of v in [0, 1]; *d = derivative of the branch taken
__device__ __forceinline__ float pal_lin(float v, float* d) {
  if (v > 0.04045f) {
    const float u = (v + 0.055f) / 1.055f;           // >= 0.09: u^1.4 = u^2.4 / u
    const float p = powf(u, 2.4f);
    if (d) *d = (2.4f / 1.055f) * (p / u);
    return p;
  }
  if (d) *d = 1.f / 12.92f;
  return v / 12.92f;
}

// f(t) of the Lab transform; *d = derivative of the branch taken (t > 0.008856: f >= 0.2, no division by zero)
__device__ __forceinline__ float pal_f(float t, float* d) {
  if (t > PAL_EPS) {
    const float f = cbrtf(t);
    if (d) *d = 1.f / (3.f * f * f);
    return f;
  }
  if (d) *d = PAL_KAPPA / 116.f;
  return (PAL_KAPPA * t + 16.f) / 116.f;
}

__device__ __forceinline__ Lab pal_lab(float x0, float x1, float x2) {
  const float r = pal_lin(pal_clamp01(x0 * 0.5f + 0.5f), nullptr);
  const float g = pal_lin(pal_clamp01(x1 * 0.5f + 0.5f), nullptr);
  const float b = pal_lin(pal_clamp01(x2 * 0.5f + 0.5f), nullptr);
  const float X = (r * PAL_XR + g * PAL_XG + b * PAL_XB) / PAL_WX;
  const float Y = r * PAL_YR + g * PAL_YG + b * PAL_YB;
  const float Z = (r * PAL_ZR + g * PAL_ZG + b * PAL_ZB) / PAL_WZ;
  const float fx = pal_f(X, nullptr), fy = pal_f(Y, nullptr), fz = pal_f(Z, nullptr);
  Lab o;
  o.L = 116.f * fy - 16.f;
  o.a = 500.f * (fx - fy);
  o.b = 200.f * (fy - fz);
  return o;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block-wide fp64 sum, waves added in order; blockDim.x a multiple of 64, <= 1024; result valid in every thread
__device__ __forceinline__ double block_sum_d(double v, double* sh /* >= 16 doubles */) {
  v = wave_sum_d(v);
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double r = 0.0;
  for (int i = 0; i < nw; ++i) r += sh[i];
  return r;
}

// three block-wide fp64 sums at once (same order as block_sum_d), in place
__device__ __forceinline__ void block_sum_d3(double* v, double (*sh)[16]) {
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = wave_sum_d(v[c]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sh[0][w] = v[0]; sh[1][w] = v[1]; sh[2][w] = v[2]; }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double r = 0.0;
    for (int i = 0; i < nw; ++i) r += sh[c][i];
    v[c] = r;
  }
}

// adaptive_avg_pool2d windows: cell i of T over n pixels covers [floor(i n / T), ceil((i + 1) n / T))
__device__ __forceinline__ int cell_lo(int i, int n, int T) { return (i * n) / T; }
__device__ __forceinline__ int cell_hi(int i, int n, int T) { return ((i + 1) * n + T - 1) / T; }

// ---- cells[b][i * T + j][c] = mean of Lab channel c over the cell's pixels.  One wave per cell (64 lanes stride over its pixels,
// fp32 per lane, fp64 across the lanes), four cells per block.
template <typename T>
__global__ __launch_bounds__(256) void palette_cells_kernel(DView x, int Tg, float* __restrict__ cells) {
  constexpr int N = Chunk<T>::N;
  const int lane = threadIdx.x & 63;
  const int64_t cell = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int NC = Tg * Tg;
  if (cell >= (int64_t)x.B * NC) return;             // whole waves leave together: nothing below synchronises the block
  const int b = (int)(cell / NC), n = (int)(cell % NC);
  const int i = n / Tg, j = n % Tg;
  const int r0 = cell_lo(i, x.H, Tg), r1 = cell_hi(i, x.H, Tg);
  const int c0 = cell_lo(j, x.W, Tg), c1 = cell_hi(j, x.W, Tg);
  const int cw = c1 - c0, cnt = (r1 - r0) * cw;
  const T* xp = reinterpret_cast<const T*>(x.ptr);
  float sL = 0.f, sa = 0.f, sb = 0.f;
  for (int p = lane; p < cnt; p += 64) {
    float v[N];
    Chunk<T>::load(xp + x.pix(b, r0 + p / cw, c0 + p % cw), v);
    const Lab q = pal_lab(v[0], v[1], v[2]);
    sL += q.L; sa += q.a; sb += q.b;
  }
  const double dL = wave_sum_d((double)sL), da = wave_sum_d((double)sa), db = wave_sum_d((double)sb);
  if (lane == 0) {
    float* o = cells + cell * 3;
    o[0] = (float)(dL / cnt); o[1] = (float)(da / cnt); o[2] = (float)(db / cnt);
  }
}

// ---- stats[b][c] = (mean of the N cells, unbiased std): two passes over the stored cells in fp64, one block per image; the three
// channels share each pass (two block reductions per image instead of six: the launch is latency, not work)
__global__ __launch_bounds__(256) void palette_stats_kernel(const float* __restrict__ cells, int NC, float* __restrict__ stats) {
  __shared__ double sh[3][16];
  const float* cp = cells + (int64_t)blockIdx.x * NC * 3;
  double s[3] = {0.0, 0.0, 0.0}, m[3], q[3] = {0.0, 0.0, 0.0};
  for (int n = threadIdx.x; n < NC; n += blockDim.x)
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += (double)cp[n * 3 + c];
  block_sum_d3(s, sh);
#pragma unroll
  for (int c = 0; c < 3; ++c) m[c] = s[c] / NC;
  for (int n = threadIdx.x; n < NC; n += blockDim.x)
#pragma unroll
    for (int c = 0; c < 3; ++c) { const double d = (double)cp[n * 3 + c] - m[c]; q[c] += d * d; }
  block_sum_d3(q, sh);
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    stats[(blockIdx.x * 3 + c) * 2] = (float)m[c];
    stats[(blockIdx.x * 3 + c) * 2 + 1] = (float)sqrt(q[c] / (NC - 1));
  }
}

// ---- batch[c][k] = mean over the images of stats[b][c][k], images in order, fp64
__global__ void palette_batch_mean_kernel(const float* __restrict__ stats, int B, float* __restrict__ batch) {
  const int t = threadIdx.x;
  if (t >= 6) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += (double)stats[b * 6 + t];
  batch[t] = (float)(s / B);
}

// ---- prior <- batch * batch_scale (first update, or no EMA), else decay * prior + (1 - decay) * batch * batch_scale; ++*steps
__global__ void palette_prior_update_kernel(const float* __restrict__ batch, float batch_scale, float* __restrict__ prior, int* __restrict__ steps,
                                            int use_ema, float decay) {
  const int t = threadIdx.x;
  const int first = *steps == 0;
  __syncthreads();
  if (t < 6) {
    const float v = batch[t] * batch_scale;
    prior[t] = (!use_ema || first) ? v : decay * prior[t] + (1.f - decay) * v;
  }
  if (t == 0) *steps = *steps + 1;
}

// ---- loss = scale / (3B) sum_{b,c} (|m - mp| + |s - sp|) / 100;  gstats = d(loss / scale) / d stats, sign(0) = 0 (a NaN gives 0)
__global__ __launch_bounds__(256) void palette_loss_kernel(const float* __restrict__ stats, const float* __restrict__ prior, int B, float scale,
                                                         float* __restrict__ loss, float* __restrict__ gstats) {
  __shared__ double sh[16];
  const float g = 1.f / (300.f * (float)B);
  double s = 0.0;
  for (int i = threadIdx.x; i < B * 6; i += blockDim.x) {
    const float d = stats[i] - prior[i % 6];
    s += (double)fabsf(d);
    if (gstats) gstats[i] = d > 0.f ? g : (d < 0.f ? -g : 0.f);
  }
  s = block_sum_d(s, sh);
  if (threadIdx.x == 0) *loss = (float)(s / (300.0 * B) * (double)scale);
}

// ---- gx[b,h,w,0..2] (+)= scale * dLoss/dx.  One pixel per lane: the gradient of every cell that holds the pixel (cells in order),
// then the transposed Jacobian of the Lab chain recomputed from x.
template <typename T, bool ACC>
__global__ __launch_bounds__(256) void palette_bwd_kernel(DView x, int Tg, const float* __restrict__ cells, const float* __restrict__ stats,
                                                        const float* __restrict__ gstats, float scale, DView gx) {
  constexpr int N = Chunk<T>::N;
  const int64_t total = (int64_t)x.B * x.H * x.W;
  const int NC = Tg * Tg;
  const T* xp = reinterpret_cast<const T*>(x.ptr);
  T* gp = reinterpret_cast<T*>(gx.ptr);
  const float invN = 1.f / (float)NC;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int w = (int)(idx % x.W), h = (int)((idx / x.W) % x.H), b = (int)(idx / ((int64_t)x.W * x.H));
    // per image and channel: d/dcell = A + K * (cell - m),  A = gm / N,  K = gs / ((N - 1) s), 0 where s == 0 (or NaN)
    float A[3], K[3], M[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float m = stats[(b * 3 + c) * 2], s = stats[(b * 3 + c) * 2 + 1];
      A[c] = gstats[(b * 3 + c) * 2] * invN;
      K[c] = s > 0.f ? gstats[(b * 3 + c) * 2 + 1] / ((float)(NC - 1) * s) : 0.f;
      M[c] = m;
    }
    // cells i with floor(i H / T) <= h < ceil((i + 1) H / T):  floor(h T / H) .. ceil((h + 1) T / H) - 1
    const int i0 = (h * Tg) / x.H, i1 = min(Tg - 1, ((h + 1) * Tg + x.H - 1) / x.H - 1);
    const int j0 = (w * Tg) / x.W, j1 = min(Tg - 1, ((w + 1) * Tg + x.W - 1) / x.W - 1);
    float gl[3] = {0.f, 0.f, 0.f};
    for (int i = i0; i <= i1; ++i) {
      const int rh = cell_hi(i, x.H, Tg) - cell_lo(i, x.H, Tg);
      for (int j = j0; j <= j1; ++j) {
        const float inv_area = 1.f / (float)(rh * (cell_hi(j, x.W, Tg) - cell_lo(j, x.W, Tg)));
        const float* cp = cells + ((int64_t)b * NC + i * Tg + j) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) gl[c] += (A[c] + K[c] * (cp[c] - M[c])) * inv_area;
      }
    }
    float v[N];
    Chunk<T>::load(xp + x.pix(b, h, w), v);
    float lin[3], dlin[3], pass[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float t = v[c] * 0.5f + 0.5f;
      pass[c] = (t >= 0.f && t <= 1.f) ? 0.5f : 0.f;       // torch.clamp passes the gradient on [0, 1] inclusive; x 0.5 of the denormalisation
      lin[c] = pal_lin(pal_clamp01(t), &dlin[c]);
    }
    const float X = (lin[0] * PAL_XR + lin[1] * PAL_XG + lin[2] * PAL_XB) / PAL_WX;
    const float Y = lin[0] * PAL_YR + lin[1] * PAL_YG + lin[2] * PAL_YB;
    const float Z = (lin[0] * PAL_ZR + lin[1] * PAL_ZG + lin[2] * PAL_ZB) / PAL_WZ;
    float dfx, dfy, dfz;
    pal_f(X, &dfx); pal_f(Y, &dfy); pal_f(Z, &dfz);
    // L = 116 fy - 16, a = 500 (fx - fy), b = 200 (fy - fz)
    const float gX = 500.f * gl[1] * dfx / PAL_WX;
    const float gY = (116.f * gl[0] - 500.f * gl[1] + 200.f * gl[2]) * dfy;
    const float gZ = -200.f * gl[2] * dfz / PAL_WZ;
    float o[3];
    o[0] = scale * pass[0] * dlin[0] * (gX * PAL_XR + gY * PAL_YR + gZ * PAL_ZR);
    o[1] = scale * pass[1] * dlin[1] * (gX * PAL_XG + gY * PAL_YG + gZ * PAL_ZG);
    o[2] = scale * pass[2] * dlin[2] * (gX * PAL_XB + gY * PAL_YB + gZ * PAL_ZB);
    T* dst = gp + gx.pix(b, h, w);
    if (ACC) {
      // channels 3..7 keep their bits: only the 16-byte chunk's first three values are recomputed
      Raw<T> raw = ldraw<T>(dst);
      if constexpr (N == 4) {
        raw[0] += o[0]; raw[1] += o[1]; raw[2] += o[2];
      } else {
        const float a0 = __builtin_bit_cast(float, raw[0] << 16) + o[0];
        const float a1 = __builtin_bit_cast(float, raw[0] & 0xffff0000u) + o[1];
        const float a2 = __builtin_bit_cast(float, raw[1] << 16) + o[2];
        raw[0] = (uint32_t)f2bf(a0) | ((uint32_t)f2bf(a1) << 16);
        raw[1] = (raw[1] & 0xffff0000u) | (uint32_t)f2bf(a2);
      }
      *reinterpret_cast<Raw<T>*>(dst) = raw;
    } else {
      float z[N];
#pragma unroll
      for (int e = 0; e < N; ++e) z[e] = e < 3 ? o[e] : 0.f;
      Chunk<T>::store(dst, z);
      if (N == 4) { const float zz[4] = {0.f, 0.f, 0.f, 0.f}; Chunk<T>::store(dst + 4, zz); }
    }
  }
}

}  // namespace

#define VCHK(v, name) do { if (gan_check_view(v, name)) return -1; } while (0)
#define PAL_T_OK(t, v) GAN_CHECK((t) >= 2 && (t) <= 1024 && (int64_t)(t) * (v)->H < (1 << 30) && (int64_t)(t) * (v)->W < (1 << 30), \
                                 "palette: low_freq_size must be in [2, 1024] (got %d): the unbiased std of one cell is NaN", (t))

extern "C" int gan_palette_stats(const gan_view* x, int tsize, float* cells, float* stats, void* stream) {
  VCHK(x, "palette_stats.x");
  GAN_CHECK(x->C == 8 && (x->dtype == GAN_F32 || x->dtype == GAN_BF16) && cells && stats, "palette_stats: x must be an fp32 or bf16 view with C=8 (3 real channels)");
  PAL_T_OK(tsize, x);
  hipStream_t s = (hipStream_t)stream;
  DView vx = to_dview(x);
  const int64_t ncell = (int64_t)x->B * tsize * tsize;
  GAN_CHECK((ncell + 3) / 4 < (1ll << 31), "palette_stats: too many cells");
  GAN_DISPATCH_DTYPE(x->dtype, hipLaunchKernelGGL((palette_cells_kernel<T>), dim3((unsigned)((ncell + 3) / 4)), dim3(256), 0, s, vx, tsize, cells);)
  hipLaunchKernelGGL(palette_stats_kernel, dim3(x->B), dim3(256), 0, s, cells, tsize * tsize, stats);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_palette_batch_mean(const float* stats, int B, float* batch, void* stream) {
  GAN_CHECK(stats && batch && B > 0, "palette_batch_mean: null pointer or empty batch");
  hipLaunchKernelGGL(palette_batch_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stats, B, batch);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_palette_prior_update(const float* batch, float batch_scale, float* prior, int* steps, int use_ema, float decay, void* stream) {
  GAN_CHECK(batch && prior && steps, "palette_prior_update: null pointer");
  GAN_CHECK(decay >= 0.f && decay <= 1.f, "palette_prior_update: ema_decay %g outside [0, 1]", (double)decay);
  hipLaunchKernelGGL(palette_prior_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, batch, batch_scale, prior, steps, use_ema, decay);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_palette_loss(const float* stats, const float* prior, int B, float scale, float* loss, float* gstats, void* stream) {
  GAN_CHECK(stats && prior && loss && B > 0, "palette_loss: null pointer or empty batch");
  hipLaunchKernelGGL(palette_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, stats, prior, B, scale, loss, gstats);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_palette_bwd(const gan_view* x, int tsize, const float* cells, const float* stats, const float* gstats, float scale,
                               const gan_view* gx, int accumulate, void* stream) {
  VCHK(x, "palette_bwd.x"); VCHK(gx, "palette_bwd.gx");
  GAN_CHECK(x->C == 8 && gx->C == 8 && (x->dtype == GAN_F32 || x->dtype == GAN_BF16) && x->dtype == gx->dtype,
            "palette_bwd: x and gx must be fp32 or bf16 views with C=8 and the same dtype");
  GAN_CHECK(x->B == gx->B && x->H == gx->H && x->W == gx->W && cells && stats && gstats, "palette_bwd: shape mismatch or null pointer");
  PAL_T_OK(tsize, x);
  const int64_t total = (int64_t)x->B * x->H * x->W;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  DView vx = to_dview(x), vg = to_dview(gx);
  hipStream_t s = (hipStream_t)stream;
  GAN_DISPATCH_DTYPE(x->dtype,
    if (accumulate) hipLaunchKernelGGL((palette_bwd_kernel<T, true>), dim3(grid), dim3(256), 0, s, vx, tsize, cells, stats, gstats, scale, vg);
    else hipLaunchKernelGGL((palette_bwd_kernel<T, false>), dim3(grid), dim3(256), 0, s, vx, tsize, cells, stats, gstats, scale, vg);)
  GAN_LAUNCH_CHECK();
  return 0;
}
