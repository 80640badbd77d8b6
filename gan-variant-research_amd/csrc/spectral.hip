// Spectral normalisation of a convolution weight, forward and backward.
//
// Replaces torch.nn.utils.spectral_norm as the reference applies it to every discriminator convolution when
// `use_spectral_norm` is set (GAN_Variant1/models/discriminator_patchgan.py:21-23; Basic_GAN/src/models.py:68-69):
// W is weight_orig viewed as an h x w matrix (h = Cout, w = Cin*kh*kw; OIHW is already that matrix, row-major),
//   training-mode forward:  v <- normalize(W^T u),  u <- normalize(W v)      (one power iteration, in place, no gradient)
//   always:                 sigma = u . (W v),  W_sn = W / sigma
//   backward (u, v constants):  dL/dW = (G - <G, W_sn> u v^T) / sigma,  G = dL/dW_sn
// The matrices are small (<= 512 x 8192 fp32); every kernel is one pass over W at HBM/L2 speed, reductions are fixed-order
// (no atomics), so results are deterministic.
//
// gan_spectral_norm_batch_fwd / _bwd do the same for every spectral-norm convolution of a discriminator (all scales) in a fixed
// number of launches: each matrix is cut into tiles of SN_RB rows x SN_CB columns, one block per tile, and the blocks of all
// descriptors form one grid (block -> descriptor by binary search over first_block, as gan_pack_weight_batch does).  The fused
// trainer never materialises W_sn: the operand copies are packed from W with scale = sigma, and the backward uses <G, W> / sigma.
#include "common.h"

// max(x, eps) as F.normalize takes it (torch.clamp_min): a NaN norm stays NaN, so a NaN anywhere in the vector makes all of the
// normalised vector NaN.  fmaxf(NaN, eps) is eps, which would leave the other elements finite (and huge).
static __device__ __forceinline__ float sn_clamp_min(float x, float eps) { return x < eps ? eps : x; }

namespace {

// t[j] = sum_i W[i][j] * u[i]      (one thread per column, coalesced across j)
__global__ __launch_bounds__(256) void sn_wt_u_kernel(const float* __restrict__ W, int h, int w, const float* __restrict__ u, float* __restrict__ t) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= w) return;
  float s = 0.f;
  for (int i = 0; i < h; ++i) s += W[(int64_t)i * w + j] * u[i];
  t[j] = s;
}

// out = x / max(||x||, eps), single block
__global__ __launch_bounds__(1024) void sn_normalize_kernel(const float* __restrict__ x, int n, float eps, float* __restrict__ out) {
  __shared__ float sh[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 1024) s += x[i] * x[i];
  s = block_sum(s, sh);
  const float d = sn_clamp_min(sqrtf(s), eps);
  for (int i = threadIdx.x; i < n; i += 1024) out[i] = x[i] / d;
}

// s[i] = sum_j W[i][j] * v[j]      (one block per row)
__global__ __launch_bounds__(256) void sn_w_v_kernel(const float* __restrict__ W, int w, const float* __restrict__ v, float* __restrict__ s) {
  __shared__ float sh[16];
  const float* row = W + (int64_t)blockIdx.x * w;
  float a = 0.f;
  for (int j = threadIdx.x; j < w; j += 256) a += row[j] * v[j];
  a = block_sum(a, sh);
  if (threadIdx.x == 0) s[blockIdx.x] = a;
}

// power_iter: u <- s / max(||s||, eps); then sigma = u . s      (s = W v), single block
__global__ __launch_bounds__(1024) void sn_sigma_kernel(const float* __restrict__ s, int h, int power_iter, float eps, float* __restrict__ u, float* __restrict__ sigma) {
  __shared__ float sh[16];
  float d = 1.f;
  if (power_iter) {
    float q = 0.f;
    for (int i = threadIdx.x; i < h; i += 1024) q += s[i] * s[i];
    q = block_sum(q, sh);
    d = sn_clamp_min(sqrtf(q), eps);
  }
  float a = 0.f;
  for (int i = threadIdx.x; i < h; i += 1024) {
    float ui = u[i];
    if (power_iter) { ui = s[i] / d; u[i] = ui; }
    a += ui * s[i];
  }
  a = block_sum(a, sh);
  if (threadIdx.x == 0) sigma[0] = a;
}

__global__ __launch_bounds__(256) void sn_scale_kernel(const float* __restrict__ W, int64_t n, const float* __restrict__ sigma, float* __restrict__ out) {
  const float sg = sigma[0];
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = W[i] / sg;
}

// part[b] = sum over a fixed slice of G .* Wsn
__global__ __launch_bounds__(256) void sn_dot_kernel(const float* __restrict__ G, const float* __restrict__ Wsn, int64_t n, float* __restrict__ part) {
  __shared__ float sh[16];
  float a = 0.f;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) a += G[i] * Wsn[i];
  a = block_sum(a, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// dW[i][j] = (G[i][j] - dot * u[i] * v[j]) / sigma,  dot = sum(part[0..np))  (every block re-reduces the np partials: np <= 256)
__global__ __launch_bounds__(256) void sn_bwd_kernel(const float* __restrict__ G, const float* __restrict__ part, int np, const float* __restrict__ u,
                                                     const float* __restrict__ v, const float* __restrict__ sigma, int h, int w, float* __restrict__ dW) {
  __shared__ float sh[16];
  float a = threadIdx.x < np ? part[threadIdx.x] : 0.f;
  const float dot = block_sum(a, sh);
  const float sg = sigma[0];
  const int64_t n = (int64_t)h * w;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i / w), c = (int)(i - (int64_t)r * w);
    dW[i] = (G[i] - dot * u[r] * v[c]) / sg;
  }
}

// ---------------------------------------------------------------------------------------------------------------- batched
constexpr int SN_RB = 32;    // rows per tile
constexpr int SN_CB = 256;   // columns per tile (one per thread)

struct SnGeom {
  int R, Cb;                 // row tiles, column tiles
  float *part, *t, *nrm, *sp, *dotp;
};
__host__ __device__ inline SnGeom sn_geom(int h, int w, float* ws) {
  SnGeom g;
  g.R = (h + SN_RB - 1) / SN_RB;
  g.Cb = (w + SN_CB - 1) / SN_CB;
  g.part = ws;                                  // [R][w]    column sums of W^T u per row tile
  g.t = g.part + (int64_t)g.R * w;              // [w]       W^T u
  g.nrm = g.t + w;                              // [Cb]      sum of t^2 per column tile
  g.sp = g.nrm + g.Cb;                          // [Cb][h]   row sums of W t per column tile
  g.dotp = g.sp + (int64_t)g.Cb * h;            // [R*Cb]    <G, W> per tile
  return g;
}

__device__ __forceinline__ int sn_find(const gan_sn_desc* __restrict__ d, int n, int blk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].first_block <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// part[r][j] = sum_{i in row tile r} W[i][j] u[i]
__global__ __launch_bounds__(256) void snb_wtu_kernel(const gan_sn_desc* __restrict__ descs, int n) {
  const gan_sn_desc D = descs[sn_find(descs, n, blockIdx.x)];
  const int lb = blockIdx.x - D.first_block;
  if (lb >= D.nblocks) return;
  const SnGeom g = sn_geom(D.h, D.w, D.ws);
  const int r = lb / g.Cb, c = lb - r * g.Cb;
  const int j = c * SN_CB + threadIdx.x;
  if (j >= D.w) return;
  const int i0 = r * SN_RB, i1 = min(D.h, i0 + SN_RB);
  float s = 0.f;
  for (int i = i0; i < i1; ++i) s += D.W[(int64_t)i * D.w + j] * D.u[i];
  g.part[(int64_t)r * D.w + j] = s;
}

// t = sum_r part[r] (power iteration) or v; tile (r, c) writes sp[c][i] = sum_{j in tile c} W[i][j] t[j] for its rows; the tiles of
// row 0 also keep t and the sum of t^2 over their columns
__global__ __launch_bounds__(256) void snb_wt_kernel(const gan_sn_desc* __restrict__ descs, int n, int power_iter) {
  const gan_sn_desc D = descs[sn_find(descs, n, blockIdx.x)];
  const int lb = blockIdx.x - D.first_block;
  if (lb >= D.nblocks) return;
  const SnGeom g = sn_geom(D.h, D.w, D.ws);
  const int r = lb / g.Cb, c = lb - r * g.Cb;
  __shared__ float tl[SN_CB];
  __shared__ float sh[16];
  const int j = c * SN_CB + threadIdx.x;
  float t = 0.f;
  if (j < D.w) {
    if (power_iter) {
      for (int q = 0; q < g.R; ++q) t += g.part[(int64_t)q * D.w + j];
    } else {
      t = D.v[j];
    }
  }
  tl[threadIdx.x] = t;
  if (r == 0) {                                   // block-uniform
    if (j < D.w) g.t[j] = t;
    const float q = block_sum(t * t, sh);
    if (threadIdx.x == 0) g.nrm[c] = q;
  }
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = 0; k < SN_RB / 4; ++k) {
    const int i = r * SN_RB + wv * (SN_RB / 4) + k;
    if (i >= D.h) break;                          // wave-uniform
    const float* row = D.W + (int64_t)i * D.w;
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < SN_CB / 64; ++q) {
      const int col = c * SN_CB + q * 64 + lane;
      if (col < D.w) a += row[col] * tl[q * 64 + lane];
    }
    a = wave_sum(a);
    if (lane == 0) g.sp[(int64_t)c * D.h + i] = a;
  }
}

// one block per descriptor: v = t / max(||t||, eps) (power iteration), s = W v = (sum_c sp[c]) / max(||t||, eps),
// u = s / max(||s||, eps) (power iteration), sigma = u . s, snapshots of (u, v) for the backward
__global__ __launch_bounds__(1024) void snb_finish_kernel(const gan_sn_desc* __restrict__ descs, int power_iter, float eps) {
  const gan_sn_desc D = descs[blockIdx.x];
  const SnGeom g = sn_geom(D.h, D.w, D.ws);
  __shared__ float sh[16];
  float d = 1.f;
  if (power_iter) {
    float q = 0.f;
    for (int c = threadIdx.x; c < g.Cb; c += blockDim.x) q += g.nrm[c];
    q = block_sum(q, sh);
    d = sn_clamp_min(sqrtf(q), eps);
    for (int j = threadIdx.x; j < D.w; j += blockDim.x) {
      const float vj = g.t[j] / d;
      D.v[j] = vj;
      D.v_snap[j] = vj;
    }
  } else {
    for (int j = threadIdx.x; j < D.w; j += blockDim.x) D.v_snap[j] = D.v[j];
  }
  float q2 = 0.f;
  for (int i = threadIdx.x; i < D.h; i += blockDim.x) {   // a thread owns row i: sp[0][i] is overwritten with s[i]
    float s = 0.f;
    for (int c = 0; c < g.Cb; ++c) s += g.sp[(int64_t)c * D.h + i];
    if (power_iter) s = s / d;
    g.sp[i] = s;
    q2 += s * s;
  }
  float du = 1.f;
  if (power_iter) du = sn_clamp_min(sqrtf(block_sum(q2, sh)), eps);
  float a = 0.f;
  for (int i = threadIdx.x; i < D.h; i += blockDim.x) {
    const float s = g.sp[i];
    float ui = D.u[i];
    if (power_iter) { ui = s / du; D.u[i] = ui; }
    D.u_snap[i] = ui;
    a += ui * s;
  }
  a = block_sum(a, sh);
  if (threadIdx.x == 0) D.sigma[0] = a;
}

// dotp[tile] = sum over the tile of G .* W
__global__ __launch_bounds__(256) void snb_dot_kernel(const gan_sn_desc* __restrict__ descs, int n) {
  const gan_sn_desc D = descs[sn_find(descs, n, blockIdx.x)];
  const int lb = blockIdx.x - D.first_block;
  if (lb >= D.nblocks) return;
  const SnGeom g = sn_geom(D.h, D.w, D.ws);
  const int r = lb / g.Cb, c = lb - r * g.Cb;
  __shared__ float sh[16];
  const int j = c * SN_CB + threadIdx.x;
  float a = 0.f;
  if (j < D.w) {
    const int i0 = r * SN_RB, i1 = min(D.h, i0 + SN_RB);
    for (int i = i0; i < i1; ++i) {
      const int64_t o = (int64_t)i * D.w + j;
      a += D.G[o] * D.W[o];
    }
  }
  a = block_sum(a, sh);
  if (threadIdx.x == 0) g.dotp[lb] = a;
}

// dW (+)= (G - (<G, W> / sigma) u v^T) / sigma over the tile; every block re-reduces the descriptor's tile partials in one order
__global__ __launch_bounds__(256) void snb_bwd_kernel(const gan_sn_desc* __restrict__ descs, int n, int accumulate) {
  const gan_sn_desc D = descs[sn_find(descs, n, blockIdx.x)];
  const int lb = blockIdx.x - D.first_block;
  if (lb >= D.nblocks) return;
  const SnGeom g = sn_geom(D.h, D.w, D.ws);
  const int r = lb / g.Cb, c = lb - r * g.Cb;
  __shared__ float sh[16];
  float a = 0.f;
  for (int k = threadIdx.x; k < D.nblocks; k += blockDim.x) a += g.dotp[k];
  const float sg = D.sigma[0];
  const float kk = block_sum(a, sh) / sg;
  const int j = c * SN_CB + threadIdx.x;
  if (j >= D.w) return;
  const float vj = D.v_snap[j];
  const int i0 = r * SN_RB, i1 = min(D.h, i0 + SN_RB);
  for (int i = i0; i < i1; ++i) {
    const int64_t o = (int64_t)i * D.w + j;
    const float val = (D.G[o] - kk * D.u_snap[i] * vj) / sg;
    D.dW[o] = accumulate ? D.dW[o] + val : val;
  }
}
}  // namespace

extern "C" int64_t gan_spectral_norm_batch_ws_floats(int h, int w) {
  if (h <= 0 || w <= 0) return 0;
  const int64_t R = (h + SN_RB - 1) / SN_RB, Cb = (w + SN_CB - 1) / SN_CB;
  return R * w + w + Cb + Cb * h + R * Cb;     // part, t, nrm, sp, dotp (sn_geom)
}

extern "C" int gan_spectral_norm_batch_blocks(int h, int w) {
  if (h <= 0 || w <= 0) return 0;
  return ((h + SN_RB - 1) / SN_RB) * ((w + SN_CB - 1) / SN_CB);
}

extern "C" int gan_spectral_norm_batch_fwd(const gan_sn_desc* descs, int n, int total_blocks, int power_iter, float eps, void* stream) {
  GAN_CHECK(descs && n > 0 && total_blocks > 0, "spectral_norm_batch_fwd: bad arguments (n=%d, total_blocks=%d)", n, total_blocks);
  hipStream_t s = (hipStream_t)stream;
  if (power_iter) hipLaunchKernelGGL(snb_wtu_kernel, dim3(total_blocks), dim3(256), 0, s, descs, n);
  hipLaunchKernelGGL(snb_wt_kernel, dim3(total_blocks), dim3(256), 0, s, descs, n, power_iter);
  hipLaunchKernelGGL(snb_finish_kernel, dim3(n), dim3(1024), 0, s, descs, power_iter, eps);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_spectral_norm_batch_bwd(const gan_sn_desc* descs, int n, int total_blocks, int accumulate, void* stream) {
  GAN_CHECK(descs && n > 0 && total_blocks > 0, "spectral_norm_batch_bwd: bad arguments (n=%d, total_blocks=%d)", n, total_blocks);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(snb_dot_kernel, dim3(total_blocks), dim3(256), 0, s, descs, n);
  hipLaunchKernelGGL(snb_bwd_kernel, dim3(total_blocks), dim3(256), 0, s, descs, n, accumulate);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t gan_spectral_norm_ws_floats(int h, int w) { return (int64_t)h + w + 256 + 16; }

extern "C" int gan_spectral_norm_fwd(const float* W, int h, int w, float* u, float* v, int power_iter, float eps, float* sigma, float* Wsn,
                                     float* ws, void* stream) {
  GAN_CHECK(W && u && v && sigma && Wsn && ws && h > 0 && w > 0, "spectral_norm_fwd: null pointer or empty matrix (h=%d, w=%d)", h, w);
  hipStream_t s = (hipStream_t)stream;
  float* t = ws;          // [w]
  float* sv = ws + w;     // [h]
  if (power_iter) {
    hipLaunchKernelGGL(sn_wt_u_kernel, dim3((w + 255) / 256), dim3(256), 0, s, W, h, w, u, t);
    hipLaunchKernelGGL(sn_normalize_kernel, dim3(1), dim3(1024), 0, s, t, w, eps, v);
  }
  hipLaunchKernelGGL(sn_w_v_kernel, dim3(h), dim3(256), 0, s, W, w, v, sv);
  hipLaunchKernelGGL(sn_sigma_kernel, dim3(1), dim3(1024), 0, s, sv, h, power_iter, eps, u, sigma);
  const int64_t n = (int64_t)h * w;
  const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(sn_scale_kernel, dim3(grid), dim3(256), 0, s, W, n, sigma, Wsn);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_spectral_norm_bwd(const float* G, const float* Wsn, const float* u, const float* v, const float* sigma, int h, int w, float* dW,
                                     float* ws, void* stream) {
  GAN_CHECK(G && Wsn && u && v && sigma && dW && ws && h > 0 && w > 0, "spectral_norm_bwd: null pointer or empty matrix (h=%d, w=%d)", h, w);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)h * w;
  const int np = (int)((n + 255) / 256 < 256 ? (n + 255) / 256 : 256);
  float* part = ws + h + w;   // [256]
  hipLaunchKernelGGL(sn_dot_kernel, dim3(np), dim3(256), 0, s, G, Wsn, n, part);
  const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(sn_bwd_kernel, dim3(grid), dim3(256), 0, s, G, part, np, u, v, sigma, h, w, dW);
  GAN_LAUNCH_CHECK();
  return 0;
}
