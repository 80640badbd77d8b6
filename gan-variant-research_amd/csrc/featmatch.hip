// Feature-matching loss between two discriminator feature maps (include/mi355x_gan.h "feature matching"): one pass reads f and r once,
// sums |f - r| and adds sign(f - r) * act'(f) * grad_scale / n into the gradient view.
//
// HBM-bound: every lane owns 16-byte chunks along C (8 bf16 / 4 fp32) of interior pixels, a grid-stride walk over
// items = B*H*W*ceil(C/N) chunks in row order, so a wave reads 1 KiB of a row at a time.  U = 4 chunks per lane are loaded back to back (f,
// r and, when accumulating, g: up to 12 x 16 B per lane) before anything is computed, which keeps well over the ~32 KiB per CU in flight
// that hides an HBM miss (MI355X: 256 CUs).  The grid is min(2048, ceil(items / 256)) blocks of 256 lanes: at the largest trainer layer
// (16 x 128 x 128 x 64 bf16) a lane's whole share is ONE such group of four.
//
// Sums: fp32 per lane over its own chunks in walk order (element 0 .. N-1 of a chunk, then the next chunk), lanes -> block in fp64 (fixed
// shuffle tree, then the four waves in order), one fp64 partial per block into ws; a one-block tail launch adds the partials in fp64 in a
// fixed order and does the single `+=` onto the slot.  No atomics: repeated calls repeat their bits.
#include "common.h"

namespace {

constexpr int FM_THREADS = 256, FM_MAX_BLOCKS = 2048, FM_U = 4;

static inline int fm_chunk(int dtype) { return dtype == GAN_F32 ? 4 : 8; }
static inline int64_t fm_items(const gan_view* f, int C) {
  const int N = fm_chunk(f->dtype);
  return (int64_t)f->B * f->H * f->W * ((C + N - 1) / N);
}
static inline int fm_blocks(int64_t items) {
  const int64_t nb = (items + FM_THREADS - 1) / FM_THREADS;
  return (int)(nb < FM_MAX_BLOCKS ? (nb < 1 ? 1 : nb) : FM_MAX_BLOCKS);
}

struct FmGeom {
  uint32_t items, row_items, nck, H;      // chunks in all, per interior row (W * nck), per pixel; rows per image
  int C;
};

template <typename T, bool HAS_G>
__global__ __launch_bounds__(FM_THREADS) void featmatch_kernel(DView f, DView r, DView g, FmGeom q, int act, float inv, float inv02,
                                                              int accumulate, double* __restrict__ part) {
  constexpr int N = Chunk<T>::N;
  const T* fp = reinterpret_cast<const T*>(f.ptr);
  const T* rp = reinterpret_cast<const T*>(r.ptr);
  T* gp = reinterpret_cast<T*>(g.ptr);
  const int64_t stride = (int64_t)gridDim.x * FM_THREADS;
  float s = 0.f;
  for (int64_t i0 = (int64_t)blockIdx.x * FM_THREADS + threadIdx.x; i0 < (int64_t)q.items; i0 += FM_U * stride) {
    Raw<T> rf[FM_U], rr[FM_U], rg[FM_U];
    int64_t og[FM_U];
    int nv[FM_U];                             // real channels of the chunk (0: no chunk)
#pragma unroll
    for (int u = 0; u < FM_U; ++u) {
      const int64_t i = i0 + u * stride;
      nv[u] = 0;
      if (i < (int64_t)q.items) {
        const uint32_t row = (uint32_t)i / q.row_items, w = (uint32_t)i % q.row_items;
        const int b = (int)(row / q.H), y = (int)(row % q.H), x = (int)(w / q.nck), k = (int)(w % q.nck);
        nv[u] = q.C - k * N < N ? q.C - k * N : N;
        rf[u] = ldraw<T>(fp + f.pix(b, y, x) + k * N);
        rr[u] = ldraw<T>(rp + r.pix(b, y, x) + k * N);
        if (HAS_G) {
          og[u] = g.pix(b, y, x) + k * N;
          if (accumulate) rg[u] = ldraw<T>(gp + og[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < FM_U; ++u) {
      if (nv[u] == 0) continue;
      float vf[N], vr[N], vg[N];
      cvtraw<T>(rf[u], vf);
      cvtraw<T>(rr[u], vr);
      if (HAS_G && accumulate) cvtraw<T>(rg[u], vg);
#pragma unroll
      for (int e = 0; e < N; ++e) {
        if (e < nv[u]) {
          const float d = vf[e] - vr[e];
          s += fabsf(d);
          if (HAS_G) {
            const float m = (act == GAN_ACT_LRELU && !(vf[e] > 0.f)) ? inv02 : inv;
            const float v = d > 0.f ? m : (d < 0.f ? -m : 0.f);       // selects, never a product: nothing to contract into an fma
            vg[e] = accumulate ? vg[e] + v : v;
          }
        }
      }
      if (HAS_G) {
        if (nv[u] == N) {
          Chunk<T>::store(gp + og[u], vg);
        } else {                              // the pixel's last chunk holds pad channels: their bits stay
#pragma unroll
          for (int e = 0; e < N; ++e)
            if (e < nv[u]) st1<T>(gp + og[u] + e, vg[e]);
        }
      }
    }
  }
  // lanes -> block in fp64, fixed order
  double t = (double)s;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  __shared__ double sh[FM_THREADS / 64];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(FM_THREADS) void featmatch_tail_kernel(const double* __restrict__ part, int nblocks, double scale_over_n,
                                                                   float* __restrict__ loss) {
  double t = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += FM_THREADS) t += part[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  __shared__ double sh[FM_THREADS / 64];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) *loss = *loss + (float)((((sh[0] + sh[1]) + sh[2]) + sh[3]) * scale_over_n);
}

}  // namespace

#define VCHK(v, name) do { if (gan_check_view(v, name)) return -1; } while (0)

extern "C" int64_t gan_featmatch_ws_floats(const gan_view* f) {
  if (!f || f->B <= 0 || f->H <= 0 || f->W <= 0 || f->C <= 0) return 0;
  return 2 * (int64_t)fm_blocks(fm_items(f, f->C));       // one fp64 partial per block, for every C <= f->C
}

extern "C" int gan_featmatch(const gan_view* f, const gan_view* r, int C, float loss_scale, float* loss, float grad_scale, int act,
                             const gan_view* g, int accumulate, float* ws, void* stream) {
  VCHK(f, "featmatch.f"); VCHK(r, "featmatch.r");
  GAN_CHECK(f->dtype == GAN_F32 || f->dtype == GAN_BF16, "featmatch: fp32 or bf16 views");
  GAN_CHECK(r->dtype == f->dtype && r->B == f->B && r->H == f->H && r->W == f->W, "featmatch: f and r must share B, H, W and dtype");
  GAN_CHECK(C > 0 && C <= f->C && C <= r->C, "featmatch: C=%d real channels do not fit the views (%d, %d)", C, f->C, r->C);
  GAN_CHECK(act == GAN_ACT_NONE || act == GAN_ACT_LRELU, "featmatch: act must be GAN_ACT_NONE or GAN_ACT_LRELU");
  GAN_CHECK(loss && ws && (uintptr_t)ws % 8 == 0, "featmatch: loss and an 8-byte aligned workspace are required");
  if (g) {
    VCHK(g, "featmatch.g");
    GAN_CHECK(g->dtype == f->dtype && g->B == f->B && g->H == f->H && g->W == f->W && C <= g->C, "featmatch: g must share B, H, W and dtype with f and hold C channels");
  }
  const int N = fm_chunk(f->dtype);
  const int64_t items = fm_items(f, C);
  GAN_CHECK(items < ((int64_t)1 << 31), "featmatch: more than 2^31 - 1 chunks");
  const int64_t n = (int64_t)f->B * f->H * f->W * C;
  const int nblocks = fm_blocks(items);
  FmGeom q;
  q.nck = (uint32_t)((C + N - 1) / N);
  q.row_items = (uint32_t)f->W * q.nck;
  q.items = (uint32_t)items;
  q.H = (uint32_t)f->H;
  q.C = C;
  const float inv = grad_scale / (float)n, inv02 = 0.2f * inv;
  DView vf = to_dview(f), vr = to_dview(r), vg = g ? to_dview(g) : null_dview();
  hipStream_t s = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  GAN_DISPATCH_DTYPE(f->dtype,
    if (g) hipLaunchKernelGGL((featmatch_kernel<T, true>), dim3(nblocks), dim3(FM_THREADS), 0, s, vf, vr, vg, q, act, inv, inv02, accumulate ? 1 : 0, part);
    else hipLaunchKernelGGL((featmatch_kernel<T, false>), dim3(nblocks), dim3(FM_THREADS), 0, s, vf, vr, vg, q, act, inv, inv02, 0, part);)
  hipLaunchKernelGGL(featmatch_tail_kernel, dim3(1), dim3(FM_THREADS), 0, s, part, nblocks, (double)loss_scale / (double)n, loss);
  GAN_LAUNCH_CHECK();
  return 0;
}
