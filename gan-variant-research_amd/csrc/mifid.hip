// Evaluation kernels (FID / MiFID over feature matrices): float64 moments, one float64 contraction on v_mfma_f64_16x16x4_f64 with
// two operand walks, and the cosine row minimum that never writes the n_a x n_b matrix.  The selection step (select_7k.py) adds a
// column transform (x - c[k]) * s[k] in the operand load, the squared-Euclidean row minimum on the same tile, and the k-means update.
//
// Replaces, on the reference's side (EVAL/eval/mifid.py), numpy's np.mean / np.cov over the Inception features and the batched
// float32 cosine loop of compute_cosine_distances_batched; the Frechet term itself is restated through the identity
//   tr sqrt(Sr Sf) = sum of the singular values of Rc Fc^T / sqrt((nr-1)(nf-1))          (Rc, Fc: column-centred features)
// so that the device work is contractions over D and the host factors one small matrix (evaluate.py).
//
// Feature matrices are row-major float32 or float64 with a row stride ld >= cols.  Every value is promoted to float64 when it is
// loaded and every sum is float64; reductions run in a fixed order and there is no floating-point atomic, so a repeated call repeats
// its bits.  The one atomic is the integer OR of the non-finite flag.
//
// Contraction tile: a 256-lane workgroup owns a 64 x 64 tile of C and walks the contraction 16 at a time.  Wave w owns the 32 x 32
// quarter (w >> 1, w & 1) as 2 x 2 MFMA tiles: 16 float64 accumulators (32 VGPRs) per lane, and per step of 4 two A and two B
// values from LDS feed four MFMAs.  Both operands sit in LDS k-major ([16][80] float64: 20 KiB for the pair) whatever their walk in
// memory, so the MFMA loop is the same for trans = 0 (k contiguous in memory, stored transposed) and trans = 1 (rows contiguous).
// A row stride of 80 float64 puts the k-rows l >> 4 = 0, 1 of one ds_read_b64 half-wave on disjoint halves of the 64 banks.  Centring,
// row scaling and the f32 -> f64 conversion happen between the global load and the LDS store; elements past an extent are stored
// as 0, so the tails cost nothing in the loop and the epilogue alone checks bounds.  The next k-slab's global loads are issued
// before the MFMAs of the current one.
#include "common.h"
#include <cmath>

typedef __attribute__((ext_vector_type(4))) double f64x4_t;

namespace {

constexpr int TM = 64, TK = 16, LDS_LD = 80;

__device__ __forceinline__ double ldf(const void* p, int f64, int64_t i) {
  return f64 ? reinterpret_cast<const double*>(p)[i] : (double)reinterpret_cast<const float*>(p)[i];
}

// ---- moments, columns: 16 columns x 16 row groups per workgroup (D / 16 workgroups: 128 for D = 2048, where 64 columns each would
// leave most of the chip idle); the mean, then the centred sum of squares in a second pass; the row groups fold in a fixed order
constexpr int CW = 16, RG = 16;
__device__ __forceinline__ double fold_groups(const double (*sh)[CW], int cl) {
  double s = sh[0][cl];
#pragma unroll
  for (int g = 1; g < RG; ++g) s += sh[g][cl];
  return s;
}

__global__ __launch_bounds__(256) void feat_cols_kernel(const void* __restrict__ X, int f64, int64_t n, int64_t D, int64_t ld,
                                                        double* __restrict__ mean, double* __restrict__ colcss) {
  __shared__ double sh[RG][CW];
  const int cl = threadIdx.x % CW, g = threadIdx.x / CW;
  const int64_t c = (int64_t)blockIdx.x * CW + cl;
  const bool in = c < D;
  double s = 0.0;
  if (in)
    for (int64_t r = g; r < n; r += RG) s += ldf(X, f64, r * ld + c);
  sh[g][cl] = s;
  __syncthreads();
  const double mu = fold_groups(sh, cl) / (double)n;
  __syncthreads();
  double q = 0.0;
  if (in)
    for (int64_t r = g; r < n; r += RG) {
      const double d = ldf(X, f64, r * ld + c) - mu;
      q += d * d;
    }
  sh[g][cl] = q;
  __syncthreads();
  if (g == 0 && in) {
    mean[c] = mu;
    colcss[c] = fold_groups(sh, cl);
  }
}

// ---- the D column sums -> one number, one workgroup, fixed order
__global__ __launch_bounds__(256) void feat_css_kernel(const double* __restrict__ colcss, int64_t D, double* __restrict__ css) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int64_t c = threadIdx.x; c < D; c += 256) s += colcss[c];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *css = sh[0];
}

// ---- moments, rows: one wave per row; L2 norm, sum, and the non-finite flag
__global__ __launch_bounds__(256) void feat_rows_kernel(const void* __restrict__ X, int f64, int64_t n, int64_t D, int64_t ld,
                                                        double* __restrict__ norm, double* __restrict__ rowsum, int32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  double s = 0.0, q = 0.0;
  bool bad = false;
  for (int64_t c = lane; c < D; c += 64) {
    const double v = ldf(X, f64, r * ld + c);
    bad |= !(fabs(v) <= 1.7976931348623157e308);      // NaN or Inf
    s += v;
    q += v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  if (bad) atomicOr(flag, 1);
  if (lane == 0) {
    norm[r] = sqrt(q);
    rowsum[r] = s;
  }
}

// ---- the contraction
struct GramArgs {
  const void* A; const void* B;
  const double* ca; const double* cb; const double* ra; const double* rb;
  const double* sa; const double* sb;      // MODE 2: column scales (trans = 0: indexed by k), applied after the centre
  const double* na; const double* nb;      // MODE 2: squared norms of the transformed rows, [M] and [N]
  int64_t lda, ldb, ldc;
  int M, N, K, a_f64, b_f64, trans, absolute, ntn;
  double alpha;
  double* C;          // MODE 0
  double* ws_min;     // MODE 1: [ntn][M]
  int32_t* ws_idx;    //         [ntn][M]
};

// Four elements of one operand's 64 x 16 slab at k0, as this lane stores them to LDS: trans = 0 lane -> row t >> 2, k 4 (t & 3) .. + 3;
// trans = 1 lane -> k t >> 4, rows 4 (t & 15) .. + 3.  (m: index along the tile's output extent, k: along the contraction)
// cs (column scale, trans = 0 only): the element becomes (x - cen[k]) * cs[k], two rounded operations in that order.
__device__ __forceinline__ void slab_load(const void* P, int f64, int64_t ld, const double* cen, const double* cs, const double* scl, int trans,
                                          int m0, int ext, int k0, int K, double v[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = m0 + (trans ? 4 * (t & 15) + j : t >> 2);
    const int k = k0 + (trans ? t >> 4 : 4 * (t & 3) + j);
    double x = 0.0;
    if (m < ext && k < K) {
      x = ldf(P, f64, trans ? (int64_t)k * ld + m : (int64_t)m * ld + k);
      if (cen) x -= cen[trans ? m : k];
      if (cs) x *= cs[k];
      if (scl) x *= scl[m];
    }
    v[j] = x;
  }
}

__device__ __forceinline__ void slab_store(double (*S)[LDS_LD], int trans, const double v[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (trans) S[t >> 4][4 * (t & 15) + j] = v[j];
    else S[4 * (t & 3) + j][t >> 2] = v[j];
  }
}

// MODE 0: C = alpha * sum.  MODE 1: per row of the tile, the minimum of d = 1 - s (or 1 - |s|) over the tile's columns and its column.
// MODE 2: the same minimum of d = max(0, na[i] + nb[j] - 2 s) over operands with the column transform; no row or column is left out.
template <int MODE>
__global__ __launch_bounds__(256) void gram_kernel(GramArgs p) {
  const double* const sa = MODE == 2 ? p.sa : nullptr;
  const double* const sb = MODE == 2 ? p.sb : nullptr;
  __shared__ double As[TK][LDS_LD], Bs[TK][LDS_LD];
  __shared__ double red_min[2][TM];
  __shared__ int32_t red_idx[2][TM];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1;
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TM;
  f64x4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4_t{0.0, 0.0, 0.0, 0.0};

  double va[4], vb[4];
  slab_load(p.A, p.a_f64, p.lda, p.ca, sa, p.ra, p.trans, m0, p.M, 0, p.K, va);
  slab_load(p.B, p.b_f64, p.ldb, p.cb, sb, p.rb, p.trans, n0, p.N, 0, p.K, vb);
  for (int k0 = 0; k0 < p.K; k0 += TK) {
    __syncthreads();                       // the previous slab's MFMAs have read LDS
    slab_store(As, p.trans, va);
    slab_store(Bs, p.trans, vb);
    __syncthreads();
    if (k0 + TK < p.K) {
      slab_load(p.A, p.a_f64, p.lda, p.ca, sa, p.ra, p.trans, m0, p.M, k0 + TK, p.K, va);
      slab_load(p.B, p.b_f64, p.ldb, p.cb, sb, p.rb, p.trans, n0, p.N, k0 + TK, p.K, vb);
    }
#pragma unroll
    for (int kk = 0; kk < TK / 4; ++kk) {
      const int k = 4 * kk + (lane >> 4);
      const double a0 = As[k][wm * 32 + (lane & 15)], a1 = As[k][wm * 32 + 16 + (lane & 15)];
      const double b0 = Bs[k][wn * 32 + (lane & 15)], b1 = Bs[k][wn * 32 + 16 + (lane & 15)];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }

  // accumulator register r of MFMA tile (mi, ni): row (lane >> 4) + 4 r, column lane & 15 (the f64 map, not the f32 one)
  if (MODE == 0) {
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + wm * 32 + mi * 16 + (lane >> 4) + 4 * r, col = n0 + wn * 32 + ni * 16 + (lane & 15);
          if (row < p.M && col < p.N) p.C[(int64_t)row * p.ldc + col] = p.alpha * acc[mi][ni][r];
        }
    return;
  }

  const double inf = __builtin_huge_val();
  bool col_in[2];
  int colj[2];
  double nbj[2] = {0.0, 0.0};
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    colj[ni] = n0 + wn * 32 + ni * 16 + (lane & 15);
    if (MODE == 2) {
      col_in[ni] = colj[ni] < p.N;
      if (col_in[ni]) nbj[ni] = p.nb[colj[ni]];
    } else {
      col_in[ni] = colj[ni] < p.N && (!p.rb || p.rb[colj[ni]] != 0.0);
    }
  }
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double best = inf;
      int bj = 0x7fffffff;
      double nai = 0.0;
      if (MODE == 2) {
        const int row = m0 + wm * 32 + mi * 16 + (lane >> 4) + 4 * r;
        if (row < p.M) nai = p.na[row];
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {          // ascending columns: a strict < keeps the lowest index of a tie
        double d;
        if (MODE == 2) {
          d = (nai + nbj[ni]) - 2.0 * acc[mi][ni][r];
          d = d < 0.0 ? 0.0 : d;                // not fmax: a NaN stays a NaN and loses every comparison
        } else {
          const double s = p.alpha * acc[mi][ni][r];
          d = 1.0 - (p.absolute ? fabs(s) : s);
        }
        if (col_in[ni] && d < best) { best = d; bj = colj[ni]; }
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
      }
      if ((lane & 15) == 0) {
        const int rl = wm * 32 + mi * 16 + (lane >> 4) + 4 * r;
        red_min[wn][rl] = best;
        red_idx[wn][rl] = bj;
      }
    }
  __syncthreads();
  if (threadIdx.x < TM) {
    const int rl = threadIdx.x, row = m0 + rl;
    if (row < p.M) {
      double best = red_min[0][rl];
      int bj = red_idx[0][rl];
      if (red_min[1][rl] < best) { best = red_min[1][rl]; bj = red_idx[1][rl]; }
      if (MODE != 2 && p.ra && p.ra[row] == 0.0) { best = inf; bj = 0x7fffffff; }
      p.ws_min[(int64_t)blockIdx.x * p.M + row] = best;
      p.ws_idx[(int64_t)blockIdx.x * p.M + row] = bj;
    }
  }
}

// ---- fold of the column tiles' partial minima, in tile order (ascending columns); a row with nothing to compare against: +inf, -1
__global__ __launch_bounds__(256) void rowmin_fold_kernel(const double* __restrict__ ws_min, const int32_t* __restrict__ ws_idx, int M, int ntn,
                                                          double* __restrict__ dmin, int32_t* __restrict__ imin) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  double best = __builtin_huge_val();
  int bj = -1;
  for (int t = 0; t < ntn; ++t) {
    const double v = ws_min[(int64_t)t * M + row];
    if (v < best) { best = v; bj = ws_idx[(int64_t)t * M + row]; }
  }
  dmin[row] = best;
  imin[row] = bj;
}

// tile counts in 64-bit arithmetic: an extent near INT_MAX must reach the checks, not wrap before them
inline int tiles(int n) { return (int)(((int64_t)n + TM - 1) / TM); }
constexpr int MAX_EXTENT = 0x7fffffff - TM;       // the kernels' int tile and slab offsets (n0 + 63, k0 + TK) stay below 2^31

int feat_args(const char* who, const void* X, int dtype, int64_t n, int64_t D, int64_t ld) {
  GAN_CHECK(X, "%s: null feature matrix", who);
  GAN_CHECK(dtype == GAN_FEAT_F32 || dtype == GAN_FEAT_F64, "%s: dtype %d is neither GAN_FEAT_F32 nor GAN_FEAT_F64", who, dtype);
  GAN_CHECK(n > 0 && D > 0 && n < (1ll << 31) && D < (1ll << 31), "%s: %lld x %lld: extents must be positive and below 2^31", who, (long long)n, (long long)D);
  GAN_CHECK(ld >= D, "%s: row stride %lld below the %lld columns", who, (long long)ld, (long long)D);
  GAN_CHECK((uintptr_t)X % (dtype == GAN_FEAT_F64 ? 8 : 4) == 0, "%s: misaligned feature matrix", who);
  return 0;
}

int gram_args(const char* who, GramArgs* g, const void* A, int a_dtype, int64_t lda, const void* B, int b_dtype, int64_t ldb, int trans,
              int M, int N, int K, const double* ca, const double* cb, const double* ra, const double* rb, double alpha) {
  GAN_CHECK(trans == 0 || trans == 1, "%s: trans must be 0 or 1 (got %d)", who, trans);
  GAN_CHECK(M > 0 && N > 0 && K > 0, "%s: extents must be positive (M=%d N=%d K=%d)", who, M, N, K);
  GAN_CHECK(M <= MAX_EXTENT && N <= MAX_EXTENT && K <= MAX_EXTENT, "%s: extents above %d are refused (M=%d N=%d K=%d)", who, MAX_EXTENT, M, N, K);
  if (feat_args(who, A, a_dtype, trans ? K : M, trans ? M : K, lda)) return -1;
  if (feat_args(who, B, b_dtype, trans ? K : N, trans ? N : K, ldb)) return -1;
  GAN_CHECK(!trans || (!ra && !rb), "%s: row scales belong to trans = 0", who);
  GAN_CHECK(tiles(M) <= 65535, "%s: M=%d beyond 65535 row tiles", who, M);
  GAN_CHECK(alpha == alpha, "%s: alpha is NaN", who);
  g->A = A; g->B = B; g->ca = ca; g->cb = cb; g->ra = ra; g->rb = rb;
  g->lda = lda; g->ldb = ldb; g->ldc = 0;
  g->M = M; g->N = N; g->K = K; g->a_f64 = a_dtype == GAN_FEAT_F64; g->b_f64 = b_dtype == GAN_FEAT_F64; g->trans = trans;
  g->absolute = 0; g->ntn = tiles(N); g->alpha = alpha;
  g->sa = nullptr; g->sb = nullptr; g->na = nullptr; g->nb = nullptr;
  g->C = nullptr; g->ws_min = nullptr; g->ws_idx = nullptr;
  return 0;
}

int64_t rowmin_idx_off(int M, int N) { return (((int64_t)(tiles(N)) * M * 8) + 15) / 16 * 16; }

// ---- the column transform outside the contraction: the same two rounded operations as slab_load (never one fused multiply-add with
// what follows, so a host restatement of x' repeats its bits)
__device__ __forceinline__ double xform(double x, const double* cen, const double* cs, int64_t k) {
#pragma clang fp contract(off)
  if (cen) x = x - cen[k];
  if (cs) x = x * cs[k];
  return x;
}

// ---- squared norms of the transformed rows: one wave per row, lane l sums columns l, l + 64, ... in order, then the xor tree
__global__ __launch_bounds__(256) void sqnorm_rows_kernel(const void* __restrict__ X, int f64, int64_t n, int64_t D, int64_t ld,
                                                          const double* __restrict__ cen, const double* __restrict__ cs, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  double q = 0.0;
  for (int64_t c = lane; c < D; c += 64) {
    const double v = xform(ldf(X, f64, r * ld + c), cen, cs, c);
    q += v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  if (lane == 0) out[r] = q;
}

// ---- k-means update.  Workgroup (cluster c, column strip of 256): the labels are scanned 256 at a time, the rows of cluster c are
// compacted in ascending order into LDS (ballot + prefix over the four waves), and lane t adds x'[row][strip + t] for those rows in
// that order -- per cluster and column one fixed, ascending-row sum, whatever the scheduling.  LDS is 1 KiB for the row list and 16
// bytes of wave counts, independent of k: k is bounded by the grid alone.  Strip 0 stores the count; cluster 0, strip 0 also raises
// the error word for a label outside [0, k) (such rows match no cluster and are skipped).
constexpr int KU = 256;
__global__ __launch_bounds__(KU) void kmeans_update_kernel(const void* __restrict__ X, int f64, int64_t n, int64_t D, int64_t ld,
                                                           const double* __restrict__ cen, const double* __restrict__ cs,
                                                           const int32_t* __restrict__ labels, int k, double* __restrict__ sums, int64_t lds,
                                                           int32_t* __restrict__ counts, int32_t* __restrict__ err) {
  __shared__ int32_t rows[KU];
  __shared__ int32_t wave_n[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int c = blockIdx.x;
  const int64_t col = (int64_t)blockIdx.y * KU + t;
  const bool col_in = col < D;
  const bool police = blockIdx.x == 0 && blockIdx.y == 0;
  double acc = 0.0;
  int32_t total = 0;
  bool bad = false;
  for (int64_t r0 = 0; r0 < n; r0 += KU) {
    const int64_t r = r0 + t;
    int32_t lab = -1;
    if (r < n) {
      lab = labels[r];
      bad |= lab < 0 || lab >= k;
    }
    const bool mine = r < n && lab == c;
    const unsigned long long b = __ballot(mine);
    if (lane == 0) wave_n[w] = __popcll(b);
    __syncthreads();
    int base = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < w) base += wave_n[i];
      cnt += wave_n[i];
    }
    if (mine) rows[base + __popcll(b & ((1ull << lane) - 1ull))] = (int32_t)(r - r0);
    __syncthreads();
    if (col_in)
      for (int i = 0; i < cnt; ++i) acc += xform(ldf(X, f64, (r0 + rows[i]) * ld + col), cen, cs, col);
    total += cnt;
    __syncthreads();                       // the list and the wave counts are rewritten by the next chunk
  }
  if (col_in) sums[(int64_t)c * lds + col] = acc;
  if (blockIdx.y == 0 && t == 0) counts[c] = total;
  if (police && bad) atomicOr(err, 1);
}

struct SqdistLayout { int64_t nb, wmin, widx, total; };
SqdistLayout sqdist_layout(int M, int N) {
  SqdistLayout l;
  const int64_t pairs = (int64_t)tiles(N) * M;
  l.nb = (int64_t)M * 8;
  l.wmin = (((int64_t)M + N) * 8 + 15) / 16 * 16;
  l.widx = l.wmin + (pairs * 8 + 15) / 16 * 16;
  l.total = l.widx + pairs * 4;
  return l;
}
}  // namespace

extern "C" int gan_feat_moments(const void* X, int dtype, int64_t n, int64_t D, int64_t ld, double* mean, double* colcss, double* norm,
                                double* rowsum, double* css, int32_t* flag, void* stream) {
  if (feat_args("feat_moments", X, dtype, n, D, ld)) return -1;
  GAN_CHECK(mean && colcss && norm && rowsum && css && flag, "feat_moments: null output");
  hipStream_t s = (hipStream_t)stream;
  const int f64 = dtype == GAN_FEAT_F64;
  if (hipMemsetAsync(flag, 0, sizeof(int32_t), s) != hipSuccess) return gan_set_error(-2, "feat_moments: clearing the flag failed");
  hipLaunchKernelGGL(feat_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, X, f64, n, D, ld, norm, rowsum, flag);
  hipLaunchKernelGGL(feat_cols_kernel, dim3((unsigned)((D + CW - 1) / CW)), dim3(256), 0, s, X, f64, n, D, ld, mean, colcss);
  hipLaunchKernelGGL(feat_css_kernel, dim3(1), dim3(256), 0, s, colcss, D, css);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_gram_f64(const void* A, int a_dtype, int64_t lda, const void* B, int b_dtype, int64_t ldb, int trans, int M, int N, int K,
                            const double* ca, const double* cb, const double* ra, const double* rb, double alpha, double* Cout, int64_t ldc,
                            void* stream) {
  GramArgs g;
  if (gram_args("gram_f64", &g, A, a_dtype, lda, B, b_dtype, ldb, trans, M, N, K, ca, cb, ra, rb, alpha)) return -1;
  GAN_CHECK(Cout && (uintptr_t)Cout % 8 == 0, "gram_f64: null or misaligned output");
  GAN_CHECK(ldc >= N, "gram_f64: output row stride %lld below the %d columns", (long long)ldc, N);
  g.C = Cout; g.ldc = ldc;
  hipLaunchKernelGGL(gram_kernel<0>, dim3(g.ntn, tiles(M)), dim3(256), 0, (hipStream_t)stream, g);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_cos_rowmin_bounds(int M, int N, int64_t* ws_bytes) {
  GAN_CHECK(ws_bytes, "cos_rowmin_bounds: null output");
  GAN_CHECK(M > 0 && N > 0, "cos_rowmin_bounds: extents must be positive (M=%d N=%d)", M, N);
  GAN_CHECK(M <= MAX_EXTENT && N <= MAX_EXTENT, "cos_rowmin_bounds: extents above %d are refused (M=%d N=%d)", MAX_EXTENT, M, N);
  *ws_bytes = rowmin_idx_off(M, N) + (int64_t)(tiles(N)) * M * 4;
  return 0;
}

extern "C" int gan_cos_rowmin(const void* A, int a_dtype, int64_t lda, const void* B, int b_dtype, int64_t ldb, int M, int N, int K,
                              const double* ca, const double* cb, const double* ra, const double* rb, double alpha, int absolute, void* ws,
                              int64_t ws_bytes, double* dmin, int32_t* imin, void* stream) {
  GramArgs g;
  if (gram_args("cos_rowmin", &g, A, a_dtype, lda, B, b_dtype, ldb, 0, M, N, K, ca, cb, ra, rb, alpha)) return -1;
  GAN_CHECK(absolute == 0 || absolute == 1, "cos_rowmin: absolute must be 0 or 1 (got %d)", absolute);
  GAN_CHECK(dmin && imin, "cos_rowmin: null output");
  int64_t need = 0;
  if (gan_cos_rowmin_bounds(M, N, &need)) return -1;
  GAN_CHECK(ws && (uintptr_t)ws % 16 == 0 && ws_bytes >= need, "cos_rowmin: workspace of %lld bytes, gan_cos_rowmin_bounds asks %lld (16-byte aligned)",
            (long long)ws_bytes, (long long)need);
  g.absolute = absolute;
  g.ws_min = reinterpret_cast<double*>(ws);
  g.ws_idx = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ws) + rowmin_idx_off(M, N));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gram_kernel<1>, dim3(g.ntn, tiles(M)), dim3(256), 0, s, g);
  hipLaunchKernelGGL(rowmin_fold_kernel, dim3((unsigned)(((int64_t)M + 255) / 256)), dim3(256), 0, s, g.ws_min, g.ws_idx, M, g.ntn, dmin, imin);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_sqdist_rowmin_bounds(int M, int N, int64_t* ws_bytes) {
  GAN_CHECK(ws_bytes, "sqdist_rowmin_bounds: null output");
  GAN_CHECK(M > 0 && N > 0, "sqdist_rowmin_bounds: extents must be positive (M=%d N=%d)", M, N);
  GAN_CHECK(M <= MAX_EXTENT && N <= MAX_EXTENT, "sqdist_rowmin_bounds: extents above %d are refused (M=%d N=%d)", MAX_EXTENT, M, N);
  *ws_bytes = sqdist_layout(M, N).total;
  return 0;
}

extern "C" int gan_sqdist_rowmin(const void* A, int a_dtype, int64_t lda, const void* B, int b_dtype, int64_t ldb, int M, int N, int K,
                                 const double* ca, const double* sa, const double* cb, const double* sb, void* ws, int64_t ws_bytes,
                                 double* dmin, int32_t* imin, void* stream) {
  GramArgs g;
  if (gram_args("sqdist_rowmin", &g, A, a_dtype, lda, B, b_dtype, ldb, 0, M, N, K, ca, cb, nullptr, nullptr, 1.0)) return -1;
  GAN_CHECK(dmin && imin, "sqdist_rowmin: null output");
  int64_t need = 0;
  if (gan_sqdist_rowmin_bounds(M, N, &need)) return -1;
  GAN_CHECK(ws && (uintptr_t)ws % 16 == 0 && ws_bytes >= need, "sqdist_rowmin: workspace of %lld bytes, gan_sqdist_rowmin_bounds asks %lld (16-byte aligned)",
            (long long)ws_bytes, (long long)need);
  const SqdistLayout l = sqdist_layout(M, N);
  char* base = reinterpret_cast<char*>(ws);
  double* na = reinterpret_cast<double*>(base);
  double* nb = reinterpret_cast<double*>(base + l.nb);
  g.sa = sa; g.sb = sb; g.na = na; g.nb = nb;
  g.ws_min = reinterpret_cast<double*>(base + l.wmin);
  g.ws_idx = reinterpret_cast<int32_t*>(base + l.widx);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sqnorm_rows_kernel, dim3((unsigned)(((int64_t)M + 3) / 4)), dim3(256), 0, s, A, g.a_f64, (int64_t)M, (int64_t)K, lda, ca, sa, na);
  hipLaunchKernelGGL(sqnorm_rows_kernel, dim3((unsigned)(((int64_t)N + 3) / 4)), dim3(256), 0, s, B, g.b_f64, (int64_t)N, (int64_t)K, ldb, cb, sb, nb);
  hipLaunchKernelGGL(gram_kernel<2>, dim3(g.ntn, tiles(M)), dim3(256), 0, s, g);
  hipLaunchKernelGGL(rowmin_fold_kernel, dim3((unsigned)(((int64_t)M + 255) / 256)), dim3(256), 0, s, g.ws_min, g.ws_idx, M, g.ntn, dmin, imin);
  GAN_LAUNCH_CHECK();
  return 0;
}

extern "C" int gan_kmeans_update(const void* X, int dtype, int64_t n, int64_t D, int64_t ld, const double* c, const double* s,
                                 const int32_t* labels, int k, double* sums, int64_t lds, int32_t* counts, int32_t* err, void* stream) {
  if (feat_args("kmeans_update", X, dtype, n, D, ld)) return -1;
  GAN_CHECK(labels && sums && counts && err, "kmeans_update: null labels or output");
  GAN_CHECK((uintptr_t)sums % 8 == 0 && (uintptr_t)labels % 4 == 0 && (uintptr_t)counts % 4 == 0 && (uintptr_t)err % 4 == 0, "kmeans_update: misaligned buffer");
  GAN_CHECK(k > 0 && k <= MAX_EXTENT, "kmeans_update: k = %d: between 1 and %d", k, MAX_EXTENT);
  GAN_CHECK(lds >= D, "kmeans_update: sums row stride %lld below the %lld columns", (long long)lds, (long long)D);
  const int64_t strips = (D + KU - 1) / KU;
  GAN_CHECK(strips <= 65535, "kmeans_update: D=%lld beyond 65535 column strips", (long long)D);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(err, 0, sizeof(int32_t), st) != hipSuccess) return gan_set_error(-2, "kmeans_update: clearing the error word failed");
  hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)k, (unsigned)strips), dim3(KU), 0, st, X, dtype == GAN_FEAT_F64, n, D, ld, c, s, labels, k, sums,
                     lds, counts, err);
  GAN_LAUNCH_CHECK();
  return 0;
}
