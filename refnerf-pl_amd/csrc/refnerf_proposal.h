/*
 * refnerf_proposal.h -- the two host-side pieces of the proposal-network configuration (num_levels = 3, separate PropMLP,
 * dilation and interlevel loss on: the Model constructor's defaults) as kernels:
 *   max_dilate_weights_kernel   stepfun.max_dilate_weights(..., renormalize=True)[..., 1:-1] between two levels
 *                               (internal/models.py:167-187, internal/stepfun.py:92-131);
 *   interlevel_fwd / bwd_kernel stepfun.lossfun_outer of one proposal level against the detached final level
 *                               (internal/train_utils.py:151-162, internal/stepfun.py:31-89).
 * Same shape as the other loss kernels: one wave per ray, four waves per block, the ray's arrays in wave-private LDS (no
 * __syncthreads: a wave never reads another wave's rows), no atomics, no scratch, every sum in one fixed order.
 * EVERY index that comes out of a search on the data is clamped to its array: unsorted or non-finite input gives
 * meaningless numbers, never an access outside the ray's rows.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#include "refnerf_hip.h"
#include "refnerf_level_common.h"

namespace rn {

constexpr int PROP_WAVES = 4;            /* rays per block */
constexpr int DILATE_MAX_M = 171;        /* 3 M - 2 <= 512, the resampler's limit */
constexpr int INTERLEVEL_MAX_N = 512;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

/* number of k in [0, n) with seq(k) <= v (LE) or seq(k) < v, for a nondecreasing seq: at most 10 probes for n <= 513 (the loop is bounded at 12), result in [0, n]
 * whatever the data */
template <bool LE, typename Seq>
__device__ __forceinline__ int count_below(Seq seq, int n, float v) {
  int lo = 0, hi = n;
#pragma clang loop unroll(disable)
  for (int it = 0; it < 12 && lo < hi; ++it) {
    const int mid = (lo + hi) >> 1;
    const float s = seq(mid);
    if (LE ? (s <= v) : (s < v)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* t [R][M+1], w [R][M] -> t_out [R][3M-1], w_out [R][3M-2].
 * Knots: the union of a = t (M+1), b = t[:-1] - d (M) and c = t[1:] + d (M), each already nondecreasing, so an element's
 * place in the sorted union is its own index plus its rank in the other two sequences (ties: a before b before c); the
 * VALUES are those of torch.sort, bit for bit, and are then clamped to [lo, hi].  Knot x covers the old intervals
 * { i : t_i - d <= x < t_{i+1} + d } = [ #{c <= x}, #{b <= x} ), a contiguous range since b and c are nondecreasing. */
__global__ __launch_bounds__(64 * PROP_WAVES) void max_dilate_weights_kernel(const float *__restrict__ t_in, const float *__restrict__ w_in,
                                                                             int R, int M, float d, float dom_lo, float dom_hi,
                                                                             float *__restrict__ t_out, float *__restrict__ w_out) {
  __shared__ float s_t[PROP_WAVES][DILATE_MAX_M + 1];
  __shared__ float s_p[PROP_WAVES][DILATE_MAX_M + 1];
  __shared__ float s_x[PROP_WAVES][3 * DILATE_MAX_M + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ray = blockIdx.x * PROP_WAVES + wave;
  if (ray >= R) return;                                    /* wave-uniform */
  float *tt = s_t[wave], *pp = s_p[wave], *xx = s_x[wave];
  const float *t_row = t_in + (size_t)ray * (M + 1), *w_row = w_in + (size_t)ray * M;
  const int K = 3 * M + 1;                                 /* knots of the dilated step function */
  for (int i = lane; i <= M; i += 64) tt[i] = t_row[i];
  for (int j = lane; j < K; j += 64) xx[j] = dom_lo;       /* a place no element lands on (unsorted input) is still defined */
  wave_sync();
  const float eps2 = FLT_EPSILON * FLT_EPSILON;
  for (int i = lane; i < M; i += 64) pp[i] = w_row[i] / fmaxf(eps2, tt[i + 1] - tt[i]);     /* weight_to_pdf */
  auto seq_a = [&](int k) { return tt[k]; };
  auto seq_b = [&](int k) { return tt[k] - d; };
  auto seq_c = [&](int k) { return tt[k + 1] + d; };
  for (int e = lane; e < K; e += 64) {                     /* e over the 3M + 1 elements: a | b | c */
    float v;
    int pos;
    if (e <= M) {
      v = seq_a(e);
      pos = e + count_below<false>(seq_b, M, v) + count_below<false>(seq_c, M, v);
    } else if (e <= 2 * M) {
      const int j = e - (M + 1);
      v = seq_b(j);
      pos = j + count_below<true>(seq_a, M + 1, v) + count_below<false>(seq_c, M, v);
    } else {
      const int j = e - (2 * M + 1);
      v = seq_c(j);
      pos = j + count_below<true>(seq_a, M + 1, v) + count_below<true>(seq_b, M, v);
    }
    xx[clampi(pos, 0, K - 1)] = fminf(fmaxf(v, dom_lo), dom_hi);
  }
  wave_sync();
  /* p'_j on the first 3M knots, w'_j = p'_j (x_{j+1} - x_j), kept in registers: 3M <= 513 -> at most 9 per lane */
  float wd[9];
  float part = 0.0f;
#pragma unroll
  for (int u = 0; u < 9; ++u) {
    const int j = lane + 64 * u;
    wd[u] = 0.0f;
    if (j < K - 1) {
      const float x = xx[j];
      const int i0 = clampi(count_below<true>(seq_c, M, x), 0, M), i1 = clampi(count_below<true>(seq_b, M, x), 0, M);
      float m = 0.0f;
#pragma clang loop unroll(disable)
      for (int i = i0; i < i1; ++i) m = fmaxf(m, pp[i]);
      wd[u] = m * (xx[j + 1] - x);                         /* pdf_to_weight */
      part += wd[u];
    }
  }
  /* renormalisation: the sum runs over all 3M intervals (the two dropped ones included), lane partials in index order
   * j = lane, lane + 64, ..., then the butterfly */
  const float denom = fmaxf(eps2, wave_sum(part));
  float *to_row = t_out + (size_t)ray * (K - 2), *wo_row = w_out + (size_t)ray * (K - 3);
  for (int j = lane + 1; j < K - 1; j += 64) to_row[j - 1] = xx[j];
#pragma unroll
  for (int u = 0; u < 9; ++u) {
    const int j = lane + 64 * u;
    if (j >= 1 && j < K - 2) wo_row[j - 1] = wd[u] / denom;
  }
}

/* The envelope side of one ray in wave-private LDS: te[Np+1] = t_env, cy[Np+1] = [0, cumsum(w_env)] in double (each lane
 * sums its contiguous chunk in order, an exclusive scan over the lanes joins them: one fixed order). */
__device__ __forceinline__ void interlevel_stage_env(const float *te_row, const float *we_row, int Np, float *te, double *cy, int lane) {
  for (int k = lane; k <= Np; k += 64) te[k] = te_row[k];
  const int chunk = (Np + 63) >> 6, k0 = lane * chunk;      /* <= 8 */
  double s = 0.0;
  for (int u = 0; u < chunk; ++u)
    if (k0 + u < Np) s += (double)we_row[k0 + u];
  const double incl = wave_scan_incl(s, lane);
  double run = incl - s;                                   /* sum of the chunks before this lane's */
  if (lane == 0) cy[0] = 0.0;
  for (int u = 0; u < chunk; ++u)
    if (k0 + u < Np) { run += (double)we_row[k0 + u]; cy[k0 + u + 1] = run; }
  wave_sync();
}

/* searchsorted of the mirror (stepfun.searchsorted): cnt = #{ k : t_env[k] <= v } over the Np + 1 knots,
 * idx_lo = max(cnt - 1, 0), idx_hi = min(cnt, Np) */
__device__ __forceinline__ int interlevel_count(const float *te, int Np, float v) {
  return count_below<true>([&](int k) { return te[k]; }, Np + 1, v);
}

/* excess r_i = max(0, w_i - w_outer_i) of fine interval i over the envelope, in double; lo / hi: the range of envelope
 * intervals [lo, hi) that w_outer_i sums */
__device__ __forceinline__ double interlevel_excess(const float *te, const double *cy, int Np, float ta, float tb, float w, int *lo, int *hi) {
  *lo = clampi(interlevel_count(te, Np, ta) - 1, 0, Np);
  *hi = clampi(interlevel_count(te, Np, tb), 0, Np);
  const double wo = cy[*hi] - cy[*lo];
  const double r = (double)w - wo;
  return r > 0.0 ? r : 0.0;
}

/* ray_loss[ray] = sum_i max(0, w_i - w_outer_i)^2 / (w_i + FLT_EPSILON) */
__global__ __launch_bounds__(64 * PROP_WAVES) void interlevel_fwd_kernel(const float *__restrict__ t, const float *__restrict__ w,
                                                                         const float *__restrict__ t_env, const float *__restrict__ w_env,
                                                                         int R, int N, int Np, float *__restrict__ ray_loss) {
  __shared__ float s_te[PROP_WAVES][INTERLEVEL_MAX_N + 2];
  __shared__ double s_cy[PROP_WAVES][INTERLEVEL_MAX_N + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ray = blockIdx.x * PROP_WAVES + wave;
  if (ray >= R) return;                                    /* wave-uniform */
  const float *te = s_te[wave];
  const double *cy = s_cy[wave];
  interlevel_stage_env(t_env + (size_t)ray * (Np + 1), w_env + (size_t)ray * Np, Np, s_te[wave], s_cy[wave], lane);
  const float *t_row = t + (size_t)ray * (N + 1), *w_row = w + (size_t)ray * N;
  double sum = 0.0;
  for (int i = lane; i < N; i += 64) {
    int lo, hi;
    const float wi = w_row[i];
    const double r = interlevel_excess(te, cy, Np, t_row[i], t_row[i + 1], wi, &lo, &hi);
    sum += r * r / ((double)wi + (double)FLT_EPSILON);
  }
  sum = wave_sum_f64(sum);
  if (lane == 0) ray_loss[ray] = (float)sum;
}

/* g_w_env[ray][k] = upstream * sum_{i : lo_i <= k < hi_i} -2 max(0, w_i - w_outer_i) / (w_i + FLT_EPSILON).
 * lo_i and hi_i are nondecreasing in i, so the i of one k are the contiguous range [ first i with hi_i > k, first i with
 * lo_i > k ): two searches per k and a sum in index order -- an element no penalised interval covers gets an exact zero. */
__global__ __launch_bounds__(64 * PROP_WAVES) void interlevel_bwd_kernel(const float *__restrict__ t, const float *__restrict__ w,
                                                                         const float *__restrict__ t_env, const float *__restrict__ w_env,
                                                                         int R, int N, int Np, const float *__restrict__ upstream,
                                                                         float *__restrict__ g_w_env) {
  __shared__ float s_te[PROP_WAVES][INTERLEVEL_MAX_N + 2];
  __shared__ double s_cy[PROP_WAVES][INTERLEVEL_MAX_N + 1];
  __shared__ float s_c[PROP_WAVES][INTERLEVEL_MAX_N];
  __shared__ unsigned short s_lo[PROP_WAVES][INTERLEVEL_MAX_N], s_hi[PROP_WAVES][INTERLEVEL_MAX_N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ray = blockIdx.x * PROP_WAVES + wave;
  if (ray >= R) return;                                    /* wave-uniform */
  const float *te = s_te[wave];
  const double *cy = s_cy[wave];
  float *cc = s_c[wave];
  unsigned short *ilo = s_lo[wave], *ihi = s_hi[wave];
  interlevel_stage_env(t_env + (size_t)ray * (Np + 1), w_env + (size_t)ray * Np, Np, s_te[wave], s_cy[wave], lane);
  const float *t_row = t + (size_t)ray * (N + 1), *w_row = w + (size_t)ray * N;
  for (int i = lane; i < N; i += 64) {
    int lo, hi;
    const float wi = w_row[i];
    const double r = interlevel_excess(te, cy, Np, t_row[i], t_row[i + 1], wi, &lo, &hi);
    cc[i] = (float)(-2.0 * r / ((double)wi + (double)FLT_EPSILON));
    ilo[i] = (unsigned short)lo;
    ihi[i] = (unsigned short)hi;
  }
  wave_sync();
  const double up = (double)upstream[0];
  float *g_row = g_w_env + (size_t)ray * Np;
  for (int k = lane; k < Np; k += 64) {
    const float kf = (float)k;                             /* indices <= 512 are exact in fp32 */
    const int ia = clampi(count_below<true>([&](int i) { return (float)ihi[i]; }, N, kf), 0, N);     /* #{ i : hi_i <= k } */
    const int ib = clampi(count_below<true>([&](int i) { return (float)ilo[i]; }, N, kf), 0, N);     /* #{ i : lo_i <= k } */
    double s = 0.0;
#pragma clang loop unroll(disable)
    for (int i = ia; i < ib; ++i) s += (double)cc[i];
    g_row[k] = (float)(up * s);
  }
}

}  // namespace rn
