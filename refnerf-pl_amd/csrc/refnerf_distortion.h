/*
 * refnerf_distortion.h -- mip-NeRF 360's distortion loss of one step function per ray (stepfun.lossfun_distortion,
 * internal/stepfun.py:261-272) in O(N) per ray, forward and the gradient to the weights:
 *     u_i = (t_i + t_{i+1}) / 2,  delta_i = t_{i+1} - t_i,
 *     L   = sum_i sum_j w_i w_j |u_i - u_j| + (1/3) sum_i w_i^2 delta_i.
 * On nondecreasing knots the midpoints are nondecreasing too, so with
 *     du_k = 0.5 (t_{k+1} - t_{k-1})    (= u_k - u_{k-1}, taken as ONE subtraction of inputs, never as a difference of
 *                                         rounded midpoints)
 *     W_k  = sum_{j<k} w_j,   D_0 = 0,  D_k = D_{k-1} + du_k W_k       (= sum_{j<k} w_j (u_k - u_j))
 *     V_k  = sum_{j>k} w_j,   E_{N-1} = 0,  E_k = E_{k+1} + du_{k+1} V_k   (= sum_{j>k} w_j (u_j - u_k))
 * the loss is L = 2 sum_k w_k D_k + (1/3) sum_k w_k^2 delta_k and dL/dw_k = 2 (D_k + E_k) + (2/3) w_k delta_k.  Every term
 * of every sum is a product of non-negative factors (for non-negative weights): nothing cancels, so fp32 holds a relative
 * error of a few ulp per addition whatever the order, and a sum whose terms are all zero is an exact zero.  There is no
 * gradient to t: every sdist the model emits is detached.
 *
 * Same shape as refnerf_proposal.h: one wave per ray, four waves per block, the ray's t and w staged into wave-private LDS
 * with coalesced loads (rows of N + 1 floats are not 16-byte aligned: plain dword loads), no __syncthreads (a wave never
 * reads another wave's rows), no atomics, no scratch.  Lane l owns the contiguous run [l C, min((l + 1) C, N)) with
 * C = ceil(N / 64) <= 8: a serial scan inside the lane, a 64-lane scan across lanes, one fixed order throughout, so a ray
 * gives the same bits alone and inside any batch.
 * Unsorted knots give meaningless numbers, never an access outside the ray's rows (no index depends on the data).
 */
#pragma once
#include <hip/hip_runtime.h>

namespace rn {

constexpr int DIST_WAVES = 4;            /* rays per block */
constexpr int DIST_MAX_N = 512;          /* the interlevel kernels' limit */

__device__ __forceinline__ void dist_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

/* sum of v over the lanes below this one (lane 0: 0).  The exclusive value is the inclusive scan of the lane below, not
 * incl - v: no subtraction anywhere. */
__device__ __forceinline__ float dist_scan_below(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  const float below = __shfl_up(v, 1, 64);
  return lane == 0 ? 0.0f : below;
}

/* sum of v over the lanes above this one (lane 63: 0) */
__device__ __forceinline__ float dist_scan_above(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_down(v, o, 64);
    if (lane + o < 64) v += t;
  }
  const float above = __shfl_down(v, 1, 64);
  return lane == 63 ? 0.0f : above;
}

__device__ __forceinline__ float dist_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

/* the ray's rows into LDS: tt[0..N], ww[0..N-1] */
__device__ __forceinline__ void dist_stage(const float *__restrict__ t_row, const float *__restrict__ w_row, int N, float *tt, float *ww,
                                           int lane) {
  for (int i = lane; i <= N; i += 64) tt[i] = t_row[i];
  for (int i = lane; i < N; i += 64) ww[i] = w_row[i];
  dist_wave_sync();
}

/* The left recurrence on this lane's run [k0, k1): returns W_{k0} (*Wb) and D_{k0 - 1} (*Db, the sum of du_m W_m over
 * every m >= 1 below the run); lane_w: the sum of the run's weights. */
__device__ __forceinline__ void dist_left_bases(const float *tt, const float *ww, int k0, int k1, int lane, float *lane_w, float *Wb,
                                                float *Db) {
  float sw = 0.0f;
#pragma clang loop unroll(disable)
  for (int k = k0; k < k1; ++k) sw += ww[k];
  *lane_w = sw;
  *Wb = dist_scan_below(sw, lane);
  float W = *Wb, A = 0.0f;
#pragma clang loop unroll(disable)
  for (int k = k0; k < k1; ++k) {
    if (k >= 1) A += (0.5f * (tt[k + 1] - tt[k - 1])) * W;
    W += ww[k];
  }
  *Db = dist_scan_below(A, lane);
}

/* ray_loss[ray] = L */
__global__ __launch_bounds__(64 * DIST_WAVES) void distortion_fwd_kernel(const float *__restrict__ t, const float *__restrict__ w, int R, int N,
                                                                         float *__restrict__ ray_loss) {
  __shared__ float s_t[DIST_WAVES][DIST_MAX_N + 1];
  __shared__ float s_w[DIST_WAVES][DIST_MAX_N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ray = blockIdx.x * DIST_WAVES + wave;
  if (ray >= R) return;                                    /* wave-uniform */
  float *tt = s_t[wave], *ww = s_w[wave];
  dist_stage(t + (size_t)ray * (N + 1), w + (size_t)ray * N, N, tt, ww, lane);
  const int chunk = (N + 63) >> 6, k0 = lane * chunk, k1 = (k0 + chunk < N) ? k0 + chunk : N;      /* k0 >= N: an empty run */
  float sw, W, D;
  dist_left_bases(tt, ww, k0, k1, lane, &sw, &W, &D);
  float inter = 0.0f, intra = 0.0f;
#pragma clang loop unroll(disable)
  for (int k = k0; k < k1; ++k) {
    if (k >= 1) D += (0.5f * (tt[k + 1] - tt[k - 1])) * W;
    const float wk = ww[k];
    inter += wk * D;
    intra += (wk * wk) * (tt[k + 1] - tt[k]);
    W += wk;
  }
  inter = dist_wave_sum(inter);
  intra = dist_wave_sum(intra);
  if (lane == 0) ray_loss[ray] = 2.0f * inter + intra / 3.0f;
}

/* grad_w[ray][k] = g[0] (2 (D_k + E_k) + (2/3) w_k delta_k): both scans again, nothing saved by the forward */
__global__ __launch_bounds__(64 * DIST_WAVES) void distortion_bwd_kernel(const float *__restrict__ t, const float *__restrict__ w,
                                                                         const float *__restrict__ g, int R, int N,
                                                                         float *__restrict__ grad_w) {
  __shared__ float s_t[DIST_WAVES][DIST_MAX_N + 1];
  __shared__ float s_w[DIST_WAVES][DIST_MAX_N];
  __shared__ float s_d[DIST_WAVES][DIST_MAX_N];            /* D_k: written and read by the lane that owns k */
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ray = blockIdx.x * DIST_WAVES + wave;
  if (ray >= R) return;                                    /* wave-uniform */
  float *tt = s_t[wave], *ww = s_w[wave], *dd = s_d[wave];
  dist_stage(t + (size_t)ray * (N + 1), w + (size_t)ray * N, N, tt, ww, lane);
  const int chunk = (N + 63) >> 6, k0 = lane * chunk, k1 = (k0 + chunk < N) ? k0 + chunk : N;
  float sw, W, D;
  dist_left_bases(tt, ww, k0, k1, lane, &sw, &W, &D);
#pragma clang loop unroll(disable)
  for (int k = k0; k < k1; ++k) {
    if (k >= 1) D += (0.5f * (tt[k + 1] - tt[k - 1])) * W;
    dd[k] = D;
    W += ww[k];
  }
  /* the mirrored recurrence, from the run's last interval down: V_{k1 - 1} and E_{k1} (0 past the ray's end) */
  const float Vb = dist_scan_above(sw, lane);
  float V = Vb, B = 0.0f;
#pragma clang loop unroll(disable)
  for (int k = k1 - 1; k >= k0; --k) {
    if (k + 1 < N) B += (0.5f * (tt[k + 2] - tt[k])) * V;
    V += ww[k];
  }
  float E = dist_scan_above(B, lane);
  V = Vb;
  const float up = g[0];
  float *g_row = grad_w + (size_t)ray * N;
#pragma clang loop unroll(disable)
  for (int k = k1 - 1; k >= k0; --k) {
    if (k + 1 < N) E += (0.5f * (tt[k + 2] - tt[k])) * V;
    const float wk = ww[k];
    dd[k] = up * (2.0f * (dd[k] + E) + (2.0f * (wk * (tt[k + 1] - tt[k]))) / 3.0f);
    V += wk;
  }
  dist_wave_sync();
  for (int i = lane; i < N; i += 64) g_row[i] = dd[i];     /* coalesced */
}

}  // namespace rn
