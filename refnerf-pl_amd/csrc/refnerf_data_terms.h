/*
 * refnerf_data_terms.h -- the rest of the training step's loss assembly, one pass each way per level:
 *   the data term with either penalty and its two statistics (internal/train_utils.py:33-88 compute_data_loss: 'mse' or
 *   'charb', the disparity MSE of :62-67, the weighted angular error of the normals of :69-84 with ref_utils.py:40-50), and
 *   the edge-aware depth smoothness of patch batches (:90-119 compute_depth_smoothness_loss).
 * These kernels stream a few bytes per ray: one thread per ray / pixel in 256-thread blocks, the project's default for
 * that class (docs/EXPERIMENTS.md section 18; no other geometry was measured); the smoothness forward, which sums the cells
 * of a patch, takes one wave per patch and a lane loop over the cells, as ray_regularisers_fwd_kernel does over samples.
 * No atomics, no LDS: per-ray / per-patch rows that the host adds up with one column sum and normalises ON THE DEVICE, so
 * two runs give the same bits and nothing is read back.  The kernels take the C ABI's argument structs as they are
 * (include/refnerf_hip.h).
 */
#pragma once
#include <hip/hip_runtime.h>

#include "refnerf_hip.h"
#include "refnerf_level_common.h"

namespace rn {

constexpr float DATA_TERMS_EPS = 1.1920928955078125e-07f;      /* torch.finfo(float32).eps = 2^-23 */

/* ref_utils.l2_normalize (:40-42): x / sqrt(max(sum x^2, eps)) */
__device__ __forceinline__ void l2_normalize3(const float *x, float *out) {
  const float norm = sqrtf(fmaxf((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2], DATA_TERMS_EPS));
  out[0] = x[0] / norm; out[1] = x[1] / norm; out[2] = x[2] / norm;
}

/* terms[ray] = { sum_c lossmult r_c^2, sum_c lossmult penalty(r_c^2), (1 / (1 + distance_mean) - disps)^2,
 *                w acos(clip(n_hat . ngt_hat)), w = acc alphas }: refnerf_data_terms_forward in include/refnerf_hip.h */
__global__ __launch_bounds__(256) void data_terms_fwd_kernel(refnerf_data_terms_args A) {
  const int ray = blockIdx.x * 256 + threadIdx.x;
  if (ray >= A.R) return;
  const size_t x = (size_t)ray * 3;
  const float lm = A.d_lossmult[ray], pad2 = A.charb_padding * A.charb_padding;
  float mse = 0.0f, pen = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float r = A.d_rgb[x + c] - A.d_gt_rgb[x + c], r2 = r * r;     /* r^2 first, the padding after: train_utils.py:49,58 */
    mse += lm * r2;
    pen += lm * (A.penalty == REFNERF_PENALTY_CHARB ? sqrtf(r2 + pad2) : r2);
  }
  float disp = 0.0f, ang = 0.0f, w = 0.0f;
  if (A.d_distance_mean) {
    const float d = 1.0f / (1.0f + A.d_distance_mean[ray]) - A.d_disps[ray];
    disp = d * d;
  }
  if (A.d_normals) {
    float n[3], g[3];
    l2_normalize3(A.d_normals + x, n);
    l2_normalize3(A.d_normals_gt + x, g);
    const float lim = 1.0f - DATA_TERMS_EPS;
    const float dot = fminf(fmaxf((n[0] * g[0] + n[1] * g[1]) + n[2] * g[2], -lim), lim);
    w = A.d_acc[ray] * A.d_alphas[ray];
    ang = w * acosf(dot);
  }
  float *t = A.d_terms + (size_t)ray * 5;
  t[0] = mse; t[1] = pen; t[2] = disp; t[3] = ang; t[4] = w;
}

/* d_g_rgb[ray][c] = upstream lossmult d penalty(r_c^2) / d rgb_c; the statistics carry no gradient */
__global__ __launch_bounds__(256) void data_terms_bwd_kernel(refnerf_data_terms_args A) {
  const int ray = blockIdx.x * 256 + threadIdx.x;
  if (ray >= A.R) return;
  const size_t x = (size_t)ray * 3;
  const float k = A.d_upstream[0] * A.d_lossmult[ray], pad2 = A.charb_padding * A.charb_padding;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float r = A.d_rgb[x + c] - A.d_gt_rgb[x + c];
    A.d_g_rgb[x + c] = k * (A.penalty == REFNERF_PENALTY_CHARB ? r / sqrtf(r * r + pad2) : 2.0f * r);
  }
}

/* the bilateral weight of train_utils.py:95 between two pixels of the guide image: exp(-mean_c |a_c - b_c|) */
__device__ __forceinline__ float bilateral_weight(const float *a, const float *b) {
  return expf(-(((fabsf(a[0] - b[0]) + fabsf(a[1] - b[1])) + fabsf(a[2] - b[2])) / 3.0f));
}

/* |acc w d^2| of one cell edge */
__device__ __forceinline__ float smooth_edge(float acc, float w, float d) { return fabsf((acc * w) * (d * d)); }

/* its derivative with respect to d: the sign of the product is kept, as abs() does (0 at 0) */
__device__ __forceinline__ float smooth_edge_grad(float acc, float w, float d) {
  const float t = (acc * w) * (d * d);
  const float sgn = t > 0.0f ? 1.0f : (t < 0.0f ? -1.0f : 0.0f);
  return sgn * ((acc * w) * (2.0f * d));
}

/* terms[patch] = { sum over the (S-1)^2 cells of |acc00 w01 (v00 - v01)^2|, the same with the pixel below }; one wave per
 * patch, cell k = y (S-1) + x on lane k mod 64 */
__global__ __launch_bounds__(256) void depth_smoothness_fwd_kernel(refnerf_depth_smoothness_args A) {
  const int lane = threadIdx.x & 63, patch = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (patch >= A.P) return;                                /* wave-uniform: the shuffles below see whole waves */
  const int S = A.S, C = S - 1;
  const size_t p0 = (size_t)patch * S * S;
  float s01 = 0.0f, s10 = 0.0f;
  for (int k = lane; k < C * C; k += 64) {
    const int y = k / C, xx = k - y * C;
    const size_t i00 = p0 + (size_t)y * S + xx, i01 = i00 + 1, i10 = i00 + S;
    const float acc = A.d_acc[i00], v00 = A.d_distance[i00];
    s01 += smooth_edge(acc, bilateral_weight(A.d_rgb + 3 * i00, A.d_rgb + 3 * i01), v00 - A.d_distance[i01]);
    s10 += smooth_edge(acc, bilateral_weight(A.d_rgb + 3 * i00, A.d_rgb + 3 * i10), v00 - A.d_distance[i10]);
  }
  s01 = wave_sum(s01);
  s10 = wave_sum(s10);
  if (lane == 0) { A.d_terms[(size_t)patch * 2] = s01; A.d_terms[(size_t)patch * 2 + 1] = s10; }
}

/* Gather form, one thread per pixel: its own cell (as v00, both edges), the cell to its left (as v01) and the cell above
 * (as v10).  acc and the guide image get no gradient (the reference reads them under no_grad). */
__global__ __launch_bounds__(256) void depth_smoothness_bwd_kernel(refnerf_depth_smoothness_args A) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int S = A.S;
  if (e >= (size_t)A.P * S * S) return;
  const int in_patch = (int)(e % ((size_t)S * S)), y = in_patch / S, x = in_patch - y * S;
  const float v = A.d_distance[e];
  const float *c = A.d_rgb + 3 * e;
  float g = 0.0f;
  if (y < S - 1 && x < S - 1) {
    const float acc = A.d_acc[e];
    g += smooth_edge_grad(acc, bilateral_weight(c, c + 3), v - A.d_distance[e + 1]);
    g += smooth_edge_grad(acc, bilateral_weight(c, c + 3 * S), v - A.d_distance[e + S]);
  }
  if (x >= 1 && y < S - 1)
    g -= smooth_edge_grad(A.d_acc[e - 1], bilateral_weight(c - 3, c), A.d_distance[e - 1] - v);
  if (y >= 1 && x < S - 1)
    g -= smooth_edge_grad(A.d_acc[e - S], bilateral_weight(c - 3 * S, c), A.d_distance[e - S] - v);
  A.d_g_distance[e] = A.d_upstream[0] * g;
}

}  // namespace rn
