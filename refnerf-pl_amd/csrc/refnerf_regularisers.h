/*
 * refnerf_regularisers.h -- the six geometry regularisers of one level in one pass each way, and the perturbed-ray
 * sampler that feeds them (internal/train_utils.py:207-329, internal/sample_utils.py:40-79):
 *   weights entropy (:318-329), accumulated weights (:313-316), diffuse / specular / normal consistency (:207-279) and
 *   distance consistency (:282-310) between each of the first n rays and its `a` perturbed copies.
 * Same shape as refnerf_losses_fwd_kernel: one wave per ray, a lane loop over the samples, shuffles for the sums; no
 * atomics, no LDS.  Every masked mean of the reference (x[mask].mean()) becomes a (sum, count) pair of columns that the
 * host adds up over the rays and divides ON THE DEVICE, so nothing is read back: an empty mask is 0 / 0 = NaN, as
 * mean() of an empty selection is.  The kernels take the C ABI's argument structs as they are (include/refnerf_hip.h).
 */
#pragma once
#include <hip/hip_runtime.h>

#include "refnerf_hip.h"
#include "refnerf_level_common.h"

namespace rn {

/* lanes 0..2 hold one channel each: their sum in channel order (torch's sum over a last axis of 3), on every lane */
__device__ __forceinline__ float sum3_lanes(float v) {
  return (__shfl(v, 0, 64) + __shfl(v, 1, 64)) + __shfl(v, 2, 64);
}

/* One channel of a colour-consistency measure (train_utils.py:222-248) between the clean value x and its `a` noisy copies
 * y[0], y[3], ...: 'mse' mean_j (x - y_j)^2; 'avg_mse' (x - mean_j y_j)^2; 'var' the unbiased variance of the a + 1 values,
 * two-pass (mean, then squared deviations: these terms live on 1e-3-sized differences of O(1) renderings). */
__device__ __forceinline__ float colour_consistency_channel(int kind, float x, const float *y, int a) {
  float s = 0.0f;
  if (kind == REFNERF_CONSISTENCY_MSE) {
    for (int j = 0; j < a; ++j) { const float d = x - y[3 * j]; s += d * d; }
    return s / (float)a;
  }
  for (int j = 0; j < a; ++j) s += y[3 * j];
  if (kind == REFNERF_CONSISTENCY_AVG_MSE) {
    const float d = x - s / (float)a;
    return d * d;
  }
  const float mu = (x + s) / (float)(a + 1);
  float v = (x - mu) * (x - mu);
  for (int j = 0; j < a; ++j) { const float d = y[3 * j] - mu; v += d * d; }
  return v / (float)a;
}

/* terms[ray] = { entropy, entropy mask, (1 - acc)^2, diffuse, specular, normal, distance, consistency mask }: see
 * refnerf_ray_regularisers_forward in include/refnerf_hip.h.  The noisy copy (ray, j) is noisy ray ray * a + j. */
__global__ __launch_bounds__(256) void ray_regularisers_fwd_kernel(refnerf_regularisers_args A) {
  const int lane = threadIdx.x & 63, ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= A.R) return;                                  /* wave-uniform: the shuffles below see whole waves */
  const float acc = A.d_acc[ray];
  const bool hit_e = acc > A.thr_entropy;
  float ent = 0.0f;
  if (A.d_weights && hit_e) {
    const float *w_row = A.d_weights + (size_t)ray * A.S;
    for (int i = lane; i < A.S; i += 64) {
      const float w = w_row[i];
      ent += -w * logf(w + 1e-10f);
    }
  }
  ent = wave_sum(ent);
  const bool hit_c = ray < A.n && acc > A.thr_consistency;
  float dif = 0.0f, spc = 0.0f, nrm = 0.0f, dst = 0.0f;
  if (hit_c) {                                             /* wave-uniform as well */
    const size_t k0 = (size_t)ray * A.a;
    float p_dif = 0.0f, p_spc = 0.0f, p_nrm = 0.0f, p_dst = 0.0f;
    if (lane < 3) {
      const size_t x = (size_t)ray * 3 + lane, y = k0 * 3 + lane;
      if (A.d_diffuse) p_dif = colour_consistency_channel(A.diffuse_type, A.d_diffuse[x], A.d_n_diffuse + y, A.a);
      if (A.d_specular) p_spc = colour_consistency_channel(A.specular_type, A.d_specular[x], A.d_n_specular + y, A.a);
      if (A.d_normals) {
        const float nx = A.d_normals[x];
        for (int j = 0; j < A.a; ++j) p_nrm += nx * A.d_n_normals[y + 3 * j];
      }
      if (A.d_distance) {
        const float p = A.d_origins[x] + A.d_directions[x] * A.d_distance[ray];
        for (int j = 0; j < A.a; ++j) {
          const float d = p - (A.d_n_origins[y + 3 * j] + A.d_n_directions[y + 3 * j] * A.d_n_distance[k0 + j]);
          p_dst += d * d;
        }
      }
    }
    if (A.d_diffuse) { dif = sum3_lanes(p_dif); if (A.diffuse_type == REFNERF_CONSISTENCY_VAR) dif = dif / 3.0f; }
    if (A.d_specular) { spc = sum3_lanes(p_spc); if (A.specular_type == REFNERF_CONSISTENCY_VAR) spc = spc / 3.0f; }
    if (A.d_normals) nrm = 1.0f - sum3_lanes(p_nrm) / (float)A.a;       /* mean_j (1 - n . n_j) */
    if (A.d_distance) dst = sum3_lanes(p_dst) / (float)A.a;
  }
  if (lane == 0) {
    float *t = A.d_terms + (size_t)ray * 8;
    t[0] = ent; t[1] = hit_e ? 1.0f : 0.0f; t[2] = (1.0f - acc) * (1.0f - acc);
    t[3] = dif; t[4] = spc; t[5] = nrm; t[6] = dst; t[7] = hit_c ? 1.0f : 0.0f;
  }
}

/* gradient of k * colour_consistency(kind) of one ray into its clean row gx[3] and its noisy rows gy[a][3]; k = 0 for a
 * ray outside the mask, whose rows are then exact zeros (never 0 * NaN) */
__device__ __forceinline__ void colour_consistency_grad(int kind, bool hit, float k, const float *x, const float *y, int a,
                                                        float *gx, float *gy) {
  for (int c = 0; c < 3; ++c) {
    if (!hit) {
      gx[c] = 0.0f;
      for (int j = 0; j < a; ++j) gy[3 * j + c] = 0.0f;
      continue;
    }
    const float xc = x[c];
    if (kind == REFNERF_CONSISTENCY_MSE) {
      const float kk = k * (2.0f / (float)a);
      float s = 0.0f;
      for (int j = 0; j < a; ++j) { const float d = xc - y[3 * j + c]; s += d; gy[3 * j + c] = -kk * d; }
      gx[c] = kk * s;
      continue;
    }
    float s = 0.0f;
    for (int j = 0; j < a; ++j) s += y[3 * j + c];
    if (kind == REFNERF_CONSISTENCY_AVG_MSE) {
      const float d = xc - s / (float)a, gn = -(k * (2.0f / (float)a)) * d;
      gx[c] = (k * 2.0f) * d;
      for (int j = 0; j < a; ++j) gy[3 * j + c] = gn;
      continue;
    }
    const float mu = (xc + s) / (float)(a + 1), kk = k * (2.0f / (3.0f * (float)a));
    gx[c] = kk * (xc - mu);
    for (int j = 0; j < a; ++j) gy[3 * j + c] = kk * (y[3 * j + c] - mu);
  }
}

/* One pass over R * S elements for dL/d weights; the first R threads also write the per-ray gradients of their ray and
 * of its noisy copies.  Counts (the forward's column sums) and the upstream scales are read from device memory. */
__global__ __launch_bounds__(256) void ray_regularisers_bwd_kernel(refnerf_regularisers_args A) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (A.d_g_weights && e < (size_t)A.R * A.S) {
    const int ray = (int)(e / A.S);
    float g = 0.0f;
    if (A.d_acc[ray] > A.thr_entropy) {
      const float w = A.d_weights[e], k = A.d_scales[0] / A.d_sums[1];
      g = k * -(logf(w + 1e-10f) + w / (w + 1e-10f));
    }
    A.d_g_weights[e] = g;
  }
  if (e >= (size_t)A.R) return;
  const int r = (int)e;
  const float acc = A.d_acc[r];
  if (A.d_g_acc) A.d_g_acc[r] = (A.d_scales[1] / (float)A.R) * (-2.0f * (1.0f - acc));
  const bool in_n = r < A.n, hit = in_n && acc > A.thr_consistency;
  const float inv_count = hit ? 1.0f / A.d_sums[7] : 0.0f;
  const int a = in_n ? A.a : 0;                             /* rows past n have no noisy copies to write */
  const size_t x = (size_t)r * 3, k0 = (size_t)r * A.a, y = k0 * 3;
  if (A.d_g_diffuse)
    colour_consistency_grad(A.diffuse_type, hit, A.d_scales[2] * inv_count, A.d_diffuse + x, A.d_n_diffuse + y, a,
                            A.d_g_diffuse + x, A.d_g_n_diffuse + y);
  if (A.d_g_specular)
    colour_consistency_grad(A.specular_type, hit, A.d_scales[3] * inv_count, A.d_specular + x, A.d_n_specular + y, a,
                            A.d_g_specular + x, A.d_g_n_specular + y);
  if (A.d_g_normals) {
    const float k = hit ? -(A.d_scales[4] * inv_count) / (float)A.a : 0.0f;
    for (int c = 0; c < 3; ++c) {
      float s = 0.0f;
      for (int j = 0; j < a; ++j) {
        if (hit) s += A.d_n_normals[y + 3 * j + c];
        A.d_g_n_normals[y + 3 * j + c] = hit ? k * A.d_normals[x + c] : 0.0f;
      }
      A.d_g_normals[x + c] = hit ? k * s : 0.0f;
    }
  }
  if (A.d_g_distance) {
    const float k = hit ? (A.d_scales[5] * inv_count) * (2.0f / (float)A.a) : 0.0f;
    float p[3] = {0.0f, 0.0f, 0.0f}, g = 0.0f;
    if (hit)
      for (int c = 0; c < 3; ++c) p[c] = A.d_origins[x + c] + A.d_directions[x + c] * A.d_distance[r];
    for (int j = 0; j < a; ++j) {
      float gn = 0.0f;
      if (hit) {
        float dn = 0.0f;
        for (int c = 0; c < 3; ++c) {
          const float dj = A.d_n_directions[y + 3 * j + c];
          const float d = p[c] - (A.d_n_origins[y + 3 * j + c] + dj * A.d_n_distance[k0 + j]);
          g += d * A.d_directions[x + c];
          dn += d * dj;
        }
        gn = -k * dn;
      }
      A.d_g_n_distance[k0 + j] = gn;
    }
    A.d_g_distance[r] = hit ? k * g : 0.0f;
  }
}

/* sample_utils.sample_noisy_rays (:40-79), one thread per output ray k = j * n + i (angle-major, the order of the
 * reference's cat over the rotations): the ray looks at the same surface point o + dist d from the rotated direction. */
__global__ __launch_bounds__(256) void noisy_rays_kernel(refnerf_noisy_rays_args A) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= (size_t)A.a * A.n) return;
  const int j = (int)(k / A.n);
  const size_t i = k - (size_t)j * A.n;
  const float *T = A.d_rotations + 9 * j;
  const float dist = A.d_distance[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float d = (A.d_directions[3 * i] * T[3 * c] + A.d_directions[3 * i + 1] * T[3 * c + 1]) + A.d_directions[3 * i + 2] * T[3 * c + 2];
    const float v = (A.d_viewdirs[3 * i] * T[3 * c] + A.d_viewdirs[3 * i + 1] * T[3 * c + 1]) + A.d_viewdirs[3 * i + 2] * T[3 * c + 2];
    A.d_out_directions[3 * k + c] = d;
    A.d_out_viewdirs[3 * k + c] = v;
    A.d_out_origins[3 * k + c] = (A.d_origins[3 * i + c] + dist * A.d_directions[3 * i + c]) - dist * d;
  }
  A.d_out_radii[k] = A.d_radii[i];
  A.d_out_imageplane[2 * k] = A.d_imageplane[2 * i];
  A.d_out_imageplane[2 * k + 1] = A.d_imageplane[2 * i + 1];
  A.d_out_lossmult[k] = A.d_lossmult[i];
  A.d_out_near[k] = A.d_near[i];
  A.d_out_far[k] = A.d_far[i];
  A.d_out_cam_idx[k] = A.d_cam_idx[i];
}

}  // namespace rn
