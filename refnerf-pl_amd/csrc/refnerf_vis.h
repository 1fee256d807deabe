/* Validation visualisations on the device (the reference's internal/vis.py: weighted_percentile, visualize_cmap, matte,
 * visualize_coord_mod, visualize_rays and the panels of visualize_suite).  include/refnerf_hip.h states the contracts.
 *
 *   vis_scan_partial_kernel  one block per 2048 sorted elements: the sum of their gathered weights -> one block sum
 *   vis_scan_blocks_kernel   one lane: the exclusive scan of the block sums in index order; zeroes the counts
 *   vis_scan_final_kernel    the inclusive scan acc[i]: block offset + the scan inside the block (a lane's 8 elements in
 *                            order, the lanes of a wave by a shuffle scan, the four waves in order)
 *   vis_pct_count_kernel     #{acc[i] <= target_p} for every percentile (integer atomics: exact in any order)
 *   vis_pct_final_kernel     one lane per percentile: the reference's interp from the two knots at the count
 *   vis_panels_kernel        one lane per pixel: every per-pixel panel of visualize_suite
 *   vis_cmap_kernel          one lane per pixel: visualize_cmap (curve, normalisation, table, matte, null colour)
 *   vis_resample_kernel      one block per ray: use_avg resampling of its step functions onto the uniform bins
 *   vis_ray_panel_kernel     one lane per panel pixel: renormalise, tile, strip, matte over bg_color
 *
 * Inputs are float32 or float64; all arithmetic is float64 (the library is compiled without contraction, so v * a + b * c
 * is two products and a sum, as torch evaluates it) and a float32 output is rounded once, by the store.  No float atomics:
 * the scan has one fixed order, so two runs are bit-identical. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "refnerf_hip.h"

namespace rn {

constexpr int VIS_THREADS = 256;
constexpr int VIS_SCAN_ITEMS = 8;
constexpr int VIS_SCAN_BLOCK = VIS_THREADS * VIS_SCAN_ITEMS;
constexpr double VIS_EPS32 = 0x1p-23;
constexpr int VIS_MATTE_WIDTH = 8;
constexpr double VIS_MATTE_DARK = (double)0.8f;      /* torch.where(mask, 1.0, 0.8) is a float32 tensor */
constexpr double VIS_MATTE_LIGHT = 1.0;

__device__ __forceinline__ double vis_load(const void *p, int64_t i, int f64) {
  return f64 ? static_cast<const double *>(p)[i] : (double)static_cast<const float *>(p)[i];
}
__device__ __forceinline__ void vis_store(void *p, int64_t i, int f64, double v) {
  if (f64) static_cast<double *>(p)[i] = v;
  else static_cast<float *>(p)[i] = (float)v;        /* the one rounding of a float32 panel */
}

/* ------------------------------------------------------------------------------------------ weighted percentiles */
struct VisPctArgs {
  const void *values, *weights, *nan_mask;
  const int64_t *order;
  int64_t n, n_weights;
  int32_t values_f64, weights_f64, n_ps, target_f32;
  double ps[REFNERF_VIS_MAX_PS];
  double *acc, *block_sums, *block_offs, *out;
  unsigned long long *counts;
  int64_t n_blocks;
};

__device__ __forceinline__ double vis_pct_weight(const VisPctArgs &a, int64_t i) {
  if (!a.weights) return 1.0;
  const int64_t o = a.order[i];
  if (o < 0 || o >= a.n) return NAN;                 /* not an order of these values: poison, never read out of bounds */
  const int64_t j = o % a.n_weights;                 /* vis.py:32: weight[remainder(sortidx, len(weight))] */
  double w = vis_load(a.weights, j, a.weights_f64);
  if (a.nan_mask && isnan(vis_load(a.nan_mask, j, a.weights_f64))) w = 0.0;
  return w;
}

__device__ __forceinline__ double vis_pct_value(const VisPctArgs &a, int64_t i) {
  const int64_t o = a.order[i];
  if (o < 0 || o >= a.n) return NAN;
  return vis_load(a.values, o, a.values_f64);
}

/* ps * acc_w[-1] / 100 as the reference's tensors evaluate it */
__device__ __forceinline__ double vis_pct_target(double p, double total, int f32) {
  if (f32) {
    float t = (float)p * (float)total;
    t = t / 100.0f;
    return (double)t;
  }
  return p * total / 100.0;
}

__global__ __launch_bounds__(VIS_THREADS) void vis_scan_partial_kernel(VisPctArgs a) {
  __shared__ double red[VIS_THREADS / 64];
  const int64_t base = (int64_t)blockIdx.x * VIS_SCAN_BLOCK + (int64_t)threadIdx.x * VIS_SCAN_ITEMS;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < VIS_SCAN_ITEMS; ++k)
    if (base + k < a.n) s += vis_pct_weight(a, base + k);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = red[0];
#pragma unroll
    for (int k = 1; k < VIS_THREADS / 64; ++k) t += red[k];
    a.block_sums[blockIdx.x] = t;
  }
}

__global__ void vis_scan_blocks_kernel(VisPctArgs a) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double run = 0.0;
    for (int64_t b = 0; b < a.n_blocks; ++b) {
      a.block_offs[b] = run;
      run += a.block_sums[b];
    }
    for (int p = 0; p < REFNERF_VIS_MAX_PS; ++p) a.counts[p] = 0ull;
  }
}

__global__ __launch_bounds__(VIS_THREADS) void vis_scan_final_kernel(VisPctArgs a) {
  __shared__ double wave_tot[VIS_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * VIS_SCAN_BLOCK + (int64_t)tid * VIS_SCAN_ITEMS;
  double loc[VIS_SCAN_ITEMS];
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < VIS_SCAN_ITEMS; ++k) {
    if (base + k < a.n) s += vis_pct_weight(a, base + k);
    loc[k] = s;
  }
  double inc = s;                                    /* inclusive scan of the lane totals inside the wave */
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  double before = a.block_offs[blockIdx.x];
  for (int w = 0; w < wave; ++w) before += wave_tot[w];
  before += inc - s;                                 /* the lanes before this one */
#pragma unroll
  for (int k = 0; k < VIS_SCAN_ITEMS; ++k)
    if (base + k < a.n) a.acc[base + k] = before + loc[k];
}

__global__ __launch_bounds__(VIS_THREADS) void vis_pct_count_kernel(VisPctArgs a) {
  const int64_t base = (int64_t)blockIdx.x * VIS_SCAN_BLOCK + (int64_t)threadIdx.x * VIS_SCAN_ITEMS;
  const double total = a.acc[a.n - 1];
  for (int p = 0; p < a.n_ps; ++p) {
    const double target = vis_pct_target(a.ps[p], total, a.target_f32);
    unsigned int c = 0;
#pragma unroll
    for (int k = 0; k < VIS_SCAN_ITEMS; ++k)
      if (base + k < a.n && target >= a.acc[base + k]) ++c;      /* torch.ge: false on a NaN */
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&a.counts[p], (unsigned long long)c);
  }
}

__global__ void vis_pct_final_kernel(VisPctArgs a) {
  const int p = threadIdx.x;
  if (blockIdx.x != 0 || p >= a.n_ps) return;
  const double target = vis_pct_target(a.ps[p], a.acc[a.n - 1], a.target_f32);
  int64_t idx = (int64_t)a.counts[p] - 1;
  idx = idx < 0 ? 0 : (idx > a.n - 2 ? a.n - 2 : idx);
  const double x0 = vis_pct_value(a, idx), x1 = vis_pct_value(a, idx + 1);
  const double a0 = a.acc[idx], a1 = a.acc[idx + 1];
  const double m = (x1 - x0) / (a1 - a0);
  const double b = x0 - m * a0;
  a.out[p] = m * target + b;
}

/* ------------------------------------------------------------------------------------------ per-pixel helpers */
__device__ __forceinline__ double vis_checker(int y, int x) {
  const int by = (y % (2 * VIS_MATTE_WIDTH)) / VIS_MATTE_WIDTH, bx = (x % (2 * VIS_MATTE_WIDTH)) / VIS_MATTE_WIDTH;
  return (by != 0) != (bx != 0) ? VIS_MATTE_LIGHT : VIS_MATTE_DARK;
}
/* vis * acc + bg * (1 - acc) */
__device__ __forceinline__ double vis_matte(double v, double acc, double bg) { return v * acc + bg * (1.0 - acc); }

__device__ __forceinline__ double vis_srgb(double x) {
  const double lin = 323.0 / 25.0 * x;
  const double mx = x != x ? x : fmax(VIS_EPS32, x);           /* torch.maximum keeps a NaN */
  const double cur = (211.0 * pow(mx, 5.0 / 12.0) - 11.0) / 200.0;
  return x <= 0.0031308 ? lin : cur;
}

__device__ __forceinline__ double vis_curve(double x, int curve) {
  if (curve == REFNERF_VIS_CURVE_NEG_LOG) return -log(x + VIS_EPS32);
  if (curve == REFNERF_VIS_CURVE_LOG) return log(x + VIS_EPS32);
  return x;
}

/* nan_to_num(clip((v - min(lo, hi)) / |hi - lo|, 0, 1)); v, lo, hi already curved */
__device__ __forceinline__ double vis_normalise(double v, double lo, double hi) {
  const double mn = (lo != lo || hi != hi) ? NAN : fmin(lo, hi);   /* torch.min keeps a NaN */
  double q = (v - mn) / fabs(hi - lo);
  q = q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);                          /* torch.clip keeps a NaN */
  return q != q ? 0.0 : q;                                          /* nan_to_num; no infinity survives the clip */
}

/* matplotlib's Colormap.__call__ on a float in [0, 1]: int(q N), N itself folded onto N - 1 */
__device__ __forceinline__ int vis_table_index(double q, int n) {
  const int i = (int)(q * (double)n);
  return i > n - 1 ? n - 1 : (i < 0 ? 0 : i);
}

/* torch.remainder(a, 2): the sign of the divisor */
__device__ __forceinline__ double vis_mod2(double a) {
  double r = fmod(a, 2.0);
  if (r != 0.0 && r < 0.0) r += 2.0;
  return r;
}

/* ------------------------------------------------------------------------------------------ the panels of the suite */
__global__ __launch_bounds__(VIS_THREADS) void vis_panels_kernel(refnerf_vis_panels_args a) {
  const int64_t p = (int64_t)blockIdx.x * VIS_THREADS + threadIdx.x;
  const int64_t npix = (int64_t)a.H * a.W;
  if (p >= npix) return;
  const int f = a.f64;
  const int y = (int)(p / a.W), x = (int)(p - (int64_t)y * a.W);
  const double bg = vis_checker(y, x);
  const double dm = a.d_distance_mean ? vis_load(a.d_distance_mean, p, f) : 0.0;
  double acc = a.d_acc ? vis_load(a.d_acc, p, f) : 1.0;
  if (a.d_distance_mean && dm != dm) acc = 0.0;                    /* vis.py:198 */
  if (a.d_acc_out && a.d_acc) vis_store(a.d_acc_out, p, f, acc);

  /* colour-like panels: (input, plain output, matted output, sRGB curve) */
  const void *c_in[4] = {a.d_rgb, a.d_diffuse, a.d_specular, a.d_tint};
  void *c_plain[4] = {a.d_color, a.d_diffuse_out, a.d_specular_out, nullptr};
  void *c_matte[4] = {a.d_color_matte, a.d_diffuse_matte, a.d_specular_matte, a.d_tint_matte};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!c_in[k] || (!c_plain[k] && !c_matte[k])) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double v = vis_load(c_in[k], p * 3 + c, f);
      if (k < 3 && a.linear_to_srgb) v = vis_srgb(v);
      if (c_plain[k]) vis_store(c_plain[k], p * 3 + c, f, v);
      if (c_matte[k] && a.d_acc) vis_store(c_matte[k], p * 3 + c, f, vis_matte(v, acc, bg));
    }
  }
  if (a.d_rgb_cc && a.d_color_corrected)
#pragma unroll
    for (int c = 0; c < 3; ++c) vis_store(a.d_color_corrected, p * 3 + c, f, vis_load(a.d_rgb_cc, p * 3 + c, f));

  /* colour-mapped depth */
  const void *d_in[2] = {a.d_distance_mean, a.d_distance_median};
  const double *d_lohi[2] = {a.d_lohi_mean, a.d_lohi_median};
  void *d_out[2] = {a.d_depth_mean, a.d_depth_median};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (!d_in[k] || !d_lohi[k] || !d_out[k] || !a.d_table || !a.d_acc) continue;
    const double lo = vis_curve(d_lohi[k][0] - VIS_EPS32, REFNERF_VIS_CURVE_NEG_LOG);
    const double hi = vis_curve(d_lohi[k][1] + VIS_EPS32, REFNERF_VIS_CURVE_NEG_LOG);
    const double q = vis_normalise(vis_curve(vis_load(d_in[k], p, f), REFNERF_VIS_CURVE_NEG_LOG), lo, hi);
    const float *rgb = a.d_table + 3 * vis_table_index(q, a.table_n);
#pragma unroll
    for (int c = 0; c < 3; ++c) vis_store(d_out[k], p * 3 + c, f, vis_matte((double)rgb[c], acc, bg));
  }
  if (a.d_depth_triplet && a.d_distance_median && a.d_distance_p5 && a.d_distance_p95 && a.d_lohi_triplet && a.d_acc) {
    const double med = vis_load(a.d_distance_median, p, f);
    const double t[3] = {2.0 * med - vis_load(a.d_distance_p5, p, f), med, vis_load(a.d_distance_p95, p, f)};
    const double lo = vis_curve(a.d_lohi_triplet[0] - VIS_EPS32, REFNERF_VIS_CURVE_LOG);
    const double hi = vis_curve(a.d_lohi_triplet[1] + VIS_EPS32, REFNERF_VIS_CURVE_LOG);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      vis_store(a.d_depth_triplet, p * 3 + c, f, vis_matte(vis_normalise(vis_curve(t[c], REFNERF_VIS_CURVE_LOG), lo, hi), acc, bg));
  }
  if (a.d_coords_mod && a.d_origins && a.d_directions && a.d_distance_mean && a.d_acc) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double coord = vis_load(a.d_origins, p * 3 + c, f) + vis_load(a.d_directions, p * 3 + c, f) * dm;
      vis_store(a.d_coords_mod, p * 3 + c, f, vis_matte(vis_mod2(coord + 1.0) / 2.0, acc, bg));   /* NaN * 0 stays NaN */
    }
  }
#pragma unroll
  for (int k = 0; k < REFNERF_VIS_MAX_NORMALS; ++k) {
    if (!a.d_normals[k] || !a.d_normals_out[k] || !a.d_acc) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      vis_store(a.d_normals_out[k], p * 3 + c, f, vis_matte(vis_load(a.d_normals[k], p * 3 + c, f) / 2.0 + 0.5, acc, bg));
  }
  if (a.d_roughness && a.d_roughness_out && a.d_acc)
    for (int c = 0; c < a.roughness_channels; ++c) {
      const int64_t i = p * a.roughness_channels + c;
      vis_store(a.d_roughness_out, i, f, vis_matte(tanh(vis_load(a.d_roughness, i, f)), acc, bg));
    }
}

/* ------------------------------------------------------------------------------------------ visualize_cmap */
__global__ __launch_bounds__(VIS_THREADS) void vis_cmap_kernel(refnerf_vis_cmap_args a) {
  const int64_t p = (int64_t)blockIdx.x * VIS_THREADS + threadIdx.x;
  if (p >= (int64_t)a.H * a.W) return;
  const int y = (int)(p / a.W), x = (int)(p - (int64_t)y * a.W);
  double lo = 0.0, hi = 0.0;
  if (a.normalise) {
    lo = vis_curve((a.d_lo ? *a.d_lo : 0.0) + a.lo_bias, a.curve);
    hi = vis_curve((a.d_hi ? *a.d_hi : 0.0) + a.hi_bias, a.curve);
  }
  const int C = a.channels, OC = a.d_table ? 3 : C;
  const bool null_px = a.d_alpha && a.d_alpha[p] == 0.0;            /* vis.py:249-253 */
  const double acc = a.d_acc ? vis_load(a.d_acc, p, a.f64) : 1.0, bg = vis_checker(y, x);
  const float *rgb = nullptr;
  for (int c = 0; c < OC; ++c) {
    double v;
    if (c < C) {
      v = vis_curve(vis_load(a.d_values, p * C + c, a.f64), a.curve);
      if (a.normalise) v = vis_normalise(v, lo, hi);
      if (a.d_table) rgb = a.d_table + 3 * vis_table_index(v, a.table_n);
    }
    if (a.d_table) v = (double)rgb[c];
    if (a.d_acc) v = vis_matte(v, acc, bg);
    if (null_px) v = a.null_color[c < 3 ? c : 2];
    vis_store(a.d_out, p * OC + c, a.out_f64, v);
  }
}

/* ------------------------------------------------------------------------------------------ ray lines */
struct VisResampleArgs {
  const void *sdist, *values, *weights;
  const double *edges;
  double *out_values, *out_alpha;
  int64_t line_stride;
  int32_t f64, n, N, C, resolution, accumulate, value_op;
};

__device__ __forceinline__ double vis_ray_value(const VisResampleArgs &a, int64_t i) {
  const double v = vis_load(a.values, i, a.f64);
  if (a.value_op == REFNERF_VIS_OP_CLIP01) return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
  if (a.value_op == REFNERF_VIS_OP_SQRT) return sqrt(v);
  return v;
}

/* math.interp(x, tp, fp) with fp strided by `fs`: K knots */
__device__ __forceinline__ double vis_interp(double x, int idx, const double *tp, const double *fp, int fs) {
  const double m = (fp[(idx + 1) * fs] - fp[idx * fs]) / (tp[idx + 1] - tp[idx]);
  const double b = fp[idx * fs] - m * tp[idx];
  return m * x + b;
}

/* one block per ray.  LDS: tp [N+1], then acc0 [N+1][C+2]: the cumulative sums of (value_c w_p, weight w_p, w_p) with a
 * leading zero, w_p = diff(tp).  Lane j < C + 2 sums function j serially (torch.cumsum's order). */
__global__ __launch_bounds__(VIS_THREADS) void vis_resample_kernel(VisResampleArgs a) {
  extern __shared__ double vis_lds[];
  const int ray = blockIdx.x, tid = threadIdx.x, N = a.N, C = a.C, F = C + 2;
  double *tp = vis_lds, *acc0 = vis_lds + (N + 1);
  for (int i = tid; i <= N; i += VIS_THREADS) tp[i] = vis_load(a.sdist, (int64_t)ray * (N + 1) + i, a.f64);
  __syncthreads();
  if (tid < F) {
    double run = 0.0, wsum = 0.0, rwsum = 0.0;
    acc0[tid] = 0.0;
    for (int i = 0; i < N; ++i) {
      const double wp = tp[i + 1] - tp[i];
      const double w = a.weights ? vis_load(a.weights, (int64_t)ray * N + i, a.f64) : 1.0;
      double f;
      if (tid < C) {
        double r = vis_ray_value(a, ((int64_t)ray * N + i) * C + tid);
        if (a.accumulate) {                          /* vis.py:138-143 */
          wsum += w;
          rwsum += r * w;
          r = (rwsum + VIS_EPS32) / (wsum + 2.0 * VIS_EPS32);
        }
        f = r * wp;
      } else if (tid == C) {
        wsum += w;
        f = (a.accumulate ? wsum : w) * wp;
      } else {
        f = wp;
      }
      run += f;
      acc0[(i + 1) * F + tid] = run;
    }
  }
  __syncthreads();
  const int64_t line = (int64_t)ray * a.line_stride;
  for (int k = tid; k < a.resolution; k += VIS_THREADS) {
    double lo_v[6], hi_v[6];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const double x = a.edges[k + e];
      int cnt = 0;
      for (int i = 0; i <= N; ++i) cnt += x >= tp[i] ? 1 : 0;
      int idx = cnt - 1;
      idx = idx < 0 ? 0 : (idx > N - 1 ? N - 1 : idx);
      for (int j = 0; j < F; ++j) (e ? hi_v : lo_v)[j] = vis_interp(x, idx, tp, acc0 + j, F);
    }
    const double denom = hi_v[C + 1] - lo_v[C + 1];
    const double den = denom != denom ? denom : fmax(VIS_EPS32, denom);      /* torch.maximum keeps a NaN */
    for (int c = 0; c < C; ++c) a.out_values[(line * a.resolution + k) * C + c] = (hi_v[c] - lo_v[c]) / den;
    a.out_alpha[line * a.resolution + k] = (hi_v[C] - lo_v[C]) / den;
  }
}

/* one lane per pixel of the [rows][resolution] panel */
__global__ __launch_bounds__(VIS_THREADS) void vis_ray_panel_kernel(const double *__restrict__ lines_v,
                                                                    const double *__restrict__ lines_a, int32_t L, int32_t res,
                                                                    int32_t C, int32_t rep, int64_t rows, double bg_color,
                                                                    const double *__restrict__ alpha_max, double *__restrict__ out_v,
                                                                    double *__restrict__ out_a) {
  const int64_t p = (int64_t)blockIdx.x * VIS_THREADS + threadIdx.x;
  if (p >= rows * res) return;
  const int64_t row = p / res;
  const int col = (int)(p - row * res);
  int64_t line = row;
  if (rep > 0) {
    const int64_t per_ray = (int64_t)L * rep + 1, ray = row / per_ray, j = row - ray * per_ray;
    line = j == (int64_t)L * rep ? -1 : ray * L + j / rep;        /* -1: the strip of background pixels */
  }
  double alpha = 0.0;
  if (line >= 0) {
    alpha = lines_a[line * res + col];
    if (alpha_max) {                                 /* vis.py:151-154 */
      const double mx = *alpha_max;
      alpha = alpha / (mx != mx ? mx : fmax(VIS_EPS32, mx));
    }
  }
  const double back = bg_color * (1.0 - alpha);
  for (int c = 0; c < C; ++c) {
    const double v = line >= 0 ? lines_v[(line * res + col) * C + c] : 0.0;
    out_v[p * C + c] = v * alpha + back;
  }
  out_a[p] = alpha;
}

}  // namespace rn
