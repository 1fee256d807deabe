/*
 * refnerf_raycast.h -- the kernel of include/refnerf_raycast.h: a fixed-step march through the TSDF grid, a bisection of the
 * first front-face bracket, depth, normal and colour at the refined crossing.  Included by refnerf_raycast.hip alone.  One
 * thread per pixel; a workgroup is a 16 x 16 pixel block and each of its four wavefronts an 8 x 8 tile (lane l is pixel
 * (l & 7, l >> 3) of the tile), so that neighbouring lanes march through neighbouring cells, their eight-corner gathers share
 * cache lines and a wave's rays leave the loop at similar k.  Arithmetic in double in the order the public header writes
 * down (the build has -ffp-contract=off: no fused multiply-add; sqrt and / are the correctly rounded ones), one rounding at
 * each store.  No LDS.  Voxel and pixel offsets are 64-bit.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/refnerf_raycast.h"

namespace rn {

constexpr int RAYCAST_TILE = 8;         /* a wavefront's pixels: 8 x 8 */
constexpr int RAYCAST_BLOCK_SIDE = 16;  /* a workgroup's pixels: 2 x 2 tiles */
constexpr int RAYCAST_BLOCK = RAYCAST_BLOCK_SIDE * RAYCAST_BLOCK_SIDE;

struct TsdfRaycastArgs {
  refnerf_tsdf_grid g;
  const float *tsdf, *weight, *rgb, *pixtocam, *pose;
  int width, height, refine;
  float iso, min_weight, step, t_near, t_far;
  float *depth, *normals, *view_rgb, *acc;
};

/* what the march needs of the grid and the ray, hoisted out of the loop */
struct RaycastRay {
  double o[3], d[3], origin[3], h, iso;
  int top[3];                    /* n[a] - 2: the highest cell index */
  long long sy, sz;              /* index distances of the y and z neighbours */
  float min_weight;
};

/* the SAMPLE lines of the public header: the cell's corner values and fractions at P = o + t d; returns the validity */
__device__ inline bool raycast_cell(const RaycastRay &r, const float *tsdf, const float *weight, double t, double c[8], double fr[3],
                                    long long *cell) {
  int i[3];
  for (int a = 0; a < 3; ++a) {
    const double P = r.o[a] + t * r.d[a];
    const double g = (P - r.origin[a]) / r.h;
    const double f = floor(g);
    i[a] = f > 0.0 ? (f < (double)r.top[a] ? (int)f : r.top[a]) : 0;      /* a NaN gives 0 */
    fr[a] = g - (double)i[a];
  }
  const long long p = ((long long)i[2] * r.sz + (long long)i[1] * r.sy) + i[0];
  *cell = p;
  bool ok = true;
  for (int m = 0; m < 8; ++m) {
    const long long q = p + (m & 1) + ((m >> 1) & 1) * r.sy + ((m >> 2) & 1) * r.sz;
    c[m] = (double)tsdf[q];
    ok = ok & (weight[q] >= r.min_weight);
  }
  return ok;
}

__device__ inline double raycast_lerp3(const double c[8], const double fr[3]) {
  const double x0 = c[0] + fr[0] * (c[1] - c[0]), x1 = c[2] + fr[0] * (c[3] - c[2]);
  const double x2 = c[4] + fr[0] * (c[5] - c[4]), x3 = c[6] + fr[0] * (c[7] - c[6]);
  const double y0 = x0 + fr[1] * (x1 - x0), y1 = x2 + fr[1] * (x3 - x2);
  return y0 + fr[2] * (y1 - y0);
}

template <bool kColour>
__global__ __launch_bounds__(RAYCAST_BLOCK) void tsdf_raycast_kernel(TsdfRaycastArgs A) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = (int)blockIdx.x * RAYCAST_BLOCK_SIDE + (wave & 1) * RAYCAST_TILE + (lane & 7);
  const int y = (int)blockIdx.y * RAYCAST_BLOCK_SIDE + (wave >> 1) * RAYCAST_TILE + (lane >> 3);
  if (x >= A.width || y >= A.height) return;
  const long long pix = (long long)y * A.width + x;

  RaycastRay r;
  const double h = (double)A.g.voxel_size;
  const int n[3] = {A.g.nx, A.g.ny, A.g.nz};
  r.h = h, r.iso = (double)A.iso, r.min_weight = A.min_weight;
  r.sy = A.g.nx, r.sz = (long long)A.g.nx * A.g.ny;
  const float *K = A.pixtocam, *m = A.pose;
  const double px = (double)x + 0.5, py = (double)y + 0.5;
  const double cx = (double)K[0] * px + (double)K[1] * py + (double)K[2];
  const double cy = -((double)K[3] * px + (double)K[4] * py + (double)K[5]);
  const double cz = -1.0;
  double t0 = (double)A.t_near, t1 = (double)A.t_far;
  bool miss = false;
  for (int a = 0; a < 3; ++a) {
    r.d[a] = (double)m[4 * a] * cx + (double)m[4 * a + 1] * cy + (double)m[4 * a + 2] * cz;
    r.o[a] = (double)m[4 * a + 3];
    r.origin[a] = (double)A.g.origin[a];
    r.top[a] = n[a] - 2;
    const double lo = r.origin[a], hi = r.origin[a] + (double)(n[a] - 1) * h;
    if (r.d[a] == 0.0) {
      miss = miss | !(lo <= r.o[a] && r.o[a] <= hi);
    } else {
      const double ta = (lo - r.o[a]) / r.d[a], tb = (hi - r.o[a]) / r.d[a];
      const double lo_t = ta < tb ? ta : tb, hi_t = ta > tb ? ta : tb;
      t0 = t0 > lo_t ? t0 : lo_t;
      t1 = t1 < hi_t ? t1 : hi_t;
    }
  }
  miss = miss | !(t1 >= t0);
  const double dt = (double)A.step * h / sqrt(r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2]);
  const double N = floor((t1 - t0) / dt);
  miss = miss | !(N <= (double)((long long)n[0] + n[1] + n[2]) / (double)A.step);

  /* the march: validity and crossing are selects, the only early exit is the hit */
  bool hit = false;
  double a_t = 0.0, b_t = 0.0, fa = 0.0, fb = 0.0;
  if (!miss) {
    bool prev = false;
    double v_prev = 0.0, t_prev = 0.0;
    const long long last = (long long)N;
    for (long long k = 0; k <= last; ++k) {
      const double t = t0 + (double)k * dt;
      double c[8], fr[3];
      long long cell;
      const bool ok = raycast_cell(r, A.tsdf, A.weight, t, c, fr, &cell);
      const double v = raycast_lerp3(c, fr) - r.iso;
      if (ok & prev & (v_prev >= 0.0) & (v < 0.0)) {
        hit = true, a_t = t_prev, b_t = t, fa = v_prev, fb = v;
        break;
      }
      prev = ok;
      v_prev = ok ? v : v_prev;
      t_prev = ok ? t : t_prev;
    }
  }

  float out_depth = 0.0f, out_acc = 0.0f, out_n[3] = {0.0f, 0.0f, 0.0f}, out_rgb[3] = {0.0f, 0.0f, 0.0f};
  if (hit) {
    double c[8], fr[3];
    long long cell;
    for (int it = 0; it < A.refine; ++it) {
      const double tm = 0.5 * (a_t + b_t);
      raycast_cell(r, A.tsdf, A.weight, tm, c, fr, &cell);
      const double vm = raycast_lerp3(c, fr) - r.iso;
      if (vm < 0.0) {
        b_t = tm, fb = vm;
      } else {
        a_t = tm, fa = vm;
      }
    }
    const double ts = a_t + (fa / (fa - fb)) * (b_t - a_t);
    raycast_cell(r, A.tsdf, A.weight, ts, c, fr, &cell);
    const double u0 = 1.0 - fr[0], u1 = 1.0 - fr[1], u2 = 1.0 - fr[2];
    const double gx = u1 * u2 * (c[1] - c[0]) + fr[1] * u2 * (c[3] - c[2]) + u1 * fr[2] * (c[5] - c[4]) + fr[1] * fr[2] * (c[7] - c[6]);
    const double gy = u0 * u2 * (c[2] - c[0]) + fr[0] * u2 * (c[3] - c[1]) + u0 * fr[2] * (c[6] - c[4]) + fr[0] * fr[2] * (c[7] - c[5]);
    const double gz = u0 * u1 * (c[4] - c[0]) + fr[0] * u1 * (c[5] - c[1]) + u0 * fr[1] * (c[6] - c[2]) + fr[0] * fr[1] * (c[7] - c[3]);
    const double s = sqrt(gx * gx + gy * gy + gz * gz);
    out_depth = (float)ts, out_acc = 1.0f;
    if (s > 0.0) out_n[0] = (float)(gx / s), out_n[1] = (float)(gy / s), out_n[2] = (float)(gz / s);
    if (kColour) {
      for (int ch = 0; ch < 3; ++ch) {
        double col[8];
        for (int mm = 0; mm < 8; ++mm)
          col[mm] = (double)A.rgb[3 * (cell + (mm & 1) + ((mm >> 1) & 1) * r.sy + ((mm >> 2) & 1) * r.sz) + ch];
        out_rgb[ch] = (float)raycast_lerp3(col, fr);
      }
    }
  }
  A.depth[pix] = out_depth;
  A.acc[pix] = out_acc;
  for (int ch = 0; ch < 3; ++ch) A.normals[3 * pix + ch] = out_n[ch];
  if (kColour) {
    for (int ch = 0; ch < 3; ++ch) A.view_rgb[3 * pix + ch] = out_rgb[ch];
  }
}

}  // namespace rn
