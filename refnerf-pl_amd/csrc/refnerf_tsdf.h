/*
 * refnerf_tsdf.h -- the kernels of include/refnerf_tsdf.h: TSDF fusion of one view and marching tetrahedra on the Kuhn
 * decomposition.  Included by refnerf_tsdf.hip alone.  Every kernel is one thread per voxel, x fastest (a wavefront's 64
 * lanes are 64 consecutive floats of a row), arithmetic in double in the order the public header writes down (the build has
 * -ffp-contract=off: no fused multiply-add), one rounding at each store.  Measured, the fusion kernel is bound by its 13 double
 * divisions per voxel, not by memory (docs/EXPERIMENTS.md, section 21).
 *
 * Workspace of the mesh entries, N = nx ny nz voxels, NB = ceil(N / 256) blocks:
 *     uint32 voff[N]    vertex count of the voxel's 7 edge slots, after the scan the index of its first vertex
 *     uint32 toff[N]    triangle count of the voxel's cell, after the scan the index of its first triangle
 *     uint32 vblk[NB], tblk[NB]   per-block sums, after the scan the blocks' offsets
 *     uint8  mask[N]    bits 0..6: the active edge slots; bit 7: the cell contributes and emits triangles
 * (7 N < 2^31 bounds the vertex count; 12 N < 2^32 bounds the triangle count, hence unsigned offsets.)
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/refnerf_tsdf.h"

namespace rn {

constexpr int TSDF_BLOCK = 256;

struct TsdfWorkspace {
  uint32_t *voff, *toff, *vblk, *tblk;
  uint8_t *mask;
};

__host__ __device__ inline long long tsdf_blocks(long long N) { return (N + TSDF_BLOCK - 1) / TSDF_BLOCK; }
__host__ __device__ inline size_t tsdf_workspace_bytes(long long N) {
  return (size_t)((8 * N + 8 * tsdf_blocks(N) + N + 15) / 16 * 16);
}
__host__ __device__ inline TsdfWorkspace tsdf_workspace(void *base, long long N) {
  TsdfWorkspace w;
  w.voff = (uint32_t *)base;
  w.toff = w.voff + N;
  w.vblk = w.toff + N;
  w.tblk = w.vblk + tsdf_blocks(N);
  w.mask = (uint8_t *)(w.tblk + tsdf_blocks(N));
  return w;
}

/* (i, j, k) of the linear index p: 7 N < 2^31, so 32-bit divisions do */
__device__ inline void tsdf_voxel_of(long long p, int nx, int ny, int *i, int *j, int *k) {
  const uint32_t q = (uint32_t)p, row = q / (uint32_t)nx;
  *i = (int)(q - row * (uint32_t)nx);
  *k = (int)(row / (uint32_t)ny);
  *j = (int)(row - (uint32_t)*k * (uint32_t)ny);
}

/* ------------------------------------------------------------------------------------------------------------ fusion */
struct TsdfIntegrateArgs {
  refnerf_tsdf_grid g;
  float *tsdf, *weight, *rgb;
  const float *pixtocam, *pose, *depth, *acc, *view_rgb;
  int width, height;
  float acc_min, view_weight, z_min;
};

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_integrate_kernel(TsdfIntegrateArgs A) {
  const long long N = (long long)A.g.nx * A.g.ny * A.g.nz;
  const long long p = (long long)blockIdx.x * TSDF_BLOCK + threadIdx.x;
  if (p >= N) return;
  int i, j, k;
  tsdf_voxel_of(p, A.g.nx, A.g.ny, &i, &j, &k);
  const double h = (double)A.g.voxel_size;
  const float *m = A.pose;
  const double dx = ((double)A.g.origin[0] + (double)i * h) - (double)m[3];
  const double dy = ((double)A.g.origin[1] + (double)j * h) - (double)m[7];
  const double dz = ((double)A.g.origin[2] + (double)k * h) - (double)m[11];
  const double q0 = (double)m[0] * dx + (double)m[4] * dy + (double)m[8] * dz;
  const double q1 = -((double)m[1] * dx + (double)m[5] * dy + (double)m[9] * dz);
  const double z = -((double)m[2] * dx + (double)m[6] * dy + (double)m[10] * dz);
  if (!(z > (double)A.z_min)) return;
  const double a = A.pixtocam[0], b = A.pixtocam[1], c = A.pixtocam[2], d = A.pixtocam[3], e = A.pixtocam[4], f = A.pixtocam[5];
  const double det = a * e - b * d;
  const double u = ((e / det) * q0 + (-b / det) * q1 + ((b * f - c * e) / det) * z) / z;
  const double v = ((-d / det) * q0 + (a / det) * q1 + ((c * d - a * f) / det) * z) / z;
  const double fx = floor(u), fy = floor(v);
  if (!(fx >= 0.0 && fx < (double)A.width && fy >= 0.0 && fy < (double)A.height)) return;
  const long long pix = (long long)fy * A.width + (long long)fx;
  const float Df = A.depth[pix];
  if (!(Df > 0.0f && Df < INFINITY)) return;                /* NaN, inf, 0 and negative depths are holes */
  if (A.acc && A.acc[pix] < A.acc_min) return;
  const double trunc = (double)A.g.trunc;
  const double sdf = (double)Df - z;
  if (sdf < -trunc) return;
  double obs = sdf / trunc;
  if (obs > 1.0) obs = 1.0;
  const double w = (double)A.view_weight, W = (double)A.weight[p], Wn = W + w;
  A.tsdf[p] = (float)((W * (double)A.tsdf[p] + w * obs) / Wn);
  if (A.rgb) {
    for (int ch = 0; ch < 3; ++ch)
      A.rgb[3 * p + ch] = (float)((W * (double)A.rgb[3 * p + ch] + w * (double)A.view_rgb[3 * pix + ch]) / Wn);
  }
  A.weight[p] = (float)Wn;
}

/* -------------------------------------------------------------------------------------------------- marching tetrahedra */
/* The triangles of a tetrahedron of even parity by case (bit n: corner v_n inside), each vertex an edge (lo << 2 | hi) of
 * the tetrahedron's corners: the rule of the public header, tabulated. */
struct TetCase {
  uint8_t n, e[6];
};
__device__ const TetCase TET_CASES[16] = {
    {0, {0x0, 0x0, 0x0, 0x0, 0x0, 0x0}},
    {1, {0x1, 0x2, 0x3, 0x0, 0x0, 0x0}},   /* case  1: (01,02,03) */
    {1, {0x1, 0x7, 0x6, 0x0, 0x0, 0x0}},   /* case  2: (01,13,12) */
    {2, {0x2, 0x3, 0x7, 0x2, 0x7, 0x6}},   /* case  3: (02,03,13) (02,13,12) */
    {1, {0x2, 0x6, 0xb, 0x0, 0x0, 0x0}},   /* case  4: (02,12,23) */
    {2, {0x3, 0x1, 0x6, 0x3, 0x6, 0xb}},   /* case  5: (03,01,12) (03,12,23) */
    {2, {0x1, 0x7, 0xb, 0x1, 0xb, 0x2}},   /* case  6: (01,13,23) (01,23,02) */
    {1, {0x3, 0x7, 0xb, 0x0, 0x0, 0x0}},   /* case  7: (03,13,23) */
    {1, {0x3, 0xb, 0x7, 0x0, 0x0, 0x0}},   /* case  8: (03,23,13) */
    {2, {0x1, 0x2, 0xb, 0x1, 0xb, 0x7}},   /* case  9: (01,02,23) (01,23,13) */
    {2, {0x6, 0x1, 0x3, 0x6, 0x3, 0xb}},   /* case 10: (12,01,03) (12,03,23) */
    {1, {0x2, 0xb, 0x6, 0x0, 0x0, 0x0}},   /* case 11: (02,23,12) */
    {2, {0x2, 0x6, 0x7, 0x2, 0x7, 0x3}},   /* case 12: (02,12,13) (02,13,03) */
    {1, {0x1, 0x6, 0x7, 0x0, 0x0, 0x0}},   /* case 13: (01,12,13) */
    {1, {0x1, 0x3, 0x2, 0x0, 0x0, 0x0}},   /* case 14: (01,03,02) */
    {0, {0x0, 0x0, 0x0, 0x0, 0x0, 0x0}},
};
/* tetrahedron n: the corner masks v1, v2 (v0 = 0, v3 = 7) of the axis orders xyz, xzy, yxz, yzx, zxy, zyx, and the parity */
__device__ const uint8_t TET_V1[6] = {1, 1, 2, 2, 4, 4};
__device__ const uint8_t TET_V2[6] = {3, 5, 3, 6, 5, 6};
__device__ const uint8_t TET_ODD[6] = {0, 1, 1, 0, 0, 1};

struct TsdfGridDims {
  int nx, ny, nz;
  __device__ long long step(int m) const {      /* the index distance to the neighbour p + m */
    return (m & 1) + (long long)((m >> 1) & 1) * nx + (long long)((m >> 2) & 1) * nx * ny;
  }
  __device__ bool cell(int i, int j, int k) const {
    return i >= 0 && j >= 0 && k >= 0 && i < nx - 1 && j < ny - 1 && k < nz - 1;
  }
};

__device__ inline bool tsdf_cell_observed(const float *weight, const TsdfGridDims &G, long long p, float min_weight) {
  bool ok = true;
  for (int m = 0; m < 8; ++m) ok = ok && (weight[p + G.step(m)] >= min_weight);
  return ok;
}

/* the case of tetrahedron n from the cell's 8 inside bits */
__device__ inline int tet_case(int inside, int n) {
  return (inside & 1) | (((inside >> TET_V1[n]) & 1) << 1) | (((inside >> TET_V2[n]) & 1) << 2) | (((inside >> 7) & 1) << 3);
}

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_mesh_flag_kernel(TsdfGridDims G, const float *tsdf, const float *weight, float iso,
                                                                    float min_weight, TsdfWorkspace ws) {
  __shared__ uint32_t s_v[TSDF_BLOCK], s_t[TSDF_BLOCK];
  const long long N = (long long)G.nx * G.ny * G.nz;
  const long long p = (long long)blockIdx.x * TSDF_BLOCK + threadIdx.x;
  uint32_t nv = 0, nt = 0;
  if (p < N) {
    int i, j, k;
    tsdf_voxel_of(p, G.nx, G.ny, &i, &j, &k);
    int inside = 0, have = 0;      /* bit m: the neighbour p + m exists / is inside */
    for (int m = 0; m < 8; ++m) {
      if (i + (m & 1) < G.nx && j + ((m >> 1) & 1) < G.ny && k + ((m >> 2) & 1) < G.nz) {
        have |= 1 << m;
        if (tsdf[p + G.step(m)] < iso) inside |= 1 << m;
      }
    }
    int mask = 0;
    const int in0 = inside & 1;
    for (int m = 1; m < 8; ++m) {
      if (!((have >> m) & 1) || ((inside >> m) & 1) == in0) continue;
      /* a contributing cell that has p and p + m as corners: its lowest corner is p - d for an axis set d disjoint from m */
      bool active = false;
      for (int d = 0; d < 8 && !active; ++d) {
        if (d & m) continue;
        const int ci = i - (d & 1), cj = j - ((d >> 1) & 1), ck = k - ((d >> 2) & 1);
        if (G.cell(ci, cj, ck)) active = tsdf_cell_observed(weight, G, p - G.step(d), min_weight);
      }
      if (active) mask |= 1 << (m - 1);
    }
    nv = (uint32_t)__popc(mask);
    if (have == 0xff && inside != 0 && inside != 0xff && tsdf_cell_observed(weight, G, p, min_weight)) {
      for (int n = 0; n < 6; ++n) nt += TET_CASES[tet_case(inside, n)].n;
      if (nt) mask |= 0x80;
    }
    ws.mask[p] = (uint8_t)mask;
    ws.voff[p] = nv;
    ws.toff[p] = nt;
  }
  s_v[threadIdx.x] = nv;
  s_t[threadIdx.x] = nt;
  __syncthreads();
  for (int s = TSDF_BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      s_v[threadIdx.x] += s_v[threadIdx.x + s];
      s_t[threadIdx.x] += s_t[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ws.vblk[blockIdx.x] = s_v[0];
    ws.tblk[blockIdx.x] = s_t[0];
  }
}

/* exclusive scan of TSDF_BLOCK values in LDS (all threads of the block call it); returns the total */
__device__ inline uint32_t tsdf_block_scan(uint32_t *s, uint32_t value, uint32_t *exclusive) {
  const int t = threadIdx.x;
  s[t] = value;
  __syncthreads();
  for (int off = 1; off < TSDF_BLOCK; off <<= 1) {
    const uint32_t add = t >= off ? s[t - off] : 0u;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  *exclusive = s[t] - value;
  const uint32_t total = s[TSDF_BLOCK - 1];
  __syncthreads();
  return total;
}

/* one block: the block sums become block offsets, the totals go to d_counts */
__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_mesh_scan_blocks_kernel(long long NB, TsdfWorkspace ws, long long *d_counts) {
  __shared__ uint32_t s[TSDF_BLOCK];
  unsigned long long carry_v = 0, carry_t = 0;
  for (long long base = 0; base < NB; base += TSDF_BLOCK) {
    const long long b = base + threadIdx.x;
    uint32_t ex;
    uint32_t total = tsdf_block_scan(s, b < NB ? ws.vblk[b] : 0u, &ex);
    if (b < NB) ws.vblk[b] = (uint32_t)(carry_v + ex);
    carry_v += total;
    total = tsdf_block_scan(s, b < NB ? ws.tblk[b] : 0u, &ex);
    if (b < NB) ws.tblk[b] = (uint32_t)(carry_t + ex);
    carry_t += total;
  }
  if (threadIdx.x == 0) {
    d_counts[0] = (long long)carry_v;
    d_counts[1] = (long long)carry_t;
  }
}

/* per block: counts -> offsets */
__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_mesh_scan_voxels_kernel(long long N, TsdfWorkspace ws) {
  __shared__ uint32_t s[TSDF_BLOCK];
  const long long p = (long long)blockIdx.x * TSDF_BLOCK + threadIdx.x;
  uint32_t ex;
  tsdf_block_scan(s, p < N ? ws.voff[p] : 0u, &ex);
  if (p < N) ws.voff[p] = ws.vblk[blockIdx.x] + ex;
  tsdf_block_scan(s, p < N ? ws.toff[p] : 0u, &ex);
  if (p < N) ws.toff[p] = ws.tblk[blockIdx.x] + ex;
}

__device__ inline int tet_corner(int r, int v1, int v2) { return r == 0 ? 0 : r == 1 ? v1 : r == 2 ? v2 : 7; }

struct TsdfEmitArgs {
  refnerf_tsdf_grid g;
  const float *tsdf, *rgb;
  float iso;
  TsdfWorkspace ws;
  long long n_vertices, n_triangles;
  float *vertices, *vertex_rgb;
  int32_t *triangles;
};

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_mesh_emit_kernel(TsdfEmitArgs A) {
  const TsdfGridDims G = {A.g.nx, A.g.ny, A.g.nz};
  const long long N = (long long)G.nx * G.ny * G.nz;
  const long long p = (long long)blockIdx.x * TSDF_BLOCK + threadIdx.x;
  if (p >= N) return;
  const int mask = A.ws.mask[p];
  if (!mask) return;
  int i, j, k;
  tsdf_voxel_of(p, G.nx, G.ny, &i, &j, &k);
  if (mask & 0x7f) {
    const double h = (double)A.g.voxel_size, iso = (double)A.iso;
    const double a = (double)A.tsdf[p] - iso;
    long long vi = A.ws.voff[p];
    for (int m = 1; m < 8; ++m) {
      if (!((mask >> (m - 1)) & 1)) continue;
      const long long q = p + G.step(m);
      if (vi < A.n_vertices) {
        const double b = (double)A.tsdf[q] - iso;
        const double t = a / (a - b);
        A.vertices[3 * vi + 0] = (float)((double)A.g.origin[0] + ((double)i + ((m & 1) ? t : 0.0)) * h);
        A.vertices[3 * vi + 1] = (float)((double)A.g.origin[1] + ((double)j + ((m & 2) ? t : 0.0)) * h);
        A.vertices[3 * vi + 2] = (float)((double)A.g.origin[2] + ((double)k + ((m & 4) ? t : 0.0)) * h);
        if (A.vertex_rgb) {
          for (int ch = 0; ch < 3; ++ch) {
            const double ca = (double)A.rgb[3 * p + ch], cb = (double)A.rgb[3 * q + ch];
            A.vertex_rgb[3 * vi + ch] = (float)(ca + t * (cb - ca));
          }
        }
      }
      ++vi;
    }
  }
  if (mask & 0x80) {      /* only cells inside the grid carry the bit: all 8 corners exist */
    int inside = 0;
    for (int m = 0; m < 8; ++m)
      if (A.tsdf[p + G.step(m)] < A.iso) inside |= 1 << m;
    long long ti = A.ws.toff[p];
    for (int n = 0; n < 6; ++n) {
      const TetCase tc = TET_CASES[tet_case(inside, n)];
      const int v1 = TET_V1[n], v2 = TET_V2[n];
      for (int r = 0; r < tc.n; ++r, ++ti) {
        if (ti >= A.n_triangles) continue;
        int32_t idx[3];
        for (int c = 0; c < 3; ++c) {
          const int lo = tet_corner(tc.e[3 * r + c] >> 2, v1, v2), hi = tet_corner(tc.e[3 * r + c] & 3, v1, v2);
          const long long base = p + G.step(lo);
          const int slot = (hi ^ lo) - 1;
          idx[c] = (int32_t)(A.ws.voff[base] + (uint32_t)__popc(A.ws.mask[base] & ((1 << slot) - 1)));
        }
        A.triangles[3 * ti + 0] = idx[0];
        A.triangles[3 * ti + 1] = idx[TET_ODD[n] ? 2 : 1];
        A.triangles[3 * ti + 2] = idx[TET_ODD[n] ? 1 : 2];
      }
    }
  }
}

}  // namespace rn
