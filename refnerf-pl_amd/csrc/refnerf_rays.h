/*
 * refnerf_rays.h -- on-device ray generation: the step in front of the path
 * (camera_utils.pixels_to_rays, internal/camera_utils.py:502-614, perspective
 * cameras, optionally with radial-tangential lens undistortion, :409-493 and
 * :558-565; optional NDC conversion, camera_utils.convert_to_ndc :31-97).  One
 * thread per pixel; 8 B in (pixel coordinates), 56 B out per ray -- HBM-bound,
 * trivially so for the pinhole instantiation.  image_rays_kernel below is the
 * whole-frame form: pixel coordinates from the flat index, all nine Rays fields
 * out (64 B per ray, nothing in), pinhole or spherical (cast_spherical_rays,
 * :700-746).
 */
#pragma once
#include <hip/hip_runtime.h>

namespace rn {

/* the keyword parameters of camera_utils._radial_and_tangential_undistort (:459-470) */
struct LensDistortion {
  double k1, k2, k3, k4, p1, p2, eps;
  int max_iterations;
};

struct RayGenArgs {
  const int *pix_x, *pix_y;
  const float *pixtocams;   /* [3,3] shared (stride 0) or per ray (stride 9) */
  const float *camtoworlds; /* [3,4] shared (stride 0) or per ray (stride 12) */
  const float *pixtocam_ndc; /* [3,3] or NULL */
  int p2c_stride, c2w_stride;
  int n;
  float *origins, *directions, *viewdirs, *radii, *imageplane;
  LensDistortion dist;      /* read by the distorted instantiation only */
};

/* camera_utils._radial_and_tangential_undistort on one point, in double (the reference's dataset path
 * computes in float64): Newton on the residual / Jacobian of _compute_residual_and_jacobian (:409-456),
 * in the reference's operation order; the step is taken only where |denominator| > eps (:480-491). */
__device__ __forceinline__ void undistort(const LensDistortion &D, float &xf, float &yf) {
  const double xd = xf, yd = yf;
  double x = xd, y = yd;
  for (int it = 0; it < D.max_iterations; ++it) {
    const double r = x * x + y * y;
    const double d = 1.0 + r * (D.k1 + r * (D.k2 + r * (D.k3 + r * D.k4)));
    const double fx = d * x + 2 * D.p1 * x * y + D.p2 * (r + 2 * x * x) - xd;
    const double fy = d * y + 2 * D.p2 * x * y + D.p1 * (r + 2 * y * y) - yd;
    const double d_r = D.k1 + r * (2.0 * D.k2 + r * (3.0 * D.k3 + r * 4.0 * D.k4));
    const double d_x = 2.0 * x * d_r, d_y = 2.0 * y * d_r;
    const double fx_x = d + d_x * x + 2.0 * D.p1 * y + 6.0 * D.p2 * x;
    const double fx_y = d_y * x + 2.0 * D.p1 * x + 2.0 * D.p2 * y;
    const double fy_x = d_x * y + 2.0 * D.p2 * y + 2.0 * D.p1 * x;
    const double fy_y = d + d_y * y + 2.0 * D.p2 * x + 6.0 * D.p1 * y;
    const double den = fy_x * fx_y - fx_x * fy_y;
    if (fabs(den) > D.eps) {
      x = x + (fx * fy_y - fy * fx_y) / den;
      y = y + (fy * fx_x - fx * fy_x) / den;
    }
  }
  xf = (float)x; yf = (float)y;
}

__device__ __forceinline__ void mat3_vec(const float *M, int ld, const float v[3], float out[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = (M[i * ld] * v[0] + M[i * ld + 1] * v[1]) + M[i * ld + 2] * v[2];
}

/* camera_utils.convert_to_ndc for one ray (near = 1) */
__device__ __forceinline__ void to_ndc(const float o_in[3], const float d[3], const float *p2c, float o_ndc[3], float d_ndc[3]) {
  const float t = -(1.0f + o_in[2]) / d[2];
  float o[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = o_in[i] + t * d[i];
  const float xm = 1.0f / p2c[2], ym = 1.0f / p2c[5];
  o_ndc[0] = xm * o[0] / o[2]; o_ndc[1] = ym * o[1] / o[2]; o_ndc[2] = -1.0f;
  const float inf[3] = {xm * d[0] / d[2], ym * d[1] / d[2], 1.0f};
#pragma unroll
  for (int i = 0; i < 3; ++i) d_ndc[i] = inf[i] - o_ndc[i];
}

/* One perspective ray from the integer pixel (x, y), the body every pinhole generator shares (pixels_to_rays_kernel here,
 * train_batch_kernel in refnerf_dataset.h), so that they agree bit for bit.  kDistort = false: the pinhole camera; true:
 * undistort the camera-space points first (distortion_params, :558-565).  `p2c` [3,3], `c2w` [3,4], `ndc` [3,3] or NULL;
 * `D` is read by the distorted instantiation only.  Out: origin, direction, viewdir, radius, imageplane (x, y). */
template <bool kDistort>
__device__ __forceinline__ void cast_pixel_ray(const float *p2c, const float *c2w, const float *ndc, const LensDistortion &D,
                                               const float x, const float y, float o[3], float d_out[3], float v_out[3],
                                               float &radius, float ip[2]) {
  float dir[3][3], cam0[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {                       /* the pixel and its +x / +y neighbours */
    const float pd[3] = {x + (q == 1 ? 1.0f : 0.0f) + 0.5f, y + (q == 2 ? 1.0f : 0.0f) + 0.5f, 1.0f};
    float cam[3];
    mat3_vec(p2c, 3, pd, cam);
    if constexpr (kDistort) {                         /* restacked with ones_like (:565) */
      undistort(D, cam[0], cam[1]);
      cam[2] = 1.0f;
    }
    cam[1] = -cam[1]; cam[2] = -cam[2];               /* OpenCV -> OpenGL */
    if (q == 0) { cam0[0] = cam[0]; cam0[1] = cam[1]; cam0[2] = cam[2]; }
    mat3_vec(c2w, 4, cam, dir[q]);
  }
  o[0] = c2w[3]; o[1] = c2w[7]; o[2] = c2w[11];
  const float nrm = sqrtf((dir[0][0] * dir[0][0] + dir[0][1] * dir[0][1]) + dir[0][2] * dir[0][2]);
  float dxn, dyn;
  if (ndc == nullptr) {
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = dir[1][c] - dir[0][c], b = dir[2][c] - dir[0][c];
      s1 += a * a; s2 += b * b;
      d_out[c] = dir[0][c];
    }
    dxn = sqrtf(s1); dyn = sqrtf(s2);
  } else {
    float ox[3], oy[3], on[3], tmp[3];
    to_ndc(o, dir[1], ndc, ox, tmp);
    to_ndc(o, dir[2], ndc, oy, tmp);
    to_ndc(o, dir[0], ndc, on, d_out);
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = ox[c] - on[c], b = oy[c] - on[c];
      s1 += a * a; s2 += b * b;
      o[c] = on[c];
    }
    dxn = sqrtf(s1); dyn = sqrtf(s2);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) v_out[c] = dir[0][c] / nrm;   /* from the world-space direction, before NDC */
  radius = (0.5f * (dxn + dyn)) * 2.0f / sqrtf(12.0f);
  ip[0] = cam0[0]; ip[1] = cam0[1];
}

template <bool kDistort>
__global__ void pixels_to_rays_kernel(const RayGenArgs A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const float *p2c = A.pixtocams + (size_t)i * A.p2c_stride;
  const float *c2w = A.camtoworlds + (size_t)i * A.c2w_stride;
  float o[3], d_out[3], v_out[3], radius, ip[2];
  cast_pixel_ray<kDistort>(p2c, c2w, A.pixtocam_ndc, A.dist, (float)A.pix_x[i], (float)A.pix_y[i], o, d_out, v_out, radius, ip);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    A.origins[(size_t)i * 3 + c] = o[c];
    A.directions[(size_t)i * 3 + c] = d_out[c];
    A.viewdirs[(size_t)i * 3 + c] = v_out[c];
  }
  A.radii[i] = radius;
  if (A.imageplane) { A.imageplane[(size_t)i * 2] = ip[0]; A.imageplane[(size_t)i * 2 + 1] = ip[1]; }
}

/* A whole frame's `Rays` from (width, height, camera, pose): Dataset.generate_ray_batch (internal/datasets.py:487-498)
 * for the flat, row-major pixel range [first, first + count) -- no pixel-index input, all nine fields in one launch. */
struct ImageRaysArgs {
  int width, height;
  long long first;          /* flat index of the first pixel of the range */
  int count;
  const float *pixtocam;    /* [3,3]; unused by the spherical instantiation */
  const float *camtoworld;  /* [3,4]: the frame's pose */
  const float *pixtocam_ndc; /* [3,3] or NULL (pinhole only) */
  float near, far;
  int cam_idx;
  float *origins, *directions, *viewdirs, *radii;             /* required */
  float *imageplane, *lossmult, *near_out, *far_out;          /* each may be NULL */
  int *cam_idx_out;                                           /* may be NULL */
  LensDistortion dist;      /* read by the distorted instantiation only */
};

/* kSpherical = false: the arithmetic of pixels_to_rays_kernel<kDistort>, expression for expression (the library is built
 * with -ffp-contract=off, so the five ray fields are the same bits), on the pixel (x, y) of the flat index.
 * kSpherical = true: camera_utils.cast_spherical_rays (:700-746): node (i, j) of the (height+1) x (width+1) grid looks along
 * (-sin phi sin theta, cos phi, sin phi cos theta), theta = 2 pi j / width, phi = pi i / height; dx / dy are the
 * differences to the j+1 / i+1 nodes.  The three directions and their differences are computed in double from the
 * float32 pose and rounded at the store: |dx| is a difference of unit vectors 2 pi / width apart, and its float32
 * cancellation error (6e-8 * width / 2 pi relative) would pass the generator's 2e-6 bar at a few hundred columns. */
template <bool kSpherical, bool kDistort>
__global__ void image_rays_kernel(const ImageRaysArgs A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.count) return;
  const long long flat = A.first + i;
  const int py = (int)(flat / A.width), px = (int)(flat - (long long)py * A.width);
  const float *c2w = A.camtoworld;
  float o[3] = {c2w[3], c2w[7], c2w[11]};
  float d_out[3], v_out[3], radius, ip[2];
  if constexpr (kSpherical) {
    const double kPi = 3.14159265358979323846;
    const double th0 = px * (2.0 * kPi / A.width), th1 = px + 1 == A.width ? 2.0 * kPi : (px + 1) * (2.0 * kPi / A.width);
    const double ph0 = py * (kPi / A.height), ph1 = py + 1 == A.height ? kPi : (py + 1) * (kPi / A.height);
    const double st0 = sin(th0), ct0 = cos(th0), st1 = sin(th1), ct1 = cos(th1);
    const double sp0 = sin(ph0), cp0 = cos(ph0), sp1 = sin(ph1), cp1 = cos(ph1);
    const double cam[3][3] = {{-sp0 * st0, cp0, sp0 * ct0},      /* the node, its j+1 and its i+1 neighbour */
                              {-sp0 * st1, cp0, sp0 * ct1},
                              {-sp1 * st0, cp1, sp1 * ct0}};
    double dir[3][3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int r = 0; r < 3; ++r)
        dir[q][r] = ((double)c2w[r * 4] * cam[q][0] + (double)c2w[r * 4 + 1] * cam[q][1]) + (double)c2w[r * 4 + 2] * cam[q][2];
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double a = dir[1][c] - dir[0][c], b = dir[2][c] - dir[0][c];
      s1 += a * a; s2 += b * b;
      d_out[c] = (float)dir[0][c];
      v_out[c] = d_out[c];                                /* viewdirs = directions, not renormalised (:725) */
    }
    radius = (float)((0.5 * (sqrt(s1) + sqrt(s2))) * 2.0 / sqrt(12.0));
    ip[0] = 0.0f; ip[1] = 0.0f;
  } else {
    const float *p2c = A.pixtocam;
    const float x = (float)px, y = (float)py;
    float dir[3][3], cam0[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {                       /* the pixel and its +x / +y neighbours */
      const float pd[3] = {x + (q == 1 ? 1.0f : 0.0f) + 0.5f, y + (q == 2 ? 1.0f : 0.0f) + 0.5f, 1.0f};
      float cam[3];
      mat3_vec(p2c, 3, pd, cam);
      if constexpr (kDistort) {
        undistort(A.dist, cam[0], cam[1]);
        cam[2] = 1.0f;
      }
      cam[1] = -cam[1]; cam[2] = -cam[2];               /* OpenCV -> OpenGL */
      if (q == 0) { cam0[0] = cam[0]; cam0[1] = cam[1]; cam0[2] = cam[2]; }
      mat3_vec(c2w, 4, cam, dir[q]);
    }
    const float nrm = sqrtf((dir[0][0] * dir[0][0] + dir[0][1] * dir[0][1]) + dir[0][2] * dir[0][2]);
    float dxn, dyn;
    if (A.pixtocam_ndc == nullptr) {
      float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float a = dir[1][c] - dir[0][c], b = dir[2][c] - dir[0][c];
        s1 += a * a; s2 += b * b;
        d_out[c] = dir[0][c];
      }
      dxn = sqrtf(s1); dyn = sqrtf(s2);
    } else {
      float ox[3], oy[3], on[3], tmp[3];
      to_ndc(o, dir[1], A.pixtocam_ndc, ox, tmp);
      to_ndc(o, dir[2], A.pixtocam_ndc, oy, tmp);
      to_ndc(o, dir[0], A.pixtocam_ndc, on, d_out);
      float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float a = ox[c] - on[c], b = oy[c] - on[c];
        s1 += a * a; s2 += b * b;
        o[c] = on[c];
      }
      dxn = sqrtf(s1); dyn = sqrtf(s2);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v_out[c] = dir[0][c] / nrm;   /* from the world-space direction, before NDC */
    radius = (0.5f * (dxn + dyn)) * 2.0f / sqrtf(12.0f);
    ip[0] = cam0[0]; ip[1] = cam0[1];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    A.origins[(size_t)i * 3 + c] = o[c];
    A.directions[(size_t)i * 3 + c] = d_out[c];
    A.viewdirs[(size_t)i * 3 + c] = v_out[c];
  }
  A.radii[i] = radius;
  if (A.imageplane) { A.imageplane[(size_t)i * 2] = ip[0]; A.imageplane[(size_t)i * 2 + 1] = ip[1]; }
  if (A.lossmult) A.lossmult[i] = 1.0f;
  if (A.near_out) A.near_out[i] = A.near;
  if (A.far_out) A.far_out[i] = A.far;
  if (A.cam_idx_out) A.cam_idx_out[i] = A.cam_idx;
}

}  // namespace rn
