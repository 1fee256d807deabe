/*
 * refnerf_raycast.h -- C ABI of TSDF ray casting in librefnerf_hip.so: the fused volume of refnerf_tsdf.h rendered back
 * into depth, normal and colour images of a pinhole view.  A header of its own next to
 * refnerf_tsdf.h, whose grid struct it uses: the same library, the same conventions -- device pointers to contiguous rows,
 * `stream` a hipStream_t (NULL: the default stream), no allocation, 64-bit voxel and pixel offsets, one fixed order of
 * operations, and the return codes of refnerf_hip.h: 0 (REFNERF_OK), -1 (REFNERF_EINVAL, text in refnerf_last_error()),
 * -3 (REFNERF_EHIP).  The entry never synchronises with the host: d_pixtocam is read on the device, and only its first two
 * rows are (the camera looks along cz = -1 whatever the third row holds).
 *
 * ARITHMETIC.  Everything is computed in double from the float32 inputs, without contraction, in exactly the order written
 * here (`a + b + c` is `(a + b) + c`), sqrt and / correctly rounded, and each stored value is rounded once to float32: a
 * float64 restatement of these lines gives the same bits, every branch included.  min(a, b) is `a < b ? a : b` and
 * max(a, b) is `a > b ? a : b`.
 *
 * refnerf_tsdf_raycast: one view of the grid (THE GRID of refnerf_tsdf.h).  R[r][c] = m[4 r + c] and c[r] = m[4 r + 3] of
 * m = d_camtoworlds + 12 * frame, K = d_pixtocam, h = voxel_size, n = (nx, ny, nz).  Per pixel (x, y), 0 <= x < width,
 * 0 <= y < height, stored at row y, column x:
 *     px, py = x + .5, y + .5
 *     cx     =   K[0][0] * px + K[0][1] * py + K[0][2]
 *     cy     = -(K[1][0] * px + K[1][1] * py + K[1][2]);   cz = -1             (camera_utils.pixels_to_rays)
 *     d[a]   = R[a][0] * cx + R[a][1] * cy + R[a][2] * cz;   o = c              (the unnormalised Rays.directions: t below is
 *                                                                               the distance refnerf_tsdf_integrate calls depth)
 *   BOX, per axis a:   lo = origin[a];   hi = origin[a] + (n[a] - 1) * h
 *   SLAB TEST, from t0 = t_near, t1 = t_far, axis 0, 1, 2 in turn:
 *     d[a] == 0:   the ray misses unless lo <= o[a] and o[a] <= hi; the axis sets no bound
 *     otherwise:   ta = (lo - o[a]) / d[a];   tb = (hi - o[a]) / d[a]
 *                  t0 = max(t0, min(ta, tb));   t1 = min(t1, max(ta, tb))
 *     the ray misses unless t1 >= t0
 *   STEPS:   dt = step * h / sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);   N = floor((t1 - t0) / dt)
 *     the samples are t_k = t0 + k * dt, k = 0 .. N (a product, not a running sum).  The ray misses unless
 *     N <= (nx + ny + nz) / step: finite inputs stay far below (the box's diagonal is shorter than (nx + ny + nz) h), so
 *     this line only ends a ray whose pose or pixtocam is not finite.
 *   SAMPLE at t:   P[a] = o[a] + t * d[a];   g[a] = (P[a] - origin[a]) / h
 *     i[a]  = min(max(floor(g[a]), 0), n[a] - 2)   (0 for a NaN; the clamp keeps a rounding at a box face inside the grid)
 *     fr[a] = g[a] - i[a]
 *     c[m]  = d_tsdf[p + m], m = 0 .. 7 the corners of the cell p = (i[0], i[1], i[2]) as in MESH of refnerf_tsdf.h
 *             (bit 0 = x, 1 = y, 2 = z)
 *     valid iff all eight corners have d_weight >= min_weight
 *     x_q   = c[2 q] + fr[0] * (c[2 q + 1] - c[2 q]), q = 0 .. 3;   y_r = x_{2 r} + fr[1] * (x_{2 r + 1} - x_{2 r}), r = 0, 1
 *     v     = (y_0 + fr[2] * (y_1 - y_0)) - iso
 *   MARCH, k = 0 .. N:   an invalid sample clears "previous valid".  A valid sample with v < 0 after a valid previous
 *     sample with v_prev >= 0 is the hit bracket (a, b) = (t_{k-1}, t_k), (fa, fb) = (v_prev, v): a front face, from free
 *     space into the surface.  Any other valid sample becomes the previous one.  Crossings from inside to outside are
 *     ignored, and a ray that starts inside hits nothing until it has been outside.  No bracket: a miss.
 *   REFINE, `refine` times:   tm = 0.5 * (a + b);   vm = v of the sample at tm, valid or not;
 *     vm < 0: (b, fb) = (tm, vm);   otherwise: (a, fa) = (tm, vm)
 *   HIT:   t* = a + (fa / (fa - fb)) * (b - a);   c, fr of the sample at t*;   u[a] = 1 - fr[a]
 *     gx = u[1] * u[2] * (c[1] - c[0]) + fr[1] * u[2] * (c[3] - c[2]) + u[1] * fr[2] * (c[5] - c[4]) + fr[1] * fr[2] * (c[7] - c[6])
 *     gy = u[0] * u[2] * (c[2] - c[0]) + fr[0] * u[2] * (c[3] - c[1]) + u[0] * fr[2] * (c[6] - c[4]) + fr[0] * fr[2] * (c[7] - c[5])
 *     gz = u[0] * u[1] * (c[4] - c[0]) + fr[0] * u[1] * (c[5] - c[1]) + u[0] * fr[1] * (c[6] - c[2]) + fr[0] * fr[1] * (c[7] - c[3])
 *     (`p * q * r` is `(p * q) * r`: the gradient of the trilinear interpolant in that cell, without its common 1 / h)
 *     s = sqrt(gx * gx + gy * gy + gz * gz)
 *     d_depth = t*;   d_acc = 1;   d_normals = (gx / s, gy / s, gz / s) if s > 0, else 0: towards increasing tsdf, free space
 *     d_view_rgb[ch] = the x, y, z lerps above on the corner colours d_rgb[p + m][ch], with the same fr
 *   MISS:   d_depth = 0, d_normals = 0, d_view_rgb = 0, d_acc = 0.  Every output element is written on every path.
 * d_view_rgb may be NULL; it needs d_rgb.  t_far may be +inf, and t_far < t_near is legal: every ray misses.
 * REFNERF_EINVAL: a bad grid, a NULL required pointer, d_view_rgb without d_rgb, a non-positive width or height, a height
 * above 16 * 65535 (the launch grid's limit), frame outside [0, n_frames), a non-finite iso or min_weight, step not finite
 * or outside [1/64, 64] (which bounds the loop), refine outside [0, 32], t_near not >= 0 (a NaN included), t_far NaN.
 */
#ifndef REFNERF_RAYCAST_H
#define REFNERF_RAYCAST_H

#include <stdint.h>

#include "refnerf_tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

int refnerf_tsdf_raycast(const refnerf_tsdf_grid *grid, const float *d_tsdf, const float *d_weight,
                         const float *d_rgb /* [nz][ny][nx][3] or NULL */, const float *d_pixtocam /* [3][3] */,
                         const float *d_camtoworlds /* [n_frames][3][4] */, int32_t n_frames, int32_t frame,
                         int32_t width, int32_t height, float iso, float min_weight, float step /* voxels */,
                         int32_t refine, float t_near, float t_far /* +inf allowed */,
                         float *d_depth /* [H][W] */, float *d_normals /* [H][W][3] */,
                         float *d_view_rgb /* [H][W][3] or NULL; needs d_rgb */, float *d_acc /* [H][W] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif
