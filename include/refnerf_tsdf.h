/*
 * refnerf_tsdf.h -- C ABI of geometry export in librefnerf_hip.so: fusion of rendered depth maps into a truncated signed
 * distance function (TSDF) on a voxel grid, and extraction of its iso-surface as an indexed triangle mesh by marching
 * tetrahedra.  A header of its own next to refnerf_hip.h: the same library, the same conventions --
 * device pointers to contiguous rows, `stream` a hipStream_t (NULL: the default stream), no allocation, 64-bit offsets, one
 * fixed order of operations, and the return codes of refnerf_hip.h: 0 (REFNERF_OK), -1 (REFNERF_EINVAL, text in
 * refnerf_last_error()), -3 (REFNERF_EHIP).  No entry synchronises with the host, with one exception named below
 * (refnerf_tsdf_integrate reads the 36 bytes of d_pixtocam).
 *
 * THE GRID.  Voxel (i, j, k), 0 <= i < nx, 0 <= j < ny, 0 <= k < nz, has its centre at origin + (i, j, k) * voxel_size and
 * lives at linear index (k * ny + j) * nx + i.  REFNERF_EINVAL: a dimension < 2, 7 * nx * ny * nz >= 2^31, a voxel_size or
 * trunc that is not a positive finite number, a non-finite origin.
 *
 * ARITHMETIC.  Every entry computes in double from the float32 inputs, without contraction, in exactly the order written
 * here (`a + b + c` is `(a + b) + c`), and rounds each value once to float32 at the store: a float64 restatement of these
 * lines gives the same bits, every branch included.
 *
 * refnerf_tsdf_integrate: fuses one view.  R[r][c] = m[4 r + c] and c[r] = m[4 r + 3] of m = d_camtoworlds + 12 * frame;
 * pixtocam = [[a, b, c], [d, e, f], [0, 0, 1]].  Per voxel:
 *     P      = (origin[0] + i * h, origin[1] + j * h, origin[2] + k * h),   h = voxel_size;        dx, dy, dz = P - c
 *     q0     =   R[0][0] * dx + R[1][0] * dy + R[2][0] * dz
 *     q1     = -(R[0][1] * dx + R[1][1] * dy + R[2][1] * dz)                (the OpenCV camera frame: the inverse of the
 *     z      = -(R[0][2] * dx + R[1][2] * dy + R[2][2] * dz)                 flip in camera_utils.pixels_to_rays)
 *     skip unless z > z_min
 *     det    = a * e - b * d;   u = ((e / det) * q0 + (-b / det) * q1 + ((b * f - c * e) / det) * z) / z
 *                               v = ((-d / det) * q0 + (a / det) * q1 + ((c * d - a * f) / det) * z) / z
 *     x, y   = floor(u), floor(v)   (rays go through x + .5, y + .5);   skip unless 0 <= x < width and 0 <= y < height
 *     D      = d_depth[y][x];   skip unless D is finite and D > 0;   skip if d_acc and d_acc[y][x] < acc_min
 *     sdf    = D - z;   skip if sdf < -trunc;   obs = min(1, sdf / trunc)
 *     W      = d_weight[p];   Wn = W + view_weight
 *     d_tsdf[p] = (W * d_tsdf[p] + view_weight * obs) / Wn;   d_rgb[p][ch] = (W * d_rgb[p][ch] + view_weight * d_view_rgb[y][x][ch]) / Wn
 *     d_weight[p] = Wn
 * A skipped voxel is not written.  D is the rendering's distance along Rays.directions, whose camera-space z is exactly 1
 * when the third row of pixtocam is (0, 0, 1): D is then the z-depth.  The entry reads d_pixtocam back (36 bytes, ordered
 * on `stream`: the one host synchronisation of this header) and refuses any other third row or a zero `det`.
 * d_rgb and d_view_rgb are given together or both NULL; d_acc may be NULL.
 * REFNERF_EINVAL: a bad grid, a NULL required pointer, d_rgb without d_view_rgb or the reverse, a non-positive width or
 * height, frame outside [0, n_frames), view_weight not > 0, z_min not >= 0, a pixtocam as above.
 *
 * MESH.  Corner p is inside iff d_tsdf[p] < iso.  Cell (i, j, k) (i < nx - 1, ...; its index is its lowest voxel's) has the
 * corners p + m, m a bit mask of axes (1 = x, 2 = y, 4 = z); it contributes iff all eight corners have d_weight >=
 * min_weight.  It is cut into the six tetrahedra of the Kuhn decomposition, tetrahedron n = 0..5 for the n-th axis order
 * (a, b, c) in lexicographic order (xyz, xzy, yxz, yzx, zxy, zyx), with the corners v0 = 0, v1 = a, v2 = a | b, v3 = 7;
 * its parity is that of the permutation (+ - - + + -).  A mesh vertex lives on a grid edge: voxel p, slot s = m - 1 for
 * the edge from p to p + m (7 slots: x, y, xy, z, xz, yz, xyz).  The edge is active iff its two ends differ in insideness
 * and a contributing cell has both as corners.  Vertices are numbered by (voxel index, slot), and with A = d_tsdf[p] - iso,
 * B = d_tsdf[p + m] - iso, t = A / (A - B):   position[axis] = origin[axis] + (index[axis] + (m has axis ? t : 0)) * h,
 * colour[ch] = ca + t * (cb - ca).  Triangles are numbered by (cell index, tetrahedron, triangle).  With e(r, s) the vertex
 * on the edge between the tetrahedron's corners v_r and v_s, a tetrahedron of even parity emits
 *     one corner i inside:       (e(i, j), e(i, k), e(i, l))            j < k < l the others, k and l exchanged if the
 *     one corner i outside:      (e(i, j), e(i, l), e(i, k))            permutation (i, j, k, l) of (0, 1, 2, 3) is odd
 *     i < j inside, k < l out:   (e(i, k), e(i, l), e(j, l)) and (e(i, k), e(j, l), e(j, k)),   k and l exchanged likewise
 * and one of odd parity the same with the last two vertices of every triangle exchanged: the normal points towards
 * increasing tsdf, decided by the case alone, also where a triangle has no area.
 *
 * refnerf_tsdf_mesh_workspace_bytes: the workspace of one grid, 0 for a bad grid: two 32-bit offsets and a mask byte per
 * voxel plus two offsets per 256 voxels (9.03 bytes per voxel; 151.5 MB at 256^3).
 * refnerf_tsdf_mesh_count: flags the active edges, counts, scans; d_counts (device int64[2]) = {n_vertices, n_triangles}.
 * refnerf_tsdf_mesh_emit: d_vertices [n_vertices][3], d_vertex_rgb [n_vertices][3] (may be NULL; needs d_rgb),
 * d_triangles [n_triangles][3] int32, from the workspace refnerf_tsdf_mesh_count filled for the same grid, d_tsdf and iso;
 * n_vertices and n_triangles are the counts it wrote (nothing is stored past them).  With both 0 nothing is launched.
 * REFNERF_EINVAL: a bad grid, a NULL required pointer, a workspace smaller than the query says or not 4-byte aligned, a non-finite iso or
 * min_weight, negative counts or n_vertices >= 2^31, d_vertex_rgb without d_rgb.
 */
#ifndef REFNERF_TSDF_H
#define REFNERF_TSDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct refnerf_tsdf_grid {
  int32_t nx, ny, nz;
  float origin[3];  /* the centre of voxel (0, 0, 0) */
  float voxel_size;
  float trunc;      /* world units, > 0 */
} refnerf_tsdf_grid;

int refnerf_tsdf_integrate(const refnerf_tsdf_grid *grid, float *d_tsdf /* [nz][ny][nx] */, float *d_weight /* [nz][ny][nx] */,
                           float *d_rgb /* [nz][ny][nx][3] or NULL */, const float *d_pixtocam /* [3][3] */,
                           const float *d_camtoworlds /* [n_frames][3][4] */, int32_t n_frames, int32_t frame, int32_t width,
                           int32_t height, const float *d_depth /* [H][W] */, const float *d_acc /* [H][W] or NULL */,
                           float acc_min, const float *d_view_rgb /* [H][W][3] or NULL */, float view_weight, float z_min,
                           void *stream);

size_t refnerf_tsdf_mesh_workspace_bytes(const refnerf_tsdf_grid *grid);
int refnerf_tsdf_mesh_count(const refnerf_tsdf_grid *grid, const float *d_tsdf, const float *d_weight, float iso,
                            float min_weight, void *d_workspace, size_t workspace_bytes, int64_t *d_counts /* [2] */,
                            void *stream);
int refnerf_tsdf_mesh_emit(const refnerf_tsdf_grid *grid, const float *d_tsdf, const float *d_rgb /* or NULL */, float iso,
                           const void *d_workspace, size_t workspace_bytes, int64_t n_vertices, int64_t n_triangles,
                           float *d_vertices, float *d_vertex_rgb /* or NULL */, int32_t *d_triangles, void *stream);

#ifdef __cplusplus
}
#endif
#endif
