/*
 * refnerf_tsdf.hip -- fourth translation unit of librefnerf_hip.so: TSDF fusion and marching tetrahedra (refnerf_tsdf.h) and
 * their C entries (include/refnerf_tsdf.h).  A unit of its own, so the code objects of the other three stay what they are.
 * Errors go through rnh::fail (refnerf_sq_host.h): refnerf_last_error() reports them like every other entry's.
 */
#include <hip/hip_runtime.h>

#include <cmath>

#include "refnerf_hip.h"
#include "refnerf_tsdf.h"      /* the kernels (this directory comes first on the include path); it includes the C declarations */
#include "refnerf_sq_host.h"

#define TSDF_HIP_TRY(expr)                                                   \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess) return rnh::fail(REFNERF_EHIP, #expr ": %s", hipGetErrorString(e_)); \
  } while (0)

namespace {
bool grid_ok(const refnerf_tsdf_grid *g) {
  if (!g || g->nx < 2 || g->ny < 2 || g->nz < 2) return false;
  if (7LL * g->nx * g->ny >= (1LL << 31) || 7LL * g->nx * g->ny * g->nz >= (1LL << 31)) return false;
  if (!(g->voxel_size > 0.0f && std::isfinite(g->voxel_size) && g->trunc > 0.0f && std::isfinite(g->trunc))) return false;
  return std::isfinite(g->origin[0]) && std::isfinite(g->origin[1]) && std::isfinite(g->origin[2]);
}
int check_grid(const char *fn, const refnerf_tsdf_grid *g) {
  if (!grid_ok(g))
    return rnh::fail(REFNERF_EINVAL, "%s: grid: dimensions >= 2 with 7 nx ny nz < 2^31, a finite origin, voxel_size > 0 and trunc > 0 are required", fn);
  return REFNERF_OK;
}
long long voxels(const refnerf_tsdf_grid *g) { return (long long)g->nx * g->ny * g->nz; }
}  // namespace

extern "C" int refnerf_tsdf_integrate(const refnerf_tsdf_grid *grid, float *d_tsdf, float *d_weight, float *d_rgb, const float *d_pixtocam,
                                      const float *d_camtoworlds, int32_t n_frames, int32_t frame, int32_t width, int32_t height,
                                      const float *d_depth, const float *d_acc, float acc_min, const float *d_view_rgb,
                                      float view_weight, float z_min, void *stream) {
  const char *fn = "refnerf_tsdf_integrate";
  if (int rc = check_grid(fn, grid)) return rc;
  if (!d_tsdf || !d_weight || !d_pixtocam || !d_camtoworlds || !d_depth) return rnh::fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if ((d_rgb == nullptr) != (d_view_rgb == nullptr))
    return rnh::fail(REFNERF_EINVAL, "%s: d_rgb and d_view_rgb are given together or both NULL", fn);
  if (width < 1 || height < 1) return rnh::fail(REFNERF_EINVAL, "%s: width and height must be positive", fn);
  if (n_frames < 1 || frame < 0 || frame >= n_frames) return rnh::fail(REFNERF_EINVAL, "%s: frame outside [0, n_frames)", fn);
  if (!(view_weight > 0.0f) || !std::isfinite(view_weight)) return rnh::fail(REFNERF_EINVAL, "%s: view_weight must be a positive finite number", fn);
  if (!(z_min >= 0.0f) || !std::isfinite(z_min)) return rnh::fail(REFNERF_EINVAL, "%s: z_min must be a finite number >= 0", fn);
  if (std::isnan(acc_min)) return rnh::fail(REFNERF_EINVAL, "%s: acc_min is NaN", fn);
  hipStream_t st = (hipStream_t)stream;
  float k[9];
  TSDF_HIP_TRY(hipMemcpyAsync(k, d_pixtocam, sizeof(k), hipMemcpyDeviceToHost, st));
  TSDF_HIP_TRY(hipStreamSynchronize(st));
  if (!(k[6] == 0.0f && k[7] == 0.0f && k[8] == 1.0f))
    return rnh::fail(REFNERF_EINVAL, "%s: the third row of pixtocam must be (0, 0, 1): the depth is a z-depth only then", fn);
  const double det = (double)k[0] * (double)k[4] - (double)k[1] * (double)k[3];
  if (!(det != 0.0) || !std::isfinite(det)) return rnh::fail(REFNERF_EINVAL, "%s: pixtocam is singular or not finite", fn);
  rn::TsdfIntegrateArgs A;
  A.g = *grid;
  A.tsdf = d_tsdf, A.weight = d_weight, A.rgb = d_rgb;
  A.pixtocam = d_pixtocam, A.pose = d_camtoworlds + 12 * (long long)frame;
  A.depth = d_depth, A.acc = d_acc, A.view_rgb = d_view_rgb;
  A.width = width, A.height = height;
  A.acc_min = acc_min, A.view_weight = view_weight, A.z_min = z_min;
  hipLaunchKernelGGL(rn::tsdf_integrate_kernel, dim3((unsigned)rn::tsdf_blocks(voxels(grid))), dim3(rn::TSDF_BLOCK), 0, st, A);
  TSDF_HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

extern "C" size_t refnerf_tsdf_mesh_workspace_bytes(const refnerf_tsdf_grid *grid) {
  return grid_ok(grid) ? rn::tsdf_workspace_bytes(voxels(grid)) : 0;
}

extern "C" int refnerf_tsdf_mesh_count(const refnerf_tsdf_grid *grid, const float *d_tsdf, const float *d_weight, float iso,
                                       float min_weight, void *d_workspace, size_t workspace_bytes, int64_t *d_counts, void *stream) {
  const char *fn = "refnerf_tsdf_mesh_count";
  if (int rc = check_grid(fn, grid)) return rc;
  if (!d_tsdf || !d_weight || !d_workspace || !d_counts) return rnh::fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (!std::isfinite(iso) || !std::isfinite(min_weight)) return rnh::fail(REFNERF_EINVAL, "%s: iso and min_weight must be finite", fn);
  const long long N = voxels(grid);
  if (workspace_bytes < rn::tsdf_workspace_bytes(N) || (uintptr_t)d_workspace % 4)
    return rnh::fail(REFNERF_EINVAL, "%s: the workspace is smaller than refnerf_tsdf_mesh_workspace_bytes says, or not 4-byte aligned", fn);
  hipStream_t st = (hipStream_t)stream;
  const rn::TsdfWorkspace ws = rn::tsdf_workspace(d_workspace, N);
  const rn::TsdfGridDims G = {grid->nx, grid->ny, grid->nz};
  const long long NB = rn::tsdf_blocks(N);
  hipLaunchKernelGGL(rn::tsdf_mesh_flag_kernel, dim3((unsigned)NB), dim3(rn::TSDF_BLOCK), 0, st, G, d_tsdf, d_weight, iso, min_weight, ws);
  hipLaunchKernelGGL(rn::tsdf_mesh_scan_blocks_kernel, dim3(1), dim3(rn::TSDF_BLOCK), 0, st, NB, ws, (long long *)d_counts);
  hipLaunchKernelGGL(rn::tsdf_mesh_scan_voxels_kernel, dim3((unsigned)NB), dim3(rn::TSDF_BLOCK), 0, st, N, ws);
  TSDF_HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

extern "C" int refnerf_tsdf_mesh_emit(const refnerf_tsdf_grid *grid, const float *d_tsdf, const float *d_rgb, float iso,
                                      const void *d_workspace, size_t workspace_bytes, int64_t n_vertices, int64_t n_triangles,
                                      float *d_vertices, float *d_vertex_rgb, int32_t *d_triangles, void *stream) {
  const char *fn = "refnerf_tsdf_mesh_emit";
  if (int rc = check_grid(fn, grid)) return rc;
  if (n_vertices < 0 || n_triangles < 0 || n_vertices >= (1LL << 31))
    return rnh::fail(REFNERF_EINVAL, "%s: n_vertices outside [0, 2^31) or n_triangles < 0", fn);
  if (!std::isfinite(iso)) return rnh::fail(REFNERF_EINVAL, "%s: iso must be finite", fn);
  const long long N = voxels(grid);
  if (workspace_bytes < rn::tsdf_workspace_bytes(N) || (uintptr_t)d_workspace % 4)
    return rnh::fail(REFNERF_EINVAL, "%s: the workspace is smaller than refnerf_tsdf_mesh_workspace_bytes says, or not 4-byte aligned", fn);
  if (d_vertex_rgb && !d_rgb) return rnh::fail(REFNERF_EINVAL, "%s: d_vertex_rgb needs d_rgb", fn);
  if (n_vertices == 0 && n_triangles == 0) return REFNERF_OK;
  if (!d_tsdf || !d_workspace || (n_vertices && !d_vertices) || (n_triangles && !d_triangles))
    return rnh::fail(REFNERF_EINVAL, "%s: null pointer", fn);
  rn::TsdfEmitArgs A;
  A.g = *grid;
  A.tsdf = d_tsdf, A.rgb = d_rgb, A.iso = iso;
  A.ws = rn::tsdf_workspace(const_cast<void *>(d_workspace), N);
  A.n_vertices = n_vertices, A.n_triangles = n_triangles;
  A.vertices = d_vertices, A.vertex_rgb = d_vertex_rgb, A.triangles = d_triangles;
  hipLaunchKernelGGL(rn::tsdf_mesh_emit_kernel, dim3((unsigned)rn::tsdf_blocks(N)), dim3(rn::TSDF_BLOCK), 0, (hipStream_t)stream, A);
  TSDF_HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}
