/*
 * refnerf_raycast.hip -- fifth translation unit of librefnerf_hip.so: the TSDF ray caster (refnerf_raycast.h) and its C entry
 * (include/refnerf_raycast.h).  A unit of its own, so the code objects of the other four stay what they are.  Errors go
 * through rnh::fail (refnerf_sq_host.h): refnerf_last_error() reports them like every other entry's.
 */
#include <hip/hip_runtime.h>

#include <cmath>

#include "refnerf_hip.h"
#include "refnerf_raycast.h"   /* the kernel (this directory comes first on the include path); it includes the C declarations */
#include "refnerf_sq_host.h"

namespace {
/* the grid rule of include/refnerf_tsdf.h */
bool grid_ok(const refnerf_tsdf_grid *g) {
  if (!g || g->nx < 2 || g->ny < 2 || g->nz < 2) return false;
  if (7LL * g->nx * g->ny >= (1LL << 31) || 7LL * g->nx * g->ny * g->nz >= (1LL << 31)) return false;
  if (!(g->voxel_size > 0.0f && std::isfinite(g->voxel_size) && g->trunc > 0.0f && std::isfinite(g->trunc))) return false;
  return std::isfinite(g->origin[0]) && std::isfinite(g->origin[1]) && std::isfinite(g->origin[2]);
}
}  // namespace

extern "C" int refnerf_tsdf_raycast(const refnerf_tsdf_grid *grid, const float *d_tsdf, const float *d_weight, const float *d_rgb,
                                    const float *d_pixtocam, const float *d_camtoworlds, int32_t n_frames, int32_t frame, int32_t width,
                                    int32_t height, float iso, float min_weight, float step, int32_t refine, float t_near, float t_far,
                                    float *d_depth, float *d_normals, float *d_view_rgb, float *d_acc, void *stream) {
  const char *fn = "refnerf_tsdf_raycast";
  if (!grid_ok(grid))
    return rnh::fail(REFNERF_EINVAL, "%s: grid: dimensions >= 2 with 7 nx ny nz < 2^31, a finite origin, voxel_size > 0 and trunc > 0 are required", fn);
  if (!d_tsdf || !d_weight || !d_pixtocam || !d_camtoworlds || !d_depth || !d_normals || !d_acc)
    return rnh::fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (d_view_rgb && !d_rgb) return rnh::fail(REFNERF_EINVAL, "%s: d_view_rgb needs d_rgb", fn);
  if (width < 1 || height < 1) return rnh::fail(REFNERF_EINVAL, "%s: width and height must be positive", fn);
  if (n_frames < 1 || frame < 0 || frame >= n_frames) return rnh::fail(REFNERF_EINVAL, "%s: frame outside [0, n_frames)", fn);
  if (!std::isfinite(iso) || !std::isfinite(min_weight)) return rnh::fail(REFNERF_EINVAL, "%s: iso and min_weight must be finite", fn);
  if (!(step >= 1.0f / 64.0f && step <= 64.0f)) return rnh::fail(REFNERF_EINVAL, "%s: step must lie in [1/64, 64] voxels", fn);
  if (refine < 0 || refine > 32) return rnh::fail(REFNERF_EINVAL, "%s: refine outside [0, 32]", fn);
  if (!(t_near >= 0.0f)) return rnh::fail(REFNERF_EINVAL, "%s: t_near must be >= 0", fn);
  if (std::isnan(t_far)) return rnh::fail(REFNERF_EINVAL, "%s: t_far is NaN", fn);
  rn::TsdfRaycastArgs A;
  A.g = *grid;
  A.tsdf = d_tsdf, A.weight = d_weight, A.rgb = d_rgb;
  A.pixtocam = d_pixtocam, A.pose = d_camtoworlds + 12 * (long long)frame;
  A.width = width, A.height = height, A.refine = refine;
  A.iso = iso, A.min_weight = min_weight, A.step = step, A.t_near = t_near, A.t_far = t_far;
  A.depth = d_depth, A.normals = d_normals, A.view_rgb = d_view_rgb, A.acc = d_acc;
  const long long bx = ((long long)width + rn::RAYCAST_BLOCK_SIDE - 1) / rn::RAYCAST_BLOCK_SIDE;
  const long long by = ((long long)height + rn::RAYCAST_BLOCK_SIDE - 1) / rn::RAYCAST_BLOCK_SIDE;
  if (by > 65535) return rnh::fail(REFNERF_EINVAL, "%s: height above 16 * 65535", fn);
  const dim3 blocks((unsigned)bx, (unsigned)by), threads(rn::RAYCAST_BLOCK);
  if (d_view_rgb)
    hipLaunchKernelGGL(rn::tsdf_raycast_kernel<true>, blocks, threads, 0, (hipStream_t)stream, A);
  else
    hipLaunchKernelGGL(rn::tsdf_raycast_kernel<false>, blocks, threads, 0, (hipStream_t)stream, A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return rnh::fail(REFNERF_EHIP, "refnerf_tsdf_raycast: launch: %s", hipGetErrorString(e));
  return REFNERF_OK;
}
