/*
 * refnerf_distortion.hip -- third translation unit of librefnerf_hip.so: the distortion loss (refnerf_distortion.h) and its
 * two C entries (include/refnerf_distortion.h).  A unit of its own, so the code objects of the other two stay what they are.
 * Errors go through rnh::fail (refnerf_sq_host.h): refnerf_last_error() reports them like every other entry's.
 */
#include <hip/hip_runtime.h>

#include "refnerf_hip.h"
#include "refnerf_distortion.h"      /* the kernels (this directory comes first on the include path ...) */
#include "../../include/refnerf_distortion.h"      /* ... and the C declarations */
#include "refnerf_sq_host.h"

#define DIST_HIP_TRY(expr)                                                   \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess) return rnh::fail(REFNERF_EHIP, #expr ": %s", hipGetErrorString(e_)); \
  } while (0)

namespace {
int check_distortion(const char *fn, int32_t R, int32_t N) {
  if (R < 0) return rnh::fail(REFNERF_EINVAL, "%s: R < 0", fn);
  if (N < 1 || N > rn::DIST_MAX_N) return rnh::fail(REFNERF_EINVAL, "%s: N outside [1, 512]", fn);
  return REFNERF_OK;
}
}  // namespace

extern "C" int refnerf_distortion_forward(const float *d_t, const float *d_w, int32_t R, int32_t N, float *d_ray_loss, void *stream) {
  const char *fn = "refnerf_distortion_forward";
  if (int rc = check_distortion(fn, R, N)) return rc;
  if (R == 0) return REFNERF_OK;
  if (!d_t || !d_w || !d_ray_loss) return rnh::fail(REFNERF_EINVAL, "%s: null pointer", fn);
  hipLaunchKernelGGL(rn::distortion_fwd_kernel, dim3((R + rn::DIST_WAVES - 1) / rn::DIST_WAVES), dim3(64 * rn::DIST_WAVES), 0,
                     (hipStream_t)stream, d_t, d_w, R, N, d_ray_loss);
  DIST_HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

extern "C" int refnerf_distortion_backward(const float *d_t, const float *d_w, const float *d_g, int32_t R, int32_t N, float *d_grad_w,
                                           void *stream) {
  const char *fn = "refnerf_distortion_backward";
  if (int rc = check_distortion(fn, R, N)) return rc;
  if (R == 0) return REFNERF_OK;
  if (!d_t || !d_w || !d_g || !d_grad_w) return rnh::fail(REFNERF_EINVAL, "%s: null pointer", fn);
  hipLaunchKernelGGL(rn::distortion_bwd_kernel, dim3((R + rn::DIST_WAVES - 1) / rn::DIST_WAVES), dim3(64 * rn::DIST_WAVES), 0,
                     (hipStream_t)stream, d_t, d_w, d_g, R, N, d_grad_w);
  DIST_HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}
