/*
 * refnerf_distortion.h -- C ABI of the distortion loss in librefnerf_hip.so: mip-NeRF 360's regulariser on one step
 * function per ray (stepfun.lossfun_distortion of the reference, internal/stepfun.py:261-272),
 *
 *     L = sum_i sum_j w_i w_j |u_i - u_j| + (1/3) sum_i w_i^2 (t_{i+1} - t_i),     u_i = (t_i + t_{i+1}) / 2,
 *
 * evaluated in O(N) per ray by a recurrence over the sorted knots in which every term is non-negative (DESIGN.md,
 * section 5).  A header of its own next to refnerf_hip.h: the same library, the same conventions -- device pointers to
 * contiguous float32 rows, `stream` a hipStream_t (NULL: the default stream), no host synchronisation, no allocation, one
 * fixed summation order (a ray gives the same bits alone and inside any batch), and the return codes of refnerf_hip.h:
 * 0 (REFNERF_OK), -1 (REFNERF_EINVAL, text in refnerf_last_error()), -3 (REFNERF_EHIP).
 *
 * Contract: the knots of every ray are nondecreasing (ties allowed: an interval of zero length adds nothing) and the
 * weights non-negative.  Unsorted knots give meaningless numbers, never an access outside the rows.  A ray whose weights
 * are all zero gives exactly 0 and an all-zero gradient.
 *
 * refnerf_distortion_forward:  d_ray_loss[r] = L of ray r (the caller takes the mean and applies
 *                              Config.distortion_loss_mult).
 * refnerf_distortion_backward: d_grad_w[r][k] = d_g[0] dL_r / dw_k; d_g is a DEVICE scalar, the gradient of the total
 *                              with respect to the sum of the per-ray values (as refnerf_interlevel_backward's upstream).
 *                              There is no gradient to t: every sdist the model emits is detached.
 * REFNERF_EINVAL: R < 0, N outside [1, 512], a null pointer.  R == 0 succeeds and launches nothing.
 */
#ifndef REFNERF_DISTORTION_H
#define REFNERF_DISTORTION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int refnerf_distortion_forward(const float *d_t /* [R][N+1] */, const float *d_w /* [R][N] */, int32_t R, int32_t N,
                               float *d_ray_loss /* [R] */, void *stream);
int refnerf_distortion_backward(const float *d_t, const float *d_w, const float *d_g /* [1] */, int32_t R, int32_t N,
                                float *d_grad_w /* [R][N] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif
