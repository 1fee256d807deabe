/*
 * refnerf_sq_train.hip -- second translation unit of librefnerf_hip.so: the round-5 training path of the parity-grade 16-bit
 * mode (REFNERF_PREC_F16X2, built-in IPE basis) on the eval kernel's skeleton.  Weight image (packed by the first unit:
 * refnerf_pack.h), ACT / DELTA formats: refnerf_sq_layout.h; kernels: refnerf_level_sq_fwd.h, refnerf_level_sq_bwd.h, refnerf_wgrad_sq.h.
 * Entry points (C++, internal): refnerf_sq_host.h; the C ABI stays in refnerf_hip.hip.
 */
#define REFNERF_SECONDARY_TU 1
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "refnerf_hip.h"
#include "refnerf_sq_host.h"
#include "refnerf_level_common.h"
#include "refnerf_level_bf16.h"
#include "refnerf_sq_layout.h"
#include "refnerf_level_sq_fwd.h"
#include "refnerf_level_sq_bwd.h"
#include "refnerf_wgrad_sq.h"

/* ================================================================== */
/* host                                                               */
/* ================================================================== */

#define SQ_HIP_TRY(expr)                                                     \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess) return rnh::fail(REFNERF_EHIP, #expr ": %s", hipGetErrorString(e_)); \
  } while (0)

namespace rnsq {

static int rays_per_wg_sq(int N) {
  if (N % rn::BT == 0) return 1;
  if (rn::BT % N == 0) return rn::BT / N;
  if ((2 * N) % rn::BT == 0 && 2 * N <= 512) return 2;
  if ((4 * N) % rn::BT == 0 && 4 * N <= 512) return 4;
  return 1;
}
static size_t fwd_lds_bytes(int rays, int N) {
  const size_t per_wg = sizeof(float) * (size_t)(2 * rays * (N + 1) + rn::NPS_TRAIN * rays * N + 3 * rn::BT + 8 + 12 * rays);
  return (size_t)rn::BF_RING_BYTES + rn::BF_X_BYTES + sizeof(float) * rn::HD_ROWS * rn::BT + per_wg;
}

int forward(const void *d_packed, const refnerf_level_cfg *cfg, const refnerf_rays *rays, int R, const float *d_sdist_in,
            const float *d_weights_in, const refnerf_level_out *out, const refnerf_level_out_extra *extra, float *d_act, hipStream_t st) {
  const int N = cfg->n_samples;
  int rpw = rays_per_wg_sq(N);
  /* the per-ray phases (resample, compositing) occupy one wave per ray: as many rays per workgroup as the LDS holds */
  while (2 * rpw <= rn::BF_NW && 2 * rpw * N <= 640 && fwd_lds_bytes(2 * rpw, N) + (size_t)rnh::lds_pad() <= 160 * 1024 && R / (2 * rpw) >= 512) rpw *= 2;
  while (rpw > 1 && fwd_lds_bytes(rpw, N) + (size_t)rnh::lds_pad() > 160 * 1024) rpw /= 2;
  size_t lds = fwd_lds_bytes(rpw, N) + (size_t)rnh::lds_pad();
  if (lds > 160 * 1024) return rnh::fail(REFNERF_EINVAL, "n_samples too large for the 160 KiB LDS budget of the REFNERF_PREC_F16X2 training forward%s");
  {
    const int nw = rpw < rn::BF_NW ? rpw : rn::BF_NW;
    const size_t scratch = sizeof(float) * (size_t)nw * (3 * (cfg->n_in + 4) + N + 3);
    if (scratch > (size_t)rn::BF_X_BYTES) return rnh::fail(REFNERF_EINVAL, "n_in / n_samples too large for the resampler scratch of this precision mode%s");
  }
  static hipError_t attr = [] {
    hipError_t e = hipFuncSetAttribute((const void *)rn::level_fwd_train_sq, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return e != hipSuccess ? e : hipFuncSetAttribute((const void *)rn::level_fwd_train_sq_h, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }();
  if (attr != hipSuccess) return rnh::fail(REFNERF_EHIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(attr));
  rn::LevelArgs a;
  a.packed = d_packed;
  a.cfg = *cfg;
  a.rays = *rays;
  a.R = R;
  a.rpw = rpw;
  a.sdist_in = d_sdist_in;
  a.weights_in = d_weights_in;
  a.out = *out;
  if (extra) a.xout = *extra;
  a.prof = nullptr;
  a.g_means = nullptr; a.g_covs = nullptr; a.cov_full = 0;
  a.act = d_act; a.act_pitch = 0;
  a.ring_off = 0;
  if (rnh::prof_on()) {
    int prc = rnh::prof_buffer(&a.prof);
    if (prc) return prc;
  }
  const int grid = (R + rpw - 1) / rpw;
  long tslot = -1;
  { int trc = rnh::timer_begin(st, &tslot, REFNERF_TIMER_FORWARD); if (trc) return trc; }
  if (cfg->wgrad_mode == REFNERF_WGRAD_F16) hipLaunchKernelGGL(rn::level_fwd_train_sq_h, dim3(grid), dim3(rn::BF_NTHREADS), lds, st, a);
  else hipLaunchKernelGGL(rn::level_fwd_train_sq, dim3(grid), dim3(rn::BF_NTHREADS), lds, st, a);
  SQ_HIP_TRY(hipGetLastError());
  { int trc = rnh::timer_end(st, tslot); if (trc) return trc; }
  if (a.prof) {
    long long hbuf[8 * 32];
    SQ_HIP_TRY(hipMemcpy(hbuf, a.prof, sizeof(hbuf), hipMemcpyDeviceToHost));
    for (int w = 0; w < 8; ++w) {
      fprintf(stderr, "[prof sq-fwd] wave %d:", w);
      for (int sl = 1; sl <= 18; ++sl) fprintf(stderr, " %lld", hbuf[w * 32 + sl] ? hbuf[w * 32 + sl] - hbuf[w * 32] : -1LL);
      fprintf(stderr, "\n");
    }
  }
  return REFNERF_OK;
}

int backward_chain(const void *d_packed, const refnerf_level_cfg *cfg, const refnerf_rays *rays, int R, const float *d_sdist,
                   const refnerf_level_grads *grads, const float *d_act, float *d_delta, const float *d_seeds, long long pitch,
                   hipStream_t st) {
  (void)d_sdist;
  static hipError_t attr = hipFuncSetAttribute((const void *)rn::level_bwd_sq, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (attr != hipSuccess) return rnh::fail(REFNERF_EHIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(attr));
  rn::SqBwdArgs a;
  a.packed = d_packed;
  a.cfg = *cfg;
  a.viewdirs = rays->d_viewdirs;
  a.S = (long long)R * cfg->n_samples;
  /* passes per workgroup: at least two workgroups per CU in flight over the launch, at most 8 passes (the prologue is short) */
  long long total = (a.S + rn::BT - 1) / rn::BT;
  int passes = (int)(total / 1024);
  passes = passes < 1 ? 1 : (passes > 8 ? 8 : passes);
  a.passes = passes;
  a.g_s_diffuse = grads->d_g_diffuse; a.g_s_specular = grads->d_g_specular; a.g_s_tint = grads->d_g_tint; a.g_s_rough = grads->d_g_roughness;
  a.act = d_act;
  a.delta = d_delta;
  a.seeds = d_seeds;
  a.pitch = pitch;
  a.prof = nullptr;
  if (rnh::prof_on()) {
    int prc = rnh::prof_buffer(&a.prof);
    if (prc) return prc;
    SQ_HIP_TRY(hipMemset(a.prof, 0, 8 * 32 * sizeof(long long)));
  }
  const int grid = (int)((total + passes - 1) / passes);
  const size_t lds = (size_t)rn::SQB_LDS_BYTES + (size_t)rnh::lds_pad();
  long tslot = -1;
  { int trc = rnh::timer_begin(st, &tslot, REFNERF_TIMER_BACKWARD); if (trc) return trc; }
  hipLaunchKernelGGL(rn::level_bwd_sq, dim3(grid), dim3(rn::BF_NTHREADS), lds, st, a);
  SQ_HIP_TRY(hipGetLastError());
  { int trc = rnh::timer_end(st, tslot); if (trc) return trc; }
  if (a.prof) {
    long long hbuf[8 * 32];
    SQ_HIP_TRY(hipMemcpy(hbuf, a.prof, sizeof(hbuf), hipMemcpyDeviceToHost));
    for (int w = 0; w < 8; ++w) {
      fprintf(stderr, "[prof sq-bwd] wave %d:", w);
      for (int sl = 1; sl <= 9; ++sl) fprintf(stderr, " %lld", hbuf[w * 32 + sl] ? hbuf[w * 32 + sl] - hbuf[w * 32] : -1LL);
      fprintf(stderr, "  | counted-wait %lld barrier-wait %lld\n", hbuf[w * 32 + 20], hbuf[w * 32 + 21]);
    }
  }
  return REFNERF_OK;
}

int wgrad(const float *d_act, const float *d_delta, long long S, long long pitch, int k_per_slice, int slices, float *d_part,
          float *d_kmin, int act11, int *slices_used, hipStream_t st) {
  (void)pitch;
  *slices_used = slices;
  static hipError_t attr = hipFuncSetAttribute((const void *)rn::wgrad_sq_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, rn::SQW_LDS);
  if (attr != hipSuccess) return rnh::fail(REFNERF_EHIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(attr));
  static hipError_t attr2 = hipFuncSetAttribute((const void *)rn::wgrad_sq256_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, rn::SQ2_LDS);
  if (attr2 != hipSuccess) return rnh::fail(REFNERF_EHIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(attr2));
  /* REFNERF_WGRAD_SQ_TILE=128: the four-wave 128 x 128 tiles (measurement aid; the default 256 x 256 tile fetches every operand once) */
  static const bool tile128 = [] { const char *e = getenv("REFNERF_WGRAD_SQ_TILE"); return e && atoi(e) == 128; }();
  SQ_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_kmin, 0x7f800000, 32, st));
  hipLaunchKernelGGL(rn::delta_kappa_min, dim3(256), dim3(256), 0, st, d_delta, S, d_kmin);
  rn::WgradSqArgs w;
  w.act = d_act; w.delta = d_delta; w.S = S; w.k_per_slice = k_per_slice; w.part = d_part;
  long tslot = -1;
  { int trc = rnh::timer_begin(st, &tslot, REFNERF_TIMER_WGRAD); if (trc) return trc; }
  if (tile128) {
    const dim3 grid(8 * ((slices + 7) / 8) * rn::WJOBS_SQ.tiles);
    hipLaunchKernelGGL(rn::wgrad_sq_kernel, grid, dim3(64 * rn::SQW_NW), rn::SQW_LDS, st, w, slices, d_kmin, act11);
  } else {
    /* One workgroup per CU (160 KB of LDS), so jobs x slices workgroups run in rounds of #CUs and a partial last round leaves
     * most of the chip idle behind compute-bound stragglers: the slice count is cut to whole rounds (20 jobs x 32 slices =
     * 2.5 rounds on 256 CUs -> 25 slices = 500 workgroups: 2.52 -> 2.10 ms at 4096 x 128; 24: 2.23, 28: 2.85, 19: 2.80).
     * REFNERF_WGRAD_SQ_SLICES overrides (measurement aid). */
    static const int cus = [] { int dev = 0, n = 256; if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); return n > 0 ? n : 256; }();
    static const int want = [] { const char *e = getenv("REFNERF_WGRAD_SQ_SLICES"); return e ? atoi(e) : 0; }();
    int se = slices;
    if (rn::WJOBS_SQ.n * se > cus) se = (rn::WJOBS_SQ.n * se / cus) * cus / rn::WJOBS_SQ.n;
    if (want > 0 && want <= slices) se = want;
    const long long blocks = (S + rn::RB - 1) / rn::RB;
    const long long per = (blocks + se - 1) / se;
    se = (int)((blocks + per - 1) / per);
    w.k_per_slice = (int)(per * rn::RB);
    *slices_used = se;
    hipLaunchKernelGGL(rn::wgrad_sq256_kernel, dim3(rn::WJOBS_SQ.n * se), dim3(512), rn::SQ2_LDS, st, w, se, d_kmin, act11);
  }
  SQ_HIP_TRY(hipGetLastError());
  { int trc = rnh::timer_end(st, tslot); if (trc) return trc; }
  return REFNERF_OK;
}

}  // namespace rnsq
