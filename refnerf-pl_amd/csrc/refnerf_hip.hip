/*
 * refnerf_hip.hip -- gfx950 (MI355X / CDNA4) kernels + C ABI of the Ref-NeRF
 * rendering inner loop.  Written for gfx950 only: 64-wide wavefronts, MFMA,
 * 160 KiB LDS per CU.
 *
 * Kernel map (one launch per sampling level):
 *   level_fwd_f32 : workgroup = 4 waves = RPW whole rays; each wave owns
 *   32-sample blocks.  resample -> warp -> conical frusta -> IPE (LDS) ->
 *   8x256 spatial MLP -> heads -> reflect + IDE (LDS) -> 8x256 directional MLP
 *   -> colour -> per-ray alpha scan + compositing.  The MLP runs transposed,
 *   D[out][sample] = W x X on v_mfma_f32_32x32x2_f32, so a layer's output
 *   registers ARE the next layer's B operands: activations never leave the
 *   register file; only the encodings (IPE 96, dir-MLP input 202) sit in LDS.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <utility>
#include <vector>

#include "refnerf_hip.h"
#include "refnerf_level_common.h"
#include "refnerf_level_f32.h"
#include "refnerf_level_bf16.h"
#include "refnerf_level_bwd_f32.h"
#include "refnerf_wgrad.h"
#include "refnerf_wgrad_bf16x3.h"
#include "refnerf_rays.h"
#include "refnerf_dataset.h"
#include "refnerf_optim.h"
#include "refnerf_regularisers.h"
#include "refnerf_data_terms.h"
#include "refnerf_proposal.h"
#include "refnerf_image.h"
#include "refnerf_vis.h"
#include "refnerf_sq_host.h"
#include "refnerf_sq_layout.h"
#include "refnerf_pack.h"

namespace rn {

/* ------------------------------------------------------------------ */
/* stage kernels                                                      */
/* ------------------------------------------------------------------ */

__global__ __launch_bounds__(256) void sample_intervals_kernel(const float *t, const float *logits, int R, int M, int N,
                                                               float smin, float smax, float *sdist, int32_t *bin_idx) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = (M + 1) + M + (M + 1) + N + (N + 1) + 8;
  float *scr = smem + wave * per;
  float *t_in = scr, *lg = t_in + (M + 1), *cw = lg + M, *c = cw + (M + 1), *sd = c + N;
  int ray = blockIdx.x * 4 + wave;
  if (ray >= R) return;
  for (int i = lane; i <= M; i += 64) t_in[i] = t[(size_t)ray * (M + 1) + i];
  for (int i = lane; i < M; i += 64) lg[i] = logits[(size_t)ray * M + i];
  wave_sync();
  sample_intervals_wave<true>(t_in, lg, cw, c, M, N, smin, smax, sd, bin_idx ? bin_idx + (size_t)ray * N : nullptr, lane);
  for (int k = lane; k <= N; k += 64) sdist[(size_t)ray * (N + 1) + k] = sd[k];
}

__global__ void ipe_kernel(const float *lmean, const float *lvar, int n, float *feat) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float lm[3] = {lmean[i * 3], lmean[i * 3 + 1], lmean[i * 3 + 2]};
  float lv[3] = {lvar[i * 3], lvar[i * 3 + 1], lvar[i * 3 + 2]};
  for (int hb = 0; hb < 2; ++hb)
    for (int j = 0; j < 16; ++j)
      for (int b = 0; b < 3; ++b) feat[(size_t)i * IPE_DIM + 48 * hb + j * 3 + b] = ipe_feature(lm[b], lv[b], j, hb);
}

__global__ void ide_kernel(const float *xyz, const float *kappa_inv, int n, float *out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float *o = out + (size_t)i * IDE_DIM;
  for (int part = 0; part < 2; ++part)
    ide_eval(xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], kappa_inv[i], part,
             [&](int q, float val) { o[part * IDE_TERMS + q] = val; });
}

/* compute_alpha_weights + volumetric_rendering (render.py:132-254) on caller-supplied per-sample values: the P7
 * device code of the level kernels (composite_phase) behind its own entry.  One wave per ray, rpw rays per workgroup. */
struct RenderArgs {
  refnerf_level_cfg cfg;
  int R, rpw;
  const float *density, *tdist, *dirs, *far, *rgb, *dif, *spc, *nrm, *npred, *rough, *tint;
  refnerf_level_out out;
};
__global__ __launch_bounds__(256) void render_rays_kernel(RenderArgs ra) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int N = ra.cfg.n_samples, rpw = ra.rpw;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float *TD = smem, *XP = TD + rpw * (N + 1), *PS = XP + rpw * (N + 1), *wscr = PS + (size_t)rpw * N * NPS_TRAIN;
  const int ray0 = blockIdx.x * rpw;
  for (int e = threadIdx.x; e < rpw * (N + 1); e += NTHREADS) {
    const int rl = e / (N + 1), ray = ray0 + rl;
    if (ray < ra.R) TD[e] = ra.tdist[(size_t)ray * (N + 1) + (e - rl * (N + 1))];
  }
  for (int e = threadIdx.x; e < rpw * N; e += NTHREADS) {
    const int rl = e / N, ray = ray0 + rl;
    if (ray >= ra.R) continue;
    const size_t g = (size_t)ray * N + (e - rl * N);
    float *ps = PS + (size_t)e * NPS_TRAIN;
    ps[PS_DENSITY] = ra.density[g];
    ps[PS_ROUGH] = ra.rough ? ra.rough[g] : 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ps[PS_RGB + c] = ra.rgb ? ra.rgb[3 * g + c] : 0.0f;
      ps[PS_DIF + c] = ra.dif ? ra.dif[3 * g + c] : 0.0f;
      ps[PS_SPC + c] = ra.spc ? ra.spc[3 * g + c] : 0.0f;
      ps[PS_NPRED + c] = ra.npred ? ra.npred[3 * g + c] : 0.0f;
      ps[PS_TINT + c] = ra.tint ? ra.tint[3 * g + c] : 0.0f;
      ps[PS_NORMALS + c] = ra.nrm ? ra.nrm[3 * g + c] : 0.0f;
    }
  }
  __syncthreads();
  LevelArgs A{};
  A.cfg = ra.cfg;
  A.R = ra.R;
  A.rpw = rpw;
  A.rays.d_directions = ra.dirs;
  A.rays.d_far = ra.far;
  A.out = ra.out;
  composite_phase<4, false, NPS_TRAIN>(A, TD, XP, PS, rpw * N, ray0, wave, lane, wscr, nullptr);
}

/* The three Ref-NeRF losses of one level as ONE pass over the level's outputs (train_utils.py:33-88 mse data term,
 * :165-183 orientation, :186-204 predicted normals), one wave per ray:
 *   terms[ray] = { sum_c lossmult (rgb_c - gt_c)^2,  sum_i w_i min(0, n_i . (-v))^2,  sum_i w_i (1 - n_i . npred_i) }
 * with n = `normals_o` (the orientation target: normals_pred or the density normals) / `normals` (density normals,
 * detached in the reference).  The host sums over the rays and applies multipliers and normalisers. */
struct LossArgs {
  int R, N;
  const float *rgb, *gt, *lossmult, *weights, *normals_o, *normals, *normals_pred, *viewdirs;
  float *terms;                 /* forward: [R,3] */
  /* backward: upstream scalars (already multiplied by multiplier / normaliser) and the gradient tensors */
  float g_data, g_orient, g_normal;
  const float *upstream;        /* device float[3]: dL/d(data, orientation, normal term) multiplying g_*, or NULL (= 1) */
  int orient_on_pred;           /* the orientation target IS normals_pred (its gradient then reaches g_npred) */
  float *g_rgb, *g_weights, *g_npred;
};
__global__ __launch_bounds__(256) void refnerf_losses_fwd_kernel(LossArgs a) {
  const int lane = threadIdx.x & 63, ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= a.R) return;
  const float v0 = -a.viewdirs[ray * 3], v1 = -a.viewdirs[ray * 3 + 1], v2 = -a.viewdirs[ray * 3 + 2];
  float s_o = 0.0f, s_n = 0.0f;
  for (int i = lane; i < a.N; i += 64) {
    const size_t e = (size_t)ray * a.N + i;
    const float w = a.weights[e];
    if (a.normals_o) {
      const float ndv = (a.normals_o[3 * e] * v0 + a.normals_o[3 * e + 1] * v1) + a.normals_o[3 * e + 2] * v2;
      const float m = fminf(ndv, 0.0f);
      s_o += w * (m * m);
    }
    if (a.normals) {
      const float d = (a.normals[3 * e] * a.normals_pred[3 * e] + a.normals[3 * e + 1] * a.normals_pred[3 * e + 1]) +
                      a.normals[3 * e + 2] * a.normals_pred[3 * e + 2];
      s_n += w * (1.0f - d);
    }
  }
  s_o = wave_sum(s_o);
  s_n = wave_sum(s_n);
  if (lane == 0) {
    float d = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) { const float r = a.rgb[ray * 3 + c] - a.gt[ray * 3 + c]; d += a.lossmult[ray] * (r * r); }
    a.terms[ray * 3] = d; a.terms[ray * 3 + 1] = s_o; a.terms[ray * 3 + 2] = s_n;
  }
}
__global__ __launch_bounds__(256) void refnerf_losses_bwd_kernel(LossArgs a) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)a.R * a.N) return;
  const int ray = (int)(e / a.N);
  const float g_data = a.g_data * (a.upstream ? a.upstream[0] : 1.0f), g_orient = a.g_orient * (a.upstream ? a.upstream[1] : 1.0f),
              g_normal = a.g_normal * (a.upstream ? a.upstream[2] : 1.0f);
  const float v0 = -a.viewdirs[ray * 3], v1 = -a.viewdirs[ray * 3 + 1], v2 = -a.viewdirs[ray * 3 + 2];
  const float w = a.weights[e];
  float gw = 0.0f, gn[3] = {0.0f, 0.0f, 0.0f};
  if (a.normals_o) {
    const float ndv = (a.normals_o[3 * e] * v0 + a.normals_o[3 * e + 1] * v1) + a.normals_o[3 * e + 2] * v2;
    const float m = fminf(ndv, 0.0f);
    gw += g_orient * (m * m);
    if (a.orient_on_pred) { const float k = g_orient * w * 2.0f * m; gn[0] += k * v0; gn[1] += k * v1; gn[2] += k * v2; }
  }
  if (a.normals) {
    const float d = (a.normals[3 * e] * a.normals_pred[3 * e] + a.normals[3 * e + 1] * a.normals_pred[3 * e + 1]) +
                    a.normals[3 * e + 2] * a.normals_pred[3 * e + 2];
    gw += g_normal * (1.0f - d);
    const float k = -g_normal * w;
#pragma unroll
    for (int c = 0; c < 3; ++c) gn[c] += k * a.normals[3 * e + c];
  }
  a.g_weights[e] = gw;
#pragma unroll
  for (int c = 0; c < 3; ++c) a.g_npred[3 * e + c] = gn[c];
  if (e < (size_t)a.R * 3) {      /* the first 3R threads also write the rendering gradient: d/d rgb of the mse term */
    const int r = (int)(e / 3);
    a.g_rgb[e] = g_data * a.lossmult[r] * 2.0f * (a.rgb[e] - a.gt[e]);
  }
}

}  // namespace rn

/* ================================================================== */
/* C ABI                                                              */
/* ================================================================== */

namespace {
thread_local char g_err[512] = "";
int fail(int code, const char *fmt, const char *detail = "") {
  snprintf(g_err, sizeof(g_err), fmt, detail);
  return code;
}
#define HIP_TRY(expr)                                                        \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess) return fail(REFNERF_EHIP, #expr ": %s", hipGetErrorString(e_)); \
  } while (0)

/* The library's only process-wide state (everything else lives in caller-owned buffers):
 *  - the opt-in kernel timer of refnerf_set_timing / refnerf_get_timing: event pairs recorded on the launch stream and
 *    resolved lazily in refnerf_get_timing(), so the timed region is not serialised by event syncs; guarded by `mu`, so
 *    level calls from several host threads stay safe while it is on;
 *  - two debug knobs read from the environment ONCE (REFNERF_PROF: per-phase cycle stamps, REFNERF_LDS_PAD: force one
 *    workgroup per CU) and the 2 KB device buffer of the stamps, allocated on first use and kept for the process. */
struct Runtime {
  std::mutex mu;
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  std::vector<int> family;       /* REFNERF_TIMER_* of each recorded pair */
  size_t events_used = 0;
  bool prof = false;
  int lds_pad = 0;
  long long *d_prof = nullptr;
  Runtime() {
    prof = getenv("REFNERF_PROF") != nullptr;
    if (const char *pad = getenv("REFNERF_LDS_PAD")) lds_pad = atoi(pad);
  }
};
Runtime &rt() {
  static Runtime r;
  return r;
}
/* cycle-stamp buffer of the REFNERF_PROF debug mode (8 waves x 32 slots) */
int prof_buffer(long long **out) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> lk(r.mu);
  if (!r.d_prof) HIP_TRY(hipMalloc(&r.d_prof, 8 * 32 * sizeof(long long)));
  *out = r.d_prof;
  return REFNERF_OK;
}
/* begin / end of a timed launch on stream `st`; `slot` < 0 = timer off */
int timer_begin(hipStream_t st, long *slot, int fam = REFNERF_TIMER_FORWARD) {
  Runtime &r = rt();
  *slot = -1;
  std::lock_guard<std::mutex> lk(r.mu);
  if (!r.timing || r.events_used >= 65536) return REFNERF_OK;
  if (r.events_used == r.events.size()) {
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    r.events.emplace_back(e0, e1);
    r.family.push_back(fam);
  }
  *slot = (long)r.events_used++;
  r.family[*slot] = fam;
  HIP_TRY(hipEventRecord(r.events[*slot].first, st));
  return REFNERF_OK;
}
int timer_end(hipStream_t st, long slot) {
  if (slot < 0) return REFNERF_OK;
  Runtime &r = rt();
  std::lock_guard<std::mutex> lk(r.mu);
  HIP_TRY(hipEventRecord(r.events[slot].second, st));
  return REFNERF_OK;
}
/* opt a kernel into the 160 KiB dynamic-LDS limit; the first failure is remembered and reported by every later call */
template <typename K>
hipError_t lds_attr(K kernel, int bytes = 160 * 1024) {
  return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}
#define LDS_ATTR_ONCE(...)                                                                         \
  do {                                                                                             \
    static hipError_t attr_err_ = [] {                                                             \
      hipError_t es_[] = {__VA_ARGS__};                                                            \
      for (hipError_t e_ : es_) if (e_ != hipSuccess) return e_;                                   \
      return hipSuccess;                                                                           \
    }();                                                                                           \
    if (attr_err_ != hipSuccess) return fail(REFNERF_EHIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(attr_err_)); \
  } while (0)

}  // namespace

namespace rnh {
int fail(int code, const char *fmt, const char *detail) { return ::fail(code, fmt, detail); }
int timer_begin(hipStream_t st, long *slot, int fam) { return ::timer_begin(st, slot, fam); }
int timer_end(hipStream_t st, long slot) { return ::timer_end(st, slot); }
bool prof_on() { return rt().prof; }
int prof_buffer(long long **out) { return ::prof_buffer(out); }
int lds_pad() { return rt().lds_pad; }
}  // namespace rnh

extern "C" {

int refnerf_abi_version(void) { return REFNERF_ABI_VERSION; }
const char *refnerf_last_error(void) { return g_err; }

void refnerf_level_cfg_default(refnerf_level_cfg *c) {
  memset(c, 0, sizeof(*c));
  c->n_samples = 128; c->n_in = 1; c->training = 0; c->compute_extras = 1;
  c->srgb_mapping = 1; c->srgb_mapping_normalization = 1; c->render_srgb_mode = REFNERF_SRGB_NONE;
  c->opaque_background = 0; c->ray_shape = 0; c->precision = REFNERF_PREC_F32; c->wgrad_mode = REFNERF_WGRAD_BF16X3; c->dir_enc = REFNERF_DIRENC_IDE; c->raydist = REFNERF_RAYDIST_NONE; c->disable_integration = 0; c->ipe_groups = 0;
  c->anneal = 1.0f; c->resample_padding = 0.01f; c->s_near = 0.0f; c->s_far = 1.0f;
  c->density_bias = 0.5f; c->roughness_bias = -1.0f;
  c->rgb_premultiplier = 1.0f; c->rgb_bias = 0.0f; c->rgb_padding = 0.001f; c->bg_rgb = 1.0f;
}

int refnerf_device_ok(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(REFNERF_ENOGPU, "no HIP device%s");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  hipDeviceProp_t p;
  HIP_TRY(hipGetDeviceProperties(&p, dev));
  if (strncmp(p.gcnArchName, "gfx950", 6) != 0) return fail(REFNERF_ENOGPU, "device is %s, this library is built for gfx950 only", p.gcnArchName);
  return REFNERF_OK;
}

size_t refnerf_packed_weights_bytes(int precision) {
  if (precision == REFNERF_PREC_F32) return (size_t)rn::PACKED.total * sizeof(float);
  if (precision == REFNERF_PREC_BF16 || precision == REFNERF_PREC_F16) return ((size_t)rn::BFPACKED.chunks_per_pass + 2) * rn::BF_CHUNK_BYTES;
  if (precision == REFNERF_PREC_F16X2) return ((size_t)rn::SPPACKED.total_chunks + 2) * rn::BF_CHUNK_BYTES;
  if (precision == REFNERF_IMAGE_F16X2_TRAIN) return rn::TR_IMAGE_BYTES;
  return 0;
}

/* ---- which image a device pointer holds (v11): recorded by the pack entries, checked by the level entries ---- */
#include <mutex>
#include <unordered_map>
namespace {
constexpr int IMAGE_KIND_BASIS = 0x100;      /* + REFNERF_PREC_F32: the extended image of refnerf_pack_weights_basis */
std::mutex g_image_mu;
std::unordered_map<const void *, int> g_image_kind;
void remember_image(const void *p, int kind) {
  std::lock_guard<std::mutex> lk(g_image_mu);
  g_image_kind[p] = kind;
}
const char *image_name(int kind) {
  switch (kind) {
    case REFNERF_PREC_F32: return "REFNERF_PREC_F32";
    case REFNERF_PREC_BF16: return "REFNERF_PREC_BF16";
    case REFNERF_PREC_F16: return "REFNERF_PREC_F16";
    case REFNERF_PREC_F16X2: return "REFNERF_PREC_F16X2";
    case REFNERF_IMAGE_F16X2_TRAIN: return "REFNERF_IMAGE_F16X2_TRAIN";
    case IMAGE_KIND_BASIS + REFNERF_PREC_F32: return "REFNERF_PREC_F32 (general basis)";
    default: return "?";
  }
}
/* 0, or REFNERF_EINVAL when the library itself packed `p` as something else than this level streams */
int check_image(const void *p, const refnerf_level_cfg *cfg, const char *who) {
  const int want = refnerf_level_image(cfg) + (cfg->ipe_groups > 1 ? IMAGE_KIND_BASIS : 0);
  int have = -1;
  {
    std::lock_guard<std::mutex> lk(g_image_mu);
    auto it = g_image_kind.find(p);
    if (it != g_image_kind.end()) have = it->second;
  }
  if (have < 0 || have == want) return REFNERF_OK;
  /* (the plain f32 image in place of the extended one reads past its end; the extended one in place of the plain one is a superset) */
  if (have == IMAGE_KIND_BASIS + REFNERF_PREC_F32 && want == REFNERF_PREC_F32) return REFNERF_OK;
  snprintf(g_err, sizeof(g_err), "%s: d_packed was packed as the %s image, this level configuration streams the %s image (refnerf_level_image)",
           who, image_name(have), image_name(want));
  return REFNERF_EINVAL;
}
}  // namespace

int refnerf_level_image(const refnerf_level_cfg *cfg) {
  if (!cfg) return -1;
  if (cfg->ipe_groups > 1) return REFNERF_PREC_F32;
  if (cfg->training) return cfg->precision == REFNERF_PREC_F16X2 ? REFNERF_IMAGE_F16X2_TRAIN : REFNERF_PREC_F32;
  return cfg->precision;
}

int refnerf_pack_weights(const float *d_params, void *d_packed, int precision, void *stream) {
  if (!d_params || !d_packed) return fail(REFNERF_EINVAL, "refnerf_pack_weights: null pointer%s");
  remember_image(d_packed, precision);
  if (precision == REFNERF_PREC_F32) {
    dim3 grid(64, 3 * rn::NUM_OPS + 3 * rn::NUM_TOPS + 1);
    hipLaunchKernelGGL(rn::pack_weights_f32, grid, dim3(256), 0, (hipStream_t)stream, d_params, (float *)d_packed);
  } else if (precision == REFNERF_PREC_BF16) {
    dim3 grid(8, rn::NUM_OPS);
    hipLaunchKernelGGL(rn::pack_weights_16<__bf16>, grid, dim3(256), 0, (hipStream_t)stream, d_params, (char *)d_packed);
  } else if (precision == REFNERF_PREC_F16) {
    dim3 grid(8, rn::NUM_OPS);
    hipLaunchKernelGGL(rn::pack_weights_16<_Float16>, grid, dim3(256), 0, (hipStream_t)stream, d_params, (char *)d_packed);
  } else if (precision == REFNERF_PREC_F16X2) {
    dim3 grid(8, rn::NUM_OPS);
    hipLaunchKernelGGL(rn::pack_weights_split, grid, dim3(256), 0, (hipStream_t)stream, d_params, (char *)d_packed);
  } else if (precision == REFNERF_IMAGE_F16X2_TRAIN) {
    hipLaunchKernelGGL(rn::pack_train_chunks, dim3(rn::TR_CHUNKS), dim3(256), 0, (hipStream_t)stream, d_params, (char *)d_packed);
    hipLaunchKernelGGL(rn::pack_train_consts, dim3(rn::TRG_N), dim3(1024), 0, (hipStream_t)stream, d_params,
                       (float *)((char *)d_packed + rn::TR_CONST_OFF));
  } else {
    return fail(REFNERF_EINVAL, "refnerf_pack_weights: unknown precision%s");
  }
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

size_t refnerf_packed_weights_bytes_basis(int precision, int ipe_groups) {
  if (ipe_groups <= 1) return refnerf_packed_weights_bytes(precision);
  if (precision != REFNERF_PREC_F32 || ipe_groups > rn::IPE_MAX_GROUPS) return 0;
  return (size_t)rn::PACKED_EXT_TOTAL * sizeof(float);
}

int refnerf_pack_weights_basis(const float *d_params, const float *d_basis, int ipe_groups, void *d_packed, int precision, void *stream) {
  if (ipe_groups <= 1) return refnerf_pack_weights(d_params, d_packed, precision, stream);
  if (!d_basis) return fail(REFNERF_EINVAL, "refnerf_pack_weights_basis: null basis%s");
  if (ipe_groups > rn::IPE_MAX_GROUPS) return fail(REFNERF_EUNSUPPORTED, "refnerf_pack_weights_basis: at most 7 groups of three directions (21: icosahedron / 2)%s");
  if (precision != REFNERF_PREC_F32)
    return fail(REFNERF_EUNSUPPORTED, "refnerf_pack_weights_basis builds the REFNERF_PREC_F32 image (levels with REFNERF_PREC_F32 or REFNERF_PREC_F16X2 run on it); the plain bf16 / f16 images have no direction groups%s");
  const int rc = refnerf_pack_weights(d_params, d_packed, precision, stream);
  if (rc) return rc;
  remember_image(d_packed, IMAGE_KIND_BASIS + REFNERF_PREC_F32);
  hipLaunchKernelGGL(rn::pack_weights_ext, dim3(32, 1 + 8 * rn::EXT_GROUPS), dim3(256), 0, (hipStream_t)stream, d_params, d_basis, ipe_groups, (float *)d_packed);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

static int rays_per_wg(int N, int tile) {
  if (N % tile == 0) return 1;
  if (tile % N == 0) return tile / N;
  /* otherwise whole passes only if a small multiple fits the per-sample LDS budget */
  if ((2 * N) % tile == 0 && 2 * N <= 512) return 2;
  if ((4 * N) % tile == 0 && 4 * N <= 512) return 4;
  return 1;   /* last pass partially filled */
}

namespace {
struct BwdPlan { long long S, pitch; int slices, k_per_slice; size_t act_bytes, delta_off, part_off, seed_off, cmin_off, total, act_ext_off, part_ext_off; };
/* groups > 1 (general IPE basis): the tail matrix of the groups' IPE features behind ACT, the tail's split-K partials behind the seeds */
/* split-K slices of the weight-gradient GEMMs (one PART image of NUM_PARAMS floats each, reduced in a fixed order) */
constexpr int MAX_SLICES = 32;
BwdPlan bwd_plan(int R, int N, int groups = 0) {
  BwdPlan p;
  p.S = (long long)R * N;
  p.pitch = (p.S + 127) / 128 * 128;
  long long sl = (p.S + 2047) / 2048;
  p.slices = (int)(sl < 1 ? 1 : (sl > MAX_SLICES ? MAX_SLICES : sl));
  long long per = (p.S + p.slices - 1) / p.slices;
  p.k_per_slice = (int)((per + rn::WG_KT - 1) / rn::WG_KT * rn::WG_KT);
  p.act_bytes = sizeof(float) * (size_t)rn::ACT_ALLOC_ROWS * p.pitch;
  p.delta_off = 0;
  p.part_off = p.delta_off + sizeof(float) * (size_t)rn::DEL_ALLOC_ROWS * p.pitch;
  p.seed_off = p.part_off + sizeof(float) * (size_t)p.slices * rn::NUM_PARAMS;
  p.cmin_off = p.seed_off + sizeof(float) * (size_t)rn::NGS * p.pitch;      /* REFNERF_ACT_SQ: the smallest delta factor per layer id (kmin of rnsq::wgrad) */
  p.total = p.cmin_off + 128;
  p.act_ext_off = p.act_bytes;
  p.part_ext_off = p.total;
  if (groups > 1) {
    p.act_bytes += sizeof(float) * (size_t)rn::ACT_EXT_UNITS * p.pitch;
    p.total += sizeof(float) * (size_t)p.slices * rn::EXT_PARAMS;
  }
  return p;
}
}  // namespace

static int level_forward_impl(const void *d_packed, const refnerf_level_cfg *cfg, const refnerf_rays *rays,
                              int32_t R, const float *d_sdist_in, const float *d_weights_in,
                              const refnerf_level_out *out, const refnerf_level_out_extra *extra, float *d_act, long long act_pitch,
                              void *stream) {
  if (!d_packed || !cfg || !rays || !out)
    return fail(REFNERF_EINVAL, "refnerf_level_forward: null pointer%s");
  /* d_sdist_in = d_weights_in = NULL: the model's initial step function [s_near, s_far], weight 1 (closed form in the resampler) */
  if (!d_sdist_in != !d_weights_in)
    return fail(REFNERF_EINVAL, "refnerf_level_forward: d_sdist_in and d_weights_in are given together, or both NULL (the initial step function)%s");
  if (!d_sdist_in && cfg->n_in != 1)
    return fail(REFNERF_EINVAL, "refnerf_level_forward: a NULL step function is the initial one, n_in must be 1%s");
  if (!d_sdist_in && !(cfg->s_far > cfg->s_near))
    return fail(REFNERF_EINVAL, "refnerf_level_forward: a NULL step function needs s_near < s_far%s");
  if (R <= 0) return fail(REFNERF_EINVAL, "refnerf_level_forward: R must be positive%s");
  /* stepfun.py:234-235 */
  if (cfg->n_samples <= 1) return fail(REFNERF_EINVAL, "num_samples must be > 1%s");
  /* render.py:126 */
  if (cfg->ray_shape != 0 && cfg->ray_shape != 1) return fail(REFNERF_EINVAL, "ray_shape must be 'cone' or 'cylinder'%s");
  if (cfg->n_in < 1 || cfg->n_in > 512) return fail(REFNERF_EINVAL, "n_in must be in [1,512]%s");
  if (cfg->precision != REFNERF_PREC_F32 && cfg->precision != REFNERF_PREC_BF16 && cfg->precision != REFNERF_PREC_F16 &&
      cfg->precision != REFNERF_PREC_F16X2)
    return fail(REFNERF_EINVAL, "unknown precision mode%s");
  if (cfg->raydist < REFNERF_RAYDIST_NONE || cfg->raydist > REFNERF_RAYDIST_SQUARE)
    return fail(REFNERF_EINVAL, "unknown raydist (REFNERF_RAYDIST_*)%s");
  if (cfg->dir_enc != REFNERF_DIRENC_IDE && cfg->dir_enc != REFNERF_DIRENC_POSENC)
    return fail(REFNERF_EINVAL, "unknown dir_enc (REFNERF_DIRENC_IDE / REFNERF_DIRENC_POSENC)%s");
  if (cfg->training && cfg->precision == REFNERF_PREC_F16)
    return fail(REFNERF_EUNSUPPORTED, "REFNERF_PREC_F16 is an inference mode (training levels: REFNERF_PREC_F32, REFNERF_PREC_F16X2 or REFNERF_PREC_BF16)%s");
  const bool gbasis = cfg->ipe_groups > 1;
  if (cfg->ipe_groups < 0 || cfg->ipe_groups > rn::IPE_MAX_GROUPS) return fail(REFNERF_EINVAL, "ipe_groups must be in [0,7]%s");
  if (gbasis && cfg->precision != REFNERF_PREC_F32 && cfg->precision != REFNERF_PREC_F16X2)
    return fail(REFNERF_EUNSUPPORTED, "a general IPE basis (ipe_groups > 1) runs with REFNERF_PREC_F32 or REFNERF_PREC_F16X2 (d_packed: the REFNERF_PREC_F32 image of refnerf_pack_weights_basis in both)%s");
  /* training + BF16: the fp32-structure kernel with its MLP chains on bf16 MFMA (level_fwd_train_bf16c); d_packed is
   * the REFNERF_PREC_F32 image in that case (it carries the bf16 copies of the ops) */
  const bool train_bf = cfg->training && cfg->precision == REFNERF_PREC_BF16;
  if (!rays->d_origins || !rays->d_directions || !rays->d_viewdirs || !rays->d_radii || !rays->d_near || !rays->d_far)
    return fail(REFNERF_EINVAL, "refnerf_level_forward: null ray field%s");
  const int N = cfg->n_samples;
  /* a general basis in F16X2, training or inference: the fp32-structure kernel with its chains on split-f16 operands
   * (level_fwd_f16x2c_gb), fp32 ACT rows */
  const bool gb_split = gbasis && cfg->precision == REFNERF_PREC_F16X2;
  if (int irc = check_image(d_packed, cfg, "refnerf_level_forward")) return irc;
  /* training + F16X2 on the built-in basis: the kernels on the eval kernel's skeleton (refnerf_sq_train.hip);
   * d_packed is the REFNERF_IMAGE_F16X2_TRAIN image, the activations REFNERF_ACT_SQ */
  const bool train_sq = cfg->training && cfg->precision == REFNERF_PREC_F16X2 && !gbasis;
  if (train_sq && !d_act)
    return fail(REFNERF_EINVAL, "a training level in REFNERF_PREC_F16X2 runs through refnerf_level_forward_train: its kernel keeps the ReLU sign words and "
                                "the bottleneck rows in the activation buffer (d_packed: the REFNERF_IMAGE_F16X2_TRAIN image)%s");
  if (cfg->wgrad_mode == REFNERF_WGRAD_F16 && !train_sq)
    return fail(REFNERF_EUNSUPPORTED, "wgrad_mode = REFNERF_WGRAD_F16 belongs to training levels in REFNERF_PREC_F16X2 on the built-in IPE basis%s");
  if (train_sq) return rnsq::forward(d_packed, cfg, rays, R, d_sdist_in, d_weights_in, out, extra, d_act, (hipStream_t)stream);
  const bool split = cfg->precision == REFNERF_PREC_F16X2 && !gb_split;
  const bool bf = (cfg->precision == REFNERF_PREC_BF16 && !train_bf) || cfg->precision == REFNERF_PREC_F16 || split;     /* the LDS-ring 16-bit eval kernels */
  int rpw = rays_per_wg(N, bf ? rn::BT : rn::T_TILE);
  /* 16-bit inference, rays that do not tile the 256-sample pass within 640 samples (N = 192: 2 rays = one and a half
   * passes): take the smallest ray count that does (N = 192: 4 rays = three full passes) with the per-sample records in a
   * ring (level_fwd_*_ring composites every ray behind the pass that completes it) -- if a ray plus a pass fit the ring,
   * there are still at least two workgroups per CU, and the per-ray arrays fit */
  bool ps_ring = false;
  if (bf && N <= rn::BF_PS_RING - rn::BT && (rpw * N) % rn::BT != 0) {
    int r = 1;
    while (r <= rn::BF_NW && (r * N) % rn::BT != 0) ++r;
    if (r <= rn::BF_NW && r * N > 640 && R / r >= 512) { rpw = r; ps_ring = true; }
  }
  auto lds_bytes = [&](int rays) -> size_t {
    const int np = bf ? rn::NPS_EVAL : rn::NPS_TRAIN, tile = bf ? rn::BT : rn::T_TILE;
    const int ps_rows = ps_ring ? rn::BF_PS_RING : rays * N;
    const size_t per_wg = sizeof(float) * (size_t)(2 * rays * (N + 1) + np * ps_rows + 3 * tile + 8 + 12 * rays);
    if (bf) return (size_t)rn::BF_RING_BYTES + rn::BF_X_BYTES + sizeof(float) * rn::HD_ROWS * rn::BT + per_wg;
    return sizeof(float) * (size_t)(rn::DIR_PAD * rn::T_TILE + rn::HD_ROWS * rn::T_TILE) + per_wg;
  };
  if (ps_ring && lds_bytes(rpw) + (size_t)rt().lds_pad > 160 * 1024) { ps_ring = false; rpw = rays_per_wg(N, rn::BT); }
  /* bf16: the per-ray phases (resample, compositing) occupy one wave per ray, so take as many rays per
   * workgroup as the LDS holds (up to one per wave): the other waves idle for a shorter share of the pass */
  if (bf && !ps_ring) while (2 * rpw <= rn::BF_NW && 2 * rpw * N <= 640 && lds_bytes(2 * rpw) <= 160 * 1024 &&
                 R / (2 * rpw) >= 512)        /* ... but keep at least two workgroups per CU in flight */
    rpw *= 2;
  if (rpw * N > 640 && !ps_ring) return fail(REFNERF_EINVAL, "n_samples too large for the LDS budget (rays_per_wg*N must be <= 640)%s");
  size_t lds = lds_bytes(rpw);
  {
    const int nwmax = bf ? rn::BF_NW : 4;
    const int nw = rpw < nwmax ? rpw : nwmax;
    const size_t scratch = sizeof(float) * (size_t)nw * (3 * (cfg->n_in + 4) + N + 3);
    if (scratch > (bf ? (size_t)rn::BF_X_BYTES : sizeof(float) * rn::DIR_PAD * rn::T_TILE))
      return fail(REFNERF_EINVAL, "n_in / n_samples too large for the resampler scratch of this precision mode%s");
  }
  /* bf16 chains: the shared weight-stream ring comes on top; fewer rays per workgroup (a partly filled last pass)
   * when the whole-pass choice no longer fits */
  while (train_bf && rpw > 1 && (lds + 15) / 16 * 16 + rn::RING_BYTES > 160 * 1024) { rpw /= 2; lds = lds_bytes(rpw); }
  const size_t ring_off = (lds + 15) / 16 * 16;
  if (train_bf) lds = ring_off + rn::RING_BYTES;
  lds += (size_t)rt().lds_pad;   /* debug (REFNERF_LDS_PAD): force 1 workgroup/CU */
  if (lds > 160 * 1024) return fail(REFNERF_EINVAL, "n_samples too large for the 160 KiB LDS budget of this precision mode%s");
  LDS_ATTR_ONCE(lds_attr(rn::level_fwd_f32), lds_attr(rn::level_fwd_train_f32), lds_attr(rn::level_fwd_train_bf16c),
                lds_attr(rn::level_fwd_bf16), lds_attr(rn::level_fwd_f16), lds_attr(rn::level_fwd_bf16_ring), lds_attr(rn::level_fwd_f16_ring),
                lds_attr(rn::level_fwd_f16x2), lds_attr(rn::level_fwd_f16x2_ring), lds_attr(rn::level_fwd_f32_gb), lds_attr(rn::level_fwd_train_f32_gb), lds_attr(rn::level_fwd_f16x2c_gb));
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
  a.act = d_act; a.act_pitch = act_pitch;
  a.ring_off = (int)ring_off;
  if (rt().prof) {
    int prc = prof_buffer(&a.prof);
    if (prc) return prc;
  }
  int grid = (R + rpw - 1) / rpw;
  hipStream_t st = (hipStream_t)stream;
  long tslot = -1;
  {
    int trc = timer_begin(st, &tslot);
    if (trc) return trc;
  }
  if (split && ps_ring) hipLaunchKernelGGL(rn::level_fwd_f16x2_ring, dim3(grid), dim3(rn::BF_NTHREADS), lds, st, a);
  else if (split) hipLaunchKernelGGL(rn::level_fwd_f16x2, dim3(grid), dim3(rn::BF_NTHREADS), lds, st, a);
  else if (bf && ps_ring && cfg->precision == REFNERF_PREC_F16) hipLaunchKernelGGL(rn::level_fwd_f16_ring, dim3(grid), dim3(rn::BF_NTHREADS), lds, st, a);
  else if (bf && ps_ring) hipLaunchKernelGGL(rn::level_fwd_bf16_ring, dim3(grid), dim3(rn::BF_NTHREADS), lds, st, a);
  else if (bf && cfg->precision == REFNERF_PREC_F16) hipLaunchKernelGGL(rn::level_fwd_f16, dim3(grid), dim3(rn::BF_NTHREADS), lds, st, a);
  else if (bf) hipLaunchKernelGGL(rn::level_fwd_bf16, dim3(grid), dim3(rn::BF_NTHREADS), lds, st, a);
  else if (train_bf) hipLaunchKernelGGL(rn::level_fwd_train_bf16c, dim3(grid), dim3(rn::NTHREADS), lds, st, a);
  else if (gb_split) hipLaunchKernelGGL(rn::level_fwd_f16x2c_gb, dim3(grid), dim3(rn::NTHREADS), lds, st, a);
  else if (cfg->training && gbasis) hipLaunchKernelGGL(rn::level_fwd_train_f32_gb, dim3(grid), dim3(rn::NTHREADS), lds, st, a);
  else if (cfg->training) hipLaunchKernelGGL(rn::level_fwd_train_f32, dim3(grid), dim3(rn::NTHREADS), lds, st, a);
  else if (gbasis) hipLaunchKernelGGL(rn::level_fwd_f32_gb, dim3(grid), dim3(rn::NTHREADS), lds, st, a);
  else hipLaunchKernelGGL(rn::level_fwd_f32, dim3(grid), dim3(rn::NTHREADS), lds, st, a);
  HIP_TRY(hipGetLastError());
  {
    int trc = timer_end(st, tslot);
    if (trc) return trc;
  }
  if (a.prof) {   /* debug aid (REFNERF_PROF=1): per-phase cycle stamps of a mid-grid workgroup */
    long long hbuf[8 * 32];
    HIP_TRY(hipMemcpy(hbuf, a.prof, sizeof(hbuf), hipMemcpyDeviceToHost));
    const int nw = bf ? 8 : 4;
    for (int w = 0; w < nw; ++w) {
      fprintf(stderr, "[prof] wave %d:", w);
      for (int sl = 1; sl <= 18; ++sl) fprintf(stderr, " %lld", hbuf[w * 32 + sl] ? hbuf[w * 32 + sl] - hbuf[w * 32] : -1LL);
      fprintf(stderr, "  | dma-wait %lld barrier-wait %lld", hbuf[w * 32 + 20], hbuf[w * 32 + 21]);
#ifdef REFNERF_PROF_WAITS
      fprintf(stderr, " | P0 split");   /* stamps inside the resample phase (RN_STAMP_P0) */
      for (int sl = 24; sl <= 28; ++sl) fprintf(stderr, " %lld", hbuf[w * 32 + sl] ? hbuf[w * 32 + sl] - hbuf[w * 32] : -1LL);
#endif
      if (hbuf[w * 32 + 23] > hbuf[w * 32 + 22])   /* -DREFNERF_PROF_WAITS builds: shader clock from the 100 MHz counter */
        fprintf(stderr, " | clock %.0f MHz", 100.0 * (double)(hbuf[w * 32 + 15] - hbuf[w * 32]) / (double)(hbuf[w * 32 + 23] - hbuf[w * 32 + 22]));
      fprintf(stderr, "\n");
    }
  }
  return REFNERF_OK;
}

int refnerf_level_forward(const void *d_packed, const refnerf_level_cfg *cfg, const refnerf_rays *rays,
                          int32_t R, const float *d_sdist_in, const float *d_weights_in,
                          const refnerf_level_out *out, void *stream) {
  return level_forward_impl(d_packed, cfg, rays, R, d_sdist_in, d_weights_in, out, nullptr, nullptr, 0, stream);
}

int refnerf_level_forward_ex(const void *d_packed, const refnerf_level_cfg *cfg, const refnerf_rays *rays,
                             int32_t R, const float *d_sdist_in, const float *d_weights_in,
                             const refnerf_level_out *out, const refnerf_level_out_extra *extra, void *stream) {
  return level_forward_impl(d_packed, cfg, rays, R, d_sdist_in, d_weights_in, out, extra, nullptr, 0, stream);
}

int refnerf_level_forward_train_ex(const void *d_packed, const refnerf_level_cfg *cfg, const refnerf_rays *rays,
                                int32_t R, const float *d_sdist_in, const float *d_weights_in,
                                const refnerf_level_out *out, const refnerf_level_out_extra *extra, void *d_activations,
                                   size_t activations_bytes,
                                void *stream) {
  if (!cfg || !d_activations) return fail(REFNERF_EINVAL, "refnerf_level_forward_train: null pointer%s");
  if (!cfg->training) return fail(REFNERF_EINVAL, "refnerf_level_forward_train: cfg->training must be 1%s");
  if (R <= 0 || cfg->n_samples <= 1) return fail(REFNERF_EINVAL, "refnerf_level_forward_train: bad R / num_samples%s");
  const BwdPlan plan = bwd_plan(R, cfg->n_samples, cfg->ipe_groups);
  if (activations_bytes < plan.act_bytes)
    return fail(REFNERF_EINVAL, "refnerf_level_forward_train: activation buffer too small (see refnerf_activation_workspace_bytes)%s");
  return level_forward_impl(d_packed, cfg, rays, R, d_sdist_in, d_weights_in, out, extra, (float *)d_activations, plan.pitch, stream);
}

int refnerf_level_forward_train(const void *d_packed, const refnerf_level_cfg *cfg, const refnerf_rays *rays,
                                int32_t R, const float *d_sdist_in, const float *d_weights_in,
                                const refnerf_level_out *out, void *d_activations, size_t activations_bytes,
                                void *stream) {
  return refnerf_level_forward_train_ex(d_packed, cfg, rays, R, d_sdist_in, d_weights_in, out, nullptr, d_activations, activations_bytes, stream);
}

/* both ray-generation entries; dist == NULL: the pinhole kernel */
static int pixels_to_rays_impl(const char *fn, const int32_t *d_pix_x, const int32_t *d_pix_y, const float *d_pixtocams,
                               int32_t pixtocam_per_ray, const float *d_camtoworlds, int32_t camtoworld_per_ray,
                               const float *d_pixtocam_ndc, int32_t n, float *d_origins, float *d_directions, float *d_viewdirs,
                               float *d_radii, float *d_imageplane, const refnerf_lens_distortion *dist, void *stream) {
  if (!d_pix_x || !d_pix_y || !d_pixtocams || !d_camtoworlds || !d_origins || !d_directions || !d_viewdirs || !d_radii)
    return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (n <= 0) return fail(REFNERF_EINVAL, "%s: n must be positive", fn);
  rn::RayGenArgs a{};
  a.pix_x = d_pix_x; a.pix_y = d_pix_y;
  a.pixtocams = d_pixtocams; a.camtoworlds = d_camtoworlds; a.pixtocam_ndc = d_pixtocam_ndc;
  a.p2c_stride = pixtocam_per_ray ? 9 : 0;
  a.c2w_stride = camtoworld_per_ray ? 12 : 0;
  a.n = n;
  a.origins = d_origins; a.directions = d_directions; a.viewdirs = d_viewdirs; a.radii = d_radii; a.imageplane = d_imageplane;
  if (dist) {
    a.dist = {dist->k1, dist->k2, dist->k3, dist->k4, dist->p1, dist->p2, dist->eps, dist->max_iterations};
    hipLaunchKernelGGL(rn::pixels_to_rays_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(rn::pixels_to_rays_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
  }
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_pixels_to_rays(const int32_t *d_pix_x, const int32_t *d_pix_y, const float *d_pixtocams, int32_t pixtocam_per_ray,
                           const float *d_camtoworlds, int32_t camtoworld_per_ray, const float *d_pixtocam_ndc, int32_t n,
                           float *d_origins, float *d_directions, float *d_viewdirs, float *d_radii, float *d_imageplane,
                           void *stream) {
  return pixels_to_rays_impl("refnerf_pixels_to_rays", d_pix_x, d_pix_y, d_pixtocams, pixtocam_per_ray, d_camtoworlds,
                             camtoworld_per_ray, d_pixtocam_ndc, n, d_origins, d_directions, d_viewdirs, d_radii, d_imageplane,
                             nullptr, stream);
}

int refnerf_pixels_to_rays_distorted(const int32_t *d_pix_x, const int32_t *d_pix_y, const float *d_pixtocams,
                                     int32_t pixtocam_per_ray, const float *d_camtoworlds, int32_t camtoworld_per_ray,
                                     const float *d_pixtocam_ndc, int32_t n, float *d_origins, float *d_directions,
                                     float *d_viewdirs, float *d_radii, float *d_imageplane,
                                     const refnerf_lens_distortion *distortion, void *stream) {
  if (!distortion) return fail(REFNERF_EINVAL, "refnerf_pixels_to_rays_distorted: null distortion%s");
  const double c[7] = {distortion->k1, distortion->k2, distortion->k3, distortion->k4, distortion->p1, distortion->p2,
                       distortion->eps};
  for (double v : c)
    if (!std::isfinite(v)) return fail(REFNERF_EINVAL, "refnerf_pixels_to_rays_distorted: non-finite distortion parameter%s");
  if (distortion->max_iterations < 0 || distortion->max_iterations > REFNERF_MAX_UNDISTORT_ITERATIONS)
    return fail(REFNERF_EINVAL, "refnerf_pixels_to_rays_distorted: max_iterations must be in [0, 64]%s");
  return pixels_to_rays_impl("refnerf_pixels_to_rays_distorted", d_pix_x, d_pix_y, d_pixtocams, pixtocam_per_ray,
                             d_camtoworlds, camtoworld_per_ray, d_pixtocam_ndc, n, d_origins, d_directions, d_viewdirs,
                             d_radii, d_imageplane, distortion, stream);
}

int refnerf_image_rays(int32_t projection, int32_t width, int32_t height, const float *d_pixtocam, const float *d_camtoworlds,
                       int32_t n_frames, int32_t frame, const float *d_pixtocam_ndc, const refnerf_lens_distortion *distortion,
                       float near, float far, int64_t first, int32_t count, const refnerf_image_rays_out *out, void *stream) {
  if (projection != REFNERF_PROJ_PINHOLE && projection != REFNERF_PROJ_SPHERICAL)
    return fail(REFNERF_EINVAL, "refnerf_image_rays: unknown projection%s");
  const bool spherical = projection == REFNERF_PROJ_SPHERICAL;
  if (width <= 0 || height <= 0 || n_frames <= 0 || count <= 0)
    return fail(REFNERF_EINVAL, "refnerf_image_rays: width, height, n_frames and count must be positive%s");
  if (frame < 0 || frame >= n_frames) return fail(REFNERF_EINVAL, "refnerf_image_rays: frame outside [0, n_frames)%s");
  if (first < 0 || first + (int64_t)count > (int64_t)width * height)
    return fail(REFNERF_EINVAL, "refnerf_image_rays: [first, first + count) outside the image%s");
  if (!d_camtoworlds || !out || !out->d_origins || !out->d_directions || !out->d_viewdirs || !out->d_radii ||
      (!spherical && !d_pixtocam))
    return fail(REFNERF_EINVAL, "refnerf_image_rays: null pointer%s");
  if (spherical && (d_pixtocam_ndc || distortion))
    return fail(REFNERF_EINVAL, "refnerf_image_rays: the spherical projection takes neither NDC nor lens distortion%s");
  if (distortion) {
    const double c[7] = {distortion->k1, distortion->k2, distortion->k3, distortion->k4, distortion->p1, distortion->p2,
                         distortion->eps};
    for (double v : c)
      if (!std::isfinite(v)) return fail(REFNERF_EINVAL, "refnerf_image_rays: non-finite distortion parameter%s");
    if (distortion->max_iterations < 0 || distortion->max_iterations > REFNERF_MAX_UNDISTORT_ITERATIONS)
      return fail(REFNERF_EINVAL, "refnerf_image_rays: max_iterations must be in [0, 64]%s");
  }
  rn::ImageRaysArgs a{};
  a.width = width; a.height = height; a.first = first; a.count = count;
  a.pixtocam = d_pixtocam; a.camtoworld = d_camtoworlds + (size_t)12 * frame; a.pixtocam_ndc = d_pixtocam_ndc;
  a.near = near; a.far = far;
  a.cam_idx = spherical ? 0 : frame;      /* cast_spherical_rays broadcasts 0 whatever the frame (camera_utils.py:743) */
  a.origins = out->d_origins; a.directions = out->d_directions; a.viewdirs = out->d_viewdirs; a.radii = out->d_radii;
  a.imageplane = out->d_imageplane; a.lossmult = out->d_lossmult; a.near_out = out->d_near; a.far_out = out->d_far;
  a.cam_idx_out = out->d_cam_idx;
  const dim3 grid((unsigned)(((int64_t)count + 255) / 256)), block(256);
  if (spherical) {
    hipLaunchKernelGGL((rn::image_rays_kernel<true, false>), grid, block, 0, (hipStream_t)stream, a);
  } else if (distortion) {
    a.dist = {distortion->k1, distortion->k2, distortion->k3, distortion->k4, distortion->p1, distortion->p2, distortion->eps,
              distortion->max_iterations};
    hipLaunchKernelGGL((rn::image_rays_kernel<false, true>), grid, block, 0, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL((rn::image_rays_kernel<false, false>), grid, block, 0, (hipStream_t)stream, a);
  }
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_prepare_images(const void *d_src, int32_t src_is_f32, int64_t n, int32_t H, int32_t W, int32_t C, int32_t factor,
                           int32_t op, float *d_out, float *d_alpha, void *stream) {
  const char *fn = "refnerf_prepare_images";
  if (!d_src || !d_out) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (n <= 0 || H <= 0 || W <= 0) return fail(REFNERF_EINVAL, "%s: n, H and W must be positive", fn);
  if (C != 1 && C != 3 && C != 4) return fail(REFNERF_EINVAL, "%s: C must be 1, 3 or 4", fn);
  if (factor < 1) return fail(REFNERF_EINVAL, "%s: factor must be at least 1", fn);
  if (factor > 256) return fail(REFNERF_EINVAL, "%s: factor above 256 (a block sum of factor^2 bytes must stay below 2^24)", fn);
  if (H % factor != 0 || W % factor != 0) {
    char what[96];
    snprintf(what, sizeof(what), "refnerf_prepare_images: factor %d does not evenly divide image shape (%d, %d)", factor, H, W);
    return fail(REFNERF_EINVAL, "%s", what);
  }
  if (op < REFNERF_PREP_SCALE || op > REFNERF_PREP_RAW) return fail(REFNERF_EINVAL, "%s: unknown operation", fn);
  if (op == REFNERF_PREP_WHITE && C != 4) return fail(REFNERF_EINVAL, "%s: REFNERF_PREP_WHITE needs C = 4", fn);
  if (op == REFNERF_PREP_NORMALS && C < 3) return fail(REFNERF_EINVAL, "%s: REFNERF_PREP_NORMALS needs C >= 3", fn);
  if (d_alpha && op != REFNERF_PREP_WHITE) return fail(REFNERF_EINVAL, "%s: d_alpha is written by REFNERF_PREP_WHITE only", fn);
  if (((uintptr_t)d_out & 3u) || ((uintptr_t)d_alpha & 3u) || (src_is_f32 && ((uintptr_t)d_src & 3u)))
    return fail(REFNERF_EINVAL, "%s: misaligned float32 pointer", fn);
  rn::ImagePrepareArgs a{};
  a.src = d_src; a.H = H; a.W = W; a.h = H / factor; a.w = W / factor; a.factor = factor; a.op = op;
  a.out = d_out; a.alpha = d_alpha;
  if (n > ((int64_t)1 << 39) / ((int64_t)a.h * a.w)) return fail(REFNERF_EINVAL, "%s: more than 2^39 output pixels", fn);
  a.total = n * a.h * a.w;
  hipStream_t st = (hipStream_t)stream;
  long tslot;
  { int trc = timer_begin(st, &tslot, REFNERF_TIMER_DATASET); if (trc) return trc; }
  if (src_is_f32) {
    if (C == 1) rn::launch_image_prepare<float, 1, false>(a, st);
    else if (C == 3) rn::launch_image_prepare<float, 3, false>(a, st);
    else rn::launch_image_prepare<float, 4, false>(a, st);
  } else {
    if (C == 1) rn::launch_image_prepare<uint8_t, 1, false>(a, st);
    else if (C == 3) rn::launch_image_prepare<uint8_t, 3, false>(a, st);
    else if (((uintptr_t)d_src & 3u) == 0) rn::launch_image_prepare<uint8_t, 4, true>(a, st);   /* whole pixels as 32-bit words */
    else rn::launch_image_prepare<uint8_t, 4, false>(a, st);
  }
  HIP_TRY(hipGetLastError());
  return timer_end(st, tslot);
}

int refnerf_train_batch(const refnerf_train_batch_args *args, void *stream) {
  const char *fn = "refnerf_train_batch";
  if (!args) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  const refnerf_train_batch_args &g = *args;
  const refnerf_image_rays_out &o = g.rays;
  if (!g.d_px0 || !g.d_py0 || !g.d_cam || !g.d_images || !g.d_pixtocams || !g.d_camtoworlds || !g.d_rgb || !o.d_origins ||
      !o.d_directions || !o.d_viewdirs || !o.d_radii || !o.d_imageplane || !o.d_lossmult || !o.d_near || !o.d_far || !o.d_cam_idx)
    return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (g.n_patches <= 0 || g.patch_size <= 0 || g.n_images <= 0 || g.height <= 0 || g.width <= 0)
    return fail(REFNERF_EINVAL, "%s: n_patches, patch_size, n_images, height and width must be positive", fn);
  if (g.patch_size > g.height || g.patch_size > g.width) return fail(REFNERF_EINVAL, "%s: patch_size larger than the image", fn);
  const int64_t n = (int64_t)g.n_patches * g.patch_size * g.patch_size;
  if (n >= ((int64_t)1 << 31)) return fail(REFNERF_EINVAL, "%s: n_patches * patch_size^2 must be below 2^31", fn);
  if ((g.d_disps == nullptr) != (g.d_out_disps == nullptr) || (g.d_normals == nullptr) != (g.d_out_normals == nullptr) ||
      (g.d_alphas == nullptr) != (g.d_out_alphas == nullptr))
    return fail(REFNERF_EINVAL, "%s: disps / normals / alphas need both the stack and the output", fn);
  const refnerf_lens_distortion *dist = g.distortion;
  if (dist) {
    const double c[7] = {dist->k1, dist->k2, dist->k3, dist->k4, dist->p1, dist->p2, dist->eps};
    for (double v : c)
      if (!std::isfinite(v)) return fail(REFNERF_EINVAL, "%s: non-finite distortion parameter", fn);
    if (dist->max_iterations < 0 || dist->max_iterations > REFNERF_MAX_UNDISTORT_ITERATIONS)
      return fail(REFNERF_EINVAL, "%s: max_iterations must be in [0, 64]", fn);
  }
  rn::TrainBatchArgs a{};
  a.px0 = g.d_px0; a.py0 = g.d_py0; a.cam = g.d_cam; a.idx64 = g.index_is_int64 ? 1 : 0; a.cam_stride = g.cam_per_patch ? 1 : 0;
  a.ps = g.patch_size; a.n = (int)n;
  a.n_images = g.n_images; a.H = g.height; a.W = g.width;
  a.images = g.d_images; a.disps = g.d_disps; a.normals = g.d_normals; a.alphas = g.d_alphas;
  a.pixtocams = g.d_pixtocams; a.p2c_stride = g.pixtocam_per_camera ? 9 : 0;
  a.camtoworlds = g.d_camtoworlds; a.pixtocam_ndc = g.d_pixtocam_ndc;
  a.near = g.near; a.far = g.far;
  a.origins = o.d_origins; a.directions = o.d_directions; a.viewdirs = o.d_viewdirs; a.radii = o.d_radii;
  a.imageplane = o.d_imageplane; a.lossmult = o.d_lossmult; a.near_out = o.d_near; a.far_out = o.d_far; a.cam_idx_out = o.d_cam_idx;
  a.rgb = g.d_rgb; a.disps_out = g.d_out_disps; a.normals_out = g.d_out_normals; a.alphas_out = g.d_out_alphas;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + rn::DATASET_THREADS - 1) / rn::DATASET_THREADS)), block(rn::DATASET_THREADS);
  long tslot;
  { int trc = timer_begin(st, &tslot, REFNERF_TIMER_DATASET); if (trc) return trc; }
  if (dist) {
    a.dist = {dist->k1, dist->k2, dist->k3, dist->k4, dist->p1, dist->p2, dist->eps, dist->max_iterations};
    hipLaunchKernelGGL(rn::train_batch_kernel<true>, grid, block, 0, st, a);
  } else {
    hipLaunchKernelGGL(rn::train_batch_kernel<false>, grid, block, 0, st, a);
  }
  HIP_TRY(hipGetLastError());
  return timer_end(st, tslot);
}

int refnerf_mlp_forward(const void *d_packed, const refnerf_level_cfg *cfg, const float *d_means, const float *d_covs,
                        int32_t cov_is_full, const float *d_viewdirs, int32_t R, int32_t N, const refnerf_level_out *out,
                        void *stream) {
  if (!d_packed || !cfg || !d_means || !d_covs || !d_viewdirs || !out)
    return fail(REFNERF_EINVAL, "refnerf_mlp_forward: null pointer%s");
  if (R <= 0 || N <= 0) return fail(REFNERF_EINVAL, "refnerf_mlp_forward: R and N must be positive%s");
  if (cfg->precision != REFNERF_PREC_F32)
    return fail(REFNERF_EUNSUPPORTED, "refnerf_mlp_forward runs in the f32 precision mode only%s");
  int rpw = rays_per_wg(N, rn::T_TILE);
  if (rpw * N > 640) return fail(REFNERF_EINVAL, "n too large for the LDS budget (rays_per_wg*N must be <= 640)%s");
  const size_t lds = sizeof(float) * (size_t)(rn::DIR_PAD * rn::T_TILE + rn::HD_ROWS * rn::T_TILE + 2 * rpw * (N + 1) +
                                              rn::NPS_TRAIN * rpw * N + 3 * rn::T_TILE + 8);
  if (lds > 160 * 1024) return fail(REFNERF_EINVAL, "n too large for the 160 KiB LDS budget%s");
  if (cfg->ipe_groups < 0 || cfg->ipe_groups > rn::IPE_MAX_GROUPS) return fail(REFNERF_EINVAL, "ipe_groups must be in [0,7]%s");
  const bool gbasis = cfg->ipe_groups > 1;     /* d_packed then comes from refnerf_pack_weights_basis */
  LDS_ATTR_ONCE(lds_attr(rn::mlp_fwd_f32), lds_attr(rn::mlp_fwd_train_f32), lds_attr(rn::mlp_fwd_f32_gb), lds_attr(rn::mlp_fwd_train_f32_gb));
  rn::LevelArgs a{};
  a.packed = d_packed;
  a.cfg = *cfg;
  a.cfg.n_samples = N;
  a.rays.d_viewdirs = d_viewdirs;
  a.R = R;
  a.rpw = rpw;
  a.out = *out;
  a.prof = nullptr;
  a.g_means = d_means;
  a.g_covs = d_covs;
  a.cov_full = cov_is_full;
  const int grid = (R + rpw - 1) / rpw;
  if (gbasis && cfg->training) hipLaunchKernelGGL(rn::mlp_fwd_train_f32_gb, dim3(grid), dim3(rn::NTHREADS), lds, (hipStream_t)stream, a);
  else if (gbasis) hipLaunchKernelGGL(rn::mlp_fwd_f32_gb, dim3(grid), dim3(rn::NTHREADS), lds, (hipStream_t)stream, a);
  else if (cfg->training) hipLaunchKernelGGL(rn::mlp_fwd_train_f32, dim3(grid), dim3(rn::NTHREADS), lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(rn::mlp_fwd_f32, dim3(grid), dim3(rn::NTHREADS), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}


size_t refnerf_backward_workspace_bytes(int32_t R, int32_t n_samples) {
  if (R <= 0 || n_samples <= 1) return 0;
  return bwd_plan(R, n_samples).total;
}

size_t refnerf_activation_workspace_bytes(int32_t R, int32_t n_samples) {
  if (R <= 0 || n_samples <= 1) return 0;
  return bwd_plan(R, n_samples).act_bytes;
}

size_t refnerf_backward_workspace_bytes_basis(int32_t R, int32_t n_samples, int32_t ipe_groups) {
  if (R <= 0 || n_samples <= 1 || ipe_groups < 0 || ipe_groups > rn::IPE_MAX_GROUPS) return 0;
  return bwd_plan(R, n_samples, ipe_groups).total;
}

size_t refnerf_activation_workspace_bytes_basis(int32_t R, int32_t n_samples, int32_t ipe_groups) {
  if (R <= 0 || n_samples <= 1 || ipe_groups < 0 || ipe_groups > rn::IPE_MAX_GROUPS) return 0;
  return bwd_plan(R, n_samples, ipe_groups).act_bytes;
}

int refnerf_activations_format(const refnerf_level_cfg *cfg) {
  if (!cfg) return -1;
  if (cfg->precision == REFNERF_PREC_BF16) return REFNERF_ACT_BF16;
  if (cfg->precision == REFNERF_PREC_F16X2 && cfg->ipe_groups <= 1) return REFNERF_ACT_SQ;
  return REFNERF_ACT_F32;
}

int refnerf_level_backward(const void *d_packed, const refnerf_level_cfg *cfg, const refnerf_rays *rays, int32_t R,
                           const refnerf_level_saved *saved, const refnerf_level_grads *grads, float *d_param_grads,
                           void *d_workspace, size_t workspace_bytes, void *stream) {
  if (!d_packed || !cfg || !rays || !saved || !grads || !d_param_grads || !d_workspace)
    return fail(REFNERF_EINVAL, "refnerf_level_backward: null pointer%s");
  if (R <= 0) return fail(REFNERF_EINVAL, "refnerf_level_backward: R must be positive%s");
  if (cfg->n_samples <= 1) return fail(REFNERF_EINVAL, "num_samples must be > 1%s");
  if (cfg->ray_shape != 0 && cfg->ray_shape != 1) return fail(REFNERF_EINVAL, "ray_shape must be 'cone' or 'cylinder'%s");
  if (cfg->precision != REFNERF_PREC_F32 && cfg->precision != REFNERF_PREC_BF16 && cfg->precision != REFNERF_PREC_F16X2)
    return fail(REFNERF_EINVAL, "refnerf_level_backward: unknown precision mode (REFNERF_PREC_F32, REFNERF_PREC_F16X2 or REFNERF_PREC_BF16)%s");
  if (saved->activations_format == REFNERF_ACT_F16X2)
    return fail(REFNERF_EUNSUPPORTED, "activations_format REFNERF_ACT_F16X2 (the split-f16 pair units) is retired: no forward writes it, no backward reads it%s");
  if (cfg->precision == REFNERF_PREC_F16X2 && saved->activations_format != REFNERF_ACT_F32 && saved->activations_format != REFNERF_ACT_SQ)
    return fail(REFNERF_EUNSUPPORTED, "the split-f16 backward chains read the REFNERF_PREC_F16X2 forward's activations (REFNERF_ACT_SQ) or fp32 rows (REFNERF_PREC_F32, or a general IPE basis)%s");
  if (cfg->precision != REFNERF_PREC_F16X2 && saved->activations_format == REFNERF_ACT_SQ)
    return fail(REFNERF_EUNSUPPORTED, "activations written by the split-f16 training forward (REFNERF_ACT_SQ) are read by the split-f16 backward: cfg->precision = REFNERF_PREC_F16X2%s");
  if (cfg->wgrad_mode != REFNERF_WGRAD_F32 && cfg->wgrad_mode != REFNERF_WGRAD_BF16X3 && cfg->wgrad_mode != REFNERF_WGRAD_F16)
    return fail(REFNERF_EINVAL, "refnerf_level_backward: unknown wgrad_mode%s");
  if (cfg->wgrad_mode == REFNERF_WGRAD_F16 && saved->activations_format != REFNERF_ACT_SQ)
    return fail(REFNERF_EUNSUPPORTED, "wgrad_mode = REFNERF_WGRAD_F16 belongs to the REFNERF_PREC_F16X2 training kernels (REFNERF_ACT_SQ activations, written with the same wgrad_mode)%s");
  {
    /* the backward streams the image of the TRAINING level it belongs to, whatever cfg->training says */
    refnerf_level_cfg tc = *cfg;
    tc.training = 1;
    /* (the split-f16 backward on fp32 rows -- an exact-fp32 forward, or a general basis -- reads the f32 image) */
    if (tc.precision == REFNERF_PREC_F16X2 && saved->activations_format == REFNERF_ACT_F32) tc.precision = REFNERF_PREC_F32;
    if (int irc = check_image(d_packed, &tc, "refnerf_level_backward")) return irc;
  }
  if (!saved->d_sdist || !saved->d_density || !saved->d_rgb || !saved->d_weights || !grads->d_g_r_rgb)
    return fail(REFNERF_EINVAL, "refnerf_level_backward: null saved tensor / rendering gradient%s");
  if (!saved->d_activations)
    return fail(REFNERF_EINVAL, "refnerf_level_backward: the level was not run through refnerf_level_forward_train (no saved activations)%s");
  if (!rays->d_origins || !rays->d_directions || !rays->d_viewdirs || !rays->d_radii || !rays->d_near || !rays->d_far)
    return fail(REFNERF_EINVAL, "refnerf_level_backward: null ray field%s");
  const int N = cfg->n_samples;
  const bool gbasis = cfg->ipe_groups > 1;
  if (cfg->ipe_groups < 0 || cfg->ipe_groups > rn::IPE_MAX_GROUPS) return fail(REFNERF_EINVAL, "ipe_groups must be in [0,7]%s");
  if (gbasis && ((cfg->precision != REFNERF_PREC_F32 && cfg->precision != REFNERF_PREC_F16X2) || cfg->wgrad_mode != REFNERF_WGRAD_BF16X3 ||
                 saved->activations_format != REFNERF_ACT_F32))
    return fail(REFNERF_EUNSUPPORTED, "a general IPE basis (ipe_groups > 1) trains with the f32 or split-f16 chains and the bf16x3 weight-gradient GEMM%s");
  const BwdPlan plan = bwd_plan(R, N, cfg->ipe_groups);
  if (workspace_bytes < plan.total) return fail(REFNERF_EINVAL, "refnerf_level_backward: workspace too small (see refnerf_backward_workspace_bytes)%s");
  const int rpw = rays_per_wg(N, rn::T_TILE);
  size_t lds = sizeof(float) * (size_t)(rn::DIR_PAD * rn::T_TILE + rn::HD_ROWS * rn::T_TILE + rpw * (N + 1) + 8);
  const size_t ring_off = (lds + 15) / 16 * 16;
  if (cfg->precision == REFNERF_PREC_BF16)
    lds = ring_off + rn::RING_BYTES;       /* the chains' shared weight-stream ring */
  if (lds > 160 * 1024) return fail(REFNERF_EINVAL, "n_samples too large for the 160 KiB LDS budget%s");
  LDS_ATTR_ONCE(lds_attr(rn::level_bwd_f32), lds_attr(rn::level_bwd_bf16c), lds_attr(rn::level_bwd_f16x2c_r32),
                lds_attr(rn::wgrad_kernel, (rn::WG_TM + rn::WG_TN) * rn::WG_LDK * 4),
                lds_attr(rn::wgrad_bf16x3_kernel<false, false>, rn::wb_lds(false, false)),
                lds_attr(rn::wgrad_bf16x3_kernel<false, true>, rn::wb_lds(false, true)),
                lds_attr(rn::wgrad_bf16x3_kernel<true, false>, rn::wb_lds(true, false)),
                lds_attr(rn::wgrad_bf16x3_kernel<true, true>, rn::wb_lds(true, true)),
                lds_attr(rn::wgrad_bf16x3_kernel<false, false, true>, rn::wb_lds(false, false)));
  char *ws = (char *)d_workspace;
  rn::BwdArgs a;
  a.packed = d_packed;
  a.cfg = *cfg;
  a.rays = *rays;
  a.R = R;
  a.rpw = rpw;
  a.sdist = saved->d_sdist; a.density = saved->d_density; a.rgb = saved->d_rgb; a.weights = saved->d_weights;
  a.g_r_rgb = grads->d_g_r_rgb; a.g_weights = grads->d_g_weights; a.g_npred = grads->d_g_normals_pred;
  a.g_r_acc = grads->d_g_r_acc; a.g_r_dist = grads->d_g_r_distance;
  a.g_s_density = grads->d_g_density; a.g_s_rgb = grads->d_g_rgb; a.g_s_diffuse = grads->d_g_diffuse;
  a.g_s_specular = grads->d_g_specular; a.g_s_tint = grads->d_g_tint; a.g_s_rough = grads->d_g_roughness;
  a.act = (const float *)saved->d_activations;
  a.delta = (float *)(ws + plan.delta_off);
  a.seeds = (float *)(ws + plan.seed_off);
  a.pitch = plan.pitch;
  const bool act16 = saved->activations_format == REFNERF_ACT_BF16, del16 = cfg->precision == REFNERF_PREC_BF16;
  const bool sq = saved->activations_format == REFNERF_ACT_SQ;
  if (saved->activations_format != REFNERF_ACT_F32 && saved->activations_format != REFNERF_ACT_BF16 && !sq)
    return fail(REFNERF_EINVAL, "refnerf_level_backward: unknown activations_format%s");
  if (sq && gbasis) return fail(REFNERF_EUNSUPPORTED, "a general IPE basis keeps fp32 activation rows (REFNERF_ACT_F32)%s");
  if (sq && cfg->wgrad_mode != REFNERF_WGRAD_BF16X3 && cfg->wgrad_mode != REFNERF_WGRAD_F16)
    return fail(REFNERF_EUNSUPPORTED, "REFNERF_ACT_SQ activations go with wgrad_mode = REFNERF_WGRAD_BF16X3 (the f16 weight-gradient GEMM on the saved halves; "
                                      "fp32 weight-gradient products: the REFNERF_PREC_F32 chains)%s");
  if ((act16 || del16) && cfg->wgrad_mode != REFNERF_WGRAD_BF16X3)
    return fail(REFNERF_EUNSUPPORTED, "16-bit activation / delta rows (bf16 chains) need wgrad_mode = REFNERF_WGRAD_BF16X3 "
                                      "(fp32 weight-gradient products: the REFNERF_PREC_F32 chains)%s");
  a.act16 = act16 ? 1 : 0;
  a.ring_off = (int)ring_off;
  a.prof = nullptr;
  if (rt().prof) {
    int prc = prof_buffer(&a.prof);
    if (prc) return prc;
    HIP_TRY(hipMemset(a.prof, 0, 8 * 32 * sizeof(long long)));
  }
  hipStream_t st = (hipStream_t)stream;
  /* per-ray seeds first (one wave per ray), then the per-sample backward */
  hipLaunchKernelGGL(rn::bwd_seed_kernel, dim3((R + 3) / 4), dim3(rn::NTHREADS), sizeof(float) * 4 * (size_t)(N + 1), st, a);
  if (sq) {
    /* refnerf_sq_train.hip: the per-sample chains, then the f16 weight-gradient GEMM on (ACT_SQ, DELTA + factor units) */
    int rc = rnsq::backward_chain(d_packed, cfg, rays, R, saved->d_sdist, grads, a.act, a.delta, a.seeds, plan.pitch, st);
    if (rc) return rc;
    if (plan.pitch > plan.S) {
      hipLaunchKernelGGL(rn::wgrad_zero_tail, dim3(256), dim3(256), 0, st, const_cast<float *>(a.act), rn::AQ_MASK, rn::AQ_UNITS, plan.pitch, plan.S);
      hipLaunchKernelGGL(rn::wgrad_zero_tail, dim3(256), dim3(256), 0, st, a.delta, rn::DEL_ROWS / 2, rn::DQ_UNITS, plan.pitch, plan.S);
    }
    const int slices = (int)((plan.S + plan.k_per_slice - 1) / plan.k_per_slice);
    float *part = (float *)(ws + plan.part_off);
    int used = slices;
    rc = rnsq::wgrad(a.act, a.delta, plan.S, plan.pitch, plan.k_per_slice, slices, part, (float *)(ws + plan.cmin_off),
                     cfg->wgrad_mode == REFNERF_WGRAD_F16 ? 1 : 0, &used, st);
    if (rc) return rc;
    hipLaunchKernelGGL(rn::wgrad_reduce, dim3(1024), dim3(256), 0, st, part, used, d_param_grads, (int)rn::NUM_PARAMS);
    HIP_TRY(hipGetLastError());
    return REFNERF_OK;
  }
  /* d_packed is the f32 image in both modes (it carries the bf16 transposed ops behind the fp32 ones) */
  long tslot = -1;
  { int trc = timer_begin(st, &tslot, REFNERF_TIMER_BACKWARD); if (trc) return trc; }
  if (cfg->precision == REFNERF_PREC_BF16)
    hipLaunchKernelGGL(rn::level_bwd_bf16c, dim3((R + rpw - 1) / rpw), dim3(rn::NTHREADS), lds, st, a);
  else if (cfg->precision == REFNERF_PREC_F16X2)
    hipLaunchKernelGGL(rn::level_bwd_f16x2c_r32, dim3((R + rpw - 1) / rpw), dim3(rn::NTHREADS), lds, st, a);
  else
    hipLaunchKernelGGL(rn::level_bwd_f32, dim3((R + rpw - 1) / rpw), dim3(rn::NTHREADS), lds, st, a);
  HIP_TRY(hipGetLastError());
  { int trc = timer_end(st, tslot); if (trc) return trc; }
  if (a.prof) {   /* debug aid (REFNERF_PROF=1): cycle stamps of workgroup 0: prologue | heads recompute | rgb recompute + colour head | seed | dir chain | IDE / heads | spatial chain */
    long long hbuf[8 * 32];
    HIP_TRY(hipMemcpy(hbuf, a.prof, sizeof(hbuf), hipMemcpyDeviceToHost));
    for (int w = 0; w < 4; ++w) {
      fprintf(stderr, "[prof bwd] wave %d:", w);
      for (int sl = 1; sl <= 14; ++sl) fprintf(stderr, " %lld", hbuf[w * 32 + sl] ? hbuf[w * 32 + sl] - hbuf[w * 32] : -1LL);
      fprintf(stderr, "\n");
    }
  }
  if (plan.pitch > plan.S) {   /* pad columns of both operand matrices must read as zero in the wgrad GEMM */
    hipLaunchKernelGGL(rn::wgrad_zero_tail, dim3(256), dim3(256), 0, st, const_cast<float *>(a.act), act16 ? rn::ACT_ROWS / 2 : rn::ACT_ROWS, rn::act_units(act16), plan.pitch, plan.S);
    hipLaunchKernelGGL(rn::wgrad_zero_tail, dim3(256), dim3(256), 0, st, a.delta, del16 ? rn::DEL_ROWS / 2 : rn::DEL_ROWS,
                       rn::del_units(del16), plan.pitch, plan.S);
  }
  rn::WgradArgs w;
  w.act = a.act; w.delta = a.delta; w.a_units = rn::act_units(act16); w.d_units = rn::del_units(del16); w.pitch = plan.pitch; w.S = plan.S; w.k_per_slice = plan.k_per_slice;
  w.part = (float *)(ws + plan.part_off);
  const int slices = (int)((plan.S + plan.k_per_slice - 1) / plan.k_per_slice);
  { int trc = timer_begin(st, &tslot, REFNERF_TIMER_WGRAD); if (trc) return trc; }
  if (cfg->wgrad_mode == REFNERF_WGRAD_BF16X3)
  {
    const dim3 wg_grid(8 * ((slices + 7) / 8) * rn::WJOBS.tiles);
    if (del16 && act16) hipLaunchKernelGGL((rn::wgrad_bf16x3_kernel<true, true>), wg_grid, dim3(256), rn::wb_lds(true, true), st, w, slices);
    else if (del16) hipLaunchKernelGGL((rn::wgrad_bf16x3_kernel<true, false>), wg_grid, dim3(256), rn::wb_lds(true, false), st, w, slices);
    else if (act16) hipLaunchKernelGGL((rn::wgrad_bf16x3_kernel<false, true>), wg_grid, dim3(256), rn::wb_lds(false, true), st, w, slices);
    else hipLaunchKernelGGL((rn::wgrad_bf16x3_kernel<false, false>), wg_grid, dim3(256), rn::wb_lds(false, false), st, w, slices);
  }
  else
    hipLaunchKernelGGL(rn::wgrad_kernel, dim3(rn::WJOBS.tiles, slices), dim3(256), (rn::WG_TM + rn::WG_TN) * rn::WG_LDK * 4, st, w);
  HIP_TRY(hipGetLastError());
  { int trc = timer_end(st, tslot); if (trc) return trc; }
  hipLaunchKernelGGL(rn::wgrad_reduce, dim3(1024), dim3(256), 0, st, w.part, slices, d_param_grads, (int)rn::NUM_PARAMS);
  if (gbasis) {
    /* the tail of the parameter blob: dW_ext[L] = DELTA(layer 0 | 5) x (IPE features of groups 1..)^T, same kernel on the
     * tail matrix behind ACT and its own job table, partials behind the seeds */
    rn::WgradArgs we = w;
    we.act = (const float *)((const char *)saved->d_activations + plan.act_ext_off);
    we.a_units = rn::ACT_EXT_UNITS;
    we.part = (float *)(ws + plan.part_ext_off);
    if (plan.pitch > plan.S)
      hipLaunchKernelGGL(rn::wgrad_zero_tail, dim3(256), dim3(256), 0, st, const_cast<float *>(we.act), rn::ACT_EXT_ROWS, rn::ACT_EXT_UNITS, plan.pitch, plan.S);
    /* fewer than 7 groups (icosahedron / 1, octahedron / 2): the forward wrote the rows of groups 1..G-1 only; the GEMM
     * contracts all 576, so the others must read as zeros -- their gradient is then exactly 0, as the header promises */
    if (cfg->ipe_groups - 1 < rn::EXT_GROUPS)
      hipLaunchKernelGGL(rn::wgrad_zero_units, dim3(2048), dim3(256), 0, st, const_cast<float *>(we.act), (cfg->ipe_groups - 1) * rn::IPE_DIM,
                         rn::ACT_EXT_ROWS, rn::ACT_EXT_UNITS, plan.pitch);
    hipLaunchKernelGGL((rn::wgrad_bf16x3_kernel<false, false, true>), dim3(8 * ((slices + 7) / 8) * rn::WJOBS_EXT.tiles), dim3(256), rn::wb_lds(false, false), st, we, slices);
    hipLaunchKernelGGL(rn::wgrad_reduce, dim3(256), dim3(256), 0, st, we.part, slices, d_param_grads + rn::NUM_PARAMS, (int)rn::EXT_PARAMS);
  }
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_sample_intervals(const float *d_t, const float *d_logits, int32_t R, int32_t M, int32_t N,
                             float s_min, float s_max, float *d_sdist, int32_t *d_bin_idx, void *stream) {
  if (!d_t || !d_logits || !d_sdist) return fail(REFNERF_EINVAL, "refnerf_sample_intervals: null pointer%s");
  if (N <= 1) return fail(REFNERF_EINVAL, "num_samples must be > 1%s");
  if (M < 1 || M > 2048 || N > 2048 || R <= 0) return fail(REFNERF_EINVAL, "refnerf_sample_intervals: size out of range%s");
  size_t lds = sizeof(float) * 4 * (size_t)((M + 1) + M + (M + 1) + N + (N + 1) + 8);
  if (lds > 160 * 1024) return fail(REFNERF_EINVAL, "refnerf_sample_intervals: M,N too large%s");
  LDS_ATTR_ONCE(lds_attr(rn::sample_intervals_kernel));
  hipLaunchKernelGGL(rn::sample_intervals_kernel, dim3((R + 3) / 4), dim3(256), lds, (hipStream_t)stream,
                     d_t, d_logits, R, M, N, s_min, s_max, d_sdist, d_bin_idx);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_integrated_pos_enc(const float *d_lmean, const float *d_lvar, int32_t n, float *d_feat, void *stream) {
  if (!d_lmean || !d_lvar || !d_feat || n <= 0) return fail(REFNERF_EINVAL, "refnerf_integrated_pos_enc: bad argument%s");
  hipLaunchKernelGGL(rn::ipe_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_lmean, d_lvar, n, d_feat);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_integrated_dir_enc(const float *d_xyz, const float *d_kappa_inv, int32_t n, float *d_ide, void *stream) {
  if (!d_xyz || !d_kappa_inv || !d_ide || n <= 0) return fail(REFNERF_EINVAL, "refnerf_integrated_dir_enc: bad argument%s");
  hipLaunchKernelGGL(rn::ide_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_xyz, d_kappa_inv, n, d_ide);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_render_rays(const refnerf_level_cfg *cfg, int32_t R, const float *d_density, const float *d_tdist,
                        const float *d_directions, const float *d_far, const float *d_rgb, const float *d_diffuse,
                        const float *d_specular, const float *d_normals, const float *d_normals_pred,
                        const float *d_roughness, const float *d_tint, const refnerf_level_out *out, void *stream) {
  if (!cfg || !d_density || !d_tdist || !d_directions || !d_far || !out)
    return fail(REFNERF_EINVAL, "refnerf_render_rays: null pointer%s");
  const int N = cfg->n_samples;
  if (R <= 0 || N < 1 || N > 1024) return fail(REFNERF_EINVAL, "refnerf_render_rays: R must be positive and n_samples in [1,1024]%s");
  rn::RenderArgs a;
  a.cfg = *cfg;
  a.cfg.training = d_normals != nullptr;
  a.R = R;
  a.rpw = N <= 256 ? 4 : 1;
  a.density = d_density; a.tdist = d_tdist; a.dirs = d_directions; a.far = d_far;
  a.rgb = d_rgb; a.dif = d_diffuse; a.spc = d_specular; a.nrm = d_normals; a.npred = d_normals_pred;
  a.rough = d_roughness; a.tint = d_tint;
  a.out = *out;
  const size_t lds = sizeof(float) * ((size_t)a.rpw * (2 * (N + 1) + rn::NPS_TRAIN * N) + 4 * 22 * rn::WSUM_PITCH);
  LDS_ATTR_ONCE(lds_attr(rn::render_rays_kernel));
  hipLaunchKernelGGL(rn::render_rays_kernel, dim3((R + a.rpw - 1) / a.rpw), dim3(rn::NTHREADS), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_losses_forward(int32_t R, int32_t N, const float *d_r_rgb, const float *d_gt_rgb, const float *d_lossmult,
                           const float *d_weights, const float *d_orientation_normals, const float *d_normals,
                           const float *d_normals_pred, const float *d_viewdirs, float *d_terms, void *stream) {
  if (!d_r_rgb || !d_gt_rgb || !d_lossmult || !d_weights || !d_viewdirs || !d_terms || (d_normals && !d_normals_pred))
    return fail(REFNERF_EINVAL, "refnerf_losses_forward: null pointer%s");
  if (R <= 0 || N <= 0) return fail(REFNERF_EINVAL, "refnerf_losses_forward: R and N must be positive%s");
  rn::LossArgs a{};
  a.R = R; a.N = N; a.rgb = d_r_rgb; a.gt = d_gt_rgb; a.lossmult = d_lossmult; a.weights = d_weights;
  a.normals_o = d_orientation_normals; a.normals = d_normals; a.normals_pred = d_normals_pred; a.viewdirs = d_viewdirs;
  a.terms = d_terms;
  hipLaunchKernelGGL(rn::refnerf_losses_fwd_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_losses_backward(int32_t R, int32_t N, const float *d_r_rgb, const float *d_gt_rgb, const float *d_lossmult,
                            const float *d_weights, const float *d_orientation_normals, int32_t orientation_on_pred,
                            const float *d_normals, const float *d_normals_pred, const float *d_viewdirs,
                            float g_data, float g_orientation, float g_normal, const float *d_upstream,
                            float *d_g_r_rgb, float *d_g_weights, float *d_g_normals_pred, void *stream) {
  if (!d_r_rgb || !d_gt_rgb || !d_lossmult || !d_weights || !d_viewdirs || !d_g_r_rgb || !d_g_weights || !d_g_normals_pred ||
      (d_normals && !d_normals_pred))
    return fail(REFNERF_EINVAL, "refnerf_losses_backward: null pointer%s");
  if (R <= 0 || N < 3) return fail(REFNERF_EINVAL, "refnerf_losses_backward: R must be positive and N >= 3%s");
  rn::LossArgs a{};
  a.R = R; a.N = N; a.rgb = d_r_rgb; a.gt = d_gt_rgb; a.lossmult = d_lossmult; a.weights = d_weights;
  a.normals_o = d_orientation_normals; a.orient_on_pred = orientation_on_pred; a.normals = d_normals;
  a.normals_pred = d_normals_pred; a.viewdirs = d_viewdirs;
  a.g_data = g_data; a.g_orient = g_orientation; a.g_normal = g_normal; a.upstream = d_upstream;
  a.g_rgb = d_g_r_rgb; a.g_weights = d_g_weights; a.g_npred = d_g_normals_pred;
  const size_t n = (size_t)R * N;
  hipLaunchKernelGGL(rn::refnerf_losses_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

/* ---- the six geometry regularisers and the perturbed-ray sampler (refnerf_regularisers.h) ---- */
namespace {
static int check_regularisers(const refnerf_regularisers_args *a, const char *fn) {
  if (!a || !a->d_acc) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (a->R <= 0 || a->S <= 0) return fail(REFNERF_EINVAL, "%s: R and S must be positive", fn);
  if (a->n < 0 || a->n > a->R) return fail(REFNERF_EINVAL, "%s: n must be in [0, R]", fn);
  if (a->n > 0 && a->a <= 0) return fail(REFNERF_EINVAL, "%s: a must be positive when n > 0", fn);
  for (int t : {a->diffuse_type, a->specular_type})
    if (t != REFNERF_CONSISTENCY_MSE && t != REFNERF_CONSISTENCY_AVG_MSE && t != REFNERF_CONSISTENCY_VAR)
      return fail(REFNERF_EINVAL, "%s: unknown consistency loss type (REFNERF_CONSISTENCY_*)", fn);
  if (a->distance_type != REFNERF_CONSISTENCY_MSE)
    return fail(REFNERF_EINVAL, "%s: the distance consistency type must be REFNERF_CONSISTENCY_MSE", fn);
  /* a term is given whole (clean and noisy side; the distance term with the four ray tensors) or not at all */
  if (!a->d_diffuse != !a->d_n_diffuse || !a->d_specular != !a->d_n_specular || !a->d_normals != !a->d_n_normals ||
      !a->d_distance != !a->d_n_distance ||
      (a->d_distance && (!a->d_origins || !a->d_directions || !a->d_n_origins || !a->d_n_directions)))
    return fail(REFNERF_EINVAL, "%s: a consistency term needs its clean and its noisy tensors (distance: the rays as well)", fn);
  return REFNERF_OK;
}
}  // namespace

int refnerf_ray_regularisers_forward(const refnerf_regularisers_args *args, void *stream) {
  if (int rc = check_regularisers(args, "refnerf_ray_regularisers_forward")) return rc;
  if (!args->d_terms) return fail(REFNERF_EINVAL, "refnerf_ray_regularisers_forward: null pointer%s");
  hipLaunchKernelGGL(rn::ray_regularisers_fwd_kernel, dim3((args->R + 3) / 4), dim3(256), 0, (hipStream_t)stream, *args);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_ray_regularisers_backward(const refnerf_regularisers_args *args, void *stream) {
  const char *fn = "refnerf_ray_regularisers_backward";
  if (int rc = check_regularisers(args, fn)) return rc;
  if (!args->d_sums || !args->d_scales) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (args->d_g_weights && !args->d_weights) return fail(REFNERF_EINVAL, "%s: d_g_weights without d_weights", fn);
  /* a gradient is written for a term that is on, to both sides */
  if ((args->d_g_diffuse && !args->d_diffuse) || (args->d_g_specular && !args->d_specular) ||
      (args->d_g_normals && !args->d_normals) || (args->d_g_distance && !args->d_distance) ||
      !args->d_g_diffuse != !args->d_g_n_diffuse || !args->d_g_specular != !args->d_g_n_specular ||
      !args->d_g_normals != !args->d_g_n_normals || !args->d_g_distance != !args->d_g_n_distance)
    return fail(REFNERF_EINVAL, "%s: a consistency term's gradient needs the term's inputs and both output tensors", fn);
  const size_t n = args->d_g_weights ? (size_t)args->R * args->S : (size_t)args->R;
  hipLaunchKernelGGL(rn::ray_regularisers_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *args);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_noisy_rays(const refnerf_noisy_rays_args *args, void *stream) {
  if (!args) return fail(REFNERF_EINVAL, "refnerf_noisy_rays: null pointer%s");
  const void *ptrs[] = {args->d_rotations, args->d_distance, args->d_origins, args->d_directions, args->d_viewdirs, args->d_radii,
                        args->d_imageplane, args->d_lossmult, args->d_near, args->d_far, args->d_cam_idx, args->d_out_origins,
                        args->d_out_directions, args->d_out_viewdirs, args->d_out_radii, args->d_out_imageplane, args->d_out_lossmult,
                        args->d_out_near, args->d_out_far, args->d_out_cam_idx};
  for (const void *p : ptrs)
    if (!p) return fail(REFNERF_EINVAL, "refnerf_noisy_rays: null pointer%s");
  if (args->n <= 0 || args->a <= 0) return fail(REFNERF_EINVAL, "refnerf_noisy_rays: n and a must be positive%s");
  const size_t total = (size_t)args->n * args->a;
  if (total > (size_t)INT32_MAX) return fail(REFNERF_EINVAL, "refnerf_noisy_rays: n * a must be below 2^31%s");
  hipLaunchKernelGGL(rn::noisy_rays_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *args);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

/* ---- the data term with either penalty, its statistics, and the patch depth smoothness (refnerf_data_terms.h) ---- */
namespace {
static int check_data_terms(const refnerf_data_terms_args *a, const char *fn) {
  if (!a || !a->d_rgb || !a->d_gt_rgb || !a->d_lossmult) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (a->R <= 0) return fail(REFNERF_EINVAL, "%s: R must be positive", fn);
  if (a->penalty != REFNERF_PENALTY_MSE && a->penalty != REFNERF_PENALTY_CHARB)
    return fail(REFNERF_EINVAL, "%s: unknown penalty (REFNERF_PENALTY_*)", fn);
  if (!std::isfinite(a->charb_padding) || a->charb_padding < 0.0f)
    return fail(REFNERF_EINVAL, "%s: charb_padding must be finite and not negative", fn);
  /* an optional group is given whole or not at all */
  if (!a->d_distance_mean != !a->d_disps)
    return fail(REFNERF_EINVAL, "%s: the disparity statistic needs d_distance_mean and d_disps", fn);
  const int n_normal = !!a->d_acc + !!a->d_alphas + !!a->d_normals + !!a->d_normals_gt;
  if (n_normal != 0 && n_normal != 4)
    return fail(REFNERF_EINVAL, "%s: the normal statistic needs d_acc, d_alphas, d_normals and d_normals_gt", fn);
  return REFNERF_OK;
}

static int check_depth_smoothness(const refnerf_depth_smoothness_args *a, const char *fn) {
  if (!a || !a->d_distance || !a->d_acc || !a->d_rgb) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (a->P <= 0) return fail(REFNERF_EINVAL, "%s: P must be positive", fn);
  if (a->S < 2) return fail(REFNERF_EINVAL, "%s: S must be at least 2", fn);
  if ((int64_t)a->P * a->S * a->S >= ((int64_t)1 << 31)) return fail(REFNERF_EINVAL, "%s: P * S * S must be below 2^31", fn);
  return REFNERF_OK;
}
}  // namespace

int refnerf_data_terms_forward(const refnerf_data_terms_args *args, void *stream) {
  const char *fn = "refnerf_data_terms_forward";
  if (int rc = check_data_terms(args, fn)) return rc;
  if (!args->d_terms) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  hipLaunchKernelGGL(rn::data_terms_fwd_kernel, dim3((args->R + 255) / 256), dim3(256), 0, (hipStream_t)stream, *args);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_data_terms_backward(const refnerf_data_terms_args *args, void *stream) {
  const char *fn = "refnerf_data_terms_backward";
  if (int rc = check_data_terms(args, fn)) return rc;
  if (!args->d_upstream || !args->d_g_rgb) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  hipLaunchKernelGGL(rn::data_terms_bwd_kernel, dim3((args->R + 255) / 256), dim3(256), 0, (hipStream_t)stream, *args);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_depth_smoothness_forward(const refnerf_depth_smoothness_args *args, void *stream) {
  const char *fn = "refnerf_depth_smoothness_forward";
  if (int rc = check_depth_smoothness(args, fn)) return rc;
  if (!args->d_terms) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  hipLaunchKernelGGL(rn::depth_smoothness_fwd_kernel, dim3((args->P + 3) / 4), dim3(256), 0, (hipStream_t)stream, *args);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_depth_smoothness_backward(const refnerf_depth_smoothness_args *args, void *stream) {
  const char *fn = "refnerf_depth_smoothness_backward";
  if (int rc = check_depth_smoothness(args, fn)) return rc;
  if (!args->d_upstream || !args->d_g_distance) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  const size_t n = (size_t)args->P * args->S * args->S;
  hipLaunchKernelGGL(rn::depth_smoothness_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *args);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

/* ---- dilation between proposal levels and the interlevel loss (refnerf_proposal.h) ---- */
int refnerf_max_dilate_weights(const float *d_t, const float *d_w, int32_t R, int32_t M, float dilation, float domain_lo,
                               float domain_hi, float *d_t_out, float *d_w_out, void *stream) {
  if (R < 0) return fail(REFNERF_EINVAL, "refnerf_max_dilate_weights: R must not be negative%s");
  if (M < 1 || M > rn::DILATE_MAX_M)
    return fail(REFNERF_EINVAL, "refnerf_max_dilate_weights: M must be in [1,171] (the dilated step function has 3 M - 2 intervals; the resampler takes at most 512)%s");
  if (R == 0) return REFNERF_OK;                           /* nothing to do: the pointers are not looked at */
  if (!d_t || !d_w || !d_t_out || !d_w_out) return fail(REFNERF_EINVAL, "refnerf_max_dilate_weights: null pointer%s");
  hipLaunchKernelGGL(rn::max_dilate_weights_kernel, dim3((R + rn::PROP_WAVES - 1) / rn::PROP_WAVES), dim3(64 * rn::PROP_WAVES), 0,
                     (hipStream_t)stream, d_t, d_w, R, M, dilation, domain_lo, domain_hi, d_t_out, d_w_out);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

namespace {
static int check_interlevel(const char *fn, int32_t R, int32_t N, int32_t Np) {
  if (R < 0) return fail(REFNERF_EINVAL, "%s: R must not be negative", fn);
  if (N < 1 || N > rn::INTERLEVEL_MAX_N || Np < 1 || Np > rn::INTERLEVEL_MAX_N)
    return fail(REFNERF_EINVAL, "%s: N and Np must be in [1,512]", fn);
  return REFNERF_OK;
}
}  // namespace

int refnerf_interlevel_forward(const float *d_t, const float *d_w, const float *d_t_env, const float *d_w_env, int32_t R,
                               int32_t N, int32_t Np, float *d_ray_loss, void *stream) {
  const char *fn = "refnerf_interlevel_forward";
  if (int rc = check_interlevel(fn, R, N, Np)) return rc;
  if (R == 0) return REFNERF_OK;
  if (!d_t || !d_w || !d_t_env || !d_w_env || !d_ray_loss) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  hipLaunchKernelGGL(rn::interlevel_fwd_kernel, dim3((R + rn::PROP_WAVES - 1) / rn::PROP_WAVES), dim3(64 * rn::PROP_WAVES), 0,
                     (hipStream_t)stream, d_t, d_w, d_t_env, d_w_env, R, N, Np, d_ray_loss);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_interlevel_backward(const float *d_t, const float *d_w, const float *d_t_env, const float *d_w_env, int32_t R,
                                int32_t N, int32_t Np, const float *d_upstream, float *d_g_w_env, void *stream) {
  const char *fn = "refnerf_interlevel_backward";
  if (int rc = check_interlevel(fn, R, N, Np)) return rc;
  if (R == 0) return REFNERF_OK;
  if (!d_t || !d_w || !d_t_env || !d_w_env || !d_upstream || !d_g_w_env) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  hipLaunchKernelGGL(rn::interlevel_bwd_kernel, dim3((R + rn::PROP_WAVES - 1) / rn::PROP_WAVES), dim3(64 * rn::PROP_WAVES), 0,
                     (hipStream_t)stream, d_t, d_w, d_t_env, d_w_env, R, N, Np, d_upstream, d_g_w_env);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

/* ---- the optimiser step (refnerf_optim.h) ---- */
namespace {
struct OptimLayout { size_t max_items, items_off, partials_off, segitem_off, total; };
bool optim_layout(int64_t n, int32_t n_seg, OptimLayout *L) {
  if (n <= 0 || n > INT32_MAX || n_seg <= 0 || (int64_t)n_seg > n) return false;
  L->max_items = (size_t)((n + rn::OPTIM_CHUNK - 1) / rn::OPTIM_CHUNK) + (size_t)n_seg;
  L->items_off = 0;
  L->partials_off = L->max_items * sizeof(rn::OptimItem);
  L->segitem_off = L->partials_off + L->max_items * 4 * sizeof(float);
  L->total = L->segitem_off + (((size_t)n_seg + 1) * sizeof(int32_t) + 15) / 16 * 16;
  return true;
}
}  // namespace

size_t refnerf_optim_workspace_bytes(int64_t n_elements, int32_t n_segments) {
  OptimLayout L;
  return optim_layout(n_elements, n_segments, &L) ? L.total : 0;
}

size_t refnerf_optim_state_bytes(int32_t max_tensors) {
  return max_tensors <= 0 ? 0 : rn::OPTIM_STATE_HEADER + (size_t)max_tensors * sizeof(rn::OptimDesc);
}

int refnerf_optim_plan(int64_t n, const int32_t *seg_off, int32_t n_seg, void *d_workspace, size_t workspace_bytes,
                       int32_t *n_items, void *stream) {
  OptimLayout L;
  if (!seg_off || !d_workspace || !n_items) return fail(REFNERF_EINVAL, "refnerf_optim_plan: null pointer%s");
  if (!optim_layout(n, n_seg, &L)) return fail(REFNERF_EINVAL, "refnerf_optim_plan: n must be in [1, 2^31) and n_seg in [1, n]%s");
  if (workspace_bytes < L.total || ((uintptr_t)d_workspace & 15u)) return fail(REFNERF_EINVAL, "refnerf_optim_plan: workspace too small or not 16-byte aligned%s");
  if (seg_off[0] != 0 || (int64_t)seg_off[n_seg] != n) return fail(REFNERF_EINVAL, "refnerf_optim_plan: the segment table does not tile [0, n)%s");
  for (int32_t s = 0; s < n_seg; ++s)
    if (seg_off[s + 1] <= seg_off[s]) return fail(REFNERF_EINVAL, "refnerf_optim_plan: the segment table does not tile [0, n) (offsets must increase)%s");
  std::vector<unsigned char> img(L.total, 0);
  rn::OptimItem *items = reinterpret_cast<rn::OptimItem *>(img.data() + L.items_off);
  int32_t *seg_item = reinterpret_cast<int32_t *>(img.data() + L.segitem_off);
  int32_t k = 0;
  for (int32_t s = 0; s < n_seg; ++s) {
    seg_item[s] = k;
    for (int32_t at = seg_off[s]; at < seg_off[s + 1]; at += rn::OPTIM_CHUNK) {
      const int32_t len = seg_off[s + 1] - at < rn::OPTIM_CHUNK ? seg_off[s + 1] - at : rn::OPTIM_CHUNK;
      items[k++] = rn::OptimItem{s, at, len, 0};
    }
  }
  seg_item[n_seg] = k;
  if ((size_t)k > L.max_items) return fail(REFNERF_EINVAL, "refnerf_optim_plan: internal error (work items)%s");
  /* a setup call: the host image must outlive the copy */
  HIP_TRY(hipMemcpyAsync(d_workspace, img.data(), L.total, hipMemcpyHostToDevice, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  *n_items = k;
  return REFNERF_OK;
}

int refnerf_optim_stats(const float *d_grad, const float *d_param, int64_t n, int32_t n_seg, int32_t n_items,
                        double grad_max_val, void *d_workspace, size_t workspace_bytes, float *d_seg_stats,
                        void *d_state, size_t state_bytes, int32_t slot, void *stream) {
  OptimLayout L;
  if (!d_grad || !d_param || !d_workspace || !d_seg_stats || !d_state) return fail(REFNERF_EINVAL, "refnerf_optim_stats: null pointer%s");
  if (!optim_layout(n, n_seg, &L)) return fail(REFNERF_EINVAL, "refnerf_optim_stats: n must be in [1, 2^31) and n_seg in [1, n]%s");
  if (workspace_bytes < L.total || ((uintptr_t)d_workspace & 15u)) return fail(REFNERF_EINVAL, "refnerf_optim_stats: workspace too small or not 16-byte aligned%s");
  if (n_items < n_seg || (size_t)n_items > L.max_items) return fail(REFNERF_EINVAL, "refnerf_optim_stats: n_items is not what refnerf_optim_plan returned%s");
  if (((uintptr_t)d_grad & 3u) || ((uintptr_t)d_param & 3u) || ((uintptr_t)d_state & 15u)) return fail(REFNERF_EINVAL, "refnerf_optim_stats: misaligned pointer%s");
  if (slot < 0 || state_bytes < refnerf_optim_state_bytes(slot + 1)) return fail(REFNERF_EINVAL, "refnerf_optim_stats: slot outside the state%s");
  unsigned char *ws = static_cast<unsigned char *>(d_workspace);
  rn::OptimDesc d;
  d.seg_item_off = reinterpret_cast<const int32_t *>(ws + L.segitem_off);
  d.partials = reinterpret_cast<const float *>(ws + L.partials_off);
  d.seg_stats = d_seg_stats;
  d.n_seg = n_seg;
  d.n_items = n_items;
  rn::OptimDesc *slot_ptr = reinterpret_cast<rn::OptimDesc *>(static_cast<unsigned char *>(d_state) + rn::OPTIM_STATE_HEADER) + slot;
  hipLaunchKernelGGL(rn::optim_stats_kernel, dim3((unsigned)n_items), dim3(rn::OPTIM_THREADS), 0, (hipStream_t)stream, d_grad, d_param,
                     (int32_t)n, reinterpret_cast<const rn::OptimItem *>(ws + L.items_off), reinterpret_cast<float *>(ws + L.partials_off),
                     (float)grad_max_val, d, slot_ptr);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_optim_finalize(void *d_state, size_t state_bytes, int32_t n_tensors, double grad_max_norm, void *stream) {
  if (!d_state || ((uintptr_t)d_state & 15u)) return fail(REFNERF_EINVAL, "refnerf_optim_finalize: null or misaligned state%s");
  if (n_tensors <= 0 || state_bytes < refnerf_optim_state_bytes(n_tensors)) return fail(REFNERF_EINVAL, "refnerf_optim_finalize: n_tensors outside the state%s");
  hipLaunchKernelGGL(rn::optim_finalize_kernel, dim3(1), dim3(rn::OPTIM_THREADS), 0, (hipStream_t)stream,
                     static_cast<unsigned char *>(d_state), n_tensors, (float)grad_max_norm);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_optim_adam_step(float *d_param, float *d_grad, float *d_exp_avg, float *d_exp_avg_sq, int64_t n,
                            const refnerf_adam_cfg *cfg, const void *d_state, void *stream) {
  if (!cfg || !d_grad || !d_state) return fail(REFNERF_EINVAL, "refnerf_optim_adam_step: null pointer%s");
  if (!cfg->no_step && (!d_param || !d_exp_avg || !d_exp_avg_sq)) return fail(REFNERF_EINVAL, "refnerf_optim_adam_step: null pointer%s");
  if (cfg->no_step && !cfg->write_grad) return fail(REFNERF_EINVAL, "refnerf_optim_adam_step: no_step without write_grad does nothing%s");
  if (n <= 0 || n > INT32_MAX) return fail(REFNERF_EINVAL, "refnerf_optim_adam_step: n must be in [1, 2^31)%s");
  if (((uintptr_t)d_param | (uintptr_t)d_grad | (uintptr_t)d_exp_avg | (uintptr_t)d_exp_avg_sq | (uintptr_t)d_state) & 3u)
    return fail(REFNERF_EINVAL, "refnerf_optim_adam_step: misaligned pointer%s");
  if (!cfg->no_step && !(cfg->bias_correction1 > 0.0 && cfg->sqrt_bias_correction2 > 0.0))
    return fail(REFNERF_EINVAL, "refnerf_optim_adam_step: bias corrections must be positive (t >= 1)%s");
  rn::OptimAdamArgs a;
  a.p = d_param; a.g = d_grad; a.m = d_exp_avg; a.v = d_exp_avg_sq;
  a.n = (int32_t)n;
  a.grad_max_val = (float)cfg->grad_max_val;
  a.w1 = (float)(1.0 - cfg->beta1); a.beta2 = (float)cfg->beta2; a.w2 = (float)(1.0 - cfg->beta2);
  a.step_size = cfg->no_step ? 0.0f : (float)(cfg->lr / cfg->bias_correction1);
  a.sqrt_bc2 = (float)cfg->sqrt_bias_correction2; a.eps = (float)cfg->eps;
  a.write_grad = cfg->write_grad; a.no_step = cfg->no_step;
  a.clip_coef = static_cast<const float *>(d_state) + 1;
  const int64_t nvec = (n + 3) / 4;
  int64_t blocks = (nvec + rn::OPTIM_THREADS - 1) / rn::OPTIM_THREADS;
  blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
  hipLaunchKernelGGL(rn::optim_adam_kernel, dim3((unsigned)blocks), dim3(rn::OPTIM_THREADS), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

/* ---- test-image evaluation (refnerf_image.h) ---- */
namespace {
struct ImageLayout { size_t sq_blocks, px_blocks, ssim_tiles, scratch /* doubles shared by the reductions */, total /* bytes */; };
bool image_layout(int32_t H, int32_t W, int32_t C, ImageLayout *L) {
  if (H <= 0 || W <= 0 || C < 1 || C > 4 || (int64_t)H * W * C > INT32_MAX) return false;
  const int64_t npix = (int64_t)H * W;
  L->sq_blocks = (size_t)((npix * C + rn::IMG_ELEMS_PER_BLOCK - 1) / rn::IMG_ELEMS_PER_BLOCK);
  L->px_blocks = (size_t)((npix + rn::IMG_PIX_PER_BLOCK - 1) / rn::IMG_PIX_PER_BLOCK);
  L->ssim_tiles = 0;
  if (H >= rn::SSIM_TAPS && W >= rn::SSIM_TAPS)
    L->ssim_tiles = (size_t)((H - rn::SSIM_TAPS + rn::SSIM_TILE) / rn::SSIM_TILE) * (size_t)((W - rn::SSIM_TAPS + rn::SSIM_TILE) / rn::SSIM_TILE);
  L->scratch = L->sq_blocks;
  if (2 * L->px_blocks > L->scratch) L->scratch = 2 * L->px_blocks;
  if (L->ssim_tiles > L->scratch) L->scratch = L->ssim_tiles;
  /* colour correction: the warp [10][3] (32 doubles), then [px_blocks][3][65] partials */
  L->total = (L->scratch + 32 + L->px_blocks * 3 * rn::CC_PART) * sizeof(double);
  return true;
}
int check_image_pair(const char *fn, const void *a, int64_t pitch_a, const void *b, int64_t pitch_b, int32_t H, int32_t W, int32_t C,
                     const void *d_out, const void *ws, ImageLayout *L) {
  if (!a || !b || !d_out || !ws) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (C < 1 || C > 4) return fail(REFNERF_EINVAL, "%s: C must be in [1,4]", fn);
  if (!image_layout(H, W, C, L)) return fail(REFNERF_EINVAL, "%s: H and W must be positive and H * W * C below 2^31", fn);
  if (pitch_a < (int64_t)W * C || pitch_b < (int64_t)W * C) return fail(REFNERF_EINVAL, "%s: a row pitch below W * C", fn);
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)d_out | (uintptr_t)ws) & 7u) return fail(REFNERF_EINVAL, "%s: misaligned pointer", fn);
  return REFNERF_OK;
}
int image_finalize(hipStream_t st, const double *partials, size_t n_part, int n_val, int mode, double denom, double *d_out) {
  hipLaunchKernelGGL(rn::image_finalize_kernel, dim3(1), dim3(rn::IMG_THREADS), 0, st, partials, (int32_t)n_part, n_val, mode, denom, d_out);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}
}  // namespace

size_t refnerf_image_workspace_bytes(int32_t H, int32_t W, int32_t C) {
  ImageLayout L;
  return image_layout(H, W, C, &L) ? L.total : 0;
}

int refnerf_image_mse(const double *d_a, int64_t pitch_a, const double *d_b, int64_t pitch_b, int32_t H, int32_t W, int32_t C,
                      int32_t quantize_a, double *d_out, void *d_workspace, size_t workspace_bytes, void *stream) {
  const char *fn = "refnerf_image_mse";
  ImageLayout L;
  if (int rc = check_image_pair(fn, d_a, pitch_a, d_b, pitch_b, H, W, C, d_out, d_workspace, &L)) return rc;
  if (workspace_bytes < L.sq_blocks * sizeof(double)) return fail(REFNERF_EINVAL, "%s: workspace too small (see refnerf_image_workspace_bytes)", fn);
  hipStream_t st = (hipStream_t)stream;
  double *partials = static_cast<double *>(d_workspace);
  const int64_t n = (int64_t)H * W * C;
  long tslot;
  { int trc = timer_begin(st, &tslot, REFNERF_TIMER_IMAGE); if (trc) return trc; }
  hipLaunchKernelGGL(rn::image_sqerr_kernel, dim3((unsigned)L.sq_blocks), dim3(rn::IMG_THREADS), 0, st, d_a, pitch_a, d_b, pitch_b,
                     W * C, n, quantize_a ? 1 : 0, partials);
  HIP_TRY(hipGetLastError());
  if (int rc = image_finalize(st, partials, L.sq_blocks, 1, rn::IMG_FIN_MSE_PSNR, (double)n, d_out)) return rc;
  return timer_end(st, tslot);
}

int refnerf_image_ssim(const double *d_a, int64_t pitch_a, const double *d_b, int64_t pitch_b, int32_t H, int32_t W, int32_t C,
                       int32_t quantize_a, double *d_out, double *d_map, void *d_workspace, size_t workspace_bytes, void *stream) {
  const char *fn = "refnerf_image_ssim";
  ImageLayout L;
  if (int rc = check_image_pair(fn, d_a, pitch_a, d_b, pitch_b, H, W, C, d_out, d_workspace, &L)) return rc;
  if (H < rn::SSIM_TAPS || W < rn::SSIM_TAPS) return fail(REFNERF_EINVAL, "%s: H and W must be at least 11 (the filter's support)", fn);
  if ((uintptr_t)d_map & 7u) return fail(REFNERF_EINVAL, "%s: misaligned pointer", fn);
  if (workspace_bytes < L.ssim_tiles * sizeof(double)) return fail(REFNERF_EINVAL, "%s: workspace too small (see refnerf_image_workspace_bytes)", fn);
  rn::SsimTaps taps;
  double sum = 0.0;
  for (int i = 0; i < rn::SSIM_TAPS; ++i) {
    const double z = (i - 5) / 1.5;
    taps.g[i] = std::exp(-0.5 * (z * z));
    sum += taps.g[i];
  }
  for (int i = 0; i < rn::SSIM_TAPS; ++i) taps.g[i] /= sum;
  hipStream_t st = (hipStream_t)stream;
  double *partials = static_cast<double *>(d_workspace);
  const int OH = H - (rn::SSIM_TAPS - 1), OW = W - (rn::SSIM_TAPS - 1);
  const dim3 grid((unsigned)((OW + rn::SSIM_TILE - 1) / rn::SSIM_TILE), (unsigned)((OH + rn::SSIM_TILE - 1) / rn::SSIM_TILE));
  long tslot;
  { int trc = timer_begin(st, &tslot, REFNERF_TIMER_IMAGE); if (trc) return trc; }
  hipLaunchKernelGGL(rn::image_ssim_kernel, grid, dim3(rn::IMG_THREADS), 0, st, d_a, pitch_a, d_b, pitch_b, H, W, C, quantize_a ? 1 : 0,
                     taps, partials, d_map);
  HIP_TRY(hipGetLastError());
  if (int rc = image_finalize(st, partials, (size_t)grid.x * grid.y, 1, rn::IMG_FIN_MEAN, (double)OH * OW * C, d_out)) return rc;
  return timer_end(st, tslot);
}

int refnerf_color_correct(const double *d_img, int64_t pitch_img, const double *d_ref, int64_t pitch_ref, int32_t H, int32_t W,
                          int32_t C, int32_t num_iters, double eps, double *d_out, double *d_warp, void *d_workspace,
                          size_t workspace_bytes, void *stream) {
  const char *fn = "refnerf_color_correct";
  ImageLayout L;
  if (C != 3) return fail(REFNERF_EINVAL, "%s: C must be 3", fn);
  if (int rc = check_image_pair(fn, d_img, pitch_img, d_ref, pitch_ref, H, W, C, d_out, d_workspace, &L)) return rc;
  if (num_iters < 0 || num_iters > 64) return fail(REFNERF_EINVAL, "%s: num_iters must be in [0, 64]", fn);
  if (!std::isfinite(eps)) return fail(REFNERF_EINVAL, "%s: non-finite eps", fn);
  if ((uintptr_t)d_warp & 7u) return fail(REFNERF_EINVAL, "%s: misaligned pointer", fn);
  if (workspace_bytes < L.total) return fail(REFNERF_EINVAL, "%s: workspace too small (see refnerf_image_workspace_bytes)", fn);
  hipStream_t st = (hipStream_t)stream;
  double *warp = static_cast<double *>(d_workspace) + L.scratch, *partials = warp + 32;
  const int64_t npix = (int64_t)H * W;
  const dim3 apply_grid((unsigned)((npix + rn::IMG_THREADS - 1) / rn::IMG_THREADS));
  long tslot;
  { int trc = timer_begin(st, &tslot, REFNERF_TIMER_IMAGE); if (trc) return trc; }
  if (num_iters == 0) {
    hipLaunchKernelGGL(rn::cc_apply_kernel, apply_grid, dim3(rn::IMG_THREADS), 0, st, d_img, pitch_img, d_out, W, npix, (const double *)nullptr);
    HIP_TRY(hipGetLastError());
  }
  for (int it = 0; it < num_iters; ++it) {
    /* the current estimate: the input itself, then the dense output (updated in place) */
    const double *x = it == 0 ? d_img : d_out;
    const int64_t pitch_x = it == 0 ? pitch_img : (int64_t)W * 3;
    hipLaunchKernelGGL(rn::cc_accum_kernel, dim3((unsigned)L.px_blocks, 3), dim3(rn::IMG_THREADS), 0, st, x, pitch_x, d_img, pitch_img,
                       d_ref, pitch_ref, W, npix, eps, partials);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rn::cc_solve_kernel, dim3(1), dim3(rn::IMG_THREADS), 0, st, partials, (int32_t)L.px_blocks, warp,
                       it == num_iters - 1 ? d_warp : (double *)nullptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rn::cc_apply_kernel, apply_grid, dim3(rn::IMG_THREADS), 0, st, x, pitch_x, d_out, W, npix, (const double *)warp);
    HIP_TRY(hipGetLastError());
  }
  return timer_end(st, tslot);
}

int refnerf_weighted_mae(const double *d_weights, const double *d_normals, const double *d_normals_gt, int64_t n, double *d_out,
                         void *d_workspace, size_t workspace_bytes, void *stream) {
  const char *fn = "refnerf_weighted_mae";
  if (!d_weights || !d_normals || !d_normals_gt || !d_out || !d_workspace) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (n <= 0 || n > INT32_MAX / 3) return fail(REFNERF_EINVAL, "%s: n must be positive and 3 n below 2^31", fn);
  if (((uintptr_t)d_weights | (uintptr_t)d_normals | (uintptr_t)d_normals_gt | (uintptr_t)d_out | (uintptr_t)d_workspace) & 7u)
    return fail(REFNERF_EINVAL, "%s: misaligned pointer", fn);
  const size_t blocks = (size_t)((n + rn::IMG_PIX_PER_BLOCK - 1) / rn::IMG_PIX_PER_BLOCK);
  if (workspace_bytes < 2 * blocks * sizeof(double)) return fail(REFNERF_EINVAL, "%s: workspace too small (see refnerf_image_workspace_bytes)", fn);
  hipStream_t st = (hipStream_t)stream;
  double *partials = static_cast<double *>(d_workspace);
  long tslot;
  { int trc = timer_begin(st, &tslot, REFNERF_TIMER_IMAGE); if (trc) return trc; }
  hipLaunchKernelGGL(rn::image_wmae_kernel, dim3((unsigned)blocks), dim3(rn::IMG_THREADS), 0, st, d_weights, d_normals, d_normals_gt, n, partials);
  HIP_TRY(hipGetLastError());
  if (int rc = image_finalize(st, partials, blocks, 2, rn::IMG_FIN_DEGREES, 1.0, d_out)) return rc;
  return timer_end(st, tslot);
}

/* ---- validation visualisations (refnerf_vis.h) ---- */
namespace {
bool vis_misaligned(const void *p, int f64) { return ((uintptr_t)p & (f64 ? 7u : 3u)) != 0; }
}  // namespace

size_t refnerf_vis_percentile_workspace_bytes(int64_t n) {
  if (n < 2 || n > INT32_MAX) return 0;
  const size_t blocks = (size_t)((n + rn::VIS_SCAN_BLOCK - 1) / rn::VIS_SCAN_BLOCK);
  return ((size_t)n + 2 * blocks + REFNERF_VIS_MAX_PS) * sizeof(double);
}

int refnerf_vis_weighted_percentile(const void *d_values, int32_t values_f64, const void *d_weights, int32_t weights_f64,
                                    int64_t n_weights, const void *d_nan_mask, const int64_t *d_order, int64_t n, const double *ps,
                                    int32_t n_ps, int32_t target_f32, double *d_out, void *d_workspace, size_t workspace_bytes,
                                    void *stream) {
  const char *fn = "refnerf_vis_weighted_percentile";
  if (!d_values || !d_order || !ps || !d_out || !d_workspace) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (n < 2 || n > INT32_MAX) return fail(REFNERF_EINVAL, "%s: n must be in [2, 2^31) (the interpolation needs two knots)", fn);
  if (n_ps < 1 || n_ps > REFNERF_VIS_MAX_PS) return fail(REFNERF_EINVAL, "%s: n_ps must be in [1, 8]", fn);
  if (d_weights && (n_weights < 1 || n_weights > n)) return fail(REFNERF_EINVAL, "%s: n_weights must be in [1, n]", fn);
  if (d_nan_mask && !d_weights) return fail(REFNERF_EINVAL, "%s: d_nan_mask needs d_weights", fn);
  if (vis_misaligned(d_values, values_f64) || vis_misaligned(d_weights, weights_f64) || vis_misaligned(d_nan_mask, weights_f64) ||
      (((uintptr_t)d_order | (uintptr_t)d_out | (uintptr_t)d_workspace) & 7u))
    return fail(REFNERF_EINVAL, "%s: misaligned pointer", fn);
  if (workspace_bytes < refnerf_vis_percentile_workspace_bytes(n))
    return fail(REFNERF_EINVAL, "%s: workspace too small (see refnerf_vis_percentile_workspace_bytes)", fn);
  rn::VisPctArgs a{};
  a.values = d_values; a.weights = d_weights; a.nan_mask = d_nan_mask; a.order = d_order;
  a.n = n; a.n_weights = d_weights ? n_weights : 1;
  a.values_f64 = values_f64 ? 1 : 0; a.weights_f64 = weights_f64 ? 1 : 0; a.n_ps = n_ps; a.target_f32 = target_f32 ? 1 : 0;
  for (int p = 0; p < n_ps; ++p) a.ps[p] = ps[p];
  a.n_blocks = (n + rn::VIS_SCAN_BLOCK - 1) / rn::VIS_SCAN_BLOCK;
  a.acc = static_cast<double *>(d_workspace);
  a.block_sums = a.acc + n;
  a.block_offs = a.block_sums + a.n_blocks;
  a.counts = reinterpret_cast<unsigned long long *>(a.block_offs + a.n_blocks);
  a.out = d_out;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)a.n_blocks), block(rn::VIS_THREADS);
  hipLaunchKernelGGL(rn::vis_scan_partial_kernel, grid, block, 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(rn::vis_scan_blocks_kernel, dim3(1), dim3(64), 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(rn::vis_scan_final_kernel, grid, block, 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(rn::vis_pct_count_kernel, grid, block, 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(rn::vis_pct_final_kernel, dim3(1), dim3(64), 0, st, a);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_vis_panels(const refnerf_vis_panels_args *args, void *stream) {
  const char *fn = "refnerf_vis_panels";
  if (!args) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (args->H <= 0 || args->W <= 0 || (int64_t)args->H * args->W * 3 > INT32_MAX)
    return fail(REFNERF_EINVAL, "%s: H and W must be positive and 3 H W below 2^31", fn);
  if (args->d_table && args->table_n < 1) return fail(REFNERF_EINVAL, "%s: table_n must be positive", fn);
  if (args->d_roughness && (args->roughness_channels < 1 || args->roughness_channels > 4))
    return fail(REFNERF_EINVAL, "%s: roughness_channels must be in [1, 4]", fn);
  if ((args->d_depth_mean || args->d_depth_median) && !(args->d_table && args->d_acc))
    return fail(REFNERF_EINVAL, "%s: the depth panels need d_table and d_acc", fn);
  const int64_t npix = (int64_t)args->H * args->W;
  hipLaunchKernelGGL(rn::vis_panels_kernel, dim3((unsigned)((npix + rn::VIS_THREADS - 1) / rn::VIS_THREADS)), dim3(rn::VIS_THREADS), 0,
                     (hipStream_t)stream, *args);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_vis_cmap(const refnerf_vis_cmap_args *args, void *stream) {
  const char *fn = "refnerf_vis_cmap";
  if (!args || !args->d_values || !args->d_out) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (args->H <= 0 || args->W <= 0 || (int64_t)args->H * args->W * 4 > INT32_MAX)
    return fail(REFNERF_EINVAL, "%s: H and W must be positive and 4 H W below 2^31", fn);
  if (args->channels < 1 || args->channels > 4) return fail(REFNERF_EINVAL, "%s: channels must be in [1, 4]", fn);
  if (args->d_table && (args->channels != 1 || args->table_n < 1))
    return fail(REFNERF_EINVAL, "%s: a table needs one channel and table_n >= 1", fn);
  if (args->curve < REFNERF_VIS_CURVE_NONE || args->curve > REFNERF_VIS_CURVE_LOG) return fail(REFNERF_EINVAL, "%s: unknown curve", fn);
  const int64_t npix = (int64_t)args->H * args->W;
  hipLaunchKernelGGL(rn::vis_cmap_kernel, dim3((unsigned)((npix + rn::VIS_THREADS - 1) / rn::VIS_THREADS)), dim3(rn::VIS_THREADS), 0,
                     (hipStream_t)stream, *args);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_vis_resample_rays(const void *d_sdist, const void *d_values, const void *d_weights, int32_t f64, int32_t n, int32_t N,
                              int32_t C, const double *d_edges, int32_t resolution, int32_t accumulate, int32_t value_op,
                              int64_t line_stride, double *d_out_values, double *d_out_alpha, void *stream) {
  const char *fn = "refnerf_vis_resample_rays";
  if (!d_sdist || !d_values || !d_edges || !d_out_values || !d_out_alpha) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (n < 1 || N < 1 || C < 1 || C > 4 || resolution < 1 || line_stride < 1)
    return fail(REFNERF_EINVAL, "%s: n, N, resolution and line_stride must be positive and C in [1, 4]", fn);
  const size_t lds = (size_t)(N + 1) * (C + 3) * sizeof(double);
  if (lds > 48 * 1024) return fail(REFNERF_EINVAL, "%s: (N + 1) (C + 3) doubles must fit 48 KB of LDS", fn);
  if ((int64_t)n * line_stride * resolution * C > INT32_MAX) return fail(REFNERF_EINVAL, "%s: the lines exceed 2^31 elements", fn);
  if (value_op < REFNERF_VIS_OP_NONE || value_op > REFNERF_VIS_OP_SQRT) return fail(REFNERF_EINVAL, "%s: unknown value_op", fn);
  rn::VisResampleArgs a{};
  a.sdist = d_sdist; a.values = d_values; a.weights = d_weights; a.edges = d_edges;
  a.out_values = d_out_values; a.out_alpha = d_out_alpha; a.line_stride = line_stride;
  a.f64 = f64 ? 1 : 0; a.n = n; a.N = N; a.C = C; a.resolution = resolution; a.accumulate = accumulate ? 1 : 0; a.value_op = value_op;
  hipLaunchKernelGGL(rn::vis_resample_kernel, dim3((unsigned)n), dim3(rn::VIS_THREADS), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_vis_ray_panel(const double *d_lines_values, const double *d_lines_alpha, int32_t n, int32_t L, int32_t resolution,
                          int32_t C, int32_t rep, double bg_color, const double *d_alpha_max, double *d_out_vis, double *d_out_alpha,
                          void *stream) {
  const char *fn = "refnerf_vis_ray_panel";
  if (!d_lines_values || !d_lines_alpha || !d_out_vis || !d_out_alpha) return fail(REFNERF_EINVAL, "%s: null pointer", fn);
  if (n < 1 || L < 1 || resolution < 1 || C < 1 || C > 4 || rep < 0) return fail(REFNERF_EINVAL, "%s: bad sizes", fn);
  const int64_t rows = rep > 0 ? (int64_t)n * ((int64_t)L * rep + 1) - 1 : (int64_t)(n - 1) * L;
  if (rows * resolution * C > INT32_MAX) return fail(REFNERF_EINVAL, "%s: the panel exceeds 2^31 elements", fn);
  if (rows == 0) return REFNERF_OK;
  const int64_t npix = rows * resolution;
  hipLaunchKernelGGL(rn::vis_ray_panel_kernel, dim3((unsigned)((npix + rn::VIS_THREADS - 1) / rn::VIS_THREADS)), dim3(rn::VIS_THREADS), 0,
                     (hipStream_t)stream, d_lines_values, d_lines_alpha, L, resolution, C, rep, rows, bg_color, d_alpha_max, d_out_vis,
                     d_out_alpha);
  HIP_TRY(hipGetLastError());
  return REFNERF_OK;
}

int refnerf_set_timing(int enable) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> lk(r.mu);
  r.timing = enable != 0;
  r.events_used = 0;
  return REFNERF_OK;
}
int refnerf_get_timing_family(int family, double *total_ms, int64_t *launches) {
  Runtime &r = rt();
  std::lock_guard<std::mutex> lk(r.mu);
  double tot = 0.0;
  int64_t n = 0;
  for (size_t i = 0; i < r.events_used; ++i) {
    if (r.family[i] != family) continue;
    HIP_TRY(hipEventSynchronize(r.events[i].second));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, r.events[i].first, r.events[i].second));
    tot += ms;
    n += 1;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = n;
  return REFNERF_OK;
}
int refnerf_get_timing(double *total_ms, int64_t *launches) {
  return refnerf_get_timing_family(REFNERF_TIMER_FORWARD, total_ms, launches);
}

}  /* extern "C" */
