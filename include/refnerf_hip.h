/*
 * refnerf_hip.h -- C ABI of the MI355X (gfx950) Ref-NeRF rendering inner loop.
 *
 * Shared library: refnerf-pl_amd/csrc/librefnerf_hip.so.  Plain pointers and
 * sizes only; every `d_*` pointer is DEVICE memory owned by the caller; every
 * call is asynchronous on `stream` (a hipStream_t passed as void*, NULL = the
 * default stream) and returns 0 or a negative REFNERF_E* code (message via
 * refnerf_last_error()).  Level / stage calls keep no state between calls and
 * may be issued concurrently from several host threads (each on its own
 * stream); the error string is per thread.  The only process-wide state is the
 * opt-in kernel timer of refnerf_set_timing / refnerf_get_timing (mutex-guarded)
 * and two debug knobs read once from the environment (REFNERF_PROF,
 * REFNERF_LDS_PAD).
 *
 * The upstream reference (minfenli/refnerf-pl) has no FFI: its boundary is the
 * Python call surface of internal/models.py.  Each entry point below names the
 * reference function (file:line, relative to the upstream repo root) whose
 * ATen op sequence it replaces; INTEGRATION.md shows the ctypes binding a
 * maintainer adds on the reference side.
 */
#ifndef REFNERF_HIP_H
#define REFNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REFNERF_ABI_VERSION 11  /* (additive since v11, no layout changed: refnerf_level_forward_ex / refnerf_level_forward_train_ex + refnerf_level_out_extra, and d_sdist_in = d_weights_in = NULL for the initial step function in all four level-forward entries) v11:refnerf_level_image (which weight image a level configuration expects as d_packed) + the library remembers the kind of every image it packs and refuses a mismatching d_packed; v10: REFNERF_IMAGE_F16X2_TRAIN + REFNERF_ACT_SQ (training levels of REFNERF_PREC_F16X2 on the eval kernel's skeleton: d_packed of refnerf_level_forward_train / refnerf_level_backward is the train image then); v9: REFNERF_ACT_F16X2 (split-f16 ACT / DELTA formats of the split-f16 training chains), refnerf_activations_format; v8: cfg.ipe_groups, refnerf_pack_weights_basis (general IPE bases: icosahedron); v7: REFNERF_PREC_F16X2 (split-operand f16: the parity-grade 16-bit inference mode); v6: cfg.dir_enc (REFNERF_DIRENC_*), cfg.raydist (REFNERF_RAYDIST_*), cfg.disable_integration; v5: refnerf_render_rays, REFNERF_PREC_F16, refnerf_get_timing_family, refnerf_losses_forward / _backward; v4: cfg.wgrad_mode, refnerf_level_saved.activations_format, bf16-chain training modes */
#define REFNERF_NUM_PARAMS 1110158 /* canonical fp32 blob, nerf_mlp.* state_dict order */

enum {
  REFNERF_OK = 0,
  REFNERF_EINVAL = -1,      /* bad argument / unsupported configuration     */
  REFNERF_ENOGPU = -2,      /* no gfx950 device                             */
  REFNERF_EHIP = -3,        /* HIP runtime error                            */
  REFNERF_EUNSUPPORTED = -4 /* valid in the reference, not built here yet   */
};

/* arithmetic of the MLP contractions */
enum {
  REFNERF_PREC_F32 = 0,  /* v_mfma_f32_32x32x2_f32: exact fp32 fma chains (parity mode) */
  REFNERF_PREC_BF16 = 1, /* v_mfma_f32_32x32x16_bf16, fp32 accumulate (training forward / backward in
                            this mode: n_samples <= 294, REFNERF_EINVAL beyond -- LDS budget)  */
  REFNERF_PREC_F16 = 2,  /* v_mfma_f32_32x32x16_f16 (IEEE half operands, fp32 accumulate): the bf16 inference kernel
                            with 11 instead of 8 significand bits -- 8-10x closer to REFNERF_PREC_F32 at ~3 % lower
                            throughput; hidden activations must stay below 65504.  refnerf_level_forward only. */
  REFNERF_PREC_F16X2 = 3 /* split-operand f16: in the spatial trunk and the density / scalar head block BOTH operands are
                            hi + lo pairs of IEEE halves (22 significand bits; the partial products hi*hi + lo*hi + hi*lo
                            on v_mfma_f32_16x16x32_f16, fp32 accumulate; lo*lo = 2^-22 of a product is dropped), the
                            directional trunk is plain f16; resampler,
                            encodings, activations and compositing are the fp32 parity code.  The 16-bit mode that holds
                            the reference's fp32 nn.Linear arithmetic (internal/models.py:576-580, 686-700) on trained
                            weights: every ray within max(1e-4, 4 x the reference's own fp32 rounding error) of the float64
                            value of the same function (131 k rays; worst ray 1.8e-4 from the fp32 reference, 1.6e-4 from
                            float64 where the reference itself is 1.6e-4 off; within 1e-4 of the fp32 reference on all but <= 2
                            rays of a batch of 8192: tests/test_hip_f16x2.py);
                            ~1.5x the matrix cycles of REFNERF_PREC_F16.  Range: the hi halves are IEEE
                            halves, so weights and hidden activations must stay below 65504 in magnitude (a trained
                            Ref-NeRF's reach ~1e2; checked up to 8e3: 1e-6).  Beyond it a unit becomes hi = inf, lo = -inf, the
                            next layer's accumulators NaN; the ReLUs of the split kernels (inference, training chains, general
                            basis) let a NaN through, so the ray's outputs are NaN: loud, never a finite wrong colour.
                            REFNERF_PREC_F32 has no such limit.
                            refnerf_level_forward_train / refnerf_level_backward in this mode, built-in IPE basis (v10):
                            the eval kernel's skeleton on the REFNERF_IMAGE_F16X2_TRAIN image -- spatial trunk and
                            density-normal VJP W_hi x_hi + W_lo x_hi + W_hi x_lo, directional trunk [W_hi | W_lo] x on one
                            half of x, backward W^T (22 bits) x delta (11 bits); saved activations REFNERF_ACT_SQ (then the
                            backward must run in this mode too).  General basis: the f32 skeleton with three-product
                            contractions, REFNERF_ACT_F32.  MEASURED gradient rel-L2 from the reference's autograd (GPU
                            fixtures, tests/test_hip_f16x2.py): 3.5e-5 (shiny) .. 8.1e-5 (llff) .. 1.1e-4 (trained-like),
                            1.6e-4 (icosahedron basis); trained_long 1.5e-3 in EVERY chain mode incl. f32 (level-1 sample
                            positions on a sharp surface, not arithmetic); between the chain modes from identical step
                            functions 7e-5 .. 2.7e-4.  Strict gradient parity = REFNERF_PREC_F32 chains; 22-bit deltas on
                            fp32 rows = f32 forward + this mode's backward (level_bwd_f16x2c_r32: 2e-6 between the modes). */
};

/* arithmetic of the weight-gradient GEMM of refnerf_level_backward (dW = DELTA x ACT^T over the samples) */
enum {
  REFNERF_WGRAD_F32 = 0,    /* v_mfma_f32_32x32x2_f32: fp32 products                                     */
  REFNERF_WGRAD_BF16X3 = 1, /* the 16-bit-MFMA GEMM that goes with the chains (default).  After f32 chains: operands split hi + lo into
                               bf16 pairs, hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16, fp32 accumulate: 2^-16 per product,
                               HBM-bound.  After REFNERF_PREC_F16X2 chains (REFNERF_ACT_SQ): the f16 GEMM on the saved halves --
                               spatial layer inputs hi + lo (22 bits), directional layer inputs and every delta ONE half.
                               After bf16 chains: bf16 rows. */
  REFNERF_WGRAD_F16 = 2     /* v10, REFNERF_PREC_F16X2 training levels on the built-in basis only (set it in the cfg of BOTH
                               refnerf_level_forward_train and refnerf_level_backward): the spatial layer inputs at ONE half as
                               well -- the forward does not write their lo halves, the GEMM does not read them: 17.4 instead of
                               21.7 KB of weight-gradient operands per ray-sample, one MFMA product per tile.  A layer input's
                               rounding is independent per sample, so it averages over the batch where a weight's does not:
                               scripts/exp_train_sq_precision.py measures +1 .. 5 % on the gradient's distance from the
                               reference's autograd (three trained weight sets). */
};

/* element type of the saved layer inputs: fp32 rows (f32 training forward; any forward with a general IPE basis), bf16 rows
 * (bf16-chain training forward, whose activations are bf16-exact: half the stream; rows 2j and 2j+1 share the dwords of
 * pair-row j, low / high half) or REFNERF_ACT_SQ (below).  REFNERF_ACT_F16X2 = 2 is RETIRED: it named the pair units of an
 * earlier generation of the split-f16 training kernels; the number stays reserved, refnerf_activations_format never returns it
 * and refnerf_level_backward answers it with REFNERF_EUNSUPPORTED.  The buffer is opaque to the caller, only its size is part
 * of the ABI.  refnerf_activations_format(cfg) tells which one refnerf_level_forward_train
 * writes for a configuration: pass it on in refnerf_level_saved.activations_format. */
enum { REFNERF_ACT_F32 = 0, REFNERF_ACT_BF16 = 1, REFNERF_ACT_F16X2 = 2 /* retired */,
       REFNERF_ACT_SQ = 3 /* v10: what the REFNERF_PREC_F16X2 training forward writes on the built-in basis: spatial layer inputs as
                             hi / lo pair units, directional layer inputs as the ONE half their trunk multiplies, lane-local ReLU
                             sign words, the raw scalar head rows and raw rgb (13.7 KB per ray-sample; the buffer keeps the size
                             refnerf_activation_workspace_bytes reports); the backward writes its deltas as one half per element
                             + two power-of-two factors per (layer, sample): 22 KB of weight-gradient operands per ray-sample */ };

/* a weight image that is not an arithmetic mode of refnerf_level_forward: refnerf_pack_weights / refnerf_packed_weights_bytes
 * take it in place of a REFNERF_PREC_* code */
enum {
  REFNERF_IMAGE_F16X2_TRAIN = 4 /* v10: forward + transposed operands of the REFNERF_PREC_F16X2 TRAINING kernels (built-in IPE
                                   basis) as one stream of 17 KB chunks (11.5 MB): d_packed of refnerf_level_forward_train and
                                   refnerf_level_backward when cfg.precision = REFNERF_PREC_F16X2 and cfg.ipe_groups <= 1
                                   (a general basis and the other precisions keep the REFNERF_PREC_F32 image) */
};

/* encoding of the (reflected) direction fed to the directional MLP (internal/models.py:484-492) */
enum {
  REFNERF_DIRENC_IDE = 0,    /* MLP.use_directional_enc = True: ref_utils.generate_ide_fn(5), 72 features                 */
  REFNERF_DIRENC_POSENC = 1  /* False: coord.pos_enc(d, 0, 5, append_identity) (coord.py:136-147), its 33 features in the
                                slots [x y z | sin(2^j d_i) j-major | 0 x18 || sin(2^j d_i + pi/2) | 0 x21] of the same 72-wide
                                block (the caller embeds the [.., 33] weight columns there; the roughness is not used)   */
};

/* Model.raydist_fn: the bijection between normalised and metric ray distance (coord.construct_ray_warps, coord.py:63-99):
 * t = fn_inv(s * fn(far) + (1 - s) * fn(near)) */
enum {
  REFNERF_RAYDIST_NONE = 0,        /* fn = None: linear in t                                   */
  REFNERF_RAYDIST_PIECEWISE = 1,   /* 'piecewise': x < 1 ? x / 2 : 1 - 1 / (2 x) (allows near = 0) */
  REFNERF_RAYDIST_RECIPROCAL = 2,  /* torch.reciprocal (linear in disparity)                   */
  REFNERF_RAYDIST_LOG = 3, REFNERF_RAYDIST_EXP = 4, REFNERF_RAYDIST_SQRT = 5, REFNERF_RAYDIST_SQUARE = 6
};

enum { REFNERF_SRGB_NONE = 0, REFNERF_SRGB_LINEAR = 1, REFNERF_SRGB_NORM_LINEAR = 2,
       REFNERF_SRGB_SRGB = 3, REFNERF_SRGB_NORM_SRGB = 4 };

/* One sampling level of Model.__call__ (internal/models.py:162-306).
 * Field-for-field the knobs the reference reads on this path. */
typedef struct refnerf_level_cfg {
  int32_t n_samples;          /* Model.num_prop_samples / num_nerf_samples (models.py:164) */
  int32_t n_in;               /* intervals of the incoming step function (1 at level 0)    */
  int32_t training;           /* MLP.training: also emit density-gradient normals (:603)   */
  int32_t compute_extras;     /* models.py:133                                             */
  int32_t srgb_mapping;       /* MLP.srgb_mapping (:712)                                   */
  int32_t srgb_mapping_normalization; /* (:718)                                           */
  int32_t render_srgb_mode;   /* Config.srgb_mapping_type if srgb_mapping_when_rendering (:285-287) */
  int32_t opaque_background;  /* Model.opaque_background (render.py:139-143)               */
  int32_t ray_shape;          /* 0 'cone', 1 'cylinder' (render.py:121-126)                */
  int32_t precision;          /* REFNERF_PREC_*                                            */
  int32_t wgrad_mode;         /* REFNERF_WGRAD_*: arithmetic of the weight-gradient GEMM (backward only) */
  int32_t dir_enc;            /* REFNERF_DIRENC_*: MLP.use_directional_enc (:484-492)      */
  int32_t raydist;            /* REFNERF_RAYDIST_*: Model.raydist_fn (:147, coord.py:63-99) */
  int32_t disable_integration;/* Model.disable_integration (:228-231): zero covariances -> plain positional encoding */
  int32_t ipe_groups;         /* MLP.basis_shape / basis_subdivisions (:384-385, 482-484): 0 or 1 = the octahedron/1 basis the kernels are
                                 built around; G = 2..7: 3 G basis directions, d_packed from refnerf_pack_weights_basis */
  float anneal;               /* models.py:190-195                                         */
  float resample_padding;     /* Model.resample_padding (:202)                             */
  float s_near, s_far;        /* Model.init_s_near / init_s_far (:213)                     */
  float density_bias;         /* MLP.density_bias (:623)                                   */
  float roughness_bias;       /* MLP.roughness_bias (:641)                                 */
  float rgb_premultiplier, rgb_bias, rgb_padding; /* (:700, :729)                          */
  float bg_rgb;               /* Model.bg_intensity_range midpoint (:261-267)              */
} refnerf_level_cfg;

void refnerf_level_cfg_default(refnerf_level_cfg *cfg);

/* utils.Rays (internal/utils.py:51-93): the six fields the path reads. */
typedef struct refnerf_rays {
  const float *d_origins;    /* [R,3] */
  const float *d_directions; /* [R,3] */
  const float *d_viewdirs;   /* [R,3] */
  const float *d_radii;      /* [R]   */
  const float *d_near;       /* [R]   */
  const float *d_far;        /* [R]   */
} refnerf_rays;

/* Outputs of one level; any pointer may be NULL (not stored).
 * Per-sample = ray_history[l] (models.py:731-750, 304-305),
 * per-ray = renderings[l] (render.py:152-254). */
typedef struct refnerf_level_out {
  float *d_sdist;        /* [R,N+1] */
  int32_t *d_bin_idx;    /* [R,N]   CDF bin of each sample centre (math.py:93) */
  float *d_density;      /* [R,N]   */
  float *d_rgb;          /* [R,N,3] */
  float *d_normals;      /* [R,N,3] training only */
  float *d_normals_pred; /* [R,N,3] */
  float *d_grad_pred;    /* [R,N,3] */
  float *d_tint;         /* [R,N,3] */
  float *d_diffuse;      /* [R,N,3] */
  float *d_specular;     /* [R,N,3] */
  float *d_roughness;    /* [R,N]   */
  float *d_weights;      /* [R,N]   */
  float *d_r_rgb, *d_r_diffuse, *d_r_specular; /* [R,3] */
  float *d_r_distance;   /* [R] */
  float *d_r_acc;        /* [R] */
  float *d_r_normals, *d_r_normals_pred, *d_r_tint; /* [R,3] extras */
  float *d_r_roughness;  /* [R] */
  float *d_r_distance_mean; /* [R] */
  double *d_r_percentiles;  /* [R,3] float64: 5 / 50 / 95 (math.py:133-135) */
} refnerf_level_out;

/* Two more optional per-ray outputs of a level (NULL = not stored), in the layout Model.__call__ hands on, so that no copy or
 * reduction kernel runs behind the level.  A struct of its own, taken by the _ex entries below: refnerf_level_out keeps its
 * layout, and callers compiled against it keep working. */
typedef struct refnerf_level_out_extra {
  double *d_r_percentiles_soa; /* [3,R] float64: percentile p of ray r at [p * R + r] INSTEAD of refnerf_level_out.d_r_percentiles
                                  (which is then not written): the three rows are the reference's distance_percentile_5 /
                                  distance_median / distance_percentile_95 (render.py:240-247) without a strided copy each */
  float *d_r_rgb_fg;           /* [R,3] sum_i w_i rgb_i: d_r_rgb before the background term and the render-time sRGB curve --
                                  `final_rgb` of the vis rays (models.py:308-312) */
} refnerf_level_out_extra;

/* Library / device probe.  refnerf_device_ok() returns REFNERF_OK only when
 * the current HIP device is gfx950. */
int refnerf_abi_version(void);
int refnerf_device_ok(void);
const char *refnerf_last_error(void);

/* Bytes of the kernel-side weight image for a precision mode. */
size_t refnerf_packed_weights_bytes(int precision);

/* Re-layout the 46 nn.Parameters of NerfMLP (canonical blob, device) into the
 * MFMA operand image the level kernel streams.  Replaces nothing in the
 * reference (its weights are consumed in place by nn.Linear, models.py:576-
 * 700); must be re-run after every optimiser step. */
int refnerf_pack_weights(const float *d_params, void *d_packed, int precision, void *stream);

/* The same for an MLP whose integrated positional encoding projects onto a general basis (geopoly.generate_basis,
 * internal/geopoly.py:78-123; coord.lift_and_diagonalize, internal/coord.py:129-133; NerfMLP's constructor default is
 * the 21 directions of 'icosahedron' / 2): d_basis [3 * ipe_groups][3] = the basis rows in the reference's order and
 * component order, ipe_groups <= 7.  d_params is then REFNERF_NUM_PARAMS_EXT floats: the canonical blob, whose IPE
 * columns of spatial_net.0 / .5 belong to directions 0..2, followed by W_ext[layer: 0, 5][256 rows][576]: column
 * 96 (g - 1) + 48 c + 3 j + b = (direction group g = 1..6, sin | cos block c, degree j, direction 3 g + b); unused
 * groups zero.  The image is built for REFNERF_PREC_F32 only (levels then run with cfg.precision REFNERF_PREC_F32 or
 * REFNERF_PREC_F16X2 on it: it carries the split-f16 copies); it is
 * refnerf_packed_weights_bytes_basis(precision, ipe_groups) bytes and levels run with cfg.ipe_groups = ipe_groups. */
#define REFNERF_NUM_PARAMS_EXT (REFNERF_NUM_PARAMS + 2 * 6 * 256 * 96)
size_t refnerf_packed_weights_bytes_basis(int precision, int ipe_groups);
int refnerf_pack_weights_basis(const float *d_params, const float *d_basis, int ipe_groups, void *d_packed, int precision, void *stream);

/* One fused launch = one iteration of the level loop of Model.__call__
 * (models.py:162-306): resample (stepfun.py:209-258) -> s_to_t (coord.py:96-98)
 * -> cast_rays (render.py:105-129) -> MLP.__call__ (models.py:533-750) ->
 * compute_alpha_weights (render.py:132-149) -> volumetric_rendering
 * (render.py:152-254).  d_sdist_in [R,n_in+1], d_weights_in [R,n_in].
 * d_sdist_in == NULL && d_weights_in == NULL with cfg->n_in == 1 is the step function every Model.__call__ starts
 * from (models.py:153-157): knots cfg->s_near, cfg->s_far, weight 1 on every ray.  Nothing is read for it and the
 * resampler takes its closed form, sample centre k = s_near + u_k (s_far - s_near): the same bits as the explicit
 * tensors give (the softmax of one logit is 1, the CDF {0, 1}).  Also in refnerf_level_forward_train and the _ex entries.
 * REFNERF_EINVAL: one of the two pointers NULL and the other not, NULL with n_in != 1, NULL with s_far <= s_near. */
int refnerf_level_forward(const void *d_packed, const refnerf_level_cfg *cfg,
                          const refnerf_rays *rays, int32_t R,
                          const float *d_sdist_in, const float *d_weights_in,
                          const refnerf_level_out *out, void *stream);
/* The same launch with the outputs of refnerf_level_out_extra as well (`extra` NULL: exactly refnerf_level_forward). */
int refnerf_level_forward_ex(const void *d_packed, const refnerf_level_cfg *cfg,
                             const refnerf_rays *rays, int32_t R,
                             const float *d_sdist_in, const float *d_weights_in,
                             const refnerf_level_out *out, const refnerf_level_out_extra *extra, void *stream);

/* ---- training (the autograd graph of the same level) ----
 * With cfg->training = 1 (f32 precision mode) refnerf_level_forward also emits
 * the density-gradient normals (models.py:603-609).  refnerf_level_backward is
 * what `loss.backward()` runs for one level in the reference
 * (internal/nerf_system.py training_step -> autograd through models.py:162-306):
 * given the level's saved forward outputs and dL/d(outputs) for the outputs the
 * reference's losses read (train_utils.py:33-204: rendering rgb, history
 * weights, history normals_pred; plus rendering acc / distance, which are
 * linear in the weights; the density-gradient normals, sdist and the
 * resampling inputs are detached there as well), it ACCUMULATES dL/d(params)
 * into d_param_grads (canonical blob, REFNERF_NUM_PARAMS floats).
 * d_workspace holds the per-sample output gradients of every layer, which the
 * weight-gradient GEMM contracts with the saved layer inputs, the split-K
 * partial sums and the per-sample seeds of the per-ray pre-pass. */
typedef struct refnerf_level_saved {
  const float *d_sdist;     /* [R,N+1] refnerf_level_out.d_sdist   */
  const float *d_density;   /* [R,N]                               */
  const float *d_rgb;       /* [R,N,3]                             */
  const float *d_weights;   /* [R,N]                               */
  const void *d_activations; /* the buffer refnerf_level_forward_train filled */
  int32_t activations_format; /* REFNERF_ACT_*: how that forward wrote it (its cfg->precision)              */
} refnerf_level_saved;

typedef struct refnerf_level_grads {
  const float *d_g_r_rgb;         /* [R,3]   dL/d renderings['rgb']                  */
  const float *d_g_weights;       /* [R,N]   dL/d ray_history['weights'], or NULL    */
  const float *d_g_normals_pred;  /* [R,N,3] dL/d ray_history['normals_pred'], or NULL */
  const float *d_g_r_acc;         /* [R]     dL/d renderings['acc'], or NULL             */
  const float *d_g_r_distance;    /* [R]     dL/d renderings['distance'], or NULL        */
  /* ABI v3: optional per-sample seeds on the remaining differentiable entries of ray_history
   * (internal/models.py:731-750), consumed by the regularisers of internal/train_utils.py:207-325.
   * Per-RAY seeds on renderings['diffuse' / 'specular' / 'normals' / 'normals_pred' / 'tint' /
   * 'roughness'] are linear in (weights, history) -- render.py:161-165,227-231 -- and are folded into
   * d_g_weights and these per-sample seeds by the host (refnerf-pl_amd/models.py::_fold_ray_seeds). */
  const float *d_g_density;       /* [R,N]   dL/d ray_history['density'], or NULL           */
  const float *d_g_rgb;           /* [R,N,3] dL/d ray_history['rgb'], or NULL               */
  const float *d_g_diffuse;       /* [R,N,3] dL/d ray_history['diffuse'], or NULL           */
  const float *d_g_specular;      /* [R,N,3] dL/d ray_history['specular'], or NULL          */
  const float *d_g_tint;          /* [R,N,3] dL/d ray_history['tint'], or NULL              */
  const float *d_g_roughness;     /* [R,N]   dL/d ray_history['roughness'], or NULL         */
} refnerf_level_grads;

/* Training forward that also keeps every linear layer's input for the backward
 * (what autograd saves for nn.Linear in the reference): d_activations is a
 * caller-owned buffer of refnerf_activation_workspace_bytes(R, N) bytes
 * (18.1 KB per ray-sample) that must stay untouched until the level's
 * refnerf_level_backward has run.  cfg->training must be 1.  d_packed is the REFNERF_PREC_F32 image;
 * cfg->precision = REFNERF_PREC_BF16 runs the MLP chains (and the density-normal VJP) on bf16 MFMA with the
 * activations rounded to bf16 once per layer (RGB within 1e-4 of the f32 mode); REFNERF_PREC_F32 is the parity mode. */
size_t refnerf_activation_workspace_bytes(int32_t R, int32_t n_samples);
int refnerf_activations_format(const refnerf_level_cfg *cfg);   /* REFNERF_ACT_* of refnerf_level_forward_train(cfg), -1 for NULL */
/* v11: the weight image refnerf_level_forward / _forward_train / _backward expect as `d_packed` for this configuration -- the
 * `precision` argument to pass to refnerf_pack_weights (REFNERF_PREC_* or REFNERF_IMAGE_F16X2_TRAIN; a general IPE basis:
 * REFNERF_PREC_F32 through refnerf_pack_weights_basis), -1 for NULL.  One rule, inside the library (it depends on
 * cfg->training, cfg->precision and cfg->ipe_groups only).
 * The library also remembers, per device pointer, the kind of every image refnerf_pack_weights* wrote: a level entry handed a
 * pointer it packed as ANOTHER kind returns REFNERF_EINVAL instead of streaming garbage (pointers it never packed -- a
 * caller's own copy of an image -- are taken on trust). */
int refnerf_level_image(const refnerf_level_cfg *cfg);
int refnerf_level_forward_train(const void *d_packed, const refnerf_level_cfg *cfg,
                                const refnerf_rays *rays, int32_t R,
                                const float *d_sdist_in, const float *d_weights_in,
                                const refnerf_level_out *out, void *d_activations,
                                size_t activations_bytes, void *stream);
int refnerf_level_forward_train_ex(const void *d_packed, const refnerf_level_cfg *cfg,
                                   const refnerf_rays *rays, int32_t R,
                                   const float *d_sdist_in, const float *d_weights_in,
                                   const refnerf_level_out *out, const refnerf_level_out_extra *extra, void *d_activations,
                                   size_t activations_bytes, void *stream);   /* refnerf_level_forward_train + refnerf_level_out_extra */

/* Scratch of refnerf_level_backward (per-layer output gradients + split-K partials; 17 KB per ray-sample).
 * refnerf_level_backward: d_packed is the REFNERF_PREC_F32 image of refnerf_pack_weights; cfg->precision selects the
 * arithmetic of the transposed GEMM chains (REFNERF_PREC_F32: exact fp32 MFMA, the parity mode; REFNERF_PREC_BF16:
 * bf16 MFMA with deltas rounded to bf16 once per layer, gradients within ~1e-3 relative L2 of the f32 mode),
 * cfg->wgrad_mode that of the weight-gradient GEMM. */
size_t refnerf_backward_workspace_bytes(int32_t R, int32_t n_samples);
/* ... and of both buffers for a level with a general IPE basis (cfg.ipe_groups > 1: the IPE features of the extra direction
 * groups behind the activations, the tail's partial sums behind the workspace; d_param_grads is then
 * REFNERF_NUM_PARAMS_EXT floats, the gradient of the tail columns of groups the basis does not have -- group index >=
 * ipe_groups -- is exactly 0; f32 / split-f16 chains and the bf16x3 weight-gradient GEMM) */
size_t refnerf_backward_workspace_bytes_basis(int32_t R, int32_t n_samples, int32_t ipe_groups);
size_t refnerf_activation_workspace_bytes_basis(int32_t R, int32_t n_samples, int32_t ipe_groups);

int refnerf_level_backward(const void *d_packed, const refnerf_level_cfg *cfg,
                           const refnerf_rays *rays, int32_t R,
                           const refnerf_level_saved *saved, const refnerf_level_grads *grads,
                           float *d_param_grads, void *d_workspace, size_t workspace_bytes,
                           void *stream);

/* MLP.__call__ (internal/models.py:533-750) on caller-supplied Gaussians -- the
 * reference's per-sample entry point: d_means [R,N,3], d_covs [R,N,3,3]
 * (cov_is_full) or [R,N,3] (diagonal), d_viewdirs [R,3] -> the `ray_results`
 * dict as the per-sample fields of the refnerf_level_out struct: density, rgb, normals
 * when cfg->training, normals_pred, grad_pred, tint, diffuse, specular,
 * roughness; the other pointers are ignored.  Same device code as the fused
 * level kernel without the resampling and compositing phases; f32 mode. */
int refnerf_mlp_forward(const void *d_packed, const refnerf_level_cfg *cfg,
                        const float *d_means, const float *d_covs, int32_t cov_is_full,
                        const float *d_viewdirs, int32_t R, int32_t N,
                        const refnerf_level_out *out, void *stream);

/* The step in front of the path, on the device: camera_utils.pixels_to_rays
 * (internal/camera_utils.py:502-614) for perspective cameras (pinhole here;
 * with lens distortion through refnerf_pixels_to_rays_distorted below), with
 * the optional NDC conversion (:31-97, near = 1).
 * d_pix_x / d_pix_y [n] int32; d_pixtocams [3,3] (or [n,3,3] when
 * pixtocam_per_ray); d_camtoworlds [3,4] (or [n,3,4]); d_pixtocam_ndc [3,3] or
 * NULL.  Outputs: origins / directions / viewdirs [n,3], radii [n],
 * imageplane [n,2] (optional).  Saves the 64 B/ray host-to-device copy and the
 * numpy ray casting of whole-image rendering. */
int refnerf_pixels_to_rays(const int32_t *d_pix_x, const int32_t *d_pix_y,
                           const float *d_pixtocams, int32_t pixtocam_per_ray,
                           const float *d_camtoworlds, int32_t camtoworld_per_ray,
                           const float *d_pixtocam_ndc, int32_t n,
                           float *d_origins, float *d_directions, float *d_viewdirs,
                           float *d_radii, float *d_imageplane, void *stream);

/* Radial-tangential lens distortion: the `distortion_params` dict of the
 * reference's cameras, i.e. the keyword parameters of
 * camera_utils._radial_and_tangential_undistort (internal/camera_utils.py:459-470;
 * reference defaults: coefficients 0, eps 1e-9, max_iterations 10). */
#define REFNERF_MAX_UNDISTORT_ITERATIONS 64
typedef struct refnerf_lens_distortion {
  double k1, k2, k3, k4;  /* radial */
  double p1, p2;          /* tangential */
  double eps;             /* a Newton step is taken only where |denominator| > eps */
  int32_t max_iterations; /* Newton steps, 0 .. REFNERF_MAX_UNDISTORT_ITERATIONS */
} refnerf_lens_distortion;

/* refnerf_pixels_to_rays with distortion_params (camera_utils.py:558-565): the
 * three camera-space points of each ray (pixel, +x and +y neighbour) are
 * undistorted by max_iterations Newton steps in double precision (:409-493),
 * rounded to float and restacked as (x, y, 1) before the OpenCV -> OpenGL flip;
 * imageplane, viewdirs, radii and the NDC conversion then see the undistorted
 * directions.  With all coefficients 0 (or max_iterations 0) and a pixtocam
 * whose third row is (0, 0, 1) the output is bit-identical to
 * refnerf_pixels_to_rays.  REFNERF_EINVAL for a NULL `distortion`, a
 * non-finite coefficient or eps, or max_iterations outside [0, 64]. */
int refnerf_pixels_to_rays_distorted(const int32_t *d_pix_x, const int32_t *d_pix_y,
                                     const float *d_pixtocams, int32_t pixtocam_per_ray,
                                     const float *d_camtoworlds, int32_t camtoworld_per_ray,
                                     const float *d_pixtocam_ndc, int32_t n,
                                     float *d_origins, float *d_directions, float *d_viewdirs,
                                     float *d_radii, float *d_imageplane,
                                     const refnerf_lens_distortion *distortion, void *stream);

/* A whole frame's rays from (width, height, camera, pose) in one launch:
 * Dataset.generate_ray_batch (internal/datasets.py:487-498) for the flat,
 * row-major pixel range [first, first + count) of a width x height image, so a
 * rank of a sharded render produces only its own rays.  No pixel-index input;
 * all nine utils.Rays fields out (64 B/ray). */
#define REFNERF_PROJ_PINHOLE 0
#define REFNERF_PROJ_SPHERICAL 1
typedef struct refnerf_image_rays_out {
  float *d_origins, *d_directions, *d_viewdirs; /* [count,3] */
  float *d_radii;                               /* [count] */
  float *d_imageplane;                          /* [count,2]; may be NULL, as may every pointer below */
  float *d_lossmult, *d_near, *d_far;           /* [count]: 1, near, far */
  int32_t *d_cam_idx;                           /* [count]: frame (pinhole), 0 (spherical) */
} refnerf_image_rays_out;

/* The pose is d_camtoworlds + 12 * frame of the [n_frames,3,4] path.
 * REFNERF_PROJ_PINHOLE: the arithmetic of refnerf_pixels_to_rays (or, with
 * `distortion`, of refnerf_pixels_to_rays_distorted) on pixel (x, y) =
 * (index % width, index / width): origins, directions, viewdirs, radii and
 * imageplane are bit-identical to those entries' on the same pixels.
 * REFNERF_PROJ_SPHERICAL: camera_utils.cast_spherical_rays (:700-746), an
 * equirectangular panorama; d_pixtocam is unused (may be NULL), viewdirs =
 * directions, imageplane = 0; directions and radii are computed in double from
 * the float32 pose and rounded at the store.
 * REFNERF_EINVAL: an unknown projection, a NULL required pointer, a
 * non-positive size, frame outside [0, n_frames), a range outside the image,
 * NDC or distortion with the spherical projection, or a `distortion` that
 * refnerf_pixels_to_rays_distorted refuses. */
int refnerf_image_rays(int32_t projection, int32_t width, int32_t height,
                       const float *d_pixtocam, const float *d_camtoworlds,
                       int32_t n_frames, int32_t frame, const float *d_pixtocam_ndc,
                       const refnerf_lens_distortion *distortion, float near, float far,
                       int64_t first, int32_t count, const refnerf_image_rays_out *out,
                       void *stream);

/* Scene loaders (internal/datasets.py:519-708), the device stages.
 *
 * refnerf_prepare_images: a stack of decoded images d_src [n,H,W,C] (uint8, or
 * float32 with src_is_f32) to the float32 arrays `_load_renderings` keeps:
 * area downsample by `factor` (image.downsample: the mean of each factor x
 * factor block, float32(sum) / float32(factor^2)), then
 *   REFNERF_PREP_SCALE    mean / 255                      -> d_out [n,h,w,C]   (LLFF rgb, :636-637)
 *   REFNERF_PREP_WHITE    C = 4: v = mean / 255, v_rgb * v_a + (1 - v_a)
 *                                                         -> d_out [n,h,w,3], d_alpha [n,h,w] = v_a when not NULL
 *                                                                              (Blender, :550, :567-570)
 *   REFNERF_PREP_NORMALS  C >= 3: mean_rgb * 2 / 255 - 1  -> d_out [n,h,w,3]   (:557)
 *   REFNERF_PREP_RAW      mean                            -> d_out [n,h,w,C]   (disparity TIFFs, :554)
 * with h = H / factor, w = W / factor.  Every operation is rounded to float32
 * on its own, in the reference's order, so uint8 sources reproduce its numpy
 * arrays bit for bit: their block sums are exact integers, which is why
 * factor^2 * 255 must stay below 2^24 (factor <= 256).  float32 sources are
 * summed in double and rounded once.  All offsets are 64-bit.
 * REFNERF_EINVAL: a NULL d_src / d_out, a non-positive size, C outside
 * {1, 3, 4}, a factor outside [1, 256] or one that does not divide H and W, an
 * unknown op, WHITE without C = 4, NORMALS with C = 1, d_alpha without WHITE,
 * a float32 pointer that is not 4-byte aligned, or more than 2^39 outputs. */
#define REFNERF_PREP_SCALE 0
#define REFNERF_PREP_WHITE 1
#define REFNERF_PREP_NORMALS 2
#define REFNERF_PREP_RAW 3
int refnerf_prepare_images(const void *d_src, int32_t src_is_f32, int64_t n, int32_t H, int32_t W,
                           int32_t C, int32_t factor, int32_t op, float *d_out, float *d_alpha,
                           void *stream);

/* refnerf_train_batch: one training batch of `Dataset._next_train` /
 * `_make_ray_batch` (:395-485) in one launch.  Patch p has its origin at pixel
 * (d_px0[p], d_py0[p]) of camera d_cam[p] (cam_per_patch) or d_cam[0]
 * ('single_image' batching); its patch_size^2 rays are the pixels (x0 + dx,
 * y0 + dy), dy major.  Outputs are [n_patches, patch_size, patch_size, .]:
 * the nine Rays fields (all required; origins, directions, viewdirs, radii and
 * imageplane bit-identical to refnerf_pixels_to_rays[_distorted] on the same
 * pixels and cameras; lossmult 1, near, far, cam_idx as given), d_rgb =
 * d_images[cam, y, x], and d_out_disps / d_out_normals / d_out_alphas likewise
 * from their stacks when both the stack and the output are given.  The camera
 * is read inside the kernel: d_pixtocams is [3,3] or, with
 * pixtocam_per_camera, [n_images,3,3]; d_camtoworlds [n_images,3,4].  Image
 * and camera loads clamp their indices into the stacks.
 * REFNERF_EINVAL: a NULL required pointer, a non-positive size, patch_size
 * larger than the image, n_patches * patch_size^2 >= 2^31, an optional output
 * without its stack (or the reverse), or a `distortion` that
 * refnerf_pixels_to_rays_distorted refuses. */
typedef struct refnerf_train_batch_args {
  const void *d_px0, *d_py0, *d_cam;           /* int32, or int64 with index_is_int64 (the dtype torch.randint draws) */
  int32_t index_is_int64, cam_per_patch, n_patches, patch_size;
  int32_t n_images, height, width;
  const float *d_images;                       /* [n_images,H,W,3] */
  const float *d_disps, *d_normals, *d_alphas; /* [n_images,H,W], [n_images,H,W,3], [n_images,H,W]; each may be NULL */
  const float *d_pixtocams, *d_camtoworlds, *d_pixtocam_ndc; /* d_pixtocam_ndc may be NULL */
  int32_t pixtocam_per_camera;
  float near, far;
  const refnerf_lens_distortion *distortion;   /* NULL: pinhole */
  refnerf_image_rays_out rays;
  float *d_rgb;                                /* [.,3] */
  float *d_out_disps, *d_out_normals, *d_out_alphas;
} refnerf_train_batch_args;
int refnerf_train_batch(const refnerf_train_batch_args *args, void *stream);

/* Stage entry points (same device code as the fused kernel; used by the
 * parity tests and for drop-in use of the individual reference functions). */

/* stepfun.sample_intervals (stepfun.py:209-258) with deterministic centres.
 * d_t [R,M+1], d_logits [R,M] -> d_sdist [R,N+1], d_bin_idx [R,N] (optional). */
int refnerf_sample_intervals(const float *d_t, const float *d_logits, int32_t R, int32_t M,
                             int32_t N, float s_min, float s_max, float *d_sdist,
                             int32_t *d_bin_idx, void *stream);

/* coord.integrated_pos_enc(min_deg=0,max_deg=16) on lifted Gaussians
 * (coord.py:107-126): d_lmean/d_lvar [n,3] -> d_feat [n,96]. */
int refnerf_integrated_pos_enc(const float *d_lmean, const float *d_lvar, int32_t n,
                               float *d_feat, void *stream);

/* ref_utils.generate_ide_fn(5) (ref_utils.py:98-161): d_xyz [n,3],
 * d_kappa_inv [n] -> d_ide [n,72]. */
int refnerf_integrated_dir_enc(const float *d_xyz, const float *d_kappa_inv, int32_t n,
                               float *d_ide, void *stream);

/* render.compute_alpha_weights (render.py:132-149) + render.volumetric_rendering (render.py:152-254, all five
 * render-time `srgb_mapping` modes :186-216, float64 percentiles via stepfun.py:294-307 / math.py:114-142) on
 * caller-supplied per-sample values -- the compositing phase of the fused level kernel behind its own entry.
 * d_density / d_roughness [R,N]; d_tdist [R,N+1]; d_directions [R,3]; d_far [R]; the [R,N,3] inputs may be NULL
 * (zero).  Reads cfg->n_samples (<= 1024), opaque_background, render_srgb_mode, compute_extras, bg_rgb; writes
 * out->d_weights and the d_r_* fields (d_r_normals only when d_normals is given). */
int refnerf_render_rays(const refnerf_level_cfg *cfg, int32_t R, const float *d_density, const float *d_tdist,
                        const float *d_directions, const float *d_far, const float *d_rgb, const float *d_diffuse,
                        const float *d_specular, const float *d_normals, const float *d_normals_pred,
                        const float *d_roughness, const float *d_tint, const refnerf_level_out *out, void *stream);

/* The three Ref-NeRF losses of one level, fused (internal/train_utils.py:33-88 compute_data_loss with
 * data_loss_type 'mse', :165-183 orientation_loss, :186-204 predicted_normal_loss): ONE pass over the level's outputs
 * instead of ~25 elementwise ATen ops and their autograd graph.
 * refnerf_losses_forward writes per-ray terms d_terms [R,3] = { sum_c lossmult (rgb_c - gt_c)^2,
 * sum_i w_i min(0, n_i . (-viewdir))^2, sum_i w_i (1 - n_i . n_pred,i) }; the caller sums them over the rays and applies
 * the normalisers (sum of the broadcast lossmult; ray count) and Config's coarse / fine multipliers.
 * d_orientation_normals = ray_history[Config.orientation_loss_target] (NULL: term off); d_normals = the density normals
 * (NULL: predicted-normal term off).  refnerf_losses_backward produces what autograd would hand to the level's
 * backward: dL/d renderings['rgb'] [R,3], dL/d ray_history['weights'] [R,N], dL/d ray_history['normals_pred'] [R,N,3],
 * given g_* = d(term)/d(term sum) (multiplier / normaliser included) times d_upstream[0..2] = dL/d(data, orientation,
 * predicted-normal term) (device float[3], NULL = 1: on the device so that autograd's grad_output needs no host sync); the density normals are detached as in the reference
 * (models.py:609), so an orientation target other than normals_pred only reaches the weights. */
int refnerf_losses_forward(int32_t R, int32_t N, const float *d_r_rgb, const float *d_gt_rgb, const float *d_lossmult,
                           const float *d_weights, const float *d_orientation_normals, const float *d_normals,
                           const float *d_normals_pred, const float *d_viewdirs, float *d_terms, void *stream);
int refnerf_losses_backward(int32_t R, int32_t N, const float *d_r_rgb, const float *d_gt_rgb, const float *d_lossmult,
                            const float *d_weights, const float *d_orientation_normals, int32_t orientation_on_pred,
                            const float *d_normals, const float *d_normals_pred, const float *d_viewdirs,
                            float g_data, float g_orientation, float g_normal, const float *d_upstream,
                            float *d_g_r_rgb, float *d_g_weights, float *d_g_normals_pred, void *stream);

/* The six geometry regularisers of one level, fused (internal/train_utils.py:207-279 noisy_consistency_loss, :282-310
 * noisy_distance_consistency_loss, :313-316 accumulated_weights_loss, :318-329 weights_entropy_loss): one pass each way
 * instead of a chain of small ATen ops per term whose masked means (x[mask].mean()) are boolean indexings, i.e. a
 * nonzero and a host synchronisation each.  R rays of S samples; the first n rays have `a` perturbed copies each, the
 * copy (r, j) being noisy ray r * a + j (the reference reshapes its angle-major noisy batch with reshape(n, a): that
 * pairing is part of the contract).
 * refnerf_ray_regularisers_forward writes per-ray rows d_terms [R,8]:
 *   0  sum_i -w_i log(w_i + 1e-10) where acc > thr_entropy, else 0          1  that mask as 1.0 / 0
 *   2  (1 - acc)^2
 *   3..6  diffuse, specular, normal and distance consistency of ray r with its copies where r < n and
 *         acc > thr_consistency, else 0                                      7  that mask as 1.0 / 0
 * The caller sums the rows over the rays and forms sum / count * multiplier on the device (an empty mask gives
 * 0 / 0 = NaN, as mean() of an empty selection does).  Colour measures (REFNERF_CONSISTENCY_*): MSE
 * sum_c mean_j (x_c - y_jc)^2; AVG_MSE sum_c (x_c - mean_j y_jc)^2; VAR mean_c of the unbiased variance of the a + 1
 * values.  The specular term's sign flip is the caller's.  Normal: mean_j (1 - n . n_j) on the rendered normals of the
 * caller's target.  Distance (MSE only): sum_c mean_j ((o + d dist) - (o_j + d_j dist_j))_c^2.
 * refnerf_ray_regularisers_backward writes dL/d weights [R,S], dL/d acc [R] and, per consistency term, the gradient rows
 * of the clean side ([R, .]; zero past n) and of the noisy side ([n a, .]), given d_sums = the column sums of d_terms
 * (float[8]: the counts) and d_scales = float[6] { entropy, acc, diffuse, specular, normal, distance }: multiplier x
 * warm-up x upstream gradient of each term -- both on the device, so nothing is read back.  Masks carry no gradient;
 * rays outside a mask get exact zeros.
 * A term is ON when its pointers are given and costs nothing when they are NULL: entropy d_weights (and d_g_weights),
 * diffuse / specular / normal the clean and the noisy tensor, distance those two and the four ray tensors.  Mandatory:
 * d_acc and d_terms (forward) / d_sums and d_scales (backward).  REFNERF_EINVAL: a null mandatory pointer or a term given
 * in part, R <= 0, S <= 0, n < 0, n > R, n > 0 with a <= 0, an unknown type. */
enum { REFNERF_CONSISTENCY_MSE = 0, REFNERF_CONSISTENCY_AVG_MSE = 1, REFNERF_CONSISTENCY_VAR = 2 };
typedef struct refnerf_regularisers_args {
  int32_t R, S, n, a;
  float thr_entropy, thr_consistency;          /* Config.acc_threshold_for_weights_entropy_loss / _for_consistency_loss */
  int32_t diffuse_type, specular_type, distance_type;   /* REFNERF_CONSISTENCY_*; distance: MSE only */
  const float *d_weights;                      /* [R,S] ray_history['weights'] */
  const float *d_acc;                          /* [R]   renderings['acc'] */
  const float *d_distance, *d_diffuse, *d_specular, *d_normals;           /* clean renderings: [R], [R,3] x 3 */
  const float *d_n_distance, *d_n_diffuse, *d_n_specular, *d_n_normals;   /* noisy renderings: [n a], [n a,3] x 3 */
  const float *d_origins, *d_directions;       /* [R,3] clean rays (distance term) */
  const float *d_n_origins, *d_n_directions;   /* [n a,3] noisy rays */
  float *d_terms;                              /* forward: [R,8] */
  const float *d_sums, *d_scales;              /* backward: float[8], float[6] */
  float *d_g_weights, *d_g_acc;                /* backward: [R,S], [R] */
  float *d_g_distance, *d_g_diffuse, *d_g_specular, *d_g_normals;         /* [R], [R,3] x 3 */
  float *d_g_n_distance, *d_g_n_diffuse, *d_g_n_specular, *d_g_n_normals; /* [n a], [n a,3] x 3 */
} refnerf_regularisers_args;
int refnerf_ray_regularisers_forward(const refnerf_regularisers_args *args, void *stream);
int refnerf_ray_regularisers_backward(const refnerf_regularisers_args *args, void *stream);

/* The perturbed rays of the consistency terms (internal/sample_utils.py:40-79 sample_noisy_rays) in one launch instead of
 * a Python loop over the rotations: output ray k = j n + i (angle-major) is ray i seen from rotation j,
 * directions' = T_j d_i, viewdirs' = T_j v_i, origins' = o_i + dist_i d_i - dist_i directions'; the other six fields are
 * copied from ray i.  d_rotations [a,3,3] row-major (the caller draws the Euler angles); d_distance [n]; inputs [n, .]
 * (the first n rays of the batch), outputs [a n, .] with the widths of the Rays fields: origins / directions / viewdirs
 * 3, imageplane 2, the others 1.  REFNERF_EINVAL: a null pointer, n <= 0 or a <= 0. */
typedef struct refnerf_noisy_rays_args {
  int32_t n, a;
  const float *d_rotations, *d_distance;
  const float *d_origins, *d_directions, *d_viewdirs, *d_radii, *d_imageplane, *d_lossmult, *d_near, *d_far, *d_cam_idx;
  float *d_out_origins, *d_out_directions, *d_out_viewdirs, *d_out_radii, *d_out_imageplane, *d_out_lossmult, *d_out_near,
        *d_out_far, *d_out_cam_idx;
} refnerf_noisy_rays_args;
int refnerf_noisy_rays(const refnerf_noisy_rays_args *args, void *stream);

/* The data term of one level with either penalty, and its two statistics (internal/train_utils.py:33-88
 * compute_data_loss; refnerf_losses_forward covers 'mse' without statistics only).  R flat rays.
 * refnerf_data_terms_forward writes per-ray rows d_terms [R,5]:
 *   0  sum_c lossmult (rgb_c - gt_c)^2                                  (the numerator of stats['mses'])
 *   1  sum_c lossmult p_c, p = r^2 (REFNERF_PENALTY_MSE) or sqrt(r^2 + charb_padding^2) (REFNERF_PENALTY_CHARB; r^2 is
 *      formed first and the squared padding added after, as the reference does)
 *   2  (1 / (1 + distance_mean) - disps)^2                              (stats['disparity_mses'], :62-67)
 *   3  w acos(clip(n_hat . ngt_hat, -(1 - 2^-23), 1 - 2^-23))           4  w = acc alphas       (stats['normal_maes'], :69-84)
 * with x_hat = x / sqrt(max(sum x^2, 2^-23)) (ref_utils.py:40-50).  The caller sums the rows over the rays (one column
 * sum: no float atomics, two runs give the same bits) and forms the normalisers on the device: 3 sum(lossmult) for columns
 * 0 and 1, R for column 2, column 3 / column 4 times 180 / pi.  d_gt_rgb is the target the loss compares with (already
 * linearised under Config.supervised_by_linear_rgb).  Optional groups: { d_distance_mean, d_disps } and { d_acc, d_alphas,
 * d_normals, d_normals_gt }; an absent group leaves its columns 0.
 * refnerf_data_terms_backward writes d_g_rgb [R,3] = d_upstream[0] lossmult (2 r | r / sqrt(r^2 + charb_padding^2));
 * d_upstream is a DEVICE float (multiplier / normaliser x autograd's grad_output: no host synchronisation).  The statistics
 * carry no gradient (the reference rebuilds them with torch.tensor).
 * REFNERF_EINVAL: a null args / d_rgb / d_gt_rgb / d_lossmult / d_terms (forward) / d_upstream, d_g_rgb (backward), R <= 0,
 * an unknown penalty, a negative or non-finite charb_padding, an optional group given in part. */
enum { REFNERF_PENALTY_MSE = 0, REFNERF_PENALTY_CHARB = 1 };
typedef struct refnerf_data_terms_args {
  int32_t R, penalty;                          /* REFNERF_PENALTY_* */
  float charb_padding;                         /* Config.charb_padding */
  const float *d_rgb, *d_gt_rgb, *d_lossmult;  /* [R,3] renderings['rgb'], [R,3] target, [R] rays.lossmult */
  const float *d_distance_mean, *d_disps;      /* [R] renderings['distance_mean'], [R] batch.disps */
  const float *d_acc, *d_alphas, *d_normals, *d_normals_gt;   /* [R], [R], [R,3] renderings['normals'], [R,3] batch.normals */
  float *d_terms;                              /* forward: [R,5] */
  const float *d_upstream;                     /* backward: float[1] */
  float *d_g_rgb;                              /* backward: [R,3] */
} refnerf_data_terms_args;
int refnerf_data_terms_forward(const refnerf_data_terms_args *args, void *stream);
int refnerf_data_terms_backward(const refnerf_data_terms_args *args, void *stream);

/* The edge-aware depth smoothness of one level of a patch batch (internal/train_utils.py:90-119
 * compute_depth_smoothness_loss): P patches of S x S rays, d_distance [P,S,S], d_acc [P,S,S], d_rgb [P,S,S,3].
 * refnerf_depth_smoothness_forward writes per-patch rows d_terms [P,2] =
 *   { sum |acc00 w01 (v00 - v01)^2|, sum |acc00 w10 (v00 - v10)^2| } over the (S-1)^2 cells of the patch, 00 the cell's
 * pixel, 01 its right and 10 its lower neighbour, w = exp(-mean_c |rgb00 - rgb_neighbour|).  The caller forms
 * (column 0 + column 1) / (2 P (S-1)^2) and applies Config's coarse / fine multiplier on the device.
 * refnerf_depth_smoothness_backward writes d_g_distance [P,S,S] in gather form (one thread per pixel, no atomics): the
 * pixel's contribution as v00 of its own cell, as v01 of the cell to its left and as v10 of the cell above, times
 * d_upstream[0] (a DEVICE float); the sign of the product is kept, as abs() does.  acc and rgb get no gradient (the
 * reference reads them under no_grad).
 * REFNERF_EINVAL: a null pointer, P <= 0, S < 2, P S S >= 2^31. */
typedef struct refnerf_depth_smoothness_args {
  int32_t P, S;
  const float *d_distance, *d_acc, *d_rgb;
  float *d_terms;                              /* forward: [P,2] */
  const float *d_upstream;                     /* backward: float[1] */
  float *d_g_distance;                         /* backward: [P,S,S] */
} refnerf_depth_smoothness_args;
int refnerf_depth_smoothness_forward(const refnerf_depth_smoothness_args *args, void *stream);
int refnerf_depth_smoothness_backward(const refnerf_depth_smoothness_args *args, void *stream);

/* The two host-side stages of the proposal-network configuration (num_levels = 3, a separate PropMLP, dilation and
 * interlevel loss on), one wave per ray, no host synchronisation, no allocation, every sum in one fixed order.
 *
 * refnerf_max_dilate_weights: stepfun.max_dilate_weights(t, w, dilation, domain = (lo, hi), renormalize = True) followed by
 * [..., 1:-1] on both results (internal/models.py:167-187, internal/stepfun.py:92-131): what Model.__call__ puts in front
 * of every level after the first.  p_i = w_i / max(eps^2, t_{i+1} - t_i), eps = FLT_EPSILON; knots x = the sorted union
 * of t (M + 1 values), t[:-1] - dilation and t[1:] + dilation, clamped to [lo, hi] after sorting (bit-equal to torch.sort
 * of the fp32 values); p'_j = max({ p_i : t_i - dilation <= x_j < t_{i+1} + dilation } U { 0 }) with the CLAMPED knot;
 * w'_j = p'_j (x_{j+1} - x_j) / max(eps^2, sum_j w'_j), the sum over all 3 M intervals.  Written: knots 1 .. 3M - 1 and
 * intervals 1 .. 3M - 2.  t must be nondecreasing along a ray; otherwise the values are meaningless (no access leaves
 * the rows).  REFNERF_EINVAL: R < 0, M < 1, M > 171 (3 M - 2 > 512, the resampler's limit), a null pointer.  R == 0
 * succeeds and launches nothing.
 *
 * refnerf_interlevel_forward / _backward: stepfun.lossfun_outer(t, w, t_env, w_env) of ONE proposal level (t_env, w_env:
 * Np intervals) against the detached final level (t, w: N intervals) (internal/train_utils.py:151-162,
 * internal/stepfun.py:31-89).  cy = [0, cumsum(w_env)] (accumulated in double); idx_lo(v) = the last k with
 * t_env[k] <= v, or 0; idx_hi(v) = the first k with t_env[k] > v, or Np; w_outer_i = cy[idx_hi(t_{i+1})] - cy[idx_lo(t_i)];
 * l_i = max(0, w_i - w_outer_i)^2 / (w_i + FLT_EPSILON).  Forward: d_ray_loss[r] = sum_i l_i; the caller sums the rays,
 * divides by R N and applies Config.interlevel_loss_mult on the device.  Backward: d_upstream is a DEVICE scalar,
 * d total / d (sum of d_ray_loss); d_g_w_env[r][k] = upstream * sum over the i with idx_lo(t_i) <= k < idx_hi(t_{i+1}) of
 * -2 max(0, w_i - w_outer_i) / (w_i + FLT_EPSILON), an exact zero where no penalised interval covers k.  t, w and t_env
 * get no gradient (the reference detaches the first two; the knots are not differentiable here).  Two calls on the same
 * inputs are bit-identical.  REFNERF_EINVAL: R < 0, N or Np outside [1, 512], a null pointer.  R == 0 succeeds and
 * launches nothing. */
int refnerf_max_dilate_weights(const float *d_t /* [R][M+1] */, const float *d_w /* [R][M] */, int32_t R, int32_t M,
                               float dilation, float domain_lo, float domain_hi, float *d_t_out /* [R][3M-1] */,
                               float *d_w_out /* [R][3M-2] */, void *stream);
int refnerf_interlevel_forward(const float *d_t /* [R][N+1] */, const float *d_w /* [R][N] */,
                               const float *d_t_env /* [R][Np+1] */, const float *d_w_env /* [R][Np] */, int32_t R, int32_t N,
                               int32_t Np, float *d_ray_loss /* [R] */, void *stream);
int refnerf_interlevel_backward(const float *d_t, const float *d_w, const float *d_t_env, const float *d_w_env, int32_t R,
                                int32_t N, int32_t Np, const float *d_upstream /* device scalar */,
                                float *d_g_w_env /* [R][Np] */, void *stream);

/* The optimiser step of the reference's loop, fused (nerf_system.py:205-217 configure_gradient_clipping +
 * on_after_backward, torch.optim.Adam.step): clip_grad_value_(grad_max_val), clip_grad_norm_(grad_max_norm) over ALL
 * tensors of the step, Adam (no AMSGrad, no weight decay), and the per-segment statistics grad_norm = |g|_2 and
 * grad_max = max|g| of the raw gradient and weight_l2 = |w|_2^2.  fp32 tensors of n < 2^31 elements.
 *
 * A tensor is cut into segments by a HOST table seg_off[n_seg + 1] (elements; seg_off[0] = 0 < ... < seg_off[n_seg] = n:
 * the segments tile [0, n), need no alignment and may be one element long) -- the layers of a flat parameter blob, or one
 * segment for a plain tensor.  Per tensor the caller owns
 *   d_workspace  refnerf_optim_workspace_bytes(n, n_seg) bytes, 16-byte aligned; refnerf_optim_plan fills it ONCE with the
 *                work items (segment, start, length <= 4096) the statistics kernel runs over (a setup call: it
 *                synchronises the stream) and returns their number;
 *   d_seg_stats  float [n_seg][3] = { grad_norm, grad_max, weight_l2 }, written by refnerf_optim_finalize;
 * and per optimiser one d_state of refnerf_optim_state_bytes(max_tensors) bytes, 16-byte aligned: float total_norm,
 * float clip_coef, double total_norm^2, then the library's table of the step's tensors.
 * One step = refnerf_optim_stats per tensor (slot = 0 .. k-1: which tensor of THIS step; tensors without a gradient are
 * simply left out) -> refnerf_optim_finalize(k) -> refnerf_optim_adam_step per tensor: 2k + 1 launches on one stream, no
 * host synchronisation, no allocation, no float atomics -- every sum has one fixed order, so a step is bit-reproducible.
 * total_norm is the norm of the value-clipped gradients (what clip_grad_norm_ returns); clip_coef =
 * min(1, grad_max_norm / (total_norm + 1e-6)), or 1 when grad_max_norm <= 0; a non-finite norm reaches the parameters as
 * it does in torch.  REFNERF_EINVAL: a null pointer, n <= 0, a table that does not tile [0, n), a workspace or state
 * too small or misaligned, a slot outside the state. */
typedef struct refnerf_adam_cfg {
  double lr, beta1, beta2, eps;
  double bias_correction1;        /* 1 - beta1^t, t = 1 for the first step */
  double sqrt_bias_correction2;   /* sqrt(1 - beta2^t) */
  double grad_max_val;            /* <= 0: no value clipping */
  int32_t write_grad;             /* also store the clipped gradient back into d_grad */
  int32_t no_step;                /* clip only (needs write_grad): d_param / d_exp_avg / d_exp_avg_sq may be NULL */
} refnerf_adam_cfg;
size_t refnerf_optim_workspace_bytes(int64_t n_elements, int32_t n_segments);   /* 0 for bad arguments */
size_t refnerf_optim_state_bytes(int32_t max_tensors);
int refnerf_optim_plan(int64_t n, const int32_t *seg_off, int32_t n_seg, void *d_workspace, size_t workspace_bytes,
                       int32_t *n_items, void *stream);
int refnerf_optim_stats(const float *d_grad, const float *d_param, int64_t n, int32_t n_seg, int32_t n_items,
                        double grad_max_val, void *d_workspace, size_t workspace_bytes, float *d_seg_stats,
                        void *d_state, size_t state_bytes, int32_t slot, void *stream);
int refnerf_optim_finalize(void *d_state, size_t state_bytes, int32_t n_tensors, double grad_max_norm, void *stream);
int refnerf_optim_adam_step(float *d_param, float *d_grad, float *d_exp_avg, float *d_exp_avg_sq, int64_t n,
                            const refnerf_adam_cfg *cfg, const void *d_state, void *stream);

/* Test-image evaluation, the metric half of the reference's test_step (nerf_system.py:391-444), on the device.
 * Images are double [H][W][C] with a row pitch in ELEMENTS (>= W * C; a border crop is a pointer offset), 8-byte aligned;
 * all arithmetic is float64, as in the reference, which casts to float64 before it evaluates.  Every sum over pixels is a
 * two-stage reduction in one fixed order (per-workgroup partials in d_workspace, then one workgroup adds them in index
 * order): no float atomics, two runs are bit-identical, and a pitched view gives the bits of its contiguous copy.  No
 * entry synchronises the host or allocates; results are written to device memory at d_out.  d_workspace holds at least
 * refnerf_image_workspace_bytes(H, W, C) bytes (0 for bad sizes; enough for every entry at that shape, for
 * refnerf_weighted_mae with n = H * W) and must not be shared by calls on different streams.
 *
 *   refnerf_image_mse      d_out[0] = mean over H W C of (q(a) - b)^2, d_out[1] = its PSNR, mse_to_psnr as the reference
 *                          evaluates it: float32(-10 / float32(ln 10)) * ln(mse).  q(x) = rint(x * 255) / 255 (half to
 *                          even, torch.round) when quantize_a is set, else x.  C = 1 gives the disparity MSE.
 *   refnerf_image_ssim     d_out[0] = dm_pix.ssim(a, b) with its defaults (max_val 1, 11 taps, sigma 1.5, k1 0.01, k2 0.03):
 *                          taps g[i] = exp(-0.5 ((i - 5) / 1.5)^2) normalised to sum 1 (host, double); F = 'valid'
 *                          separable correlation along H then W per channel; mu = F(.), s_aa = max(e, F(a^2) - mu_a^2),
 *                          s_bb alike, e = (2^-23)^2, s = F(ab) - mu_a mu_b, s_ab = sign(s) min(sqrt(s_aa s_bb), |s|);
 *                          map = (2 mu_a mu_b + c1)(2 s_ab + c2) / ((mu_a^2 + mu_b^2 + c1)(s_aa + s_bb + c2)), c1 = 1e-4,
 *                          c2 = 9e-4; the mean over the [H-10][W-10][C] map.  d_map (optional, dense) receives the map.
 *                          quantize_a as above.  H < 11 or W < 11: REFNERF_EINVAL (the reference's map would be empty).
 *   refnerf_color_correct  image.color_correct(img, ref, num_iters, eps) (internal/image.py:84-127), C = 3: per iteration the
 *                          masked normal equations of the ten-term quadratic expansion, one 10 x 10 pseudo-inverse solve
 *                          per channel (eigenvalues <= 10 * 2^-52 * lambda_max dropped; an all-masked channel gives a
 *                          zero warp, as lstsq does), x <- clip(a W, 0, 1).  d_out: the corrected image, dense [H][W][3],
 *                          must not overlap d_img; d_warp (optional): the last [10][3] warp.  num_iters = 0 copies the
 *                          input.  3 launches per iteration.  Agrees with the reference's lstsq to 1e-13 where the masked
 *                          systems are well conditioned; near-rank-deficient images (a constant colour) are outside
 *                          that: the rank decision on A^T A is not lstsq's on A.
 *   refnerf_weighted_mae   ref_utils.compute_weighted_mae: d_out[0] = sum w acos(clip(n . n_gt, +-(1 - 2^-23))) / sum w
 *                          * 180 / pi; d_weights [n], d_normals and d_normals_gt [n][3], dense.
 * REFNERF_EINVAL: a null pointer (d_map / d_warp may be null), C outside 1..4 (colour correction: C != 3), a pitch below
 * W * C, num_iters outside 0..64, a non-finite eps, a misaligned pointer, a workspace too small, H W C >= 2^31. */
size_t refnerf_image_workspace_bytes(int32_t H, int32_t W, int32_t C);
int refnerf_image_mse(const double *d_a, int64_t pitch_a, const double *d_b, int64_t pitch_b, int32_t H, int32_t W, int32_t C,
                      int32_t quantize_a, double *d_out /* [2] */, void *d_workspace, size_t workspace_bytes, void *stream);
int refnerf_image_ssim(const double *d_a, int64_t pitch_a, const double *d_b, int64_t pitch_b, int32_t H, int32_t W, int32_t C,
                       int32_t quantize_a, double *d_out /* [1] */, double *d_map /* [H-10][W-10][C] or NULL */,
                       void *d_workspace, size_t workspace_bytes, void *stream);
int refnerf_color_correct(const double *d_img, int64_t pitch_img, const double *d_ref, int64_t pitch_ref, int32_t H, int32_t W,
                          int32_t C, int32_t num_iters, double eps, double *d_out /* [H][W][3] */,
                          double *d_warp /* [10][3] or NULL */, void *d_workspace, size_t workspace_bytes, void *stream);
int refnerf_weighted_mae(const double *d_weights, const double *d_normals, const double *d_normals_gt, int64_t n,
                         double *d_out /* [1] */, void *d_workspace, size_t workspace_bytes, void *stream);

/* Validation visualisations, the reference's internal/vis.py (visualize_suite, nerf_system.py:307), on the device.
 * Image and ray inputs are dense float32 or float64 (one `f64` flag per call: 0 = float, 1 = double); ALL arithmetic is
 * float64, and a float32 output is rounded once, when it is written.  No entry synchronises the host, allocates or uses a
 * float atomic: two runs are bit-identical.  eps = 2^-23 (finfo(float32).eps) throughout.
 *
 *   refnerf_vis_weighted_percentile   vis.weighted_percentile (vis.py:26-36, math.py:114-142).  d_order is a STABLE ascending
 *       order of the n values (NaNs last; the caller sorts, ties in index order); the weight of the value at flat index j is
 *       d_weights[j % n_weights], exactly as the reference indexes a [H][W] weight map by a [H][W][3] value map (NULL: all
 *       ones), and 0 where d_nan_mask[j % n_weights] is NaN (optional: visualize_suite's `acc` at NaN distances).  Launches:
 *       per-workgroup sums of the gathered weights (2048 per workgroup) -> their exclusive scan in index order by one lane
 *       -> the inclusive scan acc[] -> #{acc[i] <= target_p} (integer counts) -> per percentile the reference's interp:
 *       target = ps[p] * acc[n-1] / 100 (evaluated in float32 when target_f32 is set: the reference's torch.tensor(ps) is a
 *       float32 tensor and wins the promotion against the 0-dim total), idx = clamp(count - 1, 0, n - 2),
 *       m = (x[idx+1] - x[idx]) / (acc[idx+1] - acc[idx]), b = x[idx] - m acc[idx], d_out[p] = m target + b -- including the
 *       linear extrapolation below the first knot, and NaN where all weights are 0.  n_ps in 1..8, n >= 2.  An order entry
 *       outside [0, n) poisons the result with NaN and reads nothing out of bounds.
 *   refnerf_vis_panels   every per-pixel panel of visualize_suite in one launch; every pointer is optional and an output is
 *       written when it and its inputs are given.  acc' = acc, 0 where distance_mean is NaN.  matte(v) = v acc' +
 *       bg (1 - acc') with the 8-pixel checker bg in {float32(0.8), 1}.  color / diffuse / specular: the sRGB curve when
 *       linear_to_srgb is set.  depth_mean / depth_median: c(v) = -log(v + eps), q = nan_to_num(clip((c(v) - min(lo, hi)) /
 *       |hi - lo|, 0, 1)) with lo = c(lohi[0] - eps), hi = c(lohi[1] + eps), colour d_table[min(int(q N), N - 1)], matted.
 *       depth_triplet: (2 median - p5, median, p95) through c(v) = log(v + eps) alike, no table.  coords_mod:
 *       ((origins + directions distance_mean + 1) mod 2) / 2 with the sign of the divisor, matted (NaN where the distance
 *       is NaN, as in the reference).  normals_out[k]: matte(n / 2 + 0.5); roughness: matte(tanh(r)), roughness_channels
 *       wide; tint_matte; color_corrected: a copy.  d_lohi_*: two doubles each, the RAW percentiles of entry 1.
 *   refnerf_vis_cmap   visualize_cmap on n = H * W values of `channels` channels: optional curve, optional normalisation
 *       (lo = [*d_lo +] lo_bias, hi = [*d_hi +] hi_bias, then curved), optional table (channels must be 1; output 3
 *       channels), optional matte (d_acc), optional null colour where d_alpha == 0 (visualize_suite's ray_weights panel).
 *   refnerf_vis_resample_rays   stepfun.resample(edges, sdist, ., use_avg=True) of n step functions (sdist [n][N+1], values
 *       [n][N][C], weights [n][N] or NULL = ones) onto the `resolution` bins between the resolution + 1 edges d_edges:
 *       sequential float64 cumulative sums, the reference's interp at every edge INCLUDING its extrapolation outside
 *       [sdist[0], sdist[N]], numer / max(eps, denom).  accumulate: visualize_rays' accumulated colour and weight.
 *       value_op: REFNERF_VIS_OP_*.  Line i goes to d_out_values + i * line_stride * resolution * C (alpha alike), so the
 *       levels of one bundle interleave into [n][L][resolution][C].  (N + 1) * (C + 3) * 8 bytes of LDS: at most 48 KB.
 *   refnerf_vis_ray_panel   visualize_rays' panel from the [n][L] lines: alpha / max(eps, *d_alpha_max) when d_alpha_max is
 *       given (renormalize), rep > 0: every line rep times, one background strip per ray, the last row dropped
 *       (n (L rep + 1) - 1 rows); rep = 0: the lines of the first n - 1 rays; out = v alpha + bg_color (1 - alpha).
 * REFNERF_EINVAL: a missing required pointer, sizes outside the stated ranges, a workspace too small. */
enum { REFNERF_VIS_CURVE_NONE = 0, REFNERF_VIS_CURVE_NEG_LOG = 1 /* -log(x + eps) */, REFNERF_VIS_CURVE_LOG = 2 /* log(x + eps) */ };
enum { REFNERF_VIS_OP_NONE = 0, REFNERF_VIS_OP_CLIP01 = 1 /* clip(v, 0, 1) */, REFNERF_VIS_OP_SQRT = 2 /* sqrt(v) */ };
#define REFNERF_VIS_MAX_PS 8
#define REFNERF_VIS_MAX_NORMALS 4
typedef struct refnerf_vis_panels_args {
  int32_t H, W, f64, linear_to_srgb, table_n, roughness_channels;
  const float *d_table;                                            /* [table_n][3] */
  const double *d_lohi_mean, *d_lohi_median, *d_lohi_triplet;      /* [2] each */
  const void *d_rgb, *d_acc, *d_distance_mean, *d_distance_median, *d_distance_p5, *d_distance_p95, *d_origins, *d_directions,
      *d_normals[REFNERF_VIS_MAX_NORMALS], *d_roughness, *d_diffuse, *d_specular, *d_tint, *d_rgb_cc;
  void *d_color, *d_acc_out, *d_color_matte, *d_depth_mean, *d_depth_median, *d_depth_triplet, *d_coords_mod,
      *d_normals_out[REFNERF_VIS_MAX_NORMALS], *d_roughness_out, *d_diffuse_out, *d_diffuse_matte, *d_specular_out,
      *d_specular_matte, *d_tint_matte, *d_color_corrected;
} refnerf_vis_panels_args;
typedef struct refnerf_vis_cmap_args {
  int32_t H, W, channels, f64 /* d_values, d_acc */, out_f64, curve, normalise, table_n;
  double lo_bias, hi_bias, null_color[3];
  const void *d_values, *d_acc /* [H][W] or NULL: no matte */;
  const double *d_lo, *d_hi /* device scalars or NULL */, *d_alpha /* [H][W] or NULL */;
  const float *d_table;
  void *d_out;                                                     /* [H][W][table ? 3 : channels] */
} refnerf_vis_cmap_args;
size_t refnerf_vis_percentile_workspace_bytes(int64_t n);
int refnerf_vis_weighted_percentile(const void *d_values, int32_t values_f64, const void *d_weights, int32_t weights_f64,
                                    int64_t n_weights, const void *d_nan_mask, const int64_t *d_order, int64_t n,
                                    const double *ps /* host */, int32_t n_ps, int32_t target_f32, double *d_out /* [n_ps] */,
                                    void *d_workspace, size_t workspace_bytes, void *stream);
int refnerf_vis_panels(const refnerf_vis_panels_args *args, void *stream);
int refnerf_vis_cmap(const refnerf_vis_cmap_args *args, void *stream);
int refnerf_vis_resample_rays(const void *d_sdist, const void *d_values, const void *d_weights, int32_t f64, int32_t n, int32_t N,
                              int32_t C, const double *d_edges, int32_t resolution, int32_t accumulate, int32_t value_op,
                              int64_t line_stride, double *d_out_values, double *d_out_alpha, void *stream);
int refnerf_vis_ray_panel(const double *d_lines_values, const double *d_lines_alpha, int32_t n, int32_t L, int32_t resolution,
                          int32_t C, int32_t rep, double bg_color, const double *d_alpha_max, double *d_out_vis,
                          double *d_out_alpha, void *stream);

/* Total duration (ms) and count of the `refnerf_level_forward` kernels launched
 * since refnerf_set_timing(1), from HIP event pairs on the launch stream.
 * Used by bench.py for the roofline line. */
enum { REFNERF_TIMER_FORWARD = 0,   /* the level kernel of refnerf_level_forward / _forward_train           */
       REFNERF_TIMER_BACKWARD = 1,  /* the per-sample backward kernel of refnerf_level_backward              */
       REFNERF_TIMER_WGRAD = 2,     /* its weight-gradient GEMM                                              */
       REFNERF_TIMER_IMAGE = 3,     /* one pair per image-evaluation entry, around all of its launches       */
       REFNERF_TIMER_DATASET = 4 }; /* the one kernel of refnerf_prepare_images / refnerf_train_batch        */
int refnerf_set_timing(int enable);
int refnerf_get_timing(double *total_ms, int64_t *launches);                         /* REFNERF_TIMER_FORWARD */
int refnerf_get_timing_family(int family, double *total_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif
