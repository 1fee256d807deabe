/*
 * refnerf_dataset.h -- the two device stages of the scene loaders (internal/datasets.py):
 *
 * image_prepare_kernel: a stack of decoded images [n,H,W,C] (uint8 as PIL decodes them, or float32) to the float32
 * arrays the reference's `_load_renderings` builds: area downsample by an integer factor (image.downsample, a block
 * mean), `/ 255`, and the white-background compositing of Blender (:550, :567-570), the normal decoding (:557) or the
 * bare mean of the disparity TIFFs (:554).  One thread per output pixel; HBM-bound (C bytes in per source pixel,
 * 4 * C_out bytes out per output pixel).  The arithmetic is the reference's float32 numpy flow, operation for
 * operation and rounding for rounding: every product, quotient, sum and difference is rounded on its own (the *_rn
 * spellings say so; contraction is switched off in the kernel body, and the library is built with -ffp-contract=off).
 *
 * train_batch_kernel: one training batch in one launch -- `Dataset._next_train` / `_make_ray_batch` (:395-485) from the
 * integer patch origins and camera indices: the nine `Rays` fields (the arithmetic of pixels_to_rays_kernel, through
 * cast_pixel_ray) and the gathered rgb / disps / normals / alphas.  The camera is indexed inside the kernel, so no
 * per-ray camera tensor exists.  One thread per ray; 64 B of rays + up to 32 B of gathered pixels out per ray.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "refnerf_rays.h"

namespace rn {

enum { PREP_SCALE = 0, PREP_WHITE = 1, PREP_NORMALS = 2, PREP_RAW = 3 };
constexpr int DATASET_THREADS = 256;

struct ImagePrepareArgs {
  const void *src;          /* [n,H,W,C] uint8 or float32 */
  long long total;          /* n * h * w output pixels, h = H / factor, w = W / factor */
  int H, W, h, w, factor, op;
  float *out;               /* [n,h,w,C_out] */
  float *alpha;             /* [n,h,w] or NULL (PREP_WHITE only) */
};

/* The block mean of one channel set, as numpy computes `img.reshape(h, f, w, f, C).mean((1, 3))` on float32:
 * float32(sum) / float32(f * f).  uint8 sources: the integer sum is exact and equals numpy's float32 sum whatever its
 * order while f * f * 255 < 2^24 (the host refuses larger factors).  float32 sources: the sum is taken in double and
 * rounded once.  kVec: C = 4 uint8 pixels read as one aligned 32-bit word (the host checks the alignment). */
template <typename T, int C, bool kVec>
__device__ __forceinline__ void block_mean(const ImagePrepareArgs &A, long long img, int oy, int ox, float mean[C]) {
  const int f = A.factor;
  const T *src = static_cast<const T *>(A.src);
  const float count = (float)(f * f);
  if constexpr (sizeof(T) == 1) {
    unsigned sum[C];
#pragma unroll
    for (int c = 0; c < C; ++c) sum[c] = 0u;
    for (int dy = 0; dy < f; ++dy) {
      const long long row = ((img * A.H + ((long long)oy * f + dy)) * A.W + (long long)ox * f) * C;
      for (int dx = 0; dx < f; ++dx) {
        if constexpr (kVec) {
          const uint32_t word = *reinterpret_cast<const uint32_t *>(src + row + (long long)dx * 4);
#pragma unroll
          for (int c = 0; c < 4; ++c) sum[c] += (word >> (8 * c)) & 0xffu;
        } else {
#pragma unroll
          for (int c = 0; c < C; ++c) sum[c] += src[row + (long long)dx * C + c];
        }
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) mean[c] = __fdiv_rn((float)sum[c], count);
  } else {
    double sum[C];
#pragma unroll
    for (int c = 0; c < C; ++c) sum[c] = 0.0;
    for (int dy = 0; dy < f; ++dy) {
      const long long row = ((img * A.H + ((long long)oy * f + dy)) * A.W + (long long)ox * f) * C;
      for (int dx = 0; dx < f; ++dx)
#pragma unroll
        for (int c = 0; c < C; ++c) sum[c] += (double)src[row + (long long)dx * C + c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) mean[c] = __fdiv_rn((float)sum[c], count);
  }
}

template <typename T, int C, bool kVec>
__global__ void image_prepare_kernel(const ImagePrepareArgs A) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * DATASET_THREADS + threadIdx.x;
  if (i >= A.total) return;
  const long long per_image = (long long)A.h * A.w;
  const long long img = i / per_image, rem = i - img * per_image;
  const int oy = (int)(rem / A.w), ox = (int)(rem - (long long)oy * A.w);
  float m[C];
  block_mean<T, C, kVec>(A, img, oy, ox, m);
  if (A.op == PREP_RAW) {                                  /* get_img('_disp.tiff') (:554) */
#pragma unroll
    for (int c = 0; c < C; ++c) A.out[i * C + c] = m[c];
  } else if (A.op == PREP_SCALE) {                         /* np.stack(images) / 255. (:637) */
#pragma unroll
    for (int c = 0; c < C; ++c) A.out[i * C + c] = __fdiv_rn(m[c], 255.0f);
  } else if (A.op == PREP_NORMALS) {                       /* [..., :3] * 2. / 255. - 1. (:557) */
    if constexpr (C >= 3) {
#pragma unroll
      for (int c = 0; c < 3; ++c) A.out[i * 3 + c] = __fsub_rn(__fdiv_rn(__fmul_rn(m[c], 2.0f), 255.0f), 1.0f);
    }
  } else {                                                 /* PREP_WHITE: rgb * alpha + (1. - alpha) (:550, :567-570) */
    if constexpr (C == 4) {
      const float a = __fdiv_rn(m[3], 255.0f);
      const float bg = __fsub_rn(1.0f, a);
#pragma unroll
      for (int c = 0; c < 3; ++c) A.out[i * 3 + c] = __fadd_rn(__fmul_rn(__fdiv_rn(m[c], 255.0f), a), bg);
      if (A.alpha) A.alpha[i] = a;
    }
  }
}

template <typename T, int C, bool kVec>
inline void launch_image_prepare(const ImagePrepareArgs &a, hipStream_t st) {
  const unsigned blocks = (unsigned)((a.total + DATASET_THREADS - 1) / DATASET_THREADS);
  hipLaunchKernelGGL((image_prepare_kernel<T, C, kVec>), dim3(blocks), dim3(DATASET_THREADS), 0, st, a);
}

struct TrainBatchArgs {
  const void *px0, *py0;    /* [P]: the patch origins, int32 or (idx64) int64 as torch.randint draws them */
  const void *cam;          /* [P] (cam_stride 1) or one index for the batch (cam_stride 0) */
  int idx64, cam_stride;
  int ps;                   /* patch size: ps * ps rays per patch */
  int n;                    /* P * ps * ps rays */
  int n_images, H, W;
  const float *images;      /* [n_images,H,W,3] */
  const float *disps, *normals, *alphas;   /* [n_images,H,W(,3)] or NULL */
  const float *pixtocams;   /* [3,3] (p2c_stride 0) or [n_images,3,3] (p2c_stride 9) */
  int p2c_stride;
  const float *camtoworlds; /* [n_images,3,4] */
  const float *pixtocam_ndc; /* [3,3] or NULL */
  float near, far;
  float *origins, *directions, *viewdirs, *radii, *imageplane, *lossmult, *near_out, *far_out;
  int *cam_idx_out;
  float *rgb, *disps_out, *normals_out, *alphas_out;
  LensDistortion dist;      /* read by the distorted instantiation only */
};

/* Ray i is pixel (px0[p] + i % ps, py0[p] + (i / ps) % ps) of camera cam[p], p = i / ps^2: the [P,ps,ps] broadcast of
 * datasets.py:472-477.  The rays are cast from the coordinates as given (as pixels_to_rays_kernel does); the image and
 * camera loads clamp them into the stacks, so indices from outside the scene cannot read out of bounds. */
__device__ __forceinline__ int load_index(const void *base, int idx64, size_t i) {
  return idx64 ? (int)static_cast<const long long *>(base)[i] : static_cast<const int *>(base)[i];
}

template <bool kDistort>
__global__ void train_batch_kernel(const TrainBatchArgs A) {
  const int i = blockIdx.x * DATASET_THREADS + threadIdx.x;
  if (i >= A.n) return;
  const int pp = A.ps * A.ps;
  const int p = i / pp, r = i - p * pp;
  const int dy = r / A.ps, dx = r - dy * A.ps;
  const int x = load_index(A.px0, A.idx64, p) + dx, y = load_index(A.py0, A.idx64, p) + dy;
  const int cam_given = load_index(A.cam, A.idx64, (size_t)p * A.cam_stride);
  const int cam = min(max(cam_given, 0), A.n_images - 1);
  const float *p2c = A.pixtocams + (size_t)cam * A.p2c_stride;
  const float *c2w = A.camtoworlds + (size_t)cam * 12;
  float o[3], d_out[3], v_out[3], radius, ip[2];
  cast_pixel_ray<kDistort>(p2c, c2w, A.pixtocam_ndc, A.dist, (float)x, (float)y, o, d_out, v_out, radius, ip);
  const int xc = min(max(x, 0), A.W - 1), yc = min(max(y, 0), A.H - 1);
  const long long pix = ((long long)cam * A.H + yc) * A.W + xc;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    A.origins[(size_t)i * 3 + c] = o[c];
    A.directions[(size_t)i * 3 + c] = d_out[c];
    A.viewdirs[(size_t)i * 3 + c] = v_out[c];
    A.rgb[(size_t)i * 3 + c] = A.images[pix * 3 + c];
  }
  A.radii[i] = radius;
  A.imageplane[(size_t)i * 2] = ip[0]; A.imageplane[(size_t)i * 2 + 1] = ip[1];
  A.lossmult[i] = 1.0f;
  A.near_out[i] = A.near;
  A.far_out[i] = A.far;
  A.cam_idx_out[i] = cam_given;
  if (A.disps_out) A.disps_out[i] = A.disps[pix];
  if (A.alphas_out) A.alphas_out[i] = A.alphas[pix];
  if (A.normals_out) {
#pragma unroll
    for (int c = 0; c < 3; ++c) A.normals_out[(size_t)i * 3 + c] = A.normals[pix * 3 + c];
  }
}

}  // namespace rn
