/* Test-image evaluation on the device (the metric half of the reference's test_step, nerf_system.py:391-444): squared error
 * and PSNR, SSIM (dm_pix.ssim with its defaults), colour correction (internal/image.py:84-127) and the weighted angular
 * error of normals (ref_utils.py:45-50).
 *
 * Images are double [H][W][C] with a row pitch in ELEMENTS (a border crop is a pointer offset, never a copy), and ALL
 * arithmetic is float64: the reference casts to float64 before it evaluates.
 *
 *   image_sqerr_kernel     one block per 4096 elements: sum (q(a) - b)^2 -> one partial
 *   image_wmae_kernel      one block per 1024 pixels: { sum w acos(clip(n . n_gt)), sum w } -> two partials
 *   image_ssim_kernel      one block per 16 x 16 output tile (all channels): sum of the tile's SSIM map -> one partial
 *   image_finalize_kernel  one block: the partials in index order -> the result (mean, PSNR, degrees)
 *   cc_accum_kernel        one block per (1024 pixels, channel): the masked normal equations G_c = sum m a a^T (55 unique
 *                          entries) and r_c = sum m a ref_c of the ten-term expansion a = [r2 rg rb g2 gb b2 r g b 1]
 *   cc_solve_kernel        one block: the partials in index order, then one lane per channel runs a serial cyclic-Jacobi
 *                          eigendecomposition of its 10 x 10 system and applies the pseudo-inverse -> warp [10][3]
 *   cc_apply_kernel        per pixel: x <- clip(a W, 0, 1) (in place from the second iteration on)
 *
 * No float atomics anywhere: every sum has one fixed order (thread's elements in order -> wave64 butterfly -> the four
 * waves in order -> the blocks in index order), so two runs of the same inputs are bit-identical, and a pitched view gives
 * the bits of its contiguous copy (the work is cut by the logical index, never by the address).  No host synchronisation,
 * no allocation: partials live in the caller's workspace.
 *
 * SSIM tile.  A T x T output tile needs two (T+10)^2 input tiles and five T x (T+10) planes filtered along H in LDS:
 * 8 (2 (T+10)^2 + 5 T (T+10)) bytes.  T = 16 is 27.5 KB, so five workgroups (20 waves) share the 160 KiB of a CU and hide
 * each other's LDS latency and barriers; one thread owns one output pixel of the pass along W.  T = 32 would cut the apron
 * overhead from (26/16)^2 = 2.6 to 1.7 loads per pixel but needs 82 KB, one 256-thread workgroup per CU, which waits on
 * its own barriers alone.  The kernel is LDS-latency bound, not load bound (an 800 x 800 x 3 image is 2500 tiles of 10 KB of
 * input each), so the occupancy wins.
 *
 * Colour correction replaces the reference's masked lstsq on the [n][10] system by the normal equations, which agree with
 * it to 1e-13 on images whose masked G_c is well conditioned.  It does NOT reproduce lstsq on near-rank-deficient input
 * (a constant colour, say): there lstsq decides the rank on A and the pseudo-inverse here decides it on G = A^T A
 * (eigenvalues <= 10 * 2^-52 * lambda_max are dropped), and the two decisions differ.  An all-masked channel gives w = 0 in
 * both. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RN_IMG_HD __host__ __device__
#else
#define RN_IMG_HD
#endif

namespace rn {

constexpr int IMG_THREADS = 256;
constexpr int IMG_ELEMS_PER_BLOCK = 4096;     /* squared error: 16 elements per thread */
constexpr int IMG_PIX_PER_BLOCK = 1024;       /* colour correction, angular error: 4 pixels per thread */
constexpr int SSIM_TAPS = 11;
constexpr int SSIM_TILE = 16;
constexpr int SSIM_IN = SSIM_TILE + SSIM_TAPS - 1;
constexpr int CC_TERMS = 10;
constexpr int CC_GRAM = 55;                   /* upper triangle of a a^T, row-major */
constexpr int CC_PART = CC_GRAM + CC_TERMS;   /* + a ref_c */
constexpr int CC_SWEEPS = 50;
static_assert(IMG_THREADS == SSIM_TILE * SSIM_TILE, "one thread per output pixel of an SSIM tile");

enum { IMG_FIN_MEAN = 0, IMG_FIN_MSE_PSNR = 1, IMG_FIN_DEGREES = 2 };

/* mse_to_psnr's factor.  The reference writes -10. / torch.log(torch.tensor(10.)): a float32 tensor, so the factor its
 * float64 PSNR is multiplied by is float32(-10 / float32(ln 10)), 5e-9 (relative) away from -10 / ln 10. */
constexpr double IMG_PSNR_FACTOR = -0x1.15f2cep+2;   /* -4.342944622039795 */

struct SsimTaps { double g[SSIM_TAPS]; };

__device__ __forceinline__ double img_quant(double x, int quantize) {
  return quantize ? rint(x * 255.0) / 255.0 : x;      /* rint: half to even, as torch.round */
}

__device__ __forceinline__ double img_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

/* the block's total (waves in order), valid on every thread; `red` holds IMG_THREADS / 64 doubles */
__device__ __forceinline__ double img_block_sum(double v, double *red) {
  v = img_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int k = 1; k < IMG_THREADS / 64; ++k) t += red[k];
  __syncthreads();
  return t;
}

/* ------------------------------------------------------------------------------------------ squared error */
__global__ __launch_bounds__(IMG_THREADS) void image_sqerr_kernel(const double *__restrict__ a, int64_t pitch_a,
                                                                  const double *__restrict__ b, int64_t pitch_b, int32_t row_len,
                                                                  int64_t n, int32_t quantize, double *__restrict__ partials) {
  __shared__ double red[IMG_THREADS / 64];
  const int64_t base = (int64_t)blockIdx.x * IMG_ELEMS_PER_BLOCK + threadIdx.x;
  double acc = 0.0;
#pragma unroll 4
  for (int k = 0; k < IMG_ELEMS_PER_BLOCK / IMG_THREADS; ++k) {
    const int64_t i = base + (int64_t)k * IMG_THREADS;
    if (i < n) {
      const int64_t row = i / row_len, col = i - row * row_len;
      const double d = img_quant(a[row * pitch_a + col], quantize) - b[row * pitch_b + col];
      acc += d * d;
    }
  }
  const double tot = img_block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

/* ------------------------------------------------------------------------------------------ weighted angular error */
__global__ __launch_bounds__(IMG_THREADS) void image_wmae_kernel(const double *__restrict__ w, const double *__restrict__ nrm,
                                                                 const double *__restrict__ nrm_gt, int64_t n,
                                                                 double *__restrict__ partials) {
  __shared__ double red[IMG_THREADS / 64];
  const double one_eps = 1.0 - 0x1p-23;            /* 1 - finfo(float32).eps */
  const int64_t base = (int64_t)blockIdx.x * IMG_PIX_PER_BLOCK + threadIdx.x;
  double num = 0.0, den = 0.0;
#pragma unroll
  for (int k = 0; k < IMG_PIX_PER_BLOCK / IMG_THREADS; ++k) {
    const int64_t i = base + (int64_t)k * IMG_THREADS;
    if (i < n) {
      const double *p = nrm + 3 * i, *q = nrm_gt + 3 * i;
      double d = p[0] * q[0] + p[1] * q[1] + p[2] * q[2];
      d = d < -one_eps ? -one_eps : (d > one_eps ? one_eps : d);      /* torch.clip: a NaN stays a NaN */
      const double wi = w[i];
      num += wi * acos(d);
      den += wi;
    }
  }
  const double tn = img_block_sum(num, red), td = img_block_sum(den, red);
  if (threadIdx.x == 0) {
    partials[2 * (int64_t)blockIdx.x + 0] = tn;
    partials[2 * (int64_t)blockIdx.x + 1] = td;
  }
}

/* ------------------------------------------------------------------------------------------ the final pass
 * One block.  Thread t adds the partials t, t + 256, ... in order, then thread 0 adds the 256 sums in order. */
__global__ __launch_bounds__(IMG_THREADS) void image_finalize_kernel(const double *__restrict__ partials, int32_t n_part,
                                                                     int32_t n_val, int32_t mode, double denom,
                                                                     double *__restrict__ out) {
  __shared__ double red[2][IMG_THREADS];
  const int tid = threadIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (int i = tid; i < n_part; i += IMG_THREADS) {
    s0 += partials[(int64_t)i * n_val];
    if (n_val > 1) s1 += partials[(int64_t)i * n_val + 1];
  }
  red[0][tid] = s0;
  red[1][tid] = s1;
  __syncthreads();
  if (tid == 0) {
    double t0 = 0.0, t1 = 0.0;
    for (int k = 0; k < IMG_THREADS; ++k) {
      t0 += red[0][k];
      t1 += red[1][k];
    }
    if (mode == IMG_FIN_MSE_PSNR) {
      const double mse = t0 / denom;
      out[0] = mse;
      out[1] = IMG_PSNR_FACTOR * log(mse);
    } else if (mode == IMG_FIN_DEGREES) {
      out[0] = t0 / t1 * 180.0 / 3.141592653589793;
    } else {
      out[0] = t0 / denom;
    }
  }
}

/* ------------------------------------------------------------------------------------------ SSIM */
__global__ __launch_bounds__(IMG_THREADS) void image_ssim_kernel(const double *__restrict__ a, int64_t pitch_a,
                                                                 const double *__restrict__ b, int64_t pitch_b, int32_t H, int32_t W,
                                                                 int32_t C, int32_t quantize, SsimTaps taps,
                                                                 double *__restrict__ partials, double *__restrict__ map) {
  __shared__ double sa[SSIM_IN][SSIM_IN], sb[SSIM_IN][SSIM_IN];
  __shared__ double pl[5][SSIM_TILE][SSIM_IN];       /* filtered along H: mu_a, mu_b, a^2, b^2, ab */
  __shared__ double red[IMG_THREADS / 64];
  const int tid = threadIdx.x;
  const int OH = H - (SSIM_TAPS - 1), OW = W - (SSIM_TAPS - 1);
  const int oy0 = blockIdx.y * SSIM_TILE, ox0 = blockIdx.x * SSIM_TILE;
  const int oy = tid / SSIM_TILE, ox = tid % SSIM_TILE;
  const bool inside = oy0 + oy < OH && ox0 + ox < OW;
  const double eps = 0x1p-23 * 0x1p-23, c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
  double acc = 0.0;
  for (int c = 0; c < C; ++c) {
    for (int idx = tid; idx < SSIM_IN * SSIM_IN; idx += IMG_THREADS) {
      const int iy = idx / SSIM_IN, ix = idx % SSIM_IN;
      const int gy = oy0 + iy, gx = ox0 + ix;
      double va = 0.0, vb = 0.0;                     /* outside the image: feeds only outputs that are never used */
      if (gy < H && gx < W) {
        va = img_quant(a[(int64_t)gy * pitch_a + (int64_t)gx * C + c], quantize);
        vb = b[(int64_t)gy * pitch_b + (int64_t)gx * C + c];
      }
      sa[iy][ix] = va;
      sb[iy][ix] = vb;
    }
    __syncthreads();
    for (int idx = tid; idx < SSIM_TILE * SSIM_IN; idx += IMG_THREADS) {
      const int py = idx / SSIM_IN, ix = idx % SSIM_IN;
      double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
      for (int k = 0; k < SSIM_TAPS; ++k) {
        const double x = sa[py + k][ix], y = sb[py + k][ix], g = taps.g[k];
        m0 += g * x;
        m1 += g * y;
        m2 += g * (x * x);
        m3 += g * (y * y);
        m4 += g * (x * y);
      }
      pl[0][py][ix] = m0;
      pl[1][py][ix] = m1;
      pl[2][py][ix] = m2;
      pl[3][py][ix] = m3;
      pl[4][py][ix] = m4;
    }
    __syncthreads();
    double mu_a = 0.0, mu_b = 0.0, f_aa = 0.0, f_bb = 0.0, f_ab = 0.0;
#pragma unroll
    for (int k = 0; k < SSIM_TAPS; ++k) {
      const double g = taps.g[k];
      mu_a += g * pl[0][oy][ox + k];
      mu_b += g * pl[1][oy][ox + k];
      f_aa += g * pl[2][oy][ox + k];
      f_bb += g * pl[3][oy][ox + k];
      f_ab += g * pl[4][oy][ox + k];
    }
    if (inside) {
      const double mu_aa = mu_a * mu_a, mu_bb = mu_b * mu_b, mu_ab = mu_a * mu_b;
      const double s_aa = fmax(eps, f_aa - mu_aa), s_bb = fmax(eps, f_bb - mu_bb);
      const double s = f_ab - mu_ab;
      const double mag = fmin(sqrt(s_aa * s_bb), fabs(s));
      const double s_ab = s > 0.0 ? mag : (s < 0.0 ? -mag : 0.0);
      const double v = ((2.0 * mu_ab + c1) * (2.0 * s_ab + c2)) / ((mu_aa + mu_bb + c1) * (s_aa + s_bb + c2));
      acc += v;
      if (map) map[((int64_t)(oy0 + oy) * OW + (ox0 + ox)) * C + c] = v;
    }
    __syncthreads();                                 /* the next channel overwrites sa / sb / pl */
  }
  const double tot = img_block_sum(acc, red);
  if (tid == 0) partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

/* ------------------------------------------------------------------------------------------ colour correction */
__device__ __forceinline__ bool cc_unclipped(double z, double eps) { return z >= eps && z <= 1.0 - eps; }

__device__ __forceinline__ void cc_expand(double r, double g, double b, double *t) {
  t[0] = r * r; t[1] = r * g; t[2] = r * b; t[3] = g * g; t[4] = g * b; t[5] = b * b;
  t[6] = r; t[7] = g; t[8] = b; t[9] = 1.0;
}

/* grid (blocks of 1024 pixels, 3 channels).  x: the current estimate, img0: the original image (mask0), ref: the target */
__global__ __launch_bounds__(IMG_THREADS) void cc_accum_kernel(const double *x, int64_t pitch_x, const double *__restrict__ img0,
                                                               int64_t pitch_0, const double *__restrict__ ref, int64_t pitch_r,
                                                               int32_t W, int64_t npix, double eps, double *__restrict__ partials) {
  __shared__ double red[IMG_THREADS / 64][CC_PART];
  const int tid = threadIdx.x, c = blockIdx.y;
  double acc[CC_PART];
#pragma unroll
  for (int e = 0; e < CC_PART; ++e) acc[e] = 0.0;
  const int64_t base = (int64_t)blockIdx.x * IMG_PIX_PER_BLOCK + tid;
  for (int k = 0; k < IMG_PIX_PER_BLOCK / IMG_THREADS; ++k) {
    const int64_t p = base + (int64_t)k * IMG_THREADS;
    if (p >= npix) continue;
    const int64_t row = p / W, col = (p - row * W) * 3;
    const double *px = x + row * pitch_x + col;
    const double xr = px[0], xg = px[1], xb = px[2];
    const double xc = c == 0 ? xr : (c == 1 ? xg : xb);
    const double oc = img0[row * pitch_0 + col + c], rc = ref[row * pitch_r + col + c];
    if (!(cc_unclipped(oc, eps) && cc_unclipped(xc, eps) && cc_unclipped(rc, eps))) continue;
    double t[CC_TERMS];
    cc_expand(xr, xg, xb, t);
    int e = 0;
#pragma unroll
    for (int i = 0; i < CC_TERMS; ++i)
#pragma unroll
      for (int j = i; j < CC_TERMS; ++j) acc[e++] += t[i] * t[j];
#pragma unroll
    for (int i = 0; i < CC_TERMS; ++i) acc[CC_GRAM + i] += t[i] * rc;
  }
#pragma unroll
  for (int e = 0; e < CC_PART; ++e) {
    const double v = img_wave_sum(acc[e]);
    if ((tid & 63) == 0) red[tid >> 6][e] = v;
  }
  __syncthreads();
  if (tid < CC_PART) {
    double s = red[0][tid];
#pragma unroll
    for (int k = 1; k < IMG_THREADS / 64; ++k) s += red[k][tid];
    partials[((int64_t)blockIdx.x * 3 + c) * CC_PART + tid] = s;
  }
}

/* The pseudo-inverse solve of one channel: G (symmetric 10 x 10, row-major in A, destroyed), r -> w = pinv(G) r.
 * Cyclic Jacobi (Rutishauser's thresholds): rotations J^T A J in the (p, q) planes until the off-diagonal is exactly
 * zero; an element that no longer changes either diagonal in double is set to zero.  V collects the eigenvectors. */
RN_IMG_HD inline void cc_solve_channel(double *A, double *V, const double *r, double *w, int w_stride) {
  const int n = CC_TERMS;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) V[i * n + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < CC_SWEEPS; ++sweep) {
    double sm = 0.0;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) sm += fabs(A[p * n + q]);
    if (!(sm > 0.0)) break;                       /* converged (or NaN: give up, the NaN reaches w) */
    const double tresh = sweep < 3 ? 0.2 * sm / (n * n) : 0.0;
    for (int p = 0; p < n - 1; ++p) {
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q], app = A[p * n + p], aqq = A[q * n + q];
        const double g = 100.0 * fabs(apq);
        if (sweep > 3 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
          A[p * n + q] = A[q * n + p] = 0.0;
          continue;
        }
        if (!(fabs(apq) > tresh)) continue;
        const double h = aqq - app;
        double t;
        if (fabs(h) + g == fabs(h)) {
          t = apq / h;
        } else {
          const double theta = 0.5 * h / apq;
          t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
          if (theta < 0.0) t = -t;
        }
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs;
        for (int k = 0; k < n; ++k) {             /* columns p, q of A and V */
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = cs * akp - sn * akq;
          A[k * n + q] = sn * akp + cs * akq;
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = cs * vkp - sn * vkq;
          V[k * n + q] = sn * vkp + cs * vkq;
        }
        for (int k = 0; k < n; ++k) {             /* rows p, q of A */
          const double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = cs * apk - sn * aqk;
          A[q * n + k] = sn * apk + cs * aqk;
        }
        A[p * n + q] = A[q * n + p] = 0.0;
      }
    }
  }
  double lmax = 0.0;
  for (int k = 0; k < n; ++k) lmax = A[k * n + k] > lmax ? A[k * n + k] : lmax;
  const double tol = 10.0 * 0x1p-52 * lmax;         /* torch.linalg.pinv(hermitian=True): rtol = n * eps */
  for (int i = 0; i < n; ++i) w[i * w_stride] = 0.0;
  for (int k = 0; k < n; ++k) {
    const double lam = A[k * n + k];
    if (!(lam > tol)) continue;
    double proj = 0.0;
    for (int j = 0; j < n; ++j) proj += V[j * n + k] * r[j];
    proj /= lam;
    for (int i = 0; i < n; ++i) w[i * w_stride] += V[i * n + k] * proj;
  }
}

__global__ __launch_bounds__(IMG_THREADS) void cc_solve_kernel(const double *__restrict__ partials, int32_t n_blocks,
                                                               double *__restrict__ warp, double *__restrict__ warp_out) {
  __shared__ double S[3][CC_PART];
  __shared__ double A[3][CC_TERMS * CC_TERMS], V[3][CC_TERMS * CC_TERMS];
  __shared__ double wl[CC_TERMS * 3];
  const int tid = threadIdx.x;
  if (tid < 3 * CC_PART) {
    const int c = tid / CC_PART, e = tid % CC_PART;
    double s = 0.0;
#pragma unroll 8                                   /* the loads of eight partials in flight, the adds still in index order */
    for (int b = 0; b < n_blocks; ++b) s += partials[((int64_t)b * 3 + c) * CC_PART + e];
    S[c][e] = s;
  }
  __syncthreads();
  if (tid < 3) {
    int e = 0;
    for (int i = 0; i < CC_TERMS; ++i)
      for (int j = i; j < CC_TERMS; ++j) {
        A[tid][i * CC_TERMS + j] = A[tid][j * CC_TERMS + i] = S[tid][e];
        ++e;
      }
    cc_solve_channel(A[tid], V[tid], &S[tid][CC_GRAM], wl + tid, 3);
  }
  __syncthreads();
  if (tid < CC_TERMS * 3) {
    warp[tid] = wl[tid];
    if (warp_out) warp_out[tid] = wl[tid];
  }
}

/* out [H][W][3] dense; src may BE out (each thread reads its pixel before it writes it).  warp == nullptr: a copy. */
__global__ __launch_bounds__(IMG_THREADS) void cc_apply_kernel(const double *src, int64_t pitch_s, double *out, int32_t W,
                                                               int64_t npix, const double *__restrict__ warp) {
  const int64_t p = (int64_t)blockIdx.x * IMG_THREADS + threadIdx.x;
  if (p >= npix) return;
  const int64_t row = p / W, col = (p - row * W) * 3;
  const double *px = src + row * pitch_s + col;
  double y[3] = {px[0], px[1], px[2]};
  if (warp) {
    double t[CC_TERMS];
    cc_expand(y[0], y[1], y[2], t);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < CC_TERMS; ++i) s += t[i] * warp[i * 3 + c];
      y[c] = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);   /* torch.clip: a NaN stays a NaN */
    }
  }
  double *po = out + p * 3;
  po[0] = y[0];
  po[1] = y[1];
  po[2] = y[2];
}

}  // namespace rn
