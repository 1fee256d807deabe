/* The optimiser step of the reference's training loop (nerf_system.configure_gradient_clipping + on_after_backward,
 * torch.optim.Adam.step): gradient statistics, value + global-norm clipping and Adam, as three kernels.
 *
 *   optim_stats_kernel     one block per work item (a run of <= OPTIM_CHUNK elements inside ONE segment): four partials
 *                          { sum g^2, max |g| (as bits), sum w^2, sum clamp(g)^2 } -> workspace
 *   optim_finalize_kernel  one block: the partials of every tensor of the step, summed in work-item order in double ->
 *                          per-segment statistics, total_norm, clip_coef
 *   optim_adam_kernel      per element: g = clip_coef * clamp(g), torch's Adam update (optionally g written back)
 *
 * No float atomics anywhere: every sum has one fixed order (lane -> wave butterfly -> waves in order -> work items in
 * order -> segments by thread -> threads in order), so two runs of the same inputs are bit-identical. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rn {

constexpr int OPTIM_THREADS = 256;
constexpr int OPTIM_CHUNK = 4096;          /* elements per work item: 4 float4 per thread */
constexpr int OPTIM_STATE_HEADER = 64;     /* bytes: float total_norm, float clip_coef, double sum of clamp(g)^2 */

struct OptimItem { int32_t seg, start, len, pad; };                     /* 16 bytes: one int4 load */
struct OptimDesc {                                                      /* 32 bytes, one per tensor of a step, in the state */
  const int32_t *seg_item_off;  /* [n_seg + 1] first work item of each segment */
  const float *partials;        /* [n_items][4] */
  float *seg_stats;             /* [n_seg][3] grad_norm, grad_max, weight_l2 */
  int32_t n_seg, n_items;
};
static_assert(sizeof(OptimItem) == 16 && sizeof(OptimDesc) == 32, "optimiser workspace layout");

__device__ __forceinline__ float optim_clamp(float g, float val) {
  /* torch.clamp semantics: a NaN stays a NaN (fminf / fmaxf would return the bound) */
  return val > 0.0f ? (g < -val ? -val : (g > val ? val : g)) : g;
}

struct OptimAcc {
  float g2 = 0.0f, w2 = 0.0f, c2 = 0.0f;
  uint32_t gmax = 0u;   /* bits of max |g|: for non-negative floats the integer order is the float order and every NaN sorts
                           above +inf, so an integer max propagates a NaN gradient where fmaxf would drop it */
  __device__ __forceinline__ void add(float g, float w, float val) {
    const float c = optim_clamp(g, val);
    g2 += g * g;
    w2 += w * w;
    c2 += c * c;
    const uint32_t a = __float_as_uint(fabsf(g));
    gmax = a > gmax ? a : gmax;
  }
};

__global__ __launch_bounds__(OPTIM_THREADS) void optim_stats_kernel(const float *__restrict__ grad, const float *__restrict__ param,
                                                                    int32_t n, const OptimItem *__restrict__ items,
                                                                    float *__restrict__ partials, float grad_max_val,
                                                                    OptimDesc desc, OptimDesc *__restrict__ desc_slot) {
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && tid == 0) *desc_slot = desc;      /* the finalize kernel finds this tensor through the state */
  const OptimItem it = items[blockIdx.x];
  /* the plan lives in device memory: never trust it further than the tensor */
  int start = it.start, len = it.len;
  if (start < 0 || start >= n || len < 0) len = 0;
  if (len > OPTIM_CHUNK) len = OPTIM_CHUNK;
  if (len > n - start) len = n - start;
  const float *g = grad + start, *w = param + start;
  OptimAcc acc;
  /* 16-byte loads where both pointers allow: a scalar head up to the boundary, float4 body, scalar tail */
  const uintptr_t ga = (uintptr_t)g & 15u, wa = (uintptr_t)w & 15u;
  if (ga == wa) {
    int head = (int)(((16u - ga) & 15u) >> 2);
    if (head > len) head = len;
    const int nvec = (len - head) >> 2, tail = len - head - 4 * nvec;
    if (tid < head) acc.add(g[tid], w[tid], grad_max_val);
    const float4 *g4 = reinterpret_cast<const float4 *>(g + head), *w4 = reinterpret_cast<const float4 *>(w + head);
    for (int v = tid; v < nvec; v += OPTIM_THREADS) {
      const float4 gv = g4[v], wv = w4[v];
      acc.add(gv.x, wv.x, grad_max_val);
      acc.add(gv.y, wv.y, grad_max_val);
      acc.add(gv.z, wv.z, grad_max_val);
      acc.add(gv.w, wv.w, grad_max_val);
    }
    if (tid < tail) acc.add(g[head + 4 * nvec + tid], w[head + 4 * nvec + tid], grad_max_val);
  } else {
    for (int i = tid; i < len; i += OPTIM_THREADS) acc.add(g[i], w[i], grad_max_val);
  }
  /* wave64 butterfly, then the four waves in order */
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc.g2 += __shfl_xor(acc.g2, o, 64);
    acc.w2 += __shfl_xor(acc.w2, o, 64);
    acc.c2 += __shfl_xor(acc.c2, o, 64);
    const uint32_t m = (uint32_t)__shfl_xor((int)acc.gmax, o, 64);
    acc.gmax = m > acc.gmax ? m : acc.gmax;
  }
  __shared__ float red[OPTIM_THREADS / 64][4];
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = acc.g2;
    red[tid >> 6][1] = __uint_as_float(acc.gmax);
    red[tid >> 6][2] = acc.w2;
    red[tid >> 6][3] = acc.c2;
  }
  __syncthreads();
  if (tid == 0) {
    float g2 = red[0][0], w2 = red[0][2], c2 = red[0][3];
    uint32_t gm = __float_as_uint(red[0][1]);
    for (int k = 1; k < OPTIM_THREADS / 64; ++k) {
      g2 += red[k][0];
      w2 += red[k][2];
      c2 += red[k][3];
      const uint32_t m = __float_as_uint(red[k][1]);
      gm = m > gm ? m : gm;
    }
    float4 out;
    out.x = g2; out.y = __uint_as_float(gm); out.z = w2; out.w = c2;
    reinterpret_cast<float4 *>(partials)[blockIdx.x] = out;
  }
}

/* One block.  Thread t takes the segments t, t + 256, ... of every tensor, each summed over its work items in order.
 * Sized for parameter blobs cut into layers: a segment of m elements is m / 4096 dependent double adds on ONE lane (16 for the
 * largest layer of the Ref-NeRF blob, 271 for that blob as a single segment: microseconds).  It is correct for any size up to
 * 2^31 elements but serial in the segment's length (5e5 adds at the limit); cut such a tensor into more segments. */
__global__ __launch_bounds__(OPTIM_THREADS) void optim_finalize_kernel(unsigned char *__restrict__ state, int32_t n_tensors,
                                                                       float grad_max_norm) {
  const int tid = threadIdx.x;
  const OptimDesc *descs = reinterpret_cast<const OptimDesc *>(state + OPTIM_STATE_HEADER);
  double c2 = 0.0;
  for (int t = 0; t < n_tensors; ++t) {
    const OptimDesc d = descs[t];
    for (int s = tid; s < d.n_seg; s += OPTIM_THREADS) {
      int lo = d.seg_item_off[s], hi = d.seg_item_off[s + 1];
      lo = lo < 0 ? 0 : lo;
      hi = hi > d.n_items ? d.n_items : hi;
      double g2 = 0.0, w2 = 0.0, sc2 = 0.0;
      uint32_t gm = 0u;
      for (int i = lo; i < hi; ++i) {
        const float4 p = reinterpret_cast<const float4 *>(d.partials)[i];
        g2 += (double)p.x;
        w2 += (double)p.z;
        sc2 += (double)p.w;
        const uint32_t m = __float_as_uint(p.y);
        gm = m > gm ? m : gm;
      }
      d.seg_stats[3 * s + 0] = (float)sqrt(g2);
      d.seg_stats[3 * s + 1] = __uint_as_float(gm);
      d.seg_stats[3 * s + 2] = (float)w2;
      c2 += sc2;
    }
  }
  __shared__ double red[OPTIM_THREADS];
  red[tid] = c2;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int k = 0; k < OPTIM_THREADS; ++k) tot += red[k];
    const double total_norm = sqrt(tot);
    /* torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1); a NaN norm gives a NaN coefficient */
    double coef = 1.0;
    if (grad_max_norm > 0.0f) {
      coef = (double)grad_max_norm / (total_norm + 1e-6);
      coef = coef > 1.0 ? 1.0 : coef;
    }
    float *hdr = reinterpret_cast<float *>(state);
    hdr[0] = (float)total_norm;
    hdr[1] = (float)coef;
    *reinterpret_cast<double *>(state + 8) = tot;
  }
}

struct OptimAdamArgs {
  float *p, *g, *m, *v;
  int32_t n;
  float grad_max_val, w1 /* 1 - beta1 */, beta2, w2 /* 1 - beta2 */, step_size /* lr / bc1 */, sqrt_bc2, eps;
  int32_t write_grad, no_step;
  const float *clip_coef;
};

__device__ __forceinline__ void optim_adam_element(const OptimAdamArgs &a, float coef, float &p, float &g, float &m, float &v) {
  g = coef * optim_clamp(g, a.grad_max_val);
  if (a.no_step) return;
  /* torch/optim/adam.py _single_tensor_adam: lerp_, mul_().addcmul_(), (sqrt / bias_correction2_sqrt).add_(eps), addcdiv_ */
  m = m + a.w1 * (g - m);
  v = a.beta2 * v + (a.w2 * g) * g;
  const float denom = sqrtf(v) / a.sqrt_bc2 + a.eps;
  p = p + (-a.step_size) * (m / denom);
}

__global__ __launch_bounds__(OPTIM_THREADS) void optim_adam_kernel(OptimAdamArgs a) {
  const float coef = *a.clip_coef;
  const int tid = threadIdx.x;
  const uintptr_t al = (uintptr_t)a.g & 15u;
  const bool same = a.no_step || (((uintptr_t)a.p & 15u) == al && ((uintptr_t)a.m & 15u) == al && ((uintptr_t)a.v & 15u) == al);
  if (!same) {                                    /* no common 16-byte phase: scalar, still coalesced */
    for (int64_t i = (int64_t)blockIdx.x * OPTIM_THREADS + tid; i < a.n; i += (int64_t)gridDim.x * OPTIM_THREADS) {
      float p = 0.0f, g = a.g[i], m = 0.0f, v = 0.0f;
      if (!a.no_step) { p = a.p[i]; m = a.m[i]; v = a.v[i]; }
      optim_adam_element(a, coef, p, g, m, v);
      if (!a.no_step) { a.p[i] = p; a.m[i] = m; a.v[i] = v; }
      if (a.write_grad) a.g[i] = g;
    }
    return;
  }
  int head = (int)(((16u - al) & 15u) >> 2);
  if (head > a.n) head = a.n;
  const int nvec = (a.n - head) >> 2, tail = a.n - head - 4 * nvec;
  if (blockIdx.x == 0 && tid < 128) {             /* threads 0..2: the head; threads 64..66: the tail */
    int i = -1;
    if (tid < head) i = tid;
    else if (tid >= 64 && tid - 64 < tail) i = head + 4 * nvec + (tid - 64);
    if (i >= 0) {
      float p = 0.0f, g = a.g[i], m = 0.0f, v = 0.0f;
      if (!a.no_step) { p = a.p[i]; m = a.m[i]; v = a.v[i]; }
      optim_adam_element(a, coef, p, g, m, v);
      if (!a.no_step) { a.p[i] = p; a.m[i] = m; a.v[i] = v; }
      if (a.write_grad) a.g[i] = g;
    }
  }
  float4 *p4 = reinterpret_cast<float4 *>(a.p + head), *g4 = reinterpret_cast<float4 *>(a.g + head);
  float4 *m4 = reinterpret_cast<float4 *>(a.m + head), *v4 = reinterpret_cast<float4 *>(a.v + head);
  for (int i = blockIdx.x * OPTIM_THREADS + tid; i < nvec; i += gridDim.x * OPTIM_THREADS) {
    float4 p = {0.0f, 0.0f, 0.0f, 0.0f}, m = p, v = p, g = g4[i];
    if (!a.no_step) { p = p4[i]; m = m4[i]; v = v4[i]; }
    optim_adam_element(a, coef, p.x, g.x, m.x, v.x);
    optim_adam_element(a, coef, p.y, g.y, m.y, v.y);
    optim_adam_element(a, coef, p.z, g.z, m.z, v.z);
    optim_adam_element(a, coef, p.w, g.w, m.w, v.w);
    if (!a.no_step) { p4[i] = p; m4[i] = m; v4[i] = v; }
    if (a.write_grad) g4[i] = g;
  }
}

}  // namespace rn
