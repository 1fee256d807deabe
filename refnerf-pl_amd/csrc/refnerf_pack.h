/*
 * refnerf_pack.h -- every weight packer of librefnerf_hip.so: canonical blob -> the operand images of refnerf_layout.h (fp32 image
 * and its general-basis tail, the chunked bf16 / f16 / split-f16 images) and of refnerf_sq_layout.h (the training image of the
 * split-f16 mode: its chunk table TR_TABLE and constants block).  Included by refnerf_hip.hip only.  The index maps of the MFMA
 * operand layouts are the named functions of refnerf_layout.h; none of them is written out here.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "refnerf_layout.h"
#include "refnerf_sq_layout.h"

namespace rn {

/* ---------------- canonical blob ---------------- */
/* W[row][k] of GEMM op `op` in canonical storage; k = canonical input column. */
__device__ inline float canon_w(const float *P, int op, int row, int k) {
  if (op < 8) {
    int in = CANON.sp_in[op];
    return (k < in) ? P[CANON.sp_w[op] + row * in + k] : 0.0f;
  }
  if (op == OP_HEADS) {
    if (row < BNECK) return P[CANON.bneck_w + row * WIDTH + k];
    if (row == HROW_DENSITY) return P[CANON.density_w + k];
    if (row < HROW_ROUGH) return P[CANON.gradpred_w + (row - HROW_GRAD) * WIDTH + k];
    if (row == HROW_ROUGH) return P[CANON.rough_w + k];
    if (row < HROW_TINT) return P[CANON.diffuse_w + (row - HROW_DIFFUSE) * WIDTH + k];
    if (row < HROWS) return P[CANON.tint_w + (row - HROW_TINT) * WIDTH + k];
    return 0.0f;
  }
  if (op < OP_RGB) {
    int i = op - 9, in = CANON.vd_in[i];
    return (k < in) ? P[CANON.vd_w[i] + row * in + k] : 0.0f;
  }
  return (row < 3) ? P[CANON.rgb_w + row * WIDTH + k] : 0.0f;
}
__device__ inline float canon_b(const float *P, int op, int row) {
  if (op < 8) return P[CANON.sp_b[op] + row];
  if (op == OP_HEADS) {
    if (row < BNECK) return P[CANON.bneck_b + row];
    if (row == HROW_DENSITY) return P[CANON.density_b];
    if (row < HROW_ROUGH) return P[CANON.gradpred_b + row - HROW_GRAD];
    if (row == HROW_ROUGH) return P[CANON.rough_b];
    if (row < HROW_TINT) return P[CANON.diffuse_b + row - HROW_DIFFUSE];
    if (row < HROWS) return P[CANON.tint_b + row - HROW_TINT];
    return 0.0f;
  }
  if (op < OP_RGB) return P[CANON.vd_b[op - 9] + row];
  return (row < 3) ? P[CANON.rgb_b + row] : 0.0f;
}

/* ---------------- 17 KB chunks: [1 KB bias piece][16 fragment pieces of 1 KB], one workgroup per chunk ---------------- */
/* how a plain chunk stores a value: as bf16 or f16, or as the hi / lo half of its split-f16 pair */
template <typename E> struct StoreAs { __device__ E operator()(float v) const { return (E)v; } };
struct StoreF16Part { int part; __device__ _Float16 operator()(float v) const { return f16_part(v, part); } };

/* bias piece: fp32 bias(e) for e < 32, rest of the KB zero */
template <typename F>
__device__ inline void fill_bias_piece(char *__restrict__ chunk, F &&bias) {
  for (int e = threadIdx.x; e < 256; e += blockDim.x) reinterpret_cast<float *>(chunk)[e] = (e < 32) ? bias(e) : 0.0f;
}
/* fragment pieces 0 .. n - 1: element e of lane `lane` of piece t = value(t, lane, e) */
template <typename E, typename F>
__device__ inline void fill_pieces(char *__restrict__ chunk, int n, F &&value) {
  for (int idx = threadIdx.x; idx < n * 512; idx += blockDim.x) reinterpret_cast<E *>(chunk + 1024)[idx] = value(idx >> 9, (idx >> 3) & 63, idx & 7);
}

/* One plain chunk of `kind` BF_* (refnerf_layout.h, bf16 MFMA operand image) of slice ob of forward op `op`; `first`: it opens the
 * slice and carries the bias in accumulator layout [h][16]; base: canonical column of the first non-register input */
template <typename S>
__device__ inline void fill_chunk_plain(const float *__restrict__ P, char *__restrict__ chunk, int op, int ob, int kind, bool first, int base, S store) {
  fill_bias_piece(chunk, [&](int e) { return first ? canon_b(P, op, acc_row(e & 15, e >> 4, ob * 32)) : 0.0f; });
  fill_pieces<decltype(store(0.0f))>(chunk, 16, [&](int t, int lane, int e) {
    const int h = lane >> 5, row = ob * 32 + (lane & 31);
    float v = 0.0f;
    if (kind == BF_REG) v = canon_w(P, op, row, kslot16(t, h, e));
    else if (kind == BF_BNLDS && t < 8) v = canon_w(P, op, row, base + kslot16(t, h, e));
    else if (kind == BF_LDS8) {                  /* LDS order = canonical IPE order */
      if (t < BF_IPE_REAL_KS) v = canon_w(P, op, row, base + klds16(t, h, e));
    } else {
      const int col = dir_lds_col(klds16(t - 8, h, e));
      if (col >= 0) v = canon_w(P, op, row, base + col);
    }
    return store(v);
  });
}
/* One plain TRANSPOSED chunk (backward): A[row = col0 + 32 ob + lane % 32][k] = W[k][row] of forward op `op`, no bias;
 * REG: k = the 256 outputs of the layer in register-step order; HEADS (kind BF_BNLDS): k = head rows, 0..127 in register-step
 * order, then 128 + k' (k' < 11) from the LDS tile */
__device__ inline void fill_chunk_plain_t(const float *__restrict__ P, char *__restrict__ chunk, int op, int col0, int ob, int kind, StoreF16Part store) {
  fill_bias_piece(chunk, [](int) { return 0.0f; });
  fill_pieces<_Float16>(chunk, 16, [&](int t, int lane, int e) {
    const int h = lane >> 5, row = col0 + ob * 32 + (lane & 31);
    if (kind == BF_REG || t < 8) return store(canon_w(P, op, kslot16(t, h, e), row));
    const int kp = klds16(t - 8, h, e);
    return store(kp < HROWS - BNECK ? canon_w(P, op, BNECK + kp, row) : 0.0f);
  });
}
/* ... and a plain BNLDS chunk whose eight bottleneck k-steps follow the merged-run order of the split image: the two runs'
 * k-blocks b of slice t / 2 side by side, k-block 2 h + t % 2 */
__device__ inline void fill_chunk_bnlds_sq(const float *__restrict__ P, char *__restrict__ chunk, int op, int ob, bool first, int base) {
  fill_chunk_plain(P, chunk, op, ob, BF_BNLDS, first, base, StoreAs<_Float16>{});
  __syncthreads();
  fill_pieces<_Float16>(chunk, 8, [&](int t, int lane, int e) {
    return (_Float16)canon_w(P, op, ob * 32 + (lane & 31), base + kcol_sq(t >> 1, 2 * (lane >> 5) + (t & 1), e));
  });
}

/* One chunk of `kind` SQ_* of the 16x16x32 sections (refnerf_layout.h, split-f16 operand image; w = hi + lo): slice ob of forward
 * op `op`, piece lane (bk, r16) = 8 halves W[16 T + r16][k-block bk]; bias piece [T][b][4] = the slice's rows in plain order */
__device__ inline void fill_chunk_sq(const float *__restrict__ P, char *__restrict__ chunk, int op, int ob, int kind, bool first, int base) {
  fill_bias_piece(chunk, [&](int e) { return first ? canon_b(P, op, ob * 32 + e) : 0.0f; });
  fill_pieces<_Float16>(chunk, 16, [&](int pi, int lane, int e) {
    const int bk = lane >> 4, r16 = lane & 15;
    int T = pi & 1, part, col;
    bool live = true;
    if (kind == SQ_BN) { part = 0; col = kcol_sq(pi >> 1, bk, e); }                      /* [WhT0 WhT1] x 8 */
    else if (kind == SQ_SC) { T = 0; part = pi & 1; col = kcol_sq(pi >> 1, bk, e); }     /* tile T0 only: [WhT0 WlT0] x 8 */
    else {                                                                               /* [WhT0 WhT1 WlT0 WlT1] x 4 */
      const int sl = pi >> 2;
      part = (pi >> 1) & 1;
      if (kind == SQ_X) { live = sl < 3; col = base + 32 * sl + 8 * bk + e; }            /* LDS planes: k' = 32 s + 8 b + i */
      else col = kcol_sq((kind == SQ_B ? 4 : 0) + sl, bk, e);
    }
    return f16_part(live ? canon_w(P, op, ob * 32 + 16 * T + r16, col) : 0.0f, part);
  });
}
/* One transposed SQ_A / SQ_B chunk (the VJP): A[row = input feature col0 + 32 ob + 16 T + r16][k] = W[k][row] of forward op `op`,
 * k in the k-step order of the forward's spatial chunks, no bias */
__device__ inline void fill_chunk_sqt(const float *__restrict__ P, char *__restrict__ chunk, int op, int col0, int ob, int kind) {
  fill_bias_piece(chunk, [](int) { return 0.0f; });
  fill_pieces<_Float16>(chunk, 16, [&](int pi, int lane, int e) {
    const int T = pi & 1, part = (pi >> 1) & 1, st = (kind == SQ_B ? 4 : 0) + (pi >> 2);
    return f16_part(canon_w(P, op, kcol_sq(st, lane >> 4, e), col0 + ob * 32 + 16 * T + (lane & 15)), part);
  });
}

/* bf16 / f16 image: one block per (op, ob) slice, uniform chunks in execution order */
template <typename E>   /* E = __bf16 (REFNERF_PREC_BF16) or _Float16 (REFNERF_PREC_F16): same image layout */
__global__ void pack_weights_16(const float *__restrict__ P, char *__restrict__ out) {
  const int op = blockIdx.y, ob = blockIdx.x;
  const BfOp o = BFPACKED.op[op];
  if (ob >= o.nob) return;
  const int base = (o.nchunk == 2) ? WIDTH : 0;
  for (int j = 0; j < o.nchunk; ++j)
    fill_chunk_plain(P, out + (size_t)(o.chunk0 + ob * o.nchunk + j) * BF_CHUNK_BYTES, op, ob, o.kind[j], j == 0, base, StoreAs<E>{});
}
/* split-f16 image (REFNERF_PREC_F16X2): spatial ops and heads as SQ_* chunks, the directional ops as plain f16 chunks */
__global__ void pack_weights_split(const float *__restrict__ P, char *__restrict__ out) {
  const int op = blockIdx.y, ob = blockIdx.x;
  const int nob = (op == OP_HEADS) ? 5 : (op == OP_RGB ? 1 : 8);
  if (ob >= nob) return;
  int c = SPPACKED.chunk0[op];
  for (int o2 = 0; o2 < ob; ++o2) c += sp_slice_chunks(op, o2);
  char *chunk = out + (size_t)c * BF_CHUNK_BYTES;
  if (op > OP_HEADS) {
    const BfOp o = BFPACKED.op[op];
    const int base = (o.nchunk == 2) ? WIDTH : 0;
    for (int j = 0; j < o.nchunk; ++j) {
      if (o.kind[j] == BF_BNLDS) fill_chunk_bnlds_sq(P, chunk + (size_t)j * BF_CHUNK_BYTES, op, ob, j == 0, base);
      else fill_chunk_plain(P, chunk + (size_t)j * BF_CHUNK_BYTES, op, ob, o.kind[j], j == 0, base, StoreAs<_Float16>{});
    }
    return;
  }
  const int n = sp_slice_chunks(op, ob);
  if (op == OP_HEADS) { fill_chunk_sq(P, chunk, op, ob, ob < 4 ? SQ_BN : SQ_SC, true, 0); return; }
  for (int j = 0; j < n; ++j)
    fill_chunk_sq(P, chunk + (size_t)j * BF_CHUNK_BYTES, op, ob, sq_sp_kind(op, j), j == 0, op == 5 ? WIDTH : 0);
}
/* training image of the split-f16 mode: grid = TR_CHUNKS blocks of 256 threads, block c fills chunk c as TR_TABLE says */
__global__ void pack_train_chunks(const float *__restrict__ P, char *__restrict__ out) {
  const TrChunk t = TR_TABLE.c[blockIdx.x];
  char *chunk = out + (size_t)blockIdx.x * BF_CHUNK_BYTES;
  switch (t.fill) {
    case TRF_SQ: fill_chunk_sq(P, chunk, t.op, t.ob, t.kind, t.first, t.col); break;
    case TRF_SQT: fill_chunk_sqt(P, chunk, t.op, t.col, t.ob, t.kind); break;
    case TRF_PLAIN: fill_chunk_plain(P, chunk, t.op, t.ob, t.kind, t.first, t.col, StoreF16Part{t.part}); break;
    default: fill_chunk_plain_t(P, chunk, t.op, t.col, t.ob, t.kind, StoreF16Part{t.part}); break;
  }
}

/* the constants block: W_density, W_rgb, and per transposed op G = max over its output rows f of sum_o |W[o][f]|;
 * grid = TRG_N blocks of 1024 threads: thread (f, rg) sums rows o = rg (mod 4) of column f with four loads in flight
 * (one thread per column walking 256 rows one dependent load at a time took 88 us of every training step; now 27) */
__global__ __launch_bounds__(1024) void pack_train_consts(const float *__restrict__ P, float *__restrict__ K) {
  __shared__ float red[1024];
  const int g = blockIdx.x, f = threadIdx.x & 255, rg = threadIdx.x >> 8;
  const TrG t = TRG_TABLE.g[g];
  const int op = t.op, rows = t.rows, col0 = t.col0, ncol = t.ncol;
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (op >= 0 && f < ncol) {
    for (int o0 = rg; o0 < rows; o0 += 16) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int o = o0 + 4 * u;
        if (o < rows) s[u] += fabsf(canon_w(P, op, g == TRG_WD ? HROW_DENSITY : o, col0 + f));
      }
    }
  }
  red[threadIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  if (rg == 0) red[f] = (red[f] + red[f + 256]) + (red[f + 512] + red[f + 768]);
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) K[TRC_G + g] = red[0];
  if (g == 0 && rg == 0) {
    K[TRC_WD + f] = canon_w(P, OP_HEADS, HROW_DENSITY, f);
    for (int c = 0; c < 3; ++c) K[TRC_WRGB + c * WIDTH + f] = canon_w(P, OP_RGB, c, f);
    if (f < TRC_WRGB - TRC_G - TRG_N) K[TRC_G + TRG_N + f] = 0.0f;
  }
}

/* ---------------- fp32 image ---------------- */
/* element e of an fp32 A image -> (k-step, row block, lane): [step][lane][ob], eight-block ops [step][q][lane][4] with ob = 4 q + e % 4 */
__device__ __forceinline__ void a_decode(int e, int stride, int &step, int &ob, int &lane) {
  step = e / (stride * 64);
  if (stride == 8) { const int rem = e % 512; ob = (rem >> 8) * 4 + (rem & 3); lane = (rem & 255) >> 2; }
  else { ob = e % stride; lane = (e / stride) % 64; }
}

/* ---- the 16-bit images of the chain GEMMs: [k-step][ob][lane][8], element e of lane (h = lane / 32, n = lane % 32) ---- */
/* transposed op t (bt_off / ht_off): W[o = k slot][in_row = 32 ob + n] */
__device__ __forceinline__ float top16_value(const float *__restrict__ P, int t, int st, int ob, int lane, int e) {
  const Op o = PACKED.top[t];
  const int h = lane >> 5, in_row = ob * 32 + (lane & 31);
  if (ob >= o.nob) return 0.0f;
  if (t == TOP_HEADS) {
    const int hr = klds16(st, h, e);                         /* head row feeding this k slot */
    return (hr < HROWS) ? canon_w(P, OP_HEADS, hr, in_row) : 0.0f;
  }
  const TopSrc src = PACKED.top_src[t];
  const int n_rows = (o.nob == 8) ? WIDTH : (o.nob == 3 ? IPE_DIM : DIR_IN);   /* rows beyond are padding */
  return (in_row < n_rows) ? canon_w(P, src.fwd_op, kslot16(st, h, e), src.col0 + in_row) : 0.0f;
}
/* forward op fo (bf_off / hf_off): W[row = 32 ob + n][k], register steps in k-slot order, then the LDS steps in plain order */
__device__ __forceinline__ float fwd16_value(const float *__restrict__ P, int fo, int st, int ob, int lane, int e) {
  const int rst = bf_reg_steps(fo);
  const int h = lane >> 5, row = ob * 32 + (lane & 31);
  if (ob >= PACKED.op[fo].nob) return 0.0f;
  if (st < rst) return canon_w(P, fo, row, kslot16(st, h, e));
  const int kl = klds16(st - rst, h, e);
  const int valid_k = (fo == 0 || fo == 5) ? IPE_DIM : DIR_IN;
  return (kl < valid_k) ? canon_w(P, fo, row, (rst ? WIDTH : 0) + kl) : 0.0f;
}
/* the two stores: bf16, or the split-f16 pair -- per k-step [hi | lo], the lo half 4096 halves behind its hi half */
__device__ __forceinline__ void store16(__bf16 *dst, int idx, float v) { dst[idx] = (__bf16)v; }
__device__ __forceinline__ void store16(_Float16 *dst, int idx, float v) {
  const size_t base = (size_t)(idx >> 12) * (2 * 4096) + (idx & 4095);
  dst[base] = f16_part(v, 0);
  dst[base + 4096] = f16_part(v, 1);
}
/* one image of `steps` k-steps, value(st, ob, lane, e), by the whole x-grid */
template <typename E, typename F>
__device__ __forceinline__ void pack_image16(E *dst, int steps, F &&value) {
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < steps * 4096; idx += gridDim.x * blockDim.x)
    store16(dst, idx, value(idx >> 12, (idx >> 9) & 7, (idx >> 3) & 63, idx & 7));
}

__global__ void pack_weights_f32(const float *__restrict__ P, float *__restrict__ out) {
  int op = blockIdx.y;
  if (op < NUM_OPS) {
    const Op o = PACKED.op[op];
    int n_a = (o.reg_steps + o.lds_steps) * 64 * o.stride;
    int n_b = o.nob * 32;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n_a + n_b; e += gridDim.x * blockDim.x) {
      if (e < n_a) {
        int step, ob, lane;
        a_decode(e, o.stride, step, ob, lane);
        int h = lane >> 5, row = ob * 32 + (lane & 31);
        float v = 0.0f;
        if (ob < o.nob) {
          if (step < o.reg_steps) {
            v = canon_w(P, op, row, kslot2(step, h));
          } else {
            int kl = 2 * (step - o.reg_steps) + h;
            int valid_k = (op == 0 || op == 5) ? IPE_DIM : DIR_IN;
            v = (kl < valid_k) ? canon_w(P, op, row, (o.reg_steps ? WIDTH : 0) + kl) : 0.0f;
          }
        }
        out[o.a_off + e] = v;
      } else {
        int b = e - n_a;                                       /* bias image in accumulator layout [ob][h][16] */
        int reg = b & 15, h = (b >> 4) & 1, ob = b >> 5;
        out[o.b_off + b] = canon_b(P, op, acc_row(reg, h, ob * 32));
      }
    }
  } else if (op < NUM_OPS + NUM_TOPS) {
    /* transposed ops: A[step][lane][ob] = W[o = k slot][in_row] (see refnerf_layout.h) */
    const int t = op - NUM_OPS;
    const Op o = PACKED.top[t];
    const TopSrc src = PACKED.top_src[t];
    int n_a = (o.reg_steps + o.lds_steps) * 64 * o.stride;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n_a; e += gridDim.x * blockDim.x) {
      int step, ob, lane;
      a_decode(e, o.stride, step, ob, lane);
      int h = lane >> 5, in_row = ob * 32 + (lane & 31);
      float v = 0.0f;
      if (ob < o.nob) {
        if (t == TOP_HEADS) {
          int hr = 2 * step + h;                               /* head row feeding this k slot */
          v = (hr < HROWS) ? canon_w(P, OP_HEADS, hr, in_row) : 0.0f;
        } else {
          v = canon_w(P, src.fwd_op, kslot2(step, h) /* output feature feeding this k slot */, src.col0 + in_row);
        }
      }
      out[o.a_off + e] = v;
    }
  } else if (op < 3 * NUM_OPS + 3 * NUM_TOPS) {
    /* the 16-bit images, in blob order: bf16 transposed (bt_off: the bf16-chain backward), bf16 forward (bf_off: the bf16-chain
     * training forward), split-f16 transposed (ht_off), split-f16 forward (hf_off) */
    const int j = op - NUM_OPS - NUM_TOPS, half = NUM_TOPS + NUM_OPS;
    const bool split = j >= half;
    const int i = split ? j - half : j;                     /* transposed op i, or forward op i - NUM_TOPS */
    if (i < NUM_TOPS) {
      const int t = i, steps = (t == TOP_HEADS) ? BT_HEADS_STEPS : BT_CHAIN_STEPS;
      auto value = [&](int st, int ob, int lane, int e) { return top16_value(P, t, st, ob, lane, e); };
      if (split) pack_image16(reinterpret_cast<_Float16 *>(out + PACKED.ht_off[t]), steps, value);
      else pack_image16(reinterpret_cast<__bf16 *>(out + PACKED.bt_off[t]), steps, value);
    } else {
      const int fo = i - NUM_TOPS, steps = bf_reg_steps(fo) + bf_lds_steps(fo);
      auto value = [&](int st, int ob, int lane, int e) { return fwd16_value(P, fo, st, ob, lane, e); };
      if (split) pack_image16(reinterpret_cast<_Float16 *>(out + PACKED.hf_off[fo]), steps, value);
      else pack_image16(reinterpret_cast<__bf16 *>(out + PACKED.bf_off[fo]), steps, value);
    }
  } else {
    /* WD / WRGB: raw_density.weight and rgb_layer.weight rows in accumulator layout [ob][h][16] */
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < 4 * 8 * 32; b += gridDim.x * blockDim.x) {
      int reg = b & 15, h = (b >> 4) & 1, ob = (b >> 5) & 7, which = b >> 8;
      int k = acc_row(reg, h, ob * 32);
      if (which == 0) out[PACKED.wd_off + (b & 255)] = P[CANON.density_w + k];
      else out[PACKED.wrgb_off + (which - 1) * 256 + (b & 255)] = P[CANON.rgb_w + (which - 1) * WIDTH + k];
    }
  }
}

/* Tail of the fp32 image for a general IPE basis (refnerf_layout.h): the basis directions, the forward group ops
 * (op 0's LDS-step format: A[step][q][lane][4] = W[32 ob + lane % 32][k = 2 step + h]) and their transposes (TOP_SP0's
 * format: A[step][lane][4] = W[o(step, h)][in_row = 32 ob + lane % 32], ob < 3) of the tail weights. */
__global__ void pack_weights_ext(const float *__restrict__ P, const float *__restrict__ basis, int groups, float *__restrict__ out) {
  const int e0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const int which = blockIdx.y;              /* 0: basis, then 12 blocks each: fp32 forward, fp32 transposed, split forward, split transposed */
  if (which == 0) {
    for (int e = e0; e < 64; e += stride) out[PEXT_BASIS + e] = (e < 9 * groups) ? basis[e] : 0.0f;
    return;
  }
  const int idx = (which - 1) % (2 * EXT_GROUPS), L = idx / EXT_GROUPS, g = idx % EXT_GROUPS + 1;
  const float *W = P + ext_w_off(L, g);      /* [256 rows, pitch EXT_K][96] */
  const bool live = g < groups;
  const int kind = (which - 1) / (2 * EXT_GROUPS);   /* 0: fp32 forward, 1: fp32 transposed, 2: split forward, 3: split transposed */
  if (kind == 0) {
    float *dst = out + pext_fwd_off(L, g);
    for (int e = e0; e < PEXT_FWD_FLOATS; e += stride) {
      const int step = e >> 9, rem = e & 511, ob = (rem >> 8) * 4 + (rem & 3), lane = (rem & 255) >> 2;
      const int h = lane >> 5, row = ob * 32 + (lane & 31), k = 2 * step + h;
      dst[e] = live ? W[row * EXT_K + k] : 0.0f;
    }
  } else if (kind == 1) {
    float *dst = out + pext_t_off(L, g);
    for (int e = e0; e < PEXT_T_FLOATS; e += stride) {
      const int ob = e & 3, lane = (e >> 2) & 63, step = e >> 8;
      const int h = lane >> 5, in_row = ob * 32 + (lane & 31);
      dst[e] = (live && ob < 3) ? W[kslot2(step, h) * EXT_K + in_row] : 0.0f;
    }
  } else {
    /* split copies: the [k-step][hi | lo][ob][lane][8] layout of ht_off / hf_off */
    const bool fwd = kind == 2;
    _Float16 *dst = reinterpret_cast<_Float16 *>(out + (fwd ? pext_hf_off(L, g) : pext_ht_off(L, g)));
    pack_image16(dst, fwd ? BF_IPE_STEPS : BT_CHAIN_STEPS, [&](int st, int ob, int lane, int e) {
      const int h = lane >> 5, r32 = ob * 32 + (lane & 31);
      if (!live) return 0.0f;
      if (fwd) return W[r32 * EXT_K + klds16(st, h, e)];   /* plain order over the fp32 X tile (bf_off's LDS steps) */
      return ob < 3 ? W[kslot16(st, h, e) * EXT_K + r32] : 0.0f;
    });
  }
}

}  // namespace rn
