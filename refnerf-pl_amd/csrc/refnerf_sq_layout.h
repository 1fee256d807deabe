/*
 * refnerf_sq_layout.h -- layouts of the round-5 training path of the parity-grade 16-bit mode (REFNERF_PREC_F16X2 on the
 * built-in IPE basis): the training forward and the backward run on the EVAL kernel's skeleton (8 waves, two per SIMD, weights
 * through the LDS-DMA chunk ring of refnerf_level_bf16.h, 0 B of scratch) instead of the one-wave-per-SIMD fp32 skeleton.
 *
 * Arithmetic (scripts/exp_train_sq_precision.py: the reference's autograd with these roundings emulated, three trained sets):
 *   forward   spatial trunk + ALL head rows : W and x as hi + lo halves, three products (the eval kernel's; the bottleneck now
 *                                             takes its W_lo product too: LLFF gradient 1.5e-4 -> 6.5e-5)
 *             directional trunk + rgb       : W as hi + lo, x as ONE half: two products [W_hi | W_lo] x (what matters is the
 *                                             coherent rounding of W, not the per-sample rounding of x: W11 x X11 3.8e-4,
 *                                             W22 x X11 1.7e-4 = the all-22-bit figure)
 *   VJP       density-gradient normals      : three products (the normals are an output)
 *   backward  every transposed layer        : W^T as hi + lo, delta as ONE half after its per-sample power-of-two factor: two
 *                                             products (gradient rel-L2 unchanged within the sets' spread)
 *   dW        ACT spatial hi + lo (pair units), ACT directional ONE half (it IS what the forward multiplied), DELTA one half.
 *
 * (1) the weight image (REFNERF_IMAGE_F16X2_TRAIN): 17 KB chunks in execution order, forward stream then backward stream;
 * (2) the ACT format REFNERF_ACT_SQ and the DELTA format (factor rows doubled);
 * (3) the job table of the weight-gradient GEMM on them.
 */
#pragma once
#include "refnerf_layout.h"

namespace rn {

/* ---------------- (1) weight image ----------------
 * FORWARD stream of a pass = [run section] x 2 (16 samples per wave each) + [directional section] (32 samples per wave):
 *   run section  : spatial ops 0..7 exactly as the eval image (SQ_X / SQ_A / SQ_B chunks, 128 chunks)
 *                  heads: 4 bottleneck slices as [SQ_A SQ_B] (hi + lo weights) + the scalar block [SQ_SC]            9
 *                  VJP  : transposed spatial layers 7..1 (8 slices x [SQ_A SQ_B]); in front of layer 5 the 96 IPE rows of layer 5
 *                         (3 slices), behind layer 1 those of layer 0 (3 slices)                                  124
 *   directional  : ops 9..16 + rgb as plain f16 chunks of refnerf_layout.h, every chunk twice: [hi][lo]              146
 * BACKWARD stream of a pass (32 samples per wave, two products): plain chunks [hi][lo] of the transposed ops
 *   directional layers 7..1 (8 slices x [REG REG])                                                                112
 *   the 204 dir-input rows: 7 slices x [layer 5's part hi lo | layer 0's part hi lo]                                28
 *   heads^T: 8 slices x [BNLDS hi lo] (K = 128 bottleneck rows from registers + the 11 scalar rows from LDS)         16
 *   spatial layers 7..1                                                                                           112
 * then a constants block (fp32): W_density[256], the column-sum bounds G of every transposed op, W_rgb[3][256]. */
constexpr int TR_SP_TRUNK = 128, TR_HEADS = 9, TR_VJP = 124;
constexpr int TR_RUN = TR_SP_TRUNK + TR_HEADS + TR_VJP;       /* 261 */
constexpr int TR_DIR = 146;
constexpr int TR_FWD = TR_RUN + TR_DIR;                       /* 407 chunks stored  */
constexpr int TR_FWD_PASS = 2 * TR_RUN + TR_DIR;              /* 668 chunks streamed per pass */
constexpr int TR_BWD_DIR = 112, TR_BWD_DIN = 28, TR_BWD_HEADS = 16, TR_BWD_SP = 112;
constexpr int TR_BWD = TR_BWD_DIR + TR_BWD_DIN + TR_BWD_HEADS + TR_BWD_SP;   /* 268 */
constexpr int TR_BWD0 = TR_FWD;
constexpr int TR_CHUNKS = TR_FWD + TR_BWD;                    /* 675 */
static_assert(SPPACKED.chunk0[OP_HEADS] == TR_SP_TRUNK, "the spatial trunk of the eval image");
/* constants block behind the chunks (+ 2 chunks of pad: the DMA never runs past the end, the fragment ring reads one piece ahead) */
constexpr size_t TR_CONST_OFF = (size_t)(TR_CHUNKS + 2) * BF_CHUNK_BYTES;
constexpr int TRC_WD = 0;                  /* raw_density.weight[256]                                   */
constexpr int TRC_G = 256;                 /* G of the transposed ops, indexed by TRG_*                 */
constexpr int TRC_WRGB = 320;              /* rgb_layer.weight[3][256]                                  */
constexpr int TRC_FLOATS = TRC_WRGB + 3 * WIDTH;
constexpr size_t TR_IMAGE_BYTES = TR_CONST_OFF + (size_t)TRC_FLOATS * 4;
/* G[op] = max over the op's output rows (= the layer's input features f) of sum_o |W[o][f]|: |W^T delta|_inf <= G |delta|_inf,
 * so a sample's deltas can be rescaled BEFORE the contraction without ever leaving the range of an IEEE half */
enum { TRG_SP = 0 /* + layer 1..7 */, TRG_SP5_IPE = 8, TRG_SP0 = 9, TRG_VD = 10 /* + layer 1..7 */, TRG_VD5_DIN = 18, TRG_VD0 = 19,
       TRG_HEADS = 20, TRG_RGB = 21, TRG_WD = 22, TRG_N = 23 };
/* what G[g] sums: `rows` output rows of forward op `op`, max over its input columns col0 .. col0 + ncol (op < 0: slot unused) */
struct TrG { short op, rows, col0, ncol; };
struct TrGTable { TrG g[TRG_N]; };
constexpr TrGTable make_trg_table() {
  TrGTable t{};
  for (int g = 0; g < TRG_N; ++g) t.g[g] = TrG{-1, WIDTH, 0, WIDTH};
  for (int l = 1; l <= 7; ++l) { t.g[TRG_SP + l].op = (short)l; t.g[TRG_VD + l].op = (short)(9 + l); }
  t.g[TRG_SP5_IPE] = TrG{5, WIDTH, WIDTH, IPE_DIM};
  t.g[TRG_SP0] = TrG{0, WIDTH, 0, IPE_DIM};
  t.g[TRG_VD5_DIN] = TrG{14, WIDTH, WIDTH, DIR_IN};
  t.g[TRG_VD0] = TrG{9, WIDTH, 0, DIR_IN};
  t.g[TRG_HEADS] = TrG{OP_HEADS, HROWS, 0, WIDTH};
  t.g[TRG_RGB] = TrG{OP_RGB, 3, 0, WIDTH};
  t.g[TRG_WD] = TrG{OP_HEADS, 1, 0, WIDTH};       /* the one row HROW_DENSITY */
  return t;
}
constexpr TrGTable TRG_TABLE = make_trg_table();

/* The chunk order above as a table: entry c says how chunk c of the image is filled (refnerf_pack.h).
 *   TRF_SQ      forward 16x16x32 chunk of `kind` SQ_*: slice ob of op, input columns from `col`; `first`: it carries the bias
 *   TRF_SQT     its transpose (the VJP): rows col + 32 ob .. of op's inputs, k-steps of kind SQ_A / SQ_B
 *   TRF_PLAIN   forward plain chunk of `kind` BF_*, half `part` of every weight; LDS-fed columns from `col`
 *   TRF_PLAIN_T its transpose (the backward): rows col + 32 ob .. of op's inputs, half `part` */
enum { TRF_SQ = 0, TRF_SQT = 1, TRF_PLAIN = 2, TRF_PLAIN_T = 3 };
struct TrChunk { unsigned char fill, op, ob, kind, part, first; unsigned short col; };
struct TrTable { TrChunk c[TR_CHUNKS]; int n; int seg[7]; };
constexpr void tr_put(TrTable &t, int fill, int op, int ob, int col, int kind, int part, bool first) {
  if (t.n < TR_CHUNKS)
    t.c[t.n] = TrChunk{(unsigned char)fill, (unsigned char)op, (unsigned char)ob, (unsigned char)kind, (unsigned char)part, (unsigned char)first, (unsigned short)col};
  ++t.n;
}
constexpr void tr_put_sqt(TrTable &t, int op, int col0, int slices) {               /* slices x [SQ_A SQ_B] */
  for (int ob = 0; ob < slices; ++ob)
    for (int j = 0; j < 2; ++j) tr_put(t, TRF_SQT, op, ob, col0, j ? SQ_B : SQ_A, 0, false);
}
constexpr void tr_put_plain_t(TrTable &t, int op, int col0, int slices, int kind) {  /* slices x [hi lo] */
  for (int ob = 0; ob < slices; ++ob)
    for (int part = 0; part < 2; ++part) tr_put(t, TRF_PLAIN_T, op, ob, col0, kind, part, false);
}
constexpr TrTable make_tr_table() {
  TrTable t{};
  /* run section: spatial ops 0..7 exactly as the eval image */
  for (int op = 0; op < OP_HEADS; ++op)
    for (int ob = 0; ob < 8; ++ob)
      for (int j = 0; j < sp_slice_chunks(op, ob); ++j) tr_put(t, TRF_SQ, op, ob, op == 5 ? WIDTH : 0, sq_sp_kind(op, j), 0, j == 0);
  t.seg[0] = t.n;
  /* heads: 4 bottleneck slices as [SQ_A SQ_B] + the scalar block [SQ_SC] */
  for (int ob = 0; ob < 4; ++ob)
    for (int j = 0; j < 2; ++j) tr_put(t, TRF_SQ, OP_HEADS, ob, 0, j ? SQ_B : SQ_A, 0, j == 0);
  tr_put(t, TRF_SQ, OP_HEADS, 4, 0, SQ_SC, 0, true);
  t.seg[1] = t.n;
  /* VJP: transposed spatial layers 7..1, the 96 IPE rows of layer 5 in front of layer 5, those of layer 0 at the end */
  for (int l = 7; l >= 1; --l) {
    if (l == 5) tr_put_sqt(t, 5, WIDTH, IPE_DIM / 32);
    tr_put_sqt(t, l, 0, 8);
  }
  tr_put_sqt(t, 0, 0, IPE_DIM / 32);
  t.seg[2] = t.n;
  /* directional: ops 9..16 + rgb as the plain chunks of refnerf_layout.h, every chunk twice: [hi][lo] */
  for (int op = OP_HEADS + 1; op < NUM_OPS; ++op)
    for (int ob = 0; ob < BFPACKED.op[op].nob; ++ob)
      for (int j = 0; j < BFPACKED.op[op].nchunk; ++j)
        for (int part = 0; part < 2; ++part)
          tr_put(t, TRF_PLAIN, op, ob, BFPACKED.op[op].nchunk == 2 ? WIDTH : 0, BFPACKED.op[op].kind[j], part, j == 0 && part == 0);
  t.seg[3] = t.n;
  /* backward: directional layers 7..1 */
  for (int l = 7; l >= 1; --l) tr_put_plain_t(t, 9 + l, 0, 8, BF_REG);
  t.seg[4] = t.n;
  /* the 204 dir-input rows: 7 slices x [layer 5's part hi lo | layer 0's part hi lo] */
  for (int ob = 0; ob < DIN_BLOCKS; ++ob)
    for (int j = 0; j < 4; ++j) tr_put(t, TRF_PLAIN_T, j < 2 ? 14 : 9, ob, j < 2 ? WIDTH : 0, BF_REG, j & 1, false);
  t.seg[5] = t.n;
  /* heads^T: 8 slices x [BNLDS hi lo] */
  tr_put_plain_t(t, OP_HEADS, 0, 8, BF_BNLDS);
  t.seg[6] = t.n;
  /* spatial layers 7..1 */
  for (int l = 7; l >= 1; --l) tr_put_plain_t(t, l, 0, 8, BF_REG);
  return t;
}
constexpr TrTable TR_TABLE = make_tr_table();
static_assert(TR_TABLE.n == TR_CHUNKS, "the table fills every chunk of the image");
static_assert(TR_TABLE.seg[0] == TR_SP_TRUNK && TR_TABLE.seg[1] == TR_SP_TRUNK + TR_HEADS && TR_TABLE.seg[2] == TR_RUN && TR_TABLE.seg[3] == TR_FWD &&
              TR_TABLE.seg[4] == TR_BWD0 + TR_BWD_DIR && TR_TABLE.seg[5] == TR_BWD0 + TR_BWD_DIR + TR_BWD_DIN &&
              TR_TABLE.seg[6] == TR_BWD0 + TR_BWD_DIR + TR_BWD_DIN + TR_BWD_HEADS, "the sections start where the kernels stream them from");
/* the first TR_SP_TRUNK entries, looked up by the eval split image's own chunk index (SPPACKED: what pack_weights_split fills) */
constexpr bool tr_trunk_is_eval_order() {
  for (int op = 0; op < OP_HEADS; ++op) {
    int c = SPPACKED.chunk0[op];
    for (int ob = 0; ob < 8; ++ob)
      for (int j = 0; j < sp_slice_chunks(op, ob); ++j, ++c) {
        const TrChunk e = TR_TABLE.c[c];
        if (c >= TR_SP_TRUNK || e.fill != TRF_SQ || e.op != op || e.ob != ob || e.kind != sq_sp_kind(op, j) || e.first != (j == 0)) return false;
      }
  }
  return true;
}
static_assert(tr_trunk_is_eval_order(), "the spatial trunk of the eval image");

/* ---------------- (2) ACT / DELTA ----------------
 * REFNERF_ACT_SQ: blocked units as every ACT format ([64-sample block][unit][64 samples], one dword per unit and sample):
 *   AQ_IPE  96 units : pair units of the 96 IPE rows (unit 2j = packed hi halves of rows 2j, 2j + 1, unit 2j + 1 their lo halves)
 *   AQ_SP 2048 units : pair units of x0..x7 (the inputs of spatial layers 1..7 and of the heads)
 *   AQ_DIN 102 units : ONE half per element, rows in pairs: [bottleneck 128 | IDE 72 | n.v | 0 0 0]
 *   AQ_VD 1024 units : the same for v0..v7
 *   AQ_MASK 128 units: ReLU sign patterns, lane-local words of the kernels (8 per layer):
 *                      spatial layer l (16-sample tiles: lane (b, n)): unit 8 l + 2 b + j, bit 8 (s % 4) + i of word j = s / 4
 *                        <-> feature 32 s + 16 (i / 4) + 4 b + i % 4;
 *                      directional layer l (32-sample tiles: lane (h, n)): unit 64 + 8 l + 4 h + q, bit 16 (ob % 2) + r of word
 *                        q = ob / 2 <-> feature 32 ob + (r & 3) + 8 (r >> 2) + 4 h
 *   AQ_RAW  16 units : fp32: the 11 raw scalar head rows (HROW_DENSITY..), raw rgb[3]                         13.7 KB / sample */
constexpr int AQ_IPE = 0, AQ_SP = AQ_IPE + IPE_DIM, AQ_DIN = AQ_SP + 8 * WIDTH, AQ_VD = AQ_DIN + DIR_PAD / 2,
              AQ_MASK = AQ_VD + 8 * WIDTH / 2, AQ_RAW = AQ_MASK + 128, AQ_RAW_RGB = AQ_RAW + 11, AQ_UNITS = AQ_RAW + 16 + 1;
static_assert((AQ_UNITS & 1) == 1 && AQ_UNITS <= ACT_ALLOC_ROWS, "odd block stride inside the allocation of the fp32 format");
/* DELTA: the pair-rows of refnerf_layout.h (one half per element, DEL_ROWS / 2 units), then per (layer id, sample) TWO fp32
 * factor units: c (what the stored halves were multiplied by) and kappa = the power of two that would bring the sample's
 * largest |delta| of that layer to [2^14, 2^15) -- the weight-gradient GEMM brings every sample to the layer's smallest kappa */
constexpr int DQ_C = DEL_ROWS / 2, DQ_K = DQ_C + DSC_ROWS, DQ_UNITS = DQ_K + DSC_ROWS + 1;
static_assert((DQ_UNITS & 1) == 1 && DQ_UNITS <= DEL_ALLOC_ROWS, "odd block stride inside the fp32-sized allocation");

}  // namespace rn
