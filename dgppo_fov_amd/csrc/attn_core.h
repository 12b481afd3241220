// The per-receiver attention core shared by the row-block kernels (attn.hip attn_fwd2r / attn_bwd2r) and the fused
// layer forward (gnn_layer.hip): one half-wave per receiving agent, one lane per candidate edge, the sender row x in
// registers.  A forward site reads: gather, pre-transform, head_weights, wsum (xbar_h per head), wsum ([ebar_h |
// sig_h] of all heads); only the sinks -- where a total is stored -- differ.  The backward recomputes the forward's
// pre-transform and must get the same bits (its ReLU gates), so the order of operations is written here once.  The
// fused policy step (policy.hip) uses the pre-transform and the small pieces; its core stays written out (DESIGN.md
// 3.5: through the helpers that kernel is allocated differently and runs 2% slower).  Everything is inlined.
#pragma once
#include "lanes.h"

namespace dgppo {

using lanes::f32x4;

constexpr int kH = 3;      // heads (GraphTransformer num_heads of the reference GNN)
constexpr int kD0 = 8;     // max raw feature width in agent mode
constexpr int kRows = 16;  // rows per workgroup: one 16-row MFMA tile (16 / n whole graphs in the GNN kernels)

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ f32x4 mma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ---- never-receivers' pre-transform relu(x_raw W + b) ---------------------------------------------------------------
// Per output element: the bias first, then += x_raw[k] * W[k][d] for k ascending (fma), then the ReLU.  W rows are
// 32 floats apart.  Both forms below are built from these two steps and nothing else.
__device__ __forceinline__ f32x4 pre_step(f32x4 v, float xk, f32x4 w) {
  v[0] += xk * w[0];
  v[1] += xk * w[1];
  v[2] += xk * w[2];
  v[3] += xk * w[3];
  return v;
}
__device__ __forceinline__ f32x4 pre_relu(f32x4 v) {
  return f32x4{v[0] > 0.0f ? v[0] : 0.0f, v[1] > 0.0f ? v[1] : 0.0f, v[2] > 0.0f ? v[2] : 0.0f, v[3] > 0.0f ? v[3] : 0.0f};
}
// one quad of one node per thread: columns 4q .. 4q + 3 (W, b point at column 4q)
template <int K>
__device__ __forceinline__ f32x4 pre_node(const float* xr, const float* W, const float* b) {
  f32x4 v = *(const f32x4*)b;
#pragma unroll
  for (int k = 0; k < K; ++k) v = pre_step(v, xr[k], *(const f32x4*)(W + k * 32));
  return pre_relu(v);
}
// a lane's whole register row x[DM] from its raw row xr[0 .. K); K = 0 in diagnostic builds
template <int K, int DM, int KA>
__device__ __forceinline__ void pre_row(const float (&xr)[KA], const float* W, const float* b, float (&x)[DM]) {
  f32x4 v[DM / 4];
#pragma unroll
  for (int q = 0; q < DM / 4; ++q) v[q] = *(const f32x4*)(b + 4 * q);
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int q = 0; q < DM / 4; ++q) v[q] = pre_step(v[q], xr[k], *(const f32x4*)(W + k * 32 + 4 * q));
#pragma unroll
  for (int q = 0; q < DM / 4; ++q) {
    v[q] = pre_relu(v[q]);
    x[4 * q] = v[q][0], x[4 * q + 1] = v[q][1], x[4 * q + 2] = v[q][2], x[4 * q + 3] = v[q][3];
  }
}

// ---- attention weights of a lane's candidate ------------------------------------------------------------------------
// aw[h] = softmax over the half-wave's candidates of (qt_h . x + beta_h) * scale; qt: the receiver's row, qt_h at
// h * hs (quads q < TQ), beta_h at NH * hs + h; ok: the candidate exists (else weight 0).  out(h, aw[h]) runs inside
// the head loop: a store loop after it would keep every head's weight live across the reductions.
template <int DM, int NH, class Out>
__device__ __forceinline__ void head_weights(const float (&x)[DM], const float* qt, int hs, int TQ, float scale,
                                             bool ok, float (&aw)[NH], Out out) {
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    float acc = 0.0f;
#pragma unroll
    for (int q = 0; q < DM / 4; ++q)
      if (q < TQ) {
        const f32x4 qq = ((const f32x4*)(qt + hs * h))[q];
        acc += x[4 * q] * qq[0] + x[4 * q + 1] * qq[1] + x[4 * q + 2] * qq[2] + x[4 * q + 3] * qq[3];
      }
    const float lg = ok ? (acc + qt[NH * hs + h]) * scale : -INFINITY;
    const float mx = lanes::max32(lg);
    const float ex = ok ? expf(lg - mx) : 0.0f;
    const float sm = lanes::sum32(ex);
    aw[h] = ok ? ex / sm : 0.0f;
    out(h, aw[h]);
  }
}

// ---- transposed weighted sum ----------------------------------------------------------------------------------------
// The half-wave totals of v[0 .. V) (lanes::treduce32; v is consumed): sink(index, total) runs on the lane that owns
// the index.  on: false for the lanes of a row that stores nothing.
template <int V, class Sink>
__device__ __forceinline__ void wsum(float (&v)[V], Sink sink, bool on = true) {
  int cnt;
  const int base = lanes::treduce32(v, cnt);
#pragma unroll
  for (int j = 0; j < lanes::tr_final<V>(); ++j)
    if (on && j < cnt) sink(base + j, v[j]);
}

// ---- LayerNorm(64) (eps 1e-6) + ReLU in place over the ROWS rows of a [ROWS][PITCH] tile ------------------------------
// 8 lanes per row (threads 0 .. 8 ROWS - 1, whole waves; the others return), flax's mean / E[x^2] - mean^2 form as
// the GEMM epilogue computes it
template <int ROWS, int PITCH>
__device__ __forceinline__ void ln_relu64(float* Y, const float* scale, const float* bias) {
  if (threadIdx.x >= ROWS * 8) return;
  const int r = threadIdx.x >> 3, q = threadIdx.x & 7;
  float v[8];
  float s = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = Y[r * PITCH + q * 8 + j];
    s += v[j];
    s2 += v[j] * v[j];
  }
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    s2 += __shfl_xor(s2, o, 64);
  }
  const float mean = s / 64.0f;
  float var = s2 / 64.0f - mean * mean;
  var = var > 0.0f ? var : 0.0f;
  const float rstd = 1.0f / sqrtf(var + 1e-6f);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int col = q * 8 + j;
    const float o = (v[j] - mean) * rstd * scale[col] + bias[col];
    Y[r * PITCH + col] = o > 0.0f ? o : 0.0f;
  }
}

}  // namespace dgppo
