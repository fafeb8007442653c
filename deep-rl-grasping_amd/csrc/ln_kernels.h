// ln_kernels.h -- layer normalisation + ReLU behind a dense layer (tf.contrib.layers.layer_norm as stable-baselines 2.10 builds
// it for `layer_norm=True`: statistics over the layer's width, biased variance, epsilon 1e-12, gamma / beta of shape [H]):
//
//   forward    u [rows, H] (x W + b, written by the dense launch with ACT_NONE)  ->  z = relu((u - mean) * rstd * gamma + beta)
//   backward   dz [rows, H] (gradient w.r.t. z, written by the backward-data launch WITHOUT its ReLU mask)  ->
//              du = rstd * (g - mean_row(g) - xhat * mean_row(g * xhat)),  g = dz * [y > 0] * gamma,  in place of dz;
//              dbeta = sum dy and dgamma = sum dy * xhat leave as one slab [2 H] per block of LN_BWD_ROWS rows -- no atomics:
//              the slabs are summed in order by a reduction descriptor, as every other gradient of the engine.
//
// The kernels know nothing about the network they serve: plain row-major buffers (row stride H) and widths, one descriptor per
// tensor, all tensors of one layer level in one launch (grid.y = descriptor).
//
// One wavefront owns a row.  Lane l holds the elements l, l + 64, ... of it in registers (NPL = ceil(H / 64) of them, a
// template argument: 1 / 2 / 4 / 8 / 16, i.e. widths up to 1024), so every load and store of a wave is a run of 64 consecutive
// floats, and the row is read once.  Mean and variance are two butterfly reductions over the 64 lanes (__shfl_xor: no LDS, and
// every lane ends with the same bits); the variance is the sum of squared deviations from the mean formed first -- never
// E[u^2] - E[u]^2, against whose cancellation an epsilon of 1e-12 does nothing.  Lanes past H carry exact zeros into both sums.
//
// What the forward leaves for the backward, counted per row: keeping u and writing (mean, rstd) costs the forward 4 H + 8
// bytes of stores and the backward 4 H + 8 bytes of loads; writing xhat instead costs the forward 8 H and the backward 4 H + 4.
// So the online network's training pass writes z to a buffer of its own, keeps u, and stores two floats per row; the backward
// forms xhat and y again with ln_xhat / ln_y below -- the very expressions the forward used, so the ReLU mask [y > 0] is the
// forward's bit for bit.  The passes nobody differentiates (online and target network on the next observations, act) run in
// place (z == u) and store no statistics.
#pragma once
#ifdef GRL_HOSTEMU
#include "hostemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <cmath>

namespace grl {

#define LN_EPS 1e-12f       /* tf.contrib.layers.layer_norm: variance_epsilon of its batch_normalization call */
#define LN_MAX_NPL 16       /* elements per lane of the widest instantiation: widths up to 64 * LN_MAX_NPL */
#define LN_FWD_ROWS 4       /* rows per forward workgroup: one per wave of its 256 threads */
#define LN_BWD_ROWS 4       /* rows per backward WAVE (taken one after the other): one slab of dbeta / dgamma each */
#define LN_BWD_WAVES 4      /* waves per backward workgroup */

struct LnDesc {
  const float* u;           // [rows, H] pre-activations (forward: may be z itself)
  float* z;                 // forward: [rows, H] output
  const float* gamma;       // [H]
  const float* beta;        // [H]
  float* stat;              // [rows, 2] mean, rstd -- forward: written when not null; backward: read
  float* dz;                // backward: [rows, H] gradient w.r.t. z in, gradient w.r.t. u out
  float* slab;              // backward: [ceil(rows / LN_BWD_ROWS)][2 H]: dbeta, then dgamma, of each block of rows
  int H;
};

// the two expressions forward and backward share (explicit fmaf: no contraction choice left to the compiler)
__host__ __device__ __forceinline__ float ln_xhat(float u, float mean, float rstd) { return (u - mean) * rstd; }
__host__ __device__ __forceinline__ float ln_y(float xhat, float gamma, float beta) { return fmaf(xhat, gamma, beta); }
__host__ __device__ __forceinline__ float ln_rstd(float var) { return 1.0f / sqrtf(var + LN_EPS); }

inline int ln_npl(int H) {      // the instantiation that holds a row of H floats; 0: none
  for (int n = 1; n <= LN_MAX_NPL; n *= 2)
    if (H <= 64 * n) return n;
  return 0;
}
inline int ln_bwd_slabs(int rows) { return (rows + LN_BWD_ROWS - 1) / LN_BWD_ROWS; }

#ifdef GRL_HOSTEMU
#include "ln_kernels_ref1.h"   // tests/hostemu: the emulation build only
#else
__device__ __forceinline__ float ln_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int NPL>
__global__ __launch_bounds__(64 * LN_FWD_ROWS) void ln_relu_fwd_kernel(const LnDesc* __restrict__ descs, int rows) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * LN_FWD_ROWS + (threadIdx.x >> 6);
  if (row >= rows) return;      // (whole waves leave: nothing below synchronises across waves)
  const LnDesc d = descs[blockIdx.y];
  const int H = d.H;
  const float* u = d.u + (long)row * H;
  float x[NPL];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int c = j * 64 + lane;
    x[j] = c < H ? u[c] : 0.f;
    s += x[j];
  }
  const float inv = 1.0f / (float)H;
  const float mean = ln_wave_sum(s) * inv;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const float dv = j * 64 + lane < H ? x[j] - mean : 0.f;
    q += dv * dv;
  }
  const float rstd = ln_rstd(ln_wave_sum(q) * inv);
  float* z = d.z + (long)row * H;
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int c = j * 64 + lane;
    if (c < H) z[c] = fmaxf(ln_y(ln_xhat(x[j], mean, rstd), d.gamma[c], d.beta[c]), 0.f);
  }
  if (d.stat && lane == 0) { d.stat[2 * (long)row] = mean; d.stat[2 * (long)row + 1] = rstd; }
}

template <int NPL>
__global__ __launch_bounds__(64 * LN_BWD_WAVES) void ln_relu_bwd_kernel(const LnDesc* __restrict__ descs, int rows) {
  const int lane = threadIdx.x & 63;
  const int blk = blockIdx.x * LN_BWD_WAVES + (threadIdx.x >> 6);      // this wave's block of LN_BWD_ROWS rows
  const int row0 = blk * LN_BWD_ROWS;
  if (row0 >= rows) return;
  const LnDesc d = descs[blockIdx.y];
  const int H = d.H;
  const float inv = 1.0f / (float)H;
  float gam[NPL], bet[NPL], db[NPL], dg[NPL];
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int c = j * 64 + lane;
    gam[j] = c < H ? d.gamma[c] : 0.f;
    bet[j] = c < H ? d.beta[c] : 0.f;
    db[j] = 0.f; dg[j] = 0.f;
  }
  const int row1 = min(row0 + LN_BWD_ROWS, rows);
  for (int row = row0; row < row1; ++row) {
    const float* u = d.u + (long)row * H;
    float* dz = d.dz + (long)row * H;
    const float mean = d.stat[2 * (long)row], rstd = d.stat[2 * (long)row + 1];
    float xh[NPL], g[NPL];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const int c = j * 64 + lane;
      const bool in = c < H;
      xh[j] = in ? ln_xhat(u[c], mean, rstd) : 0.f;
      const float dy = (in && ln_y(xh[j], gam[j], bet[j]) > 0.f) ? dz[c] : 0.f;
      db[j] += dy;
      dg[j] += dy * xh[j];
      g[j] = dy * gam[j];
      s1 += g[j];
      s2 += g[j] * xh[j];
    }
    const float m1 = ln_wave_sum(s1) * inv, m2 = ln_wave_sum(s2) * inv;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const int c = j * 64 + lane;
      if (c < H) dz[c] = rstd * (g[j] - m1 - xh[j] * m2);
    }
  }
  float* slab = d.slab + (long)blk * 2 * H;
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int c = j * 64 + lane;
    if (c < H) { slab[c] = db[j]; slab[H + c] = dg[j]; }
  }
}
#endif

// all tensors of one layer level in one launch; npl = the largest ln_npl(H) among them
inline void launch_ln_relu_fwd(const LnDesc* descs, int n_desc, int rows, int npl, hipStream_t s) {
  const dim3 grid((rows + LN_FWD_ROWS - 1) / LN_FWD_ROWS, n_desc), block(64 * LN_FWD_ROWS);
  switch (npl) {
    case 1: hipLaunchKernelGGL(ln_relu_fwd_kernel<1>, grid, block, 0, s, descs, rows); break;
    case 2: hipLaunchKernelGGL(ln_relu_fwd_kernel<2>, grid, block, 0, s, descs, rows); break;
    case 4: hipLaunchKernelGGL(ln_relu_fwd_kernel<4>, grid, block, 0, s, descs, rows); break;
    case 8: hipLaunchKernelGGL(ln_relu_fwd_kernel<8>, grid, block, 0, s, descs, rows); break;
    default: hipLaunchKernelGGL(ln_relu_fwd_kernel<16>, grid, block, 0, s, descs, rows); break;
  }
}
inline void launch_ln_relu_bwd(const LnDesc* descs, int n_desc, int rows, int npl, hipStream_t s) {
  const dim3 grid((ln_bwd_slabs(rows) + LN_BWD_WAVES - 1) / LN_BWD_WAVES, n_desc), block(64 * LN_BWD_WAVES);
  switch (npl) {
    case 1: hipLaunchKernelGGL(ln_relu_bwd_kernel<1>, grid, block, 0, s, descs, rows); break;
    case 2: hipLaunchKernelGGL(ln_relu_bwd_kernel<2>, grid, block, 0, s, descs, rows); break;
    case 4: hipLaunchKernelGGL(ln_relu_bwd_kernel<4>, grid, block, 0, s, descs, rows); break;
    case 8: hipLaunchKernelGGL(ln_relu_bwd_kernel<8>, grid, block, 0, s, descs, rows); break;
    default: hipLaunchKernelGGL(ln_relu_bwd_kernel<16>, grid, block, 0, s, descs, rows); break;
  }
}

}  // namespace grl
