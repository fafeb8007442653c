// gail_kernels.h -- the kernels a GAIL session adds to a TRPO handle (plan_gail.inl; stable-baselines 2.10.1 gail/adversary.py
// TransitionClassifier and common/mpi_running_mean_std.py restated): gfx950, float32 unless stated, VALU, no atomics.  The three
// dense layers of the discriminator stay on the igemm launches, tanh between them on tanh_fwd / tanh_bwd of ppo_kernels.h; what
// lives here is everything around them:
//
//   gail_input_kernel   one thread owns a column of the input [ (obs - mean) / std | action ].  An observation column of the
//                       update pass adds its values of the gathered generator rows, then of the expert rows, into float64 sum /
//                       sumsq in row order (RunningMeanStd.update(concat(ob_g, ob_e))), forms float32 mean / std from the
//                       UPDATED sums and writes the normalised column of all rows; an action column is copied -- as stored for
//                       the update pass, clipped to the bounds for the reward pass.  The reward pass (update = 0) is the same
//                       kernel over the T rollout rows in place, with the mean / std the last update stored.  Adjacent threads
//                       own adjacent columns: every row-strided access of a wavefront is one run of 256 bytes; a thread issues the
//                       loads of eight rows before it stores the first (gail_rows8), the float64 chains add in row order.
//   gail_loss_kernel    lane = row over the n_g + n_e logits: softplus / sigmoid in their overflow-safe forms, d total / d logit
//                       with the 1 / n_g, 1 / n_e and 1 / (n_g + n_e) factors (absent expert rows: 0), per-block sums of the
//                       diagnostics (added in index order by grl_gail_get_losses).
//   gail_reward_kernel  lane = row: logits -> -log(1 - sigmoid + 1e-8) into the rollout's reward array, the environment's
//                       reward into a copy of its own.
//
// A session's words live in GailDev (in the caller's session buffer).  The arrays of a call (table, index rows) are written there
// by gail_open_kernel, so that the launch list of an update has fixed arguments and a call of n updates repeats ONE list: the
// input launch reads the index rows of update `cursor` and leaves it in `cur`, the loss launch reads `cur` and advances `cursor`
// (no launch reads a word it writes).  The statistics' count is kept once per column, so that no thread reads a word another writes.
#pragma once
#ifdef GRL_HOSTEMU
#include "hostemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <cmath>
#include "elem_kernels.h"

namespace grl {

#define GRL_GAIL_MAX_UPDATES 4096     /* updates of one grl_gail_update call (a row of loss slots each) */
#define GAIL_LOSS_ROWS 256            /* rows per workgroup of the loss launch: one lane each */
#define GAIL_DIAG 6                   /* per-block sums: softplus(g), softplus(-e), ent (all rows), unused, g < 0, e > 0 */

struct GailDev {
  int32_t cursor;                     // update of the running call the next input launch takes (reset by the call)
  int32_t cur;                        // the update the launches behind the input launch belong to
  int32_t n_e;                        // expert rows of the current minibatch whose index is not -1
  int32_t pad;
  const float* exp_obs;               // the call's table [n_rows, obs_dim] / [n_rows, A] and index rows [n, batch]
  const float* exp_act;
  const int32_t* gen_idx;
  const int32_t* exp_idx;
};

struct GailInputArgs {
  GailDev* dev;
  DevScalars* sc;                     // the session's Adam words (update pass: ticked by the thread of column 0)
  const float* r_obs; int ldo;        // rollout observations [T, ldo], actions [T, A]
  const float* r_act;
  double *sum, *sumsq, *count;        // [obs_dim] each (the count once per column)
  float *mean, *sd;                   // [obs_dim]: float32(sum / count), sqrt(max(float32(sumsq / count) - mean^2, 1e-2))
  const float *low, *high;            // [A] (reward pass)
  float* x; int ldx;                  // [rows, ldx]; columns [obs_dim + A, ldx) stay zero
  int obs_dim, A;
  int n_gen;                          // generator rows: batch (update pass, gathered) or T (reward pass, in place)
  int update;                         // 1: gather by the index rows, expert rows behind the generator's, statistics; 0: reward pass
};

struct GailLossArgs {
  GailDev* dev;
  const float* logits;                // [2 batch]
  float* dlogits; int ld_dl;          // [2 batch, ld_dl]
  float* diag;                        // [updates, blocks, GAIL_DIAG]
  int batch;
  float entcoeff;
};
inline int gail_loss_blocks(int batch) { return (2 * batch + GAIL_LOSS_ROWS - 1) / GAIL_LOSS_ROWS; }

struct GailRewardArgs {
  const float* logits;                // [T]
  float* rew;                         // [T] the rollout's rewards: read (the environment's), then rewritten
  float* true_rew;                    // [T]
  int T;
};

__device__ __forceinline__ float gail_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float gail_sigmoid(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// float32 mean / std of a column from its float64 sums (mpi_running_mean_std.py: every operation rounded, nothing contracted)
__host__ __device__ __forceinline__ void gail_mean_sd(double sum, double sumsq, double count, float& mean, float& sd) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  mean = (float)(sum / count);
  const float msq = (float)(sumsq / count);
  const float sq = mean * mean;
  sd = sqrtf(fmaxf(msq - sq, 1e-2f));
}

struct GailRowDiag { float d[GAIL_DIAG]; };
// row r of the loss launch: writes d total / d logit, returns the row's share of the six sums
__device__ __forceinline__ GailRowDiag gail_loss_row(const GailLossArgs& a, int r, int n_e) {
  GailRowDiag o = {{0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
  const bool gen = r < a.batch;
  const bool present = gen || r - a.batch < n_e;
  float dl = 0.f;
  if (present) {
    const float x = a.logits[r];
    const float s = gail_sigmoid(x);
    const float sp_neg = gail_softplus(-x);
    const float n_all = (float)(a.batch + n_e);
    o.d[2] = (1.f - s) * x + sp_neg;
    dl = a.entcoeff * s * (1.f - s) * x / n_all;      // -entcoeff * d ent / d x, d ent / d x = -s (1 - s) x
    if (gen) {
      o.d[0] = gail_softplus(x);
      o.d[4] = x < 0.f ? 1.f : 0.f;
      dl += s / (float)a.batch;
    } else {
      o.d[1] = sp_neg;
      o.d[5] = x > 0.f ? 1.f : 0.f;
      dl -= (1.f - s) / (float)n_e;
    }
  }
  a.dlogits[(long)r * a.ld_dl] = dl;
  return o;
}

__device__ __forceinline__ float gail_reward(float logit) { return -logf(gail_sigmoid(-logit) + 1e-8f); }

// rows [0, n) of a column in batches of eight: the eight loads are issued before the first store (the compiler cannot see that
// the stores into x never feed the loads, and would otherwise wait for every row's load before it stores)
template <class L, class S>
__device__ __forceinline__ void gail_rows8(int n, L load, S store) {
  for (int b0 = 0; b0 < n; b0 += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = b0 + k < n ? load(b0 + k) : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (b0 + k < n) store(b0 + k, v[k]);
  }
}

#ifndef GRL_GAIL_TYPES_ONLY
__global__ void gail_open_kernel(GailDev* dev, const float* obs, const float* act, const int32_t* gen_idx, const int32_t* exp_idx) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  dev->exp_obs = obs; dev->exp_act = act; dev->gen_idx = gen_idx; dev->exp_idx = exp_idx;
  dev->cursor = 0; dev->cur = 0; dev->n_e = 0;
}

// grid (ceil((obs_dim + A) / 256)): thread = column.  Lane-local: compiles as it stands in the emulation build.
__global__ __launch_bounds__(256) void gail_input_kernel(GailInputArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.obs_dim + a.A) return;
  const int n_g = a.n_gen;
  // (the session's buffers, the rollout and the caller's table never overlap: loads may run ahead of the stores into x)
  const float* __restrict__ const r_obs = a.r_obs;
  const float* __restrict__ const r_act = a.r_act;
  float* __restrict__ const x = a.x;
  const int32_t* __restrict__ gi = nullptr;
  const int32_t* __restrict__ ei = nullptr;
  const float* __restrict__ e_obs = nullptr;
  const float* __restrict__ e_act = nullptr;
  int n_e = 0;
  if (a.update) {
    const long u = a.dev->cursor;
    gi = a.dev->gen_idx + u * n_g;
    ei = a.dev->exp_idx + u * n_g;
    e_obs = a.dev->exp_obs; e_act = a.dev->exp_act;
    n_e = rows_present(ei, n_g);
    if (c == 0) {
      a.dev->cur = (int32_t)u;
      a.dev->n_e = n_e;
      adam_tick_device(a.sc);
    }
  }
  if (c >= a.obs_dim) {      // an action column
    const int j = c - a.obs_dim;
    if (!a.update) {
      const float lo = a.low[j], hi = a.high[j];
      gail_rows8(n_g, [&](int b) { return r_act[(long)b * a.A + j]; }, [&](int b, float v) { x[(long)b * a.ldx + c] = fminf(fmaxf(v, lo), hi); });
      return;
    }
    gail_rows8(n_g, [&](int b) { return r_act[(long)gi[b] * a.A + j]; }, [&](int b, float v) { x[(long)b * a.ldx + c] = v; });
    gail_rows8(n_e, [&](int b) { return e_act[(long)ei[b] * a.A + j]; }, [&](int b, float v) { x[(long)(n_g + b) * a.ldx + c] = v; });
    for (int b = n_e; b < n_g; ++b) x[(long)(n_g + b) * a.ldx + c] = 0.f;
    return;
  }
  float mean, sd;
  if (a.update) {
    double s = 0.0, q = 0.0;
    // (the rows' loads are independent and run ahead of the two addition chains, whose order is the rows')
#pragma unroll 8
    for (int b = 0; b < n_g; ++b) { const double v = r_obs[(long)gi[b] * a.ldo + c]; s += v; q += v * v; }
#pragma unroll 8
    for (int b = 0; b < n_e; ++b) { const double v = e_obs[(long)ei[b] * a.obs_dim + c]; s += v; q += v * v; }
    const double sum = a.sum[c] + s, sumsq = a.sumsq[c] + q, count = a.count[c] + (double)(n_g + n_e);
    a.sum[c] = sum; a.sumsq[c] = sumsq; a.count[c] = count;
    gail_mean_sd(sum, sumsq, count, mean, sd);
    a.mean[c] = mean; a.sd[c] = sd;
  } else {
    mean = a.mean[c]; sd = a.sd[c];
  }
  const auto put = [&](long row, float v) { x[row * a.ldx + c] = (v - mean) / sd; };
  if (!a.update) {
    gail_rows8(n_g, [&](int b) { return r_obs[(long)b * a.ldo + c]; }, [&](int b, float v) { put(b, v); });
    return;
  }
  gail_rows8(n_g, [&](int b) { return r_obs[(long)gi[b] * a.ldo + c]; }, [&](int b, float v) { put(b, v); });
  gail_rows8(n_e, [&](int b) { return e_obs[(long)ei[b] * a.obs_dim + c]; }, [&](int b, float v) { put(n_g + b, v); });
  for (int b = n_e; b < n_g; ++b) x[(long)(n_g + b) * a.ldx + c] = 0.f;
}

// grid (ceil(T / 256)): lane = row.  Lane-local.
__global__ __launch_bounds__(256) void gail_reward_kernel(GailRewardArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.T) return;
  a.true_rew[i] = a.rew[i];
  a.rew[i] = gail_reward(a.logits[i]);
}

#ifdef GRL_HOSTEMU
#include "gail_kernels_ref1.h"   // tests/hostemu: the emulation build only
#else
// grid (gail_loss_blocks(batch)): lane = row; the six sums of a workgroup meet per wavefront, then in LDS, in a fixed order
__global__ __launch_bounds__(GAIL_LOSS_ROWS) void gail_loss_kernel(GailLossArgs a) {
  __shared__ float ws[GAIL_LOSS_ROWS / 64][GAIL_DIAG];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int r = blockIdx.x * GAIL_LOSS_ROWS + t;
  const int cur = a.dev->cur, n_e = a.dev->n_e;
  GailRowDiag o = {{0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
  if (r < 2 * a.batch) o = gail_loss_row(a, r, n_e);
  for (int k = 0; k < GAIL_DIAG; ++k) {
    float s = o.d[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) ws[w][k] = s;
  }
  __syncthreads();
  if (t < GAIL_DIAG) {
    float s = ws[0][t];
    for (int k = 1; k < GAIL_LOSS_ROWS / 64; ++k) s += ws[k][t];
    if (cur < GRL_GAIL_MAX_UPDATES) a.diag[((long)cur * gridDim.x + blockIdx.x) * GAIL_DIAG + t] = s;
  }
  if (blockIdx.x == 0 && t == 0) a.dev->cursor = cur + 1;      // (this launch reads `cur`, the input launch `cursor`)
}
#endif
#endif  // GRL_GAIL_TYPES_ONLY

// the launches (gail.hip)
void launch_gail_open(GailDev* dev, const float* obs, const float* act, const int32_t* gen_idx, const int32_t* exp_idx, hipStream_t s);
void launch_gail_input(const GailInputArgs& a, hipStream_t s);
void launch_gail_loss(const GailLossArgs& a, hipStream_t s);
void launch_gail_reward(const GailRewardArgs& a, hipStream_t s);

}  // namespace grl
