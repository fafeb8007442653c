// bc_kernels.h -- the kernels of behaviour-cloning pretraining (SAC.pretrain: plan_bc.inl) that are not GEMMs: the minibatch
// gather from a caller-owned (observation, action) table, the loss with its output gradient, and the launch that closes the
// loss of an update.  Everything else -- the extractor, the dense layers, their backward and weight-gradient launches, the slab
// reduction, Adam over the trained range (adam_polyak_kernel on the session's own DevScalars) -- are the launches of the SAC plan
// restricted to the policy network.
//
// One update on n valid rows (stable-baselines 2.10.1, BaseRLModel.pretrain with SAC._get_pretrain_placeholders):
//   det = tanh(mu(obs));  a_env = low + 0.5 (det + 1)(high - low);  loss = mean over n * A of (a_exp - a_env)^2
// In policy scale, with s_j = 0.5 (high_j - low_j) and a'_j = (a_exp_j - low_j) / s_j - 1:  a_exp - a_env = s_j (a'_j - det_j), so
//   d loss / d mu_j = 2 s_j^2 (det_j - a'_j)(1 - det_j^2) / (n A).
// Rows whose index is -1 (the tail of a final partial minibatch) contribute nothing to the loss or to any gradient.
//
// A session's words live in BcDev, the optimiser's in a DevScalars behind it (both in the caller's BC buffer).  The arrays of a call (table, indices) are written there by
// bc_open_kernel, so that the launch list of an update has fixed arguments and a call of n updates repeats ONE list: the
// gather reads the index row of update `step`, the closing launch writes losses[step] and advances `step`.
#pragma once
#ifdef GRL_HOSTEMU
#include "hostemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include "elem_kernels.h"

namespace grl {

#define GRL_BC_MAX_UPDATES 65536      /* updates / batches of one grl_bc_train / grl_bc_eval call (a loss slot each) */
#define BC_LOSS_ROWS 256              /* rows per workgroup of the loss launch: one lane each */

struct BcDev {
  int32_t step;                       // update (batch) of the running call
  int32_t n_valid;                    // rows of the current minibatch whose index is not -1 (written by the gather)
  const float* obs;                   // the call's table [n_rows, obs_size] / [n_rows, A] and index rows [n, batch]
  const float* act;
  const int32_t* idx;
};

struct BcGatherArgs {
  BcDev* dev;
  int batch;                          // rows of a minibatch (the plan's bc_batch)
  int hw, c_obs, c_img, n_direct, vec_dim;      // observation layout, as ActIngestArgs
  float scale_div;                    // 255 for images (the SAC update's own division), 1 for vectors
  float* x; int ldx;                  // image part [batch, hw * c_img] / the vector observation [batch, ldx]
  float* d; int ldd;                  // direct features
  int A; float* act_out;              // expert actions [batch, A], as the table holds them
};

struct BcLossArgs {
  BcDev* dev;
  int batch, A;
  const float* mu; int ld_mu;
  const float* act;                   // [batch, A] gathered expert actions (env scale)
  const float* low; const float* half;      // [A] low_j and s_j = 0.5 (high_j - low_j)
  float* det;                         // [batch, A]
  float* dmu; int ld_dm;              // [batch, ld_dm] (nullptr: forward only)
  float* row_loss;                    // [batch] sum over j of s_j^2 (det_j - a'_j)^2 (0 for absent rows)
};

struct BcCloseArgs {
  BcDev* dev;
  DevScalars* sc;                     // the session's optimiser words
  int batch, A;
  const float* row_loss;
  float* losses;                      // [GRL_BC_MAX_UPDATES]
  int tick;                           // 1: an update (Adam step size + beta powers), 0: evaluation
};

__global__ void bc_open_kernel(BcDev* dev, const float* obs, const float* act, const int32_t* idx) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  dev->obs = obs; dev->act = act; dev->idx = idx; dev->step = 0; dev->n_valid = 0;
}

// grid (ceil(elements / 256), batch): row b of the update's input from table row idx[step][b] (row 0 for -1: the loss masks it).
// The split into image and direct features and the division are those of the SAC paths (act_ingest_kernel, scale_elem).
__global__ __launch_bounds__(256) void bc_gather_kernel(BcGatherArgs a) {
  const int b = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int32_t* row = a.dev->idx + (long)a.dev->step * a.batch;
  const long src = row[b] >= 0 ? row[b] : 0;
  if (b == 0 && e == 0) a.dev->n_valid = rows_present(row, a.batch);
  if (blockIdx.x == 0 && threadIdx.x < a.A) a.act_out[(long)b * a.A + threadIdx.x] = a.dev->act[src * a.A + threadIdx.x];
  if (a.vec_dim > 0) {
    if (e < a.vec_dim) a.x[(long)b * a.ldx + e] = a.dev->obs[src * a.vec_dim + e];
    return;
  }
  const int img_elems = a.hw * a.c_img;
  const float* obs = a.dev->obs + src * (long)a.hw * a.c_obs;
  if (e < img_elems) {
    const int px = e / a.c_img, c = e - px * a.c_img;
    a.x[(long)b * a.ldx + e] = scale_elem(obs[(long)px * a.c_obs + c], a.scale_div);
  }
  if (blockIdx.x == 0 && threadIdx.x < a.n_direct) {
    const int q = threadIdx.x;
    a.d[(long)b * a.ldd + q] = scale_elem(obs[(long)q * a.c_obs + (a.c_obs - 1)], a.scale_div);
  }
}

// one lane per row: mu -> det -> the row's loss and d mu
__global__ __launch_bounds__(BC_LOSS_ROWS) void bc_loss_kernel(BcLossArgs a) {
  const int b = blockIdx.x * BC_LOSS_ROWS + threadIdx.x;
  if (b >= a.batch) return;
  const int n = a.dev->n_valid;
  const bool present = b < n;
  const float inv = 1.f / ((float)n * (float)a.A);
  float s = 0.f;
  for (int j = 0; j < a.A; ++j) {
    const float det = tanhf(a.mu[(long)b * a.ld_mu + j]);
    const float h = a.half[j];
    const float ap = (a.act[(long)b * a.A + j] - a.low[j]) / h - 1.f;
    const float diff = det - ap;
    a.det[(long)b * a.A + j] = det;
    if (present) s += (h * diff) * (h * diff);
    if (a.dmu) a.dmu[(long)b * a.ld_dm + j] = present ? 2.f * h * h * diff * (1.f - det * det) * inv : 0.f;
  }
  a.row_loss[b] = s;
}

#ifdef GRL_HOSTEMU
#include "bc_kernels_ref1.h"   // tests/hostemu: the emulation build only
#else
// 64 lanes: lane t adds rows t, t + 64, ... in order, then the lanes meet pairwise at distances 32, 16, .. 1
__device__ __forceinline__ float bc_rows_sum(const float* row_loss, int batch) {
  float s = 0.f;
  for (int b = threadIdx.x; b < batch; b += 64) s += row_loss[b];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  return s;
}
#endif

// one wavefront: the loss of the update from its rows, then -- behind every reader of `step` and in front of the update's
// Adam launch -- the step size of this update, the beta powers of the next, and the step counter
__global__ __launch_bounds__(64) void bc_close_kernel(BcCloseArgs a) {
  const float s = bc_rows_sum(a.row_loss, a.batch);
  if (threadIdx.x != 0) return;
  BcDev* d = a.dev;
  if (d->step < GRL_BC_MAX_UPDATES) a.losses[d->step] = s / ((float)d->n_valid * (float)a.A);
  if (a.tick) adam_tick_device(a.sc);
  d->step += 1;
}

}  // namespace grl
