// td3_kernels.h -- the kernels TD3 adds to the engine (plan_td3.inl; stable-baselines 2.10.1 td3/td3.py and td3/policies.py
// restated): gfx950, float32, VALU, no atomics.  The dense products of the policy, the twin critics and their targets stay on the
// igemm launches; what lives here is everything around them:
//
//   td3_smooth_kernel   a' = clip(tanh(target policy's output pre-activation) + clip(sigma * eps, -c, c), -1, 1), one thread per
//                       (row, pair of action components): eps from the caller or from normal_pair_draw (cfg.seed,
//                       DevScalars.rng_step -- the counter of the minibatch draw, whose streams do not overlap the normals').
//                       Written into the action columns of the target critics' input rows and, densely, for the debug view.  One
//                       thread also advances the update cursor (Td3Dev): no other thread of this launch reads it.
//   td3_pi_kernel       forward: tanh of the online policy's output pre-activations into the action columns q1(s, pi(s)) reads
//                       (act path: into the caller-visible actions); backward: d pre = d a * (1 - a^2) from the d a that the
//                       backward-data launch of q1's first layer leaves.
//   td3_loss_kernel     row-local, one lane per row (PPO_LOSS_ROWS rows per workgroup): the backup, both TD errors, d q1, d q2 and
//                       d q1pi = -1 / B; per-block sums of the five diagnostics (added in index order by grl_td3_get_metrics).
//                       Workgroup 0 also fixes the step sizes of the update's Adam launches -- the critics' always, the policy's
//                       on a policy update only -- and advances the Philox counter when something was drawn.
//
// Every batch sum leaves as per-block slabs and is added in index order, as ppo_kernels.h does.
#pragma once
#ifdef GRL_HOSTEMU
#include "hostemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <cmath>
#include "elem_kernels.h"
#ifndef GRL_PPO_TYPES_ONLY
#define GRL_PPO_TYPES_ONLY          // (PPO_LOSS_ROWS, tanh_bwd_elem: the PPO kernels are instantiated in ppo.hip)
#endif
#include "ppo_kernels.h"

namespace grl {

#define TD3_DIAG 5            /* per-block sums of an update: qf1 rows, qf2 rows, -q1pi rows, q1 rows, q2 rows */

// device words of a TD3 handle (state arena)
struct Td3Dev {
  int32_t cursor;     // update of the running grl_td3_train call the loss launch belongs to: -1 at the call's start, advanced by td3_smooth
  int32_t last_pol;   // the last policy update of the call so far (its row of the per-block sums), or -1: written by the loss launch
  float pl_carry;     // policy_loss of the handle's last policy update BEFORE the running call (0 before the first): td3_carry_kernel
  int32_t pad;
};

// One thread, at the start of every grl_td3_train call (no launch of a call is in flight then): the policy loss of the previous
// call's last policy update -- its per-block sums added in index order, as grl_td3_get_metrics adds them -- becomes the value
// critic-only rows carry; the cursor goes back to -1.
#ifndef GRL_TD3_TYPES_ONLY
__global__ void td3_carry_kernel(Td3Dev* dev, const float* part, int nblk, int B) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int u = dev->last_pol;
  if (u >= 0 && u < GRL_TD3_MAX_UPDATES) {
    float s = 0.f;
    for (int b = 0; b < nblk; ++b) s += part[((long)u * nblk + b) * TD3_DIAG + 2];
    dev->pl_carry = s / (float)B;
  }
  dev->last_pol = -1;
  dev->cursor = -1;
}
#endif

// ---------------------------------------------------------------------------------------------------------------- smoothing
struct Td3SmoothArgs {
  const float* pre; int ld_pre;        // [B, A] output pre-activations of the target policy on s'
  const float* eps;                    // [B, A] standard normals, or nullptr: Philox (seed, sc->rng_step)
  const DevScalars* sc; uint64_t seed;
  Td3Dev* dev;
  float* noise;                        // [B, A] the normals as used
  float* a_next;                       // [B, A] dense copy (debug view)
  float* x_act; int ld_x;              // action columns of the target critics' input rows
  int B, A;
  float sigma, clip;
};
__device__ __forceinline__ float td3_smooth_elem(const Td3SmoothArgs& a, float pre, float e) {
  const float n = fminf(fmaxf(a.sigma * e, -a.clip), a.clip);
  return fminf(fmaxf(tanhf(pre) + n, -1.0f), 1.0f);
}

#ifndef GRL_TD3_TYPES_ONLY
// grid (ceil(B * ceil(A / 2) / 256)): thread i owns components 2 p, 2 p + 1 of row b, i = b * ceil(A / 2) + p
__global__ __launch_bounds__(256) void td3_smooth_kernel(Td3SmoothArgs a) {
  const int hp = (a.A + 1) / 2;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) a.dev->cursor += 1;
  if (i >= (long)a.B * hp) return;
  const int b = (int)(i / hp), j0 = 2 * (int)(i % hp);
  float e[2] = {0.f, 0.f};
  if (a.eps) { e[0] = a.eps[(long)b * a.A + j0]; if (j0 + 1 < a.A) e[1] = a.eps[(long)b * a.A + j0 + 1]; }
  else normal_pair_draw(a.seed, a.sc->rng_step, b, j0, e[0], e[1]);
  for (int k = 0; k < 2 && j0 + k < a.A; ++k) {
    const int j = j0 + k;
    const float v = td3_smooth_elem(a, a.pre[(long)b * a.ld_pre + j], e[k]);
    a.noise[(long)b * a.A + j] = e[k];
    a.a_next[(long)b * a.A + j] = v;
    a.x_act[(long)b * a.ld_x + j] = v;
  }
}
#endif

// ---------------------------------------------------------------------------------------------------------------- policy output
struct Td3PiArgs {
  const float* pre; int ld_pre;        // forward: [rows, A] output pre-activations of the online policy
  float* a; int ld_a;                  // forward: tanh(pre) (dense debug view / the act path's output); backward: read
  float* x_act; int ld_x;              // forward: ... and the action columns of q1(s, pi(s))'s input rows, or nullptr
  const float* da; int ld_da;          // backward: [rows, A] d loss / d a
  float* dpre; int ld_dpre;            // backward: [rows, ld_dpre] d loss / d pre (columns [A, ld_dpre) are never written: kept zero)
  int rows, A, bwd;
};
#ifndef GRL_TD3_TYPES_ONLY
// grid (ceil(rows * A / 256)): one thread per element
__global__ __launch_bounds__(256) void td3_pi_kernel(Td3PiArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)a.rows * a.A) return;
  const int r = (int)(i / a.A), j = (int)(i % a.A);
  if (a.bwd) {
    a.dpre[(long)r * a.ld_dpre + j] = tanh_bwd_elem(a.da[(long)r * a.ld_da + j], a.a[(long)r * a.ld_a + j]);
    return;
  }
  const float v = tanhf(a.pre[(long)r * a.ld_pre + j]);
  a.a[(long)r * a.ld_a + j] = v;
  if (a.x_act) a.x_act[(long)r * a.ld_x + j] = v;
}
#endif

// ---------------------------------------------------------------------------------------------------------------- loss
struct Td3LossArgs {
  const float *rew, *done;                         // [B] the gathered scalars
  const float *q1, *q2, *q1t, *q2t, *q1pi;         // [B] critic outputs (q1pi: read on a policy update only)
  float* backup;                                   // [B]
  float *d_q1, *d_q2, *d_q1pi; int ld_d;           // [B, ld_d]
  float* part;                                     // [GRL_TD3_MAX_UPDATES, blocks, TD3_DIAG]
  Td3Dev* dev;
  DevScalars* sc;                                  // the critics' Adam words, lr, the Philox counter
  DevScalars* sc_pi;                               // the policy's Adam words
  int B; float gamma;
  int policy;                                      // 1: a policy update
  int tick_rng;                                    // 1: this update drew its indices or its normals on the device
};
inline int td3_loss_blocks(int B) { return (B + PPO_LOSS_ROWS - 1) / PPO_LOSS_ROWS; }

struct Td3Row { float l1, l2, lp, q1, q2; };
// row b: backup, TD errors, the output gradients
__device__ __forceinline__ Td3Row td3_loss_row(const Td3LossArgs& a, int b) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float inv_b = 1.0f / (float)a.B;
  const float qt = fminf(a.q1t[b], a.q2t[b]);
  const float g = a.gamma * qt;
  const float y = a.rew[b] + (1.0f - a.done[b]) * g;
  a.backup[b] = y;
  const float q1 = a.q1[b], q2 = a.q2[b];
  const float e1 = q1 - y, e2 = q2 - y;
  a.d_q1[(long)b * a.ld_d] = 2.0f * e1 * inv_b;
  a.d_q2[(long)b * a.ld_d] = 2.0f * e2 * inv_b;
  Td3Row r;
  r.l1 = e1 * e1; r.l2 = e2 * e2; r.q1 = q1; r.q2 = q2; r.lp = 0.f;
  if (a.policy) {
    a.d_q1pi[(long)b * a.ld_d] = -inv_b;
    r.lp = -a.q1pi[b];
  }
  return r;
}
// what ONE thread of the loss launch leaves in the optimiser words: TF ApplyAdam's step size of this update for the critics and,
// on a policy update, for the policy (its beta powers advance then only); the Philox counter
__device__ __forceinline__ void td3_open_apply(const Td3LossArgs& a) {
  adam_tick_device(a.sc);
  if (a.policy && a.dev->cursor >= 0 && a.dev->cursor < GRL_TD3_MAX_UPDATES) a.dev->last_pol = a.dev->cursor;
  if (a.policy) {
    a.sc_pi->adam_alpha = a.sc->lr * sqrtf(1.f - a.sc_pi->beta2_power) / (1.f - a.sc_pi->beta1_power);
    a.sc_pi->beta1_power *= 0.9f;
    a.sc_pi->beta2_power *= 0.999f;
  }
  if (a.tick_rng) { a.sc->rng_step += 1; a.sc->rng_used = 0u; }
}
// where the sums of block `blk` go, or nullptr outside a call's range
__device__ __forceinline__ float* td3_part_of(const Td3LossArgs& a, int blk, int nblk) {
  const int cur = a.dev->cursor;
  if (cur < 0 || cur >= GRL_TD3_MAX_UPDATES) return nullptr;
  return a.part + ((long)cur * nblk + blk) * TD3_DIAG;
}

#ifndef GRL_TD3_TYPES_ONLY
#ifdef GRL_HOSTEMU
#include "td3_kernels_ref1.h"   // tests/hostemu: the emulation build only
#else
__device__ __forceinline__ float td3_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// grid (td3_loss_blocks(B)): lane = row
__global__ __launch_bounds__(PPO_LOSS_ROWS) void td3_loss_kernel(Td3LossArgs a) {
  __shared__ float ws[PPO_LOSS_ROWS / 64][TD3_DIAG];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int b = blockIdx.x * PPO_LOSS_ROWS + t;
  Td3Row r = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (b < a.B) r = td3_loss_row(a, b);
  const float dg[TD3_DIAG] = {r.l1, r.l2, r.lp, r.q1, r.q2};
  for (int k = 0; k < TD3_DIAG; ++k) {
    const float s = td3_wave_sum(dg[k]);
    if (lane == 0) ws[w][k] = s;
  }
  __syncthreads();
  if (t < TD3_DIAG) {
    float s = ws[0][t];
    for (int k = 1; k < PPO_LOSS_ROWS / 64; ++k) s += ws[k][t];
    float* out = td3_part_of(a, (int)blockIdx.x, (int)gridDim.x);
    if (out) out[t] = s;
  }
  if (blockIdx.x == 0 && t == PPO_LOSS_ROWS - 1) td3_open_apply(a);
}
#endif
#endif  // GRL_TD3_TYPES_ONLY

// the launches (td3.hip)
void launch_td3_smooth(const Td3SmoothArgs& a, hipStream_t s);
void launch_td3_pi(const Td3PiArgs& a, hipStream_t s);
void launch_td3_loss(const Td3LossArgs& a, hipStream_t s);
void launch_td3_carry(Td3Dev* dev, const float* part, int nblk, int B, hipStream_t s);

}  // namespace grl
