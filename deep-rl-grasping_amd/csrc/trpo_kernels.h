// trpo_kernels.h -- the kernels TRPO adds to the engine (plan_trpo.inl; stable-baselines 2.10.1 trpo_mpi/trpo_mpi.py, common/cg.py
// and common/distributions.py restated): gfx950, float32, VALU, no atomics.  The policy, the rollout, GAE and the dense / tanh
// launches are PPO2's (ppo_kernels.h, plan_ppo.inl); what lives here is the natural-gradient step and the value fit around them:
//
//   trpo_prep_kernel     atarg = (adv - mean) / (std + 1e-8) over the T rows (one workgroup, two passes), flags of the update reset
//   trpo_loss_kernel     lane = row: logp, ratio, KL against the old policy; per-block sums of surrogate and KL.  Gradient mode (at
//                        the old parameters) also writes d mean, per-block slabs of d logstd and the old policy's outputs; evaluate
//                        mode serves the line-search trials and returns at once when a trial was accepted
//   trpo_scal_kernel     one lane: the per-block sums added in index order into the scalars of TrpoDev (losses before the step, rr of
//                        conjugate gradient, zero-gradient flag, the decision of a line-search trial)
//   trpo_tan_kernel      one level of the tangent forward: dh = (1 - h^2) * (h_below dW + db  +  dh_below W) from the two dense
//                        products of the level; as the output stage: d mean = mean_dot / sigma^2 / n
//   trpo_fvp_fin_kernel  F(v) += cg_damping * v; the logstd entries are 2 v + cg_damping * v
//   trpo_cg_*_kernel     conjugate gradient on vectors laid out like the gradient bucket (entries of the value variables stay 0):
//                        init (r = p = g, x = 0, g.g, max |g|), dot, x / r update with alpha from device memory, p update
//   trpo_step_kernel     fullstep = x / sqrt(|shs| / max_kl)
//   trpo_theta_kernel    snapshot / theta' = theta_old + 2^-k fullstep / restore
//   trpo_gather_kernel   the Fisher rows 0, stride, 2 stride, ... of the rollout's observations
//   trpo_vf_loss_kernel  d mean((V - tdlamret)^2) / d V of a value minibatch
//
// Every sum is two-stage: per-block sums by a fixed tree, then the blocks in index order.  Flags and scalars live in TrpoDev, the
// launch list never changes shape: a launch whose flag says "finished" / "accepted" returns at once.
#pragma once
#ifdef GRL_HOSTEMU
#include "hostemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <algorithm>
#include <cmath>
#include "ppo_kernels.h"

namespace grl {

#define GRL_TRPO_MAX_CG 64      /* grl_trpo_config.cg_iters */
#define GRL_TRPO_MAX_LS 16      /* grl_trpo_config.ls_steps */
#define TRPO_ROWS 256           /* rows per workgroup of the loss launch: one lane each */
#define TRPO_VEC_BLOCKS 256     /* most workgroups of a vector launch (one partial sum each) */

// device words of a TRPO handle (state arena, behind PpoDev)
struct TrpoDev {
  int32_t zero_grad;                      // every |g_i| <= 1e-8: no policy step
  int32_t cg_iters;                       // conjugate-gradient iterations run
  int32_t ls_accepted, ls_index;          // line search: a trial was accepted; its index (-1 restored, -2 zero gradient)
  int32_t done[GRL_TRPO_MAX_CG + 1];      // done[i]: CG had left its loop before iteration i
  float rr[GRL_TRPO_MAX_CG + 1];          // rr[i]: r.r before iteration i
  float before[5];                        // optimgain, meankl, entbonus, surrgain, meanent at the old parameters
  float trial[2];                         // optimgain, meankl of the accepted trial
  float shs, lm;                          // 0.5 x.F(x); sqrt(|shs| / max_kl)
};

inline int trpo_vec_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(TRPO_VEC_BLOCKS, (n + 4095) / 4096)); }
inline int trpo_loss_blocks(int T) { return (T + TRPO_ROWS - 1) / TRPO_ROWS; }

struct TrpoPrepArgs { const float* adv; float* atarg; TrpoDev* dev; int T; };

struct TrpoLossArgs {
  const float* mean; int ld_mean;      // [T, A] at the parameters being evaluated
  const float* logstd;                 // [A]
  const float *act, *atarg;            // [T, A], [T]
  float *mean_old, *logstd_old;        // [T, A], [A]: written in gradient mode, read in evaluate mode
  float* dmean; int ld_dm;             // [T, ld_dm] (gradient mode)
  float* dls_slab;                     // [blocks, A] (gradient mode); block 0 also carries ent_coef per component
  float* part;                         // [blocks, 2] sums of ratio * atarg and of the row KL
  const TrpoDev* dev;
  int T, A, mode;                      // mode 0 gradient, 1 evaluate
  float ent_coef;
};
struct TrpoRow { float surr, kl, w; };
// row b: ratio * atarg, KL(old || new), and w = d optimgain / d logp(b)
__device__ __forceinline__ TrpoRow trpo_loss_row(const TrpoLossArgs& a, int b) {
  float q = 0.f, qo = 0.f, sl = 0.f, slo = 0.f, kl = 0.f;
  for (int j = 0; j < a.A; ++j) {
    const float ls = a.logstd[j], lso = a.mode ? a.logstd_old[j] : ls;
    const float m = a.mean[(long)b * a.ld_mean + j], mo = a.mode ? a.mean_old[(long)b * a.A + j] : m;
    const float ac = a.act[(long)b * a.A + j];
    const float sd = expf(ls), sdo = expf(lso);
    const float u = (ac - m) / sd, uo = (ac - mo) / sdo, d = mo - m;
    q += u * u; qo += uo * uo; sl += ls; slo += lso;
    kl += ls - lso + (sdo * sdo + d * d) / (2.0f * sd * sd) - 0.5f;
  }
  const float c = ppo_half_log_2pi() * (float)a.A;
  const float logp = -(0.5f * q + c + sl), logpo = -(0.5f * qo + c + slo);
  const float ratio = expf(logp - logpo);
  TrpoRow r;
  r.surr = ratio * a.atarg[b];
  r.kl = kl;
  r.w = r.surr / (float)a.T;
  return r;
}
// component j of row b (gradient mode): writes d mean and the old mean, returns the row's share of d logstd
__device__ __forceinline__ float trpo_loss_row_j(const TrpoLossArgs& a, int b, int j, float w) {
  const float sd = expf(a.logstd[j]), m = a.mean[(long)b * a.ld_mean + j];
  const float u = (a.act[(long)b * a.A + j] - m) / sd;
  a.dmean[(long)b * a.ld_dm + j] = w * (u / sd);
  a.mean_old[(long)b * a.A + j] = m;
  return w * (u * u - 1.0f);
}

struct TrpoScalArgs {
  TrpoDev* dev;
  const float* part; int n_part;       // per-block sums: [n_part, 2]
  const float* logstd;
  int A, T, mode, k;                   // mode 0 losses before, 1 CG start (part: g.g | max |g|), 2 line-search trial k
  float ent_coef, max_kl;
};
enum { TRPO_SC_BEFORE = 0, TRPO_SC_CG = 1, TRPO_SC_TRIAL = 2 };

struct TrpoTanArgs {
  const float *t1, *t2;                // [rows, H] the two products of the level (t2 nullptr: the lowest level has no tangent below)
  const float* h;                      // [rows, H] activations (hidden level) or nullptr (output stage)
  const float* logstd;                 // output stage: [H]
  float* out; int ld_out;              // [rows, ld_out]
  int rows, H;
  float inv_n;                         // output stage: 1 / rows
};

struct TrpoVecArgs {                   // the vector launches: n entries, laid out like the gradient bucket
  float *x, *r, *p, *z;
  const float *g, *v;
  float* full;
  float *part, *part2;                 // [blocks] partial sums
  TrpoDev* dev;
  int64_t n, ls_off;
  int A, it, n_part;
  float damping, max_kl, scale;
};

#ifndef GRL_TRPO_TYPES_ONLY
#ifdef GRL_HOSTEMU
#include "trpo_kernels_ref1.h"   // tests/hostemu: the emulation build only
#else
// the lanes of a workgroup share an element range; trpo_block_sum adds their partial sums by a fixed tree
#define TRPO_LANES(t, nt) const int t = threadIdx.x, nt = 256
__device__ __forceinline__ float trpo_block_sum(float v) {
  __shared__ float red[256];
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) red[t] += red[t + off];
    __syncthreads();
  }
  const float s = red[0];
  __syncthreads();
  return s;
}
__device__ __forceinline__ float trpo_block_max(float v) {
  __shared__ float red[256];
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) red[t] = fmaxf(red[t], red[t + off]);
    __syncthreads();
  }
  const float s = red[0];
  __syncthreads();
  return s;
}
__device__ __forceinline__ float trpo_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// grid (trpo_loss_blocks(T)): lane = row
__global__ __launch_bounds__(TRPO_ROWS) void trpo_loss_kernel(TrpoLossArgs a) {
  __shared__ float ws[TRPO_ROWS / 64][PPO_MAX_A + 2];
  if (a.mode && (a.dev->ls_accepted || a.dev->zero_grad)) return;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int b = blockIdx.x * TRPO_ROWS + t;
  const bool live = b < a.T;
  TrpoRow r = {0.f, 0.f, 0.f};
  if (live) r = trpo_loss_row(a, b);
  const int nA = a.mode ? 0 : a.A;
  for (int j = 0; j < nA; ++j) {
    const float s = trpo_wave_sum(live ? trpo_loss_row_j(a, b, j, r.w) : 0.f);
    if (lane == 0) ws[w][j] = s;
  }
  const float s0 = trpo_wave_sum(r.surr), s1 = trpo_wave_sum(r.kl);
  if (lane == 0) { ws[w][PPO_MAX_A] = s0; ws[w][PPO_MAX_A + 1] = s1; }
  __syncthreads();
  if (t < nA || (t >= PPO_MAX_A && t < PPO_MAX_A + 2)) {
    float s = ws[0][t];
    for (int k = 1; k < TRPO_ROWS / 64; ++k) s += ws[k][t];
    if (t < nA) a.dls_slab[(long)blockIdx.x * a.A + t] = blockIdx.x == 0 ? s + a.ent_coef : s;
    else a.part[(long)blockIdx.x * 2 + (t - PPO_MAX_A)] = s;
  }
  if (!a.mode && blockIdx.x == 0 && t < a.A) a.logstd_old[t] = a.logstd[t];
}
#endif

// one workgroup
__global__ __launch_bounds__(256) void trpo_prep_kernel(TrpoPrepArgs a) {
  TRPO_LANES(t, nt);
  float s = 0.f;
  for (int i = t; i < a.T; i += nt) s += a.adv[i];
  const float mean = trpo_block_sum(s) / (float)a.T;
  float q = 0.f;
  for (int i = t; i < a.T; i += nt) { const float d = a.adv[i] - mean; q += d * d; }
  const float sd = sqrtf(trpo_block_sum(q) / (float)a.T) + 1e-8f;
  for (int i = t; i < a.T; i += nt) a.atarg[i] = (a.adv[i] - mean) / sd;
  if (t == 0) {
    TrpoDev* d = a.dev;
    d->zero_grad = 0; d->cg_iters = 0; d->ls_accepted = 0; d->ls_index = -1;
    d->trial[0] = d->trial[1] = 0.f; d->shs = 0.f; d->lm = 0.f;
  }
}

// one lane
__global__ __launch_bounds__(64) void trpo_scal_kernel(TrpoScalArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  TrpoDev* d = a.dev;
  float s0 = 0.f, s1 = 0.f;
  if (a.mode == TRPO_SC_CG) {
    for (int i = 0; i < a.n_part; ++i) { s0 += a.part[2 * i]; s1 = fmaxf(s1, a.part[2 * i + 1]); }
    const int zero = s1 <= 1e-8f ? 1 : 0;      // np.allclose(g, 0)
    d->zero_grad = zero;
    d->ls_index = zero ? -2 : -1;
    d->done[0] = zero;
    d->rr[0] = s0;
    return;
  }
  if (a.mode == TRPO_SC_TRIAL && (d->ls_accepted || d->zero_grad)) return;
  for (int i = 0; i < a.n_part; ++i) { s0 += a.part[2 * i]; s1 += a.part[2 * i + 1]; }
  float ent = 0.f;
  for (int j = 0; j < a.A; ++j) ent += a.logstd[j] + 1.4189385332046727f;      // 0.5 * log(2 pi e)
  const float surr = s0 / (float)a.T, kl = s1 / (float)a.T, bonus = a.ent_coef * ent, gain = surr + bonus;
  if (a.mode == TRPO_SC_BEFORE) {
    d->before[0] = gain; d->before[1] = kl; d->before[2] = bonus; d->before[3] = surr; d->before[4] = ent;
    return;
  }
  auto fin = [](float v) { return fabsf(v) <= 3.4028235e38f; };      // (false for NaN and the infinities)
  const bool finite = fin(gain) && fin(kl) && fin(bonus) && fin(surr) && fin(ent);
  if (finite && !(kl > a.max_kl * 1.5f) && !(gain - d->before[0] < 0.f)) {
    d->ls_accepted = 1; d->ls_index = a.k;
    d->trial[0] = gain; d->trial[1] = kl;
  }
}

// grid (blocks, 1): element-wise over rows * H
__global__ __launch_bounds__(256) void trpo_tan_kernel(TrpoTanArgs a) {
  const long n = (long)a.rows * a.H;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float s = a.t2 ? a.t1[i] + a.t2[i] : a.t1[i];
    if (a.h) {
      const float hv = a.h[i];
      a.out[i] = (1.0f - hv * hv) * s;
    } else {
      const long r = i / a.H;
      const int j = (int)(i - r * a.H);
      const float sd = expf(a.logstd[j]);
      a.out[r * a.ld_out + j] = s / (sd * sd) * a.inv_n;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- vectors
// workgroup blk of a vector launch owns the entries [lo, hi)
__device__ __forceinline__ void trpo_range(int64_t n, int64_t& lo, int64_t& hi) {
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  lo = (int64_t)blockIdx.x * per;
  hi = lo + per < n ? lo + per : n;
}
__device__ __forceinline__ float trpo_sum_parts(const float* part, int n) {
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += part[i];
  return s;
}

// r = p = g, x = 0; part[2 blk] = g.g, part[2 blk + 1] = max |g| of the block's range
__global__ __launch_bounds__(256) void trpo_cg_init_kernel(TrpoVecArgs a) {
  TRPO_LANES(t, nt);
  int64_t lo, hi;
  trpo_range(a.n, lo, hi);
  float s = 0.f, m = 0.f;
  for (int64_t i = lo + t; i < hi; i += nt) {
    const float g = a.g[i];
    a.r[i] = g; a.p[i] = g; a.x[i] = 0.f;
    s += g * g;
    m = fmaxf(m, fabsf(g));
  }
  s = trpo_block_sum(s);
  m = trpo_block_max(m);
  if (t == 0) { a.part[2 * blockIdx.x] = s; a.part[2 * blockIdx.x + 1] = m; }
}
// part[blk] = p.z over the block's range (it < 0: whatever the flags say -- the closing product x.F(x))
__global__ __launch_bounds__(256) void trpo_dot_kernel(TrpoVecArgs a) {
  TRPO_LANES(t, nt);
  if (a.it >= 0 ? a.dev->done[a.it] : a.dev->zero_grad) return;
  int64_t lo, hi;
  trpo_range(a.n, lo, hi);
  float s = 0.f;
  for (int64_t i = lo + t; i < hi; i += nt) s += a.p[i] * a.z[i];
  s = trpo_block_sum(s);
  if (t == 0) a.part[blockIdx.x] = s;
}
// alpha = rr / p.z; x += alpha p; r -= alpha z; part2[blk] = r.r
__global__ __launch_bounds__(256) void trpo_cg_x_kernel(TrpoVecArgs a) {
  TRPO_LANES(t, nt);
  if (a.dev->done[a.it]) return;
  const float alpha = a.dev->rr[a.it] / trpo_sum_parts(a.part, a.n_part);
  int64_t lo, hi;
  trpo_range(a.n, lo, hi);
  float s = 0.f;
  for (int64_t i = lo + t; i < hi; i += nt) {
    a.x[i] += alpha * a.p[i];
    const float rv = a.r[i] - alpha * a.z[i];
    a.r[i] = rv;
    s += rv * rv;
  }
  s = trpo_block_sum(s);
  if (t == 0) a.part2[blockIdx.x] = s;
}
// p = r + (rr' / rr) p; workgroup 0 leaves rr' and the flag of the next iteration (no launch reads what it writes)
__global__ __launch_bounds__(256) void trpo_cg_p_kernel(TrpoVecArgs a) {
  TRPO_LANES(t, nt);
  TrpoDev* d = a.dev;
  if (d->done[a.it]) {
    if (blockIdx.x == 0 && t == 0) { d->done[a.it + 1] = 1; d->rr[a.it + 1] = d->rr[a.it]; }
    return;
  }
  const float rr = d->rr[a.it], rr2 = trpo_sum_parts(a.part2, a.n_part), mu = rr2 / rr;
  int64_t lo, hi;
  trpo_range(a.n, lo, hi);
  for (int64_t i = lo + t; i < hi; i += nt) a.p[i] = a.r[i] + mu * a.p[i];
  if (blockIdx.x == 0 && t == 0) {
    d->rr[a.it + 1] = rr2;
    d->done[a.it + 1] = rr2 < 1e-10f ? 1 : 0;
    d->cg_iters = a.it + 1;
  }
}
// dst = src (p = x in front of the closing product)
__global__ __launch_bounds__(256) void trpo_copy_kernel(float* dst, const float* src, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = src[i];
}
// z += damping * v; logstd entries: z = 2 v + damping * v
__global__ __launch_bounds__(256) void trpo_fvp_fin_kernel(TrpoVecArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
    const float v = a.v[i];
    const float f = (i >= a.ls_off && i < a.ls_off + a.A) ? 2.0f * v : a.z[i];
    a.z[i] = f + a.damping * v;
  }
}
// shs = 0.5 x.F(x) from part; fullstep = x / sqrt(|shs| / max_kl)
__global__ __launch_bounds__(256) void trpo_step_kernel(TrpoVecArgs a) {
  if (a.dev->zero_grad) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) a.full[i] = 0.f;
    return;
  }
  const float shs = 0.5f * trpo_sum_parts(a.part, a.n_part);
  const float lm = sqrtf(fabsf(shs) / a.max_kl);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) a.full[i] = a.x[i] / lm;
  if (blockIdx.x == 0 && threadIdx.x == 0) { a.dev->shs = shs; a.dev->lm = lm; }
}
// x: parameters, r: theta_old.  it 0: snapshot; 1: theta' = theta_old + scale * fullstep unless a trial was accepted;
// 2: restore unless a trial was accepted
__global__ __launch_bounds__(256) void trpo_theta_kernel(TrpoVecArgs a) {
  if (a.it && (a.dev->ls_accepted || (a.it == 1 && a.dev->zero_grad))) return;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
    if (a.it == 0) a.r[i] = a.x[i];
    else if (a.it == 2) a.x[i] = a.r[i];
    else {
      const float f = a.full[i];
      a.x[i] = f != 0.f ? a.r[i] + a.scale * f : a.r[i];      // (entries of the value variables keep their bits)
    }
  }
}

// grid (n): Fisher row b is rollout row b * stride
__global__ __launch_bounds__(256) void trpo_gather_kernel(const float* r_obs, float* x, int ldo, int stride, int n) {
  const int b = blockIdx.x;
  if (b >= n) return;
  for (int i = threadIdx.x; i < ldo; i += 256) x[(long)b * ldo + i] = r_obs[(long)b * stride * ldo + i];
}
// d mean((v - ret)^2) / d v over one value minibatch; closes the update the gather opened (PpoDev.cursor)
__global__ __launch_bounds__(256) void trpo_vf_loss_kernel(const float* v, int ld_v, const float* ret, float* dv, int ld_dv, int mb, PpoDev* dev) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < mb) dv[(long)b * ld_dv] = 2.0f * (v[(long)b * ld_v] - ret[b]) / (float)mb;
  if (b == 0) dev->cursor = dev->cur + 1;
}
#endif  // GRL_TRPO_TYPES_ONLY

// the launches (trpo.hip)
void launch_trpo_prep(const TrpoPrepArgs& a, hipStream_t s);
void launch_trpo_loss(const TrpoLossArgs& a, hipStream_t s);
void launch_trpo_scal(const TrpoScalArgs& a, hipStream_t s);
void launch_trpo_tan(const TrpoTanArgs& a, hipStream_t s);
enum { TRPO_V_CG_INIT = 0, TRPO_V_DOT, TRPO_V_CG_X, TRPO_V_CG_P, TRPO_V_FVP_FIN, TRPO_V_STEP, TRPO_V_THETA };
void launch_trpo_vec(int kind, const TrpoVecArgs& a, hipStream_t s);
void launch_trpo_copy(float* dst, const float* src, int64_t n, hipStream_t s);
void launch_trpo_gather(const float* r_obs, float* x, int ldo, int stride, int n, hipStream_t s);
void launch_trpo_vf_loss(const float* v, int ld_v, const float* ret, float* dv, int ld_dv, int mb, PpoDev* dev, hipStream_t s);

}  // namespace grl
