// ppo_kernels.h -- the kernels PPO2 adds to the engine (plan_ppo.inl; stable-baselines 2.10.1 ppo2.py, common/policies.py and
// common/distributions.py restated): gfx950, float32, VALU, no atomics.  The dense products of the two towers stay on the igemm
// launches; what lives here is everything around them:
//
//   ppo_act_kernel      model.step / model.value / model.predict as ONE launch for observations up to 2048 values and widths up to
//                       256 (the limits of act_heads_kernel, whose layer loop is the model): one workgroup per (row, tower), partial
//                       sums meet in LDS, tanh between the layers, then mean -> sample -> neglogp (pi) or the value (vf), written
//                       straight into the rollout slot.  The call is latency bound and a rollout makes n_steps of them.
//   ppo_sample_kernel   the same tail behind the per-layer launch list (other shapes, GRL_TUNE ppo_act=0)
//   ppo_rewards_kernel  rewards into the open slot; closes it (the slot counter lives in device memory: captured graphs stay valid)
//   gae_kernel          one lane per environment scanning t backwards; every operation rounded to float32 in the order of
//                       Runner.run (no contraction: the test demands the bits of a NumPy float32 restatement)
//   ppo_gather_kernel   the minibatch's rows by permutation index -- observations into the towers' input buffer, the per-row scalars --
//                       and, in one more workgroup, mean and population standard deviation of the advantages (two passes, fixed
//                       summation tree) + the Adam step size of the update.  It finds its slice of `perm` through the update cursor
//                       in device memory, so every update of a call is the same launch list.
//   tanh_fwd / tanh_bwd all tensors of one layer level in one launch through a descriptor table (LnDesc of ln_kernels.h is the
//                       model); 16-byte accesses over the dense buffers, scalar tail.  The forward also adds the partial sums of a
//                       split-K first layer, in index order, and its bias.
//   ppo_loss_kernel     row-local: one lane per row, a loop over the action components.  d mean, d v, per-block slabs of d logstd
//                       (summed into the bucket by a reduction descriptor, as every other gradient) and per-block sums of the
//                       diagnostics (added in index order by grl_ppo_get_metrics).
//   ppo_observe_kernel  normalize = 2 handles: RunningMeanStd.update over one env step's raw observations and the normalised rows
//                       the act path reads, in one launch (the arithmetic of elem_kernels.h: norm_batch_moments, norm_chan_merge,
//                       norm_obs_act)
//
// Every batch sum leaves as per-block slabs and is added in index order, as ln_kernels.h does for dbeta / dgamma.
#pragma once
#ifdef GRL_HOSTEMU
#include "hostemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <cmath>
#include "elem_kernels.h"

namespace grl {

#define PPO_MAX_A 64          /* action components (check_cfg: act_dim <= 64) */
#define PPO_LOSS_ROWS 256     /* rows per workgroup of the loss launch: one lane each */
#define PPO_DIAG 5            /* per-block sums of an update: pg rows, vf rows, entropy (block 0), approxkl rows, clipped rows */
enum { PPO_ACT_MAX_IN = 2048, PPO_ACT_MAX_HID = 256 };     // the shapes ppo_act_kernel covers (ACT_HEADS_MAX_IN / _HID)

// device words of a PPO handle (state arena)
struct PpoDev {
  int32_t slot;       // rollout slots closed so far == the slot grl_ppo_step writes
  int32_t cursor;     // minibatch of the running grl_ppo_train call the next gather takes (reset by the call)
  int32_t cur;        // the update the launches behind the gather belong to: written by the gather, read by the loss launch
  int32_t pad;
  float adv_mean, adv_sd;      // of the gathered minibatch: mean, population standard deviation + 1e-8
};

// ---------------------------------------------------------------------------------------------------------------- policy tail
struct PpoSampleArgs {
  const float* mean; int ld_mean;      // [n, A]          (launch-list route; ppo_act_kernel hands its own)
  const float* v; int ld_v;            // [n]
  const float* logstd;                 // [A]
  const float* eps;                    // [n, A] standard normals, or nullptr: Philox (cfg.seed, DevScalars.rng_step)
  const float* x; int ldx;             // [n, ldx] the observations acted on
  const float* done_in;                // [n] flags from before the step (mode 1, 2)
  float *r_obs, *r_act, *r_val, *r_nlp, *r_done;      // rollout, row = env * n_steps + t
  int ldo, n_steps;
  const PpoDev* dev;
  const DevScalars* sc;
  uint64_t seed;
  float *out_act, *out_val, *out_nlp;  // [n, A], [n], [n]
  float *last_v, *last_done;           // [n] (mode 2)
  int n, A, obs_dim;
  int mode;                            // 0 act (records nothing), 1 step (slot dev->slot of the rollout), 2 finish (last values)
  int deterministic;
};

__device__ __forceinline__ float ppo_half_log_2pi() { return 0.91893853320467274f; }

// the policy half of row r: a = mean + exp(logstd) * eps (or the mean), neglogp(a); one thread
__device__ __forceinline__ void ppo_emit_pi(const PpoSampleArgs& a, int r, const float* mean) {
  const int slot = a.dev->slot;
  const bool rec = a.mode == 1 && slot < a.n_steps;
  const long row = (long)r * a.n_steps + slot;
  const uint64_t step = a.sc->rng_step;
  float q = 0.f, sl = 0.f;
  for (int j0 = 0; j0 < a.A; j0 += 2) {
    float e[2] = {0.f, 0.f};
    if (!a.deterministic) {
      if (a.eps) { e[0] = a.eps[(long)r * a.A + j0]; if (j0 + 1 < a.A) e[1] = a.eps[(long)r * a.A + j0 + 1]; }
      else normal_pair_draw(a.seed, step, r, j0, e[0], e[1]);
    }
    for (int k = 0; k < 2 && j0 + k < a.A; ++k) {
      const int j = j0 + k;
      const float ls = a.logstd[j], sd = expf(ls);
      const float act = a.deterministic ? mean[j] : mean[j] + sd * e[k];
      const float u = (act - mean[j]) / sd;
      q += u * u;
      sl += ls;
      a.out_act[(long)r * a.A + j] = act;
      if (rec) a.r_act[row * a.A + j] = act;
    }
  }
  const float nlp = 0.5f * q + ppo_half_log_2pi() * (float)a.A + sl;
  a.out_nlp[r] = nlp;
  if (rec) a.r_nlp[row] = nlp;
}
// the value half of row r; one thread
__device__ __forceinline__ void ppo_emit_v(const PpoSampleArgs& a, int r, float v) {
  const int slot = a.dev->slot;
  a.out_val[r] = v;
  if (a.mode == 1 && slot < a.n_steps) {
    const long row = (long)r * a.n_steps + slot;
    a.r_val[row] = v;
    a.r_done[row] = a.done_in[r];
  }
  if (a.mode == 2) { a.last_v[r] = v; a.last_done[r] = a.done_in[r]; }
}

struct PpoTower {
  const float* w[GRL_MAX_LAYERS]; const float* b[GRL_MAX_LAYERS]; int hid[GRL_MAX_LAYERS]; int L;
  const float* ow; const float* ob; int out;
};
struct PpoActArgs {
  PpoTower tw[2];      // 0 pi, 1 vf
  PpoSampleArgs s;     // (mean / v are not read: the launch forms them)
};

// ---------------------------------------------------------------------------------------------------------------- GAE
struct GaeArgs {
  const float *rew, *val, *done, *last_v, *last_done;      // rollout [n_envs * n_steps], row = env * n_steps + t; [n_envs]
  float *adv, *ret;
  int n_envs, n_steps;
  float gamma, c;      // c = float32(gamma * lam), the product formed in double
};
// environment e, t = n_steps - 1 ... 0: every operation rounded to float32, nothing contracted
__device__ __forceinline__ void gae_env(const GaeArgs& a, int e) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  float last = 0.f;
  for (int t = a.n_steps - 1; t >= 0; --t) {
    const long i = (long)e * a.n_steps + t;
    const bool end = t == a.n_steps - 1;
    const float nnt = 1.0f - (end ? a.last_done[e] : a.done[i + 1]);
    const float nv = end ? a.last_v[e] : a.val[i + 1];
    const float v = a.val[i];
    const float g = a.gamma * nv;
    const float gn = g * nnt;
    const float s = gn + a.rew[i];
    const float delta = s - v;
    const float cn = a.c * nnt;
    const float cl = cn * last;
    last = cl + delta;
    a.adv[i] = last;
    a.ret[i] = last + v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- gather
struct PpoGatherArgs {
  const int32_t* perm;      // [noptepochs * R]: update u of the call takes perm[u * mb, (u + 1) * mb)
  PpoDev* dev;
  DevScalars* sc;
  const float* r_obs; int ldo;      // rollout observations [R, ldo] (ldo a multiple of 4)
  const float *r_act, *r_oldv, *r_oldnlp, *r_adv, *r_ret;
  float* x;                         // [mb, ldo]
  float *act, *oldv, *oldnlp, *adv, *ret;
  int mb, A;
};

// ---------------------------------------------------------------------------------------------------------------- tanh
struct TanhDesc {
  float* z;                 // forward: [rows, H] pre-activations in (unless `parts`), activations out; backward: activations (read)
  const float* parts;       // forward: n_parts partial sums [n_parts][rows, H] of a split-K product, added in index order, + bias
  const float* bias;        // [H], with parts
  float* dz;                // backward: [rows, H] gradient w.r.t. z in, w.r.t. the pre-activation out
  int64_t part_stride;
  int32_t n_parts, H;
};
__device__ __forceinline__ float tanh_fwd_elem(const TanhDesc& d, long i, long n) {
  if (!d.parts) return tanhf(d.z[i]);
  float s = d.parts[i];
  for (int k = 1; k < d.n_parts; ++k) s += d.parts[(long)k * d.part_stride + i];
  (void)n;
  return tanhf(s + d.bias[i % d.H]);
}
__device__ __forceinline__ float tanh_bwd_elem(float dz, float z) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return dz * (1.0f - z * z);
}

// ---------------------------------------------------------------------------------------------------------------- loss
struct PpoLossArgs {
  const float* mean; int ld_mean;      // [mb, A]
  const float* logstd;                 // [A]
  const float* v; int ld_v;            // [mb]
  const float *act, *oldv, *oldnlp, *adv, *ret;      // the gathered scalars
  PpoDev* dev;
  float* dmean; int ld_dm;             // [mb, ld_dm]
  float* dv; int ld_dv;                // [mb, ld_dv]
  float* dls_slab;                     // [blocks, A]; block 0 also carries the entropy term's -ent_coef per component
  float* diag;                         // [updates, blocks, PPO_DIAG]
  int mb, A;
  float clip, clip_vf, ent_coef, vf_coef;
};
inline int ppo_loss_blocks(int mb) { return (mb + PPO_LOSS_ROWS - 1) / PPO_LOSS_ROWS; }

struct PpoRow { float g_nlp, pg, vf, kl, cf; };
// row b: losses, diagnostics, d v, and g_nlp = d loss / d neglogp(b)
__device__ __forceinline__ PpoRow ppo_loss_row(const PpoLossArgs& a, int b) {
  const float inv_mb = 1.0f / (float)a.mb;
  float q = 0.f, sl = 0.f;
  for (int j = 0; j < a.A; ++j) {
    const float ls = a.logstd[j];
    const float u = (a.act[(long)b * a.A + j] - a.mean[(long)b * a.ld_mean + j]) / expf(ls);
    q += u * u;
    sl += ls;
  }
  const float nlp = 0.5f * q + ppo_half_log_2pi() * (float)a.A + sl;
  const float old = a.oldnlp[b];
  const float ratio = expf(old - nlp);
  const float adv_n = (a.adv[b] - a.dev->adv_mean) / a.dev->adv_sd;
  const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
  const float l1 = -adv_n * ratio, l2 = -adv_n * fminf(fmaxf(ratio, lo), hi);
  PpoRow r;
  r.pg = l1 >= l2 ? l1 : l2;
  // max sends its gradient to l1 where l1 >= l2; clip passes gradient inside and on its bounds
  const float dratio = l1 >= l2 ? -adv_n : ((ratio >= lo && ratio <= hi) ? -adv_n : 0.f);
  r.g_nlp = inv_mb * dratio * -ratio;
  const float v = a.v[(long)b * a.ld_v], ov = a.oldv[b], rt = a.ret[b];
  const float e1 = (v - rt) * (v - rt);
  float dvf = 2.0f * (v - rt);
  r.vf = e1;
  if (a.clip_vf >= 0.f) {
    const float dlt = v - ov;
    const float vc = ov + fminf(fmaxf(dlt, -a.clip_vf), a.clip_vf);
    const float e2 = (vc - rt) * (vc - rt);
    if (!(e1 >= e2)) { r.vf = e2; dvf = (dlt >= -a.clip_vf && dlt <= a.clip_vf) ? 2.0f * (vc - rt) : 0.f; }
  }
  a.dv[(long)b * a.ld_dv] = a.vf_coef * 0.5f * inv_mb * dvf;
  r.kl = (nlp - old) * (nlp - old);
  r.cf = fabsf(ratio - 1.0f) > a.clip ? 1.f : 0.f;
  return r;
}
// component j of row b: writes d mean, returns the row's share of d logstd
__device__ __forceinline__ float ppo_loss_row_j(const PpoLossArgs& a, int b, int j, float g_nlp) {
  const float sd = expf(a.logstd[j]);
  const float u = (a.act[(long)b * a.A + j] - a.mean[(long)b * a.ld_mean + j]) / sd;
  a.dmean[(long)b * a.ld_dm + j] = g_nlp * (-u / sd);
  return g_nlp * (1.0f - u * u);
}
__device__ __forceinline__ float ppo_entropy(const PpoLossArgs& a) {
  float e = 0.f;
  for (int j = 0; j < a.A; ++j) e += a.logstd[j] + 1.4189385332046727f;      // 0.5 * log(2 pi e)
  return e;
}

// ---------------------------------------------------------------------------------------------------------------- observe
// VecNormalize observation statistics of a normalize = 2 handle (grl_observe): stable-baselines normalises a PPO observation ONCE,
// at step time, with the statistics as they stand right after that step's RunningMeanStd.update -- the normalised row is what the
// rollout stores -- so one launch per env step does both.  One thread owns element e of the flattened observation:
//   update = 1   norm_update_kernel's work (float32 batch moments over the n staged rows in row order, the float64 Chan merge with
//                `batch_var * n` a float32 product; mean, var, sqrt(var + eps) stored; count double buffered by parity), then
//   every call   out[i, e] = norm_obs_act(x[i, e], mean, sd, clip) for every row with the statistics just formed (update = 0: the
//                stored ones); columns [elems, ldo) of `out` are written zero.  A NaN observation stays a NaN (np.clip leaves it).
// A raw element is fetched from HBM by the first pass over its column; the second pass of the moments and the normalising pass hit
// L2 (n_envs x obs_dim floats: 512 KiB at 16 x 8192).  The arithmetic is elem_kernels.h's, one copy.  Compiles as it stands in
// the emulation build, like norm_update_kernel.
struct PpoObserveArgs {
  NormUpdateArgs nu;      // obs: the raw staged rows [n, elems]; mean, var, count, parity, eps (the derived arrays and image fields: unused)
  double* sd;             // [elems] sqrt(var + eps)
  float* out; int ldo;    // [n, ldo]
  double clip;
  int update;
};

#ifndef GRL_PPO_TYPES_ONLY
__global__ __launch_bounds__(256) void ppo_observe_kernel(PpoObserveArgs a) {
  const NormUpdateArgs& u = a.nu;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.ldo) return;
  if (e >= u.elems) {
    for (int i = 0; i < u.n; ++i) a.out[(long)i * a.ldo + e] = 0.f;
    return;
  }
  double mean = u.mean[e], sd;
  if (a.update) {
    double cnt = u.count[u.parity], var = u.var[e];
    float bm, bv;
    norm_batch_moments(u, e, bm, bv);
    norm_chan_merge(mean, var, cnt, bm, bv, u.n, true);
    sd = sqrt(var + u.eps);
    u.mean[e] = mean;
    u.var[e] = var;
    a.sd[e] = sd;
    if (e == 0) u.count[u.parity ^ 1] = cnt;
  } else {
    sd = a.sd[e];
  }
  for (int i = 0; i < u.n; ++i) a.out[(long)i * a.ldo + e] = norm_obs_act(u.obs[(long)i * u.elems + e], mean, sd, a.clip);
}
#endif

#ifndef GRL_PPO_TYPES_ONLY
#ifdef GRL_HOSTEMU
#include "ppo_kernels_ref1.h"   // tests/hostemu: the emulation build only
#else
typedef float ppo_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float ppo_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// sum over the 256 threads of a workgroup, fixed tree: the same bits whatever the schedule
__device__ __forceinline__ float ppo_block_sum(float v, float* red) {
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

// one dense layer of one row inside a workgroup: thread t owns output t % Np over the input slice t / Np (act_heads_layer)
__device__ inline void ppo_act_layer(const float* in, int K, const float* w, const float* b, int N, int act_tanh, float* part, float* outv) {
  int Np = 1;
  while (Np < N) Np <<= 1;
  const int S = 256 / Np, t = threadIdx.x, o = t % Np, q = t / Np;
  float acc = 0.f;
  if (o < N)
    for (int i = q; i < K; i += S) acc = fmaf(in[i], w[(long)i * N + o], acc);
  part[t] = acc;
  __syncthreads();
  if (t < N) {
    float v = b[t];
    for (int j = 0; j < S; ++j) v += part[j * Np + t];
    outv[t] = act_tanh ? tanhf(v) : v;
  }
  __syncthreads();
}

// grid (rows, 2): tower blockIdx.y of row blockIdx.x
__global__ __launch_bounds__(256) void ppo_act_kernel(PpoActArgs a) {
  __shared__ float xs[PPO_ACT_MAX_IN];
  __shared__ float hs[2][PPO_ACT_MAX_HID];
  __shared__ float part[256];
  __shared__ float o[PPO_MAX_A];
  const int r = blockIdx.x;
  const PpoSampleArgs& s = a.s;
  if (r >= s.n) return;
  const PpoTower& T = a.tw[blockIdx.y];
  for (int i = threadIdx.x; i < s.obs_dim; i += 256) xs[i] = s.x[(long)r * s.ldx + i];
  __syncthreads();
  const float* in = xs;
  int K = s.obs_dim;
  for (int l = 0; l < T.L; ++l) {
    ppo_act_layer(in, K, T.w[l], T.b[l], T.hid[l], 1, part, hs[l & 1]);
    in = hs[l & 1];
    K = T.hid[l];
  }
  ppo_act_layer(in, K, T.ow, T.ob, T.out, 0, part, o);
  if (blockIdx.y == 0) {
    const int slot = s.dev->slot;
    if (s.mode == 1 && slot < s.n_steps) {      // the observation into its rollout row (padding columns stay zero)
      float* dst = s.r_obs + ((long)r * s.n_steps + slot) * s.ldo;
      for (int i = threadIdx.x; i < s.obs_dim; i += 256) dst[i] = xs[i];
    }
    if (threadIdx.x == 0 && s.mode != 2) ppo_emit_pi(s, r, o);
  } else if (threadIdx.x == 0) {
    ppo_emit_v(s, r, o[0]);
  }
}

// grid (rows): the tail alone, behind the launch list
__global__ __launch_bounds__(256) void ppo_sample_kernel(PpoSampleArgs s) {
  const int r = blockIdx.x;
  if (r >= s.n) return;
  const int slot = s.dev->slot;
  if (s.mode == 1 && slot < s.n_steps) {
    float* dst = s.r_obs + ((long)r * s.n_steps + slot) * s.ldo;
    for (int i = threadIdx.x; i < s.obs_dim; i += 256) dst[i] = s.x[(long)r * s.ldx + i];
  }
  if (threadIdx.x == 0 && s.mode != 2) ppo_emit_pi(s, r, s.mean + (long)r * s.ld_mean);
  if (threadIdx.x == 64) ppo_emit_v(s, r, s.v[(long)r * s.ld_v]);
}

// one workgroup
__global__ __launch_bounds__(256) void ppo_rewards_kernel(const float* rew_in, float* r_rew, PpoDev* dev, int n, int n_steps) {
  const int slot = dev->slot;
  if (slot < n_steps)
    for (int r = threadIdx.x; r < n; r += 256) r_rew[(long)r * n_steps + slot] = rew_in[r];
  __syncthreads();
  if (threadIdx.x == 0 && slot < n_steps) dev->slot = slot + 1;
}

__global__ __launch_bounds__(64) void gae_kernel(GaeArgs a) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e < a.n_envs) gae_env(a, e);
}

// grid (mb + 1): workgroup b < mb moves row b, workgroup mb forms the advantage statistics and opens the update
__global__ __launch_bounds__(256) void ppo_gather_kernel(PpoGatherArgs a) {
  __shared__ float red[256];
  const int t = threadIdx.x;
  const int b = blockIdx.x;
  const int32_t* perm = a.perm + (long)a.dev->cursor * a.mb;
  if (b < a.mb) {
    const long src = perm[b];
    const ppo_f4* from = (const ppo_f4*)(a.r_obs + src * a.ldo);
    ppo_f4* to = (ppo_f4*)(a.x + (long)b * a.ldo);
    for (int i = t; i < a.ldo / 4; i += 256) to[i] = from[i];
    if (t < a.A) a.act[(long)b * a.A + t] = a.r_act[src * a.A + t];
    if (t == 64) { a.oldv[b] = a.r_oldv[src]; a.oldnlp[b] = a.r_oldnlp[src]; }
    if (t == 128) { a.adv[b] = a.r_adv[src]; a.ret[b] = a.r_ret[src]; }
    return;
  }
  float s = 0.f;
  for (int i = t; i < a.mb; i += 256) s += a.r_adv[perm[i]];
  const float mean = ppo_block_sum(s, red) / (float)a.mb;
  float q = 0.f;
  for (int i = t; i < a.mb; i += 256) { const float d = a.r_adv[perm[i]] - mean; q += d * d; }
  const float var = ppo_block_sum(q, red) / (float)a.mb;
  if (t == 0) {
    a.dev->adv_mean = mean;
    a.dev->adv_sd = sqrtf(var) + 1e-8f;
    a.dev->cur = a.dev->cursor;
    adam_tick_device(a.sc);
  }
}

// grid (blocks, n_desc)
__global__ __launch_bounds__(256) void tanh_fwd_kernel(const TanhDesc* __restrict__ descs, int rows) {
  const TanhDesc d = descs[blockIdx.y];
  const long n = (long)rows * d.H;
  const long nq = (d.parts && (d.part_stride & 3)) ? 0 : n / 4;      // (partial sums a multiple of 4 floats apart: aligned quads)
  const long stride = (long)gridDim.x * 256, i0 = (long)blockIdx.x * 256 + threadIdx.x;
  for (long q = i0; q < nq; q += stride) {
    ppo_f4 y;
    if (!d.parts) {
      const ppo_f4 x = ((const ppo_f4*)d.z)[q];
      y = ppo_f4{tanhf(x.x), tanhf(x.y), tanhf(x.z), tanhf(x.w)};
    } else {
      ppo_f4 x = ((const ppo_f4*)d.parts)[q];
      for (int k = 1; k < d.n_parts; ++k) x += ((const ppo_f4*)(d.parts + (long)k * d.part_stride))[q];
      const long i = 4 * q;
      y = ppo_f4{tanhf(x.x + d.bias[i % d.H]), tanhf(x.y + d.bias[(i + 1) % d.H]), tanhf(x.z + d.bias[(i + 2) % d.H]),
                 tanhf(x.w + d.bias[(i + 3) % d.H])};
    }
    ((ppo_f4*)d.z)[q] = y;
  }
  for (long i = 4 * nq + i0; i < n; i += stride) d.z[i] = tanh_fwd_elem(d, i, n);
}
__global__ __launch_bounds__(256) void tanh_bwd_kernel(const TanhDesc* __restrict__ descs, int rows) {
  const TanhDesc d = descs[blockIdx.y];
  const long n = (long)rows * d.H, nq = n / 4;
  const long stride = (long)gridDim.x * 256, i0 = (long)blockIdx.x * 256 + threadIdx.x;
  for (long q = i0; q < nq; q += stride) {
    const ppo_f4 z = ((const ppo_f4*)d.z)[q], g = ((const ppo_f4*)d.dz)[q];
    ((ppo_f4*)d.dz)[q] = ppo_f4{tanh_bwd_elem(g.x, z.x), tanh_bwd_elem(g.y, z.y), tanh_bwd_elem(g.z, z.z), tanh_bwd_elem(g.w, z.w)};
  }
  for (long i = 4 * nq + i0; i < n; i += stride) d.dz[i] = tanh_bwd_elem(d.dz[i], d.z[i]);
}

// grid (ppo_loss_blocks(mb)): lane = row
__global__ __launch_bounds__(PPO_LOSS_ROWS) void ppo_loss_kernel(PpoLossArgs a) {
  __shared__ float ws[PPO_LOSS_ROWS / 64][PPO_MAX_A + PPO_DIAG];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int b = blockIdx.x * PPO_LOSS_ROWS + t;
  const bool live = b < a.mb;
  const int cur = a.dev->cur;
  PpoRow r = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) r = ppo_loss_row(a, b);
  for (int j = 0; j < a.A; ++j) {
    const float s = ppo_wave_sum(live ? ppo_loss_row_j(a, b, j, r.g_nlp) : 0.f);
    if (lane == 0) ws[w][j] = s;
  }
  const float dg[4] = {r.pg, r.vf, r.kl, r.cf};
  for (int k = 0; k < 4; ++k) {
    const float s = ppo_wave_sum(dg[k]);
    if (lane == 0) ws[w][a.A + k] = s;
  }
  __syncthreads();
  if (t < a.A + 4) {
    float s = ws[0][t];
    for (int k = 1; k < PPO_LOSS_ROWS / 64; ++k) s += ws[k][t];
    if (t < a.A) a.dls_slab[(long)blockIdx.x * a.A + t] = blockIdx.x == 0 ? s - a.ent_coef : s;
    else {
      float* dg_out = a.diag + ((long)cur * gridDim.x + blockIdx.x) * PPO_DIAG;
      const int k = t - a.A;      // pg, vf, kl, cf -> slots 0, 1, 3, 4
      dg_out[k < 2 ? k : k + 1] = s;
    }
  }
  if (t == PPO_LOSS_ROWS - 1) a.diag[((long)cur * gridDim.x + blockIdx.x) * PPO_DIAG + 2] = blockIdx.x == 0 ? ppo_entropy(a) : 0.f;
  if (blockIdx.x == 0 && t == 0) a.dev->cursor = cur + 1;      // (this launch reads `cur`, the gather `cursor`: no launch reads what it writes)
}
#endif
#endif  // GRL_PPO_TYPES_ONLY

// the launches (ppo.hip)
void launch_ppo_act(const PpoActArgs& a, hipStream_t s);
void launch_ppo_sample(const PpoSampleArgs& a, hipStream_t s);
void launch_ppo_rewards(const float* rew_in, float* r_rew, PpoDev* dev, int n, int n_steps, hipStream_t s);
void launch_gae(const GaeArgs& a, hipStream_t s);
void launch_ppo_gather(const PpoGatherArgs& a, hipStream_t s);
void launch_tanh_fwd(const TanhDesc* descs, int n_desc, int rows, int max_h, hipStream_t s);
void launch_tanh_bwd(const TanhDesc* descs, int n_desc, int rows, int max_h, hipStream_t s);
void launch_ppo_loss(const PpoLossArgs& a, hipStream_t s);
void launch_ppo_observe(const PpoObserveArgs& a, hipStream_t s);

}  // namespace grl
