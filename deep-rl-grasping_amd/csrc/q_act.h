// q_act.h -- the ACT path of the DQN / BDQ networks as ONE launch that ends in the chosen bins (grl_act with GRL_ACT_GREEDY:
// stable-baselines DQN.learn's `self.act(...)` as entered from manipulation_main/training/sb_helper.py:159-177
// and :202-226, `model.predict` in manipulation_main/utils.py:71).
//
// The Q-value path of grl_act (plan_q.inl) is an ingest launch, one GEMM launch per layer and dueling_kernel: six launches
// for config/gripper_grasp.yaml's [[64, 64], [32], [32]], all of them launch latency at 1 - 64 rows, and the whole Q table
// crosses the bus for an arg-max on the host.  Here
//   * grid (rows / 16, D): a workgroup owns 16 observations -- the M of a 16x16x4 MFMA -- and ONE branch.  It runs the shared
//     trunk, then the branch's tower and the state-value tower side by side (two independent MFMA chains per barrier
//     interval), with the stage primitives of q_mfma.h: weights global -> registers, activations in LDS, and the operands of
//     EVERY stage -- plus the rows' observations and exploration overrides -- requested before the first stage runs (one
//     memory round trip per workgroup; the latency rules at the top of heads_mfma.h).  Trunk and value tower are recomputed
//     per branch (a few kFLOP): no workgroup waits for another one;
//   * q = v + adv - mean(adv) exactly as dueling_kernel forms it, arg-max over the bins with NumPy's rule (lowest index of
//     the largest value, a NaN counts as largest; the zero padding beyond the bins never takes part);
//   * explore[row, branch] >= 0 replaces the greedy bin (the HOST draws the randomness: seeds mean what they mean without
//     this kernel), the bins go to coherent host memory as float32 -- the type the replay ring stores -- and every workgroup
//     counts itself into the completion counter as dueling_kernel does: grl_act polls it.
// Observations and overrides are read from coherent host memory directly (a few hundred bytes per row): the call is a host
// memcpy, this launch and the poll -- no copy engine in front of it.
// GRL_ACT_RAW_OBS / GRL_ACT_OBSERVED (VecNormalize statistics on the device, observations uploaded once by grl_observe): the
// normalising instantiation reads RAW rows -- from the same host memory, or from the rows grl_observe left on the device -- and
// applies VecNormalize.normalize_obs while it stages them (norm_obs_act, elem_kernels.h: the float64 expression of the gather);
// its 2 x obs_dim doubles of statistics are requested with the observations, in front of every stage operand.
// Shapes outside qa_shape_ok (widths or bins above 64, observations above 128 values, more than 7 branches, more than
// GRL_MAX_LAYERS layers from observation to tower output) keep the launch list of the Q-value path and get q_select_kernel
// behind dueling_kernel.  The k-order of a stage is the MFMA's: bins agree with the arg-max of the Q-value path / the oracle
// wherever the two largest Q-values of a branch differ by more than float32 rounding of the forward pass.
#pragma once
#include "q_mfma.h"

namespace grl {

enum { QA_MAXD = QM_MAXP - 1, QA_MAXK = 2 * QM_W };

struct QActLayer { const float* w; const float* b; int n; };     // [k, n] kernel, [n] bias; k: width of the layer before (layer 0: obs_dim)
struct QActTower {
  QActLayer lay[GRL_MAX_LAYERS];   // hidden layers on top of the trunk (of the observation when there is no trunk)
  const float* ow; const float* ob;   // output layer [., bins] (value tower: [., 1])
  int L;
};
struct QActArgs {      // passed by value: the kernel reaches every weight pointer without a descriptor round trip
  const float* obs; int ld_obs, obs_dim, rows;     // [rows, ld_obs] normalised observations (coherent host memory)
  int Lc, D, nb;
  QActLayer trunk[GRL_MAX_LAYERS];
  QActTower tw[QA_MAXD + 1];       // [0, D): branches; [D]: state value
  const float* explore;            // [rows, D]: >= 0 overrides the greedy bin (coherent host memory)
  float* bins;                     // [rows, D] chosen bins as float32 (coherent host memory)
  unsigned* done;                  // completion counter, one increment per workgroup, or nullptr
};
// second argument of q_act_norm_kernel: `obs` holds RAW observations -- coherent host memory, or the rows grl_observe left on
// the device -- and VecNormalize.normalize_obs is applied while they are staged
struct QActNorm {
  const double* mean; const double* stdv;   // [obs_dim] running mean and sqrt(var + eps) (s_mean / s_std of the handle)
  double clip_obs;
};

// every hidden width of a DQN / BDQ network -- trunk, branch towers, value tower -- satisfies pred
template <class Pred> static inline bool q_hidden_widths_all(const grl_config& c, Pred pred) {
  const int* w[3] = {c.q_common, c.q_branch, c.q_value};
  const int n[3] = {c.q_n_common, c.q_n_branch, c.q_n_value};
  for (int s = 0; s < 3; ++s)
    for (int l = 0; l < n[s]; ++l)
      if (!pred(w[s][l])) return false;
  return true;
}

static inline bool qa_shape_ok(const grl_config& c) {
  const int Lc = c.q_n_common, Lb = c.q_n_branch, Lv = c.q_n_value;
  return c.obs_dim >= 1 && c.obs_dim <= QA_MAXK && c.q_branches >= 1 && c.q_branches <= QA_MAXD && c.q_bins >= 1 && c.q_bins <= QM_W &&
         Lb >= 1 && Lv >= 1 && Lc >= 0 && Lc + (Lb > Lv ? Lb : Lv) <= GRL_MAX_LAYERS &&
         q_hidden_widths_all(c, [](int w) { return w >= 1 && w <= QM_W; });
}

#ifndef GRL_HEADS_TYPES_ONLY

// NumPy's arg-max step: the first largest value wins, a NaN counts as largest
__device__ __forceinline__ bool qa_better(float val, float best) { return val > best || (val != val && best == best); }

// the fallback behind dueling_kernel: arg-max + override over the Q-values [rows, D, n] the launch list left on the device
__global__ __launch_bounds__(256) void q_select_kernel(const float* qv, int rows, int D, int n, const float* explore, float* bins,
                                                      unsigned* done) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < rows * D) {
    const float* a = qv + (long)i * n;
    int best = 0;
    for (int k = 1; k < n; ++k)
      if (qa_better(a[k], a[best])) best = k;
    const float e = explore[i];
    bins[i] = e >= 0.f ? e : (float)best;
  }
#ifndef GRL_HOSTEMU
  if (done) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
#else
  if (done && threadIdx.x == 0) *done += 1u;
#endif
}

#ifdef GRL_HOSTEMU
#include "q_act_ref1.h"   // tests/hostemu: the emulation build only
#include "q_act_ref2.h"
#else

struct __attribute__((aligned(16))) QaLds {
  float x[2][HT_RB][QM_LD];     // the rows' observations, two 64-wide chunks, zero beyond obs_dim
  float za[2][HT_RB][QM_LD];    // activations of the trunk, then of the branch tower
  float zv[2][HT_RB][QM_LD];    // activations of the value tower
  float q[HT_RB][QM_LD];        // advantages of the branch, zero beyond the bins
  float v[HT_RB];
};

// NORM: the observations are raw.  The 2 x 8 float64 statistics of the thread's eight staged values are requested with the
// observations, in front of every stage operand (one round trip for all of it), and norm_obs_act -- the expression of the gather
// and of act_ingest_kernel -- runs on the values once the weight loads are in flight, before they are staged in LDS.
// The kernel is a template over its trailing parameters -- none (q_act_kernel_t<>, the code the kernel always had), or one
// QActNorm (q_act_kernel_t<QActNorm>; the emulation build names the two q_act_kernel / q_act_norm_kernel) -- so that the plain instantiation's argument list and body stay exactly what they were.
__device__ __forceinline__ const QActNorm* qa_norm_of() { return nullptr; }
__device__ __forceinline__ const QActNorm* qa_norm_of(const QActNorm& nm) { return &nm; }
template <class... NM>
__global__ __launch_bounds__(256) void q_act_kernel_t(QActArgs a, NM... nm_) {
  constexpr bool NORM = sizeof...(NM) > 0;
  const QActNorm* const nm = qa_norm_of(nm_...);
  __shared__ QaLds s;
  const int t = threadIdx.x, w = t >> 6, l = t & 63, c = l & 15, q = l >> 4;
  const int n = 16 * w + c, row0 = blockIdx.x * HT_RB, rows = a.rows, br = blockIdx.y, Lc = a.Lc, K0 = a.obs_dim, nb = a.nb;
  const QActTower& TA = a.tw[br];
  const QActTower& TV = a.tw[a.D];
  const int LA = Lc + TA.L, LV = Lc + TV.L;      // layers from the observation to the tower's last hidden layer
  // ---- the rows' observations and overrides (host memory: the longest round trip, requested first)
  const int xr = t >> 4, xrow = row0 + xr;
  float xv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int col = (t & 15) + 16 * j;
    xv[j] = (xrow < rows && col < K0) ? QM_G(a.obs)[(long)xrow * a.ld_obs + col] : 0.f;
  }
  double xm[NORM ? 8 : 1], xs[NORM ? 8 : 1];
  if (NORM) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = (t & 15) + 16 * j;
      xm[j] = col < K0 ? nm->mean[col] : 0.0;
      xs[j] = col < K0 ? nm->stdv[col] : 1.0;
    }
  }
  float ex = -1.f;
  if (t < HT_RB && row0 + t < rows) ex = QM_G(a.explore)[(long)(row0 + t) * a.D + br];
  // ---- every operand of both chains.  Layer li < Lc is the trunk's (chain A carries it, the value tower reads its output)
  float wa[GRL_MAX_LAYERS][QM_KS], wv[GRL_MAX_LAYERS][QM_KS], wa0[QM_KS], wv0[QM_KS], oa[QM_KS], ov[QM_KS];
  float ba[GRL_MAX_LAYERS], bv[GRL_MAX_LAYERS];
  int na[GRL_MAX_LAYERS], nv[GRL_MAX_LAYERS];    // widths of the activations behind layer li
#pragma unroll
  for (int li = 0; li < GRL_MAX_LAYERS; ++li) {
    na[li] = nv[li] = 0;
    if (li < LA) {
      const QActLayer& y = li < Lc ? a.trunk[li] : TA.lay[li - Lc];
      const int K = li == 0 ? K0 : na[li > 0 ? li - 1 : 0];
      qm_load_b(wa[li], y.w, K, y.n, y.n, 1, n, q);
      if (li == 0) qm_load_b(wa0, y.w + (long)QM_W * y.n, K - QM_W, y.n, y.n, 1, n, q);
      ba[li] = n < y.n ? QM_G(y.b)[n] : 0.f;
      na[li] = y.n;
    }
    if (li < Lc) nv[li] = na[li];
    else if (li < LV) {
      const QActLayer& y = TV.lay[li - Lc];
      const int K = li == 0 ? K0 : nv[li > 0 ? li - 1 : 0];
      qm_load_b(wv[li], y.w, K, y.n, y.n, 1, n, q);
      if (li == 0) qm_load_b(wv0, y.w + (long)QM_W * y.n, K - QM_W, y.n, y.n, 1, n, q);
      bv[li] = n < y.n ? QM_G(y.b)[n] : 0.f;
      nv[li] = y.n;
    }
  }
  int ka = 0, kv = 0;
#pragma unroll
  for (int li = 0; li < GRL_MAX_LAYERS; ++li) {
    if (li == LA - 1) ka = na[li];
    if (li == LV - 1) kv = nv[li];
  }
  qm_load_b(oa, TA.ow, ka, nb, nb, 1, n, q);
  qm_load_b(ov, TV.ow, kv, 1, 1, 1, n, q);
  const float boa = n < nb ? QM_G(TA.ob)[n] : 0.f, bov = n < 1 ? QM_G(TV.ob)[0] : 0.f;
  if (NORM) {      // (rows beyond `rows` and columns beyond obs_dim stay the zeros they were loaded as)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (xrow < rows && (t & 15) + 16 * j < K0) xv[j] = norm_obs_act(xv[j], xm[j], xs[j], nm->clip_obs);
  }
  // ---- stage the observations (every element of both chunks is written: nothing to clear)
#pragma unroll
  for (int j = 0; j < 8; ++j) s.x[j >> 2][xr][(t & 15) + 16 * (j & 3)] = xv[j];
  __syncthreads();
  // ---- hidden layers: the branch chain (trunk first) and, from the trunk's end on, the value chain beside it
#pragma unroll
  for (int li = 0; li < GRL_MAX_LAYERS; ++li) {
    const bool do_a = li < LA, do_v = li >= Lc && li < LV;
    if (do_a || do_v) {
      qm_f4 ha = {0.f, 0.f, 0.f, 0.f}, hv = {0.f, 0.f, 0.f, 0.f};
      if (do_a) {
        ha = qm_mma(li == 0 ? s.x[0] : s.za[(li - 1) & 1], wa[li], c, q);
        if (li == 0) ha = qm_mma(s.x[1], wa0, c, q, ha);
      }
      if (do_v) {
        hv = qm_mma(li == 0 ? s.x[0] : (li == Lc ? s.za[(li - 1) & 1] : s.zv[(li - 1) & 1]), wv[li], c, q);
        if (li == 0) hv = qm_mma(s.x[1], wv0, c, q, hv);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (do_a) s.za[li & 1][4 * q + i][n] = n < na[li] ? fmaxf(ha[i] + ba[li], 0.f) : 0.f;
        if (do_v) s.zv[li & 1][4 * q + i][n] = n < nv[li] ? fmaxf(hv[i] + bv[li], 0.f) : 0.f;
      }
      __syncthreads();
    }
  }
  // ---- advantages of the branch, state value
  {
    const qm_f4 qa = qm_mma(s.za[(LA - 1) & 1], oa, c, q), qs = qm_mma(s.zv[(LV - 1) & 1], ov, c, q);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s.q[4 * q + i][n] = n < nb ? qa[i] + boa : 0.f;
      if (n == 0) s.v[4 * q + i] = qs[i] + bov;
    }
  }
  __syncthreads();
  // ---- dueling combination + arg-max + override: one thread per row, the row's advantages in registers
  if (t < HT_RB) {
    float av[QM_W];
#pragma unroll
    for (int j = 0; j < QM_W / 4; ++j) {
      const qm_f4 v4 = *(const qm_f4*)&s.q[t][4 * j];
      av[4 * j] = v4.x; av[4 * j + 1] = v4.y; av[4 * j + 2] = v4.z; av[4 * j + 3] = v4.w;
    }
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < QM_W; ++k)
      if (k < nb) m += av[k];
    m /= (float)nb;
    const float v = s.v[t];
    float best_q = v + av[0] - m;
    int best = 0;
#pragma unroll
    for (int k = 1; k < QM_W; ++k)
      if (k < nb) {
        const float val = v + av[k] - m;
        if (qa_better(val, best_q)) { best_q = val; best = k; }
      }
    const int row = row0 + t;
    if (row < rows) QM_GW(a.bins)[(long)row * a.D + br] = ex >= 0.f ? ex : (float)best;
  }
  // ---- tell the host (as dueling_kernel / act_mfma.h do): stores out, a barrier, one increment per workgroup
  if (a.done) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(a.done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

#endif  // GRL_HOSTEMU
#endif  // GRL_HEADS_TYPES_ONLY

}  // namespace grl
