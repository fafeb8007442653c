// ppo_kernels_ref1.h -- TEST-ONLY reference forms of the kernels of csrc/ppo_kernels.h: sequential loops over the same argument
// blocks, included by that header ONLY in the g++ emulation build (-DGRL_HOSTEMU -I tests/hostemu, tests/conftest.py).
// Never part of libgrl.so.  No include guard: it is pasted once, inside namespace grl.
//
// The row-local arithmetic (ppo_emit_pi / ppo_emit_v, gae_env, ppo_loss_row / ppo_loss_row_j, tanh_*_elem) is the header's own;
// what is restated here is the part a workgroup does together: the layer loop of ppo_act_kernel, the batch sums of the gather and
// the loss launch (plain sums in row order) and the element loops of the tanh launches.
inline void ppo_act_kernel(PpoActArgs a) {
  if (threadIdx.x != 0) return;
  const int r = blockIdx.x;
  const PpoSampleArgs& s = a.s;
  if (r >= s.n) return;
  const PpoTower& T = a.tw[blockIdx.y];
  float buf[2][PPO_ACT_MAX_IN];
  for (int i = 0; i < s.obs_dim; ++i) buf[0][i] = s.x[(long)r * s.ldx + i];
  int cur = 0, K = s.obs_dim;
  for (int l = 0; l < T.L; ++l) {
    for (int o = 0; o < T.hid[l]; ++o) {
      float v = T.b[l][o];
      for (int i = 0; i < K; ++i) v += buf[cur][i] * T.w[l][(long)i * T.hid[l] + o];
      buf[cur ^ 1][o] = tanhf(v);
    }
    cur ^= 1;
    K = T.hid[l];
  }
  float out[PPO_MAX_A];
  for (int o = 0; o < T.out; ++o) {
    float v = T.ob[o];
    for (int i = 0; i < K; ++i) v += buf[cur][i] * T.ow[(long)i * T.out + o];
    out[o] = v;
  }
  if (blockIdx.y == 0) {
    const int slot = s.dev->slot;
    if (s.mode == 1 && slot < s.n_steps)
      for (int i = 0; i < s.obs_dim; ++i) s.r_obs[((long)r * s.n_steps + slot) * s.ldo + i] = s.x[(long)r * s.ldx + i];
    if (s.mode != 2) ppo_emit_pi(s, r, out);
  } else {
    ppo_emit_v(s, r, out[0]);
  }
}

inline void ppo_sample_kernel(PpoSampleArgs s) {
  if (threadIdx.x != 0) return;
  const int r = blockIdx.x;
  if (r >= s.n) return;
  const int slot = s.dev->slot;
  if (s.mode == 1 && slot < s.n_steps)
    for (int i = 0; i < s.obs_dim; ++i) s.r_obs[((long)r * s.n_steps + slot) * s.ldo + i] = s.x[(long)r * s.ldx + i];
  if (s.mode != 2) ppo_emit_pi(s, r, s.mean + (long)r * s.ld_mean);
  ppo_emit_v(s, r, s.v[(long)r * s.ld_v]);
}

inline void ppo_rewards_kernel(const float* rew_in, float* r_rew, PpoDev* dev, int n, int n_steps) {
  if (threadIdx.x != 0) return;
  const int slot = dev->slot;
  if (slot >= n_steps) return;
  for (int r = 0; r < n; ++r) r_rew[(long)r * n_steps + slot] = rew_in[r];
  dev->slot = slot + 1;
}

inline void gae_kernel(GaeArgs a) {
  const int e = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (e < a.n_envs) gae_env(a, e);
}

inline void ppo_gather_kernel(PpoGatherArgs a) {
  if (threadIdx.x != 0) return;
  const int b = blockIdx.x;
  const int32_t* perm = a.perm + (long)a.dev->cursor * a.mb;
  if (b < a.mb) {
    const long src = perm[b];
    for (int i = 0; i < a.ldo; ++i) a.x[(long)b * a.ldo + i] = a.r_obs[src * a.ldo + i];
    for (int j = 0; j < a.A; ++j) a.act[(long)b * a.A + j] = a.r_act[src * a.A + j];
    a.oldv[b] = a.r_oldv[src]; a.oldnlp[b] = a.r_oldnlp[src]; a.adv[b] = a.r_adv[src]; a.ret[b] = a.r_ret[src];
    return;
  }
  float s = 0.f;
  for (int i = 0; i < a.mb; ++i) s += a.r_adv[perm[i]];
  const float mean = s / (float)a.mb;
  float q = 0.f;
  for (int i = 0; i < a.mb; ++i) { const float d = a.r_adv[perm[i]] - mean; q += d * d; }
  a.dev->adv_mean = mean;
  a.dev->adv_sd = sqrtf(q / (float)a.mb) + 1e-8f;
  a.dev->cur = a.dev->cursor;
  adam_tick_device(a.sc);
}

inline void tanh_fwd_kernel(const TanhDesc* descs, int rows) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const TanhDesc d = descs[blockIdx.y];
  const long n = (long)rows * d.H;
  for (long i = 0; i < n; ++i) d.z[i] = tanh_fwd_elem(d, i, n);
}
inline void tanh_bwd_kernel(const TanhDesc* descs, int rows) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const TanhDesc d = descs[blockIdx.y];
  const long n = (long)rows * d.H;
  for (long i = 0; i < n; ++i) d.dz[i] = tanh_bwd_elem(d.dz[i], d.z[i]);
}

inline void ppo_loss_kernel(PpoLossArgs a) {
  if (threadIdx.x != 0) return;
  const int blk = blockIdx.x, cur = a.dev->cur;
  float dls[PPO_MAX_A] = {0.f}, dg[PPO_DIAG] = {0.f};
  const int b1 = min((blk + 1) * PPO_LOSS_ROWS, a.mb);
  for (int b = blk * PPO_LOSS_ROWS; b < b1; ++b) {
    const PpoRow r = ppo_loss_row(a, b);
    for (int j = 0; j < a.A; ++j) dls[j] += ppo_loss_row_j(a, b, j, r.g_nlp);
    dg[0] += r.pg; dg[1] += r.vf; dg[3] += r.kl; dg[4] += r.cf;
  }
  if (blk == 0) dg[2] = ppo_entropy(a);
  for (int j = 0; j < a.A; ++j) a.dls_slab[(long)blk * a.A + j] = blk == 0 ? dls[j] - a.ent_coef : dls[j];
  for (int k = 0; k < PPO_DIAG; ++k) a.diag[((long)cur * gridDim.x + blk) * PPO_DIAG + k] = dg[k];
  if (blk == 0) a.dev->cursor = cur + 1;
}
