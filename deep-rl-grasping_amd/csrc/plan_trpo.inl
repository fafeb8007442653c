// plan_trpo.inl: launch plan of stable-baselines 2.10.1 TRPO with the actor-critic MlpPolicy (sb_helper.py:129-136) -- part of
// engine.hip (included there).  The parameter layout, the act path, the rollout in the replay arena and GAE are plan_ppo.inl's,
// built for ONE environment of n_steps = timesteps_per_batch rows; the kernels of its own are trpo_kernels.h; the dense products,
// backward-data and weight gradients are dense_fwd / dense_bwd / dense_wgrad, the slab reduction reduce_slabs_kernel, the value
// fit's Adam adam_polyak_kernel over the whole bucket (the policy entries of the gradient bucket are never written: moments that
// stay zero give a step of exactly zero).  One lane, no forks: the lists run through run_seq / run_repeated.
// Shared: every forward, every backward (BWD_T, BWD_F, BWD_vf) and the value fit's gather are PpoPlanner's, called with a tower mask.
//
// Vectors of the policy step (g, r, p, x, z, fullstep, theta_old) are laid out like the gradient bucket, the entries of the value
// variables held at zero: dot products over the whole bucket are dot products over the policy variables, and a tangent weight
// is `vector + the variable's offset`.
//
//   policy step  trpo_prep | theta_old = params | FWD_T | trpo_loss (gradient) | scal | BWD_T -> g | gather Fisher rows | FWD_F |
//                cg_init | scal | cg_iters x [FVP(p) | dot | cg_x | cg_p] | p = x | FVP | dot | step |
//                ls_steps x [theta' | FWD_T | trpo_loss (evaluate) | scal] | restore
//     FWD_*      per level: dense + tanh_fwd; the output launch                                  (2 L + 1 launches)
//     BWD_*      per level: backward-data + tanh_bwd; weight gradients; reduce_slabs             (2 L + 2)
//     FVP        per level: ONE dense launch of two problems (h_below dW + db | dh_below W) + trpo_tan; the same for the output
//                stage; BWD_F; trpo_fvp_fin                                                      (4 L + 5)
//                A tangent level is two dense problems in one launch and an element-wise kernel rather than a fused kernel: the
//                products stay on the tuned dense path and the new kernel is ten lines.
//     The dense launches carry no flag: behind "CG finished" / "trial accepted" they still run, and nothing reads what they write.
//   value fit    ppo_gather | FWD_vf | trpo_vf_loss | BWD_vf | adam           -- identical for every minibatch: the gather finds
//                its slice of the compacted permutations through PpoDev.cursor
namespace {
struct TrpoPlanner {
  PpoPlanner& pp;
  grl_ctx& h;
  const grl_trpo_config& tc;
  const int T, NF, A, od, ldo, B, ld_dm;
  const int64_t n;
  const float* P;
  PpoActs act_T, g_T, act_F, g_F;
  float *tan_h[GRL_MAX_LAYERS], *t1[GRL_MAX_LAYERS + 1], *t2[GRL_MAX_LAYERS + 1];
  float *atarg, *mean_old, *logstd_old, *theta_old, *g, *r, *p, *x, *z, *full, *xf, *lpart, *dls_T, *vpart, *vpart2;
  int nblk_T, nvb;
  std::vector<Op> fwd_T, fvp;

  TrpoPlanner(PpoPlanner& q)
      : pp(q), h(q.h), tc(q.h.tcfg), T(q.h.tcfg.n_steps), NF((q.h.tcfg.n_steps + q.h.tcfg.fvp_stride - 1) / q.h.tcfg.fvp_stride), A(q.A),
        od(q.od), ldo(q.ldo), B(q.B), ld_dm((int)rup(q.A, 4)), n(q.h.n_train), P(q.P) {}

  void alloc_pi(PpoActs& a, int rows, int ld_mean) {
    memset(&a, 0, sizeof(a));
    for (int l = 0; l < pp.T[0].L(); ++l) a.z[0][l] = h.wk.f32((int64_t)rows * pp.T[0].width[l]);
    a.out[0] = h.wk.f32((int64_t)rows * ld_mean); a.ld_out[0] = ld_mean;
  }
  float* zeroed(Arena& ar, int64_t cnt) {
    float* q = ar.f32(cnt);
    h.zero_once.push_back({q, (size_t)cnt * 4});
    return q;
  }
  void arenas() {
    Arena& wk = h.wk;
    h.trpo_dev = (TrpoDev*)h.st.take(sizeof(TrpoDev));
    alloc_pi(act_T, T, A); alloc_pi(g_T, T, ld_dm);
    alloc_pi(act_F, NF, A); alloc_pi(g_F, NF, ld_dm);
    h.zero_once.push_back({g_T.out[0], (size_t)T * ld_dm * 4});      // (row padding of the output gradients stays zero)
    h.zero_once.push_back({g_F.out[0], (size_t)NF * ld_dm * 4});
    const PpoTowerP& pi = pp.T[0];
    for (int l = 0; l <= pi.L(); ++l) {
      const int N = l < pi.L() ? pi.width[l] : A;
      t1[l] = wk.f32((int64_t)NF * N); t2[l] = wk.f32((int64_t)NF * N);
      if (l < pi.L()) tan_h[l] = wk.f32((int64_t)NF * N);
    }
    atarg = wk.f32(T); mean_old = wk.f32((int64_t)T * A); logstd_old = wk.f32(A);
    // the vectors: entries no launch writes (the value variables') are zero from creation on
    theta_old = zeroed(wk, n); g = zeroed(wk, n); r = zeroed(wk, n); p = zeroed(wk, n); x = zeroed(wk, n); z = zeroed(wk, n);
    full = zeroed(wk, n);
    h.zero_once.push_back({h.grads, (size_t)n * 4});      // the value fit writes the value entries only
    xf = zeroed(wk, (int64_t)NF * ldo);
    nblk_T = trpo_loss_blocks(T);
    nvb = trpo_vec_blocks(n);
    plan_note("grl plan: trpo vec      %lld entries in %d workgroups (reducing vector launches)\n", (long long)n, nvb);
    lpart = wk.f32((int64_t)nblk_T * 2); dls_T = wk.f32((int64_t)nblk_T * A);
    vpart = wk.f32((int64_t)nvb * 2); vpart2 = wk.f32(nvb);
  }

  TrpoVecArgs vec() const {
    TrpoVecArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.r = r; a.p = p; a.z = z; a.g = g; a.v = p; a.full = full; a.part = vpart; a.part2 = vpart2;
    a.dev = h.trpo_dev; a.n = n; a.ls_off = pp.logstd_off; a.A = A; a.n_part = nvb;
    a.damping = tc.cg_damping; a.max_kl = tc.max_kl;
    return a;
  }
  void add_vec(std::vector<Op>& ops, const char* tag, int kind, const TrpoVecArgs& a) {
    Op op; op.tag = tag;
    op.run = [kind, a](hipStream_t s) { launch_trpo_vec(kind, a, s); };
    ops.push_back(op);
  }
  void add_scal(std::vector<Op>& ops, int mode, int k, const float* part, int n_part) {
    TrpoScalArgs a;
    memset(&a, 0, sizeof(a));
    a.dev = h.trpo_dev; a.part = part; a.n_part = n_part; a.logstd = P + pp.logstd_off; a.A = A; a.T = T; a.mode = mode; a.k = k;
    a.ent_coef = tc.ent_coef; a.max_kl = tc.max_kl;
    Op op; op.tag = "trpo_scal";
    op.run = [a](hipStream_t s) { launch_trpo_scal(a, s); };
    ops.push_back(op);
  }
  void add_loss(std::vector<Op>& ops, int mode) {
    TrpoLossArgs a;
    memset(&a, 0, sizeof(a));
    a.mean = act_T.out[0]; a.ld_mean = A; a.logstd = P + pp.logstd_off; a.act = h.pr_act; a.atarg = atarg;
    a.mean_old = mean_old; a.logstd_old = logstd_old; a.dmean = g_T.out[0]; a.ld_dm = ld_dm; a.dls_slab = dls_T; a.part = lpart;
    a.dev = h.trpo_dev; a.T = T; a.A = A; a.mode = mode; a.ent_coef = tc.ent_coef;
    Op op; op.tag = mode ? "trpo_loss_eval" : "trpo_loss";
    op.run = [a](hipStream_t s) { launch_trpo_loss(a, s); };
    ops.push_back(op);
  }

  // ---------------- z = F(p) over the Fisher rows (their activations in act_F)
  void build_fvp() {
    const PpoTowerP& pi = pp.T[0];
    const float* V = p;
    for (int l = 0; l <= pi.L(); ++l) {
      const bool outl = l == pi.L();
      const int N = outl ? A : pi.width[l];
      const float* below = l == 0 ? xf : act_F.z[0][l - 1];
      const int ldin = l == 0 ? ldo : pi.width[l - 1], K = l == 0 ? od : pi.width[l - 1];
      std::vector<IgemmProb> pr;
      pr.push_back(h.dense_fwd(below, ldin, K, nullptr, 0, 0, NF, V + pi.w[l], N, V + pi.b[l], t1[l], N, ACT_NONE));
      if (l > 0) pr.push_back(h.dense_fwd(tan_h[l - 1], K, K, nullptr, 0, 0, NF, P + pi.w[l], N, nullptr, t2[l], N, ACT_NONE));
      h.add_launch(fvp, std::string("trpo_tan_l") + std::to_string(l), 0, pr);
      TrpoTanArgs a;
      memset(&a, 0, sizeof(a));
      a.t1 = t1[l]; a.t2 = l > 0 ? t2[l] : nullptr; a.rows = NF; a.H = N;
      if (outl) { a.logstd = P + pp.logstd_off; a.out = g_F.out[0]; a.ld_out = ld_dm; a.inv_n = 1.0f / (float)NF; }
      else { a.h = act_F.z[0][l]; a.out = tan_h[l]; a.ld_out = N; }
      Op op; op.tag = outl ? "trpo_fvp_out" : "trpo_tan";
      op.run = [a](hipStream_t s) { launch_trpo_tan(a, s); };
      fvp.push_back(op);
    }
    pp.backward(fvp, "trpo_fvp", 1, NF, xf, act_F, g_F, z, nullptr, 0);
    add_vec(fvp, "trpo_fvp_fin", TRPO_V_FVP_FIN, vec());
  }

  void gather_fisher(std::vector<Op>& ops) {
    const float* ro = h.pr_obs; float* dst = xf; const int ld = ldo, st = tc.fvp_stride, nf = NF;
    Op op; op.tag = "trpo_gather";
    op.run = [ro, dst, ld, st, nf](hipStream_t s) { launch_trpo_gather(ro, dst, ld, st, nf, s); };
    ops.push_back(op);
    pp.forward(ops, xf, NF, act_F, "trpo_fwd_f", 1);
  }

  void policy_step() {
    std::vector<Op>& ops = h.ops_trpo_policy;
    pp.forward(fwd_T, h.pr_obs, T, act_T, "trpo_fwd", 1);
    build_fvp();
    {
      TrpoPrepArgs a = {h.pr_adv, atarg, h.trpo_dev, T};
      Op op; op.tag = "trpo_prep";
      op.run = [a](hipStream_t s) { launch_trpo_prep(a, s); };
      ops.push_back(op);
    }
    TrpoVecArgs th = vec();
    th.x = h.params; th.r = theta_old;
    th.it = 0;
    add_vec(ops, "trpo_theta_old", TRPO_V_THETA, th);
    ops.insert(ops.end(), fwd_T.begin(), fwd_T.end());
    add_loss(ops, 0);
    add_scal(ops, TRPO_SC_BEFORE, 0, lpart, nblk_T);
    pp.backward(ops, "trpo_g", 1, T, h.pr_obs, act_T, g_T, g, dls_T, nblk_T);
    gather_fisher(ops);
    add_vec(ops, "trpo_cg_init", TRPO_V_CG_INIT, vec());
    add_scal(ops, TRPO_SC_CG, 0, vpart, nvb);
    for (int i = 0; i < tc.cg_iters; ++i) {
      ops.insert(ops.end(), fvp.begin(), fvp.end());
      TrpoVecArgs a = vec();
      a.it = i;
      add_vec(ops, "trpo_dot", TRPO_V_DOT, a);
      add_vec(ops, "trpo_cg_x", TRPO_V_CG_X, a);
      add_vec(ops, "trpo_cg_p", TRPO_V_CG_P, a);
    }
    {      // shs = 0.5 x.F(x): the product reads p
      float* dst = p; const float* src = x; const int64_t cnt = n;
      Op op; op.tag = "trpo_copy";
      op.run = [dst, src, cnt](hipStream_t s) { launch_trpo_copy(dst, src, cnt, s); };
      ops.push_back(op);
      ops.insert(ops.end(), fvp.begin(), fvp.end());
      TrpoVecArgs a = vec();
      a.it = -1;
      add_vec(ops, "trpo_dot", TRPO_V_DOT, a);
      add_vec(ops, "trpo_step", TRPO_V_STEP, a);
    }
    for (int k = 0; k < tc.ls_steps; ++k) {
      th.it = 1; th.scale = std::ldexp(1.0f, -k);
      add_vec(ops, "trpo_theta", TRPO_V_THETA, th);
      ops.insert(ops.end(), fwd_T.begin(), fwd_T.end());
      add_loss(ops, 1);
      add_scal(ops, TRPO_SC_TRIAL, k, lpart, nblk_T);
    }
    th.it = 2;
    add_vec(ops, "trpo_restore", TRPO_V_THETA, th);
    plan_note("grl plan: trpo policy   %d launches: %d Fisher products of %d launches over %d of %d rows, %d trials\n", (int)ops.size(),
              tc.cg_iters + 1, (int)fvp.size(), NF, T, tc.ls_steps);
    // the debug product: the Fisher rows and their activations at the current parameters, then F(trpo_fvp_in)
    gather_fisher(h.ops_trpo_fvp);
    h.ops_trpo_fvp.insert(h.ops_trpo_fvp.end(), fvp.begin(), fvp.end());
  }

  void value_fit() {
    std::vector<Op>& ops = h.ops_trpo_vf;
    pp.add_gather(ops);
    pp.forward(ops, pp.mb_x, B, pp.act_mb, "trpo_vf_fwd", 2);
    {
      const float* v = pp.act_mb.out[1]; const float* ret = pp.mb_ret; float* dv = pp.g_mb.out[1];
      const int ldv = pp.act_mb.ld_out[1], lddv = pp.g_mb.ld_out[1], mb = B; PpoDev* dev = h.ppo_dev;
      Op op; op.tag = "trpo_vf_loss";
      op.run = [v, ldv, ret, dv, lddv, mb, dev](hipStream_t s) { launch_trpo_vf_loss(v, ldv, ret, dv, lddv, mb, dev, s); };
      ops.push_back(op);
    }
    pp.backward(ops, "trpo_vf", 2, B, pp.mb_x, pp.act_mb, pp.g_mb, h.grads, nullptr, 0);
    ops.push_back(h.adam_op("adam", tc.adam_eps, false, false));
  }

  void debug_views() {
    auto& dbg = h.dbg;
    dbg["trpo_atarg"] = {atarg, T};
    dbg["trpo_g"] = {g, n}; dbg["trpo_stepdir"] = {x, n}; dbg["trpo_fullstep"] = {full, n};
    dbg["trpo_fvp_in"] = {p, n}; dbg["trpo_fvp_out"] = {z, n}; dbg["trpo_theta_old"] = {theta_old, n};
    dbg["trpo_mean_old"] = {mean_old, (int64_t)T * A};
  }
};
}  // namespace

int grl_ctx::plan_trpo() {
  // the policy, the rollout and GAE are a PPO handle's with one environment
  memset(&pcfg, 0, sizeof(pcfg));
  pcfg.n_envs = 1; pcfg.n_steps = tcfg.n_steps;
  pcfg.n_vf_layers = tcfg.n_vf_layers;
  for (int l = 0; l < tcfg.n_vf_layers; ++l) pcfg.vf_layers[l] = tcfg.vf_layers[l];
  pcfg.lam = tcfg.lam; pcfg.adam_eps = tcfg.adam_eps; pcfg.norm_eps64 = tcfg.norm_eps64;
  PpoPlanner pp(*this);
  pp.layout();
  pp.routes();
  pp.arenas();
  pp.act_path();
  pp.debug_views();
  TrpoPlanner t(pp);
  t.arenas();
  t.policy_step();
  t.value_fit();
  t.debug_views();
  return GRL_OK;
}
