// plan_ppo.inl: launch plan of stable-baselines 2.10.1 PPO2 with the actor-critic MlpPolicy (sb_helper.py:137-154) -- part of
// engine.hip (included there).  Kernels of its own: ppo_kernels.h; the dense products of the two towers are dense_fwd and the
// backward-data / weight-gradient builders of the per-layer Q route, the two towers of a layer level sharing a launch; the slab
// reduction is reduce_slabs_kernel; the global-norm clip + Adam are q_sumsq_kernel + q_clip_adam_kernel over a tile table whose
// tiles all name the same run of partial sums.  One lane, no forks: the lists run through run_seq / run_repeated like every plan.
// Shared: forward / backward take a tower mask and add_gather builds the minibatch gather -- plan_trpo.inl runs all three; the slab
// reduction, the stack weight gradients, clip + Adam and Adam come from grl_ctx (close_reduction, add_stack_wgrads, add_clip_adam, adam_op).
//
//   act path     model.step / model.value / model.predict on act_batch rows: ONE launch (ppo_act_kernel) for observations up to
//                2048 values and widths up to 256, else dense levels + tanh launches + the output launch + ppo_sample_kernel
//                normalize = 2: the step and finish lists exist a second time over the rows ppo_observe_kernel normalised
//                (grl_observe; grl_ppo_step / grl_ppo_finish with obs == NULL) -- the same launches, another input pointer
//   rollout      in the replay arena, row = env * n_steps + t (swap_and_flatten): obs [R, ldo], action, value, neglogp, reward,
//                done, advantage, return; the slot counter lives in device memory (PpoDev)
//   update       ppo_gather | per level: dense (pi, vf) + tanh_fwd | outputs | ppo_loss | per level: backward-data + tanh_bwd |
//                weight gradients | reduce_slabs | q_sumsq + q_clip_adam (max_grad_norm <= 0: adam alone)
//                -- identical for every minibatch of a grl_ppo_train call: the gather finds its slice through PpoDev.cursor
namespace {
struct PpoTowerP {      // one tower: hidden layers, then its output layer at index L()
  std::vector<int> width;
  int64_t w[GRL_MAX_LAYERS + 1], b[GRL_MAX_LAYERS + 1];
  int out = 0;
  int L() const { return (int)width.size(); }
};
struct PpoActs {        // activations (or their gradients) of both towers for one block of rows
  float* z[2][GRL_MAX_LAYERS];
  float* out[2];
  int ld_out[2];
};

// one tanh launch over the tensors of `descs` (the table goes up through the work arena); shared with plan_gail.inl
static void add_tanh_op(grl_ctx& h, std::vector<Op>& ops, const char* tag, bool bwd, const std::vector<TanhDesc>& descs, int rows) {
  if (descs.empty()) return;
  const TanhDesc* dd = h.upload_vec(h.wk, descs);
  const int n = (int)descs.size();
  int max_h = 1;
  for (auto& d : descs) max_h = std::max(max_h, (int)d.H);
  Op op; op.tag = tag;
  op.run = [dd, n, rows, max_h, bwd](hipStream_t s) { bwd ? launch_tanh_bwd(dd, n, rows, max_h, s) : launch_tanh_fwd(dd, n, rows, max_h, s); };
  ops.push_back(op);
}

struct PpoPlanner {
  grl_ctx& h;
  const grl_config& c;
  const grl_ppo_config& pc;
  const int B, A, NA, od, ldo, R;
  PpoTowerP T[2];      // 0 pi, 1 vf
  int64_t logstd_off = 0;
  const float* P = nullptr;
  bool wide = false, fused_act = false;
  PpoActs act_mb, g_mb, act_a;
  float *mb_act = nullptr, *mb_oldv = nullptr, *mb_oldnlp = nullptr, *mb_adv = nullptr, *mb_ret = nullptr, *mb_x = nullptr;
  float* dls_slab = nullptr;
  int nblk = 0;

  explicit PpoPlanner(grl_ctx& ctx)
      : h(ctx), c(ctx.cfg), pc(ctx.pcfg), B(ctx.cfg.batch_size), A(ctx.cfg.act_dim), NA(ctx.cfg.act_batch), od(ctx.cfg.obs_dim),
        ldo((int)rup(ctx.cfg.obs_dim, 4)), R(ctx.pcfg.n_envs * ctx.pcfg.n_steps) {
    h.A = A; h.B = B; h.NA = NA; h.L = c.n_layers;
    for (int l = 0; l < c.n_layers; ++l) T[0].width.push_back(c.layers[l]);
    for (int l = 0; l < pc.n_vf_layers; ++l) T[1].width.push_back(pc.vf_layers[l]);
    T[0].out = A; T[1].out = 1;
  }

  // ---------------- layout: TF creation order of stable-baselines' mlp_extractor + proba_distribution_from_latent
  void layout() {
    const char* nm[2] = {"pi", "vf"};
    for (int l = 0; l < std::max(T[0].L(), T[1].L()); ++l)
      for (int tw = 0; tw < 2; ++tw) {
        if (l >= T[tw].L()) continue;
        const int in = l == 0 ? od : T[tw].width[l - 1];
        const std::string s = std::string("model/") + nm[tw] + "_fc" + std::to_string(l);
        T[tw].w[l] = h.add_var(s + "/w:0", {in, T[tw].width[l]}, true);
        T[tw].b[l] = h.add_var(s + "/b:0", {T[tw].width[l]}, true);
      }
    const int Hp = T[0].width.back(), Hv = T[1].width.back();
    T[1].w[T[1].L()] = h.add_var("model/vf/w:0", {Hv, 1}, true);
    T[1].b[T[1].L()] = h.add_var("model/vf/b:0", {1}, true);
    T[0].w[T[0].L()] = h.add_var("model/pi/w:0", {Hp, A}, true);
    T[0].b[T[0].L()] = h.add_var("model/pi/b:0", {A}, true);
    logstd_off = h.add_var("model/pi/logstd:0", {1, A}, true);
    h.n_train = h.n_params;
    h.tgt_off = h.n_params;
    h.add_var("model/q/w:0", {Hv, A}, false);      // created by the policy, read by nothing, no gradient (TF: None, Adam skips it)
    h.add_var("model/q/b:0", {A}, false);
  }

  void routes() {
    wide = od > PPO_ACT_MAX_IN;
    bool fits = od <= PPO_ACT_MAX_IN;
    for (int tw = 0; tw < 2; ++tw)
      for (int w : T[tw].width) fits = fits && w <= PPO_ACT_MAX_HID;
    fused_act = fits && h.sw.get(Sw::ppo_act) != 0;
  }

  void alloc_acts(PpoActs& a, int rows, int ld_mean, int ld_v) {
    for (int tw = 0; tw < 2; ++tw)
      for (int l = 0; l < T[tw].L(); ++l) a.z[tw][l] = h.wk.f32((int64_t)rows * T[tw].width[l]);
    a.out[0] = h.wk.f32((int64_t)rows * ld_mean); a.ld_out[0] = ld_mean;
    a.out[1] = h.wk.f32((int64_t)rows * ld_v); a.ld_out[1] = ld_v;
  }

  void arenas() {
    Arena &st = h.st, &rp = h.rp, &wk = h.wk;
    h.params = st.f32(h.n_params);
    h.adam_m = st.f32(h.n_train);
    h.adam_v = st.f32(h.n_train);
    h.sc = (DevScalars*)st.take(sizeof(DevScalars));
    h.ppo_dev = (PpoDev*)st.take(sizeof(PpoDev));
    h.grads = h.gr.f32(h.n_train);
    h.pr_obs = rp.f32((int64_t)R * ldo); h.pr_act = rp.f32((int64_t)R * A);
    h.pr_val = rp.f32(R); h.pr_nlp = rp.f32(R); h.pr_rew = rp.f32(R); h.pr_done = rp.f32(R);
    h.pr_adv = rp.f32(R); h.pr_ret = rp.f32(R);
    h.pr_lastv = rp.f32(NA); h.pr_lastdone = rp.f32(NA);
    h.zero_once.push_back({h.pr_obs, (size_t)R * ldo * 4});      // (the row padding [obs_dim, ldo) travels with the gathered rows)
    h.ppo_ldo = ldo;
    // what one env step sends: observations [NA, ldo] | done [NA] | eps [NA, A] | rewards [NA]; what it returns: action | value | neglogp
    h.ppo_in = wk.f32((int64_t)NA * (ldo + 2 + A));
    h.ppo_out = wk.f32((int64_t)NA * (A + 2));
    h.zero_once.push_back({h.ppo_in, (size_t)NA * (ldo + 2 + A) * 4});
    h.ppo_perm = (int32_t*)wk.take((size_t)GRL_PPO_MAX_EPOCHS * R * 4);
    nblk = ppo_loss_blocks(B);
    h.ppo_nblk = nblk;
    h.ppo_diag = wk.f32((int64_t)GRL_PPO_MAX_EPOCHS * (R / B) * nblk * PPO_DIAG);
    mb_x = wk.f32((int64_t)B * ldo);
    h.zero_once.push_back({mb_x, (size_t)B * ldo * 4});
    mb_act = wk.f32((int64_t)B * A); mb_oldv = wk.f32(B); mb_oldnlp = wk.f32(B); mb_adv = wk.f32(B); mb_ret = wk.f32(B);
    alloc_acts(act_mb, B, A, 1);
    // output gradients: rows padded to 16 bytes for the weight-gradient launch, the padding stays zero
    const int ld_dm = (int)rup(A, 4);
    alloc_acts(g_mb, B, ld_dm, 4);
    h.zero_once.push_back({g_mb.out[0], (size_t)B * ld_dm * 4});
    h.zero_once.push_back({g_mb.out[1], (size_t)B * 4 * 4});
    dls_slab = wk.f32((int64_t)nblk * A);
    if (!fused_act) alloc_acts(act_a, NA, A, 1);
    if (c.normalize == 2) {
      // VecNormalize observation statistics on the device (grl_observe; ppo_observe_kernel) -- behind everything a normalize = 0
      // handle holds, whose offsets and sizes stay what they were
      h.n_elems = od;
      h.n_count = (double*)st.take(16);
      h.n_mean = (double*)st.take((size_t)od * 8);
      h.n_var = (double*)st.take((size_t)od * 8);
      h.n_sd = (double*)st.take((size_t)od * 8);
      h.n_stage = wk.f32((int64_t)NA * od);
      h.ppo_obs_n = wk.f32((int64_t)NA * ldo);
      h.zero_once.push_back({h.ppo_obs_n, (size_t)NA * ldo * 4});
    }
    P = h.params;
  }

  // ---------------- forward of both towers over `rows` rows of x: per level one dense launch + one tanh launch, then the outputs
  void add_tanh(std::vector<Op>& ops, const char* tag, bool bwd, const std::vector<TanhDesc>& descs, int rows) {
    add_tanh_op(h, ops, tag, bwd, descs, rows);
  }
  // (towers: bit 0 pi, bit 1 vf -- plan_trpo.inl runs them apart)
  void forward(std::vector<Op>& ops, const float* x, int rows, const PpoActs& a, const char* tag, int towers = 3) {
    const std::string t(tag);
    std::string l0_note;
    auto on =[&](int tw, int l) { return ((towers >> tw) & 1) && l < T[tw].L(); };
    for (int l = 0; l < std::max(T[0].L(), T[1].L()); ++l) {
      std::vector<IgemmProb> pr;
      std::vector<TanhDesc> td;
      int n_here = 0;
      for (int tw = 0; tw < 2; ++tw) n_here += on(tw, l) ? 1 : 0;
      for (int tw = 0; tw < 2; ++tw) {
        if (!on(tw, l)) continue;
        const int N = T[tw].width[l];
        const float* in = l == 0 ? x : a.z[tw][l - 1];
        const int ldin = l == 0 ? ldo : T[tw].width[l - 1], K = l == 0 ? od : T[tw].width[l - 1];
        IgemmProb p = h.dense_fwd(in, ldin, K, nullptr, 0, 0, rows, P + T[tw].w[l], N, P + T[tw].b[l], a.z[tw][l], N, ACT_NONE);
        TanhDesc d;
        memset(&d, 0, sizeof(d));
        d.z = a.z[tw][l]; d.H = N;
        if (l == 0 && wide) {
          // a wide first layer: one or two tiles would walk K = obs_dim alone -- the reduction is cut until the launch has at least
          // 64 tiles (as q_l0 of the wide Q route); the tanh launch adds the partial sums in index order, then the bias
          const int base = n_here * ((rows + 63) / 64) * ((N + 63) / 64);
          h.set_split(p, (64 + base - 1) / base);
          if (p.split > 1) {
            float* parts = h.wk.f32((int64_t)rows * N * p.split);
            p.c = parts; p.bias = nullptr;
            d.parts = parts; d.bias = P + T[tw].b[l]; d.part_stride = p.slab_stride; d.n_parts = p.split;
          }
        }
        if (l == 0) {      // GRL_PLAN_DUMP: the route of this tower's first layer and of the tanh launch behind it
          char buf[160];
          const char* nm = tw == 0 ? "pi" : "vf";
          if (p.split > 1) snprintf(buf, sizeof(buf), "  %s H %d split %d (part_stride %% 4 = %d, rows * H %% 4 = %d)", nm, N, p.split,
                                    (int)(p.slab_stride & 3), (int)(((int64_t)rows * N) & 3));
          else snprintf(buf, sizeof(buf), "  %s H %d whole (rows * H %% 4 = %d)", nm, N, (int)(((int64_t)rows * N) & 3));
          l0_note += buf;
        }
        pr.push_back(p);
        td.push_back(d);
      }
      if (l == 0) plan_note("grl plan: ppo_l0        %s: %d rows;%s\n", tag, rows, l0_note.c_str());
      h.add_launch(ops, t + "_l" + std::to_string(l), 0, pr);
      add_tanh(ops, "ppo_tanh_fwd", false, td, rows);
    }
    std::vector<IgemmProb> po;
    for (int tw = 0; tw < 2; ++tw) {
      if (!on(tw, 0)) continue;
      const int Lt = T[tw].L(), H = T[tw].width.back();
      po.push_back(h.dense_fwd(a.z[tw][Lt - 1], H, H, nullptr, 0, 0, rows, P + T[tw].w[Lt], T[tw].out, P + T[tw].b[Lt], a.out[tw], a.ld_out[tw], ACT_NONE));
    }
    h.add_launch(ops, t + "_out", 0, po);
  }

  // ---------------- the act path: model.step (records), model.value (last values), model.predict (records nothing)
  PpoSampleArgs sample_args(int mode, int deterministic, bool host_eps, const float* x) const {
    PpoSampleArgs s;
    memset(&s, 0, sizeof(s));
    if (!fused_act) { s.mean = act_a.out[0]; s.ld_mean = A; s.v = act_a.out[1]; s.ld_v = 1; }
    s.logstd = P + logstd_off;
    s.x = x; s.ldx = ldo;
    s.done_in = h.ppo_in + (int64_t)NA * ldo;
    s.eps = host_eps ? h.ppo_in + (int64_t)NA * (ldo + 1) : nullptr;
    s.r_obs = h.pr_obs; s.r_act = h.pr_act; s.r_val = h.pr_val; s.r_nlp = h.pr_nlp; s.r_done = h.pr_done;
    s.ldo = ldo; s.n_steps = pc.n_steps; s.dev = h.ppo_dev; s.sc = h.sc; s.seed = c.seed;
    s.out_act = h.ppo_out; s.out_val = h.ppo_out + (int64_t)NA * A; s.out_nlp = h.ppo_out + (int64_t)NA * (A + 1);
    s.last_v = h.pr_lastv; s.last_done = h.pr_lastdone;
    s.n = NA; s.A = A; s.obs_dim = od; s.mode = mode; s.deterministic = deterministic;
    return s;
  }
  void act_path() {
    // (observed: the rows ppo_observe_kernel normalised, normalize = 2 handles -- the same launches over the other buffer)
    std::vector<Op> fwd, fwd_n;
    if (!fused_act) forward(fwd, h.ppo_in, NA, act_a, "ppo_act");
    if (!fused_act && c.normalize == 2) forward(fwd_n, h.ppo_obs_n, NA, act_a, "ppo_act");
    PpoActArgs fa;
    memset(&fa, 0, sizeof(fa));
    for (int tw = 0; tw < 2; ++tw) {
      PpoTower& t = fa.tw[tw];
      t.L = T[tw].L(); t.out = T[tw].out;
      for (int l = 0; l < t.L; ++l) { t.w[l] = P + T[tw].w[l]; t.b[l] = P + T[tw].b[l]; t.hid[l] = T[tw].width[l]; }
      t.ow = P + T[tw].w[t.L]; t.ob = P + T[tw].b[t.L];
    }
    DevScalars* sc = h.sc;
    auto build = [&](std::vector<Op>& ops, int mode, int det, bool host_eps, bool observed = false) {
      ops = observed ? fwd_n : fwd;
      const PpoSampleArgs sa = sample_args(mode, det, host_eps, observed ? h.ppo_obs_n : h.ppo_in);
      Op op; op.tag = fused_act ? "ppo_act" : "ppo_sample";
      if (fused_act) {
        PpoActArgs a = fa;
        a.s = sa;
        op.run = [a](hipStream_t s) { launch_ppo_act(a, s); };
      } else {
        op.run = [sa](hipStream_t s) { launch_ppo_sample(sa, s); };
      }
      ops.push_back(op);
      if (mode != 2 && !det && !host_eps) {      // the draw used the Philox counter: the next call takes the next one
        Op tick; tick.tag = "rng_tick";
        tick.run = [sc](hipStream_t s) { hipLaunchKernelGGL(rng_tick_kernel, dim3(1), dim3(1), 0, s, sc); };
        ops.push_back(tick);
      }
    };
    build(h.ops_ppo_step[0], 1, 0, true);
    build(h.ops_ppo_step[1], 1, 0, false);
    build(h.ops_ppo_finish, 2, 1, false);
    build(h.ops_ppo_act[0], 0, 1, false);
    build(h.ops_ppo_act[1], 0, 0, true);
    build(h.ops_ppo_act[2], 0, 0, false);
    if (c.normalize == 2) {
      build(h.ops_ppo_step_n[0], 1, 0, true, true);
      build(h.ops_ppo_step_n[1], 1, 0, false, true);
      build(h.ops_ppo_finish_n, 2, 1, false, true);
    }
    if (fused_act) plan_note("grl plan: ppo_act       one launch per call (ppo_act_kernel): %d rows x 2 towers, obs %d\n", NA, od);
    else plan_note("grl plan: ppo_act       launch list (%s): dense levels + tanh + outputs + ppo_sample, %d rows, obs %d\n",
                   od > PPO_ACT_MAX_IN ? "observation beyond 2048 values" : (h.sw.get(Sw::ppo_act) ? "a width beyond 256" : "ppo_act=0"), NA, od);
    // rewards close the slot; GAE behind the last values
    {
      const float* rin = h.ppo_in + (int64_t)NA * (ldo + 1 + A);
      float* rr = h.pr_rew; PpoDev* dev = h.ppo_dev; const int n = NA, ns = pc.n_steps;
      Op op; op.tag = "ppo_rewards";
      op.run = [rin, rr, dev, n, ns](hipStream_t s) { launch_ppo_rewards(rin, rr, dev, n, ns, s); };
      h.ops_ppo_rew.push_back(op);
    }
    {
      GaeArgs g;
      memset(&g, 0, sizeof(g));
      g.rew = h.pr_rew; g.val = h.pr_val; g.done = h.pr_done; g.last_v = h.pr_lastv; g.last_done = h.pr_lastdone;
      g.adv = h.pr_adv; g.ret = h.pr_ret; g.n_envs = pc.n_envs; g.n_steps = pc.n_steps;
      g.gamma = c.gamma; g.c = (float)((double)c.gamma * (double)pc.lam);
      Op op; op.tag = "gae";
      op.run = [g](hipStream_t s) { launch_gae(g, s); };
      h.ops_ppo_finish.push_back(op);
      if (c.normalize == 2) h.ops_ppo_finish_n.push_back(op);
    }
  }

  // ---------------- one minibatch update
  // the minibatch PpoDev.cursor names: its rows of the rollout into mb_* (plan_trpo.inl: the value fit's minibatches)
  void add_gather(std::vector<Op>& ops) {
    PpoGatherArgs g;
    memset(&g, 0, sizeof(g));
    g.perm = h.ppo_perm; g.dev = h.ppo_dev; g.sc = h.sc;
    g.r_obs = h.pr_obs; g.ldo = ldo; g.r_act = h.pr_act; g.r_oldv = h.pr_val; g.r_oldnlp = h.pr_nlp; g.r_adv = h.pr_adv; g.r_ret = h.pr_ret;
    g.x = mb_x; g.act = mb_act; g.oldv = mb_oldv; g.oldnlp = mb_oldnlp; g.adv = mb_adv; g.ret = mb_ret;
    g.mb = B; g.A = A;
    Op op; op.tag = "ppo_gather";
    op.run = [g](hipStream_t s) { launch_ppo_gather(g, s); };
    ops.push_back(op);
  }
  // Backward of the towers in `towers` (as forward) over `rows` rows of x, activations in act, output gradients in gr.  Backward-data
  // level by level from the outputs down, the towers of a level sharing a launch `tag`_bwd (the gradient w.r.t. a layer's OUTPUT,
  // then tanh_bwd turns it, in place, into the gradient w.r.t. its pre-activation; nothing flows into the observations); the
  // weight gradients of every layer as ONE launch `tag`_wgrad; their slabs -- and the dls_blocks partial sums of d logstd in `dls`,
  // if any -- summed into the bucket-shaped dst by a reduction launch of its own.  Returns that launch's descriptors.
  ReduceDesc* backward(std::vector<Op>& ops, const std::string& tag, int towers, int rows, const float* x, const PpoActs& act, const PpoActs& gr,
                       float* dst, const float* dls, int dls_blocks) {
    auto on = [&](int tw) { return ((towers >> tw) & 1) != 0; };
    const int depth = std::max(on(0) ? T[0].L() : 0, on(1) ? T[1].L() : 0);
    for (int s = 0; s < depth; ++s) {
      std::vector<IgemmProb> pr;
      std::vector<TanhDesc> td;
      for (int tw = 0; tw < 2; ++tw) {
        const int l = T[tw].L() - 1 - s;
        if (!on(tw) || l < 0) continue;
        const grl_ctx::BwdPart above = s == 0 ? grl_ctx::BwdPart{gr.out[tw], gr.ld_out[tw], T[tw].out, P + T[tw].w[l + 1]}
                                              : grl_ctx::BwdPart{gr.z[tw][l + 1], T[tw].width[l + 1], T[tw].width[l + 1], P + T[tw].w[l + 1]};
        pr.push_back(h.dense_bwd({above}, rows, 0, T[tw].width[l], gr.z[tw][l], T[tw].width[l], nullptr));
        TanhDesc d;
        memset(&d, 0, sizeof(d));
        d.z = act.z[tw][l]; d.dz = gr.z[tw][l]; d.H = T[tw].width[l];
        td.push_back(d);
      }
      h.add_launch(ops, tag + "_bwd", 1, pr);
      add_tanh(ops, "ppo_tanh_bwd", true, td, rows);
    }
    h.reduces.clear();      // (every backward has a reduction launch of its own)
    std::vector<IgemmProb> wg;
    for (int tw = 0; tw < 2; ++tw)
      if (on(tw))
        h.add_stack_wgrads(wg, x, ldo, od, act.z[tw], gr.z[tw], T[tw].width.data(), T[tw].L(), gr.out[tw], gr.ld_out[tw], T[tw].out, T[tw].w, T[tw].b,
                           rows, dst);
    h.add_launch(ops, tag + "_wgrad", 2, wg);
    if (dls) {
      ReduceDesc rd;
      memset(&rd, 0, sizeof(rd));
      rd.src = dls; rd.splits = dls_blocks; rd.slab_stride = A; rd.dst = dst + logstd_off; rd.n = A;
      h.reduces.push_back(rd);
    }
    const grl_ctx::SumPlan sum = h.close_reduction();
    ops.push_back(sum.op);
    return sum.descs;
  }
  void update() {
    std::vector<Op>& ops = h.ops_ppo_update;
    add_gather(ops);
    forward(ops, mb_x, B, act_mb, "ppo_fwd");
    {
      PpoLossArgs a;
      memset(&a, 0, sizeof(a));
      a.mean = act_mb.out[0]; a.ld_mean = A; a.logstd = P + logstd_off; a.v = act_mb.out[1]; a.ld_v = 1;
      a.act = mb_act; a.oldv = mb_oldv; a.oldnlp = mb_oldnlp; a.adv = mb_adv; a.ret = mb_ret;
      a.dev = h.ppo_dev;
      a.dmean = g_mb.out[0]; a.ld_dm = g_mb.ld_out[0]; a.dv = g_mb.out[1]; a.ld_dv = g_mb.ld_out[1];
      a.dls_slab = dls_slab; a.diag = h.ppo_diag; a.mb = B; a.A = A;
      a.clip = pc.clip_range; a.clip_vf = pc.clip_range_vf; a.ent_coef = pc.ent_coef; a.vf_coef = pc.vf_coef;
      Op op; op.tag = "ppo_loss";
      op.run = [a](hipStream_t s) { launch_ppo_loss(a, s); };
      ops.push_back(op);
    }
    // (d logstd is in the bucket before the norm is formed)
    h.d_reduces = backward(ops, "ppo", 3, B, mb_x, act_mb, g_mb, h.grads, dls_slab, nblk);
    // clip_by_global_norm + Adam: the tiles of q_wide_kernels.h with ONE run of partial sums for all of them -- every tile adds all
    // partials in index order and forms clip / max(||g||, clip) over the whole bucket (TF-Adam, epsilon from grl_ppo_config)
    if (pc.max_grad_norm > 0.f) {
      const int n_tl = h.add_clip_adam(ops, h.trainable_segs(), pc.max_grad_norm, pc.adam_eps, true, false);
      plan_note("grl plan: ppo apply     q_sumsq + q_clip_adam over %d tiles sharing one run of partial sums (global norm %g)\n", n_tl, pc.max_grad_norm);
    } else {
      ops.push_back(h.adam_op("adam", pc.adam_eps, false, false));
    }
  }

  void debug_views() {
    auto& dbg = h.dbg;
    dbg["ppo_obs"] = {h.pr_obs, (int64_t)R * ldo};
    if (c.normalize == 2) dbg["ppo_obs_n"] = {h.ppo_obs_n, (int64_t)NA * ldo};
    dbg["ppo_act"] = {h.pr_act, (int64_t)R * A};
    dbg["ppo_old_v"] = {h.pr_val, R}; dbg["ppo_old_nlp"] = {h.pr_nlp, R};
    dbg["ppo_rew"] = {h.pr_rew, R}; dbg["ppo_done"] = {h.pr_done, R};
    dbg["ppo_adv"] = {h.pr_adv, R}; dbg["ppo_ret"] = {h.pr_ret, R};
    dbg["ppo_last_v"] = {h.pr_lastv, NA}; dbg["ppo_last_done"] = {h.pr_lastdone, NA};
    dbg["ppo_mean"] = {act_mb.out[0], (int64_t)B * A}; dbg["ppo_v"] = {act_mb.out[1], B};
    dbg["ppo_dmean"] = {g_mb.out[0], (int64_t)B * g_mb.ld_out[0]}; dbg["ppo_dv"] = {g_mb.out[1], (int64_t)B * 4};
    dbg["ppo_mb_adv"] = {mb_adv, B};
    dbg["grads"] = {h.grads, h.n_train};
    dbg["adam_m"] = {h.adam_m, h.n_train};
    dbg["adam_v"] = {h.adam_v, h.n_train};
  }
};
}  // namespace

int grl_ctx::plan_ppo() {
  PpoPlanner p(*this);
  p.layout();
  p.routes();
  p.arenas();
  p.act_path();
  p.update();
  p.debug_views();
  return GRL_OK;
}
