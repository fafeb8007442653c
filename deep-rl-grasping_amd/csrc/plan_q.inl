// plan_q.inl: launch plan of the DQN / BDQ update incl. prioritised replay (grl_ctx::plan_q) -- part of engine.hip (included there, same translation unit: the plans are methods of grl_ctx).

// --------------------------------------------------------------------------------------------------
// DQN (sb_helper.py:159-165) and BDQ (sb_helper.py:210-224): MLP towers on vector observations.
// One structure covers both: optional shared trunk -> D advantage branches + a state
// value tower, dueling aggregation per branch, double-Q target averaged over branches.
namespace {
// A stack of dense layers: hidden layers (ReLU, layer-normalised under grl_config.q_layer_norm), then an output layer of `out`
// units -- bins for a branch, 1 for the state value, 0 for the trunk, which has none.
struct QStack {
  std::string scope;                  // TF scope of its variables; stacks that share one (the branches) share its name counters
  std::vector<int> width;             // hidden widths
  int out = 0;
  std::vector<int64_t> w, b;          // offsets into params: one per hidden layer, then the output layer's
  std::vector<int64_t> beta, gam;     // layer normalisation: one per hidden layer, empty otherwise
  QStack() {}
  QStack(const char* scope, const int* w, int n, int out) : scope(scope), width(w, w + n), out(out) {}
  int L() const { return (int)width.size(); }
};
// what a pass over one stack keeps: activations per hidden layer and where the output layer writes.  u / stat: layer
// normalisation, the pass that is differentiated only -- pre-activations kept beside the activations, and the rows' (mean, rstd);
// every other pass normalises in place (ln_kernels.h)
struct QStackAct {
  std::vector<float*> z, u, stat;
  float* out = nullptr;
  int ld_out = 0;
};
// trunk + towers; stack(0) is the trunk, stack(1 + tw) tower tw: every pass over a network is one loop
template <class S> struct QTowers {
  S trunk;
  std::vector<S> tower;               // [0, D): branches, [D]: state value
  int n_stacks() const { return 1 + (int)tower.size(); }
  S& stack(int i) { return i == 0 ? trunk : tower[i - 1]; }
  const S& stack(int i) const { return i == 0 ? trunk : tower[i - 1]; }
};
typedef QTowers<QStack> QNet;
struct QNetAct : QTowers<QStackAct> {
  float *adv = nullptr, *v = nullptr; // [rows, D * bins] advantages, [rows] state values (the towers' `out` point into them)
};
struct QPass { const QNet* W; const QNetAct* a; const float* x; };      // a forward pass: weights, what it keeps, its observations [rows, ldf]
struct QIn { const float* x; int ld, k; };      // the input of a layer: rows of k values, ld apart
// the routes of a handle, decided once from its shape, the device and the switches (QPlanner::decide_routes)
struct QRoutes {
  bool ln = false;                // layer normalisation: per-layer launches; the chains and the one-launch act do not normalise
  bool wide = false;              // a trainable variable outgrows QW_WIDE_MIN: layer 0 cut into partial sums, tiled apply
  bool fused_q = false;           // row-local chains (q_kernels.h) instead of one GEMM launch per layer
  bool fits64 = false;            // every chain fits the 64-wide shape of the matrix-core stages
  bool want_mfma = false;         // ... and runs on them (q_mfma.h)
  bool l0_chain = false;          // ... with layer 0 inside the chain: no q_l0 GEMM launch in front
  bool qapply_lds = false;        // the device holds the LDS of q_reduce_clip_adam_kernel
  bool qapply_feasible = false;   // the fused apply launch is certain to exist
  bool q_chain = false;           // loss + weight gradients inside the backward chains (q_chain.h)
  bool late = false;              // ... the towers' weight gradients formed by the trunk launch
  bool rows_fit = false;          // B <= GRL_QAPPLY_THREADS: launches that carry per-row work of the minibatch on one block
};
// static LDS of q_reduce_clip_adam_kernel (~71 KB: fits gfx950's 160 KB)
inline int qapply_lds_bytes() { return (int)(GRL_QAPPLY_MAX * 4 + GRL_QAPPLY_THREADS * 4 + 3 * 256 * 4); }

// plan_q as a list of steps: what they share lives here, everything that outlasts the plan in grl_ctx
struct QPlanner {
  typedef grl_ctx::BwdPart BwdPart;
  grl_ctx& h;
  const grl_config& c;
  const int D, nb, Lc, B, NA, ldf;
  // the output gradients, which the weight-gradient GEMM fetches 16 bytes at a time: every branch's bins start 16-byte aligned
  // (nbp floats apart), the value gradient has a row stride of 4; the padding stays zero
  const int nbp, ld_dv = 4;
  const int hdim;                 // width the towers read: the trunk's last layer, else the observation
  const int max_Lt;               // hidden levels of the deepest tower
  QRoutes r;
  QNet on, tg;                    // online and target network
  QNetAct net[3], gact, aact;     // online(s), online(s'), target(s'); gradients; act path
  const float* P = nullptr;
  // 1 once the plan ends with the fused reduction + clip + Adam launch: the loss launch then leaves its batch sums to it
  // (no device-scope fence / last-workgroup pass) and the gather launch fixes the Adam step size.  Read at launch time.
  std::shared_ptr<int> q_defer = std::make_shared<int>(0);
  std::shared_ptr<GatherArgs> q_ga = std::make_shared<GatherArgs>();   // the minibatch gather of this plan (the prioritised sampler can run it)
  float* q_row_part = nullptr;
  int q_finish = 0;
  int q_l0_split = 0;             // partial sums of the q_l0 launch of a wide handle (0: no such launch, or not cut)
  int ln_tensors = 0;
  QFusedArgs qf;
  QLossArgs q_loss_args;
  // the forward launch that also opens the update (Adam step size) and the trunk launch carrying the priority write-back +
  // the block-sum refresh: the launches of the four-launch multi-update calls ("per_pf" / "q_pf")
  Op fwd_tick_op, bwd_wb_op;
  bool have_fwd_tick = false, have_bwd_wb = false;

  explicit QPlanner(grl_ctx& ctx)
      : h(ctx), c(ctx.cfg), D(c.q_branches), nb(c.q_bins), Lc(c.q_n_common), B(c.batch_size), NA(std::max(1, c.act_batch)),
        ldf((int)rup(c.obs_dim, 4)), nbp((int)rup(c.q_bins, 4)), hdim(Lc > 0 ? c.q_common[Lc - 1] : c.obs_dim),
        max_Lt(std::max(c.q_n_branch, c.q_n_value)) {
    on.trunk = QStack("common_net", c.q_common, c.q_n_common, 0);
    on.tower.assign(D, QStack("action_value", c.q_branch, c.q_n_branch, nb));
    on.tower.push_back(QStack("state_value", c.q_value, c.q_n_value, 1));
    tg = on;
    r.ln = c.q_layer_norm != 0;
    memset(q_ga.get(), 0, sizeof(GatherArgs));
    memset(&qf, 0, sizeof(qf));
    memset(&q_loss_args, 0, sizeof(q_loss_args));
  }

  // ---------------- layout (TF creation order of the shipped zips)
  // layer normalisation in front of every hidden layer's ReLU: tf.contrib.layers.layer_norm creates `LayerNorm[_k]/beta:0`, then
  // `/gamma:0`, inside the scope that holds the layer, behind the layer's own variables (no shipped model pins it)
  void add_net(const std::string& pre, QNet& N, bool tr) {
    auto numbered = [](const char* base, int k) { return k == 0 ? std::string(base) : base + ("_" + std::to_string(k)); };
    std::string scope;
    int k_fc = 0, k_ln = 0, in = c.obs_dim;
    for (int i = 0; i < N.n_stacks(); ++i) {
      QStack& S = N.stack(i);
      if (S.scope != scope) { scope = S.scope; k_fc = k_ln = 0; }     // (the branches share a scope: its counts run on over them)
      int d = i == 0 ? c.obs_dim : in;
      for (int l = 0; l < S.L() + (S.out ? 1 : 0); ++l) {
        const bool hidden = l < S.L();
        const int n = hidden ? S.width[l] : S.out;
        const std::string fc = pre + "/" + scope + "/" + numbered("fully_connected", k_fc++);
        S.w.push_back(h.add_var(fc + "/weights:0", {d, n}, tr));
        S.b.push_back(h.add_var(fc + "/biases:0", {n}, tr));
        if (hidden && r.ln) {
          const std::string lnn = pre + "/" + scope + "/" + numbered("LayerNorm", k_ln++);
          S.beta.push_back(h.add_var(lnn + "/beta:0", {n}, tr));
          S.gam.push_back(h.add_var(lnn + "/gamma:0", {n}, tr));
        }
        d = n;
      }
      if (i == 0) in = d;          // the towers read the trunk's last layer
    }
  }
  void layout() {
    h.cnn = false;
    h.qD = D; h.qN = nb;
    h.A = D; h.L = 0; h.B = B; h.NA = NA;
    h.img_elems = c.obs_dim; h.F = c.obs_dim; h.Fc = 0; h.ldf = ldf; h.C_img = 0; h.hw = c.img_hw;
    const std::string scope = c.algo == GRL_ALGO_DQN ? "deepq" : "bdq";
    h.add_var(scope + "/eps:0", {}, false);   // exploration epsilon: stored with the model, never trained
    h.q_online_off = h.n_params;
    add_net(scope + "/model", on, true);
    h.q_online_n = h.n_params - h.q_online_off;
    h.n_train = h.n_params;       // eps sits inside the bucket with a permanently zero gradient
    h.tgt_off = h.n_params;
    add_net(scope + "/target_q_func/model", tg, false);
    h.vf_off = 0; h.n_polyak = 0; h.ent_off = 0;
    for (int k = 0; k < 8; ++k) h.enc_w[k] = nullptr;
  }

  // ---------------- routes
  void decide_routes() {
    const Switches& sw = h.sw;
    // A handle is WIDE when a trainable variable outgrows the largest one of the vector-observation networks (an MLP over a
    // flattened image): layer 0 of the chains is cut into partial sums and the apply runs tiled (q_wide_kernels.h).  Every
    // other handle keeps its launch list.
    int64_t largest = 0;
    for (auto& v : h.vars) if (v.trainable) largest = std::max(largest, v.numel);
    r.wide = largest > QW_WIDE_MIN;
    r.rows_fit = B <= GRL_QAPPLY_THREADS;
    r.qapply_lds = device_lds_bytes() >= qapply_lds_bytes();
    // row-local chains (q_kernels.h) when every width fits the head primitives; else one GEMM launch per layer
    // (layer normalisation: always the per-layer launches -- the chains and the one-launch act do not normalise)
    r.fused_q = !r.ln && sw.get(Sw::fused_q) && nb <= 64 && Lc + max_Lt <= GRL_MAX_LAYERS &&
                q_hidden_widths_all(c, [](int w) { return w <= HT_MAXW; }) && (Lc == 0 || c.q_common[Lc - 1] <= HT_MAXA);
    if (!r.fused_q) return;
    // matrix-core stages (q_mfma.h) when every width fits their 64-wide shape (GRL_TUNE q_mfma=0 keeps the VALU chains); they
    // also take layer 0 (K = obs_dim <= 128) into the chain: no GEMM launch in front of it (GRL_TUNE q_l0_chain=0 keeps it)
    r.fits64 = nb <= QM_W && D + 1 <= QM_MAXP && q_hidden_widths_all(c, [](int w) { return w >= 1 && w <= QM_W; });
    r.want_mfma = q_mfma_built() && sw.get(Sw::q_mfma) != 0 && nb <= QM_W && D + 1 <= QM_MAXP &&
                  q_hidden_widths_all(c, [](int w) { return w <= QM_W; });
    r.l0_chain = r.want_mfma && c.obs_dim <= 2 * QM_W && sw.get(Sw::q_l0_chain) != 0;
    // backward chains that form the loss and the weight gradients of their own rows (q_chain.h): five launches per update instead
    // of seven.  Needs the matrix-core chains and the fused reduction + clip + Adam launch (which sums the row-block slabs and
    // the loss's row sums); GRL_TUNE q_chain=0 keeps the loss and weight-gradient launches.  Planned only where that launch is
    // certain to exist -- its LDS fits the device and no trainable variable outgrows its gradient buffer -- so that a device /
    // shape that offers less keeps the three-launch form instead of failing at the end of the plan
    r.qapply_feasible = sw.get(Sw::fused_qapply) != 0 && r.qapply_lds && largest <= GRL_QAPPLY_MAX;
    r.q_chain = q_chain_available(r.want_mfma, r.fits64) && sw.get(Sw::q_chain) != 0 && r.qapply_feasible && qc_shape_ok(nb, D, c.obs_dim);
    // the towers' pre-activation gradients are read back by the weight-gradient workgroups of the trunk launch when there is one
    // (GRL_TUNE q_chain_late=0: every tower chain forms its slabs itself, at its end)
    r.late = r.q_chain && Lc > 0 && sw.get(Sw::q_chain_late) != 0;
  }

  // ---------------- arenas
  // where the output layers write: branch tw at column tw * stride of `adv`, the state value to `v`
  void set_out(QNetAct& a, float* adv, int stride, float* v, int ld_v) {
    a.adv = adv; a.v = v;
    for (int tw = 0; tw < D; ++tw) { a.tower[tw].out = adv + tw * stride; a.tower[tw].ld_out = D * stride; }
    a.tower[D].out = v; a.tower[D].ld_out = ld_v;
  }
  void alloc_net(QNetAct& a, int rows) {
    a.tower.resize(D + 1);
    float* adv = nullptr;
    for (int i = 0; i < on.n_stacks(); ++i) {
      if (i == D + 1) adv = h.wk.f32((int64_t)rows * D * nb);      // (taken between the branches' activations and the value tower's)
      for (int w : on.stack(i).width) a.stack(i).z.push_back(h.wk.f32((int64_t)rows * w));
    }
    set_out(a, adv, nb, h.wk.f32(rows), 1);
  }
  void arenas() {
    Arena &st = h.st, &rp = h.rp, &wk = h.wk;
    h.params = st.f32(h.n_params);
    h.adam_m = st.f32(h.n_train);
    h.adam_v = st.f32(h.n_train);
    h.sc = (DevScalars*)st.take(sizeof(DevScalars));
    h.s_mean = (double*)st.take((size_t)h.img_elems * 8);
    h.s_std = (double*)st.take((size_t)h.img_elems * 8);
    h.s_dmean = (double*)st.take(8); h.s_dstd = (double*)st.take(8);
    h.s_ret = (double*)st.take(8);
    // VecNormalize running statistics on the device (grl_norm_update / grl_observe), as on SAC handles -- behind everything the
    // arena held before them: every earlier offset stays where it was
    h.n_elems = c.obs_dim;
    h.n_count = (double*)st.take(16);
    h.n_mean = (double*)st.take((size_t)h.n_elems * 8);
    h.n_var = (double*)st.take((size_t)h.n_elems * 8);
    h.grads = h.gr.f32(h.n_train);
    const int64_t cap = c.replay_capacity;
    const int A = h.A;
    h.rp_obs = rp.f32(cap * h.img_elems); h.rp_next = rp.f32(cap * h.img_elems);
    h.rp_dobs = rp.f32(cap); h.rp_dnext = rp.f32(cap);
    h.rp_act = rp.f32(cap * A); h.rp_rew = rp.f32(cap); h.rp_done = rp.f32(cap);
    h.stg_n = std::max(NA, 64);
    const int64_t stg_obs = (int64_t)h.stg_n * c.obs_dim;
    h.stg_obs = wk.f32(stg_obs); h.stg_next = wk.f32(stg_obs);
    h.stg_act = wk.f32((int64_t)h.stg_n * A); h.stg_rew = wk.f32(h.stg_n); h.stg_done = wk.f32(h.stg_n);
    // raw observations of one env step for grl_norm_update; the observed observations of grl_observe (newest, the one before,
    // terminal rows), uploaded once each
    h.n_stage = wk.f32(stg_obs);
    h.ob_latest = wk.f32(stg_obs); h.ob_prev = wk.f32(stg_obs); h.ob_term = wk.f32(stg_obs);
    h.ob_elems = c.obs_dim;
    h.idx_buf = (int64_t*)wk.take((size_t)B * 8);
    h.eps_buf = wk.f32(std::max(B, B * A));      // importance weights [B]
    for (int n = 0; n < 3; ++n) h.feat[n] = wk.f32((int64_t)B * ldf);
    h.act = wk.f32((int64_t)B * A); h.rew = wk.f32(B); h.done = wk.f32(B);

    for (int n = 0; n < 3; ++n) alloc_net(net[n], B);
    if (r.ln)      // the differentiated pass keeps its pre-activations and the rows' statistics
      for (int i = 0; i < on.n_stacks(); ++i)
        for (int w : on.stack(i).width) {
          net[0].stack(i).u.push_back(wk.f32((int64_t)B * w));
          net[0].stack(i).stat.push_back(wk.f32(2 * (int64_t)B));
        }
    alloc_net(gact, B);                   // same shapes: gradient w.r.t. each pre-activation, except the padded output gradients
    float* d_adv = wk.f32((int64_t)B * D * nbp);
    set_out(gact, d_adv, nbp, wk.f32((int64_t)B * ld_dv), ld_dv);
    h.zero_once.push_back({gact.adv, (size_t)B * D * nbp * 4});
    h.zero_once.push_back({gact.v, (size_t)B * ld_dv * 4});
    for (int n = 0; n < 3; ++n) h.zero_once.push_back({h.feat[n], (size_t)B * ldf * 4});   // (row padding [F, ldf) is read by 16-byte loads)
    h.q_td = wk.f32((int64_t)B * D); h.q_prio = wk.f32(B);
    P = h.params;
  }

  // =============================================================== prioritised replay (per_kernels.h)
  void sampler() {
    h.per_on = c.q_per != 0;
    if (!h.per_on) return;
    const int64_t cap = c.replay_capacity;
    PerArgs& per = h.per;
    memset(&per, 0, sizeof(per));
    h.per_blocks = (int)((cap + PER_BLK - 1) / PER_BLK);
    per.p = (double*)h.rp.take((size_t)cap * 8);
    per.bsum = (double*)h.rp.take((size_t)h.per_blocks * 8);
    per.bmin = (double*)h.rp.take((size_t)h.per_blocks * 8);
    per.st = (PerState*)h.rp.take(sizeof(PerState));
    h.per_u = (double*)h.wk.take((size_t)B * 8);
    per.sc = h.sc; per.seed = c.seed; per.B = B; per.alpha = c.q_per_alpha; per.eps = c.q_per_eps;
    per.alpha64 = c.q_per_alpha64 != 0.0 ? c.q_per_alpha64 : (double)c.q_per_alpha;
    per.stratified = c.q_per_stratified != 0;
    per.idx_out = h.idx_buf; per.w_out = h.eps_buf; per.prio_in = nullptr;   // set at launch time (q_prio)
    grl_ctx* self = &h;
    auto q_ga = this->q_ga;
    auto q_defer = this->q_defer;
    for (int mode = 0; mode < 2; ++mode) {
      PerArgs pa = per;
      pa.u = mode ? h.per_u : nullptr;
      const int nb = h.per_blocks;
      for (int with_gather = 0; with_gather < 2; ++with_gather) {
        Op op; op.tag = "per_sample";
        auto sampler = [self, pa, nb, with_gather, q_ga, q_defer](bool block_sums) {
          return [self, pa, nb, with_gather, q_ga, q_defer, block_sums](hipStream_t s) {
            PerArgs q = pa;
            q.prio_in = self->q_prio;
            GatherArgs g = *q_ga;
            g.adam_tick = *q_defer;
            if (block_sums) hipLaunchKernelGGL(per_blocksum_kernel, dim3(nb), dim3(256), 0, s, q);
            hipLaunchKernelGGL(per_sample_kernel, dim3(q.B), dim3(256), 0, s, q, nb, g, with_gather);   // RNG mode: marks rng_used, q_loss ticks
          };
        };
        op.run = sampler(true);
        (with_gather ? (mode ? h.ops_per_u_g : h.ops_per_rng_g) : (mode ? h.ops_per_u : h.ops_per_rng)).push_back(op);
        if (with_gather && !mode) {     // later updates of a multi-update call: the apply launch of the update before kept the block sums current
          Op oi = op;
          oi.run = sampler(false);
          h.ops_per_rng_g_inc.push_back(oi);
        }
      }
    }
    Op op; op.tag = "per_update";
    op.run = [self](hipStream_t s) {
      PerArgs q = self->per;
      q.prio_in = self->q_prio;
      hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(256), 0, s, q, (const int64_t*)self->idx_buf);
    };
    h.ops_per_update.push_back(op);
  }

  // =============================================================== RNG (uniform indices; weights = 1) + the minibatch gather
  void draw_and_gather() {
    {
      Op op; op.tag = "rng";
      RngArgs ra{h.sc, c.seed, B, 1, h.idx_buf, h.eps_buf, h.eps_buf, 1};   // weights = 1; the loss kernel advances rng_step
      op.run = [ra](hipStream_t s) {
        hipLaunchKernelGGL(rng_kernel, dim3((ra.B + 255) / 256), dim3(256), 0, s, ra);
      };
      h.ops_rng.push_back(op);
    }
    GatherArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.idx = h.idx_buf; ga.B = B; ga.img_elems = h.img_elems; ga.n_direct = 0; ga.act_dim = h.A;
    ga.rp_obs = h.rp_obs; ga.rp_next = h.rp_next; ga.rp_dobs = h.rp_dobs; ga.rp_dnext = h.rp_dnext;
    ga.rp_act = h.rp_act; ga.rp_rew = h.rp_rew; ga.rp_done = h.rp_done;
    ga.mean = h.s_mean; ga.stdv = h.s_std; ga.dmean = h.s_dmean; ga.dstd = h.s_dstd; ga.ret_std = h.s_ret;
    ga.normalize = (c.normalize == 1 || c.normalize == 2); ga.normalize_rew = (c.normalize == 1 || c.normalize == 3);
    ga.clip_obs = c.clip_obs; ga.clip_rew = c.clip_reward; ga.scale_div = 1.f;
    ga.x_obs = h.feat[0]; ga.x_obs2 = nullptr; ga.x_next = h.feat[2]; ga.ldx = ldf;
    ga.d_obs0 = ga.d_obs1 = ga.d_next = h.feat[0]; ga.ldd = ldf;
    ga.act_out = h.act; ga.ld_act = h.A; ga.rew_out = h.rew; ga.done_out = h.done;
    ga.sc = h.sc;
    *q_ga = ga;
    Op op; op.tag = "gather_norm";
    auto q_defer = this->q_defer;
    op.run = [ga, q_defer](hipStream_t s) {
      GatherArgs g2 = ga;
      g2.adam_tick = *q_defer;        // deferred loss sums: the Adam step size of the update is fixed here, as in the SAC plan
      launch_gather(g2, (g2.img_elems + 255) / 256, s);      // (scalar form, one row per workgroup)
    };
    h.ops_grads.push_back(op);
  }

  // =============================================================== forward
  // one ln_relu_fwd / ln_relu_bwd launch over all tensors of a layer level (ln_kernels.h)
  void add_ln(std::vector<Op>& ops, const char* tag, bool bwd, const std::vector<LnDesc>& descs, int rows) {
    if (descs.empty()) return;
    int npl = 1;
    for (auto& d : descs) npl = std::max(npl, ln_npl(d.H));
    const LnDesc* dd = h.upload_vec(h.wk, descs);
    const int nd = (int)descs.size();
    Op op; op.tag = tag;
    if (bwd) op.run = [dd, nd, rows, npl](hipStream_t s) { launch_ln_relu_bwd(dd, nd, rows, npl, s); };
    else op.run = [dd, nd, rows, npl](hipStream_t s) { launch_ln_relu_fwd(dd, nd, rows, npl, s); };
    ops.push_back(op);
    ln_tensors += nd;
  }
  // The forward passes as one GEMM launch per level (trunk layers, tower layers, output layers): the problems of a launch keep the
  // order of the passes, and inside a pass branches, then value.
  // (layer normalisation: the dense launches leave the pre-activations -- beside the activations where the pass keeps them,
  //  else in their place -- and the ln_relu_fwd launch behind each level turns them into the activations)
  void add_forward(std::vector<Op>& ops, const std::vector<QPass>& passes, int rows, const char* tag, const char* ln_tag) {
    std::vector<std::vector<IgemmProb>> level(Lc + max_Lt + 1);
    std::vector<std::vector<LnDesc>> ln(level.size());
    for (auto& p : passes) {
      QIn in{p.x, ldf, c.obs_dim}, trunk_end = in;
      for (int i = 0; i < p.W->n_stacks(); ++i) {
        const QStack& T = p.W->stack(i);
        const QStackAct& ta = p.a->stack(i);
        const int base = i == 0 ? 0 : Lc;
        const bool keep = !ta.u.empty();
        if (i > 0) in = trunk_end;
        for (int l = 0; l < T.L(); ++l) {
          float* pre = keep ? ta.u[l] : ta.z[l];
          level[base + l].push_back(h.dense_fwd(in.x, in.ld, in.k, nullptr, 0, 0, rows, P + T.w[l], T.width[l], P + T.b[l], pre, T.width[l],
                                                r.ln ? ACT_NONE : ACT_RELU));
          if (r.ln) {
            LnDesc d;
            memset(&d, 0, sizeof(d));
            d.u = pre; d.z = ta.z[l]; d.gamma = P + T.gam[l]; d.beta = P + T.beta[l]; d.stat = keep ? ta.stat[l] : nullptr; d.H = T.width[l];
            ln[base + l].push_back(d);
          }
          in = QIn{ta.z[l], T.width[l], T.width[l]};
        }
        if (i == 0) trunk_end = in;
        else level.back().push_back(h.dense_fwd(in.x, in.ld, in.k, nullptr, 0, 0, rows, P + T.w[T.L()], T.out, P + T.b[T.L()], ta.out, ta.ld_out, ACT_NONE));
      }
    }
    for (size_t l = 0; l < level.size(); ++l) { h.add_launch(ops, tag, 0, level[l]); add_ln(ops, ln_tag, false, ln[l], rows); }
  }
  std::vector<QPass> train_passes() const { return {{&on, &net[0], h.feat[0]}, {&on, &net[1], h.feat[2]}, {&tg, &net[2], h.feat[2]}}; }
  int forward() {
    if (r.fused_q) return forward_chains();
    add_forward(h.ops_grads, train_passes(), B, "q_fwd", "q_ln_fwd");
    return GRL_OK;
  }
  // the hidden layers [l0, l1) of stack T as layers li ... of a chain: weights, widths and -- forward -- where the activations
  // are stored (z), -- backward -- where they are read and the pre-activation gradients written (z and g)
  static int chain_layers(HtHead& hd, int li, const QStack& T, int l0, int l1, const float* P, const QStackAct* z, const QStackAct* g, bool bias) {
    for (int l = l0; l < l1; ++l, ++li) {
      hd.w[li] = P + T.w[l]; hd.hid[li] = T.width[l];
      if (bias) hd.b[li] = P + T.b[l];
      hd.z[li] = z ? z->z[l] : nullptr;
      if (g) hd.g[li] = g->z[l];
    }
    return li;
  }
  // ---- row-local chains (q_kernels.h): forward of the three passes as one launch, backward views of the online net on s
  int forward_chains() {
    Arena& wk = h.wk;
    const std::vector<QPass> passes = train_passes();
    std::vector<HtHead> hf, hb;
    std::vector<IgemmProb> l0;
    // wide handle: three to six problems of one tile each would walk K = obs_dim alone -- the reduction is cut (set_split) until
    // the launch has at least 64 tiles, from B, H and K; the chains add the partial sums in index order before bias and
    // activation (HtHead.u_split, as the SAC heads do)
    auto l0_gemm = [&](const float* x, const float* w, int H0, float*& u) {      // layer 0 as a GEMM (K = obs_dim), no bias / activation (applied by the chain)
      IgemmProb p = h.dense_fwd(x, ldf, c.obs_dim, nullptr, 0, 0, B, w, H0, nullptr, nullptr, H0, ACT_NONE);
      if (r.wide) {
        const int n_prob = 3 * (Lc > 0 ? 1 : D + 1);
        const int base = n_prob * ((B + 63) / 64) * ((H0 + 63) / 64);
        h.set_split(p, (64 + base - 1) / base);
        q_l0_split = std::max(q_l0_split, p.split);
      }
      u = wk.f32((int64_t)B * H0 * p.split);
      p.c = u;
      l0.push_back(p);
    };
    for (auto& pass : passes) {
      const QNet& W = *pass.W;
      const QNetAct& a = *pass.a;
      float* u_trunk = nullptr;
      if (Lc > 0 && !r.l0_chain) l0_gemm(pass.x, P + W.trunk.w[0], W.trunk.width[0], u_trunk);
      for (int tw = 0; tw <= D; ++tw) {
        const QStack& T = W.tower[tw];
        const QStack& S0 = Lc > 0 ? W.trunk : T;      // the stack that holds layer 0 of the chain
        HtHead hd;
        memset(&hd, 0, sizeof(hd));
        float* u = u_trunk;
        if (r.l0_chain) { hd.xa = pass.x; hd.ld_xa = ldf; hd.n_xa = c.obs_dim; hd.w0a = P + S0.w[0]; }
        else if (Lc == 0) l0_gemm(pass.x, P + T.w[0], T.width[0], u);      // no trunk: layer 0 of every tower from the GEMM launch
        const int split = Lc > 0 ? q_l0_split : (u ? l0.back().split : 0);
        if (u && split > 1) { hd.u_split = split; hd.u_stride = (long)B * S0.width[0]; }
        hd.u = u; hd.ldu = S0.width[0]; hd.b0 = P + S0.b[0]; hd.H0 = S0.width[0]; hd.hid[0] = hd.H0;
        if (Lc > 0) {      // the trunk is recomputed per tower, stored once
          hd.z0 = tw == 0 ? a.trunk.z[0] : nullptr;
          const int li = chain_layers(hd, 1, W.trunk, 1, Lc, P, tw == 0 ? &a.trunk : nullptr, nullptr, true);
          hd.L = chain_layers(hd, li, T, 0, T.L(), P, &a.tower[tw], nullptr, true);
        } else {
          hd.z0 = a.tower[tw].z[0];
          hd.L = chain_layers(hd, 1, T, 1, T.L(), P, &a.tower[tw], nullptr, true);
        }
        hd.n_out = 1; hd.out_dim = T.out;
        hd.ow[0] = P + T.w[T.L()]; hd.ob[0] = P + T.b[T.L()];
        hd.out[0] = a.tower[tw].out; hd.ld_out = a.tower[tw].ld_out;
        hf.push_back(hd);
      }
    }
    // backward views of the online net on s
    const QNetAct& a = net[0];
    auto bwd_view = [&](const QStack& T, const QStackAct& z, const QStackAct& g) {
      HtHead hd;
      memset(&hd, 0, sizeof(hd));
      hd.H0 = T.width[0]; hd.hid[0] = hd.H0;
      hd.z0 = z.z[0]; hd.g0 = g.z[0]; hd.ldg0 = hd.H0;
      hd.L = chain_layers(hd, 1, T, 1, T.L(), P, &z, &g, false);
      return hd;
    };
    for (int tw = 0; tw <= D; ++tw) {
      const QStack& T = on.tower[tw];
      HtHead hd = bwd_view(T, a.tower[tw], gact.tower[tw]);
      if (Lc > 0) { hd.n_xa = hdim; hd.w0a = P + T.w[0]; }
      hd.n_out = 1; hd.out_dim = T.out; hd.ow[0] = P + T.w[T.L()];
      hb.push_back(hd);
    }
    qf.B = B; qf.D = D; qf.nb = nb; qf.Ht = Lc > 0 ? hdim : 0;
    qf.d_adv = gact.adv; qf.d_v = gact.v; qf.nbp = nbp; qf.ld_dv = ld_dv; qf.trunk_scale = c.q_trunk_scale;
    std::vector<HtHead> htr;
    if (Lc > 0) {
      htr.push_back(bwd_view(on.trunk, a.trunk, gact.trunk));
      qf.dh_part = wk.f32((int64_t)(D + 1) * B * qf.Ht);
    }
    // the routes were decided from the shape alone: every chain as it was built fits the stages it was planned for
    bool fit = nb <= QM_W && D + 1 <= QM_MAXP;
    for (auto& hd : htr) fit = fit && qm_head_ok(hd, false);
    for (auto& hd : hb) fit = fit && qm_head_ok(hd);
    for (auto& hd : hf) fit = fit && qm_head_ok(hd, true, true);
    if (r.want_mfma && !fit) return fail(GRL_ERR_INVALID, "internal: the Q chains were planned for the matrix-core stages and do not fit them");
    qf.mfma = r.want_mfma;
    if (r.q_chain) {      // nothing reads the trunk's pre-activation gradients from memory any more: its chain keeps them in LDS;
      // the towers' only where the trunk launch forms their weight gradients (late)
      auto no_g = [](HtHead& hd) { hd.g0 = nullptr; for (int l = 0; l < GRL_MAX_LAYERS; ++l) hd.g[l] = nullptr; };
      if (!r.late) for (auto& hd : hb) no_g(hd);
      for (auto& hd : htr) no_g(hd);
    }
    qf.fwd = h.upload_vec(wk, hf);
    qf.bwd_tw = h.upload_vec(wk, hb);
    if (!htr.empty()) qf.bwd_tr = h.upload_vec(wk, htr);
    plan_note("grl plan: q chains       %s%s\n", qf.mfma ? "matrix-core stages (q_mfma.h)" : "VALU stages (q_kernels.h)",
              r.q_chain ? ", loss + weight gradients inside the backward chains (q_chain.h)" : "");
    if (!l0.empty()) h.add_launch(h.ops_grads, "q_l0", 0, l0);
    Op op; op.tag = "q_fwd";
    const QFusedArgs fa = qf;
    op.run = [fa](hipStream_t s) { launch_q_fwd(fa, s); };
    h.ops_grads.push_back(op);
    // the same launch opening the update (Adam step size): the "per_pf" updates
    QFusedArgs ft = qf;
    ft.tick_sc = h.sc;
    fwd_tick_op = op;
    fwd_tick_op.run = [ft](hipStream_t s) { launch_q_fwd(ft, s); };
    have_fwd_tick = true;
    return GRL_OK;
  }

  // =============================================================== loss
  void loss() {
    QLossArgs qa;
    qa.B = B; qa.D = D; qa.n = nb; qa.gamma = c.gamma; qa.lr = c.lr; qa.huber = c.q_huber; qa.double_q = c.q_double;
    qa.adv0 = net[0].adv; qa.v0 = net[0].v; qa.adv1 = net[1].adv; qa.adv2 = net[2].adv; qa.v2 = net[2].v;
    qa.act = h.act; qa.rew = h.rew; qa.done = h.done; qa.weights = h.eps_buf;
    qa.d_adv0 = gact.adv; qa.d_v0 = gact.v; qa.nbp = nbp; qa.ld_dv = ld_dv; qa.td = h.q_td; qa.priority = h.q_prio; qa.sc = h.sc;
    qa.row_part = h.wk.f32(3 * (int64_t)B);
    qa.counter = (unsigned*)h.wk.take(16);
    qa.defer_finish = 0;
    qa.loss_sum = (c.algo == GRL_ALGO_BDQ && c.q_loss_sum_branches) ? 1 : 0;
    h.zero_once.push_back({qa.counter, 16});
    q_row_part = qa.row_part;
    q_finish = q_loss_finishes_itself(qa.n) ? 1 : 0;     // (the one-workgroup fallback for > 64 bins forms its sums itself)
    q_loss_args = qa;
    if (r.q_chain) return;      // (the backward chains form it)
    Op op; op.tag = "q_loss";
    auto q_defer = this->q_defer;
    op.run = [qa, q_defer](hipStream_t s) {
      QLossArgs q2 = qa;
      q2.defer_finish = *q_defer;
      launch_q_loss(q2, s);
    };
    h.ops_grads.push_back(op);
  }

  // =============================================================== backward (online net on s)
  // gradient slabs (one per block of rows) the reduction sums into the bucket at `off`
  void add_reduce(const float* src, int splits, int64_t slab_stride, int64_t off, int n) {
    ReduceDesc rd;
    memset(&rd, 0, sizeof(rd));
    rd.src = src; rd.splits = splits; rd.slab_stride = slab_stride; rd.dst = h.grads + off; rd.n = n;
    h.reduces.push_back(rd);
  }
  void backward() {
    if (r.q_chain) return backward_chained();
    if (r.fused_q) {
      const QFusedArgs fa = qf;
      Op op; op.tag = "q_bwd";
      op.run = [fa](hipStream_t s) { launch_q_bwd(fa, s); };
      h.ops_grads.push_back(op);
    } else {
      backward_layers();
    }
    weight_grads();
  }
  // the chained backward: one slab per row block and variable; the apply launch sums them in row-block order
  void backward_chained() {
    Arena& wk = h.wk;
    const int n_rb = (B + HT_RB - 1) / HT_RB;
    auto slabs = [&](const QStack& T, const float* xin, int ld_xin, int kin) {
      QcHead y;
      memset(&y, 0, sizeof(y));
      y.xin = xin; y.ld_xin = ld_xin;
      for (int l = 0; l < T.L() + (T.out ? 1 : 0); ++l) {
        QcLayer& lay = y.lay[l];
        lay.K = kin; lay.N = l < T.L() ? T.width[l] : T.out;
        lay.dw = wk.f32((int64_t)n_rb * lay.K * lay.N); lay.db = wk.f32((int64_t)n_rb * lay.N);
        add_reduce(lay.dw, n_rb, (int64_t)lay.K * lay.N, T.w[l], lay.K * lay.N);
        add_reduce(lay.db, n_rb, lay.N, T.b[l], lay.N);
        kin = lay.N;
      }
      return y;
    };
    std::vector<QcHead> ytw;
    for (auto& T : on.tower) ytw.push_back(slabs(T, Lc > 0 ? net[0].trunk.z[Lc - 1] : h.feat[0], Lc > 0 ? hdim : ldf, hdim));
    QChainArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.f = qf; ca.l = q_loss_args; ca.l.defer_finish = 1;
    ca.late = r.late ? 1 : 0;
    ca.tw = h.upload_vec(wk, ytw);
    if (Lc > 0) ca.tr = h.upload_vec(wk, std::vector<QcHead>{slabs(on.trunk, h.feat[0], ldf, c.obs_dim)});
    Op op; op.tag = "q_bwd";
    op.run = [ca](hipStream_t s) { launch_q_bwd_chain(ca, s); };
    h.ops_grads.push_back(op);
    if (h.per_on && Lc > 0 && r.rows_fit) {      // the trunk launch carrying the priority write-back + the block-sum refresh ("per_pf")
      grl_ctx* self = &h;
      const int rows = B;
      bwd_wb_op = op;
      bwd_wb_op.run = [ca, self, rows](hipStream_t s) {
        QChainArgs c2 = ca;
        c2.per = self->per;
        c2.per.prio_in = self->q_prio;
        c2.per_idx = (const int64_t*)self->idx_buf;
        c2.per_wb = rows;
        launch_q_bwd_chain(c2, s);
      };
      have_bwd_wb = true;
    }
  }
  // one backward-data launch per level, towers first, then into and down the trunk
  // (layer normalisation: the backward-data launches leave the gradient w.r.t. the layer's OUTPUT (no ReLU mask) and one
  //  ln_relu_bwd launch per level turns it, in place, into the gradient w.r.t. the pre-activation that the next
  //  backward-data launch and the weight-gradient launch read; beta / gamma gradients leave as slabs per block of rows)
  void backward_layers() {
    std::vector<Op>& ops = h.ops_grads;
    auto relu_mask = [&](const float* z) { return r.ln ? nullptr : z; };
    // what flows into hidden layer l of a stack from the layer above it (the output layer above the last hidden one)
    auto from_above = [&](const QStack& T, const QStackAct& g, int l) {
      if (l + 1 == T.L()) return BwdPart{g.out, g.ld_out, T.out, P + T.w[l + 1]};
      return BwdPart{g.z[l + 1], T.width[l + 1], T.width[l + 1], P + T.w[l + 1]};
    };
    auto ln_bwd = [&](const QStack& T, const QStackAct& a, const QStackAct& g, int l) {
      LnDesc d;
      memset(&d, 0, sizeof(d));
      const int H = T.width[l];
      d.u = a.u[l]; d.stat = a.stat[l]; d.gamma = P + T.gam[l]; d.beta = P + T.beta[l]; d.dz = g.z[l]; d.H = H;
      const int n_sl = ln_bwd_slabs(B);
      d.slab = h.wk.f32((int64_t)n_sl * 2 * H);
      add_reduce(d.slab, n_sl, 2 * (int64_t)H, T.beta[l], H);
      add_reduce(d.slab + H, n_sl, 2 * (int64_t)H, T.gam[l], H);
      return d;
    };
    // level `up` of the towers (max_Lt: their output layers) -> the hidden layer below it, of every tower that has one there
    for (int up = max_Lt; up >= 1; --up) {
      std::vector<IgemmProb> pr;
      std::vector<LnDesc> lt;
      for (int tw = 0; tw <= D; ++tw) {
        const QStack& T = on.tower[tw];
        const int l = up == max_Lt ? T.L() - 1 : (up < T.L() ? up - 1 : -1);
        if (l < 0) continue;
        pr.push_back(h.dense_bwd({from_above(T, gact.tower[tw], l)}, B, 0, T.width[l], gact.tower[tw].z[l], T.width[l],
                                 relu_mask(net[0].tower[tw].z[l])));
        if (r.ln) lt.push_back(ln_bwd(T, net[0].tower[tw], gact.tower[tw], l));
      }
      h.add_launch(ops, "q_bwd", 1, pr);
      add_ln(ops, "q_ln_bwd", true, lt, B);
    }
    if (Lc == 0) return;
    // into the shared trunk: sum over the D+1 towers in chunks of three reduction parts
    const QStack& T = on.trunk;
    std::vector<BwdPart> towers;
    for (int tw = 0; tw <= D; ++tw) towers.push_back({gact.tower[tw].z[0], on.tower[tw].width[0], on.tower[tw].width[0], P + on.tower[tw].w[0]});
    for (size_t t0 = 0; t0 < towers.size(); t0 += 3) {
      std::vector<BwdPart> chunk(towers.begin() + t0, towers.begin() + std::min(towers.size(), t0 + 3));
      const bool last = t0 + 3 >= towers.size();
      IgemmProb p = h.dense_bwd(chunk, B, 0, hdim, gact.trunk.z[Lc - 1], hdim, last ? relu_mask(net[0].trunk.z[Lc - 1]) : nullptr);
      p.accumulate = t0 > 0 ? 1 : 0;
      p.out_scale = c.q_trunk_scale;
      h.add_launch(ops, "q_bwd", 1, {p});
    }
    if (r.ln) add_ln(ops, "q_ln_bwd", true, {ln_bwd(T, net[0].trunk, gact.trunk, Lc - 1)}, B);
    for (int k = Lc - 1; k >= 1; --k) {
      h.add_launch(ops, "q_bwd", 1, {h.dense_bwd({from_above(T, gact.trunk, k - 1)}, B, 0, T.width[k - 1], gact.trunk.z[k - 1], T.width[k - 1],
                                                 relu_mask(net[0].trunk.z[k - 1]))});
      if (r.ln) add_ln(ops, "q_ln_bwd", true, {ln_bwd(T, net[0].trunk, gact.trunk, k - 1)}, B);
    }
  }
  // weight gradients (not here when the chained backward has formed them)
  void weight_grads() {
    std::vector<IgemmProb> wg;
    // the trunk (no output layer) reads the observations, every tower the trunk's end
    const QIn obs{h.feat[0], ldf, c.obs_dim}, trunk_end = Lc > 0 ? QIn{net[0].trunk.z[Lc - 1], hdim, hdim} : obs;
    for (int i = 0; i < on.n_stacks(); ++i) {
      const QStack& T = on.stack(i);
      const QStackAct &a = net[0].stack(i), &g = gact.stack(i);
      const QIn& in = i == 0 ? obs : trunk_end;
      h.add_stack_wgrads(wg, in.x, in.ld, in.k, a.z.data(), g.z.data(), T.width.data(), T.L(), g.out, g.ld_out, T.out, T.w.data(), T.b.data(), B);
    }
    h.add_launch(h.ops_grads, "q_wgrad", 2, wg);
  }

  // =============================================================== slab reduction, then clip + Adam as launches of their own
  void reduction() {
    const grl_ctx::SumPlan sum = h.close_reduction();
    h.d_reduces = sum.descs;
    h.ops_grads.push_back(sum.op);
    // (the in-graph exchange publishes from this reduction: capi.inl, grl_allreduce_connect)
    h.red_all.tiles = sum.tiles; h.red_all.n = sum.n; h.red_all.has_loss = 0;
    AdamArgs& ab = h.adam_base;
    memset(&ab, 0, sizeof(ab));
    ab.params = h.params; ab.grads = h.grads; ab.m = h.adam_m; ab.v = h.adam_v; ab.n_train = h.n_train; ab.sc = h.sc;
    ab.grad_scale = 1.f; ab.eps = 1e-8f; ab.target = h.params + h.tgt_off;
    memset(&h.loss_args, 0, sizeof(h.loss_args));
  }
  void apply() {
    const std::vector<VarSeg> segs = h.trainable_segs();
    float* g = h.grads; const float clip = c.q_grad_clip;
    grl_ctx* self = &h;
    if (r.wide && clip > 0.f) {
      // wide handle: clip_by_norm (one workgroup per variable) + Adam become two launches over a tile table (q_wide_kernels.h).
      // Data parallel: as below, the sum of the replicas is clipped at clip / grad_scale and Adam's 1 / W brings it back.
      const int n_tl = h.add_clip_adam(h.ops_apply, segs, clip, 1e-8f, false, true);
      plan_note("grl plan: q_wide        apply: q_sumsq + q_clip_adam, %d tiles of <= %d floats over %zu variables; q_l0: %d partial sums (B %d, K %d)\n",
                n_tl, QW_TILE, segs.size(), std::max(1, q_l0_split), B, c.obs_dim);
      return;
    }
    if (clip > 0.f) {   // per-variable tf.clip_by_norm, after the data-parallel all-reduce point
      VarSeg* d_segs = h.upload_vec(h.wk, segs);
      const int nseg = (int)segs.size();
      Op op; op.tag = "clip_by_norm";
      // data parallel (grl_apply_grads(1 / W) on the all-reduced SUM of W replicas): clip(mean, c) * W == clip(sum, W c), so the
      // sum is clipped at clip / grad_scale and Adam's 1 / W brings it back -- the mean of the replicas clipped as one gradient
      op.run = [self, g, d_segs, nseg, clip](hipStream_t s) {
        hipLaunchKernelGGL(clip_by_norm_kernel, dim3(nseg), dim3(256), 0, s, g, d_segs, clip / self->grad_scale);
      };
      h.ops_apply.push_back(op);
    }
    h.ops_apply.push_back(h.adam_op("adam", 1e-8f, false, true));
  }

  // =============================================================== full updates: reduction + clip + Adam as one launch
  // The launch that ends an update (q_reduce_clip_adam_kernel), one workgroup per reduction descriptor and behind them
  //   with_per:     one more workgroup writes the new priorities back (per_update_kernel's work)
  //   refresh:      one more workgroup per sample rebuilds the block sums its new priority touches (per_refresh_body)
  //   next_sampler: write-back and refresh rode on the trunk launch; B workgroups draw the NEXT update's minibatch
  //   next_uniform: the riders draw row b's index with counter + 1 themselves (the draw of rng_kernel), leave it in idx_buf and
  //                 gather the row; the importance weights stay the ones the call's first update wrote
  std::function<void(hipStream_t)> apply_op(bool with_per, bool refresh = false, bool next_sampler = false, bool next_uniform = false) {
    grl_ctx* self = &h;
    const ReduceDesc* dr = h.d_reduces;
    const int nd = (int)h.reduces.size();
    const float clip = c.q_grad_clip;
    const float* rp = q_row_part; const int rows = B, fin = q_finish;
    auto qga = q_ga;      // (shared with the samplers: the minibatch gather of this plan)
    const int q_gx = (h.img_elems + 255) / 256;      // tiles per row of gather_norm_kernel on this plan (scalar form)
    return [self, dr, nd, clip, rp, rows, fin, with_per, refresh, next_sampler, next_uniform, qga, q_gx](hipStream_t s) {
      const AdamArgs aa = self->adam_args(self->grad_scale, false);
      PerArgs q = self->per;
      q.prio_in = self->q_prio;
      const int n_extra = (next_sampler || next_uniform) ? 1 : (with_per ? 2 : 1) + (refresh ? rows : 0);
      QNextArgs nx;
      memset(&nx, 0, sizeof(nx));
      int n_next = 0;
      if (next_sampler) {
        nx.per = q; nx.per.u = nullptr;
        nx.g = *qga; nx.g.adam_tick = 0;          // (the next update's forward launch fixes its Adam step size)
        nx.n_sample = rows; nx.n_blocks = self->per_blocks;
        n_next = rows;
      } else if (next_uniform) {
        nx.g = *qga; nx.g.adam_tick = 0; nx.g.use_rng = 1; nx.g.rng_ahead = 1; nx.g.quiet = 1;
        nx.g.seed = self->cfg.seed; nx.g.idx_w = self->idx_buf; nx.g.n_eps = 0;
        nx.uniform_gx = q_gx;
        n_next = q_gx * nx.g.B * 2;
      }
      // (finish bit 1 = leave the Philox counter alone: the riders of this launch read it; prioritised: the trunk launch
      //  advanced it already; uniform: the next update's forward launch will)
      hipLaunchKernelGGL(q_reduce_clip_adam_kernel, dim3(nd + n_extra + n_next), dim3(GRL_QAPPLY_THREADS), 0, s, dr, nd, clip,
                         aa, rp, rows, fin | ((next_sampler || next_uniform) ? 2 : 0), q, (const int64_t*)self->idx_buf, n_extra, nx);
    };
  }
  static Op q_apply(std::function<void(hipStream_t)> run) {
    Op op; op.tag = "q_apply";
    op.run = std::move(run);
    return op;
  }
  int fused_apply() {
    // when every trainable variable is exactly one reduction descriptor and fits the kernel's LDS buffer, and the device holds
    // that LDS (any that offers less keeps the three launches).  GRL_TUNE fused_qapply=0 keeps the three launches.
    bool ok = h.sw.get(Sw::fused_qapply) && !h.ops_grads.empty() && h.ops_grads.back().tag == "reduce_slabs";
    size_t n_tr = 0;
    for (auto& v : h.vars) {
      if (!v.trainable) continue;
      ++n_tr;
      int hits = 0;
      for (auto& rd : h.reduces) hits += (rd.dst == h.grads + v.off && rd.n == v.numel && rd.n <= GRL_QAPPLY_MAX) ? 1 : 0;
      ok = ok && hits == 1;
    }
    ok = ok && n_tr == h.reduces.size();
    for (auto& rd : h.reduces) ok = ok && rd.row_len == 0;     // the kernel reads plain (non-strided) slabs
    ok = ok && r.qapply_lds;
    plan_note("grl plan: q_apply       reduction + clip + Adam in one launch: %s (%zu variables)\n", ok ? "yes" : "no", n_tr);
    if (ok) {
      h.ops_grads_apply.assign(h.ops_grads.begin(), h.ops_grads.end() - 1);
      h.ops_grads_apply.push_back(q_apply(apply_op(false)));
      if (h.per_on && r.rows_fit) {
        for (size_t k = 0; k + 1 < h.ops_grads_apply.size(); ++k)
          if (h.ops_grads_apply[k].tag != "gather_norm") h.ops_grads_apply_per.push_back(h.ops_grads_apply[k]);   // (the sampler gathers its rows)
        h.ops_grads_apply_per.push_back(q_apply(apply_op(true)));
        if (h.sw.get(Sw::per_inc) && !h.ops_per_rng_g_inc.empty()) {      // multi-update calls on the device RNG (capi: grl_train_step_per)
          h.ops_grads_apply_per_r = h.ops_grads_apply_per;
          h.ops_grads_apply_per_r.back().run = apply_op(true, true);
        }
        plan_per_pf();
      }
      if (!h.per_on && h.sw.get(Sw::q_pf) && have_fwd_tick && q_finish && r.rows_fit) plan_q_pf();
      *q_defer = 1;
      if (q_finish) {     // split compute / apply path of this plan: the batch means as a launch of their own, behind the reduction
        Op fo; fo.tag = "q_finish";
        DevScalars* scp = h.sc;
        const float* rp = q_row_part; const int rows = B;
        fo.run = [scp, rp, rows](hipStream_t s) { hipLaunchKernelGGL(q_finish_kernel, dim3(1), dim3(256), 0, s, scp, rp, rows); };
        h.ops_grads.push_back(fo);
      }
    }
    if (r.q_chain && (!*q_defer || !q_finish))
      return fail(GRL_ERR_INVALID, "internal: the chained Q backward was planned without the fused apply launch that sums its slabs and row sums");
    return GRL_OK;
  }
  // "per_pf": FOUR launches per update inside a multi-update prioritised call.  The TD errors are final when the tower chains end,
  // so the priority write-back and the refresh of the block sums ride on the trunk launch (q_chain.h) and the launch that ends
  // update t -- reduction, clip, Adam -- carries the sampler of update t + 1 (sum-tree walks, importance weights, the rows'
  // gather): nothing it writes is read by that launch, the Philox counter was advanced by update t's loss, and the Adam
  // step size of t + 1 is fixed by its forward launch instead of its sampler (the apply launch of t still reads t's).
  //   first : sampler (all block sums) | forward | towers | trunk + write-back + refresh | apply + sampler(t + 1)
  //   middle:                            forward[tick] | towers | trunk + write-back + refresh | apply + sampler(t + 1)
  //   last  :                            forward[tick] | towers | trunk + write-back + refresh | apply
  void plan_per_pf() {
    if (h.sw.get(Sw::per_pf) && r.q_chain && have_fwd_tick && have_bwd_wb && !h.ops_per_rng_g.empty()) {
      h.per_pf.first = h.ops_per_rng_g;
      for (int v = 0; v < 3; ++v) {
        std::vector<Op>& dst = h.per_pf.part(v);
        for (size_t k = 0; k + 1 < h.ops_grads_apply_per.size(); ++k) {
          const Op& o = h.ops_grads_apply_per[k];
          if (o.tag == "q_fwd") dst.push_back(v == 0 ? o : fwd_tick_op);
          else if (o.tag == "q_bwd") dst.push_back(bwd_wb_op);
          else dst.push_back(o);
        }
        dst.push_back(q_apply(v == 2 ? apply_op(false) : apply_op(false, false, true)));
      }
      // (short_call_graph stays off here and on the SAC sequences that end in the exchange (pf_dp, built at connect): calls of
      //  <= 32 updates go out as first | grouped middles | last.  Turning it on is a speed change that needs a measurement.)
    }
    plan_note("grl plan: per_pf        multi-update prioritised calls, four launches per update (sampler on the apply launch): %s\n", h.per_pf.ok() ? "yes" : "no");
  }
  // "q_pf": uniform replay, calls of several updates on the device RNG -- FOUR launches per update instead of six: the index draw
  // and the gather of update t + 1 (rng_kernel + gather_norm_kernel) ride on the launch that ends update t, whose forward launch
  // is the first reader of the minibatch tensors; the forward launch of t + 1 opens the update (counter += 1, Adam step size).
  //   first : rng | gather | forward | towers | trunk | apply + draw / gather(t + 1)
  //   middle:                forward[counter += 1, tick] | towers | trunk | apply + draw / gather(t + 1)
  //   last  :                forward[counter += 1, tick] | towers | trunk | apply (counter += 1)
  void plan_q_pf() {
    Op fwd_adv = fwd_tick_op;
    QFusedArgs ft = qf;
    ft.tick_sc = h.sc; ft.tick_rng = 1;
    fwd_adv.run = [ft](hipStream_t s) { launch_q_fwd(ft, s); };
    h.q_pf.first = h.ops_rng;
    for (int v = 0; v < 3; ++v) {
      std::vector<Op>& dst = h.q_pf.part(v);
      for (size_t k = 0; k + 1 < h.ops_grads_apply.size(); ++k) {
        const Op& o = h.ops_grads_apply[k];
        if (o.tag == "gather_norm") { if (v == 0) dst.push_back(o); }
        else if (o.tag == "q_fwd") dst.push_back(v == 0 ? o : fwd_adv);
        else dst.push_back(o);
      }
      dst.push_back(q_apply(v == 2 ? apply_op(false) : apply_op(false, false, false, true)));
    }
    h.q_pf.short_call_graph = true;
    plan_note("grl plan: q_pf          multi-update uniform calls, four launches per update (draw + gather on the apply launch)\n");
  }

  // =============================================================== act path: Q-values of n observations
  static Op act_ingest_op(const ActIngestArgs& ia, int elems) {
    Op op; op.tag = "act_ingest";
    op.run = [ia, elems](hipStream_t s) {
      hipLaunchKernelGGL(act_ingest_kernel, dim3((elems + 255) / 256, ia.n), dim3(256), 0, s, ia);
    };
    return op;
  }
  int act_path() {
    Arena& wk = h.wk;
    h.afeat = wk.f32((int64_t)NA * ldf);
    h.q_aout = wk.f32((int64_t)NA * D * nb);
    h.a_eps = wk.f32(NA); h.a_out = h.q_aout;
    alloc_net(aact, NA);
    ActIngestArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.obs = h.stg_obs; ia.n = NA; ia.vec_dim = c.obs_dim; ia.scale_div = 1.f; ia.x = h.afeat; ia.ldx = ldf; ia.d = h.afeat; ia.ldd = ldf;
    h.ops_act.push_back(act_ingest_op(ia, c.obs_dim));
    // entry launch of the GRL_ACT_GREEDY launch list: [observed by grl_observe | handed to grl_act] x [raw | already normalised]
    ActIngestArgs ian = ia;
    ian.normalize = 1; ian.clip_obs = c.clip_obs; ian.mean = h.s_mean; ian.stdv = h.s_std; ian.nan_through = 1;
    for (int v = 0; v < 4; ++v) {
      ActIngestArgs iv = (v & 1) ? ian : ia;
      if (v & 2) iv.obs = h.ob_latest;
      h.ops_act_in[v].push_back(act_ingest_op(iv, c.obs_dim));
    }
    add_forward(h.ops_act, {{&on, &aact, h.afeat}}, NA, "act_q", "act_ln");
    if (r.ln) {
      int n_ln = 0;
      for (auto* ops : {&h.ops_grads, &h.ops_act})
        for (auto& o : *ops) n_ln += (o.tag == "q_ln_fwd" || o.tag == "q_ln_bwd" || o.tag == "act_ln") ? 1 : 0;
      plan_note("grl plan: q layer_norm   per-layer launches + ln_relu_fwd/bwd (%d tensors in %d launches); no chains, no one-launch act\n", ln_tensors, n_ln);
    }
    const float* adv = aact.adv; const float* vv = aact.v; float* qo = h.q_aout; const int rows = NA, Dq = D, nq = nb;
    // the last launch also writes the Q-values to coherent host memory and counts its workgroups there: grl_act polls the
    // counter instead of copying device -> host and synchronising the stream (GRL_TUNE act_poll=0 keeps that)
    if (!h.dry && h.sw.get(Sw::act_poll) != 0 && h.q_act_host.reserve((size_t)NA * D * nb, hipHostMallocCoherent) == hipSuccess) {
      if (h.act_done_host.reserve(16, hipHostMallocCoherent) == hipSuccess) h.act_done_wgs = (unsigned)((rows * Dq + 255) / 256);
      else h.q_act_host.reset();
    }
    float* qh = h.act_done_wgs ? h.q_act_host.get() : nullptr;
    unsigned* dn = h.act_done_wgs ? h.act_done_host.get() : nullptr;
    Op op2; op2.tag = "dueling";
    op2.run = [adv, vv, qo, rows, Dq, nq, qh, dn](hipStream_t s) {
      hipLaunchKernelGGL(dueling_kernel, dim3((rows * Dq + 255) / 256), dim3(256), 0, s, adv, vv, rows, Dq, nq, qo, qh, dn);
    };
    h.ops_act.push_back(op2);
    return h.dry ? GRL_OK : act_greedy(dn);
  }
  // ---- GRL_ACT_GREEDY: the chosen bins instead of the Q-values.  One launch (q_act.h) for the shapes its 64-wide stages
  // cover; every other shape keeps the launch list of the Q-value path and gets the select kernel behind it (GRL_TUNE q_act=0: always)
  int act_greedy(unsigned* dn) {
    const size_t io_floats = (size_t)NA * c.obs_dim + 2 * (size_t)NA * D;
    if (h.q_io_host.reserve(io_floats, hipHostMallocCoherent) != hipSuccess)
      return fail(GRL_ERR_HIP, "no page-locked memory for the act path of the Q handle");
    float* io_obs = h.q_io_host.get(); float* io_explore = io_obs + (size_t)NA * c.obs_dim; float* io_bins = io_explore + (size_t)NA * D;
    for (int i = 0; i < NA * D; ++i) io_explore[i] = -1.f;
    h.q_act_fused = !r.ln && h.sw.get(Sw::q_act) != 0 && qa_shape_ok(c);
    plan_note("grl plan: q_act         epsilon-greedy act: %s\n",
              h.q_act_fused ? "one launch (q_act.h)" : "launch list of the Q-value path + select kernel");
    const int rows = NA, Dq = D, nq = nb;
    if (h.q_act_fused) {
      QActArgs qa;
      memset(&qa, 0, sizeof(qa));
      qa.obs = io_obs; qa.ld_obs = c.obs_dim; qa.obs_dim = c.obs_dim; qa.rows = NA;
      qa.Lc = Lc; qa.D = D; qa.nb = nb;
      for (int k = 0; k < Lc; ++k) qa.trunk[k] = QActLayer{P + on.trunk.w[k], P + on.trunk.b[k], on.trunk.width[k]};
      for (int tw = 0; tw <= D; ++tw) {
        const QStack& T = on.tower[tw];
        QActTower& A = qa.tw[tw];
        A.L = T.L();
        for (int l = 0; l < A.L; ++l) A.lay[l] = QActLayer{P + T.w[l], P + T.b[l], T.width[l]};
        A.ow = P + T.w[A.L]; A.ob = P + T.b[A.L];
      }
      qa.explore = io_explore; qa.bins = io_bins; qa.done = dn;
      h.q_greedy_wgs = dn ? q_act_workgroups(qa) : 0u;
      // [observed: the rows grl_observe left in ob_latest] x [raw: q_act_norm_kernel with the statistics the handle holds]
      for (int v = 0; v < 4; ++v) {
        QActArgs qv = qa;
        if (v & 2) qv.obs = h.ob_latest;
        const QActNorm nm{h.s_mean, h.s_std, (double)c.clip_obs};
        Op og; og.tag = "q_act";
        if (v & 1) og.run = [qv, nm](hipStream_t s) { launch_q_act_norm(qv, nm, s); };
        else og.run = [qv](hipStream_t s) { launch_q_act(qv, s); };
        h.ops_act_greedy[v].push_back(og);
      }
    } else {
      // (dueling_kernel counts its workgroups too: both counts are expected)
      h.q_greedy_wgs = dn ? h.act_done_wgs + (unsigned)((rows * Dq + 255) / 256) : 0u;
      float* qo = h.q_aout;
      Op og; og.tag = "q_select";
      og.run = [qo, rows, Dq, nq, io_explore, io_bins, dn](hipStream_t s) { launch_q_select(qo, rows, Dq, nq, io_explore, io_bins, dn, s); };
      for (int v = 0; v < 4; ++v) {     // the launch list of the Q-value path behind the entry launch of the variant
        h.ops_act_greedy[v] = h.ops_act_in[v];
        h.ops_act_greedy[v].insert(h.ops_act_greedy[v].end(), h.ops_act.begin() + 1, h.ops_act.end());
        h.ops_act_greedy[v].push_back(og);
      }
    }
    return GRL_OK;
  }

  void debug_views() {
    auto& dbg = h.dbg;
    const int A = h.A;
    dbg["feat_pi"] = {h.feat[0], (int64_t)B * ldf};
    dbg["feat_tgt"] = {h.feat[2], (int64_t)B * ldf};
    dbg["adv"] = {net[0].adv, (int64_t)B * D * nb};
    dbg["v"] = {net[0].v, B};
    dbg["adv_next"] = {net[1].adv, (int64_t)B * D * nb};
    dbg["adv_tgt"] = {net[2].adv, (int64_t)B * D * nb};
    dbg["v_tgt"] = {net[2].v, B};
    dbg["td"] = {h.q_td, (int64_t)B * D};
    dbg["idx_raw"] = {(const float*)h.idx_buf, (int64_t)2 * B};     // int64 viewed as float pairs
    dbg["weights"] = {h.eps_buf, B};
    if (h.per_on) dbg["per_p"] = {(const float*)h.per.p, 2 * (int64_t)c.replay_capacity};   // float64 leaves, handed out as raw 4-byte words
    dbg["priority"] = {h.q_prio, B};
    dbg["rew"] = {h.rew, B}; dbg["done"] = {h.done, B}; dbg["act"] = {h.act, (int64_t)B * A};
    dbg["grads"] = {h.grads, h.n_train};
    dbg["adam_m"] = {h.adam_m, h.n_train};
    dbg["adam_v"] = {h.adam_v, h.n_train};
  }
};
}  // namespace

int grl_ctx::plan_q() {
  QPlanner p(*this);
  p.layout();
  p.decide_routes();
  p.arenas();
  p.sampler();
  p.draw_and_gather();
  if (int e = p.forward()) return e;
  p.loss();
  p.backward();            // chained (loss + weight gradients inside), fused or per layer; then the weight gradients
  p.reduction();
  p.apply();               // clip + Adam as launches of their own: plain or tiled (wide)
  if (int e = p.fused_apply()) return e;      // ... and as one launch with the reduction; the "per_pf" / "q_pf" call plans
  if (int e = p.act_path()) return e;
  p.debug_views();
  return GRL_OK;
}
