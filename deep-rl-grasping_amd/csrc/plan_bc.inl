// plan_bc.inl: launch plan of behaviour-cloning pretraining on a SAC handle (grl_ctx::plan_bc; the grl_bc_* calls of capi.inl) --
// part of engine.hip (included there, same translation unit: the plans are methods of grl_ctx).
//
// The plan covers NETWORK 0 (model/pi) only, at its own row count bc_batch <= cfg.batch_size, and lives entirely in the session
// buffer the caller hands to grl_bc_begin: the session's words (BcDev), the optimiser's words (a DevScalars of its own) and
// moments, the loss slots, the minibatch's activations and gradients, the addressing tables and the slabs.  The record is a
// Session (engine.hip): grl_ctx::plan_session lends the handle's builders to it, so nothing of the SAC plan is touched -- its work
// arena, launch lists, tables and debug views stay as grl_create left them -- and the body of an update is built from the SAC
// plan's own problem builders and launches (conv_stack_fwd or a launch per layer, fc_fwd, the dense forward / backward-data
// launches, exact-tap convolution backward, weight gradients into slabs, the ordered slab reduction, adam_op over the trained
// range): no kernel of those changes, and no sum is formed by atomics.  New are the gather from the caller's table, the loss
// launch and the closing launch (bc_kernels.h).
//
// An update (MLP, two hidden layers: 11 launches; depth CNN with the forward stack: 18):
//   bc_gather | [conv_stack_fwd | conv1..3_fwd] fc_fwd | heads_fwd x (L + 1) | bc_loss | bc_close |
//   heads_bwd x L | [heads_dfeat fc_bwd conv3_bwd conv2_bwd] | wgrad_dense [wgrad_small] [wgrad_conv] | reduce_slabs | bc_adam
// An evaluation batch is the list up to bc_close (bc_loss without d mu, bc_close without the optimiser's tick).

struct grl::BcPlan : Session {
  grl_bc_config cfg{};
  BcDev* dev = nullptr;
  float *m = nullptr, *v = nullptr, *losses = nullptr;
  int64_t n_bc = 0;                     // trained range [0, n_bc) of the parameter block
  std::vector<Op> ops_train, ops_eval;
  BcPlan() : Session("bc_") {}
  int plan(grl_ctx& h) override { return h.plan_bc(*this); }
};
inline grl::BcPlan* grl_ctx::bc() const { return cfg.algo == GRL_ALGO_SAC ? static_cast<BcPlan*>(session.get()) : nullptr; }

namespace {

struct BcPlanner {
  grl_ctx& h;
  BcPlan& p;
  const grl_config& c;
  const int Bb;                         // bc_batch
  const bool cnn;
  const int A, L, F, Fc, ldf, hw, C_img, img_elems;
  const SacGeom& geo;                   // the handle's image geometry (SacPlanner::shapes)
  const int* const hid;
  Arena& wk;                            // the handle's work arena, standing in for the session buffer while the plan is built
  const float* const P;
  int nd = 0;
  // minibatch tensors
  float *x_obs = nullptr, *feat = nullptr, *a1 = nullptr, *a2 = nullptr, *a3 = nullptr;
  float *act = nullptr, *det = nullptr, *dmu = nullptr, *row_loss = nullptr;
  float *dfeat = nullptr, *g3 = nullptr, *g2 = nullptr, *g1 = nullptr;
  const float *d_low = nullptr, *d_half = nullptr;
  HeadAct hPI{};
  HeadGrad gPI{};
  int ld_dm = 0;
  const int ld1 = 64;                   // pixel stride of a1 / g1: the SAC plan's layout (columns 32..63 idle here)
  ConvGeom cg[3];
  ConvFwdTabs ft[3];
  bool conv_stack = false;
  std::vector<Op> gather_ops, fwd, loss_train, loss_eval, bwd, wgrads, tail;

  BcPlanner(grl_ctx& ctx, BcPlan& plan)
      : h(ctx), p(plan), c(ctx.cfg), Bb(plan.cfg.batch), cnn(ctx.cnn), A(ctx.A), L(ctx.L), F(ctx.F), Fc(ctx.Fc), ldf(ctx.ldf), hw(ctx.hw),
        C_img(ctx.C_img), img_elems(ctx.img_elems), geo(ctx.geo), hid(ctx.hid), wk(ctx.wk), P(ctx.params) {
    nd = cnn && c.extractor == GRL_EXTRACTOR_AUGMENTED ? c.n_direct : 0;
  }

  // the session's state: its words, the optimiser's words and moments over the trained range, loss slots, the action space's tables
  void state() {
    p.dev = (BcDev*)wk.take(sizeof(BcDev));
    p.sc = (DevScalars*)wk.take(sizeof(DevScalars));
    p.n_bc = h.m_pi.ow[1];              // model/pi is laid out first and its log-std head last: [0, dense_1/kernel)
    p.m = wk.f32(p.n_bc);
    p.v = wk.f32(p.n_bc);
    p.losses = wk.f32(GRL_BC_MAX_UPDATES);
    std::vector<float> half(A);
    for (int j = 0; j < A; ++j) half[j] = 0.5f * (p.high[j] - p.low[j]);
    d_low = h.upload_vec(wk, p.low);
    d_half = h.upload_vec(wk, half);
  }

  void workspace() {
    feat = wk.f32((int64_t)Bb * ldf);   // (row padding [F, ldf) stays zero: grl_bc_begin clears the whole buffer)
    if (cnn) {
      x_obs = wk.f32((int64_t)Bb * img_elems);
      a1 = wk.f32((int64_t)Bb * geo.p1 * ld1);
      a2 = wk.f32((int64_t)Bb * geo.p2 * 64);
      a3 = wk.f32((int64_t)Bb * geo.p3 * 64);
      dfeat = wk.f32((int64_t)Bb * ldf);
      g3 = wk.f32((int64_t)Bb * geo.p3 * 64);
      g2 = wk.f32((int64_t)Bb * geo.p2 * 64);
      g1 = wk.f32((int64_t)Bb * geo.p1 * ld1);    // (pixels that no window of conv2 covers -- 64x64: row / column 14 -- stay zero)
    }
    act = wk.f32((int64_t)Bb * A);
    det = wk.f32((int64_t)Bb * A);
    row_loss = wk.f32(Bb);
    h.alloc_head(hPI, Bb, 1, A);
    h.alloc_hgrad(gPI, Bb);
    ld_dm = (int)rup(A, 4);             // padded so that the weight-gradient launch can fetch it 16 bytes at a time
    dmu = wk.f32((int64_t)Bb * ld_dm);
  }

  void gather() {
    BcGatherArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.dev = p.dev; ga.batch = Bb; ga.hw = hw * hw; ga.c_obs = c.obs_channels; ga.c_img = C_img; ga.n_direct = nd;
    ga.vec_dim = cnn ? 0 : c.obs_dim; ga.scale_div = cnn ? 255.f : 1.f;
    ga.x = cnn ? x_obs : feat; ga.ldx = cnn ? img_elems : ldf; ga.d = feat + 512; ga.ldd = ldf;
    ga.A = A; ga.act_out = act;
    const int elems = cnn ? img_elems : c.obs_dim;
    Op op; op.tag = "bc_gather";
    op.run = [ga, elems](hipStream_t s) { hipLaunchKernelGGL(bc_gather_kernel, dim3((elems + 255) / 256, ga.batch), dim3(256), 0, s, ga); };
    gather_ops.push_back(op);
  }

  // observations -> feat through pi's extractor: the forward stack where the SAC plan would use it, else a launch per layer
  void forward() {
    if (!cnn) return;
    for (int l = 0; l < 3; ++l) {
      cg[l] = cnn_geom(l, C_img, hw);
      if (l == 0) cg[l].ldy = ld1;
      if (l == 1) cg[l].ldx = ld1;
      ft[l] = h.conv_fwd_tabs(cg[l], Bb);
    }
    conv_stack = conv_stack_ok(C_img) && hw == 64 && h.sw.get(Sw::conv_stack) != 0 && !h.sw.get(Sw::GRL_NO_V2);
    float* const io[4] = {x_obs, a1, a2, a3};
    if (conv_stack) {
      ConvStackArgs ca;
      memset(&ca, 0, sizeof(ca));
      ConvStackNet& cn = ca.nets[0];
      cn.x = x_obs;
      for (int l = 0; l < 3; ++l) { cn.w[l] = P + h.ex[0].w[l]; cn.b[l] = P + h.ex[0].b[l]; }
      cn.a1 = a1; cn.a2 = a2; cn.a3 = a3; cn.ld1 = ld1;
      ca.B = Bb; ca.n_nets = 1;
      const int Ci = C_img;
      Op op; op.tag = "conv_stack_fwd";
      op.flops = op.flops_exec = 2.0 * Bb * ((double)geo.p1 * 32 * 64 * Ci + (double)geo.p2 * 64 * 512 + (double)geo.p3 * 64 * 576);
      op.run = [ca, Ci](hipStream_t s) { launch_conv_stack_fwd(Ci, ca, s); };
      fwd.push_back(op);
    } else {
      const char* tags[3] = {"conv1_fwd", "conv2_fwd", "conv3_fwd"};
      for (int l = 0; l < 3; ++l)
        h.add_launch(fwd, tags[l], 0, {h.conv_fwd(io[l], ft[l], cg[l], P + h.ex[0].w[l], P + h.ex[0].b[l], io[l + 1], ACT_RELU, 0.f)});
    }
    h.add_launch(fwd, "fc_fwd", 0, {h.dense_fwd(a3, geo.K, geo.K, nullptr, 0, 0, Bb, P + h.ex[0].fw, 512, P + h.ex[0].fb, feat, ldf, ACT_RELU)});
  }

  // per-layer route of the head: dense forward launches, the loss launch, the closing launch
  void head_forward() {
    for (int l = 0; l < L; ++l) h.add_launch(fwd, "heads_fwd", 0, {h.head_layer(h.m_pi, P, hPI, l, feat, ldf, F, nullptr, 0, 0, Bb)});
    h.add_launch(fwd, "heads_fwd", 0, {h.head_out(h.m_pi, P, hPI, 0, Bb)});
    for (int train = 0; train < 2; ++train) {
      std::vector<Op>& to = train ? loss_train : loss_eval;
      BcLossArgs la;
      memset(&la, 0, sizeof(la));
      la.dev = p.dev; la.batch = Bb; la.A = A; la.mu = hPI.out[0]; la.ld_mu = A; la.act = act; la.low = d_low; la.half = d_half;
      la.det = det; la.dmu = train ? dmu : nullptr; la.ld_dm = ld_dm; la.row_loss = row_loss;
      Op op; op.tag = "bc_loss";
      op.run = [la](hipStream_t s) { hipLaunchKernelGGL(bc_loss_kernel, dim3((la.batch + BC_LOSS_ROWS - 1) / BC_LOSS_ROWS), dim3(BC_LOSS_ROWS), 0, s, la); };
      to.push_back(op);
      BcCloseArgs ca{p.dev, p.sc, Bb, A, row_loss, p.losses, train};
      Op oc; oc.tag = "bc_close";
      oc.run = [ca](hipStream_t s) { hipLaunchKernelGGL(bc_close_kernel, dim3(1), dim3(64), 0, s, ca); };
      to.push_back(oc);
    }
  }

  // d mu -> the gradients of every hidden level (g[l]: w.r.t. the pre-activation of layer l), d feat and down through the CNN
  void backward() {
    h.add_launch(bwd, "heads_bwd", 1, {h.dense_bwd({{dmu, ld_dm, A, P + h.m_pi.ow[0]}}, Bb, 0, hid[L - 1], gPI.g[L - 1], hid[L - 1], hPI.z[L - 1])});
    for (int l = L - 1; l >= 1; --l)
      h.add_launch(bwd, "heads_bwd", 1, {h.dense_bwd({{gPI.g[l], hid[l], hid[l], P + h.m_pi.w[l]}}, Bb, 0, hid[l - 1], gPI.g[l - 1], hid[l - 1], hPI.z[l - 1])});
    if (!cnn) return;
    h.add_launch(bwd, "heads_dfeat", 1, {h.dense_bwd({{gPI.g[0], hid[0], hid[0], P + h.m_pi.w[0]}}, Bb, 0, Fc, dfeat, ldf, feat)});
    h.add_launch(bwd, "fc_bwd", 1, {h.dense_bwd({{dfeat, ldf, 512, P + h.ex[0].fw}}, Bb, 0, geo.K, g3, geo.K, a3)});
    std::vector<ConvBwdClass> bc3 = h.conv_bwd_tabs_exact(cg[2], Bb, nullptr);
    std::vector<ConvBwdClass> bc2 = h.conv_bwd_tabs_exact(cg[1], Bb, nullptr);
    std::vector<IgemmProb> p3, p2;
    for (auto& cl : bc3) p3.push_back(h.conv_bwd(g3, cl, cg[2], P + h.ex[0].w[2], g2, a2));
    for (auto& cl : bc2) p2.push_back(h.conv_bwd(g2, cl, cg[1], P + h.ex[0].w[1], g1, a1));
    h.add_launch(bwd, "conv3_bwd", 1, p3);
    h.add_launch(bwd, "conv2_bwd", 1, p2);
  }

  // reduction split of a convolution weight gradient over M output pixels: chunks of about 24 slabs of 32 rows
  static int conv_split(int M) { return std::max(1, (M + 767) / 768); }

  void weight_gradients() {
    std::vector<IgemmProb> wg, wgc;
    auto slab = [&](IgemmProb& q) { q.c = wk.f32(q.slab_stride * q.split); };
    if (cnn) {
      const float* const in[3] = {x_obs, a1, a2};
      float* const gy[3] = {g1, g2, g3};
      for (int l = 2; l >= 0; --l) {
        IgemmProb q = h.conv_wgrad(in[l], ft[l], cg[l], gy[l], nullptr, conv_split(ft[l].M));
        slab(q);
        h.add_wgrad(wgc, q, h.ex[0].w[l], 0, cg[l].K(), h.ex[0].b[l]);
      }
      IgemmProb q = h.dense_wgrad(a3, geo.K, geo.K, true, dfeat, ldf, 512, Bb, nullptr, 1);
      slab(q);
      h.add_wgrad(wg, q, h.ex[0].fw, 0, geo.K, h.ex[0].fb);
    }
    for (int l = 0; l < L; ++l) {
      IgemmProb q = l == 0 ? h.dense_wgrad(feat, ldf, F, true, gPI.g[0], hid[0], hid[0], Bb, nullptr, 1, (int)rup(F, 4))
                           : h.dense_wgrad(hPI.z[l - 1], hid[l - 1], hid[l - 1], true, gPI.g[l], hid[l], hid[l], Bb, nullptr, 1);
      slab(q);
      h.add_wgrad(wg, q, h.m_pi.w[l], 0, l == 0 ? F : hid[l - 1], h.m_pi.b[l]);
    }
    {
      IgemmProb q = h.dense_wgrad(hPI.z[L - 1], hid[L - 1], hid[L - 1], true, dmu, ld_dm, A, Bb, nullptr, 1);
      slab(q);
      h.add_wgrad(wg, q, h.m_pi.ow[0], 0, hid[L - 1], h.m_pi.ob[0]);
    }
    // the vectorised kernel takes what its addressing allows; the rest goes to igemm_kernel (as in the SAC plan)
    std::vector<IgemmProb> wg_vec, wg_rest;
    for (auto& q : wg) (h.v2_prob_ok(q, 2) && (q.K % 4) == 0 ? wg_vec : wg_rest).push_back(q);
    h.add_launch(wgrads, "wgrad_dense", 2, wg_vec);
    h.add_launch(wgrads, "wgrad_small", 2, wg_rest);
    h.add_launch(wgrads, "wgrad_conv", 2, wgc);
  }

  // slabs -> the gradient bucket (sums in slab order), then Adam over the trained range
  void reduce_and_apply() {
    tail.push_back(h.close_reduction().op);            // (into the session buffer: it stands in for the work arena here)
    AdamArgs aa;
    memset(&aa, 0, sizeof(aa));
    aa.params = h.params; aa.grads = h.grads; aa.m = p.m; aa.v = p.v; aa.n_train = p.n_bc; aa.sc = p.sc;
    aa.grad_scale = 1.f; aa.eps = p.cfg.adam_eps; aa.target = h.params;
    tail.push_back(grl_ctx::adam_op("bc_adam", aa));
  }

  void assemble() {
    for (const std::vector<Op>* part : {&gather_ops, &fwd, &loss_train, &bwd, &wgrads, &tail}) p.ops_train.insert(p.ops_train.end(), part->begin(), part->end());
    for (const std::vector<Op>* part : {&gather_ops, &fwd, &loss_eval}) p.ops_eval.insert(p.ops_eval.end(), part->begin(), part->end());
    plan_note("grl plan: bc  per-layer: the only route of this plan  bc_batch %d  launches %zu (evaluation %zu)%s\n", Bb, p.ops_train.size(),
              p.ops_eval.size(), cnn ? (conv_stack ? "  forward stack" : "  convolutions per layer") : "");
    plan_seq("ops_bc", p.ops_train);
    plan_seq("ops_bc_eval", p.ops_eval);
  }

  void debug_views() {
    auto view = [&](const char* name, const float* ptr, int64_t n) { h.dbg[name] = {ptr, n}; p.dbg_names.push_back(name); };
    view("bc_obs", cnn ? x_obs : feat, cnn ? (int64_t)Bb * img_elems : (int64_t)Bb * ldf);
    view("bc_feat", feat, (int64_t)Bb * ldf);
    view("bc_act", act, (int64_t)Bb * A);
    view("bc_mu", hPI.out[0], (int64_t)Bb * A);
    view("bc_det", det, (int64_t)Bb * A);
    view("bc_dmu", dmu, (int64_t)Bb * ld_dm);
    view("bc_loss", p.losses, GRL_BC_MAX_UPDATES);
    view("bc_adam_m", p.m, p.n_bc);
    view("bc_adam_v", p.v, p.n_bc);
  }
};

}  // namespace

int grl_ctx::plan_bc(BcPlan& p) {
  return plan_session(p, [&] {
    BcPlanner b(*this, p);
    b.state();
    b.workspace();
    b.gather();
    b.forward();
    b.head_forward();
    b.backward();
    b.weight_gradients();
    b.reduce_and_apply();
    b.assemble();
    if (!dry) b.debug_views();
  });
}
