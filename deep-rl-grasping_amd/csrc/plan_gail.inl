// plan_gail.inl: launch plan of a GAIL session on a TRPO handle (grl_ctx::plan_gail; the grl_gail_* calls of capi.inl) -- part of
// engine.hip (included there).  stable-baselines 2.10.1 gail/adversary.py TransitionClassifier on Box actions: the discriminator
//   D(obs, act) = W3 tanh(W2 tanh(W1 [ (obs - mean) / std | act ] + b1) + b2) + b3
// with the running statistics of common/mpi_running_mean_std.py (epsilon 1e-2) and an Adam of its own.
//
// The record is a Session (engine.hip; grl_ctx::plan_session lends the handle's builders to it, as for behaviour cloning).
// Everything of the session lives in the buffer the caller hands to grl_gail_begin: the device words, the optimiser's words and
// moments, the float64 statistics and their float32 mean / std, the six parameter tensors and their gradient bucket, the loss
// slots, the inputs, activations and gradients of both passes, the launch tables and the slabs.  Nothing of the TRPO plan is
// touched -- its arenas, launch lists, tables and debug views stay as grl_trpo_create left them; the reward pass rewrites the
// rollout's reward array, which is what it is for.  The dense products are dense_fwd / dense_bwd / add_stack_wgrads, the slab
// reduction close_reduction, Adam adam_op, tanh the launches of ppo_kernels.h: no kernel of those changes, no sum is formed by
// atomics.  New are the input launch, the loss launch and the reward launch (gail_kernels.h).
//
//   reward pass (one per rollout, T rows)   gail_input (stored mean / std, clipped actions) | FWD | gail_reward         (7 launches)
//   update (2 batch rows)                   gail_input (gather, statistics, Adam tick) | FWD | gail_loss | BWD | adam  (14 launches)
//     FWD   per level: dense + tanh_fwd (an input beyond 2048 values: the first product split over K, tanh_fwd adds the parts in
//           index order); the output launch                                                                            (5)
//     BWD   per level: backward-data + tanh_bwd; weight gradients; reduce_slabs                                        (6)

struct grl::GailPlan : Session {
  grl_gail_config cfg{};
  GailDev* dev = nullptr;
  double *sum = nullptr, *sumsq = nullptr, *count = nullptr;
  float *mean = nullptr, *sd = nullptr;
  float *params = nullptr, *m = nullptr, *v = nullptr, *grads = nullptr, *diag = nullptr, *true_rew = nullptr;
  int64_t n_p = 0;
  int od = 0, nblk = 0;
  struct Tensor { const char* name; int64_t off, numel; int rows, cols; } tensors[6];
  std::vector<Op> ops_rewards, ops_update;
  std::vector<int> last_ne;             // expert row counts of the last call's updates
  GailPlan() : Session("gail_") {}
  int plan(grl_ctx& h) override { return h.plan_gail(*this); }
};
inline grl::GailPlan* grl_ctx::gail() const { return cfg.algo == GRL_ALGO_TRPO ? static_cast<GailPlan*>(session.get()) : nullptr; }

namespace {

struct GailPlanner {
  grl_ctx& h;
  GailPlan& p;
  const int T, Bu, H, A, od, ldo, K, ldx;      // rollout rows; rows of an update (2 batch); hidden width; input width and its padded stride
  Arena& wk;                                   // the handle's work arena, standing in for the session buffer while the plan is built
  int64_t w[3], b[3];
  int width[2];
  const float *d_low = nullptr, *d_high = nullptr;
  struct Acts { float* x; float* z[2]; float* out; int ld_out; } act_r, act_u, g_u;
  std::string route;

  GailPlanner(grl_ctx& ctx, GailPlan& plan)
      : h(ctx), p(plan), T(ctx.tcfg.n_steps), Bu(2 * plan.cfg.batch), H(plan.cfg.hidden), A(ctx.cfg.act_dim), od(ctx.cfg.obs_dim),
        ldo(ctx.ppo_ldo), K(ctx.cfg.obs_dim + ctx.cfg.act_dim), ldx((int)rup(ctx.cfg.obs_dim + ctx.cfg.act_dim, 4)), wk(ctx.wk) {
    width[0] = width[1] = H;
  }

  // TF creation order of the adversary scope; every tensor starts on a 16-byte boundary of the block
  void layout() {
    static const char* nm[6] = {"adversary/fully_connected/weights:0", "adversary/fully_connected/biases:0",
                                "adversary/fully_connected_1/weights:0", "adversary/fully_connected_1/biases:0",
                                "adversary/fully_connected_2/weights:0", "adversary/fully_connected_2/biases:0"};
    const int in[3] = {K, H, H}, out[3] = {H, H, 1};
    int64_t off = 0;
    for (int l = 0; l < 3; ++l) {
      w[l] = off; p.tensors[2 * l] = {nm[2 * l], off, (int64_t)in[l] * out[l], in[l], out[l]};
      off = rup(off + (int64_t)in[l] * out[l], 4);
      b[l] = off; p.tensors[2 * l + 1] = {nm[2 * l + 1], off, out[l], out[l], 1};
      off = rup(off + out[l], 4);
    }
    p.n_p = off;
    p.od = od;
  }

  void state() {
    p.dev = (GailDev*)wk.take(sizeof(GailDev));
    p.sc = (DevScalars*)wk.take(sizeof(DevScalars));
    p.sum = (double*)wk.take((size_t)od * 8); p.sumsq = (double*)wk.take((size_t)od * 8); p.count = (double*)wk.take((size_t)od * 8);
    p.mean = wk.f32(od); p.sd = wk.f32(od);
    p.params = wk.f32(p.n_p); p.m = wk.f32(p.n_p); p.v = wk.f32(p.n_p); p.grads = wk.f32(p.n_p);
    p.nblk = gail_loss_blocks(p.cfg.batch);
    p.diag = wk.f32((int64_t)GRL_GAIL_MAX_UPDATES * p.nblk * GAIL_DIAG);
    p.true_rew = wk.f32(T);
    d_low = h.upload_vec(wk, p.low);
    d_high = h.upload_vec(wk, p.high);
  }

  // (row padding [K, ldx) of the inputs and [1, 4) of the output gradient stays zero: grl_gail_begin clears the whole buffer)
  void alloc(Acts& a, int rows, bool input, int ld_out) {
    a.x = input ? wk.f32((int64_t)rows * ldx) : nullptr;
    for (int l = 0; l < 2; ++l) a.z[l] = wk.f32((int64_t)rows * H);
    a.out = wk.f32((int64_t)rows * ld_out); a.ld_out = ld_out;
  }
  void workspace() {
    alloc(act_r, T, true, 1);
    alloc(act_u, Bu, true, 1);
    alloc(g_u, Bu, false, 4);
  }

  void input(std::vector<Op>& ops, const Acts& a, bool update) {
    GailInputArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.dev = p.dev; ia.sc = p.sc; ia.r_obs = h.pr_obs; ia.ldo = ldo; ia.r_act = h.pr_act;
    ia.sum = p.sum; ia.sumsq = p.sumsq; ia.count = p.count; ia.mean = p.mean; ia.sd = p.sd; ia.low = d_low; ia.high = d_high;
    ia.x = a.x; ia.ldx = ldx; ia.obs_dim = od; ia.A = A; ia.n_gen = update ? p.cfg.batch : T; ia.update = update ? 1 : 0;
    Op op; op.tag = "gail_input";
    op.run = [ia](hipStream_t s) { launch_gail_input(ia, s); };
    ops.push_back(op);
  }

  // the three layers over `rows` rows of a.x, as PpoPlanner::forward runs a tower
  void forward(std::vector<Op>& ops, const Acts& a, int rows, const char* tag) {
    const float* P = p.params;
    const std::string t(tag);
    for (int l = 0; l < 2; ++l) {
      const float* in = l == 0 ? a.x : a.z[0];
      IgemmProb q = h.dense_fwd(in, l == 0 ? ldx : H, l == 0 ? K : H, nullptr, 0, 0, rows, P + w[l], H, P + b[l], a.z[l], H, ACT_NONE);
      TanhDesc d;
      memset(&d, 0, sizeof(d));
      d.z = a.z[l]; d.H = H;
      if (l == 0) {
        if (K > PPO_ACT_MAX_IN) {      // a wide first layer: the reduction is cut until the launch has at least 64 tiles
          const int base = ((rows + 63) / 64) * ((H + 63) / 64);
          h.set_split(q, (64 + base - 1) / base);
          if (q.split > 1) {
            float* parts = wk.f32((int64_t)rows * H * q.split);
            q.c = parts; q.bias = nullptr;
            d.parts = parts; d.bias = P + b[0]; d.part_stride = q.slab_stride; d.n_parts = q.split;
          }
        }
        route = q.split > 1 ? "split " + std::to_string(q.split) : "whole";
      }
      h.add_launch(ops, t + "_l" + std::to_string(l), 0, {q});
      add_tanh_op(h, ops, "gail_tanh_fwd", false, {d}, rows);
    }
    h.add_launch(ops, t + "_out", 0, {h.dense_fwd(a.z[1], H, H, nullptr, 0, 0, rows, P + w[2], 1, P + b[2], a.out, a.ld_out, ACT_NONE)});
  }

  void rewards() {
    std::vector<Op>& ops = p.ops_rewards;
    input(ops, act_r, false);
    forward(ops, act_r, T, "gail_rew");
    GailRewardArgs ra = {act_r.out, h.pr_rew, p.true_rew, T};
    Op op; op.tag = "gail_reward";
    op.run = [ra](hipStream_t s) { launch_gail_reward(ra, s); };
    ops.push_back(op);
    plan_note("grl plan: gail rewards  %d launches over %d rows: input %d (stride %d), hidden %d, first layer %s\n", (int)ops.size(), T, K, ldx, H,
              route.c_str());
  }

  void update() {
    std::vector<Op>& ops = p.ops_update;
    const float* P = p.params;
    input(ops, act_u, true);
    forward(ops, act_u, Bu, "gail_fwd");
    {
      GailLossArgs la;
      memset(&la, 0, sizeof(la));
      la.dev = p.dev; la.logits = act_u.out; la.dlogits = g_u.out; la.ld_dl = g_u.ld_out; la.diag = p.diag; la.batch = p.cfg.batch;
      la.entcoeff = p.cfg.entcoeff;
      Op op; op.tag = "gail_loss";
      op.run = [la](hipStream_t s) { launch_gail_loss(la, s); };
      ops.push_back(op);
    }
    for (int l = 1; l >= 0; --l) {
      const grl_ctx::BwdPart above = l == 1 ? grl_ctx::BwdPart{g_u.out, g_u.ld_out, 1, P + w[2]} : grl_ctx::BwdPart{g_u.z[1], H, H, P + w[1]};
      h.add_launch(ops, "gail_bwd", 1, {h.dense_bwd({above}, Bu, 0, H, g_u.z[l], H, nullptr)});
      TanhDesc d;
      memset(&d, 0, sizeof(d));
      d.z = act_u.z[l]; d.dz = g_u.z[l]; d.H = H;
      add_tanh_op(h, ops, "gail_tanh_bwd", true, {d}, Bu);
    }
    h.reduces.clear();
    std::vector<IgemmProb> wg;
    h.add_stack_wgrads(wg, act_u.x, ldx, K, act_u.z, g_u.z, width, 2, g_u.out, g_u.ld_out, 1, w, b, Bu, p.grads);
    h.add_launch(ops, "gail_wgrad", 2, wg);
    ops.push_back(h.close_reduction().op);
    AdamArgs aa;
    memset(&aa, 0, sizeof(aa));
    aa.params = p.params; aa.grads = p.grads; aa.m = p.m; aa.v = p.v; aa.n_train = p.n_p; aa.sc = p.sc;
    aa.grad_scale = 1.f; aa.eps = p.cfg.adam_eps; aa.target = p.params;
    ops.push_back(grl_ctx::adam_op("gail_adam", aa));
    plan_note("grl plan: gail update   %d launches over %d + %d rows: input %d (stride %d), hidden %d, first layer %s\n", (int)ops.size(),
              p.cfg.batch, p.cfg.batch, K, ldx, H, route.c_str());
  }

  void debug_views() {
    auto view = [&](const char* name, const float* ptr, int64_t n) { h.dbg[name] = {ptr, n}; p.dbg_names.push_back(name); };
    view("gail_params", p.params, p.n_p);
    view("gail_adam_m", p.m, p.n_p);
    view("gail_adam_v", p.v, p.n_p);
    view("gail_grads", p.grads, p.n_p);
    view("gail_x", act_u.x, (int64_t)Bu * ldx);
    view("gail_logits", act_u.out, Bu);
    view("gail_dlogits", g_u.out, (int64_t)Bu * 4);
    view("gail_rew_x", act_r.x, (int64_t)T * ldx);
    view("gail_rew_logits", act_r.out, T);
    view("gail_true_rew", p.true_rew, T);
  }
};

}  // namespace

int grl_ctx::plan_gail(GailPlan& p) {
  return plan_session(p, [&] {
    GailPlanner g(*this, p);
    g.layout();
    g.state();
    g.workspace();
    g.rewards();
    g.update();
    if (!dry) g.debug_views();
  });
}
