// plan_td3.inl: launch plan of stable-baselines 2.10.1 TD3 with MlpPolicy (td3/td3.py, td3/policies.py) -- part of engine.hip
// (included there).  Kernels of its own: td3_kernels.h; the replay ring, the minibatch gather with sample-time VecNormalize and the
// statistics are a SAC handle's (plan_sac.inl, MLP extractor); the dense products are dense_fwd / dense_bwd / add_stack_wgrads, the
// networks of a layer level sharing a launch as heads_per_layer groups them; the slab reduction is reduce_slabs_kernel and the two
// Adams are adam_polyak_kernel over a range each, with the optimiser words of its own (DevScalars: `sc` the critics', `sc2` the
// policy's).  One lane, no forks.
//
//   inputs       the critics read ONE row buffer [obs | action | zero padding] of stride ldq = rup(obs_dim + act_dim, 4): xs for
//                (s, a), xp for (s, pi(s)), xn for (s', a').  The gather writes the observations and the replayed action into their
//                columns, td3_smooth / td3_pi the computed actions into theirs; the policies read the observation columns of the
//                same rows.  Every operand of a dense launch is a single part, so the launches stay on the vectorised GEMM.
//   critic-only  gather | per level: (pi_target(s'), q1(s, a), q2(s, a)) + outputs | td3_smooth | per level: (q1_target, q2_target)
//                (s', a') + outputs | td3_loss | backward-data of q1, q2 per level | weight gradients | reduce_slabs | Adam (critics)
//   policy       the same with pi(s) in the first group, td3_pi, q1(s, pi(s)) in the second group and in the backward levels, then
//                d a = backward-data of q1's first layer over the action columns | td3_pi backward | backward-data of pi | weight
//                gradients of q1, q2, pi (q1's from the pi path are never formed) | reduce_slabs | Adam + Polyak (critics) |
//                Adam + Polyak (policy)
// What a critic-only update leaves in the policy's slots of the gradient bucket: what the last policy update summed there (zeros
// before the first) -- its reduction holds no descriptor for them and its Adam launch covers the critics' range alone.
// Each of the two lists exists four times: [replay indices handed over | drawn] x [normals handed over | drawn]; they differ in
// the gather, the smoothing and the loss launch (which advances the Philox counter when something was drawn).
namespace {

struct Td3Planner {
  grl_ctx& h;
  const grl_config& c;
  const grl_td3_config& tc;
  int &A, &L, &B, &NA, &F, &ldf;
  int* const hid;
  Arena& wk;
  int ldq = 0, Ap = 0, nblk = 0;
  int64_t cap = 0;
  const float* P = nullptr;
  MlpP tPI, tQ1, tQ2;                              // the target copies (h.m_pi, h.m_qf1, h.m_qf2: the online networks)
  float *xs = nullptr, *xp = nullptr, *xn = nullptr;
  HeadAct hPI{}, hPIT{}, hQ1{}, hQ2{}, hQ1T{}, hQ2T{}, hQ1PI{};
  HeadGrad gQ1{}, gQ2{}, gQ1PI{}, gPI{};
  float *qbuf = nullptr, *backup = nullptr, *noise = nullptr, *a_next = nullptr, *pi_a = nullptr, *da = nullptr, *dpre = nullptr;
  float *d_q1 = nullptr, *d_q2 = nullptr, *d_q1pi = nullptr;
  GatherArgs ga0{};
  int gx = 0;
  double gather_bytes = 0;

  explicit Td3Planner(grl_ctx& ctx)
      : h(ctx), c(ctx.cfg), tc(ctx.td3cfg), A(ctx.A), L(ctx.L), B(ctx.B), NA(ctx.NA), F(ctx.F), ldf(ctx.ldf), hid(ctx.hid), wk(ctx.wk) {}

  // ---------------- shapes + layout: TF creation order of td3/policies.py (make_actor, make_critics), then the target scope
  void layout() {
    h.cnn = false;
    A = c.act_dim; L = c.n_layers; B = c.batch_size; NA = std::max(1, c.act_batch);
    for (int l = 0; l < L; ++l) hid[l] = c.layers[l];
    h.hw = 0; h.C_img = 0; h.img_elems = c.obs_dim; F = c.obs_dim; h.Fc = 0;
    ldf = (int)rup(F, 4);
    ldq = (int)rup(F + A, 4);
    Ap = (int)rup(A, 4);
    h.add_mlp("model/pi", h.m_pi, F, {"dense"}, A, true);
    h.vf_off = h.n_params;
    h.add_mlp("model/values_fn/qf1", h.m_qf1, F + A, {"qf1"}, 1, true);
    h.add_mlp("model/values_fn/qf2", h.m_qf2, F + A, {"qf2"}, 1, true);
    h.n_train = h.n_params;
    h.n_polyak = h.n_train;
    h.tgt_off = h.n_params;
    h.add_mlp("target/pi", tPI, F, {"dense"}, A, false);
    h.add_mlp("target/values_fn/qf1", tQ1, F + A, {"qf1"}, 1, false);
    h.add_mlp("target/values_fn/qf2", tQ2, F + A, {"qf2"}, 1, false);
  }

  void arenas() {
    // ---------------- state arena: a SAC handle's words, with the policy's optimiser words and the update cursor behind `sc`
    h.params = h.st.f32(h.n_params);
    h.adam_m = h.st.f32(h.n_train);
    h.adam_v = h.st.f32(h.n_train);
    h.sc = (DevScalars*)h.st.take(sizeof(DevScalars));
    h.sc2 = (DevScalars*)h.st.take(sizeof(DevScalars));
    h.td3_dev = (Td3Dev*)h.st.take(sizeof(Td3Dev));
    h.n_count = (double*)h.st.take(16);
    h.s_mean = (double*)h.st.take((size_t)F * 8);
    h.s_std = (double*)h.st.take((size_t)F * 8);
    h.s_dmean = (double*)h.st.take(8);
    h.s_dstd = (double*)h.st.take(8);
    h.s_ret = (double*)h.st.take(8);
    h.n_elems = F;
    h.n_mean = (double*)h.st.take((size_t)F * 8);     // (directly behind s_ret: grl_set_obs_stats uploads the span in one copy)
    h.n_var = (double*)h.st.take((size_t)F * 8);
    h.grads = h.gr.f32(h.n_train);
    // ---------------- replay arena
    cap = c.replay_capacity;
    h.rp_obs = h.rp.f32(cap * F);
    h.rp_next = h.rp.f32(cap * F);
    h.rp_dobs = h.rp.f32(cap);
    h.rp_dnext = h.rp.f32(cap);
    h.rp_act = h.rp.f32(cap * A);
    h.rp_rew = h.rp.f32(cap);
    h.rp_done = h.rp.f32(cap);
    // ---------------- staging (host-facing calls)
    h.stg_n = std::max(NA, 64);
    h.stg_obs = wk.f32((int64_t)h.stg_n * F);
    h.stg_next = wk.f32((int64_t)h.stg_n * F);
    h.stg_act = wk.f32((int64_t)h.stg_n * A);
    h.stg_rew = wk.f32(h.stg_n);
    h.stg_done = wk.f32(h.stg_n);
    h.n_stage = wk.f32((int64_t)h.stg_n * F);
    // ---------------- training workspace
    h.idx_buf = (int64_t*)wk.take((size_t)B * 8);
    h.eps_buf = wk.f32((int64_t)B * A);
    float** rows3[3] = {&xs, &xp, &xn};
    for (auto* r : rows3) {
      *r = wk.f32((int64_t)B * ldq);
      h.zero_once.push_back({*r, (size_t)B * ldq * 4});      // row padding [F + A, ldq) is read by 16-byte loads and by the weight-gradient launch
    }
    h.rew = wk.f32(B); h.done = wk.f32(B);
    h.alloc_head(hPI, B, 1, A); h.alloc_head(hPIT, B, 1, A);
    qbuf = wk.f32((int64_t)5 * B);                           // q1 | q2 | q1_target | q2_target | q1(s, pi(s)): one debug view
    HeadAct* qs[5] = {&hQ1, &hQ2, &hQ1T, &hQ2T, &hQ1PI};
    for (int k = 0; k < 5; ++k) { h.alloc_head(*qs[k], B, 0, 1); qs[k]->out[0] = qbuf + (int64_t)k * B; }
    backup = wk.f32(B); noise = wk.f32((int64_t)B * A); a_next = wk.f32((int64_t)B * A); pi_a = wk.f32((int64_t)B * A);
    da = wk.f32((int64_t)B * A);
    // output gradients: rows padded to 16 bytes for the weight-gradient launch, the padding stays zero
    float** dd[3] = {&d_q1, &d_q2, &d_q1pi};
    for (auto* q : dd) {
      *q = wk.f32((int64_t)B * 4);
      h.zero_once.push_back({*q, (size_t)B * 16});
    }
    dpre = wk.f32((int64_t)B * Ap);
    h.zero_once.push_back({dpre, (size_t)B * Ap * 4});
    h.alloc_hgrad(gQ1, B); h.alloc_hgrad(gQ2, B); h.alloc_hgrad(gQ1PI, B); h.alloc_hgrad(gPI, B);
    nblk = td3_loss_blocks(B);
    h.td3_nblk = nblk;
    h.td3_part = wk.f32((int64_t)GRL_TD3_MAX_UPDATES * nblk * TD3_DIAG);
    P = h.params;
  }

  // ---------------- the minibatch gather of a SAC handle on vector observations, writing into the critics' input rows
  int gather() {
    GatherArgs& ga = ga0;
    memset(&ga, 0, sizeof(ga));
    ga.idx = h.idx_buf; ga.B = B; ga.img_elems = F; ga.n_direct = 0; ga.act_dim = A;
    ga.rp_obs = h.rp_obs; ga.rp_next = h.rp_next; ga.rp_dobs = h.rp_dobs; ga.rp_dnext = h.rp_dnext;
    ga.rp_act = h.rp_act; ga.rp_rew = h.rp_rew; ga.rp_done = h.rp_done;
    ga.mean = h.s_mean; ga.stdv = h.s_std; ga.dmean = h.s_dmean; ga.dstd = h.s_dstd; ga.ret_std = h.s_ret;
    ga.normalize = (c.normalize == 1 || c.normalize == 2); ga.normalize_rew = (c.normalize == 1 || c.normalize == 3);
    ga.clip_obs = c.clip_obs; ga.clip_rew = c.clip_reward;
    ga.scale_div = 1.f;
    ga.x_obs = xs; ga.x_obs2 = xp; ga.x_next = xn; ga.ldx = ldq;
    ga.d_obs0 = ga.d_obs1 = ga.d_next = xs; ga.ldd = ldq;   // n_direct == 0: never written
    ga.act_out = xs + F; ga.ld_act = ldq; ga.rew_out = h.rew; ga.done_out = h.done;
    ga.sc = h.sc; ga.seed = c.seed; ga.idx_w = h.idx_buf; ga.eps_w = h.eps_buf;
    ga.n_eps = 0;      // (the normals are td3_smooth's: eps_buf holds what the caller handed over, if anything)
    ga.vec4 = elem_vec4_built() && (F % 4 == 0);
    ga.rows = 1;
    gx = (F + (ga.vec4 ? 1024 : 256) - 1) / (ga.vec4 ? 1024 : 256);
    gather_bytes = 2.0 * B * ((double)F * 8) + B * (4.0 * A + 8) * 2;
    return GRL_OK;
  }
  Op gather_op(bool rng) const {
    GatherArgs gm = ga0;
    gm.use_rng = rng ? 1 : 0;
    const int g = gx;
    Op op; op.tag = "gather_norm";
    op.bytes = gather_bytes;
    op.run = [gm, g](hipStream_t s) { launch_gather(gm, g, s); };
    return op;
  }
  Op smooth_op(bool rng) const {
    Td3SmoothArgs a;
    memset(&a, 0, sizeof(a));
    a.pre = hPIT.out[0]; a.ld_pre = A; a.eps = rng ? nullptr : h.eps_buf; a.sc = h.sc; a.seed = c.seed; a.dev = h.td3_dev;
    a.noise = noise; a.a_next = a_next; a.x_act = xn + F; a.ld_x = ldq; a.B = B; a.A = A;
    a.sigma = tc.target_policy_noise; a.clip = tc.target_noise_clip;
    Op op; op.tag = "td3_smooth";
    op.run = [a](hipStream_t s) { launch_td3_smooth(a, s); };
    return op;
  }
  Op loss_op(bool policy, bool tick_rng) const {
    Td3LossArgs a;
    memset(&a, 0, sizeof(a));
    a.rew = h.rew; a.done = h.done; a.q1 = hQ1.out[0]; a.q2 = hQ2.out[0]; a.q1t = hQ1T.out[0]; a.q2t = hQ2T.out[0]; a.q1pi = hQ1PI.out[0];
    a.backup = backup; a.d_q1 = d_q1; a.d_q2 = d_q2; a.d_q1pi = d_q1pi; a.ld_d = 4;
    a.part = h.td3_part; a.dev = h.td3_dev; a.sc = h.sc; a.sc_pi = h.sc2;
    a.B = B; a.gamma = c.gamma; a.policy = policy ? 1 : 0; a.tick_rng = tick_rng ? 1 : 0;
    Op op; op.tag = "td3_loss";
    op.run = [a](hipStream_t s) { launch_td3_loss(a, s); };
    return op;
  }
  static Op pi_op(const char* tag, const Td3PiArgs& a) {
    Op op; op.tag = tag;
    op.run = [a](hipStream_t s) { launch_td3_pi(a, s); };
    return op;
  }

  // ---------------- dense launches: the networks of `nets` level by level, then their output layers
  struct Net { const MlpP* m; const HeadAct* act; const float* x; int K; const HeadGrad* g; const float* dout; int ld_dout; };
  void forward(std::vector<Op>& ops, const std::vector<Net>& nets) {
    for (int l = 0; l < L; ++l) {
      std::vector<IgemmProb> pr;
      for (auto& n : nets) pr.push_back(h.head_layer(*n.m, P, *n.act, l, n.x, ldq, n.K, nullptr, 0, 0, B));
      h.add_launch(ops, "td3_fwd", 0, pr);
    }
    std::vector<IgemmProb> po;
    for (auto& n : nets) po.push_back(h.head_out(*n.m, P, *n.act, 0, B));
    h.add_launch(ops, "td3_fwd", 0, po);
  }
  // backward-data from the outputs down to the first hidden layer: g[l] = gradient w.r.t. the pre-activation of layer l
  void backward(std::vector<Op>& ops, const std::vector<Net>& nets) {
    {
      std::vector<IgemmProb> pr;
      for (auto& n : nets)
        pr.push_back(h.dense_bwd({{n.dout, n.ld_dout, n.m->out_dim, P + n.m->ow[0]}}, B, 0, hid[L - 1], n.g->g[L - 1], hid[L - 1], n.act->z[L - 1]));
      h.add_launch(ops, "td3_bwd", 1, pr);
    }
    for (int l = L - 1; l >= 1; --l) {      // (L = 1: no middle level)
      std::vector<IgemmProb> pr;
      for (auto& n : nets)
        pr.push_back(h.dense_bwd({{n.g->g[l], hid[l], hid[l], P + n.m->w[l]}}, B, 0, hid[l - 1], n.g->g[l - 1], hid[l - 1], n.act->z[l - 1]));
      h.add_launch(ops, "td3_bwd", 1, pr);
    }
  }
  void wgrads(std::vector<IgemmProb>& wg, const Net& n) {
    int64_t w[GRL_MAX_LAYERS + 1], b[GRL_MAX_LAYERS + 1];
    for (int l = 0; l < L; ++l) { w[l] = n.m->w[l]; b[l] = n.m->b[l]; }
    w[L] = n.m->ow[0]; b[L] = n.m->ob[0];
    h.add_stack_wgrads(wg, n.x, ldq, n.K, n.act->z, n.g->g, hid, L, n.dout, n.ld_dout, n.m->out_dim, w, b, B);
  }

  // Adam over [off, off + n) with the optimiser words `sc`; polyak: followed by target <- (1 - tau) target + tau online there
  Op adam_range(const char* tag, int64_t off, int64_t n, const DevScalars* sc, bool polyak) const {
    AdamArgs aa;
    memset(&aa, 0, sizeof(aa));
    aa.params = h.params + off; aa.grads = h.grads + off; aa.m = h.adam_m + off; aa.v = h.adam_v + off; aa.n_train = n; aa.sc = sc;
    aa.grad_scale = 1.f; aa.eps = 1e-8f;
    aa.tau = polyak ? c.tau : 0.f; aa.src_ofs = 0; aa.n_polyak = polyak ? n : 0; aa.target = h.params + h.tgt_off + off;
    Op op = grl_ctx::adam_op(tag, aa);
    op.bytes = (double)n * 4 * (polyak ? 9 : 7);
    return op;
  }

  // ---------------- one update: the launch list for handed-over indices and normals, then its three siblings
  void update(bool policy) {
    const Net nPIT{&tPI, &hPIT, xn, F, nullptr, nullptr, 0}, nPI{&h.m_pi, &hPI, xs, F, &gPI, dpre, Ap};
    const Net nQ1{&h.m_qf1, &hQ1, xs, F + A, &gQ1, d_q1, 4}, nQ2{&h.m_qf2, &hQ2, xs, F + A, &gQ2, d_q2, 4};
    const Net nQ1T{&tQ1, &hQ1T, xn, F + A, nullptr, nullptr, 0}, nQ2T{&tQ2, &hQ2T, xn, F + A, nullptr, nullptr, 0};
    const Net nQ1PI{&h.m_qf1, &hQ1PI, xp, F + A, &gQ1PI, d_q1pi, 4};
    std::vector<Op> ops;
    ops.push_back(gather_op(false));
    forward(ops, policy ? std::vector<Net>{nPIT, nQ1, nQ2, nPI} : std::vector<Net>{nPIT, nQ1, nQ2});
    const int at_smooth = (int)ops.size();
    ops.push_back(smooth_op(false));
    if (policy) {
      Td3PiArgs a;
      memset(&a, 0, sizeof(a));
      a.pre = hPI.out[0]; a.ld_pre = A; a.a = pi_a; a.ld_a = A; a.x_act = xp + F; a.ld_x = ldq; a.rows = B; a.A = A;
      ops.push_back(pi_op("td3_pi", a));
    }
    forward(ops, policy ? std::vector<Net>{nQ1T, nQ2T, nQ1PI} : std::vector<Net>{nQ1T, nQ2T});
    const int at_loss = (int)ops.size();
    ops.push_back(loss_op(policy, false));
    backward(ops, policy ? std::vector<Net>{nQ1, nQ2, nQ1PI} : std::vector<Net>{nQ1, nQ2});
    if (policy) {
      // d a: q1's first layer over the action columns of (s, pi(s)); nothing flows into the observations
      h.add_launch(ops, "td3_bwd", 1, {h.dense_bwd({{gQ1PI.g[0], hid[0], hid[0], P + h.m_qf1.w[0]}}, B, F, A, da, A, nullptr)});
      Td3PiArgs a;
      memset(&a, 0, sizeof(a));
      a.a = pi_a; a.ld_a = A; a.da = da; a.ld_da = A; a.dpre = dpre; a.ld_dpre = Ap; a.rows = B; a.A = A; a.bwd = 1;
      ops.push_back(pi_op("td3_pi_bwd", a));
      backward(ops, {nPI});
    }
    h.reduces.clear();      // (each of the two lists has a reduction launch of its own)
    std::vector<IgemmProb> wg;
    wgrads(wg, nQ1);
    wgrads(wg, nQ2);
    if (policy) wgrads(wg, nPI);
    h.add_launch(ops, "td3_wgrad", 2, wg);
    const grl_ctx::SumPlan sum = h.close_reduction();
    ops.push_back(sum.op);
    if (policy) h.d_reduces = sum.descs;
    ops.push_back(adam_range("adam_critic", h.vf_off, h.n_train - h.vf_off, h.sc, policy));
    if (policy) ops.push_back(adam_range("adam_pi", 0, h.vf_off, h.sc2, true));
    for (int v = 0; v < 4; ++v) {      // bit 0: indices drawn, bit 1: normals drawn
      std::vector<Op>& dst = h.ops_td3[policy ? 1 : 0][v];
      dst = ops;
      dst[0] = gather_op((v & 1) != 0);
      dst[at_smooth] = smooth_op((v & 2) != 0);
      dst[at_loss] = loss_op(policy, v != 0);
    }
  }

  // ---------------- act path (batch NA, the online policy): act_heads_kernel's layer loop where its limits allow, else a launch
  // per layer + td3_pi; the actions leave through page-locked host memory as a SAC handle's do
  int act_path() {
    h.afeat = wk.f32((int64_t)NA * ldf);
    h.zero_once.push_back({h.afeat, (size_t)NA * ldf * 4});
    if (!h.dry && h.act_io_host.reserve((size_t)2 * NA * A) != hipSuccess) return fail(GRL_ERR_HIP, "hipHostMalloc failed");
    h.a_eps = h.act_io_host.get();
    h.a_out = h.a_eps + (size_t)NA * A;
    HeadAct ahPI{};
    h.alloc_head(ahPI, NA, 1, A);
    float* const ls = wk.f32((int64_t)NA * A);
    ActIngestArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.obs = h.stg_obs; ia.n = NA; ia.vec_dim = F; ia.scale_div = 1.f;
    ia.x = h.afeat; ia.ldx = ldf; ia.d = h.afeat; ia.ldd = ldf;
    ActIngestArgs ian = ia;
    ian.normalize = 1; ian.clip_obs = c.clip_obs;
    ian.mean = h.s_mean; ian.stdv = h.s_std; ian.dmean = h.s_dmean; ian.dstd = h.s_dstd;
    for (int v = 0; v < 2; ++v) {      // [handed to grl_act] x [raw: VecNormalize applied here | already normalised]
      const ActIngestArgs iv = v ? ian : ia;
      const int elems = F;
      Op op; op.tag = "act_ingest";
      op.run = [iv, elems](hipStream_t s) { hipLaunchKernelGGL(act_ingest_kernel, dim3((elems + 255) / 256, iv.n), dim3(256), 0, s, iv); };
      h.ops_act_in[v].push_back(op);
    }
    bool one_launch = F <= ACT_HEADS_MAX_IN && A <= 64;
    for (int l = 0; l < L; ++l) one_launch = one_launch && hid[l] <= ACT_HEADS_MAX_HID;
    std::vector<Op> tail;
    if (one_launch) {
      ActHeadsArgs ha;
      memset(&ha, 0, sizeof(ha));
      ha.x = h.afeat; ha.ldx = ldf; ha.K0 = F; ha.L = L;
      for (int l = 0; l < L; ++l) { ha.w[l] = P + h.m_pi.w[l]; ha.b[l] = P + h.m_pi.b[l]; ha.hid[l] = hid[l]; }
      for (int k = 0; k < 2; ++k) { ha.ow[k] = P + h.m_pi.ow[0]; ha.ob[k] = P + h.m_pi.ob[0]; }      // (the kernel forms two output layers: the same one twice)
      ha.A = A; ha.eps = h.a_eps; ha.mu = ahPI.out[0]; ha.ls = ls; ha.out = h.a_out; ha.rows = NA; ha.deterministic = 1;
      Op op; op.tag = "act_heads";
      op.run = [ha](hipStream_t s) { hipLaunchKernelGGL(act_heads_kernel, dim3(ha.rows), dim3(256), 0, s, ha); };
      tail.push_back(op);
    } else {
      for (int l = 0; l < L; ++l)
        h.add_launch(tail, "act_head", 0, {h.head_layer(h.m_pi, P, ahPI, l, h.afeat, ldf, F, nullptr, 0, 0, NA)});
      h.add_launch(tail, "act_head", 0, {h.head_out(h.m_pi, P, ahPI, 0, NA)});
      Td3PiArgs a;
      memset(&a, 0, sizeof(a));
      a.pre = ahPI.out[0]; a.ld_pre = A; a.a = h.a_out; a.ld_a = A; a.rows = NA; a.A = A;
      tail.push_back(pi_op("td3_pi", a));
    }
    h.ops_act_det = h.ops_act_sto = tail;
    plan_note("grl plan: td3_act       %s, %d rows, obs %d\n", one_launch ? "one launch per call (act_heads_kernel)" : "launch list: dense levels + output + td3_pi", NA, F);
    return GRL_OK;
  }

  void debug_views() {
    auto& dbg = h.dbg;
    dbg["td3_a_next"] = {a_next, (int64_t)B * A}; dbg["td3_noise"] = {noise, (int64_t)B * A};
    dbg["td3_backup"] = {backup, B}; dbg["td3_q"] = {qbuf, (int64_t)5 * B};
    dbg["td3_pi"] = {pi_a, (int64_t)B * A}; dbg["td3_da"] = {da, (int64_t)B * A};
    dbg["td3_xs"] = {xs, (int64_t)B * ldq}; dbg["td3_xn"] = {xn, (int64_t)B * ldq};
    dbg["rew"] = {h.rew, B}; dbg["done"] = {h.done, B};
    dbg["td3_beta_c"] = {(const float*)h.sc, 2}; dbg["td3_beta_pi"] = {(const float*)h.sc2, 2};
    dbg["grads"] = {h.grads, h.n_train};
    dbg["adam_m"] = {h.adam_m, h.n_train};
    dbg["adam_v"] = {h.adam_v, h.n_train};
    dbg["rp_obs"] = {h.rp_obs, cap * F}; dbg["rp_next"] = {h.rp_next, cap * F};
    dbg["rp_act"] = {h.rp_act, cap * A}; dbg["rp_rew"] = {h.rp_rew, cap}; dbg["rp_done"] = {h.rp_done, cap};
    dbg["idx_raw"] = {(const float*)h.idx_buf, (int64_t)2 * B};     // replay indices of the last minibatch: int64 viewed as float pairs
    plan_note("grl plan: td3 critic-only update %zu launches, policy update %zu launches, policy_delay %d\n", h.ops_td3[0][3].size(),
              h.ops_td3[1][3].size(), tc.policy_delay);
    plan_seq("td3_critic", h.ops_td3[0][3]); plan_seq("td3_policy", h.ops_td3[1][3]);
  }
};

}  // namespace

int grl_ctx::plan_td3() {
  Td3Planner p(*this);
  p.layout();
  p.arenas();
  if (int e = p.gather()) return e;
  p.update(false);
  p.update(true);
  if (int e = p.act_path()) return e;
  p.debug_views();
  return GRL_OK;
}
