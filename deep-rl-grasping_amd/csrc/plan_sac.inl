// plan_sac.inl: launch plan of the SAC update, the act path and the encoder forward (grl_ctx::plan_sac) -- part of engine.hip (included there, same translation unit: the plans are methods of grl_ctx).

namespace {

typedef grl_ctx::SacKit SacKit;

// The launches of ONE update inside a call of several updates on the device RNG, assembled from the recorded slots of
// ops_grads_apply and the replaceable launches of h.sac_kit: position v (0 first, 1 middle, 2 last of the call), image flavour
// f (the buffer the update reads), `ride`: the "gather_ride" form (else "prefetch"); `close` ends the update in place of the
// closing reduction.  Every variant of a multi-update call -- here and at connect -- comes from this function.
std::vector<Op> sac_update_ops(const grl_ctx& h, int v, int f, bool ride, const std::vector<Op>& close) {
  const SacKit& k = h.sac_kit;
  std::vector<Op> out;
  if (v == 0) out.push_back(k.gather[ride]);
  for (int i = 0; i < k.close; ++i) {
    if (i == k.heads) out.push_back(ride && v != 2 ? k.heads_ride[f][v != 0] : k.heads_open[v != 0]);
    else if (ride && f && i == k.stack) out.push_back(k.stack_b);
    else if (ride && f && i == k.wgrad_conv) out.push_back(k.wgrad_conv_b);
    else out.push_back(h.ops_grads_apply[i]);
  }
  out.insert(out.end(), close.begin(), close.end());
  return out;
}
// ... of every part of a call plan; close(v): the launches that end an update at position v
void sac_call_plan(const grl_ctx& h, CallPlan& p, bool ride, const std::function<std::vector<Op>(int)>& close) {
  p.clear();
  p.alternate = ride;
  for (int v = 0; v < 3; ++v)
    for (int f = 0; f < (v > 0 && ride ? 2 : 1); ++f) p.part(v, f) = sac_update_ops(h, v, f, ride, close(v));
}

struct SacPlanner {
  grl_ctx& h;
  const grl_config& c;
  // the handle's shapes (written by shapes()), work arena and switches under the names every step uses
  bool& cnn;
  int &A, &L, &B, &NA, &hw, &C_img, &img_elems, &F, &Fc, &ldf;
  SacGeom& geo;                                     // o1 / o2 / o3, their squares and the dense K of the handle's image size
  int* const hid;
  Arena& wk;
  const Switches& sw;
  int nd = 0;                                       // direct features behind the 512 of the CNN
  int64_t cap = 0, obs_store = 0, obs_elems = 0;    // replay rows; floats of a stored / a staged observation
  const float* P = nullptr;                         // params (the target block uses absolute offsets too)
  // routes
  bool fused_heads = false;          // heads_kernels.h path (row-local chains) instead of per-layer GEMMs
  bool heads_mfma = false;           // heads_mfma.h: forward + backward of all heads as ONE launch on 16x16x4 MFMAs
  bool conv_stack = false;           // conv1 -> conv2 -> conv3 as one sample-local launch (conv_stack.h)
  bool conv_stack_bwd = false;       // ... and the backward-data of conv3 -> conv2
  int store_drain = 0;               // tensor groups of the CNN plan stored write-through (store_drain.h: StoreDrain bits)
  // training workspace (what a route does not allocate stays null)
  float* x_obs_b = nullptr;          // second image buffer ("gather_ride")
  float *a1[3] = {}, *a2[3] = {}, *a3[3] = {};
  HeadAct hPI{}, hVF{}, hQF1{}, hQF2{}, hTGT{}, hQF1PI{}, hQF2PI{};
  float *pi_a = nullptr, *logp = nullptr, *ent = nullptr;
  float *d_qf1 = nullptr, *d_qf2 = nullptr, *d_v = nullptr, *d_qf1pi = nullptr;
  HeadGrad gPI{}, gVF{}, gQF1{}, gQF2{}, gQF1PI{};
  float *da_pi = nullptr, *dmu = nullptr, *dls = nullptr;
  float *dfeat[2] = {}, *g3[2] = {}, *g2[2] = {}, *g1[2] = {};
  int ld1 = 64;                      // pixel stride of a1 / g1: the two trained networks side by side
  float* act_p = nullptr;            // [B, Ap] row-padded copy of the minibatch actions (Ap = rup(A, 4))
  int Ap = 0, ld_d = 1, ld_dm = 0;   // strides of the packed output-gradient buffers (fused heads)
  float* u_l0[5] = {};               // layer-0 feature partials: pi, vf, qf1, qf2, target
  int l0_split = 1;
  float* g0cat = nullptr;            // [B, 3*H0]: layer-0 gradients of vf | qf1 | qf2
  // forward / backward through the CNNs
  ConvGeom cg[3];
  ConvFwdTabs ft[3];
  ConvStackArgs stack_args{};        // arguments of the forward stack as planned (reading x_obs)
  int rider_budget = 0;              // empty slots of conv3_bwd's last dispatch round
  std::vector<IgemmProb> bwd_pr[3];  // backward-data stages fc, conv3, conv2 (launched once their fillers are known)
  std::vector<IgemmProb> wg, wgc[3]; // weight gradients: dense layers / conv layers 1..3
  std::vector<IgemmProb> dense_affine, conv_all;   // dense / conv weight-gradient problems as first built (staged plan)
  bool only_vec_dense = false;
  std::vector<Op> conv3_bwd_plain;   // conv3_bwd without riders, for the staged data-parallel plan
  int bwd_begin = -1, bwd_end = -1;  // positions in ops_grads beside the slots of h.sac_kit: the backward-data launches [begin, end),
  int conv3 = -1, conv3_n = 0;       // among them conv3_bwd with its riders (conv3_n launches)
  bool have_wgrad_conv_b = false;
  // the head launch (heads_mfma) and the reductions, as the call plans rebuild them
  GatherArgs ga0{};                  // the minibatch gather as planned (use_rng open), and its workgroups per row
  int gx = 0;
  const HeadsFusedArgs* d_heads = nullptr;   // [3] argument blocks of the head launch (plain, first, later updates)
  int heads_shape = 0, heads_nblk = 0;
  ReduceDesc* dr = nullptr;
  int2* d_rt = nullptr;
  int ntiles = 0, has_loss = 0;
  AdamArgs aa{};

  explicit SacPlanner(grl_ctx& ctx)
      : h(ctx), c(ctx.cfg), cnn(ctx.cnn), A(ctx.A), L(ctx.L), B(ctx.B), NA(ctx.NA), hw(ctx.hw), C_img(ctx.C_img), img_elems(ctx.img_elems),
        F(ctx.F), Fc(ctx.Fc), ldf(ctx.ldf), geo(ctx.geo), hid(ctx.hid), wk(ctx.wk), sw(ctx.sw) {}

  void shapes() {
    cnn = c.extractor != GRL_EXTRACTOR_MLP;
    A = c.act_dim; L = c.n_layers; B = c.batch_size; NA = std::max(1, c.act_batch);
    for (int l = 0; l < L; ++l) hid[l] = c.layers[l];
    hw = c.img_hw;
    nd = cnn && c.extractor == GRL_EXTRACTOR_AUGMENTED ? c.n_direct : 0;
    if (cnn) {
      C_img = c.obs_channels - (nd > 0 ? 1 : 0);
      img_elems = hw * hw * C_img;
      F = 512 + nd; Fc = 512;
      for (int l = 0; l < 3; ++l) cg[l] = cnn_geom(l, C_img, hw);
      cg[0].ldy = cg[1].ldx = ld1;
      geo.from(cg);
    } else {
      C_img = 0; img_elems = c.obs_dim; F = c.obs_dim; Fc = 0;
    }
    ldf = (int)rup(F, 4);
    h.build_layout();
  }

  // The addressing tables hold 32-bit element offsets, and the GEMM kernels reach their operands through buffer descriptors
  // with 32-bit byte offsets below 2 GiB (igemm2.h: i2_rsrc; beyond it a load returns zeros): the largest buffer a table
  // walks -- an image buffer, the a1 / g1 pair, for the minibatch and for the acting pass -- must stay below 2^31 bytes.
  int fits() const {
    if (!cnn) return GRL_OK;
    const int64_t rows = std::max(B, std::max(NA, 64));
    const int64_t per_row = std::max<int64_t>({(int64_t)hw * hw * c.obs_channels, (int64_t)geo.p1 * ld1, (int64_t)geo.p2 * 64, (int64_t)geo.K});
    if (4 * rows * per_row >= ((int64_t)1 << 31))
      return fail(GRL_ERR_INVALID, "SAC: " + std::to_string(hw) + "x" + std::to_string(hw) + " images at batch_size " + std::to_string(B) + " / act_batch " +
                                       std::to_string(NA) + " need a buffer of " + std::to_string(4 * rows * per_row) +
                                       " bytes: tables and buffer descriptors hold 32-bit offsets (fewer than 2^31 bytes per buffer)");
    return GRL_OK;
  }

  void arenas() {
    // ---------------- state arena
    h.params = h.st.f32(h.n_params);
    h.adam_m = h.st.f32(h.n_train);
    h.adam_v = h.st.f32(h.n_train);
    h.sc = (DevScalars*)h.st.take(sizeof(DevScalars));
    h.n_count = (double*)h.st.take(16);
    h.s_mean = (double*)h.st.take((size_t)img_elems * 8);
    h.s_std = (double*)h.st.take((size_t)img_elems * 8);
    h.s_dmean = (double*)h.st.take((size_t)std::max(nd, 1) * 8);
    h.s_dstd = (double*)h.st.take((size_t)std::max(nd, 1) * 8);
    h.s_ret = (double*)h.st.take(8);
    h.n_elems = cnn ? (int64_t)hw * hw * c.obs_channels : c.obs_dim;
    h.n_mean = (double*)h.st.take((size_t)h.n_elems * 8);     // (directly behind s_ret: grl_set_obs_stats uploads the span in one copy)
    h.n_var = (double*)h.st.take((size_t)h.n_elems * 8);
    h.grads = h.gr.f32(h.n_train);

    // ---------------- replay arena
    cap = c.replay_capacity;
    // stored observation: img_elems floats, or (replay_rgb_u8) one packed colour dword + one depth float per pixel
    obs_store = c.replay_rgb_u8 ? 2 * (int64_t)hw * hw : img_elems;
    h.rp_obs = h.rp.f32(cap * obs_store);
    h.rp_next = h.rp.f32(cap * obs_store);
    h.rp_dobs = h.rp.f32(cap * std::max(nd, 1));
    h.rp_dnext = h.rp.f32(cap * std::max(nd, 1));
    h.rp_act = h.rp.f32(cap * A);
    h.rp_rew = h.rp.f32(cap);
    h.rp_done = h.rp.f32(cap);

    // ---------------- staging (host-facing calls)
    obs_elems = cnn ? (int64_t)hw * hw * c.obs_channels : c.obs_dim;
    h.stg_n = std::max(NA, 64);
    h.stg_obs = wk.f32(h.stg_n * obs_elems);
    h.stg_next = wk.f32(h.stg_n * obs_elems);
    h.stg_act = wk.f32((int64_t)h.stg_n * A);
    h.stg_rew = wk.f32(h.stg_n);
    h.stg_done = wk.f32(h.stg_n);
    h.n_stage = wk.f32(h.stg_n * obs_elems);
    // observed observations (grl_observe): the newest env step's and the one before it, uploaded once each; terminal rows
    // and the small per-step arrays of grl_replay_add_observed
    h.ob_latest = wk.f32(h.stg_n * obs_elems);
    h.ob_prev = wk.f32(h.stg_n * obs_elems);
    h.ob_term = wk.f32(h.stg_n * obs_elems);
    h.ob_elems = obs_elems;

    // ---------------- training workspace
    h.idx_buf = (int64_t*)wk.take((size_t)B * 8);
    h.eps_buf = wk.f32((int64_t)B * A);
    for (int n = 0; n < 3; ++n) {
      h.feat[n] = wk.f32((int64_t)B * ldf);
      h.zero_once.push_back({h.feat[n], (size_t)B * ldf * 4});   // row padding [F, ldf) is read by 16-byte loads
    }
    if (cnn) {
      h.x_obs = wk.f32((int64_t)B * img_elems);
      h.x_next = wk.f32((int64_t)B * img_elems);
      x_obs_b = sw.get(Sw::gather_ride) != 0 ? wk.f32((int64_t)B * img_elems) : nullptr;     // second image buffer ("gather_ride" below)
      // Layer-1 activations of the two TRAINED networks (and their gradients below) sit side by side, pixel stride 64:
      // pi in columns 0..31, values_fn in 32..63.  Both networks read the same observations, so conv1's weight
      // gradient becomes ONE product obs-patches^T x [dY_pi | dY_vf] (N = 64: full 64x64 tiles, the gathered patches
      // read once) instead of two half-empty ones.  The target network's buffer keeps the stride (columns 32..63 idle)
      // so that one set of conv2 tables serves all three.
      ld1 = 64;
      float* a1_pair = wk.f32((int64_t)B * geo.p1 * 64);
      for (int n = 0; n < 3; ++n) {
        a1[n] = n < 2 ? a1_pair + 32 * n : wk.f32((int64_t)B * geo.p1 * 64);
        a2[n] = wk.f32((int64_t)B * geo.p2 * 64);
        a3[n] = wk.f32((int64_t)B * geo.p3 * 64);
      }
    }
    h.act = wk.f32((int64_t)B * A); h.rew = wk.f32(B); h.done = wk.f32(B);
    h.alloc_head(hPI, B, 2, A); h.alloc_head(hVF, B, 1, 1); h.alloc_head(hQF1, B, 1, 1); h.alloc_head(hQF2, B, 1, 1);
    h.alloc_head(hTGT, B, 1, 1); h.alloc_head(hQF1PI, B, 1, 1); h.alloc_head(hQF2PI, B, 1, 1);
    pi_a = wk.f32((int64_t)B * A); logp = wk.f32(B); ent = wk.f32(B);
    fused_heads = !sw.get(Sw::GRL_NO_FUSED_HEADS) && A <= HT_MAXA && (hid[0] % 4) == 0;
    for (int l = 0; l < L; ++l) fused_heads = fused_heads && hid[l] <= HT_MAXW;
    Ap = (int)rup(A, 4);
    if (fused_heads) {
      // output gradients packed / row-padded so that the weight-gradient GEMM can fetch them 16 bytes at a time
      float** dd[4] = {&d_v, &d_qf1, &d_qf2, &d_qf1pi};
      for (auto* q : dd) {
        *q = wk.f32((int64_t)B * 4);
        h.zero_once.push_back({*q, (size_t)B * 16});
      }
      ld_d = 4;
      act_p = wk.f32((int64_t)B * Ap);
      h.zero_once.push_back({act_p, (size_t)B * Ap * 4});
    } else {
      d_qf1 = wk.f32(B); d_qf2 = wk.f32(B); d_v = wk.f32(B); d_qf1pi = wk.f32(B); ld_d = 1;
    }
    if (fused_heads) {
      {
        l0_split = std::max(1, sw.get(Sw::l0_split));       // reduction of the layer-0 GEMM (K = 513) cut into partial sums
        IgemmProb probe = h.blank();
        probe.M = B; probe.N = hid[0]; probe.K = F;
        h.set_split(probe, l0_split);
        l0_split = probe.split;
      }
      for (int k = 0; k < 5; ++k) u_l0[k] = wk.f32((int64_t)B * hid[0] * l0_split);
      g0cat = wk.f32((int64_t)B * 3 * hid[0]);
      h.alloc_hgrad(gPI, B);
      h.alloc_hgrad(gVF, B, g0cat, 3 * hid[0]);
      h.alloc_hgrad(gQF1, B, g0cat + hid[0], 3 * hid[0]);
      h.alloc_hgrad(gQF2, B, g0cat + 2 * hid[0], 3 * hid[0]);
      h.alloc_hgrad(gQF1PI, B);
    } else {
      h.alloc_hgrad(gPI, B); h.alloc_hgrad(gVF, B); h.alloc_hgrad(gQF1, B); h.alloc_hgrad(gQF2, B); h.alloc_hgrad(gQF1PI, B);
    }
    ld_dm = fused_heads ? Ap : A;
    da_pi = wk.f32((int64_t)B * A); dmu = wk.f32((int64_t)B * ld_dm); dls = wk.f32((int64_t)B * ld_dm);
    if (fused_heads) {
      h.zero_once.push_back({dmu, (size_t)B * ld_dm * 4});
      h.zero_once.push_back({dls, (size_t)B * ld_dm * 4});
    }
    if (cnn) {
      float* g1_pair = wk.f32((int64_t)B * geo.p1 * 64);
      for (int n = 0; n < 2; ++n) {
        dfeat[n] = wk.f32((int64_t)B * ldf);
        g3[n] = wk.f32((int64_t)B * geo.p3 * 64);
        g2[n] = wk.f32((int64_t)B * geo.p2 * 64);
        g1[n] = g1_pair + 32 * n;
      }
    }
    P = h.params;
  }

  static Op gather_op(const GatherArgs& ga, int gx, double bytes) {
    Op op; op.tag = "gather_norm";
    op.bytes = bytes;
    op.run = [ga, gx](hipStream_t s) { launch_gather(ga, gx, s); };
    return op;
  }

  int gather() {
    // =============================================================== minibatch: replay gather (+ device RNG)
    GatherArgs& ga = ga0;
    memset(&ga, 0, sizeof(ga));
    ga.idx = h.idx_buf; ga.B = B; ga.img_elems = img_elems; ga.n_direct = nd; ga.act_dim = A;
    ga.rp_obs = h.rp_obs; ga.rp_next = h.rp_next; ga.rp_dobs = h.rp_dobs; ga.rp_dnext = h.rp_dnext;
    ga.rp_act = h.rp_act; ga.rp_rew = h.rp_rew; ga.rp_done = h.rp_done;
    ga.mean = h.s_mean; ga.stdv = h.s_std; ga.dmean = h.s_dmean; ga.dstd = h.s_dstd; ga.ret_std = h.s_ret;
    ga.normalize = (c.normalize == 1 || c.normalize == 2); ga.normalize_rew = (c.normalize == 1 || c.normalize == 3);
    ga.clip_obs = c.clip_obs; ga.clip_rew = c.clip_reward;
    ga.scale_div = cnn ? 255.f : 1.f;
    if (cnn) {
      ga.x_obs = h.x_obs; ga.x_obs2 = nullptr; ga.x_next = h.x_next; ga.ldx = img_elems;
      ga.d_obs0 = h.feat[0] + 512; ga.d_obs1 = h.feat[1] + 512; ga.d_next = h.feat[2] + 512; ga.ldd = ldf;
    } else {
      ga.x_obs = h.feat[0]; ga.x_obs2 = h.feat[1]; ga.x_next = h.feat[2]; ga.ldx = ldf;
      ga.d_obs0 = ga.d_obs1 = ga.d_next = h.feat[0]; ga.ldd = ldf;   // n_direct == 0: never written
    }
    ga.act_out = h.act; ga.ld_act = A; ga.rew_out = h.rew; ga.done_out = h.done;
    ga.act_out2 = act_p; ga.ld_act2 = Ap;
    ga.rgb_u8 = c.replay_rgb_u8;
    ga.sc = h.sc; ga.seed = c.seed; ga.idx_w = h.idx_buf; ga.eps_w = h.eps_buf; ga.n_eps = A;
    ga.adam_tick = fused_heads ? 1 : 0;   // otherwise sac_loss_kernel fixes the step size
    ga.vec4 = elem_vec4_built() && (img_elems % 4 == 0) && (ga.ldx % 4 == 0);
    const int per_block = ga.vec4 ? 1024 : 256;
    // rows per workgroup of the grouped form (elem_kernels.h: gather_norm_rows_body); GRL_TUNE gather_rows=1 keeps one row each
    {
      int rows = sw.text(Sw::gather_rows) ? sw.get(Sw::gather_rows) : (c.replay_rgb_u8 ? GATHER_ROWS_U8 : GATHER_ROWS_F32);
      if (!ga.vec4 || !gather_rows_built(rows) || B % rows) rows = 1;
      ga.rows = rows;
      if (!gather_rows_built(ga.rows)) return fail(GRL_ERR_INVALID, "gather: no kernel for this many rows per workgroup");
    }
    gx = (ga.img_elems + per_block - 1) / per_block;
    const double bytes = 2.0 * B * ((double)img_elems * 4 + (double)obs_store * 4 + 4.0 * nd) + B * (4.0 * A + 8) * 2;
    for (int mode = 0; mode < 2; ++mode) {
      GatherArgs gm = ga;
      gm.use_rng = mode;
      (mode ? h.ops_rng : h.ops_gather).push_back(gather_op(gm, gx, bytes));
    }
    return GRL_OK;
  }

  // the forward stack of the three networks reading the observations from `obs` (x_obs, or the second image buffer)
  Op stack_fwd_op(const float* obs) const {
    ConvStackArgs ca = stack_args;
    ca.nets[0].x = ca.nets[1].x = obs;
    const int Ci = C_img;
    Op op; op.tag = "conv_stack_fwd";
    op.flops = op.flops_exec = 2.0 * B * 3 * ((double)geo.p1 * 32 * 64 * Ci + (double)geo.p2 * 64 * 512 + (double)geo.p3 * 64 * 576);
    op.run = [ca, Ci](hipStream_t s) { launch_conv_stack_fwd(Ci, ca, s); };
    return op;
  }

  // conv1 -> conv2 -> conv3 of the three networks as ONE sample-local launch (conv_stack.h; a workgroup owns a sample of a network
  // and keeps the activation chain in LDS).  The target network's layer-1 / layer-2 activations are not stored.
  void forward_stack(const float* const xin[3]) {
    memset(&stack_args, 0, sizeof(stack_args));
    for (int n = 0; n < 3; ++n) {
      ConvStackNet& cn = stack_args.nets[n];
      cn.x = xin[n];
      for (int l = 0; l < 3; ++l) { cn.w[l] = P + h.ex[n].w[l]; cn.b[l] = P + h.ex[n].b[l]; }
      cn.a1 = n < 2 ? a1[n] : nullptr; cn.a2 = n < 2 ? a2[n] : nullptr; cn.a3 = a3[n]; cn.ld1 = ld1;
    }
    stack_args.B = B; stack_args.n_nets = 3;
    stack_args.drain_a12 = (store_drain & SD_A12) != 0;
    h.sac_kit.stack = (int)h.ops_grads.size();
    h.ops_grads.push_back(stack_fwd_op(h.x_obs));
  }

  // ... as one implicit-GEMM launch per layer
  void forward_layers(const float* const xin[3]) {
    const char* tags[3] = {"conv1_fwd", "conv2_fwd", "conv3_fwd"};
    for (int l = 0; l < 3; ++l) {
      std::vector<IgemmProb> pr;
      for (int n = 0; n < 3; ++n) {
        const float* in = l == 0 ? xin[n] : (l == 1 ? a1[n] : a2[n]);
        float* out = l == 0 ? a1[n] : (l == 1 ? a2[n] : a3[n]);
        pr.push_back(h.conv_fwd(in, ft[l], cg[l], P + h.ex[n].w[l], P + h.ex[n].b[l], out, ACT_RELU, 0.f));
        if (store_drain & (l == 2 ? SD_A3 : SD_A12)) pr.back().vflags |= VF_C_DRAIN;     // (the target network's a1 / a2 too: same launch)
      }
      h.add_launch(h.ops_grads, tags[l], 0, pr);
    }
  }

  // =============================================================== forward through the three CNNs: observations -> feat
  void forward() {
    if (!cnn) return;
    for (int l = 0; l < 3; ++l) ft[l] = h.conv_fwd_tabs(cg[l], B);     // (cg: shapes())
    const float* const xin[3] = {h.x_obs, h.x_obs, h.x_next};
    // tensor groups whose 16-byte stores leave write-through (store_drain.h; GRL_TUNE store_drain=<mask>, bits outside SD_ALL
    // are ignored).  The buffer instruction takes 32-bit byte offsets: the largest buffers of the groups -- an image buffer, the
    // a1 / g1 pair -- must stay below SD_MAX_BYTES, else every group keeps plain stores and the plan dump says why.
    {
      const int64_t largest = 4 * std::max<int64_t>((int64_t)B * img_elems, (int64_t)B * geo.p1 * 64);
      // (SD_A12 belongs to the forward stack, which runs 64x64 images only: other sizes do not take that bit)
      const int asked = sw.get(Sw::store_drain) & (hw == 64 ? SD_ALL : SD_ALL & ~SD_A12);
      store_drain = largest < SD_MAX_BYTES ? asked : 0;
      plan_note("grl plan: store_drain   mask %d (1 a1+a2, 2 a3 [per-layer route], 4 g1+g2, 8 weight-gradient slabs, 16 riders' images)%s\n", store_drain,
                store_drain != asked ? "  [asked for more: a buffer of this batch reaches 2 GiB, all stores plain]" : "");
    }
    // the stack for 1 / 2 / 4 image channels; GRL_TUNE conv_stack=0 or any other channel count: a launch per layer
    // (GRL_NO_V2: the scalar-gather fallback test runs the per-layer launches on igemm_kernel).  conv_stack.h is built around
    // 15x15 / 6x6 / 4x4: every other image size runs the per-layer launches whatever GRL_TUNE says (and with it conv_stack_bwd)
    conv_stack = conv_stack_ok(C_img) && hw == 64 && sw.get(Sw::conv_stack) != 0 && !sw.get(Sw::GRL_NO_V2);
    if (hw != 64) plan_note("grl plan: sac image %dx%d per-layer convolutions (conv_stack is 64x64 only)\n", hw, hw);
    if (conv_stack) forward_stack(xin);
    else forward_layers(xin);
    std::vector<IgemmProb> pr;
    for (int n = 0; n < 3; ++n)
      pr.push_back(h.dense_fwd(a3[n], geo.K, geo.K, nullptr, 0, 0, B, P + h.ex[n].fw, 512, P + h.ex[n].fb, h.feat[n], ldf, ACT_RELU));
    h.add_launch(h.ops_grads, "fc_fwd", 0, pr);
  }

  // description of one head for the row-local kernels (heads_kernels.h)
  HtHead mk_head(const MlpP& m, const HeadAct& ha, const HeadGrad* g, const float* u, const float* xa, int ld_xa, int n_xa) {
    HtHead H;
    memset(&H, 0, sizeof(H));
    H.u = u; H.ldu = hid[0]; H.u_split = l0_split; H.u_stride = (long)B * hid[0];
    H.xa = xa; H.ld_xa = ld_xa; H.n_xa = n_xa;
    H.w0a = P + m.w[0] + (int64_t)F * hid[0];
    H.b0 = P + m.b[0]; H.z0 = ha.z[0]; H.H0 = hid[0]; H.L = L;
    for (int l = 0; l < L; ++l) H.hid[l] = hid[l];
    for (int l = 1; l < L; ++l) { H.w[l] = P + m.w[l]; H.b[l] = P + m.b[l]; H.z[l] = ha.z[l]; }
    if (g) {
      H.g0 = g->g[0]; H.ldg0 = g->ld0;
      for (int l = 1; l < L; ++l) H.g[l] = g->g[l];
    }
    H.n_out = m.n_out; H.out_dim = m.out_dim;
    for (int k = 0; k < m.n_out; ++k) { H.ow[k] = P + m.ow[k]; H.ob[k] = P + m.ob[k]; H.out[k] = ha.out[k]; }
    return H;
  }

  // layer 0 of the five networks' heads, feature part only (no bias, no activation): u = feat . W0[0:F]
  void heads_l0() {
    const MlpP* ms[5] = {&h.m_pi, &h.m_vf, &h.m_qf1, &h.m_qf2, &h.m_tgt};
    const float* fin[5] = {h.feat[0], h.feat[1], h.feat[1], h.feat[1], h.feat[2]};
    std::vector<IgemmProb> pr;
    for (int k = 0; k < 5; ++k) {
      IgemmProb p = h.dense_fwd(fin[k], ldf, F, nullptr, 0, 0, B, P + ms[k]->w[0], hid[0], nullptr, u_l0[k], hid[0], ACT_NONE);
      h.set_split(p, l0_split);     // partial sums [split][B, H0]: the head chains add them (40 -> 120 workgroups)
      pr.push_back(p);
    }
    h.add_launch(h.ops_grads, "heads_l0", 0, pr);
  }

  // loss arguments (batch reductions; they ride on the slab reduction with fused heads, else a launch of their own here)
  void loss() {
    LossArgs la;
    la.B = B; la.gamma = c.gamma; la.target_entropy = c.target_entropy; la.lr = c.lr;
    la.rew = h.rew; la.done = h.done; la.v_tgt = hTGT.out[0]; la.qf1 = hQF1.out[0]; la.qf2 = hQF2.out[0];
    la.v = hVF.out[0]; la.qf1_pi = hQF1PI.out[0]; la.qf2_pi = hQF2PI.out[0]; la.logp = logp; la.entropy = ent;
    la.log_ent_coef = h.params + h.ent_off;
    la.d_qf1 = d_qf1; la.d_qf2 = d_qf2; la.d_v = d_v; la.d_qf1_pi = d_qf1pi; la.ld_d = ld_d;
    la.g_log_ent_coef = h.grads + h.ent_off; la.sc = h.sc;
    la.write_d = fused_heads ? 0 : 1;
    la.adam_ticked = fused_heads ? 1 : 0;
    la.ent_param = h.params + h.ent_off; la.ent_m = h.adam_m + h.ent_off; la.ent_v = h.adam_v + h.ent_off;
    h.loss_args = la;
    if (!fused_heads) {   // fused heads: output gradients are formed in heads_bwd_kernel, reductions ride on reduce_slabs
      Op op; op.tag = "sac_loss";
      op.run = [la](hipStream_t s) { hipLaunchKernelGGL(sac_loss_kernel, dim3(1), dim3(256), 0, s, la); };
      h.ops_grads.push_back(op);
    }
  }

  // d feat = g0 . W0[0:Fc]^T, masked by feat > 0.  Critic net: the three layer-0 gradients sit side
  // by side in g0cat and the three kernels are reached through a table (K = 3*H0 in one pass).
  void heads_dfeat() {
    const int H0 = hid[0];
    std::vector<int32_t> qt3(3 * H0), qt1(H0);
    const int64_t offs[3] = {h.m_vf.w[0], h.m_qf1.w[0], h.m_qf2.w[0]};
    for (int k = 0; k < 3; ++k)
      for (int n = 0; n < H0; ++n) qt3[k * H0 + n] = (int32_t)(offs[k] - offs[0]) + n;
    for (int n = 0; n < H0; ++n) qt1[n] = n;
    auto tab_bwd = [&](const float* g, int ldg, int K, const float* wbase, const int32_t* dtab, float* dx,
                       const float* mask) {
      IgemmProb p = h.blank();
      p.M = B; p.N = Fc; p.K = K;
      p.p_base[0] = g; p.p_ld_i[0] = ldg; p.p_ld_r[0] = 1; h.single_part(p);
      p.q_base[0] = wbase; p.q_tab_r = dtab; p.q_ld_j[0] = H0;
      p.c = dx; p.ldc = ldf; p.relu_mask = mask;
      p.vflags = VF_Q_TAB;
      h.set_split(p, 1);
      return p;
    };
    std::vector<IgemmProb> pr;
    pr.push_back(tab_bwd(g0cat, 3 * H0, 3 * H0, P + h.m_vf.w[0], h.upload_vec(wk, qt3), dfeat[1], h.feat[1]));
    pr.push_back(tab_bwd(gPI.g[0], H0, H0, P + h.m_pi.w[0], h.upload_vec(wk, qt1), dfeat[0], h.feat[0]));
    h.add_launch(h.ops_grads, "heads_dfeat", 1, pr);
    h.sac_kit.dfeat = (int)h.ops_grads.size() - 1;
  }

  // the head launch on argument block v (0 plain, 1 / 2 opening the first / a later update of a call), `riders`: with the
  // image gather of the next update as extra workgroups
  Op heads_op(int v, const GatherArgs* riders) const {
    Op op; op.tag = "heads";
    const HeadsFusedArgs* dv = d_heads + v;
    const int nblk = heads_nblk, shape = heads_shape, rgx = gx;
    if (riders) {
      const GatherArgs gi = *riders;
      op.bytes = h.ops_rng[0].bytes;
      op.run = [dv, nblk, shape, gi, rgx](hipStream_t s) { launch_heads_fused(shape, nblk, s, dv, &gi, rgx); };
    } else {
      op.run = [dv, nblk, shape](hipStream_t s) { launch_heads_fused(shape, nblk, s, dv); };
    }
    return op;
  }

  // route 1: forward and backward of every head in ONE launch on the matrix cores (heads_mfma.h)
  void heads_one_launch() {
    heads_l0();
    HeadsFusedArgs ha;
    memset(&ha, 0, sizeof(ha));
    ha.h[0] = mk_head(h.m_pi, hPI, &gPI, u_l0[0], nullptr, 0, 0);
    ha.h[1] = mk_head(h.m_vf, hVF, &gVF, u_l0[1], nullptr, 0, 0);
    ha.h[2] = mk_head(h.m_qf1, hQF1, &gQF1, u_l0[2], h.act, A, A);
    ha.h[3] = mk_head(h.m_qf2, hQF2, &gQF2, u_l0[3], h.act, A, A);
    ha.h[4] = mk_head(h.m_tgt, hTGT, nullptr, u_l0[4], nullptr, 0, 0);
    ha.h[5] = mk_head(h.m_qf1, hQF1PI, nullptr, u_l0[2], pi_a, A, A);
    ha.h[6] = mk_head(h.m_qf2, hQF2PI, nullptr, u_l0[3], pi_a, A, A);
    ha.B = B; ha.A = A; ha.eps = h.eps_buf; ha.pi_a = pi_a; ha.logp = logp; ha.ent = ent;
    ha.log_ent_coef = h.params + h.ent_off; ha.da_pi = da_pi; ha.dmu = dmu; ha.dls = dls; ha.ld_dm = ld_dm;
    ha.rew = h.rew; ha.done = h.done; ha.gamma = c.gamma;
    ha.d_out[1] = d_v; ha.d_out[2] = d_qf1; ha.d_out[3] = d_qf2; ha.d_out[4] = d_qf1pi; ha.ld_d = ld_d;
    if (sw.get(Sw::heads_stamps)) {     // in-kernel phase stamps (scripts/heads_stamps.py)
      ha.stamps = (unsigned long long*)wk.take(4 * 32 * 8);
      h.zero_once.push_back({ha.stamps, 4 * 32 * 8});
      h.dbg["heads_stamps"] = {(const float*)ha.stamps, 4 * 32 * 2};
    }
    // argument blocks: [0] the plain update, [1] / [2] updates of a prefetching multi-update call whose head launch
    // opens the update (Adam step size) and, from the second update on, advances the RNG counter
    HeadsFusedArgs hb = ha, hc = ha;
    hb.sc = hc.sc = h.sc; hb.tick = hc.tick = 1; hb.rng_advance = 0; hc.rng_advance = 1;
    const HeadsFusedArgs* d_ha = h.upload_vec(wk, std::vector<HeadsFusedArgs>{ha, hb, hc});
    const int nblk = (B + HT_RB - 1) / HT_RB;
    int wmax = 0;
    for (int l = 0; l < L; ++l) wmax = std::max(wmax, hid[l]);
    const bool wide = wmax > 64;            // two column blocks per wave (heads_mfma.h, W = 128)
    // the reference's shapes: layers [64, 64] (gripper_grasp.yaml) and [128, 128] (SAC_real_2m_buffer_128/config.yaml)
    // (the 128-wide fast form also splits its few-output stages over the waves: 2A <= 16)
    const bool fast = L == 2 && hid[0] == hid[1] && (hid[0] == 64 || (hid[0] == 128 && A <= 8)) && B % HT_RB == 0;
    const int shape = wide ? HEADS_FAST_128 : (fast ? HEADS_FAST_64 : HEADS_GENERAL_64);
    d_heads = d_ha; heads_shape = shape; heads_nblk = nblk;
    h.sac_kit.heads = (int)h.ops_grads.size();
    h.ops_grads.push_back(heads_op(0, nullptr));
    for (int v = 0; v < 2; ++v) h.sac_kit.heads_open[v] = heads_op(1 + v, nullptr);
    loss();
    if (cnn) heads_dfeat();
  }

  // route 2: row-local chains, one forward and one backward launch (heads_kernels.h)
  void heads_chains() {
    heads_l0();
    HeadsFwdArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.h[0] = mk_head(h.m_pi, hPI, nullptr, u_l0[0], nullptr, 0, 0);
    fa.h[1] = mk_head(h.m_vf, hVF, nullptr, u_l0[1], nullptr, 0, 0);
    fa.h[2] = mk_head(h.m_qf1, hQF1, nullptr, u_l0[2], h.act, A, A);
    fa.h[3] = mk_head(h.m_qf2, hQF2, nullptr, u_l0[3], h.act, A, A);
    fa.h[4] = mk_head(h.m_tgt, hTGT, nullptr, u_l0[4], nullptr, 0, 0);
    fa.h[5] = mk_head(h.m_qf1, hQF1PI, nullptr, u_l0[2], pi_a, A, A);
    fa.h[6] = mk_head(h.m_qf2, hQF2PI, nullptr, u_l0[3], pi_a, A, A);
    fa.B = B; fa.A = A; fa.eps = h.eps_buf; fa.pi_a = pi_a; fa.logp = logp; fa.ent = ent;
    {
      Op op; op.tag = "heads_fwd";
      op.run = [fa](hipStream_t s) { launch_heads_fwd(fa, s); };
      h.ops_grads.push_back(op);
    }
    loss();
    // g[l] = gradient w.r.t. the pre-activation of layer l (ReLU mask already applied)
    HeadsBwdArgs ba;
    memset(&ba, 0, sizeof(ba));
    ba.h[0] = mk_head(h.m_pi, hPI, &gPI, u_l0[0], nullptr, 0, 0);
    ba.h[1] = mk_head(h.m_vf, hVF, &gVF, u_l0[1], nullptr, 0, 0);
    ba.h[2] = mk_head(h.m_qf1, hQF1, &gQF1, u_l0[2], h.act, A, A);
    ba.h[3] = mk_head(h.m_qf2, hQF2, &gQF2, u_l0[3], h.act, A, A);
    ba.h[4] = mk_head(h.m_qf1, hQF1PI, &gQF1PI, u_l0[2], pi_a, A, A);
    ba.h[1].dout[0] = d_v; ba.h[2].dout[0] = d_qf1; ba.h[3].dout[0] = d_qf2; ba.h[4].dout[0] = d_qf1pi;
    for (int k = 1; k < 5; ++k) ba.h[k].ld_dout = ld_d;
    ba.ld_dm = ld_dm;
    ba.rew = h.rew; ba.done = h.done; ba.v_tgt = hTGT.out[0]; ba.qf1 = hQF1.out[0]; ba.qf2 = hQF2.out[0]; ba.v = hVF.out[0];
    ba.qf1_pi = hQF1PI.out[0]; ba.qf2_pi = hQF2PI.out[0]; ba.logp = logp; ba.gamma = c.gamma;
    ba.d_out[1] = d_v; ba.d_out[2] = d_qf1; ba.d_out[3] = d_qf2; ba.d_out[4] = d_qf1pi; ba.ld_d = ld_d;
    ba.B = B; ba.A = A; ba.mu = hPI.out[0]; ba.ls_raw = hPI.out[1]; ba.eps = h.eps_buf; ba.pi_a = pi_a;
    ba.log_ent_coef = h.params + h.ent_off; ba.da_pi = da_pi; ba.dmu = dmu; ba.dls = dls;
    {
      Op op; op.tag = "heads_bwd";
      op.run = [ba](hipStream_t s) { launch_heads_bwd(ba, s); };
      h.ops_grads.push_back(op);
    }
    if (cnn) heads_dfeat();
  }

  // route 3: one GEMM launch per layer and direction
  void heads_per_layer() {
    // heads forward: pi, vf, qf1, qf2 (data action), target vf
    for (int l = 0; l < L; ++l) {
      std::vector<IgemmProb> pr;
      pr.push_back(h.head_layer(h.m_pi, P, hPI, l, h.feat[0], ldf, F, nullptr, 0, 0, B));
      pr.push_back(h.head_layer(h.m_vf, P, hVF, l, h.feat[1], ldf, F, nullptr, 0, 0, B));
      pr.push_back(h.head_layer(h.m_qf1, P, hQF1, l, h.feat[1], ldf, F, h.act, A, A, B));
      pr.push_back(h.head_layer(h.m_qf2, P, hQF2, l, h.feat[1], ldf, F, h.act, A, A, B));
      pr.push_back(h.head_layer(h.m_tgt, P, hTGT, l, h.feat[2], ldf, F, nullptr, 0, 0, B));
      h.add_launch(h.ops_grads, "heads_fwd", 0, pr);
    }
    {
      std::vector<IgemmProb> pr;
      pr.push_back(h.head_out(h.m_pi, P, hPI, 0, B));
      pr.push_back(h.head_out(h.m_pi, P, hPI, 1, B));
      pr.push_back(h.head_out(h.m_vf, P, hVF, 0, B));
      pr.push_back(h.head_out(h.m_qf1, P, hQF1, 0, B));
      pr.push_back(h.head_out(h.m_qf2, P, hQF2, 0, B));
      pr.push_back(h.head_out(h.m_tgt, P, hTGT, 0, B));
      h.add_launch(h.ops_grads, "heads_fwd", 0, pr);
    }
    {
      SampleArgs sa{hPI.out[0], hPI.out[1], h.eps_buf, B, A, pi_a, nullptr, logp, ent};
      Op op; op.tag = "sample";
      op.run = [sa](hipStream_t s) {
        hipLaunchKernelGGL(sample_kernel, dim3((sa.B + 255) / 256), dim3(256), 0, s, sa);
      };
      h.ops_grads.push_back(op);
    }
    for (int l = 0; l < L; ++l) {
      std::vector<IgemmProb> pr;
      pr.push_back(h.head_layer(h.m_qf1, P, hQF1PI, l, h.feat[1], ldf, F, pi_a, A, A, B));
      pr.push_back(h.head_layer(h.m_qf2, P, hQF2PI, l, h.feat[1], ldf, F, pi_a, A, A, B));
      h.add_launch(h.ops_grads, "heads_fwd", 0, pr);
    }
    {
      std::vector<IgemmProb> pr;
      pr.push_back(h.head_out(h.m_qf1, P, hQF1PI, 0, B));
      pr.push_back(h.head_out(h.m_qf2, P, hQF2PI, 0, B));
      h.add_launch(h.ops_grads, "heads_fwd", 0, pr);
    }
    loss();
    // g[l] = gradient w.r.t. the pre-activation of layer l (ReLU mask already applied)
    {
      std::vector<IgemmProb> pr;   // output layer -> g[L-1]
      pr.push_back(h.dense_bwd({{d_v, 1, 1, P + h.m_vf.ow[0]}}, B, 0, hid[L - 1], gVF.g[L - 1], hid[L - 1], hVF.z[L - 1]));
      pr.push_back(h.dense_bwd({{d_qf1, 1, 1, P + h.m_qf1.ow[0]}}, B, 0, hid[L - 1], gQF1.g[L - 1], hid[L - 1], hQF1.z[L - 1]));
      pr.push_back(h.dense_bwd({{d_qf2, 1, 1, P + h.m_qf2.ow[0]}}, B, 0, hid[L - 1], gQF2.g[L - 1], hid[L - 1], hQF2.z[L - 1]));
      pr.push_back(h.dense_bwd({{d_qf1pi, 1, 1, P + h.m_qf1.ow[0]}}, B, 0, hid[L - 1], gQF1PI.g[L - 1], hid[L - 1], hQF1PI.z[L - 1]));
      h.add_launch(h.ops_grads, "heads_bwd", 1, pr);
    }
    for (int l = L - 1; l >= 1; --l) {
      std::vector<IgemmProb> pr;
      pr.push_back(h.dense_bwd({{gVF.g[l], hid[l], hid[l], P + h.m_vf.w[l]}}, B, 0, hid[l - 1], gVF.g[l - 1], hid[l - 1], hVF.z[l - 1]));
      pr.push_back(h.dense_bwd({{gQF1.g[l], hid[l], hid[l], P + h.m_qf1.w[l]}}, B, 0, hid[l - 1], gQF1.g[l - 1], hid[l - 1], hQF1.z[l - 1]));
      pr.push_back(h.dense_bwd({{gQF2.g[l], hid[l], hid[l], P + h.m_qf2.w[l]}}, B, 0, hid[l - 1], gQF2.g[l - 1], hid[l - 1], hQF2.z[l - 1]));
      pr.push_back(h.dense_bwd({{gQF1PI.g[l], hid[l], hid[l], P + h.m_qf1.w[l]}}, B, 0, hid[l - 1], gQF1PI.g[l - 1], hid[l - 1], hQF1PI.z[l - 1]));
      h.add_launch(h.ops_grads, "heads_bwd", 1, pr);
    }
    {
      std::vector<IgemmProb> pr;   // first layer: d a_pi (policy path) and d feat (critic CNN path)
      pr.push_back(h.dense_bwd({{gQF1PI.g[0], hid[0], hid[0], P + h.m_qf1.w[0]}}, B, F, A, da_pi, A, nullptr));
      if (cnn)
        pr.push_back(h.dense_bwd({{gVF.g[0], hid[0], hid[0], P + h.m_vf.w[0]},
                                {gQF1.g[0], hid[0], hid[0], P + h.m_qf1.w[0]},
                                {gQF2.g[0], hid[0], hid[0], P + h.m_qf2.w[0]}},
                               B, 0, Fc, dfeat[1], ldf, h.feat[1]));
      h.add_launch(h.ops_grads, "heads_bwd", 1, pr);
    }
    {
      SampleBwdArgs sb{hPI.out[0], hPI.out[1], h.eps_buf, pi_a, da_pi, A, h.params + h.ent_off, B, A, dmu, dls};
      Op op; op.tag = "sample_bwd";
      op.run = [sb](hipStream_t s) {
        hipLaunchKernelGGL(sample_bwd_kernel, dim3((sb.B + 255) / 256), dim3(256), 0, s, sb);
      };
      h.ops_grads.push_back(op);
    }
    {
      std::vector<IgemmProb> pr;
      pr.push_back(h.dense_bwd({{dmu, A, A, P + h.m_pi.ow[0]}, {dls, A, A, P + h.m_pi.ow[1]}}, B, 0, hid[L - 1],
                             gPI.g[L - 1], hid[L - 1], hPI.z[L - 1]));
      h.add_launch(h.ops_grads, "heads_bwd", 1, pr);
    }
    for (int l = L - 1; l >= 1; --l) {
      std::vector<IgemmProb> pr;
      pr.push_back(h.dense_bwd({{gPI.g[l], hid[l], hid[l], P + h.m_pi.w[l]}}, B, 0, hid[l - 1], gPI.g[l - 1], hid[l - 1], hPI.z[l - 1]));
      h.add_launch(h.ops_grads, "heads_bwd", 1, pr);
    }
    if (cnn) {
      std::vector<IgemmProb> pr;
      pr.push_back(h.dense_bwd({{gPI.g[0], hid[0], hid[0], P + h.m_pi.w[0]}}, B, 0, Fc, dfeat[0], ldf, h.feat[0]));
      h.add_launch(h.ops_grads, "heads_bwd", 1, pr);
    }
  }

  // =============================================================== the heads: forward, losses, backward down to d feat
  void heads() {
    if (fused_heads) {
      // heads_mfma.h: any layers up to 64 wide with 2A <= 64, and the shipped wide shape -- layers [128, 128], A <= 8,
      // whole 16-row blocks (the general form at that width runs out of registers: those stay on heads_kernels.h)
      heads_mfma = !sw.get(Sw::GRL_NO_HEADS_MFMA) && 2 * A <= 64;
      bool narrow = true;
      for (int l = 0; l < L; ++l) narrow = narrow && hid[l] <= 64;
      bool wide_ok = L == 2 && hid[0] == 128 && hid[1] == 128 && A <= 8 && B % HT_RB == 0;
      // the 128-wide kernel keeps 75 KB of static LDS per workgroup: fits gfx950's 160 KB; a device that offers less keeps the VALU chains
      if (!narrow && wide_ok && device_lds_bytes() < (int)heads_fused_lds_bytes(HEADS_FAST_128)) wide_ok = false;
      heads_mfma = heads_mfma && (narrow || wide_ok);
    }
    if (heads_mfma) heads_one_launch();
    else if (fused_heads) heads_chains();
    else heads_per_layer();
  }

  // =============================================================== backward through the two CNNs: the problems of fc_bwd /
  // conv3_bwd / conv2_bwd (launched by weight_gradients(), once their fillers are known)
  void backward_data() {
    if (!cnn) return;
    // Measured and rejected on top of the merged weight-gradient launch (MI355X, B = 256, updates/s; conv2_bwd needs 46 KB of
    // LDS, so a CU holds three of its 1024 tiles and the launch runs as a wave of 768 plus a third-full wave of 256):
    //  * every weight gradient except conv1's riding on conv2_bwd's launch, longest tiles first, conv1 (the only consumer
    //    of conv2_bwd's result) as a launch of its own: the pair launch takes 57.7 us against 31.8 + 36.5, but conv1 alone
    //    costs 13.2 us (one short tile per CU) and its 225 slabs another 8 us of reduction: 4 395 against 4 600;
    //  * only the dense layers' weight gradients (303 tiles of 8 slabs, the length of a conv2_bwd tile) riding behind
    //    conv2_bwd's tiles: they start when the first wave drains (18 us) and end at 36 us instead of 28: conv2_bwd
    //    31.8 -> 41.2 us, the weight-gradient launch 36.6 -> 28.2 us, reduction +2.5 us: 4 519 against 4 580.
    // backward-data with exact taps (conv_bwd_tabs_exact; the masked parity-class form of conv_bwd_tabs gives bit-identical
    // sums with 1.8-2.25x the MACs -- the auto-encoder's padded convolutions still use it)
    std::vector<int32_t> untouched;
    std::vector<ConvBwdClass> bc3 = h.conv_bwd_tabs_exact(cg[2], B, nullptr);
    std::vector<ConvBwdClass> bc2 = h.conv_bwd_tabs_exact(cg[1], B, &untouched);
    if (!untouched.empty())   // input pixels of conv2 that no output window covers (row / column 14): their gradient is zero
      for (int n = 0; n < 2; ++n) h.zero_once.push_back({g1[n], (size_t)(((int64_t)B * geo.p1 - 1) * ld1 + 32) * 4});
    for (int n = 0; n < 2; ++n)
      bwd_pr[0].push_back(h.dense_bwd({{dfeat[n], ldf, 512, P + h.ex[n].fw}}, B, 0, geo.K, g3[n], geo.K, a3[n]));
    for (int n = 0; n < 2; ++n)
      for (auto& cl : bc3) bwd_pr[1].push_back(h.conv_bwd(g3[n], cl, cg[2], P + h.ex[n].w[2], g2[n], a2[n]));
    for (int n = 0; n < 2; ++n)
      for (auto& cl : bc2) bwd_pr[2].push_back(h.conv_bwd(g2[n], cl, cg[1], P + h.ex[n].w[1], g1[n], a1[n]));
    // conv / fc weight gradients (split reductions land in slabs, summed by reduce_slabs)
    // conv3_bwd (576 tiles of the 32x64 shape at B = 256, three per CU) fills two dispatch rounds and a quarter of the third:
    // 192 CUs hold two tiles, 64 hold three, and the launch lasts as long as those 64.  Dense-layer weight gradients
    // whose operands are complete by then (d feat, head gradients) and whose tiles are as long as conv3_bwd's (reduction
    // = the batch, 8 slabs) ride in the empty slots of that round -- list positions 576.. land exactly on the CUs that
    // hold two -- and leave the merged weight-gradient launch.
    // backward-data of conv3 and conv2 as ONE sample-local launch (conv_stack.h: conv_stack_bwd_kernel, scatter form with the
    // forward's MACs) -- OPT-IN, GRL_TUNE conv_stack_bwd=1.  Measured on the MI355X at B = 256 (same box, scripts/ab_env.sh):
    // first cut 5 660 against 5 689 updates/s; with the masks prefetched, wave-local epilogues, batched LDS read-modify-writes
    // and falling issue priority 5 741 - 5 762 against 5 755 - 5 757: NEUTRAL.  The launch itself (33 - 35 us) replaces 17.0 +
    // 20.3 us, but the dense weight gradients that ride in conv3_bwd's empty slots go back into the weight-gradient launch
    // (30.5 -> 35 us), and the conv3 half is bound by its kernel stream: 16 output pixels per sample reuse every 4 KB of
    // kernel for 16 MFMAs, where the batched exact-tap launch reuses it over 128 rows (profiles/r05_ab_conv_stack_bwd.txt)
    conv_stack_bwd = conv_stack && sw.get(Sw::conv_stack_bwd) != 0;
    if (!conv_stack_bwd) {
      int cfg3 = -1;
      const int t3 = h.planned_tiles(bwd_pr[1], 1, "conv3_bwd", &cfg3);
      rider_budget = cfg3 == 3 ? h.free_slots(t3, 3) : 0;
    }
  }

  // conv / fc weight gradients of the two trained CNNs (split reductions land in slabs, summed by reduce_slabs)
  void conv_wgrad_problems() {
    int wsplit[3] = {72, 12, 6};   // reduction splits of conv1..3 (GRL_TUNE wg_split=a/b/c overrides the model's choice)
    h.pick_wgrad_splits(cg, ft, 2, wsplit, rider_budget);
    sw.get3(Sw::wg_split, wsplit);
    {   // conv1 of both networks: one problem over the side-by-side gradient buffer, columns 32n.. -> net n
      IgemmProb p = h.conv_wgrad(h.x_obs, ft[0], cg[0], g1[0], nullptr, wsplit[0], 2);
      p.c = wk.f32(p.slab_stride * p.split);
      wgc[0].push_back(p);
      for (int n = 0; n < 2; ++n) {
        ReduceDesc r;
        memset(&r, 0, sizeof(r));
        r.src = p.c + 32 * n; r.splits = p.split; r.slab_stride = p.slab_stride; r.row_len = 32; r.src_ld = 64;
        r.dst = h.grads + h.ex[n].w[0]; r.n = cg[0].K() * 32;
        h.reduces.push_back(r);
        ReduceDesc rb = r;
        rb.src = p.c + (int64_t)p.p_ones_i * 64 + 32 * n; rb.dst = h.grads + h.ex[n].b[0]; rb.n = 32;
        h.reduces.push_back(rb);
      }
    }
    for (int n = 0; n < 2; ++n) {
      {
        IgemmProb p = h.conv_wgrad(a1[n], ft[1], cg[1], g2[n], nullptr, wsplit[1]);
        p.c = wk.f32(p.slab_stride * p.split);
        h.add_wgrad(wgc[1], p, h.ex[n].w[1], 0, cg[1].K(), h.ex[n].b[1]);
      }
      {
        IgemmProb p = h.conv_wgrad(a2[n], ft[2], cg[2], g3[n], nullptr, wsplit[2]);
        p.c = wk.f32(p.slab_stride * p.split);
        h.add_wgrad(wgc[2], p, h.ex[n].w[2], 0, cg[2].K(), h.ex[n].b[2]);
      }
      {
        IgemmProb p = h.dense_wgrad(a3[n], geo.K, geo.K, true, dfeat[n], ldf, 512, B, nullptr, 1);
        p.c = wk.f32(p.slab_stride * p.split);
        h.add_wgrad(wg, p, h.ex[n].fw, 0, geo.K, h.ex[n].fb);
      }
    }
  }

  // head weight gradients.  Fused-heads layout: every operand is row-padded to a multiple of 4 floats, and
  // problems without a bias still carry the ones row (its slab row is simply not reduced), so that all
  // dense weight gradients form ONE uniform launch of the vectorised kernel.
  void head_wgrads(const MlpP& m, const HeadAct& ha, const HeadGrad& g, const float* x0, int ld0, int K0, const float* x1, int ld1, int K1,
                   std::vector<const float*> douts, int ld_dout) {
    const int K0p = ld0 >= (int)rup(K0, 4) ? (int)rup(K0, 4) : K0;   // feat rows are padded to ldf (zeros)
    const int K1p = (K1 > 0 && ld1 >= (int)rup(K1, 4)) ? (int)rup(K1, 4) : K1;
    for (int l = 0; l < L; ++l) {
      if (l == 0) {
        if (K1 > 0) {
          IgemmProb p0 = h.dense_wgrad(x0, ld0, K0, fused_heads, g.g[0], g.ld0, hid[0], B, nullptr, 1, K0p);
          p0.c = wk.f32(p0.slab_stride * p0.split);
          h.add_wgrad(wg, p0, m.w[0], 0, K0, -1);
          IgemmProb p1 = h.dense_wgrad(x1, ld1, K1, true, g.g[0], g.ld0, hid[0], B, nullptr, 1, K1p);
          p1.c = wk.f32(p1.slab_stride * p1.split);
          h.add_wgrad(wg, p1, m.w[0], K0, K1, m.b[0]);
        } else {
          IgemmProb p0 = h.dense_wgrad(x0, ld0, K0, true, g.g[0], g.ld0, hid[0], B, nullptr, 1, K0p);
          p0.c = wk.f32(p0.slab_stride * p0.split);
          h.add_wgrad(wg, p0, m.w[0], 0, K0, m.b[0]);
        }
      } else {
        IgemmProb p = h.dense_wgrad(ha.z[l - 1], hid[l - 1], hid[l - 1], true, g.g[l], hid[l], hid[l], B, nullptr, 1);
        p.c = wk.f32(p.slab_stride * p.split);
        h.add_wgrad(wg, p, m.w[l], 0, hid[l - 1], m.b[l]);
      }
    }
    for (int k = 0; k < m.n_out; ++k) {
      IgemmProb p = h.dense_wgrad(ha.z[L - 1], hid[L - 1], hid[L - 1], true, douts[k], ld_dout, m.out_dim, B, nullptr, 1);
      p.c = wk.f32(p.slab_stride * p.split);
      h.add_wgrad(wg, p, m.ow[k], 0, hid[L - 1], m.ob[k]);
    }
  }

  // =============================================================== weight gradients, the riders on conv3_bwd, and the launches of the
  // backward half in their final order
  void weight_gradients() {
    if (cnn) conv_wgrad_problems();
    const float* act_w = fused_heads ? act_p : h.act;
    const int ld_act_w = fused_heads ? Ap : A;
    head_wgrads(h.m_pi, hPI, gPI, h.feat[0], ldf, F, nullptr, 0, 0, {dmu, dls}, ld_dm);
    head_wgrads(h.m_vf, hVF, gVF, h.feat[1], ldf, F, nullptr, 0, 0, {d_v}, ld_d);
    head_wgrads(h.m_qf1, hQF1, gQF1, h.feat[1], ldf, F, act_w, ld_act_w, A, {d_qf1}, ld_d);
    head_wgrads(h.m_qf2, hQF2, gQF2, h.feat[1], ldf, F, act_w, ld_act_w, A, {d_qf2}, ld_d);
    // the vectorised kernel needs uniform launches: with / without bias row; whatever it cannot take
    // goes to igemm_kernel.  (Fused heads: everything lands in the first group.)
    std::vector<IgemmProb> wg_ones, wg_plain, wg_rest;
    for (auto& p : wg) {
      if (!h.v2_prob_ok(p, 2) || (p.K % 4)) wg_rest.push_back(p);
      else if (p.p_ones_i >= 0) wg_ones.push_back(p);
      else wg_plain.push_back(p);
    }
    // One launch for all weight gradients: the dense problems (x^T read with affine addresses) are re-expressed
    // with the table addressing of the convolution ones and appended to that launch -- one kernel boundary
    // less, and their short reductions (K = B) fill the tail of the long convolution tiles.
    dense_affine = wg_ones;                                   // (kept for the staged data-parallel plan below)
    for (int l = 2; l >= 0; --l) conv_all.insert(conv_all.end(), wgc[l].begin(), wgc[l].end());
    only_vec_dense = wg_plain.empty() && wg_rest.empty();
    std::vector<IgemmProb> wg_merged;
    if (cnn && wg_plain.empty() && !wgc[0].empty() && h.v2_prob_ok(wgc[0][0], 2)) {
      for (auto p : wg_ones) {
        std::vector<int32_t> ti(p.M), tr(p.K);
        for (int i = 0; i < p.M; ++i) ti[i] = i * p.p_ld_i[0];
        for (int r = 0; r < p.K; ++r) tr[r] = r * p.p_ld_r[0];
        p.p_tab_i = h.upload_vec(wk, ti);
        p.p_tab_r = h.upload_vec(wk, tr);
        p.vflags |= VF_P_TABS;                    // v2_prob_ok held for the affine form: unit stride along i, ld_r % 4 == 0
        wg_merged.push_back(p);
      }
      wg_ones.clear();
    }
    // the problems of a launch with VF_C_DRAIN set where GRL_TUNE store_drain names their group (outputs that a later launch
    // reads; the staged data-parallel plan keeps its own, plain copies)
    auto drained = [&](std::vector<IgemmProb> pr, int group) {
      if (store_drain & group)
        for (auto& p : pr)
          if (!p.accumulate) p.vflags |= VF_C_DRAIN;
      return pr;
    };
    // The launches, planned in this order (tables, plan notes) and scheduled directly behind the last producer of their operands:
    // dense weight gradients behind the heads | backward-data | the merged weight-gradient launch
    std::vector<Op> bwd, dense, merged;
    int conv3_at = -1;
    if (cnn) h.add_launch(bwd, "fc_bwd", 1, bwd_pr[0]);
    if (cnn && conv_stack_bwd) {
      ConvStackBwdArgs ba;
      memset(&ba, 0, sizeof(ba));
      for (int n = 0; n < 2; ++n) {
        ConvStackBwdNet& bn = ba.nets[n];
        bn.g3 = g3[n]; bn.a2 = a2[n]; bn.a1 = a1[n]; bn.w2 = P + h.ex[n].w[1]; bn.w3 = P + h.ex[n].w[2];
        bn.g2 = g2[n]; bn.g1 = g1[n]; bn.ld1 = ld1;
      }
      ba.B = B; ba.n_nets = 2;
      Op op; op.tag = "conv_stack_bwd";
      op.flops = op.flops_exec = 2.0 * B * 2 * ((double)geo.p2 * 64 * 512 + (double)geo.p3 * 64 * 576);
      op.run = [ba](hipStream_t s) { launch_conv_stack_bwd(ba, s); };
      bwd.push_back(op);
    } else if (cnn) {
      std::vector<IgemmProb> riders = h.take_riders(wg_merged, rider_budget);
      if (!riders.empty()) h.add_launch(conv3_bwd_plain, "conv3_bwd", 1, bwd_pr[1]);
      conv3_at = (int)bwd.size();
      h.add_launch(bwd, "conv3_bwd", 1, drained(bwd_pr[1], SD_G12), "wgrad_dense", 2, drained(riders, SD_SLABS));
      conv3_n = (int)bwd.size() - conv3_at;
      h.add_launch(bwd, "conv2_bwd", 1, drained(bwd_pr[2], SD_G12));
    }
    h.add_launch(dense, "wgrad_dense", 2, wg_ones);
    h.add_launch(dense, "wgrad_dense", 2, wg_plain);
    h.add_launch(dense, "wgrad_small", 2, wg_rest);
    std::vector<IgemmProb> all;
    for (int l = 2; l >= 0; --l) all.insert(all.end(), wgc[l].begin(), wgc[l].end());
    all.insert(all.end(), wg_merged.begin(), wg_merged.end());
    if (cnn) all = drained(all, SD_SLABS);
    h.add_launch(merged, "wgrad_conv", 2, all);
    std::vector<Op>& G = h.ops_grads;
    G.insert(G.end(), dense.begin(), dense.end());
    bwd_begin = (int)G.size();
    G.insert(G.end(), bwd.begin(), bwd.end());
    bwd_end = (int)G.size();
    if (conv3_at >= 0) conv3 = bwd_begin + conv3_at;
    if (merged.size() == 1) h.sac_kit.wgrad_conv = (int)G.size();
    G.insert(G.end(), merged.begin(), merged.end());
    if (x_obs_b && h.sac_kit.wgrad_conv >= 0) {      // the same launch reading conv1's input from the second image buffer (flavour 1 of "gather_ride")
      bool patched = false;
      for (auto& p : all)
        if (p.p_base[0] == h.x_obs) { p.p_base[0] = x_obs_b; patched = true; }
      std::vector<Op> tmp;
      if (patched) h.add_launch(tmp, "wgrad_conv", 2, all);
      if (tmp.size() == 1) { h.sac_kit.wgrad_conv_b = tmp[0]; have_wgrad_conv_b = true; }
    }
  }

  // =============================================================== staged gradient computation (data parallel): the dense weight
  // gradients -- 90 % of the bucket's bytes -- get a launch of their own right after the feature gradients, so that their
  // all-reduce can travel while the convolution backward and the convolution weight gradients run (grasp_rl/parallel.py).
  // Costs two launches more than the single-exchange plan; same tiles, same arithmetic.  (The two reductions follow below.)
  void staged_split() {
    const std::vector<Op>& G = h.ops_grads;
    const int cut = h.sac_kit.dfeat;
    h.staged_ok = cnn && fused_heads && only_vec_dense && !dense_affine.empty() && !conv_all.empty() && cut >= 0;
    if (!h.staged_ok) return;
    h.ops_stage0.assign(G.begin(), G.begin() + cut + 1);
    h.add_launch(h.ops_stage0, "wgrad_dense", 2, dense_affine, "", 0, {}, 0);
    for (int k = bwd_begin; k < bwd_end; ++k) {
      if (k == conv3 && !conv3_bwd_plain.empty()) {      // (riders belong to stage 0 here)
        h.ops_stage1.insert(h.ops_stage1.end(), conv3_bwd_plain.begin(), conv3_bwd_plain.end());
        k += conv3_n - 1;
      } else {
        h.ops_stage1.push_back(G[k]);
      }
    }
    h.add_launch(h.ops_stage1, "wgrad_conv", 2, conv_all, "", 0, {}, 0);
  }

  // the slab reduction over `n` tiles (+ the loss workgroup), optionally applying Adam + Polyak where the sums are formed
  Op reduce_op(const char* tag, const int2* tiles, int n, int loss, int apply) const {
    return grl_ctx::reduce_op(tag, dr, tiles, n, h.loss_args, loss, aa, apply);
  }

  // =============================================================== reductions: the one that ends the gradient computation (the
  // recorded closing slot) and those of the two stages
  void reductions() {
    std::vector<int2> rt = h.reduce_tiles();          // (marks the 16-byte-eligible descriptors: before the upload)
    dr = h.d_reduces = h.upload_vec(wk, h.reduces);
    d_rt = h.upload_vec(wk, rt);
    ntiles = (int)rt.size();
    has_loss = fused_heads ? 1 : 0;
    aa = h.adam_base = h.adam_args(1.f, true);
    Op op = reduce_op("reduce_slabs", d_rt, ntiles, has_loss, 0);
    op.join = true;
    h.sac_kit.close = (int)h.ops_grads.size();
    h.ops_grads.push_back(op);
    h.red_all.tiles = d_rt; h.red_all.n = ntiles; h.red_all.has_loss = has_loss;
    if (!h.staged_ok) return;
    // reductions of the two stages: convolution descriptors are those that land in the conv variables of a net
    auto is_conv = [&](const ReduceDesc& r) {
      for (int n = 0; n < 2; ++n)
        if (r.dst >= h.grads + h.ex[n].w[0] && r.dst < h.grads + h.ex[n].fw) return true;
      return false;
    };
    std::vector<int2> rt0 = h.reduce_tiles([&](const ReduceDesc& r) { return !is_conv(r); });
    std::vector<int2> rt1 = h.reduce_tiles(is_conv);
    h.red_dense.tiles = h.upload_vec(wk, rt0); h.red_dense.n = (int)rt0.size(); h.red_dense.has_loss = 0;
    h.red_conv.tiles = h.upload_vec(wk, rt1); h.red_conv.n = (int)rt1.size(); h.red_conv.has_loss = has_loss;
    h.ops_stage0.push_back(reduce_op("reduce_dense", h.red_dense.tiles, h.red_dense.n, 0, 0));
    h.ops_stage1.push_back(reduce_op("reduce_conv", h.red_conv.tiles, h.red_conv.n, has_loss, 0));
  }

  // reduction + Adam closing a first / middle update of a call, carrying riders `g` (gather of the next update, gx workgroups per row)
  Op reduce_ride_op(const LossArgs& lk, const AdamArgs& aq, const GatherArgs& g, int rgx, double bytes) const {
    Op op; op.tag = "reduce_adam";
    op.join = true;
    op.bytes = bytes;
    const ReduceDesc* d = dr;
    const int2* tiles = d_rt;
    const int n = ntiles, loss = has_loss;
    op.run = [d, tiles, n, lk, loss, aq, g, rgx](hipStream_t s) { launch_reduce_slabs_gather(d, tiles, n, lk, loss, aq, g, rgx, s); };
    return op;
  }

  // =============================================================== call plans: the fused update and the calls of several updates
  int call_plans() {
    // Full updates (no gradient exchange in between): every trainable element is the sum of one slab
    // column, so Adam + Polyak are applied where the sum is formed -- one launch and one pass over the
    // gradient bucket less.  log_ent_coef, whose gradient comes from the loss workgroup, is applied there.
    if (!has_loss || !sw.get(Sw::fused_adam)) return GRL_OK;
    SacKit& kit = h.sac_kit;
    h.ops_grads_apply.assign(h.ops_grads.begin(), h.ops_grads.begin() + kit.close);
    Op fo = reduce_op("reduce_adam", d_rt, ntiles, has_loss, 1);
    fo.join = true;
    fo.bytes = (double)h.n_train * 4 * 7 + (double)h.n_polyak * 4 * 2;
    h.ops_grads_apply.push_back(fo);
    // ---- "prefetch": a call of n >= 2 updates on the device RNG gathers the minibatch of update t+1 inside the LAST
    // launch of update t (reduce_slabs_gather_kernel): nothing enters the replay between the updates of one call, the
    // Philox counter makes the draw independent of when it happens, and every reader of update t's minibatch tensors
    // has finished when that launch starts.  Same kernels, same arithmetic, one launch (and one dependent latency
    // chain) less per update.  The head launch opens the update instead of the gather (see HeadsFusedArgs).
    //   first : gather (does not touch the Adam step size) | body, heads[tick] | reduce + Adam + gather(t+1, counter + 1)
    //   middle:                                              body, heads[tick, counter += 1] | reduce + Adam + gather(t+1)
    //   last  :                                              body, heads[tick, counter += 1] | reduce + Adam (counter += 1)
    if (!heads_mfma || !sw.get(Sw::gather_prefetch)) return GRL_OK;
    const double gather_bytes = h.ops_rng[0].bytes;
    GatherArgs g1 = ga0;
    g1.use_rng = 1; g1.adam_tick = 0; g1.quiet = 0; g1.rng_ahead = 0;
    kit.gather[0] = gather_op(g1, gx, gather_bytes);
    SacKit::Riders& pre = kit.riders[0];       // (the data-parallel update builds its own closing launches from these at connect)
    pre.g2 = g1;
    pre.g2.quiet = 1; pre.g2.rng_ahead = 1;
    pre.lk = h.loss_args;
    pre.lk.keep_rng = 1;
    pre.gx = gx;
    AdamArgs aq = aa;
    aq.skip_bucket = 1;                 // (the call's last update -- `fo` -- leaves its gradients in the bucket)
    const double ride_bytes = fo.bytes - (double)h.n_train * 4;
    const Op ro = reduce_ride_op(pre.lk, aq, pre.g2, pre.gx, ride_bytes + gather_bytes);
    sac_call_plan(h, h.pf, false, [&](int v) { return std::vector<Op>{v == 2 ? fo : ro}; });
    h.pf.short_call_graph = true;
    // ---- "gather_ride": the IMAGES of update t+1 gathered by extra workgroups of update t's HEAD launch -- 64 workgroups of
    // row-local chains on 256 CUs for 16 us -- instead of the reduction launch, which is memory bound itself.  What the
    // gather writes and update t still reads after its head launch: x_obs (conv1's weight gradient, in the last GEMM launch)
    // -- double buffered, flavour f reads buffer f and gathers into the other; x_next (read by the forward stack only) needs
    // no second copy; the per-row extras (direct features, action, reward, done, index, noise: read by the head launch and
    // the dense weight gradients) stay with the reduction launch that ends the update, as a gather of parts = 2.  Counters:
    // the riders draw with DevScalars.rng_img (the head launch itself advances rng_step), which the call's first gather
    // sets and every riding reduction advances.
    //   first : gather[rng_img = c + 1] | body(A), heads[tick; images(t+1) -> B] | reduce + Adam + extras(t+1) [rng_img += 1]
    //   middle: body(f), heads[tick, counter += 1; images(t+1) -> other] | reduce + Adam + extras(t+1) [rng_img += 1]
    //   last  : body(f), heads[tick, counter += 1]                        | reduce + Adam (counter += 1)
    // (the emulation build has no 16-byte form: its riders walk the rows element by element)
    if (cnn && hw != 64 && x_obs_b) plan_note("grl plan: gather_ride  off for %dx%d images (it needs the forward stack's slot): multi-update calls run the prefetch form\n", hw, hw);
    if (!x_obs_b || kit.stack < 0 || !have_wgrad_conv_b || conv_stack_bwd || !(pre.g2.vec4 || !elem_vec4_built()) || B % GATHER_RIDE_ROWS != 0) return GRL_OK;
    int ride_rows = sw.get(Sw::ride_rows);
    if (!gather_ride_rows_built(ride_rows)) ride_rows = GATHER_RIDE_ROWS;
    if (!gather_ride_rows_built(ride_rows)) return fail(GRL_ERR_INVALID, "gather_ride: no kernel for this many rows per rider workgroup");
    kit.stack_b = stack_fwd_op(x_obs_b);
    SacKit::Riders& rid = kit.riders[1];
    rid.g2 = pre.g2;                            // extras of update t+1, carried by update t's reduction launch
    rid.g2.parts = 2;
    rid.lk = pre.lk;
    rid.lk.bump_img = 1;
    rid.gx = 1;
    const Op rx = reduce_ride_op(rid.lk, aq, rid.g2, rid.gx, ride_bytes);
    GatherArgs g0 = g1;                       // the call's own gather, leaving rng_img behind
    g0.set_img = 1;
    kit.gather[1] = gather_op(g0, gx, gather_bytes);
    for (int f = 0; f < 2; ++f) {
      GatherArgs gi = pre.g2;                  // images of update t+1 into the buffer flavour f does NOT read
      gi.parts = 1; gi.img_ctr = 1; gi.rng_ahead = 0; gi.quiet = 1;
      gi.rows = ride_rows;
      gi.drain = (store_drain & SD_IMAGES) != 0 && !gi.x_obs2;
      gi.x_obs = f ? h.x_obs : x_obs_b;
      for (int v = 0; v < 2; ++v) kit.heads_ride[f][v] = heads_op(1 + v, &gi);
    }
    sac_call_plan(h, h.ride, true, [&](int v) { return std::vector<Op>{v == 2 ? fo : rx}; });
    h.ride.short_call_graph = true;
    plan_note("grl plan: gather_ride  %d image-gather workgroups of the next update ride on the head launch (%d tiles per row, %d rows each); extras on the reduction launch\n",
              gx * (2 * B / ride_rows), gx, ride_rows);
    return GRL_OK;
  }

  // =============================================================== apply (a launch of its own: split API, exchanged gradients)
  void apply() {
    Op op = h.adam_op("adam_polyak", 1e-8f, true, true);
    op.bytes = (double)h.n_train * 4 * 7 + (double)h.n_polyak * 4 * 2;
    h.ops_apply.push_back(op);
  }

  // =============================================================== act path (batch NA, pi net only)
  int act_path() {
    float* const ax = cnn ? wk.f32((int64_t)NA * img_elems) : nullptr;
    h.afeat = wk.f32((int64_t)NA * ldf);
    // noise in, actions out: page-locked HOST memory that the last launch of the act path reads and writes itself -- 320 bytes
    // each way for 16 environments, for which a copy-engine transfer in the stream costs more than the whole policy head
    if (!h.dry) {    // (grl_query_sizes plans without a device)
      if (h.act_io_host.reserve((size_t)2 * NA * A) != hipSuccess) return fail(GRL_ERR_HIP, "hipHostMalloc failed");
      // (GRL_TUNE act_poll=0 keeps the stream synchronisation at the end of grl_act; so does a counter that cannot be allocated)
      if (sw.get(Sw::act_poll) != 0) (void)h.act_done_host.reserve(16, hipHostMallocCoherent);
    }
    h.a_eps = h.act_io_host.get();
    h.a_out = h.a_eps + (size_t)NA * A;
    HeadAct ahPI{};
    h.alloc_head(ahPI, NA, 2, A);
    ActIngestArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.obs = h.stg_obs; ia.n = NA; ia.hw = hw * hw; ia.c_obs = c.obs_channels; ia.c_img = C_img; ia.n_direct = nd;
    ia.vec_dim = cnn ? 0 : c.obs_dim; ia.scale_div = cnn ? 255.f : 1.f;
    ia.x = cnn ? ax : h.afeat; ia.ldx = cnn ? img_elems : ldf; ia.d = h.afeat + 512; ia.ldd = ldf;
    ActIngestArgs ian = ia;
    ian.normalize = 1; ian.clip_obs = c.clip_obs;
    ian.mean = h.s_mean; ian.stdv = h.s_std; ian.dmean = h.s_dmean; ian.dstd = h.s_dstd;
    {   // entry launch: [observed by grl_observe | handed to grl_act] x [raw: VecNormalize applied here | already normalised]
      const int elems = cnn ? img_elems : c.obs_dim;
      for (int v = 0; v < 4; ++v) {
        ActIngestArgs iv = (v & 1) ? ian : ia;
        if (v & 2) iv.obs = h.ob_latest;
        Op op; op.tag = "act_ingest";
        op.run = [iv, elems](hipStream_t s) {
          hipLaunchKernelGGL(act_ingest_kernel, dim3((elems + 255) / 256, iv.n), dim3(256), 0, s, iv);
        };
        h.ops_act_in[v].push_back(op);
      }
    }
    // the policy head on the matrix cores (act_mfma.h) for the shapes it covers (GRL_TUNE act_mfma=0: the VALU kernel): the
    // extractor's dense layer then runs as a split-K GEMM whose partial sums the head kernel adds up while it stages its input
    const bool mfma_heads = act_mfma_built() && am_shape_ok(F, L, hid, A) && sw.get(Sw::act_mfma) != 0;
    float* fc_parts = nullptr;
    int fc_split = 0;
    if (cnn) {
      float* const aa1 = wk.f32((int64_t)NA * geo.p1 * 32);
      float* const aa2 = wk.f32((int64_t)NA * geo.p2 * 64);
      float* const aa3 = wk.f32((int64_t)NA * geo.p3 * 64);
      float* io[4] = {ax, aa1, aa2, aa3};
      if (conv_stack) {     // one workgroup per observation walks conv1 -> conv2 -> conv3 (round 4: three launches, 4.9 + 9.2 + 9.2 us)
        ConvStackArgs ca;
        memset(&ca, 0, sizeof(ca));
        ca.nets[0].x = ax;
        for (int l = 0; l < 3; ++l) { ca.nets[0].w[l] = P + h.ex[0].w[l]; ca.nets[0].b[l] = P + h.ex[0].b[l]; }
        ca.nets[0].a3 = aa3;
        ca.B = NA; ca.n_nets = 1;
        const int Ci = C_img;
        Op op; op.tag = "act_conv";
        op.run = [ca, Ci](hipStream_t s) { launch_conv_stack_fwd(Ci, ca, s); };
        h.ops_act.push_back(op);
      } else {
        for (int l = 0; l < 3; ++l) {
          ConvGeom ag = cg[l];
          ag.ldx = ag.ldy = 0;                      // the acting pass keeps dense buffers of its own
          ConvFwdTabs t = h.conv_fwd_tabs(ag, NA);
          h.add_launch(h.ops_act, "act_conv", 0, {h.conv_fwd(io[l], t, ag, P + h.ex[0].w[l], P + h.ex[0].b[l], io[l + 1], ACT_RELU, 0.f)});
        }
      }
      if (mfma_heads) {
        IgemmProb p = h.dense_fwd(aa3, geo.K, geo.K, nullptr, 0, 0, NA, P + h.ex[0].fw, 512, nullptr, nullptr, 512, ACT_NONE);
        h.set_split(p, AM_MAXP);       // one tile walking 32 slabs (13.6 us for 16 rows) -> 4 x the tiles, 8 slabs each
        fc_split = p.split;
        fc_parts = wk.f32((int64_t)NA * 512 * p.split);
        p.c = fc_parts;
        h.add_launch(h.ops_act, "act_fc", 0, {p});
      } else {
        h.add_launch(h.ops_act, "act_fc", 0,
                   {h.dense_fwd(aa3, geo.K, geo.K, nullptr, 0, 0, NA, P + h.ex[0].fw, 512, P + h.ex[0].fb, h.afeat, ldf, ACT_RELU)});
      }
    }
    // the policy head: one launch (act_heads_kernel) for layer widths it covers, else a launch per layer + the output launch.
    // Two variants (deterministic / sampled) so that each is a static graph.
    bool one_launch = F <= ACT_HEADS_MAX_IN && A <= 64;
    for (int l = 0; l < L; ++l) one_launch = one_launch && hid[l] <= ACT_HEADS_MAX_HID;
    for (int det = 0; det < 2; ++det) {
      std::vector<Op>& tail = det ? h.ops_act_det : h.ops_act_sto;
      if (one_launch) {
        ActHeadsArgs ha;
        memset(&ha, 0, sizeof(ha));
        ha.x = h.afeat; ha.ldx = ldf; ha.K0 = F; ha.L = L;
        for (int l = 0; l < L; ++l) { ha.w[l] = P + h.m_pi.w[l]; ha.b[l] = P + h.m_pi.b[l]; ha.hid[l] = hid[l]; }
        for (int k = 0; k < 2; ++k) { ha.ow[k] = P + h.m_pi.ow[k]; ha.ob[k] = P + h.m_pi.ob[k]; }
        ha.A = A; ha.eps = h.a_eps; ha.mu = ahPI.out[0]; ha.ls = ahPI.out[1]; ha.out = h.a_out; ha.rows = NA; ha.deterministic = det;
        Op op; op.tag = "act_heads";
        if (mfma_heads) {
          if (fc_split > 0) {
            ha.x_parts = fc_parts; ha.n_parts = fc_split; ha.part_stride = (long)NA * 512; ha.ld_parts = 512;
            ha.x_bias = P + h.ex[0].fb; ha.n_sum = 512;
          }
          ha.done = h.act_done_host.get();
          h.act_done_wgs = h.act_done_host.get() ? (unsigned)((NA + HT_RB - 1) / HT_RB) : 0u;
          op.run = [ha](hipStream_t s) { launch_act_heads_mfma(ha, s); };
        } else {
          op.run = [ha](hipStream_t s) { hipLaunchKernelGGL(act_heads_kernel, dim3(ha.rows), dim3(256), 0, s, ha); };
        }
        tail.push_back(op);
        continue;
      }
      for (int l = 0; l < L; ++l)
        h.add_launch(tail, "act_head", 0, {h.head_layer(h.m_pi, P, ahPI, l, h.afeat, ldf, F, nullptr, 0, 0, NA)});
      h.add_launch(tail, "act_head", 0, {h.head_out(h.m_pi, P, ahPI, 0, NA), h.head_out(h.m_pi, P, ahPI, 1, NA)});
      const float* mu = ahPI.out[0]; const float* ls = ahPI.out[1]; const float* ep = h.a_eps; float* ao = h.a_out;
      const int rows = NA, Ad = A;
      Op op; op.tag = "act_out";
      op.run = [mu, ls, ep, ao, rows, Ad, det](hipStream_t s) {
        hipLaunchKernelGGL(act_out_kernel, dim3((rows * Ad + 255) / 256), dim3(256), 0, s, mu, ls, ep, rows, Ad, det, ao);
      };
      tail.push_back(op);
    }
    return GRL_OK;
  }

  // =============================================================== Keras auto-encoder (A.9), batch NA
  void encoder_path() {
    const ConvGeom eg[3] = {{64, 64, 1, 7, 7, 2, 2, 32, 32, 32}, {32, 32, 32, 5, 5, 2, 1, 16, 16, 32},
                            {16, 16, 32, 3, 3, 2, 0, 8, 8, 32}};
    const int64_t wn[8] = {7 * 7 * 32, 32, 5 * 5 * 32 * 32, 32, 3 * 3 * 32 * 32, 32, 2048 * 100, 100};
    for (int k = 0; k < 8; ++k) h.enc_w[k] = wk.f32(wn[k]);
    h.ex_in = wk.f32((int64_t)NA * 4096);
    h.ec1 = wk.f32((int64_t)NA * 32 * 32 * 32); h.ec2 = wk.f32((int64_t)NA * 16 * 16 * 32);
    h.ec3 = wk.f32((int64_t)NA * 8 * 8 * 32); h.eout = wk.f32((int64_t)NA * 100);
    float* io[4] = {h.ex_in, h.ec1, h.ec2, h.ec3};
    for (int l = 0; l < 3; ++l) {
      ConvFwdTabs t = h.conv_fwd_tabs(eg[l], NA);
      h.add_launch(h.ops_enc, "enc_conv", 0,
                 {h.conv_fwd(io[l], t, eg[l], h.enc_w[2 * l], h.enc_w[2 * l + 1], io[l + 1], ACT_LEAKY, 0.1f)});
    }
    IgemmProb p = h.dense_fwd(h.ec3, 2048, 2048, nullptr, 0, 0, NA, h.enc_w[6], 100, h.enc_w[7], h.eout, 100, ACT_LEAKY);
    p.act_alpha = 0.1f;
    h.add_launch(h.ops_enc, "enc_dense", 0, {p});
  }

  // debug taps (grl_debug_fetch / _store) and, under GRL_PLAN_DUMP, the launch order of every op list
  void debug_views() {
    h.dbg["feat_pi"] = {h.feat[0], (int64_t)B * ldf};
    h.dbg["feat_vf"] = {h.feat[1], (int64_t)B * ldf};
    h.dbg["feat_tgt"] = {h.feat[2], (int64_t)B * ldf};
    if (cnn) {
      h.dbg["x_obs"] = {h.x_obs, (int64_t)B * img_elems};
      h.dbg["x_next"] = {h.x_next, (int64_t)B * img_elems};
      h.dbg["a1_pi"] = {a1[0], (int64_t)B * geo.p1 * 32};   // (side-by-side layout: the first half of the pair buffer, stride 64)
      h.dbg["a2_pi"] = {a2[0], (int64_t)B * geo.p2 * 64};
      h.dbg["a3_pi"] = {a3[0], (int64_t)B * geo.K};
      h.dbg["a1_pair"] = {a1[0], (int64_t)B * geo.p1 * 64};   // [B * 225][pi 0..31 | values_fn 32..63]
      h.dbg["a2_vf"] = {a2[1], (int64_t)B * geo.p2 * 64};
      h.dbg["a3_vf"] = {a3[1], (int64_t)B * geo.K};
      h.dbg["g1_vf"] = {g1[1], (int64_t)B * geo.p1 * 32};
      h.dbg["g2_vf"] = {g2[1], (int64_t)B * geo.p2 * 64};
      h.dbg["g3_vf"] = {g3[1], (int64_t)B * geo.K};
      h.dbg["dfeat_pi"] = {dfeat[0], (int64_t)B * ldf};
      h.dbg["dfeat_vf"] = {dfeat[1], (int64_t)B * ldf};
    }
    h.dbg["mu"] = {hPI.out[0], (int64_t)B * A};
    h.dbg["log_std"] = {hPI.out[1], (int64_t)B * A};
    h.dbg["pi"] = {pi_a, (int64_t)B * A};
    h.dbg["logp"] = {logp, B};
    h.dbg["qf1"] = {hQF1.out[0], B}; h.dbg["qf2"] = {hQF2.out[0], B};
    h.dbg["v"] = {hVF.out[0], B}; h.dbg["v_tgt"] = {hTGT.out[0], B};
    h.dbg["qf1_pi"] = {hQF1PI.out[0], B}; h.dbg["qf2_pi"] = {hQF2PI.out[0], B};
    h.dbg["rew"] = {h.rew, B}; h.dbg["done"] = {h.done, B}; h.dbg["act"] = {h.act, (int64_t)B * A};
    h.dbg["dmu"] = {dmu, (int64_t)B * ld_dm}; h.dbg["dls"] = {dls, (int64_t)B * ld_dm};   // rows of stride ld_dm (Ap on the fused routes)
    h.dbg["da_pi"] = {da_pi, (int64_t)B * A};
    h.dbg["grads"] = {h.grads, h.n_train};
    h.dbg["adam_m"] = {h.adam_m, h.n_train};
    h.dbg["adam_v"] = {h.adam_v, h.n_train};
    h.dbg["rp_obs"] = {h.rp_obs, cap * obs_store}; h.dbg["rp_next"] = {h.rp_next, cap * obs_store};
    h.dbg["rp_dobs"] = {h.rp_dobs, cap * std::max(nd, 1)}; h.dbg["rp_dnext"] = {h.rp_dnext, cap * std::max(nd, 1)};
    h.dbg["rp_act"] = {h.rp_act, cap * A}; h.dbg["rp_rew"] = {h.rp_rew, cap}; h.dbg["rp_done"] = {h.rp_done, cap};
    h.dbg["idx_raw"] = {(const float*)h.idx_buf, (int64_t)2 * B};     // replay indices of the last minibatch: int64 viewed as float pairs
    plan_seq("ops_rng", h.ops_rng); plan_seq("ops_gather", h.ops_gather); plan_seq("ops_grads", h.ops_grads);
    plan_seq("ops_grads_apply", h.ops_grads_apply); plan_seq("ops_apply", h.ops_apply);
    plan_seq("ops_stage0", h.ops_stage0); plan_seq("ops_stage1", h.ops_stage1);
    plan_seq("pf", h.pf); plan_seq("ride", h.ride);
  }
};

}  // namespace

int grl_ctx::plan_sac() {
  SacPlanner p(*this);
  p.shapes();                // shapes + parameter layout
  if (int e = p.fits()) return e;
  p.arenas();                // state, gradient, replay and work arena (the carving order is the checkpoint format)
  if (int e = p.gather()) return e;
  p.forward();               // conv stack or a launch per layer, fc_fwd
  p.heads();                 // one of three routes: forward, losses, backward down to d feat
  p.backward_data();
  p.weight_gradients();      // ... with the riders on conv3_bwd; the launches of the backward half in their final order
  p.staged_split();
  p.reductions();
  if (int e = p.call_plans()) return e;      // reduction + Adam, "prefetch", "gather_ride"
  p.apply();
  if (int e = p.act_path()) return e;
  p.encoder_path();
  p.debug_views();
  return GRL_OK;
}
