// capi.inl: the C ABI of include/grl.h (extern "C" entry points over grl_ctx) -- part of engine.hip (included there, same translation unit: the plans are methods of grl_ctx).

// ==================================================================================================
// C ABI
// ==================================================================================================
// PPO handles (plan_ppo.inl) hold a rollout, not a replay ring, and have one update form: the entry points of the other
// algorithms stop here, before anything moves
#define NOT_ON_PPO(h, what)                                                                                                       \
  do {                                                                                                                            \
    if ((h) && (h)->cfg.algo == GRL_ALGO_PPO)                                                                                     \
      return fail(GRL_ERR_STATE, what " is not defined on a PPO handle (PPO handles: grl_ppo_step / _rewards / _finish / _train, grl_act)"); \
    if ((h) && (h)->cfg.algo == GRL_ALGO_TRPO)                                                                                    \
      return fail(GRL_ERR_STATE, what " is not defined on a TRPO handle (TRPO handles: grl_ppo_step / _rewards / _finish, grl_trpo_update, grl_act)"); \
  } while (0)
// ... except the statistics calls on a PPO / TRPO handle created with normalize = 2 (it keeps VecNormalize's observation
// statistics: grl_observe, grl_set_obs_stats, grl_set_running_stats, grl_get_obs_stats)
#define NOT_ON_PPO_WITHOUT_STATS(h, what)                                                                                         \
  do {                                                                                                                            \
    if ((h) && !(h)->n_sd) NOT_ON_PPO(h, what);                                                                                   \
  } while (0)

// TD3 handles (plan_td3.inl) keep a SAC handle's replay ring and statistics but have one update form of their own: what they do
// not define stops here, before anything moves
#define NOT_ON_TD3(h, what)                                                                                                       \
  do {                                                                                                                            \
    if ((h) && (h)->cfg.algo == GRL_ALGO_TD3)                                                                                     \
      return fail(GRL_ERR_STATE, what " is not defined on a TD3 handle (TD3 handles: grl_td3_train, grl_td3_get_metrics, grl_act, grl_replay_add, the statistics calls)"); \
  } while (0)

// `also`: the algorithm above 4 whose own create / query_sizes call is checking (GRL_ALGO_TRPO, GRL_ALGO_TD3), or -1
static int check_cfg(const grl_config* c, int also = -1) {
  if (!c) return fail(GRL_ERR_INVALID, "null config");
  if (c->algo == GRL_ALGO_AE) {
    if (c->batch_size < 1 || c->batch_size > 4096) return fail(GRL_ERR_INVALID, "batch_size out of range");
    if (c->replay_capacity < 1) return fail(GRL_ERR_INVALID, "replay_capacity must be >= 1");
    if (!cfg_ae_default(*c) && !ae_net_ok(ae_net_of(*c))) return fail(GRL_ERR_INVALID, ae_domain_text());
    return GRL_OK;
  }
  if (!cfg_ae_default(*c)) return fail(GRL_ERR_INVALID, "the ae_* fields are defined for auto-encoder handles");
  if (c->extractor < 0 || c->extractor > 2) return fail(GRL_ERR_INVALID, "extractor must be 0..2");
  if (c->n_layers < 1 || c->n_layers > GRL_MAX_LAYERS) return fail(GRL_ERR_INVALID, "n_layers out of range");
  for (int l = 0; l < c->n_layers; ++l)
    if (c->layers[l] < 1 || c->layers[l] > 4096) return fail(GRL_ERR_INVALID, "layer width out of range");
  if (c->batch_size < 1 || c->batch_size > 65536) return fail(GRL_ERR_INVALID, "batch_size out of range");
  if (c->act_dim < 1 || c->act_dim > 64) return fail(GRL_ERR_INVALID, "act_dim out of range");
  if (c->replay_capacity < 1) return fail(GRL_ERR_INVALID, "replay_capacity must be >= 1");
  if (c->algo < 0 || c->algo > 4) {
    if (!(also >= 0 && c->algo == also))
      return fail(GRL_ERR_INVALID, "algo must be 0..4 (5, GRL_ALGO_TRPO, needs a grl_trpo_config: grl_trpo_query_sizes / grl_trpo_create; "
                                   "6, GRL_ALGO_TD3, a grl_td3_config: grl_td3_query_sizes / grl_td3_create)");
  }
  if (c->algo == GRL_ALGO_TD3) {      // (read as a SAC handle's on vector observations)
    if (c->extractor != GRL_EXTRACTOR_MLP) return fail(GRL_ERR_INVALID, "TD3: extractor must be GRL_EXTRACTOR_MLP (CNN extractors are not implemented)");
    if (c->obs_dim < 1 || c->obs_dim > 64 * 64 * 5) return fail(GRL_ERR_INVALID, "TD3: obs_dim must be 1..20480");
    if (c->normalize < 0 || c->normalize > 3) return fail(GRL_ERR_INVALID, "TD3: normalize must be 0..3");
    if (c->act_batch < 0) return fail(GRL_ERR_INVALID, "TD3: act_batch must be >= 0");
    if (c->q_branches || c->q_bins || c->q_n_common || c->q_n_branch || c->q_n_value || c->q_huber || c->q_double || c->q_grad_clip != 0.f ||
        c->q_trunk_scale != 0.f || c->q_per || c->q_per_alpha != 0.f || c->q_per_eps != 0.f || c->q_per_stratified || c->q_per_alpha64 != 0.0 ||
        c->q_loss_sum_branches || c->q_layer_norm || c->replay_rgb_u8)
      return fail(GRL_ERR_INVALID, "TD3: every q_* field and replay_rgb_u8 must be 0");
    return GRL_OK;
  }
  if (c->algo == GRL_ALGO_PPO || c->algo == GRL_ALGO_TRPO) {      // (a TRPO handle's grl_config is read as a PPO handle's)
    if (c->extractor != GRL_EXTRACTOR_MLP) return fail(GRL_ERR_INVALID, "PPO runs on flattened observations (MLP extractor)");
    if (c->obs_dim < 1 || c->obs_dim > 64 * 64 * 5) return fail(GRL_ERR_INVALID, "PPO: obs_dim must be 1..20480");
    for (int l = 0; l < c->n_layers; ++l)
      if (c->layers[l] > 1024) return fail(GRL_ERR_INVALID, "PPO: tower widths must be 1..1024");
    if (c->normalize == 1 || c->normalize == 3)
      return fail(GRL_ERR_INVALID, "PPO: normalize " + std::to_string(c->normalize) + " asks for rewards normalised at sample time; a rollout stores the reward "
                                   "VecNormalize normalised at step time, on the host (normalize must be 0, or 2: observation statistics on the device, grl_observe)");
    if (c->normalize != 0 && c->normalize != 2) return fail(GRL_ERR_INVALID, "PPO: normalize must be 0 or 2");
    if (c->normalize == 2 && (!(c->clip_obs > 0.f) || !(c->norm_eps >= 0.f))) return fail(GRL_ERR_INVALID, "PPO: normalize = 2 needs clip_obs > 0 and norm_eps >= 0");
    if (c->act_batch < 1) return fail(GRL_ERR_INVALID, "PPO: act_batch must equal n_envs");
    if (c->q_branches || c->q_bins || c->q_n_common || c->q_n_branch || c->q_n_value || c->q_huber || c->q_double || c->q_grad_clip != 0.f ||
        c->q_trunk_scale != 0.f || c->q_per || c->q_per_alpha != 0.f || c->q_per_eps != 0.f || c->q_per_stratified || c->q_per_alpha64 != 0.0 ||
        c->q_loss_sum_branches || c->q_layer_norm || c->replay_rgb_u8)
      return fail(GRL_ERR_INVALID, "PPO: every q_* field and replay_rgb_u8 must be 0");
    return GRL_OK;
  }
  if (c->algo != GRL_ALGO_SAC) {
    if (c->extractor != GRL_EXTRACTOR_MLP) return fail(GRL_ERR_INVALID, "DQN/BDQ run on vector observations (MLP extractor)");
    if (c->q_branches < 1 || c->q_branches > 16 || c->q_branches != c->act_dim)
      return fail(GRL_ERR_INVALID, "q_branches must be 1..16 and equal act_dim");
    if (c->q_bins < 2 || c->q_bins > 1024) return fail(GRL_ERR_INVALID, "q_bins out of range");
    if (c->q_n_common < 0 || c->q_n_common > GRL_MAX_LAYERS || c->q_n_branch < 1 || c->q_n_branch > GRL_MAX_LAYERS ||
        c->q_n_value < 1 || c->q_n_value > GRL_MAX_LAYERS)
      return fail(GRL_ERR_INVALID, "tower depths out of range (branch and value towers need >= 1 hidden layer)");
    if (c->q_layer_norm != 0 && c->q_layer_norm != 1) return fail(GRL_ERR_INVALID, "q_layer_norm must be 0 or 1");
    if (c->q_layer_norm && !q_hidden_widths_all(*c, [](int w) { return ln_npl(w) > 0; }))
      return fail(GRL_ERR_INVALID, "layer-normalised Q-networks support hidden widths up to " + std::to_string(64 * LN_MAX_NPL));
    if (c->q_per && c->batch_size > 1024) return fail(GRL_ERR_INVALID, "prioritised replay supports batch_size <= 1024");
    if (c->q_per && c->replay_capacity > (int64_t)PER_BLK * PER_BLK)
      return fail(GRL_ERR_INVALID, "prioritised replay supports up to 1024 x 1024 transitions (two-level segment tree)");
  }
  if (c->q_layer_norm && c->algo != GRL_ALGO_DQN && c->algo != GRL_ALGO_BDQ)
    return fail(GRL_ERR_INVALID, "q_layer_norm is defined for DQN / BDQ handles");
  if (c->replay_rgb_u8) {
    const int c_img = c->obs_channels - ((c->extractor == GRL_EXTRACTOR_AUGMENTED && c->n_direct > 0) ? 1 : 0);
    if (c->algo != GRL_ALGO_SAC || c->extractor == GRL_EXTRACTOR_MLP || c_img != 4)
      return fail(GRL_ERR_INVALID, "replay_rgb_u8 needs SAC on RGB-D images with 4 image channels (R, G, B, depth)");
  }
  if (c->extractor == GRL_EXTRACTOR_MLP) {
    if (c->obs_dim < 1) return fail(GRL_ERR_INVALID, "obs_dim must be >= 1 for the MLP extractor");
  } else {
    if (c->img_hw < 36 || c->img_hw > 128)
      return fail(GRL_ERR_INVALID, "img_hw " + std::to_string(c->img_hw) + ": square images of 36x36 to 128x128 (camera_info.yaml) are supported");
    if (c->obs_channels < 1 || c->obs_channels > 8) return fail(GRL_ERR_INVALID, "obs_channels out of range");
    if (c->extractor == GRL_EXTRACTOR_AUGMENTED && (c->n_direct < 0 || c->n_direct > 64))
      return fail(GRL_ERR_INVALID, "n_direct out of range");
    if (c->extractor == GRL_EXTRACTOR_AUGMENTED && c->n_direct > 0 && c->obs_channels < 2)
      return fail(GRL_ERR_INVALID, "augmented extractor needs >= 2 observation channels");
  }
  return GRL_OK;
}

extern "C" {

const char* grl_last_error(void) { return g_err.c_str(); }
int grl_version(void) { return 1; }

static int check_ppo(const grl_config* c, const grl_ppo_config* p) {
  if (int e = check_cfg(c)) return e;
  if (c->algo != GRL_ALGO_PPO) return fail(GRL_ERR_INVALID, "grl_ppo_query_sizes / grl_ppo_create take a grl_config with algo = GRL_ALGO_PPO");
  if (!p) return fail(GRL_ERR_INVALID, "null PPO config");
  if (p->n_envs < 1 || p->n_steps < 1 || (int64_t)p->n_envs * p->n_steps > (1 << 22)) return fail(GRL_ERR_INVALID, "PPO: n_envs, n_steps must be >= 1 and n_envs * n_steps <= 4194304");
  const int64_t R = (int64_t)p->n_envs * p->n_steps;
  if (c->act_batch != p->n_envs) return fail(GRL_ERR_INVALID, "PPO: act_batch must equal n_envs");
  if (c->replay_capacity != R) return fail(GRL_ERR_INVALID, "PPO: replay_capacity must equal n_envs * n_steps");
  if (R % c->batch_size) return fail(GRL_ERR_INVALID, "PPO: batch_size (the minibatch rows) must divide n_envs * n_steps");
  if (p->n_vf_layers < 1 || p->n_vf_layers > GRL_MAX_LAYERS) return fail(GRL_ERR_INVALID, "PPO: n_vf_layers out of range");
  for (int l = 0; l < p->n_vf_layers; ++l)
    if (p->vf_layers[l] < 1 || p->vf_layers[l] > 1024) return fail(GRL_ERR_INVALID, "PPO: tower widths must be 1..1024");
  if (!(p->lam >= 0.f && p->lam <= 1.f)) return fail(GRL_ERR_INVALID, "PPO: lam must be in [0, 1]");
  if (!(p->clip_range >= 0.f)) return fail(GRL_ERR_INVALID, "PPO: clip_range must be >= 0");
  if (!(p->adam_eps > 0.f)) return fail(GRL_ERR_INVALID, "PPO: adam_eps must be > 0");
  return GRL_OK;
}

static int check_trpo(const grl_config* c, const grl_trpo_config* p) {
  if (int e = check_cfg(c, GRL_ALGO_TRPO)) return e;
  if (c->algo != GRL_ALGO_TRPO) return fail(GRL_ERR_INVALID, "grl_trpo_query_sizes / grl_trpo_create take a grl_config with algo = GRL_ALGO_TRPO");
  if (!p) return fail(GRL_ERR_INVALID, "null TRPO config");
  if (p->n_steps < 1 || p->n_steps > 65536) return fail(GRL_ERR_INVALID, "TRPO: n_steps must be 1..65536");
  if (c->act_batch != 1) return fail(GRL_ERR_INVALID, "TRPO: act_batch must be 1 (one environment)");
  if (c->replay_capacity != p->n_steps) return fail(GRL_ERR_INVALID, "TRPO: replay_capacity must equal n_steps");
  if (p->vf_batch < 1 || c->batch_size != p->vf_batch) return fail(GRL_ERR_INVALID, "TRPO: batch_size must equal vf_batch >= 1");
  if (p->n_vf_layers < 1 || p->n_vf_layers > GRL_MAX_LAYERS) return fail(GRL_ERR_INVALID, "TRPO: n_vf_layers out of range");
  for (int l = 0; l < p->n_vf_layers; ++l)
    if (p->vf_layers[l] < 1 || p->vf_layers[l] > 1024) return fail(GRL_ERR_INVALID, "TRPO: tower widths must be 1..1024");
  if (p->cg_iters < 1 || p->cg_iters > GRL_TRPO_MAX_CG) return fail(GRL_ERR_INVALID, "TRPO: cg_iters must be 1..64");
  if (p->ls_steps < 1 || p->ls_steps > GRL_TRPO_MAX_LS) return fail(GRL_ERR_INVALID, "TRPO: ls_steps must be 1..16");
  if (p->fvp_stride < 1) return fail(GRL_ERR_INVALID, "TRPO: fvp_stride must be >= 1");
  if (!(p->lam >= 0.f && p->lam <= 1.f)) return fail(GRL_ERR_INVALID, "TRPO: lam must be in [0, 1]");
  if (!(p->max_kl > 0.f)) return fail(GRL_ERR_INVALID, "TRPO: max_kl must be > 0");
  if (!(p->cg_damping >= 0.f)) return fail(GRL_ERR_INVALID, "TRPO: cg_damping must be >= 0");
  if (!(p->adam_eps > 0.f)) return fail(GRL_ERR_INVALID, "TRPO: adam_eps must be > 0");
  return GRL_OK;
}

static int check_td3(const grl_config* c, const grl_td3_config* p) {
  if (int e = check_cfg(c, GRL_ALGO_TD3)) return e;
  if (c->algo != GRL_ALGO_TD3) return fail(GRL_ERR_INVALID, "grl_td3_query_sizes / grl_td3_create take a grl_config with algo = GRL_ALGO_TD3");
  if (!p) return fail(GRL_ERR_INVALID, "null TD3 config");
  if (p->policy_delay < 1) return fail(GRL_ERR_INVALID, "TD3: policy_delay must be >= 1");
  if (!(p->target_policy_noise >= 0.f)) return fail(GRL_ERR_INVALID, "TD3: target_policy_noise must be >= 0");
  if (!(p->target_noise_clip >= 0.f)) return fail(GRL_ERR_INVALID, "TD3: target_noise_clip must be >= 0");
  return GRL_OK;
}

static int query_sizes(const grl_config* cfg, const grl_ppo_config* ppo, grl_sizes* out, const grl_trpo_config* trpo = nullptr,
                       const grl_td3_config* td3 = nullptr) {
  if (!out) return fail(GRL_ERR_INVALID, "null out");
  grl_ctx ctx;
  ctx.cfg = *cfg;
  if (ppo) ctx.pcfg = *ppo;
  if (trpo) ctx.tcfg = *trpo;
  if (td3) ctx.td3cfg = *td3;
  ctx.dry = true;
  if (int e = ctx.plan()) return e;
  out->state_bytes = ctx.st.off + 256;
  out->grads_bytes = ctx.gr.off + 256;
  out->work_bytes = ctx.wk.off + 256;
  out->replay_bytes = ctx.rp.off + 256;
  out->n_params = ctx.n_params;
  out->n_trainable = ctx.n_train;
  return GRL_OK;
}

int grl_query_sizes(const grl_config* cfg, grl_sizes* out) {
  if (int e = check_cfg(cfg)) return e;
  if (cfg->algo == GRL_ALGO_PPO) return fail(GRL_ERR_INVALID, "a PPO handle needs a grl_ppo_config: use grl_ppo_query_sizes / grl_ppo_create");
  return query_sizes(cfg, nullptr, out);
}
int grl_ppo_query_sizes(const grl_config* cfg, const grl_ppo_config* ppo, grl_sizes* out) {
  if (int e = check_ppo(cfg, ppo)) return e;
  return query_sizes(cfg, ppo, out);
}
int grl_trpo_query_sizes(const grl_config* cfg, const grl_trpo_config* trpo, grl_sizes* out) {
  if (int e = check_trpo(cfg, trpo)) return e;
  return query_sizes(cfg, nullptr, out, trpo);
}
int grl_td3_query_sizes(const grl_config* cfg, const grl_td3_config* td3, grl_sizes* out) {
  if (int e = check_td3(cfg, td3)) return e;
  return query_sizes(cfg, nullptr, out, nullptr, td3);
}

// Prioritised replay with an empty ring: all leaves 0, PerState at its starting values.  The block sums / minima (per.bsum,
// per.bmin) need no reset: the first update of every prioritised call rebuilds ALL of them from the leaves below the ring's fill
// (per_blocksum_kernel in front of the first sampler, plan_q.inl), on a used handle as on a new one.  Used by grl_create and
// by grl_state_import for a checkpoint saved without its ring.
static hipError_t per_start(grl_ctx* h) {
  hipError_t e = hipMemset(h->per.p, 0, (size_t)h->cfg.replay_capacity * 8);
  if (e != hipSuccess) return e;
  PerState ps;
  memset(&ps, 0, sizeof(ps));
  ps.max_priority = 1.f; ps.p_min = 1.0; ps.beta = 1.0;
  return hipMemcpy(h->per.st, &ps, sizeof(ps), hipMemcpyHostToDevice);
}

// epsilon of VecNormalize on a PPO / TRPO handle: the Python float when the second configuration block carries it
static double ppo_norm_eps(const grl_ctx* h) { return h->pcfg.norm_eps64 != 0.0 ? h->pcfg.norm_eps64 : (double)h->cfg.norm_eps; }
// mean, var (and sqrt(var + eps)) of a PPO / TRPO handle with normalize = 2, taken as given
static int ppo_load_stats(grl_ctx* h, const double* mean, const double* var);

static int create_handle(const grl_config* cfg, const grl_ppo_config* ppo, const grl_buffers* bufs, grl_handle* out,
                         const grl_trpo_config* trpo = nullptr, const grl_td3_config* td3 = nullptr) {
  if (!bufs || !out || !bufs->state || !bufs->grads || !bufs->work || !bufs->replay)
    return fail(GRL_ERR_INVALID, "null buffers");
  std::unique_ptr<grl_ctx> owner(new grl_ctx());      // released into *out on success: every refusal below destroys it
  grl_ctx* h = owner.get();
  h->cfg = *cfg;
  if (ppo) h->pcfg = *ppo;
  if (trpo) h->tcfg = *trpo;
  if (td3) h->td3cfg = *td3;
  h->st.base = (char*)bufs->state; h->gr.base = (char*)bufs->grads;
  h->wk.base = (char*)bufs->work; h->rp.base = (char*)bufs->replay;
  if (int e = h->plan()) return e;
  h->use_graph = !h->sw.get(Sw::GRL_NO_GRAPH);
  for (auto& u : h->uploads) {
    hipError_t e = hipMemcpy(u.dst, u.bytes.data(), u.bytes.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(GRL_ERR_HIP, std::string("table upload: ") + hipGetErrorString(e));
  }
  h->uploads.clear();
  for (auto& z : h->zero_once) hipMemset(z.first, 0, z.second);
  // state: zero Adam moments, scalars; stats = identity
  hipMemset(h->adam_m, 0, (size_t)h->n_train * 4);
  hipMemset(h->adam_v, 0, (size_t)h->n_train * 4);
  hipMemset(h->grads, 0, (size_t)h->n_train * 4);
  DevScalars s0;
  memset(&s0, 0, sizeof(s0));
  s0.beta1_power = 0.9f; s0.beta2_power = 0.999f;
  s0.lr = cfg->lr;
  hipError_t e = hipMemcpy(h->sc, &s0, sizeof(s0), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(GRL_ERR_HIP, std::string("scalar init: ") + hipGetErrorString(e));
  if (h->sc2) {      // TD3: the policy's optimiser words, the update cursor
    e = hipMemcpy(h->sc2, &s0, sizeof(s0), hipMemcpyHostToDevice);
    const Td3Dev d0 = {-1, -1, 0.f, 0};
    if (e == hipSuccess) e = hipMemcpy(h->td3_dev, &d0, sizeof(d0), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(GRL_ERR_HIP, std::string("td3 init: ") + hipGetErrorString(e));
  }
  if (h->n_mean) {   // RunningMeanStd(): mean 0, var 1, count 1e-4
    std::vector<double> ones((size_t)h->n_elems, 1.0);
    const double c2[2] = {1e-4, 1e-4};
    hipMemset(h->n_mean, 0, (size_t)h->n_elems * 8);
    hipMemcpy(h->n_var, ones.data(), ones.size() * 8, hipMemcpyHostToDevice);
    hipMemcpy(h->n_count, c2, 16, hipMemcpyHostToDevice);
    if (h->n_sd) {      // PPO / TRPO, normalize = 2: sqrt(var + eps) beside them
      std::vector<double> sd((size_t)h->n_elems, std::sqrt(1.0 + ppo_norm_eps(h)));
      hipMemcpy(h->n_sd, sd.data(), sd.size() * 8, hipMemcpyHostToDevice);
    }
  }
  if (h->per_on) {
    e = per_start(h);
    if (e != hipSuccess) return fail(GRL_ERR_HIP, std::string("per init: ") + hipGetErrorString(e));
  }
  if (h->ppo_dev) {
    e = hipMemset(h->ppo_dev, 0, sizeof(PpoDev));
    if (e != hipSuccess) return fail(GRL_ERR_HIP, std::string("ppo init: ") + hipGetErrorString(e));
  }
  if (h->trpo_dev) {
    e = hipMemset(h->trpo_dev, 0, sizeof(TrpoDev));
    if (e != hipSuccess) return fail(GRL_ERR_HIP, std::string("trpo init: ") + hipGetErrorString(e));
  }
  *out = owner.release();
  return GRL_OK;
}

int grl_create(const grl_config* cfg, const grl_buffers* bufs, grl_handle* out) {
  if (int e = check_cfg(cfg)) return e;
  if (cfg->algo == GRL_ALGO_PPO) return fail(GRL_ERR_INVALID, "a PPO handle needs a grl_ppo_config: use grl_ppo_query_sizes / grl_ppo_create");
  return create_handle(cfg, nullptr, bufs, out);
}
int grl_ppo_create(const grl_config* cfg, const grl_ppo_config* ppo, const grl_buffers* bufs, grl_handle* out) {
  if (int e = check_ppo(cfg, ppo)) return e;
  return create_handle(cfg, ppo, bufs, out);
}
int grl_trpo_create(const grl_config* cfg, const grl_trpo_config* trpo, const grl_buffers* bufs, grl_handle* out) {
  if (int e = check_trpo(cfg, trpo)) return e;
  return create_handle(cfg, nullptr, bufs, out, trpo);
}
int grl_td3_create(const grl_config* cfg, const grl_td3_config* td3, const grl_buffers* bufs, grl_handle* out) {
  if (int e = check_td3(cfg, td3)) return e;
  return create_handle(cfg, nullptr, bufs, out, nullptr, td3);
}

int grl_destroy(grl_handle h) {
  if (!h) return GRL_OK;
  hipStreamSynchronize(h->stream);
  delete h;
  return GRL_OK;
}

int grl_set_stream(grl_handle h, void* s) {
  if (!h) return fail(GRL_ERR_INVALID, "null handle");
  if ((hipStream_t)s != h->stream) h->drop_graphs();
  h->stream = (hipStream_t)s;
  return GRL_OK;
}

int grl_param_count(grl_handle h) { return h ? (int)h->vars.size() : fail(GRL_ERR_INVALID, "null handle"); }

int grl_param_info(grl_handle h, int i, char* name, int cap, int64_t* off, int64_t* numel, int32_t* ndim,
                   int64_t shape[4], int32_t* trainable) {
  if (!h || i < 0 || i >= (int)h->vars.size()) return fail(GRL_ERR_INVALID, "bad parameter index");
  const Var& v = h->vars[i];
  if (name && cap > 0) { strncpy(name, v.name.c_str(), cap - 1); name[cap - 1] = 0; }
  if (off) *off = v.off;
  if (numel) *numel = v.numel;
  if (ndim) *ndim = v.ndim;
  if (shape) for (int k = 0; k < 4; ++k) shape[k] = v.shape[k];
  if (trainable) *trainable = v.trainable ? 1 : 0;
  return GRL_OK;
}

int grl_reset_optimizer(grl_handle h) {
  if (!h) return fail(GRL_ERR_INVALID, "null handle");
  HIPCHK(hipMemsetAsync(h->adam_m, 0, (size_t)h->n_train * 4, h->stream));
  HIPCHK(hipMemsetAsync(h->adam_v, 0, (size_t)h->n_train * 4, h->stream));
  DevScalars s0;
  HIPCHK(hipMemcpy(&s0, h->sc, sizeof(s0), hipMemcpyDeviceToHost));
  s0.beta1_power = 0.9f; s0.beta2_power = 0.999f;
  HIPCHK(hipMemcpy(h->sc, &s0, sizeof(s0), hipMemcpyHostToDevice));
  if (h->sc2) {      // TD3: the policy's Adam too
    HIPCHK(hipMemcpy(&s0, h->sc2, sizeof(s0), hipMemcpyDeviceToHost));
    s0.beta1_power = 0.9f; s0.beta2_power = 0.999f;
    HIPCHK(hipMemcpy(h->sc2, &s0, sizeof(s0), hipMemcpyHostToDevice));
  }
  return GRL_OK;
}

int grl_set_learning_rate(grl_handle h, float lr) {
  if (!h) return fail(GRL_ERR_INVALID, "null handle");
  if (!(lr >= 0.f)) return fail(GRL_ERR_INVALID, "learning rate must be >= 0");
  // the step size lives in device memory (the captured graphs read it), set in stream order
  hipLaunchKernelGGL(set_f32_kernel, dim3(1), dim3(1), 0, h->stream, &h->sc->lr, lr);
  return GRL_OK;
}

int grl_set_obs_stats(grl_handle h, const double* mean, const double* var, double ret_var) {
  NOT_ON_PPO_WITHOUT_STATS(h, "grl_set_obs_stats");
  if (!h || !mean || !var) return fail(GRL_ERR_INVALID, "null argument");
  if (h->n_sd) return ppo_load_stats(h, mean, var);      // (ret_var: rewards are normalised on the host)
  const grl_config& c = h->cfg;
  const double eps = c.norm_eps;
  const int nd = h->cnn ? h->F - 512 : 0;
  // The five statistic blocks sit one after the other in the state arena (alignment gaps in between are unused):
  // they are written into a page-locked mirror of that span and leave as ONE asynchronous copy in stream order.
  // Two mirrors alternate (StagingRing), each guarded by an event, so the host never waits for the GPU here (the learn loop
  // calls this before every update: a stream synchronisation plus five blocking copies serialised host and device).  The
  // mirrors are zeroed when they are allocated and the gaps are never written: the WHOLE span lands in the state arena.
  char* base = (char*)h->s_mean;
  const size_t span = (size_t)((char*)h->s_ret + 8 - base);
  char* pm = nullptr;
  HIPCHK(h->stats_ring.acquire(span, &pm));      // (waits for the copy issued two calls ago)
  double* m = (double*)pm;
  double* s = (double*)(pm + ((char*)h->s_std - base));
  double* dm = (double*)(pm + ((char*)h->s_dmean - base));
  double* ds = (double*)(pm + ((char*)h->s_dstd - base));
  double* rs = (double*)(pm + ((char*)h->s_ret - base));
  if (h->cnn) {
    const int co = c.obs_channels, ci = h->C_img;
    for (int px = 0; px < h->hw * h->hw; ++px)
      for (int ch = 0; ch < ci; ++ch) {
        m[px * ci + ch] = mean[px * co + ch];
        s[px * ci + ch] = std::sqrt(var[px * co + ch] + eps);
      }
    for (int q = 0; q < nd; ++q) {
      dm[q] = mean[q * co + (co - 1)];
      ds[q] = std::sqrt(var[q * co + (co - 1)] + eps);
    }
  } else {
    for (int q = 0; q < h->img_elems; ++q) { m[q] = mean[q]; s[q] = std::sqrt(var[q] + eps); }
  }
  *rs = std::sqrt(ret_var + eps);
  HIPCHK(hipMemcpyAsync(base, pm, span, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h->stats_ring.release(h->stream));
  return GRL_OK;
}

// Host-to-device copy of a CALLER-owned buffer that the caller may reuse the moment the entry point returns (include/grl.h:
// "copied before the call returns").  For PAGEABLE memory (NumPy arrays, malloc) hipMemcpyAsync stages the source before it
// returns -- the documented behaviour of the asynchronous copies for pageable host memory -- so nothing more is needed.  A
// page-locked or registered source is read by the DMA engine LATER, in stream order: wait for that copy.  GRL_TUNE
// host_copy_wait=1 waits in every case (a runtime whose pageable path cannot be trusted); tests/test_gpu_api.py mutates
// the source right after each of these calls.
static int copy_from_caller(grl_handle h, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
  static const int always = Switches(SwRead::FIRST_COPY).get(Sw::host_copy_wait);
  bool wait = always != 0;
  if (!wait) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, src) == hipSuccess) wait = at.type == hipMemoryTypeHost || at.type == hipMemoryTypeManaged;
    else (void)hipGetLastError();      // unknown to the runtime: pageable
  }
  if (wait) {
    HIPCHK_AS("hipEventCreateWithFlags(&h->copy_ev, hipEventDisableTiming)", h->copy_ev.create());
    HIPCHK(hipEventRecord(h->copy_ev.raw(), h->stream));
    HIPCHK(hipEventSynchronize(h->copy_ev.raw()));
  }
  return GRL_OK;
}

int grl_set_ret_var(grl_handle h, double ret_var) {
  NOT_ON_PPO(h, "grl_set_ret_var");
  if (!h) return fail(GRL_ERR_INVALID, "null handle");
  const double sd = std::sqrt(ret_var + (double)h->cfg.norm_eps);
  HIPCHK(hipMemcpyAsync(h->s_ret, &sd, 8, hipMemcpyHostToDevice, h->stream));   // (pageable source: staged before returning)
  return GRL_OK;
}

static int ppo_load_stats(grl_ctx* h, const double* mean, const double* var) {
  const double eps = ppo_norm_eps(h);
  std::vector<double> sd((size_t)h->n_elems);
  for (size_t e = 0; e < sd.size(); ++e) sd[e] = std::sqrt(var[e] + eps);
  if (int e = copy_from_caller(h, h->n_mean, mean, sd.size() * 8)) return e;
  if (int e = copy_from_caller(h, h->n_var, var, sd.size() * 8)) return e;
  // (`sd` is pageable: hipMemcpyAsync has staged it when it returns; a GRL_TUNE host_copy_wait=1 run waits as for the others)
  return copy_from_caller(h, h->n_sd, sd.data(), sd.size() * 8);
}

int grl_set_running_stats(grl_handle h, const double* mean, const double* var, double count) {
  NOT_ON_PPO_WITHOUT_STATS(h, "grl_set_running_stats");
  if (!h || !mean || !var) return fail(GRL_ERR_INVALID, "null argument");
  if (!h->n_mean) return fail(GRL_ERR_STATE, "this handle keeps no running statistics");
  // (rare: once per attach / load; pageable sources are staged before hipMemcpyAsync returns)
  if (h->n_sd) {
    if (int e = ppo_load_stats(h, mean, var)) return e;
  } else {
    if (int e = copy_from_caller(h, h->n_mean, mean, (size_t)h->n_elems * 8)) return e;
    if (int e = copy_from_caller(h, h->n_var, var, (size_t)h->n_elems * 8)) return e;
  }
  const double c2[2] = {count, count};
  HIPCHK(hipMemcpyAsync(h->n_count, c2, 16, hipMemcpyHostToDevice, h->stream));
  return GRL_OK;
}

// DQN / BDQ handles keep their running statistics per process: on a connected handle the calls that update them are refused
// BEFORE anything moves (the merge over the ranks, dp_norm_*, is the SAC handles')
static int stats_update_refused(grl_handle h) {
  if (h->dp_on && h->cfg.algo != GRL_ALGO_SAC)
    return fail(GRL_ERR_STATE, "this DQN / BDQ handle is connected to a data-parallel exchange: merging its running statistics over the ranks is not implemented (keep them on the host)");
  return GRL_OK;
}

// RunningMeanStd.update over `n` raw observations that are already on the device
static int norm_update_from(grl_handle h, const float* dev_obs, int n) {
  const grl_config& c = h->cfg;
  NormUpdateArgs a;
  memset(&a, 0, sizeof(a));
  a.obs = dev_obs; a.n = n; a.elems = (int)h->n_elems;
  a.mean = h->n_mean; a.var = h->n_var; a.count = h->n_count; a.parity = h->n_parity; a.eps = c.norm_eps;
  a.hw = h->hw * h->hw; a.c_obs = c.obs_channels; a.c_img = h->C_img; a.n_direct = h->cnn ? h->F - 512 : 0; a.vec = h->cnn ? 0 : 1;
  a.s_mean = h->s_mean; a.s_std = h->s_std; a.s_dmean = h->s_dmean; a.s_dstd = h->s_dstd;
  const dim3 grid((unsigned)((h->n_elems + 255) / 256));
  if (h->dp_on) {   // data parallel: the batch moments of all ranks, merged in rank order by every replica (dp_kernels.h)
    if (h->dp_err_host.get() && *h->dp_err_host.get()) return fail(GRL_ERR_STATE, "an exchange timed out waiting for a peer (the replicas are no longer in step)");
    DpNormArgs na = h->dp_norm;
    na.nu = a;
    hipLaunchKernelGGL(dp_norm_moments_kernel, grid, dim3(256), 0, h->stream, na);
    hipLaunchKernelGGL(dp_wait_kernel, dim3(1), dim3(64), 0, h->stream, na.d, 0);
    hipLaunchKernelGGL(dp_norm_merge_kernel, grid, dim3(256), 0, h->stream, na);
  } else {
    hipLaunchKernelGGL(norm_update_kernel, grid, dim3(256), 0, h->stream, a);
  }
  h->n_parity ^= 1;
  HIPCHK(hipGetLastError());
  return GRL_OK;
}

int grl_norm_update(grl_handle h, const float* obs, int n) {
  NOT_ON_PPO(h, "grl_norm_update");
  if (!h || !obs || n < 1) return fail(GRL_ERR_INVALID, "bad argument");
  if (!h->n_mean) return fail(GRL_ERR_STATE, "this handle keeps no running statistics");
  if (n > h->stg_n) return fail(GRL_ERR_INVALID, "more observations than one env step of act_batch environments");
  if (int e = stats_update_refused(h)) return e;
  if (int e = copy_from_caller(h, h->n_stage, obs, (size_t)n * h->n_elems * 4)) return e;
  return norm_update_from(h, h->n_stage, n);
}

int grl_get_obs_stats(grl_handle h, double* mean, double* var, double* count) {
  NOT_ON_PPO_WITHOUT_STATS(h, "grl_get_obs_stats");
  if (!h || !mean || !var || !count) return fail(GRL_ERR_INVALID, "null argument");
  if (!h->n_mean) return fail(GRL_ERR_STATE, "this handle keeps no running statistics");
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(mean, h->n_mean, (size_t)h->n_elems * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(var, h->n_var, (size_t)h->n_elems * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(count, h->n_count + h->n_parity, 8, hipMemcpyDeviceToHost));
  return GRL_OK;
}

static int replay_add_dev(grl_handle h, const float* obs, const float* act, const float* rew, const float* nxt,
                          const float* done, int n, const int* next_row = nullptr, const float* next_alt = nullptr) {
  const grl_config& c = h->cfg;
  IngestArgs ia;
  memset(&ia, 0, sizeof(ia));
  ia.obs = obs; ia.next_obs = nxt; ia.act = act; ia.rew = rew; ia.done = done;
  ia.n = n; ia.hw = h->hw * h->hw; ia.c_obs = c.obs_channels; ia.c_img = h->C_img;
  ia.n_direct = h->cnn ? h->F - 512 : 0; ia.act_dim = h->A; ia.vec_dim = h->cnn ? 0 : c.obs_dim;
  ia.pos = h->rp_pos; ia.cap = c.replay_capacity;
  ia.rp_obs = h->rp_obs; ia.rp_next = h->rp_next; ia.rp_dobs = h->rp_dobs; ia.rp_dnext = h->rp_dnext;
  ia.rp_act = h->rp_act; ia.rp_rew = h->rp_rew; ia.rp_done = h->rp_done;
  ia.rgb_u8 = (c.algo == GRL_ALGO_SAC) ? c.replay_rgb_u8 : 0;
  ia.next_row = next_row; ia.next_alt = next_alt;
  const int elems = h->cnn ? (ia.rgb_u8 ? h->hw * h->hw : h->img_elems) : c.obs_dim;
  ia.size_out = &h->sc->replay_size;
  ia.new_size = std::min<int64_t>(c.replay_capacity, h->rp_size + n);
  hipLaunchKernelGGL(ingest_kernel, dim3((elems + 255) / 256, n, 2), dim3(256), 0, h->stream, ia);
  if (h->per_on)   // new transitions enter with max_priority ** alpha
    hipLaunchKernelGGL(per_add_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->per, h->rp_pos, n,
                       (int64_t)c.replay_capacity);
  h->rp_pos = (h->rp_pos + n) % c.replay_capacity;
  h->rp_size = ia.new_size;
  HIPCHK(hipGetLastError());
  return GRL_OK;
}

int grl_replay_add_device(grl_handle h, const float* obs, const float* act, const float* rew,
                          const float* next_obs, const float* done, int n) {
  NOT_ON_PPO(h, "grl_replay_add_device");
  if (!h || !obs || !act || !rew || !next_obs || !done || n < 1) return fail(GRL_ERR_INVALID, "bad argument");
  if (n > h->cfg.replay_capacity) return fail(GRL_ERR_INVALID, "n exceeds replay capacity");
  return replay_add_dev(h, obs, act, rew, next_obs, done, n);
}

// host buffer -> pinned staging -> device (and back): hipMemcpyAsync from pageable memory is a synchronous
// staged copy; through page-locked buffers the per-call overhead is a host memcpy plus a true async DMA
// (Pinned::reserve only grows and does not wait: the previous call has finished with both blocks)
static int pin_reserve(grl_handle h, size_t in_floats, size_t out_floats) {
  HIPCHK_AS("hipHostMalloc((void**)&h->pin_in, in_floats * 4, 0)", h->pin_in.reserve(in_floats));
  HIPCHK_AS("hipHostMalloc((void**)&h->pin_out, out_floats * 4, 0)", h->pin_out.reserve(out_floats));
  return GRL_OK;
}

int grl_replay_add(grl_handle h, const float* obs, const float* act, const float* rew, const float* next_obs,
                   const float* done, int n) {
  NOT_ON_PPO(h, "grl_replay_add");
  if (!h || !obs || !act || !rew || !next_obs || !done || n < 1) return fail(GRL_ERR_INVALID, "bad argument");
  const int64_t oe = h->cnn ? (int64_t)h->hw * h->hw * h->cfg.obs_channels : h->cfg.obs_dim;
  // (pageable copies: for these sizes -- 64 KB per transition -- an extra host copy into pinned staging costs
  // more than it saves: 77 -> 90 us for 16 transitions, 150 -> 214 us for 64; measured with scripts/act_bench.py)
  for (int k0 = 0; k0 < n; k0 += h->stg_n) {
    const int m = std::min(h->stg_n, n - k0);
    if (int e = copy_from_caller(h, h->stg_obs, obs + k0 * oe, (size_t)m * oe * 4)) return e;
    if (int e = copy_from_caller(h, h->stg_next, next_obs + k0 * oe, (size_t)m * oe * 4)) return e;
    if (int e = copy_from_caller(h, h->stg_act, act + (int64_t)k0 * h->A, (size_t)m * h->A * 4)) return e;
    if (int e = copy_from_caller(h, h->stg_rew, rew + k0, (size_t)m * 4)) return e;
    if (int e = copy_from_caller(h, h->stg_done, done + k0, (size_t)m * 4)) return e;
    // (no wait between chunks for pageable sources: the copies are stream-ordered behind the ingest launch that reads the
    // staging buffers, and the runtime has taken its copy of the source by the time copy_from_caller returns)
    if (int e = replay_add_dev(h, h->stg_obs, h->stg_act, h->stg_rew, h->stg_next, h->stg_done, m)) return e;
  }
  return GRL_OK;
}

// ---------------------------------------------------------------------------------------------- observations uploaded once
// One env step's observations serve three consumers -- the running statistics, the next action and two replay rows
// (next_obs of this step, obs of the next).  grl_observe uploads them ONCE; grl_act (GRL_ACT_OBSERVED) and
// grl_replay_add_observed read the device copy.  The small per-step arrays of the latter (actions, rewards, done flags,
// terminal rows) pass through page-locked staging that the ingest launch reads directly: grl_ctx::ob_ring, two buffers used in
// turn, each guarded by an event (StagingRing, host_res.h).

// PPO / TRPO handles with normalize = 2: one upload of the raw rows and ONE launch per env step (ppo_observe_kernel) -- the
// statistics move (with the flag) and the normalised rows grl_ppo_step / grl_ppo_finish read with obs == NULL are written
static int ppo_observe(grl_handle h, const float* obs, int n, int flags) {
  if (n != h->NA) return fail(GRL_ERR_INVALID, "grl_observe on a PPO / TRPO handle takes the observations of all n_envs = " + std::to_string(h->NA) + " environments, got " + std::to_string(n));
  if (flags & ~GRL_OBSERVE_UPDATE_STATS) return fail(GRL_ERR_INVALID, "unknown flag bits");
  if (int e = copy_from_caller(h, h->n_stage, obs, (size_t)n * h->n_elems * 4)) return e;
  PpoObserveArgs a;
  memset(&a, 0, sizeof(a));
  a.nu.obs = h->n_stage; a.nu.n = n; a.nu.elems = (int)h->n_elems;
  a.nu.mean = h->n_mean; a.nu.var = h->n_var; a.nu.count = h->n_count; a.nu.parity = h->n_parity; a.nu.eps = ppo_norm_eps(h);
  a.sd = h->n_sd; a.out = h->ppo_obs_n; a.ldo = h->ppo_ldo; a.clip = (double)h->cfg.clip_obs;
  a.update = (flags & GRL_OBSERVE_UPDATE_STATS) ? 1 : 0;
  launch_ppo_observe(a, h->stream);
  if (a.update) h->n_parity ^= 1;
  HIPCHK(hipGetLastError());
  h->ppo_observed = true;
  return GRL_OK;
}

int grl_observe(grl_handle h, const float* obs, int n, int flags) {
  NOT_ON_PPO_WITHOUT_STATS(h, "grl_observe");
  NOT_ON_TD3(h, "grl_observe");
  if (!h || !obs || n < 1) return fail(GRL_ERR_INVALID, "bad argument");
  if (h->n_sd) return ppo_observe(h, obs, n, flags);
  if (!h->ob_latest) return fail(GRL_ERR_STATE, "this handle keeps no observed observations (SAC / DQN / BDQ handles do)");
  if (n > h->stg_n) return fail(GRL_ERR_INVALID, "more observations than one env step of act_batch environments");
  if (flags & ~GRL_OBSERVE_UPDATE_STATS) return fail(GRL_ERR_INVALID, "unknown flag bits");
  if ((flags & GRL_OBSERVE_UPDATE_STATS) && !h->n_mean) return fail(GRL_ERR_STATE, "this handle keeps no running statistics");
  if (flags & GRL_OBSERVE_UPDATE_STATS)
    if (int e = stats_update_refused(h)) return e;
  const size_t bytes = (size_t)n * h->ob_elems * 4;
  if (h->ob_n > 0)   // the previous step's observations become the `obs` side of the next replay rows
    HIPCHK(hipMemcpyAsync(h->ob_prev, h->ob_latest, (size_t)h->ob_n * h->ob_elems * 4, hipMemcpyDeviceToDevice, h->stream));
  h->ob_n_prev = h->ob_n;
  // (the caller's buffer goes to hipMemcpyAsync as it is, copy_from_caller; a bounce through page-locked staging of our own
  //  measured slower: 140 vs 126 us per env step of 16 observations, round 4)
  if (int e = copy_from_caller(h, h->ob_latest, obs, bytes)) return e;
  h->ob_n = n;
  if (flags & GRL_OBSERVE_UPDATE_STATS) return norm_update_from(h, h->ob_latest, n);
  return GRL_OK;
}

int grl_replay_add_observed(grl_handle h, const float* act, const float* rew, const float* done, int n,
                            const int32_t* term_rows, const float* term_obs, int n_term) {
  NOT_ON_PPO(h, "grl_replay_add_observed");
  NOT_ON_TD3(h, "grl_replay_add_observed");
  if (!h || !act || !rew || !done || n < 1 || n_term < 0 || n_term > n) return fail(GRL_ERR_INVALID, "bad argument");
  if (n_term > 0 && (!term_rows || !term_obs)) return fail(GRL_ERR_INVALID, "terminal rows without their observations");
  if (!h->ob_latest) return fail(GRL_ERR_STATE, "this handle keeps no observed observations (SAC / DQN / BDQ handles do)");
  if (h->ob_n != n || h->ob_n_prev != n)
    return fail(GRL_ERR_STATE, "grl_replay_add_observed needs two consecutive grl_observe calls of n observations each");
  for (int j = 0; j < n_term; ++j)     // (checked before the staging slot is taken: a refusal holds nothing and moves nothing)
    if (term_rows[j] < 0 || term_rows[j] >= n) return fail(GRL_ERR_INVALID, "terminal row out of range");
  float* pin = nullptr;
  HIPCHK(h->ob_ring.acquire((size_t)h->stg_n * (size_t)(h->ob_elems + h->A + 4), &pin));   // (waits for the copies that read it two calls ago)
  const int A = h->A;
  memcpy(pin, act, (size_t)n * A * 4);
  memcpy(pin + (size_t)n * A, rew, (size_t)n * 4);
  memcpy(pin + (size_t)n * (A + 1), done, (size_t)n * 4);
  int32_t* rowmap = (int32_t*)(pin + (size_t)n * (A + 2));
  for (int k = 0; k < n; ++k) rowmap[k] = -1;
  for (int j = 0; j < n_term; ++j) rowmap[term_rows[j]] = j;
  // (the ingest launch reads actions / rewards / done flags / row map straight from the page-locked buffer: 0.5 KB)
  const size_t small = (size_t)n * (A + 3);
  if (n_term > 0) {
    memcpy(pin + small, term_obs, (size_t)n_term * h->ob_elems * 4);
    HIPCHK(hipMemcpyAsync(h->ob_term, pin + small, (size_t)n_term * h->ob_elems * 4, hipMemcpyHostToDevice, h->stream));
  }
  const int e = replay_add_dev(h, h->ob_prev, pin, pin + (size_t)n * A, h->ob_latest, pin + (size_t)n * (A + 1), n,
                               n_term > 0 ? (const int*)(pin + (size_t)n * (A + 2)) : nullptr, h->ob_term);
  HIPCHK(h->ob_ring.release(h->stream));          // (the event follows the launch that reads the buffer)
  return e;
}

int64_t grl_replay_size(grl_handle h) {
  NOT_ON_PPO(h, "grl_replay_size");
  return h ? h->rp_size : -1;
}

static int stage_noise(grl_handle h, const int64_t* idx, const float* eps, int step) {
  HIPCHK(hipMemcpyAsync(h->idx_buf, idx + (int64_t)step * h->B, (size_t)h->B * 8, hipMemcpyDeviceToDevice, h->stream));
  const int64_t per = h->cfg.algo == GRL_ALGO_SAC ? (int64_t)h->B * h->A : (int64_t)h->B;   // Q: importance weights
  HIPCHK(hipMemcpyAsync(h->eps_buf, eps + (int64_t)step * per, (size_t)per * 4, hipMemcpyDeviceToDevice, h->stream));
  return GRL_OK;
}

int grl_compute_grads(grl_handle h, const int64_t* idx, const float* eps) {
  NOT_ON_PPO(h, "grl_compute_grads");
  NOT_ON_TD3(h, "grl_compute_grads");
  if (!h) return fail(GRL_ERR_INVALID, "null handle");
  if ((idx == nullptr) != (eps == nullptr)) return fail(GRL_ERR_INVALID, "idx and eps must both be given or both be NULL");
  if (h->rp_size < 1) return fail(GRL_ERR_STATE, "replay buffer is empty");
  if (idx) {
    if (int e = stage_noise(h, idx, eps, 0)) return e;
    if (int e = h->run_seq("grads_explicit", {&h->ops_gather, &h->ops_grads})) return e;
  } else {
    if (int e = h->run_seq("grads_rng", {&h->ops_rng, &h->ops_grads})) return e;
  }
  HIPCHK(hipGetLastError());
  return GRL_OK;
}

int grl_compute_grads_staged(grl_handle h, int stage, const int64_t* idx, const float* eps) {
  NOT_ON_PPO(h, "grl_compute_grads_staged");
  NOT_ON_TD3(h, "grl_compute_grads_staged");
  if (!h) return fail(GRL_ERR_INVALID, "null handle");
  if (stage != 0 && stage != 1) return fail(GRL_ERR_INVALID, "stage must be 0 or 1");
  if (!h->staged_ok) {          // plans without a staged form: everything in stage 0, one bucket (grl_grad_ranges)
    if (stage == 1) return GRL_OK;
    return grl_compute_grads(h, idx, eps);
  }
  if (stage == 1) {
    if (int e = h->run_seq("grads_stage1", {&h->ops_stage1})) return e;
    HIPCHK(hipGetLastError());
    return GRL_OK;
  }
  if ((idx == nullptr) != (eps == nullptr)) return fail(GRL_ERR_INVALID, "idx and eps must both be given or both be NULL");
  if (h->rp_size < 1) return fail(GRL_ERR_STATE, "replay buffer is empty");
  if (idx) {
    if (int e = stage_noise(h, idx, eps, 0)) return e;
    if (int e = h->run_seq("grads_stage0_explicit", {&h->ops_gather, &h->ops_stage0})) return e;
  } else {
    if (int e = h->run_seq("grads_stage0_rng", {&h->ops_rng, &h->ops_stage0})) return e;
  }
  HIPCHK(hipGetLastError());
  return GRL_OK;
}

int grl_grad_ranges(grl_handle h, int bucket, int cap, int64_t* offsets, int64_t* numels) {
  NOT_ON_PPO(h, "grl_grad_ranges");
  NOT_ON_TD3(h, "grl_grad_ranges");
  if (!h || !offsets || !numels) return fail(GRL_ERR_INVALID, "null argument");
  if (bucket != 0 && bucket != 1) return fail(GRL_ERR_INVALID, "bucket must be 0 or 1");
  std::vector<std::pair<int64_t, int64_t>> r;
  if (!h->staged_ok) {
    if (bucket == 0) r.push_back({0, h->n_train});
  } else if (bucket == 0) {      // dense: fc + heads of the policy net, fc + vf / qf1 / qf2 heads of the value net
    r.push_back({h->ex[0].fw, h->vf_off - h->ex[0].fw});
    r.push_back({h->ex[1].fw, h->ent_off - h->ex[1].fw});
  } else {                       // convolutions of both nets + the entropy coefficient (its gradient comes with the loss sums)
    r.push_back({h->ex[0].w[0], h->ex[0].fw - h->ex[0].w[0]});
    r.push_back({h->ex[1].w[0], h->ex[1].fw - h->ex[1].w[0]});
    r.push_back({h->ent_off, h->n_train - h->ent_off});
  }
  if ((int)r.size() > cap) return fail(GRL_ERR_INVALID, "range buffer too small");
  for (size_t k = 0; k < r.size(); ++k) { offsets[k] = r[k].first; numels[k] = r[k].second; }
  return (int)r.size();
}

int grl_apply_grads(grl_handle h, float grad_scale) {
  NOT_ON_PPO(h, "grl_apply_grads");
  NOT_ON_TD3(h, "grl_apply_grads");
  if (!h) return fail(GRL_ERR_INVALID, "null handle");
  if (grad_scale != h->apply_graph_scale) {   // the scale is baked into the captured kernel arguments
    auto it = h->graphs.find("apply");
    if (it != h->graphs.end()) { (void)hipGraphExecDestroy(it->second); h->graphs.erase(it); }
    h->apply_graph_scale = grad_scale;
  }
  h->grad_scale = grad_scale;
  if (int e = h->run_seq("apply", {&h->ops_apply})) return e;
  HIPCHK(hipGetLastError());
  return GRL_OK;
}

int grl_train_step(grl_handle h, int n_steps, const int64_t* idx, const float* eps) {
  NOT_ON_PPO(h, "grl_train_step");
  NOT_ON_TD3(h, "grl_train_step");
  if (!h || n_steps < 1) return fail(GRL_ERR_INVALID, "bad argument");
  if (h->cfg.algo == GRL_ALGO_AE) return fail(GRL_ERR_STATE, "auto-encoder handles train with grl_ae_train_step");
  if ((idx == nullptr) != (eps == nullptr)) return fail(GRL_ERR_INVALID, "idx and eps must both be given or both be NULL");
  if (h->rp_size < 1) return fail(GRL_ERR_STATE, "replay buffer is empty");
  h->grad_scale = 1.f;
  // device RNG, several updates: work of update t + 1 rides on a launch of update t where the plan has such sequences (plan_sac
  // "gather_ride" with double-buffered images, else "prefetch"; plan_q "q_pf" for uniform replay)
  const bool call = !idx && n_steps >= 2 && !h->prof;
  int e = GRL_OK;
  if (call && h->ride.ok()) e = h->run_call("ride", h->ride, n_steps);
  else if (call && h->pf.ok()) e = h->run_call("pf", h->pf, n_steps);
  else if (call && h->q_pf.ok()) e = h->run_call("q_pf", h->q_pf, n_steps);
  else if (!idx) e = h->run_repeated("full_rng", h->update_seq(&h->ops_rng), n_steps);      // identical updates, several to a graph
  else
    for (int s = 0; s < n_steps && !e; ++s)
      if (!(e = stage_noise(h, idx, eps, s))) e = h->run_seq("full_explicit", h->update_seq(&h->ops_gather));
  if (e) return e;
  HIPCHK(hipGetLastError());
  return GRL_OK;
}

int grl_train_step_per(grl_handle h, int n_steps, double beta, const double* u) {
  NOT_ON_PPO(h, "grl_train_step_per");
  NOT_ON_TD3(h, "grl_train_step_per");
  if (!h || n_steps < 1) return fail(GRL_ERR_INVALID, "bad argument");
  if (!h->per_on) return fail(GRL_ERR_STATE, "prioritised replay is not enabled (grl_config.q_per)");
  if (h->rp_size < 1) return fail(GRL_ERR_STATE, "replay buffer is empty");
  if (!(beta > 0.0)) return fail(GRL_ERR_INVALID, "beta must be positive (PrioritizedReplayBuffer.sample asserts beta > 0)");
  if (h->rp_size < 2) return fail(GRL_ERR_STATE, "prioritised sampling needs at least two stored transitions (sum(0, len - 1))");
  HIPCHK(hipMemcpyAsync(&h->per.st->beta, &beta, 8, hipMemcpyHostToDevice, h->stream));
  h->grad_scale = 1.f;
  if (h->dp_on) {
    // connected handle (grl_allreduce_connect): every rank draws from ITS priority tree (importance weights against its own
    // total and minimum), the gradient sums are exchanged inside the graph, the plan's clip + Adam apply the mean, every rank
    // writes the priorities of its own rows back.  All ranks must call alike, as with grl_train_step_allreduce.
    if (*h->dp_err_host.get()) return fail(GRL_ERR_STATE, "an exchange timed out waiting for a peer (the replicas are no longer in step)");
    h->grad_scale = 1.f / (float)h->dp.world;
    if (!u) {
      if (int e = h->run_repeated("dp_per_rng", {&h->ops_per_rng_g, &h->dp_body_per, &h->ops_dp, &h->ops_per_update}, n_steps)) return e;
    } else {
      for (int s = 0; s < n_steps; ++s) {
        HIPCHK(hipMemcpyAsync(h->per_u, u + (int64_t)s * h->B, (size_t)h->B * 8, hipMemcpyDeviceToDevice, h->stream));
        if (int e = h->run_seq("dp_per_u", {&h->ops_per_u_g, &h->dp_body_per, &h->ops_dp, &h->ops_per_update})) return e;
      }
    }
    HIPCHK(hipGetLastError());
    return GRL_OK;
  }
  if (!u) {        // device Philox: identical updates, several to a graph
    if (n_steps >= 2 && h->per_pf.ok() && !h->prof) {
      // four launches per update (plan_q "per_pf"): the sampler of update t + 1 rides on the launch that ends update t
      if (int e = h->run_call("per_pf", h->per_pf, n_steps)) return e;
    } else if (n_steps >= 2 && !h->ops_grads_apply_per_r.empty() && !h->prof) {
      // nothing but the updates themselves touches the leaves inside one call: the first update sums every block of the
      // ring, each apply launch refreshes the blocks its write-back touched, the later samplers start from those
      if (int e = h->run_seq("per_rng_first", {&h->ops_per_rng_g, &h->ops_grads_apply_per_r})) return e;
      if (int e = h->run_repeated("per_rng_inc", {&h->ops_per_rng_g_inc, &h->ops_grads_apply_per_r}, n_steps - 1)) return e;
    } else if (int e = h->run_repeated("per_rng", h->per_update_seq(true), n_steps)) return e;
    HIPCHK(hipGetLastError());
    return GRL_OK;
  }
  for (int s = 0; s < n_steps; ++s) {
    HIPCHK(hipMemcpyAsync(h->per_u, u + (int64_t)s * h->B, (size_t)h->B * 8, hipMemcpyDeviceToDevice, h->stream));
    if (int e = h->run_seq("per_u", h->per_update_seq(false))) return e;
  }
  HIPCHK(hipGetLastError());
  return GRL_OK;
}

int grl_ae_train_step(grl_handle h, const float* imgs, int n_steps) {
  NOT_ON_PPO(h, "grl_ae_train_step");
  if (!h || !imgs || n_steps < 1) return fail(GRL_ERR_INVALID, "bad argument");
  if (h->cfg.algo != GRL_ALGO_AE) return fail(GRL_ERR_STATE, "not an auto-encoder handle (grl_config.algo)");
  const size_t per = (size_t)h->B * 4096;
  for (int s = 0; s < n_steps; ++s) {
    HIPCHK(hipMemcpyAsync(h->ae_x, imgs + per * s, per * 4, hipMemcpyDeviceToDevice, h->stream));
    if (int e = h->run_seq("ae_step", {&h->ops_ae})) return e;
  }
  HIPCHK(hipGetLastError());
  return GRL_OK;
}

int grl_ae_reconstruct(grl_handle h, const float* imgs, float* out) {
  NOT_ON_PPO(h, "grl_ae_reconstruct");
  if (!h || !imgs || !out) return fail(GRL_ERR_INVALID, "null argument");
  if (h->cfg.algo != GRL_ALGO_AE) return fail(GRL_ERR_STATE, "not an auto-encoder handle (grl_config.algo)");
  const size_t per = (size_t)h->B * 4096;
  HIPCHK(hipMemcpyAsync(h->ae_x, imgs, per * 4, hipMemcpyDeviceToDevice, h->stream));
  if (int e = h->run_seq("ae_fwd", {&h->ops_ae_fwd})) return e;
  HIPCHK(hipMemcpyAsync(out, h->ae_out, per * 4, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipGetLastError());
  return GRL_OK;
}

int grl_get_metrics(grl_handle h, grl_metrics* out) {
  NOT_ON_TD3(h, "grl_get_metrics");
  if (!h || !out) return fail(GRL_ERR_INVALID, "null argument");
  DevScalars s;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(&s, h->sc, sizeof(s), hipMemcpyDeviceToHost));
  out->policy_loss = s.policy_loss; out->qf1_loss = s.qf1_loss; out->qf2_loss = s.qf2_loss;
  out->value_loss = s.value_loss; out->ent_coef_loss = s.ent_loss; out->ent_coef = s.ent_coef;
  out->entropy = s.entropy; out->mean_qf1 = s.mean_qf1; out->mean_v = s.mean_v;
  return GRL_OK;
}

// the completion of the act path's last launch: poll its counter in coherent host memory (bounded -- after 2 ms, or on any
// doubt, the stream is synchronised) or, without a counter / under grl_profile_enable, synchronise the stream
static int act_wait(grl_handle h, unsigned wgs) {
  const bool poll = wgs && !h->prof;
  bool seen = false;
  if (wgs) h->act_done_seen += wgs;
  if (poll) {
    const unsigned want = h->act_done_seen;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 0;; ++spin) {
      if ((int)(__atomic_load_n(h->act_done_host.get(), __ATOMIC_ACQUIRE) - want) >= 0) { seen = true; break; }
      if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
  }
  if (!seen) {
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->act_done_host.get()) h->act_done_seen = __atomic_load_n(h->act_done_host.get(), __ATOMIC_ACQUIRE);
  }
  HIPCHK(hipGetLastError());
  return GRL_OK;
}

// grl_act(GRL_ACT_GREEDY) on a DQN / BDQ handle: bins [n, D] (plan_q.inl; q_act.h).  Observations, overrides and bins live
// in coherent host memory the launch reads and writes: the previous call has waited for its launch, so they are free
// raw: VecNormalize applied on the device; observed: the rows grl_observe uploaded (nothing but the overrides moves)
static int act_greedy(grl_handle h, const float* obs, int n, const float* explore, float* out, bool raw, bool observed) {
  if (!h->q_io_host.get()) return fail(GRL_ERR_STATE, "this handle has no act path");
  const int D = h->qD, od = h->cfg.obs_dim;
  float* io_obs = h->q_io_host.get(); float* io_explore = io_obs + (size_t)h->NA * od; float* io_bins = io_explore + (size_t)h->NA * D;
  if (observed) {}
  else if (h->q_act_fused) memcpy(io_obs, obs, (size_t)n * od * 4);
  else {
    if (int e = pin_reserve(h, (size_t)n * od, 0)) return e;
    memcpy(h->pin_in.get(), obs, (size_t)n * od * 4);
    HIPCHK(hipMemcpyAsync(h->stg_obs, h->pin_in.get(), (size_t)n * od * 4, hipMemcpyHostToDevice, h->stream));
  }
  if (explore) memcpy(io_explore, explore, (size_t)n * D * 4);
  else for (int i = 0; i < n * D; ++i) io_explore[i] = -1.f;
  __atomic_thread_fence(__ATOMIC_RELEASE);
  const int v = (observed ? 2 : 0) | (raw ? 1 : 0);
  if (int e = h->run_seq(v ? std::string("act_greedy") + char('0' + v) : std::string("act_greedy"), {&h->ops_act_greedy[v]})) return e;
  if (int e = act_wait(h, h->q_greedy_wgs)) return e;
  memcpy(out, io_bins, (size_t)n * D * 4);
  return GRL_OK;
}


// ---------------------------------------------------------------------------------------------- PPO2 (plan_ppo.inl)
// what one env step sends, packed into page-locked staging and copied once: observations [NA, ldo] (rows padded, padding zero) |
// done [NA] | eps [NA, A] | rewards [NA] (the layout of grl_ctx::ppo_in)
static int ppo_send(grl_handle h, const float* obs, const float* done, const float* eps, int n) {
  const int NA = h->NA, ldo = h->ppo_ldo, od = h->cfg.obs_dim, A = h->A;
  const size_t n_in = (size_t)NA * (ldo + 1 + A);
  if (int e = pin_reserve(h, (size_t)NA * (ldo + 2 + A), (size_t)NA * (A + 2))) return e;
  // (the previous call synchronised the stream behind its copy: the staging buffer is free)
  // obs == NULL (grl_ppo_step / grl_ppo_finish on the rows grl_observe normalised): done | eps alone travel
  const size_t lo = obs ? 0 : (size_t)NA * ldo;
  memset(h->pin_in.get() + lo, 0, (n_in - lo) * 4);
  for (int r = 0; obs && r < n; ++r) memcpy(h->pin_in.get() + (size_t)r * ldo, obs + (size_t)r * od, (size_t)od * 4);
  if (done) memcpy(h->pin_in.get() + (size_t)NA * ldo, done, (size_t)n * 4);
  if (eps) memcpy(h->pin_in.get() + (size_t)NA * (ldo + 1), eps, (size_t)n * A * 4);
  HIPCHK(hipMemcpyAsync(h->ppo_in + lo, h->pin_in.get() + lo, (n_in - lo) * 4, hipMemcpyHostToDevice, h->stream));
  return GRL_OK;
}
// ... and what it returns: action [NA, A] | value [NA] | neglogp [NA]; synchronises
static int ppo_receive(grl_handle h, int n, float* out_act, float* out_val, float* out_nlp) {
  const int NA = h->NA, A = h->A;
  HIPCHK(hipMemcpyAsync(h->pin_out.get(), h->ppo_out, (size_t)NA * (A + 2) * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  if (out_act) memcpy(out_act, h->pin_out.get(), (size_t)n * A * 4);
  if (out_val) memcpy(out_val, h->pin_out.get() + (size_t)NA * A, (size_t)n * 4);
  if (out_nlp) memcpy(out_nlp, h->pin_out.get() + (size_t)NA * (A + 1), (size_t)n * 4);
  return GRL_OK;
}
#define PPO_ONLY(h, what)                                                                                        \
  do {                                                                                                           \
    if (!(h)) return fail(GRL_ERR_INVALID, "null handle");                                                       \
    if ((h)->cfg.algo != GRL_ALGO_PPO) return fail(GRL_ERR_STATE, what " is defined for PPO handles (grl_ppo_create)"); \
  } while (0)
// the rollout calls serve both kinds of handle that keep one (a TRPO handle: one environment)
#define ROLLOUT_ONLY(h, what)                                                                                    \
  do {                                                                                                           \
    if (!(h)) return fail(GRL_ERR_INVALID, "null handle");                                                       \
    if ((h)->cfg.algo != GRL_ALGO_PPO && (h)->cfg.algo != GRL_ALGO_TRPO)                                         \
      return fail(GRL_ERR_STATE, what " is defined for PPO and TRPO handles (grl_ppo_create, grl_trpo_create)");  \
  } while (0)
#define TRPO_ONLY(h, what)                                                                                       \
  do {                                                                                                           \
    if (!(h)) return fail(GRL_ERR_INVALID, "null handle");                                                       \
    if ((h)->cfg.algo != GRL_ALGO_TRPO) return fail(GRL_ERR_STATE, what " is defined for TRPO handles (grl_trpo_create)"); \
  } while (0)

static int ppo_act(grl_handle h, const float* obs, int n, int flags, const float* eps, float* out) {
  if (flags & ~GRL_ACT_DETERMINISTIC) return fail(GRL_ERR_STATE, "a PPO handle acts on the observations handed to it: GRL_ACT_RAW_OBS / GRL_ACT_OBSERVED / GRL_ACT_GREEDY are not defined on it");
  if (!obs) return fail(GRL_ERR_INVALID, "bad argument");
  if (n > h->NA) return fail(GRL_ERR_INVALID, "n exceeds act_batch");
  const int v = (flags & GRL_ACT_DETERMINISTIC) ? 0 : (eps ? 1 : 2);
  if (int e = ppo_send(h, obs, nullptr, v == 1 ? eps : nullptr, n)) return e;
  static const char* key[3] = {"ppo_act_det", "ppo_act_eps", "ppo_act_rng"};
  if (int e = h->run_seq(key[v], {&h->ops_ppo_act[v]})) return e;
  return ppo_receive(h, n, out, nullptr, nullptr);
}

// obs == NULL: "the rows the last grl_observe normalised"
static int ppo_observed_rows(grl_handle h, const char* what) {
  if (!h->n_sd) return fail(GRL_ERR_STATE, std::string(what) + ": obs is NULL, and this handle was created with normalize = 0 (it normalises no observations: hand them over)");
  if (!h->ppo_observed) return fail(GRL_ERR_STATE, std::string(what) + ": obs is NULL, and no grl_observe call has normalised any rows yet");
  return GRL_OK;
}

int grl_ppo_step(grl_handle h, const float* obs, const float* done, const float* eps, float* out_act, float* out_val, float* out_nlp) {
  ROLLOUT_ONLY(h, "grl_ppo_step");
  if (!done || !out_act || !out_val || !out_nlp) return fail(GRL_ERR_INVALID, "null argument");
  if (!obs)
    if (int e = ppo_observed_rows(h, "grl_ppo_step")) return e;
  if (h->ppo_stepped >= h->pcfg.n_steps) return fail(GRL_ERR_STATE, "the rollout is full: grl_ppo_finish and grl_ppo_train empty it");
  if (h->ppo_stepped != h->ppo_closed) return fail(GRL_ERR_STATE, "the previous slot is still open: grl_ppo_rewards closes it");
  if (int e = ppo_send(h, obs, done, eps, h->NA)) return e;
  if (obs) {
    if (int e = h->run_seq(eps ? "ppo_step_eps" : "ppo_step_rng", {&h->ops_ppo_step[eps ? 0 : 1]})) return e;
  } else {
    if (int e = h->run_seq(eps ? "ppo_step_eps_n" : "ppo_step_rng_n", {&h->ops_ppo_step_n[eps ? 0 : 1]})) return e;
  }
  if (int e = ppo_receive(h, h->NA, out_act, out_val, out_nlp)) return e;
  h->ppo_stepped += 1;
  h->ppo_finished = false;
  h->ppo_held = h->gail_rewritten = false;      // (a GAIL session: the last full rollout is being overwritten)
  return GRL_OK;
}

int grl_ppo_rewards(grl_handle h, const float* rew, int n) {
  ROLLOUT_ONLY(h, "grl_ppo_rewards");
  if (!rew || n != h->NA) return fail(GRL_ERR_INVALID, "grl_ppo_rewards takes n_envs rewards");
  if (h->ppo_stepped != h->ppo_closed + 1) return fail(GRL_ERR_STATE, "no open slot: grl_ppo_step opens one");
  if (int e = copy_from_caller(h, h->ppo_in + (size_t)h->NA * (h->ppo_ldo + 1 + h->A), rew, (size_t)n * 4)) return e;
  if (int e = h->run_seq("ppo_rewards", {&h->ops_ppo_rew})) return e;
  HIPCHK(hipGetLastError());
  h->ppo_closed += 1;
  return GRL_OK;
}

int grl_ppo_finish(grl_handle h, const float* last_obs, const float* last_done) {
  ROLLOUT_ONLY(h, "grl_ppo_finish");
  if (!last_done) return fail(GRL_ERR_INVALID, "null argument");
  if (!last_obs)
    if (int e = ppo_observed_rows(h, "grl_ppo_finish")) return e;
  if (h->ppo_closed != h->pcfg.n_steps) return fail(GRL_ERR_STATE, "the rollout is not full: n_steps slots must be closed before grl_ppo_finish");
  if (int e = ppo_send(h, last_obs, last_done, nullptr, h->NA)) return e;
  if (int e = last_obs ? h->run_seq("ppo_finish", {&h->ops_ppo_finish}) : h->run_seq("ppo_finish_n", {&h->ops_ppo_finish_n})) return e;
  // (the staging buffer of ppo_send is reused by the next call: wait for its copy, as every per-step call does)
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  h->ppo_finished = h->ppo_held = true;
  return GRL_OK;
}

// every row of perm [rows, R] a permutation of 0..R-1 (grl_ppo_train, grl_trpo_update)
static int check_perm_rows(const int32_t* perm, int rows, int64_t R) {
  std::vector<uint8_t> seen((size_t)R);
  for (int e = 0; e < rows; ++e) {
    std::fill(seen.begin(), seen.end(), 0);
    for (int64_t i = 0; i < R; ++i) {
      const int32_t v = perm[(int64_t)e * R + i];
      if (v < 0 || v >= R || seen[(size_t)v]) return fail(GRL_ERR_INVALID, "perm row " + std::to_string(e) + " is no permutation of 0.." + std::to_string(R - 1));
      seen[(size_t)v] = 1;
    }
  }
  return GRL_OK;
}

int grl_ppo_train(grl_handle h, const int32_t* perm, int noptepochs) {
  PPO_ONLY(h, "grl_ppo_train");
  if (!perm || noptepochs < 1 || noptepochs > GRL_PPO_MAX_EPOCHS)
    return fail(GRL_ERR_INVALID, "grl_ppo_train takes 1.." + std::to_string(GRL_PPO_MAX_EPOCHS) + " permutations");
  if (!h->ppo_finished) return fail(GRL_ERR_STATE, "no finished rollout: grl_ppo_finish forms the advantages grl_ppo_train reads");
  const int64_t R = (int64_t)h->pcfg.n_envs * h->pcfg.n_steps;
  if (int e = check_perm_rows(perm, noptepochs, R)) return e;
  if (int e = copy_from_caller(h, h->ppo_perm, perm, (size_t)noptepochs * R * 4)) return e;
  HIPCHK(hipMemsetAsync(&h->ppo_dev->cursor, 0, 4, h->stream));
  const int n_updates = noptepochs * (int)(R / h->cfg.batch_size);
  if (int e = h->run_repeated("ppo_update", {&h->ops_ppo_update}, n_updates)) return e;
  HIPCHK(hipMemsetAsync(&h->ppo_dev->slot, 0, 4, h->stream));      // the rollout is empty again
  HIPCHK(hipGetLastError());
  h->ppo_updates = n_updates;
  h->ppo_stepped = h->ppo_closed = 0;
  h->ppo_finished = false;
  return GRL_OK;
}

int grl_ppo_get_metrics(grl_handle h, float* out, int cap) {
  PPO_ONLY(h, "grl_ppo_get_metrics");
  if (!out) return fail(GRL_ERR_INVALID, "null argument");
  const int nu = h->ppo_updates, nb = h->ppo_nblk, mb = h->cfg.batch_size;
  if (cap < nu * PPO_DIAG) return fail(GRL_ERR_INVALID, "metrics buffer too small");
  std::vector<float> part((size_t)std::max(1, nu * nb * PPO_DIAG));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (nu) HIPCHK(hipMemcpy(part.data(), h->ppo_diag, (size_t)nu * nb * PPO_DIAG * 4, hipMemcpyDeviceToHost));
  for (int u = 0; u < nu; ++u) {
    float s[PPO_DIAG] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < nb; ++b)      // the per-block sums of the loss launch, in index order
      for (int k = 0; k < PPO_DIAG; ++k) s[k] += part[((size_t)u * nb + b) * PPO_DIAG + k];
    float* o = out + (size_t)u * PPO_DIAG;
    o[0] = s[0] / (float)mb; o[1] = 0.5f * (s[1] / (float)mb); o[2] = s[2]; o[3] = 0.5f * (s[3] / (float)mb); o[4] = s[4] / (float)mb;
  }
  return nu;
}

// ---------------------------------------------------------------------------------------------- TRPO (plan_trpo.inl)
int grl_trpo_update(grl_handle h, const int32_t* vf_perm, int vf_iters) {
  TRPO_ONLY(h, "grl_trpo_update");
  if (vf_iters < 0 || vf_iters > GRL_PPO_MAX_EPOCHS || (vf_iters > 0 && !vf_perm))
    return fail(GRL_ERR_INVALID, "grl_trpo_update takes 0.." + std::to_string(GRL_PPO_MAX_EPOCHS) + " permutations");
  if (!h->ppo_finished) return fail(GRL_ERR_STATE, "no finished rollout: grl_ppo_finish forms the advantages grl_trpo_update reads");
  const int64_t T = h->tcfg.n_steps, B = h->tcfg.vf_batch, per = T / B;
  if (int e = check_perm_rows(vf_perm, vf_iters, T)) return e;
  const int n_vf = (int)(vf_iters * per);
  if (n_vf > 0) {      // the minibatches of every row back to back (the tail of a row is dropped): minibatch u takes [u B, (u + 1) B)
    std::vector<int32_t> packed((size_t)n_vf * B);
    for (int e = 0; e < vf_iters; ++e) memcpy(packed.data() + (size_t)e * per * B, vf_perm + (size_t)e * T, (size_t)(per * B) * 4);
    // (`packed` is pageable: copy_from_caller has staged it when it returns, as it does grl_ppo_train's caller buffer)
    if (int e = copy_from_caller(h, h->ppo_perm, packed.data(), packed.size() * 4)) return e;
  }
  HIPCHK(hipMemsetAsync(&h->ppo_dev->cursor, 0, 4, h->stream));
  if (int e = h->run_seq("trpo_policy", {&h->ops_trpo_policy})) return e;
  if (n_vf > 0)
    if (int e = h->run_repeated("trpo_vf", {&h->ops_trpo_vf}, n_vf)) return e;
  HIPCHK(hipMemsetAsync(&h->ppo_dev->slot, 0, 4, h->stream));      // the rollout is empty again
  HIPCHK(hipGetLastError());
  h->ppo_updates = n_vf;
  h->ppo_stepped = h->ppo_closed = 0;
  h->ppo_finished = false;
  return GRL_OK;
}

int grl_trpo_get_metrics(grl_handle h, float* out, int cap) {
  TRPO_ONLY(h, "grl_trpo_get_metrics");
  if (!out) return fail(GRL_ERR_INVALID, "null argument");
  if (cap < GRL_TRPO_METRICS) return fail(GRL_ERR_INVALID, "metrics buffer too small");
  TrpoDev d;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(&d, h->trpo_dev, sizeof(d), hipMemcpyDeviceToHost));
  for (int k = 0; k < 5; ++k) out[k] = d.before[k];
  out[5] = (float)d.ls_index; out[6] = d.trial[0]; out[7] = d.trial[1];
  out[8] = (float)d.cg_iters; out[9] = d.rr[std::max(0, std::min(d.cg_iters, GRL_TRPO_MAX_CG))]; out[10] = d.shs;
  return GRL_TRPO_METRICS;
}

int grl_trpo_debug_fvp(grl_handle h) {
  TRPO_ONLY(h, "grl_trpo_debug_fvp");
  if (h->ppo_closed != h->pcfg.n_steps) return fail(GRL_ERR_STATE, "the rollout is not full: the Fisher rows are taken from it");
  if (int e = h->run_seq("trpo_fvp", {&h->ops_trpo_fvp})) return e;
  HIPCHK(hipGetLastError());
  return GRL_OK;
}

// ---------------------------------------------------------------------------------------------- TD3 (plan_td3.inl)
#define TD3_ONLY(h, what)                                                                                        \
  do {                                                                                                           \
    if (!(h)) return fail(GRL_ERR_INVALID, "null handle");                                                       \
    if ((h)->cfg.algo != GRL_ALGO_TD3) return fail(GRL_ERR_STATE, what " is defined for TD3 handles (grl_td3_create)"); \
  } while (0)

int grl_td3_train(grl_handle h, int n_updates, const int64_t* idx, const float* eps, int64_t first_step) {
  TD3_ONLY(h, "grl_td3_train");
  if (n_updates < 1 || n_updates > GRL_TD3_MAX_UPDATES) return fail(GRL_ERR_INVALID, "grl_td3_train takes 1.." + std::to_string(GRL_TD3_MAX_UPDATES) + " updates per call");
  if (first_step < 0) return fail(GRL_ERR_INVALID, "first_step must be >= 0");
  if (h->rp_size < 1) return fail(GRL_ERR_STATE, "replay buffer is empty");
  const int64_t delay = h->td3cfg.policy_delay;
  auto policy = [&](int u) { return (first_step + u) % delay == 0 ? 1 : 0; };
  const int v = (idx ? 0 : 1) | (eps ? 0 : 2);
  // cursor -1 (td3_smooth advances it in front of every loss launch); the last policy loss of the call before becomes the carried one
  launch_td3_carry(h->td3_dev, h->td3_part, h->td3_nblk, h->cfg.batch_size, h->stream);
  h->td3_last_n = n_updates;
  h->td3_first_step = first_step;
  const int64_t per = (int64_t)h->B * h->A;
  if (v != 3 || h->prof) {      // something handed over (or profiling): update by update
    for (int u = 0; u < n_updates; ++u) {
      if (idx) HIPCHK(hipMemcpyAsync(h->idx_buf, idx + (int64_t)u * h->B, (size_t)h->B * 8, hipMemcpyDeviceToDevice, h->stream));
      if (eps) HIPCHK(hipMemcpyAsync(h->eps_buf, eps + (int64_t)u * per, (size_t)per * 4, hipMemcpyDeviceToDevice, h->stream));
      const int p = policy(u);
      if (int e = h->run_seq(std::string("td3_v") + char('0' + v) + (p ? "_policy" : "_critic"), {&h->ops_td3[p][v]})) return e;
    }
  } else {
    // everything drawn on the device: groups of up to `graph_updates` updates (powers of two) go out as ONE linear graph, keyed
    // by the phase of its first update in the policy_delay cycle
    const int limit = h->graphs_on() ? grl_ctx::max_group() : 1;
    for (int u = 0; u < n_updates;) {
      int group = 1;
      while (2 * group <= limit && 2 * group <= n_updates - u) group *= 2;
      std::vector<std::vector<Op>*> seq;
      for (int g = 0; g < group; ++g) seq.push_back(&h->ops_td3[policy(u + g)][3]);
      const std::string key = "td3_rng_ph" + std::to_string((first_step + u) % delay) + (group > 1 ? "_x" + std::to_string(group) : "");
      if (int e = h->run_seq(key, seq)) return e;
      u += group;
    }
  }
  HIPCHK(hipGetLastError());
  return GRL_OK;
}

int grl_td3_get_metrics(grl_handle h, float* out, int cap) {
  TD3_ONLY(h, "grl_td3_get_metrics");
  if (!out) return fail(GRL_ERR_INVALID, "null argument");
  const int nu = h->td3_last_n, nb = h->td3_nblk;
  if (cap < nu * GRL_TD3_METRICS) return fail(GRL_ERR_INVALID, "metrics buffer too small");
  std::vector<float> part((size_t)std::max(1, nu * nb * TD3_DIAG));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (nu) HIPCHK(hipMemcpy(part.data(), h->td3_part, (size_t)nu * nb * TD3_DIAG * 4, hipMemcpyDeviceToHost));
  Td3Dev dev;
  HIPCHK(hipMemcpy(&dev, h->td3_dev, sizeof(dev), hipMemcpyDeviceToHost));
  const float B = (float)h->cfg.batch_size;
  float pl = dev.pl_carry;      // the handle's last policy update before this call, whether or not its metrics were fetched
  for (int u = 0; u < nu; ++u) {
    float s[TD3_DIAG] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < nb; ++b)      // the per-block sums of the loss launch, in index order
      for (int k = 0; k < TD3_DIAG; ++k) s[k] += part[((size_t)u * nb + b) * TD3_DIAG + k];
    const bool policy = (h->td3_first_step + u) % h->td3cfg.policy_delay == 0;
    if (policy) pl = s[2] / B;
    float* o = out + (size_t)u * GRL_TD3_METRICS;
    o[0] = s[0] / B; o[1] = s[1] / B; o[2] = pl; o[3] = s[3] / B; o[4] = s[4] / B; o[5] = policy ? 1.f : 0.f;
  }
  return nu;
}

int grl_act(grl_handle h, const float* obs, int n, int flags, const float* eps, float* out) {
  if (!h || !out || n < 1) return fail(GRL_ERR_INVALID, "bad argument");
  if (flags & ~(GRL_ACT_DETERMINISTIC | GRL_ACT_RAW_OBS | GRL_ACT_OBSERVED | GRL_ACT_GREEDY)) return fail(GRL_ERR_INVALID, "unknown flag bits");
  if (h->cfg.algo == GRL_ALGO_PPO || h->cfg.algo == GRL_ALGO_TRPO) return ppo_act(h, obs, n, flags, eps, out);
  const int deterministic = flags & GRL_ACT_DETERMINISTIC;
  const bool raw = (flags & GRL_ACT_RAW_OBS) != 0;        // raw observations: VecNormalize applied on the device (grl_norm_update statistics)
  const bool observed = (flags & GRL_ACT_OBSERVED) != 0;  // act on what grl_observe uploaded: no second upload
  const bool td3 = h->cfg.algo == GRL_ALGO_TD3;            // pi(obs): no noise is read, both flag values give the same action
  const bool q = h->cfg.algo != GRL_ALGO_SAC && !td3;   // DQN / BDQ: Q-values [n, D*bins]
  if (td3 && observed) return fail(GRL_ERR_STATE, "GRL_ACT_OBSERVED is not defined on a TD3 handle (grl_observe is not)");
  if (!observed && !obs) return fail(GRL_ERR_INVALID, "bad argument");
  if (q && (raw || observed) && !(flags & GRL_ACT_GREEDY))
    return fail(GRL_ERR_STATE, "the Q-value form of grl_act takes normalised observations handed to it (GRL_ACT_GREEDY accepts GRL_ACT_RAW_OBS / GRL_ACT_OBSERVED)");
  if (raw && !h->n_mean) return fail(GRL_ERR_STATE, "this handle has no normalising act path");
  if (observed && h->ob_n != n) return fail(GRL_ERR_STATE, "n differs from the number of observations grl_observe holds");
  if (n > h->NA) return fail(GRL_ERR_INVALID, "n exceeds act_batch");
  if (flags & GRL_ACT_GREEDY) {
    if (!q) return fail(GRL_ERR_STATE, "GRL_ACT_GREEDY is defined for DQN / BDQ handles");
    return act_greedy(h, obs, n, eps, out, raw, observed);
  }
  if (!q && !td3 && !deterministic && !eps) return fail(GRL_ERR_INVALID, "stochastic action needs eps");
  const int64_t oe = (!q && h->cnn) ? (int64_t)h->hw * h->hw * h->cfg.obs_channels : h->cfg.obs_dim;
  const size_t n_in = observed ? 0 : (size_t)n * oe, n_eps = (!q && !td3 && !deterministic) ? (size_t)n * h->A : 0;
  const size_t n_out = q ? (size_t)n * h->qD * h->qN : (size_t)n * h->A;
  if (int e = pin_reserve(h, n_in, q ? n_out : 0)) return e;
  if (n_in) memcpy(h->pin_in.get(), obs, n_in * 4);
  if (n_eps) memcpy(h->a_eps, eps, n_eps * 4);      // (SAC: a_eps / a_out are host memory the launches read and write; the
  if (n_in) HIPCHK(hipMemcpyAsync(h->stg_obs, h->pin_in.get(), n_in * 4, hipMemcpyHostToDevice, h->stream));   // previous call synchronised)
  if (q) {
    if (int e = h->run_seq("act", {&h->ops_act})) return e;
  } else {
    // the launches cover act_batch rows whatever n is (rows beyond n hold stale observations: computed, not returned)
    const int v = (observed ? 2 : 0) | (raw ? 1 : 0);
    if (int e = h->run_seq(std::string(deterministic ? "act_det" : "act_sto") + char('0' + v),
                           {&h->ops_act_in[v], &h->ops_act, deterministic ? &h->ops_act_det : &h->ops_act_sto}))
      return e;
  }
  const bool poll = h->act_done_wgs && !h->prof;
  if (q && !poll) HIPCHK(hipMemcpyAsync(h->pin_out.get(), h->q_aout, n_out * 4, hipMemcpyDeviceToHost, h->stream));
  // the last launch counts its workgroups into coherent host memory once their actions are out (act_mfma.h) -- on EVERY call,
  // polled or not (a call under grl_profile_enable synchronises the stream instead): the expectation advances with it
  if (int e = act_wait(h, h->act_done_wgs)) return e;
  memcpy(out, q ? (poll ? h->q_act_host.get() : h->pin_out.get()) : h->a_out, n_out * 4);
  return GRL_OK;
}

// ---------------------------------------------------------------------------------------------- data parallel, in-graph
// this rank's two exchange allocations: flags = [DP_CHANNELS x DpCtl] (fine-grained), data = [src | red | gathered | 2 moment blocks]
static size_t dp_ctl_stride() { return (size_t)rup((int64_t)sizeof(DpCtl), 256); }
static size_t dp_arr_bytes(int64_t n) { return (size_t)rup(n * 4, 256); }
static size_t dp_mom_bytes(int64_t elems) { return (size_t)rup((2 * elems + 4) * 4, 256); }

int grl_allreduce_init(grl_handle h, int rank, int world, void* handle_out) {
  NOT_ON_PPO(h, "grl_allreduce_init");
  NOT_ON_TD3(h, "grl_allreduce_init");
  if (!h || !handle_out) return fail(GRL_ERR_INVALID, "null argument");
  if (h->cfg.algo == GRL_ALGO_AE) return fail(GRL_ERR_STATE, "the exchange step is defined for SAC / DQN / BDQ handles");
  if (world < 1 || world > DP_MAX_WORLD || rank < 0 || rank >= world) return fail(GRL_ERR_INVALID, "bad rank / world size");
  if (h->dp_buf) return fail(GRL_ERR_STATE, "grl_allreduce_init was already called on this handle");
  if (h->n_train % 4 || h->n_train * 4 >= (int64_t)1 << 31) return fail(GRL_ERR_STATE, "the gradient bucket is not a whole number of 16-byte groups below 2 GB");
  static_assert(sizeof(hipIpcMemHandle_t) == 64 && GRL_ALLREDUCE_HANDLE_BYTES == 128, "grl.h documents two 64-byte handles");
  const size_t fbytes = DP_CHANNELS * dp_ctl_stride();
  const size_t dbytes = 3 * dp_arr_bytes(h->n_train) + 2 * dp_mom_bytes(h->n_elems);
  // flags fine-grained: stores of a peer become visible to a kernel that is already running (and polling)
  hipError_t e = hipExtMallocWithFlags(&h->dp_flags, fbytes, hipDeviceMallocFinegrained);
  if (e != hipSuccess) { h->dp_flags = nullptr; return fail(GRL_ERR_HIP, std::string("exchange flags: ") + hipGetErrorString(e)); }
  // the data as well unless GRL_TUNE dp_coarse=1: the exchange kernels store it write-through and load it at system scope,
  // so its caching policy costs nothing measurable on one GPU and fine-grained is the conservative choice between GPUs
  e = Switches(SwRead::DP_INIT).get(Sw::dp_coarse) ? hipMalloc(&h->dp_buf, dbytes) : hipExtMallocWithFlags(&h->dp_buf, dbytes, hipDeviceMallocFinegrained);
  if (e != hipSuccess) { h->dp_buf = nullptr; h->dp_release(); return fail(GRL_ERR_HIP, std::string("exchange buffer: ") + hipGetErrorString(e)); }
  HIPCHK(hipMemset(h->dp_flags, 0, fbytes));
  HIPCHK(hipMemset(h->dp_buf, 0, dbytes));
  for (int k = 0; k < DP_CHANNELS; ++k) {     // the first exchange (epoch 1) uses source buffer 1
    const uint32_t one = 1u;
    HIPCHK(hipMemcpy((char*)h->dp_flags + k * dp_ctl_stride() + offsetof(DpCtl, next_buf), &one, 4, hipMemcpyHostToDevice));
  }
  // page-locked mailbox (allocated once, zeroed): a kernel that gives up waiting tells the host without a device read
  HIPCHK_AS("hipHostMalloc((void**)&h->dp_err_host, 64, 0)", h->dp_err_host.reserve(16));   // word 0: error, word 1: wait bound in ms (0 = the captured default; grl_allreduce_set_timeout)
  HIPCHK(hipDeviceSynchronize());
  hipIpcMemHandle_t mh[2];
  e = hipIpcGetMemHandle(&mh[0], h->dp_flags);
  if (e == hipSuccess) e = hipIpcGetMemHandle(&mh[1], h->dp_buf);
  if (e != hipSuccess) { h->dp_release(); return fail(GRL_ERR_HIP, std::string("hipIpcGetMemHandle: ") + hipGetErrorString(e)); }
  memcpy(handle_out, mh, GRL_ALLREDUCE_HANDLE_BYTES);
  memset(&h->dp, 0, sizeof(h->dp));
  h->dp.rank = rank; h->dp.world = world;
  return GRL_OK;
}

// arguments of one channel over the given pieces of the bucket
static DpArgs dp_channel(grl_ctx* h, int channel, const std::vector<std::pair<int64_t, int64_t>>& pieces, char* const* flags,
                         char* const* data) {
  DpArgs d;
  memset(&d, 0, sizeof(d));
  d.rank = h->dp.rank; d.world = h->dp.world;
  d.n_ranges = (int)pieces.size();
  int64_t v = 0;
  for (size_t k = 0; k < pieces.size(); ++k) { d.start[k] = pieces[k].first; d.vstart[k] = v; v += pieces[k].second; }
  for (size_t k = pieces.size(); k <= DP_MAX_RANGES; ++k) d.vstart[k] = v;
  d.n = v;
  d.chunk = rup((v + d.world - 1) / d.world, 4);      // (the last ranks' chunks may be short or empty)
  d.timeout_ticks = (uint64_t)std::max(1, Switches(SwRead::DP_CONNECT).get(Sw::dp_timeout_ms)) * 100000ull;     // 100 MHz wall clock
  d.host_err = h->dp_err_host.get();
  for (int p = 0; p < d.world; ++p) {
    d.ctl[p] = (DpCtl*)(flags[p] + (size_t)channel * dp_ctl_stride());
    d.src[p] = (float*)data[p];
    d.red[p] = (float*)(data[p] + dp_arr_bytes(h->n_train));
  }
  return d;
}
// grids of the exchange kernels (GRL_TUNE dp_blocks=reduce/gather/apply overrides: tuning aid).  Default: one quad per
// thread, no grid-stride loop -- each thread issues its loads in one batch (measured: the looping 512-block form took
// 19 us for the 5.4 MB bucket where the slab reduction with fused Adam, one quad per thread, takes 12)
static int dp_blocks(int which, int64_t quads) {
  int v[3] = {0, 0, 0};
  Switches(SwRead::DP_CONNECT).get3(Sw::dp_blocks, v);
  const int64_t all = std::max<int64_t>(1, (quads + 255) / 256);
  return (int)(v[which] > 0 ? std::min<int64_t>(v[which], all) : std::min<int64_t>(all, 4096));
}
// K1: the reduction that ends a gradient computation, publishing its sums on channel `da` as it forms them; with `ga`
// it also carries the replay gather of the next update (multi-update calls on the device RNG)
static Op dp_k1_op(grl_ctx* self, const grl_ctx::ReducePlan& rp, const DpArgs& da, const LossArgs& la, const GatherArgs* ga, int gx,
                   const char* tag) {
  Op op; op.tag = tag; op.bytes = 8.0 * (double)da.n;
  op.join = true;                                       // (takes the place of reduce_slabs, which joins the side lane)
  const ReduceDesc* dr = self->d_reduces;
  const AdamArgs aa = self->adam_base;
  GatherArgs g;
  memset(&g, 0, sizeof(g));
  if (ga) g = *ga;
  const int gxx = ga ? gx : 0;
  op.run = [dr, rp, la, aa, da, g, gxx](hipStream_t s) { launch_dp_reduce_slabs(dr, rp.tiles, rp.n, la, rp.has_loss, aa, da, g, gxx, s); };
  return op;
}
// W: one wave announces (`which` 0: ready, 1: done) and waits for every rank (the only kernel of the exchange that waits)
static Op dp_wait_op(const DpArgs& da, int which) {
  Op op; op.tag = which == 0 ? "dp_wait_ready" : "dp_wait_done";
  op.run = [da, which](hipStream_t s) { hipLaunchKernelGGL(dp_wait_kernel, dim3(1), dim3(64), 0, s, da, which); };
  return op;
}
static Op dp_reduce_op(const DpArgs& da) {
  Op op; op.tag = "dp_reduce"; op.bytes = 4.0 * (double)da.chunk * (da.world + 1);
  const int blocks = dp_blocks(0, da.chunk / 4);
  op.run = [da, blocks](hipStream_t s) { hipLaunchKernelGGL(dp_reduce_kernel, dim3(blocks), dim3(256), 0, s, da); };
  return op;
}
static Op dp_gather_op(const DpArgs& da) {
  Op op; op.tag = "dp_gather"; op.bytes = 8.0 * (double)da.n;
  const int blocks = dp_blocks(1, da.n / 4);
  op.run = [da, blocks](hipStream_t s) { hipLaunchKernelGGL(dp_gather_kernel, dim3(blocks), dim3(256), 0, s, da); };
  return op;
}
static AdamArgs dp_adam_args(grl_ctx* self, int world) {
  AdamArgs aa = self->adam_args(1.f / (float)world, true);
  aa.grads = nullptr;      // (the exchange kernels read the sums from the exchange buffers)
  return aa;
}
static Op dp_apply_op(grl_ctx* self, const DpArgs& da, const DpArgs& db) {
  Op op; op.tag = "dp_apply"; op.bytes = (double)self->n_train * 4 * 7 + (double)self->n_polyak * 4 * 2;
  op.join = true;
  const AdamArgs aa = dp_adam_args(self, da.world);
  const int blocks = dp_blocks(2, std::max(da.chunk, db.chunk) / 4);     // (a block walks the owners' chunks one after the other)
  op.run = [aa, da, db, blocks](hipStream_t s) { hipLaunchKernelGGL(dp_apply_kernel, dim3(blocks), dim3(256), 0, s, aa, da, db); };
  return op;
}
static Op dp_apply_oneshot_op(grl_ctx* self, const DpArgs& da) {
  Op op; op.tag = "dp_apply1"; op.bytes = (double)self->n_train * 4 * (6 + da.world) + (double)self->n_polyak * 4 * 2;
  op.join = true;
  const AdamArgs aa = dp_adam_args(self, da.world);
  const int blocks = dp_blocks(2, da.n / 4);
  op.run = [aa, da, blocks](hipStream_t s) { hipLaunchKernelGGL(dp_apply_oneshot_kernel, dim3(blocks), dim3(256), 0, s, aa, da); };
  return op;
}

// The sequences of a multi-update SAC call ending in the exchange (`ride`: the "gather_ride" form of the call, else "prefetch"):
// every update assembled by sac_update_ops (plan_sac.inl) and closed by the publishing reduction K1 -- carrying the riders of
// the next update except in the call's last one -- and the rest of the exchange `tail`.  short_call_graph is the caller's choice
static void close_with_exchange(grl_ctx* h, const DpArgs& d, bool ride, CallPlan& dst, const std::vector<Op>& tail, bool short_call_graph) {
  const grl_ctx::SacKit::Riders& r = h->sac_kit.riders[ride];
  sac_call_plan(*h, dst, ride, [&](int v) {
    std::vector<Op> close{v == 2 ? dp_k1_op(h, h->red_all, d, h->loss_args, nullptr, 0, "reduce_publish")
                                 : dp_k1_op(h, h->red_all, d, r.lk, &r.g2, r.gx, "reduce_publish")};
    close.insert(close.end(), tail.begin() + 1, tail.end());
    return close;
  });
  dst.short_call_graph = short_call_graph;
}

int grl_allreduce_connect(grl_handle h, const void* handles) {
  NOT_ON_PPO(h, "grl_allreduce_connect");
  NOT_ON_TD3(h, "grl_allreduce_connect");
  if (!h || !handles) return fail(GRL_ERR_INVALID, "null argument");
  if (!h->dp_buf) return fail(GRL_ERR_STATE, "call grl_allreduce_init first");
  if (h->dp_on) return fail(GRL_ERR_STATE, "already connected");
  const bool qh = h->cfg.algo != GRL_ALGO_SAC;
  // the gradient computation without the reduction that ends it (SAC: the recorded closing slot; DQN / BDQ: the batch means of
  // the loss launch follow the reduction as a launch of their own in the split plan)
  size_t n_body = h->ops_grads.size();
  bool ends_in_reduction = !qh && h->sac_kit.close + 1 == (int)n_body;
  if (qh) {
    while (n_body > 0 && h->ops_grads[n_body - 1].tag == "q_finish") --n_body;
    ends_in_reduction = n_body > 0 && h->ops_grads[n_body - 1].tag == "reduce_slabs";
  }
  if (!ends_in_reduction || !h->red_all.tiles)
    return fail(GRL_ERR_STATE, "this plan does not end in the slab reduction the exchange publishes from");
  char* flags[DP_MAX_WORLD];
  char* data[DP_MAX_WORLD];
  for (int p = 0; p < h->dp.world; ++p) {
    flags[p] = (char*)h->dp_flags;
    data[p] = (char*)h->dp_buf;
    if (p != h->dp.rank) {
      hipIpcMemHandle_t mh[2];
      memcpy(mh, (const char*)handles + (size_t)GRL_ALLREDUCE_HANDLE_BYTES * p, GRL_ALLREDUCE_HANDLE_BYTES);
      void* ptr[2] = {nullptr, nullptr};
      for (int k = 0; k < 2; ++k) {
        hipError_t e = hipIpcOpenMemHandle(&ptr[k], mh[k], hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) return fail(GRL_ERR_HIP, "hipIpcOpenMemHandle (rank " + std::to_string(p) + "): " + hipGetErrorString(e));
        h->dp_peer[2 * p + k] = ptr[k];
      }
      flags[p] = (char*)ptr[0];
      data[p] = (char*)ptr[1];
    }
  }
  DpArgs none;
  memset(&none, 0, sizeof(none));
  // ---- the plain update: one exchange of the whole bucket; the gradient computation's last launch publishes (K1)
  h->dp = dp_channel(h, 0, {{0, h->n_train}}, flags, data);
  DpArgs d1s = h->dp;
  d1s.oneshot = 1;
  h->dp_body.assign(h->ops_grads.begin(), h->ops_grads.begin() + (n_body - 1));
  if (qh) {
    // DQN / BDQ: per-variable clip_by_norm sits between the all-reduce and Adam, so the sums are pulled into the gradient
    // bucket (two-shot + gather) and the plan's own apply launches follow with grad_scale = 1 / W (clip threshold W c on the
    // sum, plan_q.inl).  One form only: grl_allreduce_set_mode accepts "auto" / two-shot on these handles.
    DpArgs d = h->dp;
    d.gathered = h->grads;
    std::vector<Op>& tail = h->ops_dp;
    tail.clear();
    tail.push_back(dp_k1_op(h, h->red_all, d, h->loss_args, nullptr, 0, "reduce_publish"));
    tail.push_back(dp_wait_op(d, 0));
    tail.push_back(dp_reduce_op(d));
    tail.push_back(dp_wait_op(d, 1));
    tail.push_back(dp_gather_op(d));
    for (size_t k = n_body; k < h->ops_grads.size(); ++k) tail.push_back(h->ops_grads[k]);      // q_finish
    for (auto& o : h->ops_apply) tail.push_back(o);
    h->dp_body_per.clear();
    for (auto& o : h->dp_body)
      if (o.tag != "gather_norm") h->dp_body_per.push_back(o);
    h->ops_dp1.clear();
    for (int one = 0; one < 2; ++one) { h->pf_dp[one].clear(); h->ride_dp[one].clear(); }
  }
  for (int one = 0; one < 2 && !qh; ++one) {
    const DpArgs& d = one ? d1s : h->dp;
    std::vector<Op>& tail = one ? h->ops_dp1 : h->ops_dp;
    tail.clear();
    tail.push_back(dp_k1_op(h, h->red_all, d, h->loss_args, nullptr, 0, "reduce_publish"));
    tail.push_back(dp_wait_op(d, 0));
    if (one) tail.push_back(dp_apply_oneshot_op(h, d));
    else { tail.push_back(dp_reduce_op(d)); tail.push_back(dp_wait_op(d, 1)); tail.push_back(dp_apply_op(h, d, none)); }
    // multi-update calls on the device RNG: the same with the gather of the next update riding on K1 (plan_sac "prefetch") or,
    // with double-buffered images, the image gather riding on the head launch and the extras on K1 (plan_sac "gather_ride").
    // (pf_dp keeps short_call_graph off: see plan_q "per_pf")
    h->pf_dp[one].clear();
    h->ride_dp[one].clear();
    if (h->pf.ok()) close_with_exchange(h, d, false, h->pf_dp[one], tail, false);
    if (h->ride.ok()) close_with_exchange(h, d, true, h->ride_dp[one], tail, true);
  }
  // ---- the overlapped update (grl_allreduce_set_overlap): the staged plan (grl_compute_grads_staged) with both exchanges in
  // the graph.  After heads_dfeat a SIDE LANE forms the dense layers' weight gradients, reduces them (publishing) and
  // exchanges them on channel 0 -- 90 % of the bytes -- while the main lane runs the backward through the convolutions and
  // their weight gradients; the small convolution bucket follows on channel 1; Adam waits for both.  Same tiles, same
  // sums: parameters are bit-identical to the plain update's.
  h->ops_dp_overlap.clear();
  if (h->staged_ok) {
    std::vector<std::pair<int64_t, int64_t>> dense, conv;
    int64_t off[8], num[8];
    for (int b = 0; b < 2; ++b) {
      const int nr = grl_grad_ranges(h, b, 8, off, num);
      if (nr < 0) return nr;
      for (int k = 0; k < nr; ++k) (b == 0 ? dense : conv).push_back({off[k], num[k]});
    }
    bool ok = dense.size() <= DP_MAX_RANGES && conv.size() <= DP_MAX_RANGES;
    for (auto& r : dense) ok = ok && r.first % 4 == 0 && r.second % 4 == 0;
    for (auto& r : conv) ok = ok && r.first % 4 == 0 && r.second % 4 == 0;
    const int cut = h->sac_kit.dfeat;       // (the stages copy ops_grads up to here; each ends in its own reduction)
    if (ok && cut >= 0) {
      DpArgs d0 = dp_channel(h, 0, dense, flags, data);
      const DpArgs d1 = dp_channel(h, 1, conv, flags, data);
      std::vector<Op>& L = h->ops_dp_overlap;
      for (int k = 0; k <= cut; ++k) L.push_back(h->ops_stage0[k]);
      bool first = true;
      auto side = [&](Op o) { o.lane = 1; o.fork = first; o.join = false; first = false; L.push_back(o); };
      for (size_t k = cut + 1; k + 1 < h->ops_stage0.size(); ++k) side(h->ops_stage0[k]);     // wgrad_dense
      side(dp_k1_op(h, h->red_dense, d0, h->loss_args, nullptr, 0, "reduce_dense_publish"));
      side(dp_wait_op(d0, 0));
      side(dp_reduce_op(d0));
      side(dp_wait_op(d0, 1));
      d0.gathered = (float*)((char*)h->dp_buf + 2 * dp_arr_bytes(h->n_train));     // the side lane also pulls the dense sums
      side(dp_gather_op(d0));
      for (size_t k = 0; k + 1 < h->ops_stage1.size(); ++k) { Op o = h->ops_stage1[k]; o.join = false; L.push_back(o); }
      { Op o = dp_k1_op(h, h->red_conv, d1, h->loss_args, nullptr, 0, "reduce_conv_publish"); o.join = false; L.push_back(o); }
      L.push_back(dp_wait_op(d1, 0));
      L.push_back(dp_reduce_op(d1));
      L.push_back(dp_wait_op(d1, 1));
      L.push_back(dp_apply_op(h, d0, d1));       // (joins the side lane)
    }
  }
  if (!qh) {
    plan_seq("ops_dp", h->ops_dp); plan_seq("ops_dp1", h->ops_dp1);
    for (int one = 0; one < 2; ++one) {
      plan_seq("pf_dp[" + std::to_string(one) + "]", h->pf_dp[one]);
      plan_seq("ride_dp[" + std::to_string(one) + "]", h->ride_dp[one]);
    }
    plan_seq("ops_dp_overlap", h->ops_dp_overlap);
  }
  // ---- the running-statistics merge (grl_norm_update on a connected handle): channel 2, moment blocks behind the three arrays
  memset(&h->dp_norm, 0, sizeof(h->dp_norm));
  h->dp_norm.d = dp_channel(h, 2, {}, flags, data);
  h->dp_norm.mom_stride = (int64_t)(dp_mom_bytes(h->n_elems) / 4);
  for (int p = 0; p < h->dp.world; ++p) h->dp_norm.mom[p] = (float*)(data[p] + 3 * dp_arr_bytes(h->n_train));
  h->dp_on = true;
  return GRL_OK;
}

int grl_allreduce_disconnect(grl_handle h) {
  NOT_ON_PPO(h, "grl_allreduce_disconnect");
  NOT_ON_TD3(h, "grl_allreduce_disconnect");
  if (!h) return fail(GRL_ERR_INVALID, "null handle");
  if (!h->dp_buf && !h->dp_flags) return GRL_OK;          // never initialised (or already released): nothing to do
  HIPCHK(hipStreamSynchronize(h->stream));
  h->drop_graphs();                                        // captured sequences hold the peers' addresses
  h->dp_on = false;
  h->dp_overlap = false;
  h->dp_mode = 0;
  for (auto* v : {&h->ops_dp, &h->ops_dp1, &h->dp_body, &h->dp_body_per, &h->ops_dp_overlap}) v->clear();
  for (int one = 0; one < 2; ++one) { h->pf_dp[one].clear(); h->ride_dp[one].clear(); }
  h->dp_release();
  memset(&h->dp, 0, sizeof(h->dp));
  memset(&h->dp_norm, 0, sizeof(h->dp_norm));
  if (h->dp_err_host.get()) *h->dp_err_host.get() = 0u;
  return GRL_OK;
}

int grl_allreduce_set_overlap(grl_handle h, int on) {
  NOT_ON_PPO(h, "grl_allreduce_set_overlap");
  NOT_ON_TD3(h, "grl_allreduce_set_overlap");
  if (!h) return fail(GRL_ERR_INVALID, "null handle");
  if (!h->dp_on) return fail(GRL_ERR_STATE, "call grl_allreduce_init / grl_allreduce_connect first");
  if (on && h->ops_dp_overlap.empty()) return fail(GRL_ERR_STATE, "this configuration has no staged plan: the exchange cannot be overlapped");
  h->dp_overlap = on != 0;
  return GRL_OK;
}

int grl_allreduce_set_mode(grl_handle h, int mode) {
  NOT_ON_PPO(h, "grl_allreduce_set_mode");
  NOT_ON_TD3(h, "grl_allreduce_set_mode");
  if (!h) return fail(GRL_ERR_INVALID, "null handle");
  if (!h->dp_on) return fail(GRL_ERR_STATE, "call grl_allreduce_init / grl_allreduce_connect first");
  if (mode < 0 || mode > 2) return fail(GRL_ERR_INVALID, "mode: 0 auto, 1 two-shot, 2 one-shot");
  if (mode == 2 && h->cfg.algo != GRL_ALGO_SAC) return fail(GRL_ERR_STATE, "DQN / BDQ handles exchange two-shot (the clipped apply reads the gathered sums)");
  h->dp_mode = mode;
  return GRL_OK;
}

int grl_allreduce_set_timeout(grl_handle h, int ms) {
  NOT_ON_PPO(h, "grl_allreduce_set_timeout");
  NOT_ON_TD3(h, "grl_allreduce_set_timeout");
  if (!h || ms < 0) return fail(GRL_ERR_INVALID, "bad argument");
  if (!h->dp_err_host.get()) return fail(GRL_ERR_STATE, "call grl_allreduce_init first");
  __atomic_store_n(h->dp_err_host.get() + 1, (uint32_t)ms, __ATOMIC_RELEASE);     // read by the waiting kernels (dp_wait_all)
  return GRL_OK;
}

int grl_train_step_allreduce(grl_handle h, int n_steps, const int64_t* idx, const float* eps) {
  NOT_ON_PPO(h, "grl_train_step_allreduce");
  NOT_ON_TD3(h, "grl_train_step_allreduce");
  if (!h || n_steps < 1) return fail(GRL_ERR_INVALID, "bad argument");
  if (!h->dp_on) return fail(GRL_ERR_STATE, "call grl_allreduce_init / grl_allreduce_connect first");
  if ((idx == nullptr) != (eps == nullptr)) return fail(GRL_ERR_INVALID, "idx and eps must both be given or both be NULL");
  if (h->rp_size < 1) return fail(GRL_ERR_STATE, "replay buffer is empty");
  if (*h->dp_err_host.get()) return fail(GRL_ERR_STATE, "an exchange timed out waiting for a peer (the replicas are no longer in step)");
  // one-shot (every rank adds all contributions itself: one kernel and one flag round less, (W - 1) n bytes per rank
  // instead of 2 (W - 1) / W n) pays for W <= 2
  const bool qh = h->cfg.algo != GRL_ALGO_SAC;
  if (qh && h->per_on) return fail(GRL_ERR_STATE, "the exchange step draws uniform minibatches: prioritised handles train with grl_train_step_per");
  if (qh) h->grad_scale = 1.f / (float)h->dp.world;       // (baked into the captured apply launches: constant per connection)
  const bool one = !qh && !h->dp_overlap && (h->dp_mode == 2 || (h->dp_mode == 0 && h->dp.world <= 2));
  std::vector<Op> none;
  std::vector<Op>* body = h->dp_overlap ? &h->ops_dp_overlap : &h->dp_body;
  std::vector<Op>* tail = h->dp_overlap ? &none : (one ? &h->ops_dp1 : &h->ops_dp);
  const std::string sfx = one ? "1" : "";
  const bool call = !idx && n_steps >= 2 && !h->dp_overlap && !h->prof;
  if (call && h->ride_dp[one].ok()) {
    // plain exchange on the device RNG, double-buffered images: the image gather of update t+1 rides on update t's head launch
    if (int e = h->run_call("dpr" + sfx, h->ride_dp[one], n_steps)) return e;
  } else if (call && h->pf_dp[one].ok()) {
    // plain exchange on the device RNG: the prefetching sequences (the gather of update t+1 rides on the reduction of update t)
    if (int e = h->run_call("dpp" + sfx, h->pf_dp[one], n_steps)) return e;
  } else if (!idx) {      // device RNG: identical updates, several to a graph
    if (int e = h->run_repeated((h->dp_overlap ? "dpo_rng" : "dp_rng") + sfx, {&h->ops_rng, body, tail}, n_steps)) return e;
  } else {
    for (int s = 0; s < n_steps; ++s) {
      if (int e = stage_noise(h, idx, eps, s)) return e;
      if (int e = h->run_seq((h->dp_overlap ? "dpo_explicit" : "dp_explicit") + sfx, {&h->ops_gather, body, tail})) return e;
    }
  }
  HIPCHK(hipGetLastError());
  return GRL_OK;
}

int grl_allreduce_status(grl_handle h, int64_t* exchanges, int* error) {
  NOT_ON_PPO(h, "grl_allreduce_status");
  NOT_ON_TD3(h, "grl_allreduce_status");
  if (!h || !h->dp_flags) return fail(GRL_ERR_STATE, "no exchange buffer");
  HIPCHK(hipStreamSynchronize(h->stream));
  DpCtl c[DP_CHANNELS];
  for (int k = 0; k < DP_CHANNELS; ++k)
    HIPCHK(hipMemcpy(&c[k], (char*)h->dp_flags + k * dp_ctl_stride(), sizeof(DpCtl), hipMemcpyDeviceToHost));
  if (exchanges) *exchanges = c[0].epoch;          // (channel 0 takes part in every update, plain or overlapped)
  for (int k = 0; k < DP_CHANNELS; ++k) {
    plan_note("grl dp: rank %d channel %d epoch %u error %u next_buf %u ready", h->dp.rank, k, c[k].epoch, c[k].error, c[k].next_buf);
    for (int p = 0; p < h->dp.world; ++p) plan_note(" %u", c[k].ready[p]);
    plan_note(" done");
    for (int p = 0; p < h->dp.world; ++p) plan_note(" %u", c[k].done[p]);
    plan_note(" mailbox %u\n", h->dp_err_host.get() ? *h->dp_err_host.get() : 0u);
  }
  int err = h->dp_err_host.get() ? (int)*h->dp_err_host.get() : 0;
  for (int k = 0; k < DP_CHANNELS; ++k) err |= (int)c[k].error;
  if (error) *error = err;
  if (err) return fail(GRL_ERR_STATE, "an exchange timed out waiting for a peer (the replicas are no longer in step)");
  return GRL_OK;
}

int grl_q_update_target(grl_handle h) {
  NOT_ON_PPO(h, "grl_q_update_target");
  NOT_ON_TD3(h, "grl_q_update_target");
  if (!h) return fail(GRL_ERR_INVALID, "null handle");
  if (h->cfg.algo == GRL_ALGO_SAC) return fail(GRL_ERR_STATE, "SAC has no hard target update");
  HIPCHK(hipMemcpyAsync(h->params + h->tgt_off, h->params + h->q_online_off, (size_t)h->q_online_n * 4,
                        hipMemcpyDeviceToDevice, h->stream));
  return GRL_OK;
}

int grl_encoder_load(grl_handle h, const float* const* w, const int64_t* numels, int n_arrays) {
  NOT_ON_PPO(h, "grl_encoder_load");
  NOT_ON_TD3(h, "grl_encoder_load");
  if (!h || !w || !numels || n_arrays != 8) return fail(GRL_ERR_INVALID, "expected 8 weight arrays");
  if (h->cfg.algo != GRL_ALGO_SAC) return fail(GRL_ERR_STATE, "grl_encoder_load is for SAC handles (auto-encoder handles encode with their own parameters)");
  const int64_t wn[8] = {7 * 7 * 32, 32, 5 * 5 * 32 * 32, 32, 3 * 3 * 32 * 32, 32, 2048 * 100, 100};
  for (int k = 0; k < 8; ++k)
    if (numels[k] != wn[k]) return fail(GRL_ERR_INVALID, "encoder weight " + std::to_string(k) + " has the wrong size");
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int k = 0; k < 8; ++k) HIPCHK(hipMemcpy(h->enc_w[k], w[k], (size_t)wn[k] * 4, hipMemcpyHostToDevice));
  h->enc_loaded = true;
  return GRL_OK;
}

int grl_encode(grl_handle h, const float* depth, int n, float* out) {
  NOT_ON_PPO(h, "grl_encode");
  NOT_ON_TD3(h, "grl_encode");
  if (!h || !depth || !out || n < 1) return fail(GRL_ERR_INVALID, "bad argument");
  if (!h->enc_loaded) return fail(GRL_ERR_STATE, "grl_encoder_load has not been called");
  if (n > h->NA) return fail(GRL_ERR_INVALID, "n exceeds act_batch");
  const size_t ed = (size_t)h->enc_dim;      // 100 for the shipped encoder; an auto-encoder handle's own encoding_dim
  if (int e = pin_reserve(h, (size_t)n * 4096, (size_t)n * ed)) return e;
  memcpy(h->pin_in.get(), depth, (size_t)n * 4096 * 4);
  HIPCHK(hipMemcpyAsync(h->ex_in, h->pin_in.get(), (size_t)n * 4096 * 4, hipMemcpyHostToDevice, h->stream));
  if (int e = h->run_seq("encode", {&h->ops_enc})) return e;
  HIPCHK(hipMemcpyAsync(h->pin_out.get(), h->eout, (size_t)n * ed * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  memcpy(out, h->pin_out.get(), (size_t)n * ed * 4);
  return GRL_OK;
}

int64_t grl_debug_fetch(grl_handle h, const char* name, float* out, int64_t cap) {
  if (!h || !name || !out) return fail(GRL_ERR_INVALID, "null argument");
  auto it = h->dbg.find(name);
  if (it == h->dbg.end()) return fail(GRL_ERR_INVALID, std::string("unknown tensor ") + name);
  const int64_t n = std::min(cap, it->second.second);
  if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(GRL_ERR_HIP, "sync failed");
  hipError_t e = hipMemcpy(out, it->second.first, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(GRL_ERR_HIP, hipGetErrorString(e));
  return n;
}

int64_t grl_debug_store(grl_handle h, const char* name, const float* in, int64_t n) {
  if (!h || !name || !in) return fail(GRL_ERR_INVALID, "null argument");
  if ((h->cfg.algo == GRL_ALGO_PPO || h->cfg.algo == GRL_ALGO_TRPO) && !strcmp(name, "ppo_slots")) {      // a rollout placed through the names below: how far it has got
    if (n != 3) return fail(GRL_ERR_INVALID, "ppo_slots takes three values: slots written, slots closed, finished");
    const int32_t st = (int32_t)in[0], cl = (int32_t)in[1];
    if (cl < 0 || cl > h->pcfg.n_steps || st < cl || st > cl + 1 || st > h->pcfg.n_steps) return fail(GRL_ERR_INVALID, "ppo_slots out of range");
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(GRL_ERR_HIP, "sync failed");
    if (hipMemcpy(&h->ppo_dev->slot, &cl, 4, hipMemcpyHostToDevice) != hipSuccess) return fail(GRL_ERR_HIP, "copy failed");
    h->ppo_stepped = st; h->ppo_closed = cl; h->ppo_finished = in[2] != 0.f && cl == h->pcfg.n_steps;
    h->ppo_held = h->ppo_finished; h->gail_rewritten = false;
    return n;
  }
  auto it = h->dbg.find(name);
  if (it == h->dbg.end()) return fail(GRL_ERR_INVALID, std::string("unknown tensor ") + name);
  if (n > it->second.second) return fail(GRL_ERR_INVALID, std::string("too many values for ") + name);
  if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(GRL_ERR_HIP, "sync failed");
  hipError_t e = hipMemcpy(const_cast<float*>(it->second.first), in, (size_t)n * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(GRL_ERR_HIP, hipGetErrorString(e));
  return n;
}

int grl_profile_enable(grl_handle h, int on) {
  if (!h) return fail(GRL_ERR_INVALID, "null handle");
  h->prof = on != 0;
  if (on) h->prof_acc.clear();
  return GRL_OK;
}

int grl_profile_query(grl_handle h, const char* name, double* avg_ms, int64_t* launches) {
  if (!h || !name) return fail(GRL_ERR_INVALID, "null argument");
  auto it = h->prof_acc.find(name);
  if (it == h->prof_acc.end()) return fail(GRL_ERR_INVALID, std::string("no profile for ") + name);
  if (avg_ms) *avg_ms = it->second.n ? it->second.ms / it->second.n : 0.0;
  if (launches) *launches = it->second.n;
  return GRL_OK;
}

/* list profiled tags: writes "tag:avg_ms:launches:flops_per_launch:bytes_per_launch:executed_flops_per_launch\n" lines */
int grl_profile_dump(grl_handle h, char* buf, int cap) {
  if (!h || !buf || cap < 1) return fail(GRL_ERR_INVALID, "bad argument");
  std::string s;
  for (auto& kv : h->prof_acc) {
    char line[256];
    snprintf(line, sizeof(line), "%s:%.6f:%lld:%.0f:%.0f:%.0f\n", kv.first.c_str(),
             kv.second.n ? kv.second.ms / kv.second.n : 0.0, (long long)kv.second.n,
             kv.second.n ? kv.second.flops / kv.second.n : 0.0, kv.second.n ? kv.second.bytes / kv.second.n : 0.0,
             kv.second.n ? kv.second.flops_exec / kv.second.n : 0.0);
    s += line;
  }
  strncpy(buf, s.c_str(), cap - 1);
  buf[cap - 1] = 0;
  return GRL_OK;
}

// ---- sessions: behaviour-cloning pretraining on a SAC handle (plan_bc.inl), GAIL on a TRPO handle (plan_gail.inl), each in a
// buffer of the caller's.  What the two share is written once here; the wording of every message is the entry point's own.
#define SAC_ONLY(h, what)                                                                                        \
  do {                                                                                                           \
    if (!(h)) return fail(GRL_ERR_INVALID, "null handle");                                                       \
    if ((h)->cfg.algo != GRL_ALGO_SAC) return fail(GRL_ERR_STATE, what " is defined for SAC handles (grl_create)"); \
  } while (0)
#define GAIL_SESSION(h, what)                                                                                     \
  do {                                                                                                            \
    TRPO_ONLY(h, what);                                                                                           \
    if (!(h)->gail()) return fail(GRL_ERR_STATE, what " needs an open session (grl_gail_begin)");                 \
  } while (0)

static int check_act_bounds(grl_handle h, const float* low, const float* high, const char* who) {
  for (int j = 0; j < h->cfg.act_dim; ++j)
    if (!(high[j] > low[j]) || !std::isfinite(high[j]) || !std::isfinite(low[j]))
      return fail(GRL_ERR_INVALID, std::string(who) + ": the action bounds must be finite with high > low (dimension " + std::to_string(j) + ")");
  return GRL_OK;
}

extern "C++" {      // (two templates; everything here is static anyway)
// a fresh record of a checked configuration: the bounds copied, the caller's pointers dropped
template <class Plan, class Config>
static std::unique_ptr<Session> session_fill(grl_handle h, const Config* c) {
  std::unique_ptr<Plan> p(new Plan());
  p->cfg = *c;
  p->low.assign(c->act_low, c->act_low + h->cfg.act_dim);
  p->high.assign(c->act_high, c->act_high + h->cfg.act_dim);
  p->cfg.act_low = p->cfg.act_high = nullptr;
  return p;
}

// n index rows of `batch` entries into a table of n_rows: every entry in [-1, n_rows), -1 only as a tail, at least one row present.
// pre(u, b) may refuse entry b of row u first (nonzero: its error); where(u, b) names the entry, asked only when it is refused
// (a string per entry in front of every call showed in the GAIL update's time); present: the rows' counts.
template <class Pre, class Where>
static int check_tail_rows(const int32_t* rows, int n, int batch, int64_t n_rows, Pre pre, Where where, std::vector<int>* present) {
  for (int u = 0; u < n; ++u) {
    const int32_t* row = rows + (size_t)u * batch;
    bool tail = false;
    int n_e = 0;
    for (int b = 0; b < batch; ++b) {
      if (int e = pre(u, b)) return e;
      if (row[b] < -1 || row[b] >= n_rows) return fail(GRL_ERR_INVALID, where(u, b) + " is outside the table (" + std::to_string(row[b]) + ")");
      if (row[b] == -1) { if (b == 0) return fail(GRL_ERR_INVALID, where(u, b) + ": a minibatch needs at least one row"); tail = true; }
      else if (tail) return fail(GRL_ERR_INVALID, where(u, b) + " follows a -1: absent rows must be trailing");
      else n_e += 1;
    }
    if (present) present->push_back(n_e);
  }
  return GRL_OK;
}
}  // extern "C++"

// the plan built dry: the bytes a session of this record needs
static int session_query(grl_handle h, std::unique_ptr<Session> s, size_t* bytes) {
  if (int e = s->plan(*h)) return e;
  *bytes = s->a.off + 256;
  return GRL_OK;
}

// Installs the record and builds its plan into buf; then the whole buffer zero (parameters, moments, row padding, untouched
// pixels), the tables and the optimiser's starting words.  On any failure the handle is left without a session.
static int session_open(grl_handle h, std::unique_ptr<Session> s, void* buf, const float lr, const char* what) {
  s->a.base = (char*)buf;
  h->session = std::move(s);
  Session& p = *h->session;
  if (int e = p.plan(*h)) { h->uploads.clear(); h->session_drop(); return e; }
  hipError_t e = hipMemsetAsync(buf, 0, p.a.off, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  for (auto& u : h->uploads)
    if (e == hipSuccess) e = hipMemcpy(u.dst, u.bytes.data(), u.bytes.size(), hipMemcpyHostToDevice);
  h->uploads.clear();
  DevScalars s0;
  memset(&s0, 0, sizeof(s0));
  s0.beta1_power = 0.9f; s0.beta2_power = 0.999f; s0.lr = lr;
  if (e == hipSuccess) e = hipMemcpy(p.sc, &s0, sizeof(s0), hipMemcpyHostToDevice);
  if (e != hipSuccess) { h->session_drop(); return fail(GRL_ERR_HIP, std::string(what) + " begin: " + hipGetErrorString(e)); }
  return GRL_OK;
}

static int check_bc(grl_handle h, const grl_bc_config* c) {
  if (!c || !c->act_low || !c->act_high) return fail(GRL_ERR_INVALID, "null behaviour-cloning config or action bounds");
  if (c->batch < 1) return fail(GRL_ERR_INVALID, "bc: batch must be >= 1");
  if (c->batch > h->cfg.batch_size)
    return fail(GRL_ERR_INVALID, "bc: batch " + std::to_string(c->batch) + " exceeds the handle's batch_size " + std::to_string(h->cfg.batch_size));
  if (!(c->lr > 0.f) || !(c->adam_eps > 0.f)) return fail(GRL_ERR_INVALID, "bc: lr and adam_eps must be > 0");
  return check_act_bounds(h, c->act_low, c->act_high, "bc");
}

int grl_bc_query_sizes(grl_handle h, const grl_bc_config* c, size_t* bytes) {
  SAC_ONLY(h, "grl_bc_query_sizes");
  if (!bytes) return fail(GRL_ERR_INVALID, "null out");
  if (int e = check_bc(h, c)) return e;
  return session_query(h, session_fill<BcPlan>(h, c), bytes);
}

int grl_bc_begin(grl_handle h, const grl_bc_config* c, void* buf) {
  SAC_ONLY(h, "grl_bc_begin");
  if (!buf) return fail(GRL_ERR_INVALID, "null buffer");
  if (h->session) return fail(GRL_ERR_STATE, "a behaviour-cloning session is open on this handle (grl_bc_end)");
  if (int e = check_bc(h, c)) return e;
  return session_open(h, session_fill<BcPlan>(h, c), buf, c->lr, "bc");
}

// a call's index rows on the host, checked before anything moves
static int bc_check_idx(grl_handle h, const int32_t* idx, int64_t n_rows, int n) {
  BcPlan& p = *h->bc();
  const int batch = p.cfg.batch;
  p.idx_host.resize((size_t)n * batch);
  HIPCHK(hipMemcpyAsync(p.idx_host.data(), idx, p.idx_host.size() * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return check_tail_rows(p.idx_host.data(), n, batch, n_rows, [](int, int) { return 0; },
                         [](int u, int b) { return "bc: index row " + std::to_string(u) + ", entry " + std::to_string(b); }, nullptr);
}

static int bc_run(grl_handle h, const char* what, const float* obs, const float* act, int64_t n_rows, const int32_t* idx, int n, bool train) {
  if (!h->bc()) return fail(GRL_ERR_STATE, std::string(what) + " needs an open session (grl_bc_begin)");
  if (!obs || !act || !idx || n_rows < 1) return fail(GRL_ERR_INVALID, "bc: null table or indices");
  if (n < 1 || n > GRL_BC_MAX_UPDATES) return fail(GRL_ERR_INVALID, "bc: the count of a call must be 1..65536");
  if (int e = bc_check_idx(h, idx, n_rows, n)) return e;
  BcPlan& p = *h->bc();
  hipLaunchKernelGGL(bc_open_kernel, dim3(1), dim3(1), 0, h->stream, p.dev, obs, act, idx);
  if (int e = h->run_repeated(train ? "bc_train" : "bc_eval", {train ? &p.ops_train : &p.ops_eval}, n)) return e;
  HIPCHK(hipGetLastError());
  p.last_n = n;
  return GRL_OK;
}

int grl_bc_train(grl_handle h, const float* obs, const float* act, int64_t n_rows, const int32_t* idx, int n_updates) {
  SAC_ONLY(h, "grl_bc_train");
  return bc_run(h, "grl_bc_train", obs, act, n_rows, idx, n_updates, true);
}

int grl_bc_eval(grl_handle h, const float* obs, const float* act, int64_t n_rows, const int32_t* idx, int n_batches) {
  SAC_ONLY(h, "grl_bc_eval");
  return bc_run(h, "grl_bc_eval", obs, act, n_rows, idx, n_batches, false);
}

int grl_bc_get_losses(grl_handle h, float* out, int cap) {
  SAC_ONLY(h, "grl_bc_get_losses");
  BcPlan* p = h->bc();
  if (!p) return fail(GRL_ERR_STATE, "grl_bc_get_losses needs an open session (grl_bc_begin)");
  if (!out || cap < p->last_n) return fail(GRL_ERR_INVALID, "bc: loss buffer too small");
  HIPCHK(hipStreamSynchronize(h->stream));
  if (p->last_n) HIPCHK(hipMemcpy(out, p->losses, (size_t)p->last_n * 4, hipMemcpyDeviceToHost));
  return p->last_n;
}

int grl_bc_end(grl_handle h) {
  SAC_ONLY(h, "grl_bc_end");
  if (!h->bc()) return fail(GRL_ERR_STATE, "grl_bc_end needs an open session (grl_bc_begin)");
  HIPCHK(hipStreamSynchronize(h->stream));
  h->session_drop();
  return GRL_OK;
}

static int check_gail(grl_handle h, const grl_gail_config* c) {
  if (!c || !c->act_low || !c->act_high) return fail(GRL_ERR_INVALID, "null GAIL config or action bounds");
  if (c->hidden < 1 || c->hidden > 1024) return fail(GRL_ERR_INVALID, "gail: hidden must be 1..1024 (" + std::to_string(c->hidden) + ")");
  if (c->batch < 1 || c->batch > h->tcfg.n_steps)
    return fail(GRL_ERR_INVALID, "gail: batch " + std::to_string(c->batch) + " is outside 1.." + std::to_string(h->tcfg.n_steps) + " (the handle's n_steps)");
  if (!(c->lr > 0.f) || !(c->adam_eps > 0.f) || !std::isfinite(c->entcoeff)) return fail(GRL_ERR_INVALID, "gail: lr and adam_eps must be > 0, entcoeff finite");
  return check_act_bounds(h, c->act_low, c->act_high, "gail");
}

int grl_gail_query_sizes(grl_handle h, const grl_gail_config* c, size_t* bytes) {
  TRPO_ONLY(h, "grl_gail_query_sizes");
  if (!bytes) return fail(GRL_ERR_INVALID, "null out");
  if (int e = check_gail(h, c)) return e;
  return session_query(h, session_fill<GailPlan>(h, c), bytes);
}

static int gail_store_stats(grl_handle h, const double* sum, const double* sumsq, double count) {
  GailPlan& p = *h->gail();
  const std::vector<double> cnt((size_t)p.od, count);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(p.sum, sum, (size_t)p.od * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(p.sumsq, sumsq, (size_t)p.od * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(p.count, cnt.data(), (size_t)p.od * 8, hipMemcpyHostToDevice));
  // the float32 mean / std the reward pass reads: the device's own arithmetic (gail_mean_sd), run here on the host
  std::vector<float> mean((size_t)p.od), sd((size_t)p.od);
  for (int c = 0; c < p.od; ++c) gail_mean_sd(sum[c], sumsq[c], count, mean[(size_t)c], sd[(size_t)c]);
  HIPCHK(hipMemcpy(p.mean, mean.data(), (size_t)p.od * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(p.sd, sd.data(), (size_t)p.od * 4, hipMemcpyHostToDevice));
  return GRL_OK;
}

int grl_gail_begin(grl_handle h, const grl_gail_config* c, void* buf) {
  TRPO_ONLY(h, "grl_gail_begin");
  if (!buf) return fail(GRL_ERR_INVALID, "null buffer");
  if (h->session) return fail(GRL_ERR_STATE, "a GAIL session is open on this handle (grl_gail_end)");
  if (int e = check_gail(h, c)) return e;
  if (int e = session_open(h, session_fill<GailPlan>(h, c), buf, c->lr, "gail")) return e;
  // the statistics' start
  const int od = h->gail()->od;
  const std::vector<double> sum0((size_t)od, 0.0), sumsq0((size_t)od, 1e-2);
  if (int e = gail_store_stats(h, sum0.data(), sumsq0.data(), 1e-2)) { h->session_drop(); return e; }
  h->gail_rewritten = false;
  return GRL_OK;
}

int grl_gail_param_info(grl_handle h, int i, char* name, int cap, int64_t* off, int64_t* numel, int32_t* rows, int32_t* cols) {
  GAIL_SESSION(h, "grl_gail_param_info");
  if (i < 0 || i >= 6) return fail(GRL_ERR_INVALID, "gail: parameter index must be 0..5");
  const GailPlan::Tensor& t = h->gail()->tensors[i];
  if (name && cap > 0) { strncpy(name, t.name, cap - 1); name[cap - 1] = 0; }
  if (off) *off = t.off;
  if (numel) *numel = t.numel;
  if (rows) *rows = t.rows;
  if (cols) *cols = t.cols;
  return 6;
}

int grl_gail_rewards(grl_handle h) {
  GAIL_SESSION(h, "grl_gail_rewards");
  if (h->ppo_closed != h->pcfg.n_steps || h->ppo_finished)
    return fail(GRL_ERR_STATE, "grl_gail_rewards rewrites the rewards of a full rollout that grl_ppo_finish has not closed yet: n_steps slots must be closed");
  if (h->gail_rewritten) return fail(GRL_ERR_STATE, "grl_gail_rewards: the rewards of this rollout are the discriminator's already");
  if (int e = h->run_seq("gail_rewards", {&h->gail()->ops_rewards})) return e;
  HIPCHK(hipGetLastError());
  h->gail_rewritten = true;
  return GRL_OK;
}

// a call's index rows on the host: generator rows all present and inside the rollout; expert rows by check_tail_rows
static int gail_check_idx(grl_handle h, const int32_t* gen_idx, const int32_t* exp_idx, int64_t n_rows, int n, std::vector<int>& ne) {
  GailPlan& p = *h->gail();
  const int batch = p.cfg.batch, T = h->tcfg.n_steps;
  const size_t cnt = (size_t)n * batch;
  p.idx_host.resize(2 * cnt);
  HIPCHK(hipMemcpyAsync(p.idx_host.data(), gen_idx, cnt * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(p.idx_host.data() + cnt, exp_idx, cnt * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const int32_t* gen = p.idx_host.data();
  auto entry = [](int u, int b) { return "update " + std::to_string(u) + ", entry " + std::to_string(b); };
  return check_tail_rows(gen + cnt, n, batch, n_rows, [&](int u, int b) {
    const int32_t g = gen[(size_t)u * batch + b];
    if (g >= 0 && g < T) return 0;
    return fail(GRL_ERR_INVALID, "gail: generator index of " + entry(u, b) + " is outside the rollout (" + std::to_string(g) + ")");
  }, [&](int u, int b) { return "gail: expert index of " + entry(u, b); }, &ne);
}

int grl_gail_update(grl_handle h, const float* exp_obs, const float* exp_act, int64_t n_rows, const int32_t* gen_idx,
                    const int32_t* exp_idx, int n_updates) {
  GAIL_SESSION(h, "grl_gail_update");
  if (n_updates < 1 || n_updates > GRL_GAIL_MAX_UPDATES) return fail(GRL_ERR_INVALID, "gail: the count of a call must be 1..4096");
  if (!exp_obs || !exp_act || !gen_idx || !exp_idx || n_rows < 1) return fail(GRL_ERR_INVALID, "gail: null table or indices");
  if (!h->ppo_held) return fail(GRL_ERR_STATE, "grl_gail_update reads the last finished rollout: none is held (grl_ppo_finish .. the next grl_ppo_step)");
  GailPlan& p = *h->gail();
  std::vector<int> ne;
  if (int e = gail_check_idx(h, gen_idx, exp_idx, n_rows, n_updates, ne)) return e;
  launch_gail_open(p.dev, exp_obs, exp_act, gen_idx, exp_idx, h->stream);
  if (int e = h->run_repeated("gail_update", {&p.ops_update}, n_updates)) return e;
  HIPCHK(hipGetLastError());
  p.last_n = n_updates;
  p.last_ne = ne;
  return GRL_OK;
}

int grl_gail_get_losses(grl_handle h, float* out, int cap) {
  GAIL_SESSION(h, "grl_gail_get_losses");
  GailPlan& p = *h->gail();
  const int nu = p.last_n, nb = p.nblk;
  if (!out || cap < nu * GAIL_DIAG) return fail(GRL_ERR_INVALID, "gail: loss buffer too small");
  std::vector<float> part((size_t)std::max(1, nu * nb * GAIL_DIAG));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (nu) HIPCHK(hipMemcpy(part.data(), p.diag, (size_t)nu * nb * GAIL_DIAG * 4, hipMemcpyDeviceToHost));
  for (int u = 0; u < nu; ++u) {
    float s[GAIL_DIAG] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < nb; ++b)      // the per-block sums of the loss launch, in index order
      for (int k = 0; k < GAIL_DIAG; ++k) s[k] += part[((size_t)u * nb + b) * GAIL_DIAG + k];
    const float n_g = (float)p.cfg.batch, n_e = (float)p.last_ne[(size_t)u];
    float* o = out + (size_t)u * GAIL_DIAG;
    o[0] = s[0] / n_g; o[1] = s[1] / n_e; o[2] = s[2] / (n_g + n_e); o[3] = -p.cfg.entcoeff * o[2]; o[4] = s[4] / n_g; o[5] = s[5] / n_e;
  }
  return nu;
}

int grl_gail_get_stats(grl_handle h, double* sum, double* sumsq, double* count) {
  GAIL_SESSION(h, "grl_gail_get_stats");
  if (!sum || !sumsq || !count) return fail(GRL_ERR_INVALID, "null argument");
  GailPlan& p = *h->gail();
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(sum, p.sum, (size_t)p.od * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(sumsq, p.sumsq, (size_t)p.od * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(count, p.count, 8, hipMemcpyDeviceToHost));
  return GRL_OK;
}

int grl_gail_set_stats(grl_handle h, const double* sum, const double* sumsq, double count) {
  GAIL_SESSION(h, "grl_gail_set_stats");
  if (!sum || !sumsq || !(count > 0.0)) return fail(GRL_ERR_INVALID, "gail: null statistics or a count that is not positive");
  return gail_store_stats(h, sum, sumsq, count);
}

int grl_gail_end(grl_handle h) {
  GAIL_SESSION(h, "grl_gail_end");
  HIPCHK(hipStreamSynchronize(h->stream));
  h->session_drop();
  return GRL_OK;
}

#include "checkpoint.inl"
#include "ppo_checkpoint.inl"

}  // extern "C"
