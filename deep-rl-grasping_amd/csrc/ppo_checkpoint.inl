// ppo_checkpoint.inl: grl_ppo_state_size / _export / _import (include/grl.h, DESIGN.md "Checkpoints of the on-policy models") --
// part of capi.inl (included inside its extern "C" block, behind checkpoint.inl whose header, field table and hash it shares).
// Host code only, valid on PPO and TRPO handles: the arenas are the caller's, who copies them; what moves here is what a later
// grl_ppo_step / _rewards / _finish / _train, grl_trpo_update or grl_observe reads and plan() does not derive from the
// configuration:
//   ppo_stepped, ppo_closed, ppo_finished   the rollout cursor (PpoDev.slot in the state arena is the device mirror of ppo_closed)
//   n_parity                                which half of the double-buffered running count is current (state arena: n_count[2])
//   ppo_observed, ppo_obs_n                 normalize = 2: whether grl_observe has normalised rows, and those rows [n_envs, ldo] --
//                                           the only training state kept in the WORK arena (obs == NULL acts on them)
// Everything else is in the two arenas the caller copies -- parameters, Adam moments, DevScalars with the beta powers, the learning
// rate and the Philox counter, PpoDev, TrpoDev and the float64 statistics in the STATE arena; the rollout with the last values and
// flags in the REPLAY arena -- or is derived (layout, plans, tables), a per-call argument (what ppo_send uploads: observations,
// flags, noise, rewards; the permutations), staging no later call reads (n_stage: the raw rows, normalised in the launch that
// uploads them), the diagnostics of the last training call (ppo_diag, ppo_updates: read by grl_ppo_get_metrics right behind it)
// or TRPO's scratch between the launches of one update (theta_old, the CG vectors, the line-search words): an update is never
// interrupted.

// Shared (checkpoint.inl): state_write_head / state_read_head for the header and the grl_config, CfgBlock for the second block.

#define GRL_PCFG_FIELD(f) {#f, offsetof(grl_ppo_config, f), sizeof(((grl_ppo_config*)nullptr)->f)}
static const CfgField k_pcfg_fields[] = {
  GRL_PCFG_FIELD(n_envs), GRL_PCFG_FIELD(n_steps), GRL_PCFG_FIELD(n_vf_layers), GRL_PCFG_FIELD(vf_layers), GRL_PCFG_FIELD(lam),
  GRL_PCFG_FIELD(clip_range), GRL_PCFG_FIELD(clip_range_vf), GRL_PCFG_FIELD(ent_coef), GRL_PCFG_FIELD(vf_coef),
  GRL_PCFG_FIELD(max_grad_norm), GRL_PCFG_FIELD(adam_eps), GRL_PCFG_FIELD(norm_eps64),
};
#undef GRL_PCFG_FIELD
#define GRL_TCFG_FIELD(f) {#f, offsetof(grl_trpo_config, f), sizeof(((grl_trpo_config*)nullptr)->f)}
static const CfgField k_tcfg_fields[] = {
  GRL_TCFG_FIELD(n_steps), GRL_TCFG_FIELD(n_vf_layers), GRL_TCFG_FIELD(vf_layers), GRL_TCFG_FIELD(cg_iters), GRL_TCFG_FIELD(ls_steps),
  GRL_TCFG_FIELD(fvp_stride), GRL_TCFG_FIELD(vf_batch), GRL_TCFG_FIELD(lam), GRL_TCFG_FIELD(max_kl), GRL_TCFG_FIELD(cg_damping),
  GRL_TCFG_FIELD(ent_coef), GRL_TCFG_FIELD(adam_eps), GRL_TCFG_FIELD(norm_eps64),
};
#undef GRL_TCFG_FIELD

// the second configuration block of the handle
static CfgBlock ppo_cfg2(const grl_ctx* h) {
  if (h->cfg.algo == GRL_ALGO_TRPO)
    return {k_tcfg_fields, (int)(sizeof(k_tcfg_fields) / sizeof(CfgField)), (const char*)&h->tcfg, sizeof(grl_trpo_config), "grl_trpo_config"};
  return {k_pcfg_fields, (int)(sizeof(k_pcfg_fields) / sizeof(CfgField)), (const char*)&h->pcfg, sizeof(grl_ppo_config), "grl_ppo_config"};
}

// cfg_hash of the grl_config, continued over the fields of the second block in field order
static uint64_t ppo_cfg_hash(const grl_ctx* h) { return ppo_cfg2(h).hash(cfg_hash(h->cfg)); }

struct PpoStateHost {      // follows the header and the two configuration blocks in the blob
  int32_t written, closed, finished;      // ppo_stepped, ppo_closed, ppo_finished
  int32_t n_parity;
  int32_t ob_n, pad;                      // rows grl_observe has normalised: 0 or n_envs
  int64_t ob_elems;                       // floats per normalised row: rup(obs_dim, 4)
};

static size_t ppo_state_bytes_now(const grl_ctx* h) {
  return sizeof(grl_state_header) + sizeof(grl_config) + ppo_cfg2(h).bytes + sizeof(PpoStateHost) +
         (h->ppo_observed ? (size_t)h->NA * (size_t)h->ppo_ldo * 4 : 0);
}

int grl_ppo_state_size(grl_handle h, size_t* bytes) {
  ROLLOUT_ONLY(h, "grl_ppo_state_size");
  if (!bytes) return fail(GRL_ERR_INVALID, "null argument");
  *bytes = ppo_state_bytes_now(h);
  return GRL_OK;
}

int64_t grl_ppo_state_export(grl_handle h, void* host_buf, size_t cap) {
  ROLLOUT_ONLY(h, "grl_ppo_state_export");
  if (!host_buf) return fail(GRL_ERR_INVALID, "null argument");
  const size_t total = ppo_state_bytes_now(h);
  if (cap < total) return fail(GRL_ERR_INVALID, "state buffer too small: " + std::to_string(total) + " bytes needed");
  HIPCHK(hipStreamSynchronize(h->stream));
  // (replay_pos / replay_size stay 0: a rollout has a cursor of its own, below)
  char* p = ppo_cfg2(h).write(state_write_head(h, (char*)host_buf, ppo_cfg_hash(h), 0, 0, total));
  PpoStateHost sh;
  memset(&sh, 0, sizeof(sh));
  sh.written = h->ppo_stepped; sh.closed = h->ppo_closed; sh.finished = h->ppo_finished ? 1 : 0;
  sh.n_parity = h->n_parity; sh.ob_n = h->ppo_observed ? h->NA : 0; sh.ob_elems = h->ppo_ldo;
  memcpy(p, &sh, sizeof(sh)); p += sizeof(sh);
  const size_t nr = (size_t)sh.ob_n * (size_t)sh.ob_elems * 4;
  if (nr) HIPCHK(hipMemcpy(p, h->ppo_obs_n, nr, hipMemcpyDeviceToHost));
  return (int64_t)total;
}

int grl_ppo_state_import(grl_handle h, const void* host_buf, size_t n) {
  ROLLOUT_ONLY(h, "grl_ppo_state_import");
  if (!host_buf) return fail(GRL_ERR_INVALID, "null argument");
  const char* p = (const char*)host_buf;
  grl_state_header hd;
  grl_config c;
  if (int e = state_read_head(&p, n, false, 0, hd, c)) return e;
  // the kind of handle first: the second configuration block of the other kind has another shape
  auto kind = [](int algo) { return algo == GRL_ALGO_PPO ? "a PPO handle" : algo == GRL_ALGO_TRPO ? "a TRPO handle" : "a handle that keeps no rollout (grl_state_export)"; };
  if (c.algo != h->cfg.algo)
    return fail(GRL_ERR_INVALID, std::string("state blob was written by ") + kind(c.algo) + ", this is " + kind(h->cfg.algo));
  const CfgBlock q = ppo_cfg2(h);
  const size_t fixed = sizeof(hd) + sizeof(grl_config) + q.bytes + sizeof(PpoStateHost);
  if (n < fixed) return fail(GRL_ERR_INVALID, "state blob is truncated (" + std::to_string(n) + " bytes, " + std::to_string(fixed) + " before the observed rows)");
  if (int e = cfg_block(h).differs((const char*)&c)) return e;
  if (int e = q.differs(p)) return e;
  p += q.bytes;
  if (hd.config_hash != ppo_cfg_hash(h)) return fail(GRL_ERR_INVALID, "state blob is damaged (configuration hash)");
  PpoStateHost sh;
  memcpy(&sh, p, sizeof(sh)); p += sizeof(sh);
  const int T = h->pcfg.n_steps;
  if (sh.closed < 0 || sh.closed > T || sh.written < sh.closed || sh.written > sh.closed + 1 || sh.written > T || (sh.finished & ~1) ||
      (sh.finished && sh.closed != T) || (sh.n_parity & ~1) || sh.ob_n < 0 || sh.ob_n > h->NA || (sh.ob_n != 0 && sh.ob_n != h->NA) ||
      sh.ob_elems != h->ppo_ldo || (sh.ob_n && !h->ppo_obs_n))
    return fail(GRL_ERR_INVALID, "state blob is damaged (host fields out of range)");
  const size_t nr = (size_t)sh.ob_n * (size_t)sh.ob_elems * 4;
  if (n != fixed + nr) return fail(GRL_ERR_INVALID, "state blob is truncated (observed rows)");
  HIPCHK(hipStreamSynchronize(h->stream));
  // ---- nothing below fails on bad input
  if (nr) HIPCHK(hipMemcpy(h->ppo_obs_n, p, nr, hipMemcpyHostToDevice));
  h->ppo_stepped = sh.written; h->ppo_closed = sh.closed; h->ppo_finished = sh.finished != 0;
  h->ppo_held = h->ppo_finished; h->gail_rewritten = false;
  h->n_parity = sh.n_parity; h->ppo_observed = sh.ob_n != 0;
  HIPCHK(hipMemcpy(&h->ppo_dev->slot, &sh.closed, 4, hipMemcpyHostToDevice));      // the device mirror follows the blob
  return GRL_OK;
}
