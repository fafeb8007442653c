// checkpoint.inl: grl_state_size / _export / _import and grl_replay_segments (include/grl.h, DESIGN.md "Checkpoints") -- part of
// capi.inl (included inside its extern "C" block).  Host code only: the arenas are the caller's, who copies them; what moves
// here is the handful of grl_ctx fields that an update, an act, a grl_observe / grl_replay_add_observed pair, a prioritised
// step or a grl_norm_update reads and that plan() does not derive from the configuration:
//   rp_pos, rp_size               ring cursor and fill (DevScalars.replay_size is the device mirror of rp_size)
//   n_parity                      which half of the double-buffered running count is current (state arena: n_count[2])
//   ob_n, ob_n_prev               rows grl_observe holds in ob_latest / ob_prev -- and those rows themselves, the only
//                                 training state kept in the WORK arena
// Everything else in grl_ctx is either derived (layout, plans, tables, graphs), a per-call argument (grad_scale,
// apply_graph_scale), staging whose content no later call reads (pin_*, stg_*, n_stage, ob_term), a completion counter that
// lives and dies with the handle (act_done_seen against act_done_host), or belongs to a data-parallel connection, which is
// set up anew after a restart (dp_*).  The prioritised-replay state is all in the replay arena (PerArgs holds addresses and
// configuration constants only).
// Shared with ppo_checkpoint.inl: CfgField (the row type of every field table), CfgBlock (a configuration struct of the handle with
// its table: written, compared and hashed field by field), state_write_head / state_read_head (the header and the grl_config).

struct CfgField { const char* name; size_t off, size; };
#define GRL_CFG_FIELD(f) {#f, offsetof(grl_config, f), sizeof(((grl_config*)nullptr)->f)}
static const CfgField k_cfg_fields[] = {
  GRL_CFG_FIELD(extractor), GRL_CFG_FIELD(img_hw), GRL_CFG_FIELD(obs_channels), GRL_CFG_FIELD(n_direct), GRL_CFG_FIELD(obs_dim),
  GRL_CFG_FIELD(act_dim), GRL_CFG_FIELD(n_layers), GRL_CFG_FIELD(layers), GRL_CFG_FIELD(batch_size), GRL_CFG_FIELD(act_batch),
  GRL_CFG_FIELD(replay_capacity), GRL_CFG_FIELD(normalize), GRL_CFG_FIELD(gamma), GRL_CFG_FIELD(lr), GRL_CFG_FIELD(tau),
  GRL_CFG_FIELD(clip_obs), GRL_CFG_FIELD(clip_reward), GRL_CFG_FIELD(norm_eps), GRL_CFG_FIELD(target_entropy), GRL_CFG_FIELD(seed),
  GRL_CFG_FIELD(algo), GRL_CFG_FIELD(q_branches), GRL_CFG_FIELD(q_bins), GRL_CFG_FIELD(q_n_common), GRL_CFG_FIELD(q_common),
  GRL_CFG_FIELD(q_n_branch), GRL_CFG_FIELD(q_branch), GRL_CFG_FIELD(q_n_value), GRL_CFG_FIELD(q_value), GRL_CFG_FIELD(q_huber),
  GRL_CFG_FIELD(q_double), GRL_CFG_FIELD(q_grad_clip), GRL_CFG_FIELD(q_trunk_scale), GRL_CFG_FIELD(q_per), GRL_CFG_FIELD(q_per_alpha),
  GRL_CFG_FIELD(q_per_eps), GRL_CFG_FIELD(replay_rgb_u8), GRL_CFG_FIELD(q_per_stratified), GRL_CFG_FIELD(q_per_alpha64),
  GRL_CFG_FIELD(q_loss_sum_branches), GRL_CFG_FIELD(q_layer_norm), GRL_CFG_FIELD(ae_kernel), GRL_CFG_FIELD(ae_filters),
  GRL_CFG_FIELD(ae_encoding_dim), GRL_CFG_FIELD(ae_alpha),
};
#undef GRL_CFG_FIELD

// FNV-1a over the bytes of every field in field order (padding between fields never enters).  q_layer_norm, appended after
// blobs of this layout existed, enters only when set: a blob written before the field existed hashes as it did then (its
// configuration bytes hold zeros there) and is still accepted by a handle without layer normalisation.  The ae_* fields
// (the auto-encoder's network, appended later still) follow the same rule: all zero -- the shipped network, cfg_ae_default in plan_ae.inl -- they stay out.
static uint64_t fnv1a(uint64_t hsh, const char* p, size_t n) {
  for (size_t k = 0; k < n; ++k) hsh = (hsh ^ (uint8_t)p[k]) * 0x100000001b3ull;
  return hsh;
}
static uint64_t cfg_hash(const grl_config& c) {
  uint64_t hsh = 0xcbf29ce484222325ull;
  for (const auto& f : k_cfg_fields) {
    if (f.off == offsetof(grl_config, q_layer_norm) && c.q_layer_norm == 0) continue;
    if (f.off >= offsetof(grl_config, ae_kernel) && cfg_ae_default(c)) continue;
    hsh = fnv1a(hsh, (const char*)&c + f.off, f.size);
  }
  return hsh;
}

struct CfgBlock {
  const CfgField* field; int n;
  const char* base; size_t bytes;      // the handle's struct
  const char* type;
  // field by field into zeroed storage: the blob holds no padding bytes of the caller's struct
  char* write(char* p) const {
    memset(p, 0, bytes);
    for (int f = 0; f < n; ++f) memcpy(p + field[f].off, base + field[f].off, field[f].size);
    return p + bytes;
  }
  // refuses, by the name of the first field that differs, a block at `blob` that is not the handle's
  int differs(const char* blob) const {
    for (int f = 0; f < n; ++f)
      if (memcmp(blob + field[f].off, base + field[f].off, field[f].size) != 0)
        return fail(GRL_ERR_INVALID, std::string("state blob was written for another configuration: ") + type + "." + field[f].name + " differs");
    return GRL_OK;
  }
  uint64_t hash(uint64_t hsh) const {
    for (int f = 0; f < n; ++f) hsh = fnv1a(hsh, base + field[f].off, field[f].size);
    return hsh;
  }
};
static CfgBlock cfg_block(const grl_ctx* h) {
  return {k_cfg_fields, (int)(sizeof(k_cfg_fields) / sizeof(k_cfg_fields[0])), (const char*)&h->cfg, sizeof(grl_config), "grl_config"};
}

// header + the zeroed grl_config of a blob of `total` bytes; returns where the next section starts
static char* state_write_head(const grl_ctx* h, char* p, uint64_t hash, int64_t replay_pos, int64_t replay_size, size_t total) {
  grl_state_header hd;
  memset(&hd, 0, sizeof(hd));
  hd.magic = GRL_STATE_MAGIC; hd.version = grl_version(); hd.layout = GRL_STATE_LAYOUT;
  hd.config_bytes = (int32_t)sizeof(grl_config); hd.config_hash = hash;
  hd.replay_pos = replay_pos; hd.replay_size = replay_size; hd.total_bytes = total;
  memcpy(p, &hd, sizeof(hd));
  return cfg_block(h).write(p + sizeof(hd));
}
// The header of a blob of n bytes, checked (magic, versions, size of its grl_config, length: at least `tail` bytes behind the
// configuration, and what the header says), and its grl_config into zeroed `c`.  short_cfg: a blob written before the ae_* fields
// were appended holds the struct up to them -- they read as zeros, the shipped network.  *p: where the next section starts.
static int state_read_head(const char** p, size_t n, bool short_cfg, size_t tail, grl_state_header& hd, grl_config& c) {
  if (n < sizeof(hd)) return fail(GRL_ERR_INVALID, "state blob is truncated (no header)");
  memcpy(&hd, *p, sizeof(hd)); *p += sizeof(hd);
  if (hd.magic != GRL_STATE_MAGIC) return fail(GRL_ERR_INVALID, "not a grl state blob (wrong magic)");
  if (hd.version != grl_version())
    return fail(GRL_ERR_INVALID, "state blob written by library version " + std::to_string(hd.version) + ", this is " + std::to_string(grl_version()));
  if (hd.layout != GRL_STATE_LAYOUT) return fail(GRL_ERR_INVALID, "state blob has layout version " + std::to_string(hd.layout) + ", expected " + std::to_string(GRL_STATE_LAYOUT));
  const size_t csz = (size_t)hd.config_bytes;
  if (csz != sizeof(grl_config) && !(short_cfg && csz == offsetof(grl_config, ae_kernel))) return fail(GRL_ERR_INVALID, "state blob holds a grl_config of another size");
  if (n < sizeof(hd) + csz + tail || hd.total_bytes != n) return fail(GRL_ERR_INVALID, "state blob is truncated (" + std::to_string(n) + " of " + std::to_string(hd.total_bytes) + " bytes)");
  memset(&c, 0, sizeof(c));
  memcpy(&c, *p, csz); *p += csz;
  return GRL_OK;
}

struct StateHost {     // follows the header and the grl_config in the blob
  int32_t n_parity, ob_n, ob_n_prev, pad;
  int64_t ob_elems;    // floats per observed row
};

static size_t state_bytes_now(const grl_ctx* h) {
  return sizeof(grl_state_header) + sizeof(grl_config) + sizeof(StateHost) +
         (size_t)(h->ob_n + h->ob_n_prev) * (size_t)h->ob_elems * 4;
}

int grl_state_size(grl_handle h, size_t* bytes) {
  NOT_ON_PPO(h, "grl_state_size");
  NOT_ON_TD3(h, "grl_state_size");
  if (!h || !bytes) return fail(GRL_ERR_INVALID, "null argument");
  *bytes = state_bytes_now(h);
  return GRL_OK;
}

int64_t grl_state_export(grl_handle h, void* host_buf, size_t cap) {
  NOT_ON_PPO(h, "grl_state_export");
  NOT_ON_TD3(h, "grl_state_export");
  if (!h || !host_buf) return fail(GRL_ERR_INVALID, "null argument");
  const size_t total = state_bytes_now(h);
  if (cap < total) return fail(GRL_ERR_INVALID, "state buffer too small: " + std::to_string(total) + " bytes needed");
  HIPCHK(hipStreamSynchronize(h->stream));
  char* p = state_write_head(h, (char*)host_buf, cfg_hash(h->cfg), h->rp_pos, h->rp_size, total);
  StateHost sh;
  memset(&sh, 0, sizeof(sh));
  sh.n_parity = h->n_parity; sh.ob_n = h->ob_n; sh.ob_n_prev = h->ob_n_prev; sh.ob_elems = h->ob_elems;
  memcpy(p, &sh, sizeof(sh)); p += sizeof(sh);
  const size_t nl = (size_t)h->ob_n * h->ob_elems * 4, np = (size_t)h->ob_n_prev * h->ob_elems * 4;
  if (nl) HIPCHK(hipMemcpy(p, h->ob_latest, nl, hipMemcpyDeviceToHost));
  p += nl;
  if (np) HIPCHK(hipMemcpy(p, h->ob_prev, np, hipMemcpyDeviceToHost));
  return (int64_t)total;
}

int grl_state_import(grl_handle h, const void* host_buf, size_t n) {
  NOT_ON_PPO(h, "grl_state_import");
  NOT_ON_TD3(h, "grl_state_import");
  if (!h || !host_buf) return fail(GRL_ERR_INVALID, "null argument");
  const char* p = (const char*)host_buf;
  grl_state_header hd;
  grl_config c;
  if (int e = state_read_head(&p, n, true, sizeof(StateHost), hd, c)) return e;
  const size_t fixed = (size_t)(p - (const char*)host_buf) + sizeof(StateHost);
  if (int e = cfg_block(h).differs((const char*)&c)) return e;
  if (hd.config_hash != cfg_hash(h->cfg)) return fail(GRL_ERR_INVALID, "state blob is damaged (configuration hash)");
  StateHost sh;
  memcpy(&sh, p, sizeof(sh)); p += sizeof(sh);
  const int64_t cap = h->cfg.replay_capacity;
  if (hd.replay_size < 0 || hd.replay_size > cap || hd.replay_pos < 0 || hd.replay_pos >= cap || (sh.n_parity & ~1) ||
      sh.ob_n < 0 || sh.ob_n_prev < 0 || sh.ob_n > h->stg_n || sh.ob_n_prev > h->stg_n || sh.ob_elems != h->ob_elems ||
      ((sh.ob_n || sh.ob_n_prev) && !h->ob_latest))
    return fail(GRL_ERR_INVALID, "state blob is damaged (host fields out of range)");
  const size_t nl = (size_t)sh.ob_n * sh.ob_elems * 4, np = (size_t)sh.ob_n_prev * sh.ob_elems * 4;
  if (n != fixed + nl + np) return fail(GRL_ERR_INVALID, "state blob is truncated (observed rows)");
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->dp_on) {     // an exchange is in flight while some rank has announced one that this rank has not begun, or the reverse
    if (h->dp_err_host.get() && *h->dp_err_host.get()) return fail(GRL_ERR_STATE, "an exchange timed out waiting for a peer (the replicas are no longer in step)");
    for (int k = 0; k < DP_CHANNELS; ++k) {
      DpCtl ctl;
      HIPCHK(hipMemcpy(&ctl, (char*)h->dp_flags + k * dp_ctl_stride(), sizeof(DpCtl), hipMemcpyDeviceToHost));
      for (int r = 0; r < h->dp.world; ++r)
        if (ctl.ready[r] != ctl.epoch) return fail(GRL_ERR_STATE, "a data-parallel exchange is in flight: drain and synchronise all ranks before importing state");
    }
  }
  // ---- nothing below fails on bad input
  if (nl) HIPCHK(hipMemcpy(h->ob_latest, p, nl, hipMemcpyHostToDevice));
  p += nl;
  if (np) HIPCHK(hipMemcpy(h->ob_prev, p, np, hipMemcpyHostToDevice));
  h->rp_pos = hd.replay_pos; h->rp_size = hd.replay_size;
  h->n_parity = sh.n_parity; h->ob_n = sh.ob_n; h->ob_n_prev = sh.ob_n_prev;
  HIPCHK(hipMemcpy(&h->sc->replay_size, &hd.replay_size, 8, hipMemcpyHostToDevice));   // the device mirror follows the blob
  if (h->per_on && hd.replay_size == 0) HIPCHK(per_start(h));     // ring left out: the priority tree starts over as in grl_create
  return GRL_OK;
}

int grl_replay_segments(grl_handle h, int cap, grl_segment* out) {
  NOT_ON_PPO(h, "grl_replay_segments");
  NOT_ON_TD3(h, "grl_replay_segments");
  if (!h || (cap > 0 && !out)) return fail(GRL_ERR_INVALID, "null argument");
  std::vector<grl_segment> s;
  if (h->cfg.algo != GRL_ALGO_AE) {
    const grl_config& c = h->cfg;
    const int64_t rows = c.replay_capacity;
    const bool sac = c.algo == GRL_ALGO_SAC;
    const int64_t obs_store = (sac && c.replay_rgb_u8) ? 2 * (int64_t)h->hw * h->hw : h->img_elems;
    const int64_t nd = (sac && h->cnn) ? h->F - 512 : 0;      // direct features per row (0: the placeholder arrays are never touched)
    auto rowwise = [&](const void* ptr, int64_t row_bytes) {
      s.push_back({(uint64_t)((const char*)ptr - h->rp.base), (uint64_t)row_bytes, rows});
    };
    auto whole = [&](const void* ptr, size_t bytes) { s.push_back({(uint64_t)((const char*)ptr - h->rp.base), (uint64_t)bytes, 0}); };
    rowwise(h->rp_obs, obs_store * 4); rowwise(h->rp_next, obs_store * 4);
    if (nd > 0) { rowwise(h->rp_dobs, nd * 4); rowwise(h->rp_dnext, nd * 4); }
    rowwise(h->rp_act, (int64_t)h->A * 4); rowwise(h->rp_rew, 4); rowwise(h->rp_done, 4);
    if (h->per_on) {
      rowwise(h->per.p, 8);
      whole(h->per.bsum, (size_t)h->per_blocks * 8); whole(h->per.bmin, (size_t)h->per_blocks * 8);
      whole(h->per.st, sizeof(PerState));
    }
  }
  if ((int)s.size() > cap) return fail(GRL_ERR_INVALID, "segment buffer too small: " + std::to_string(s.size()) + " entries needed");
  for (size_t k = 0; k < s.size(); ++k) out[k] = s[k];
  return (int)s.size();
}
