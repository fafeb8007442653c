// handle_lifetime_check.cpp -- what a handle owns outside the caller's arenas (csrc/host_res.h: page-locked blocks, events, the two
// staging rings, the launches, the exchange's allocations) over the life of every kind of handle, through include/grl.h alone, as a
// STAND-ALONE program for AddressSanitizer + UBSan + the leak checker (tests/test_handle_lifetime_sanitized.py links it with the
// emulation build of the library, whose page-locked blocks and events are heap blocks).  Every arena is a heap block of exactly
// the queried size.  A block or event freed twice, used after its release or left behind shows as a sanitizer report.
// Prints "<n> checks, 0 failed".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "grl.h"

static int n_checks = 0, n_failed = 0;
#define CHECK(cond)                                                                                  \
  do {                                                                                               \
    ++n_checks;                                                                                      \
    if (!(cond)) { ++n_failed; printf("line %d: %s  [%s]\n", __LINE__, #cond, grl_last_error()); }   \
  } while (0)

static const int OD = 24, A = 4, B = 8, NA = 3, CAP = 32, W = 16;

struct Block {      // exactly `bytes` bytes on the heap, zeroed
  size_t bytes;
  std::unique_ptr<char[]> p;
  explicit Block(size_t n) : bytes(n), p(new char[n]()) {}
  void* get() { return p.get(); }
};

struct Handle {
  std::vector<Block> arenas;
  grl_handle h = nullptr;
  void create(const grl_config& c, const grl_ppo_config* p = nullptr, const grl_trpo_config* t = nullptr) {
    grl_sizes s;
    CHECK((p ? grl_ppo_query_sizes(&c, p, &s) : t ? grl_trpo_query_sizes(&c, t, &s) : grl_query_sizes(&c, &s)) == GRL_OK);
    for (size_t b : {s.state_bytes, s.grads_bytes, s.work_bytes, s.replay_bytes}) arenas.emplace_back(b);
    float* P = (float*)arenas[0].get();      // the parameter block opens the state arena: small values that are not zero
    unsigned r = 12345u;
    for (int64_t i = 0; i < s.n_params; ++i) { r = r * 1664525u + 1013904223u; P[i] = ((float)(r >> 8) / 16777216.f - 0.5f) * 0.2f; }
    grl_buffers bufs = {arenas[0].get(), arenas[1].get(), arenas[2].get(), arenas[3].get()};
    CHECK((p ? grl_ppo_create(&c, p, &bufs, &h) : t ? grl_trpo_create(&c, t, &bufs, &h) : grl_create(&c, &bufs, &h)) == GRL_OK);
  }
  void destroy() { CHECK(grl_destroy(h) == GRL_OK); h = nullptr; }
  bool same_arena(int k, Handle& o) { return arenas[k].bytes == o.arenas[k].bytes && memcmp(arenas[k].get(), o.arenas[k].get(), arenas[k].bytes) == 0; }
};

static bool last_error_has(const char* text) { return strstr(grl_last_error(), text) != nullptr; }
static std::vector<float> ramp(size_t n, int mod, float scale, float shift) {
  std::vector<float> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = scale * (float)((i * 7 + 3) % (size_t)mod) + shift;
  return v;
}

static grl_config base_config(int algo, int obs_dim, int act_dim) {
  grl_config c;
  memset(&c, 0, sizeof(c));
  c.algo = algo; c.extractor = GRL_EXTRACTOR_MLP; c.img_hw = 64; c.obs_channels = 2; c.n_direct = 1; c.obs_dim = obs_dim; c.act_dim = act_dim;
  c.n_layers = 2; c.layers[0] = c.layers[1] = W;
  c.batch_size = B; c.act_batch = NA; c.replay_capacity = CAP;
  c.gamma = 0.99f; c.lr = 3e-4f;
  return c;
}
static grl_config sac_config() {
  grl_config c = base_config(GRL_ALGO_SAC, OD, A);
  c.normalize = 1; c.tau = 0.005f; c.clip_obs = c.clip_reward = 10.f; c.norm_eps = 1e-8f; c.target_entropy = -(float)A;
  return c;
}
static grl_config q_config(int algo, int layer_norm) {
  const int D = algo == GRL_ALGO_DQN ? 1 : A;
  grl_config c = base_config(algo, OD, D);
  c.n_layers = 1; c.layers[0] = 1; c.layers[1] = 0;
  c.normalize = 1; c.clip_obs = c.clip_reward = 10.f; c.norm_eps = 1e-8f;
  c.q_branches = D; c.q_bins = 3;
  if (algo == GRL_ALGO_BDQ) { c.q_n_common = 2; c.q_common[0] = c.q_common[1] = W; }
  c.q_n_branch = 1; c.q_branch[0] = W; c.q_n_value = 1; c.q_value[0] = W;
  c.q_huber = algo == GRL_ALGO_DQN; c.q_double = 1; c.q_grad_clip = 10.f;
  c.q_trunk_scale = algo == GRL_ALGO_BDQ ? 1.f / (float)(D + 1) : 1.f;
  c.q_layer_norm = layer_norm;
  return c;
}

// ---------------------------------------------------------------------------------------------------- every kind: create, destroy
static void every_kind() {
  {
    Handle h; h.create(sac_config()); h.destroy();
  }
  {      // SAC CnnPolicy at the smallest supported image side
    grl_config c = sac_config();
    c.extractor = GRL_EXTRACTOR_AUGMENTED; c.img_hw = 36; c.obs_dim = 0;
    Handle h; h.create(c); h.destroy();
  }
  for (int algo : {GRL_ALGO_DQN, GRL_ALGO_BDQ}) {
    Handle h; h.create(q_config(algo, 0)); h.destroy();
  }
  {
    Handle h; h.create(q_config(GRL_ALGO_DQN, 1)); h.destroy();
  }
  {      // auto-encoder (the shipped network)
    grl_config c = base_config(GRL_ALGO_AE, 4096, 1);
    c.n_layers = 1; c.layers[0] = 1; c.layers[1] = 0; c.replay_capacity = 1; c.lr = 2e-4f;
    Handle h; h.create(c); h.destroy();
  }
  {      // TRPO
    grl_config c = base_config(GRL_ALGO_TRPO, OD, A);
    c.act_batch = 1;
    grl_trpo_config t;
    memset(&t, 0, sizeof(t));
    t.n_steps = CAP; t.n_vf_layers = 2; t.vf_layers[0] = t.vf_layers[1] = W;
    t.cg_iters = 10; t.ls_steps = 10; t.fvp_stride = 5; t.vf_batch = B;
    t.lam = 0.98f; t.max_kl = 0.01f; t.cg_damping = 1e-2f; t.adam_eps = 1e-8f;
    Handle h; h.create(c, nullptr, &t); h.destroy();
  }
}

// ---------------------------------------------------------------------------------------------------- PPO2, normalize = 2
static void ppo_checks() {
  const int T = 8;
  grl_config c = base_config(GRL_ALGO_PPO, OD, A);
  c.replay_capacity = NA * T; c.normalize = 2; c.clip_obs = 10.f; c.norm_eps = 1e-8f;
  grl_ppo_config p;
  memset(&p, 0, sizeof(p));
  p.n_envs = NA; p.n_steps = T; p.n_vf_layers = 2; p.vf_layers[0] = p.vf_layers[1] = W;
  p.lam = 0.95f; p.clip_range = 0.2f; p.clip_range_vf = 0.2f; p.ent_coef = 0.01f; p.vf_coef = 0.5f; p.max_grad_norm = 0.5f; p.adam_eps = 1e-5f;
  p.norm_eps64 = 1e-8;
  Handle h;
  h.create(c, &p);
  std::vector<float> obs = ramp((size_t)NA * OD, 11, 0.1f, -0.5f), eps = ramp((size_t)NA * A, 5, 0.3f, -0.6f), done(NA, 0.f), rew(NA, 0.25f);
  std::vector<float> act((size_t)NA * A), val(NA), nlp(NA), a1((size_t)NA * A), a2((size_t)NA * A);
  for (int t = 0; t < 2; ++t) {      // observe once, step on the observed rows
    CHECK(grl_observe(h.h, obs.data(), NA, GRL_OBSERVE_UPDATE_STATS) == GRL_OK);
    CHECK(grl_ppo_step(h.h, nullptr, done.data(), eps.data(), act.data(), val.data(), nlp.data()) == GRL_OK);
    CHECK(std::isfinite(act[0]) && std::isfinite(val[NA - 1]) && std::isfinite(nlp[NA - 1]));
    CHECK(grl_ppo_rewards(h.h, rew.data(), NA) == GRL_OK);
  }
  CHECK(grl_act(h.h, obs.data(), 1, GRL_ACT_DETERMINISTIC, nullptr, a1.data()) == GRL_OK);
  CHECK(grl_act(h.h, obs.data(), NA, GRL_ACT_DETERMINISTIC, nullptr, a2.data()) == GRL_OK);
  CHECK(memcmp(a1.data(), a2.data(), (size_t)A * 4) == 0);
  h.destroy();
}

// ---------------------------------------------------------------------------------------------------- SAC: the two rings, act, exchange
static void set_stats(Handle& h, int k) {
  std::vector<double> mean(OD), var(OD);
  for (int j = 0; j < OD; ++j) { mean[j] = 0.01 * (j + 1) * (k + 1); var[j] = 0.5 + 0.125 * ((j + k) % 5); }
  CHECK(grl_set_obs_stats(h.h, mean.data(), var.data(), 1.0 + 0.5 * k) == GRL_OK);
}

// five env steps of grl_observe + grl_replay_add_observed (terminal rows in steps 1 and 3); `refuse`: step 2 is first tried with a
// terminal row out of range
static void env_steps(Handle& h, bool refuse) {
  std::vector<float> term = ramp((size_t)2 * OD, 13, 0.05f, 0.1f);
  CHECK(grl_observe(h.h, ramp((size_t)NA * OD, 17, 0.1f, -0.8f).data(), NA, 0) == GRL_OK);
  for (int s = 0; s < 5; ++s) {
    std::vector<float> obs = ramp((size_t)NA * OD, 11 + s, 0.1f, -0.5f), act = ramp((size_t)NA * A, 5 + s, 0.2f, -0.4f), rew = ramp(NA, 3 + s, 0.5f, 0.f);
    std::vector<float> done(NA, 0.f);
    const int32_t rows[2] = {2, 0};
    const int n_term = (s == 1 || s == 3) ? (s == 1 ? 1 : 2) : 0;
    for (int j = 0; j < n_term; ++j) done[rows[j]] = 1.f;
    CHECK(grl_observe(h.h, obs.data(), NA, 0) == GRL_OK);
    if (refuse && s == 2) {
      const int64_t size = grl_replay_size(h.h);
      const int32_t bad[2] = {1, NA};
      CHECK(grl_replay_add_observed(h.h, act.data(), rew.data(), done.data(), NA, bad, term.data(), 2) == GRL_ERR_INVALID && last_error_has("terminal row out of range"));
      CHECK(grl_replay_size(h.h) == size);
    }
    CHECK(grl_replay_add_observed(h.h, act.data(), rew.data(), done.data(), NA, n_term ? rows : nullptr, n_term ? term.data() : nullptr, n_term) == GRL_OK);
    CHECK(grl_replay_size(h.h) == (int64_t)NA * (s + 1));
  }
}

static void sac_checks() {
  const grl_config c = sac_config();
  Handle a, b;
  a.create(c);
  b.create(c);
  {      // statistics ring: five sets back to back (the ring wraps twice) against the last set alone.  A set may change the 2 OD + 1
         // statistic words and nothing else of the state arena: the mirror's alignment gaps travel with the span and must be zero
    Block before(a.arenas[0].bytes);
    memcpy(before.get(), a.arenas[0].get(), before.bytes);
    for (int k = 0; k < 5; ++k) set_stats(a, k);
    set_stats(b, 4);
    CHECK(a.same_arena(0, b));
    size_t changed = 0;
    for (size_t i = 0; i + 8 <= before.bytes; i += 8) changed += memcmp((char*)before.get() + i, (char*)a.arenas[0].get() + i, 8) != 0;
    CHECK(changed >= 1 && changed <= (size_t)2 * OD + 1);
  }
  {      // observe ring: the refused step leaves the ring, the replay and the following steps as they are without it
    env_steps(a, true);
    env_steps(b, false);
    CHECK(a.same_arena(3, b));
    CHECK(a.same_arena(0, b));
  }
  {      // staging growth: n = 1, act_batch, 1
    std::vector<float> obs = ramp((size_t)NA * OD, 19, 0.1f, -0.9f), o1(A), o2((size_t)NA * A), o3(A), eps = ramp((size_t)NA * A, 7, 0.25f, -0.75f);
    CHECK(grl_act(a.h, obs.data(), 1, GRL_ACT_DETERMINISTIC, nullptr, o1.data()) == GRL_OK);
    CHECK(grl_act(a.h, obs.data(), NA, GRL_ACT_DETERMINISTIC, nullptr, o2.data()) == GRL_OK);
    CHECK(grl_act(a.h, obs.data(), 1, GRL_ACT_DETERMINISTIC, nullptr, o3.data()) == GRL_OK);
    CHECK(o1 == o3 && memcmp(o1.data(), o2.data(), (size_t)A * 4) == 0 && std::isfinite(o1[0]));
    CHECK(grl_act(a.h, obs.data(), NA, GRL_ACT_RAW_OBS, eps.data(), o2.data()) == GRL_OK);
    CHECK(grl_act(a.h, nullptr, NA, GRL_ACT_OBSERVED | GRL_ACT_RAW_OBS | GRL_ACT_DETERMINISTIC, nullptr, o2.data()) == GRL_OK);
  }
  {      // data parallel, one rank: init, connect, an update, disconnect; again, a refused second init, destroyed while connected
    char handles[GRL_ALLREDUCE_HANDLE_BYTES];
    CHECK(grl_allreduce_init(a.h, 0, 1, handles) == GRL_OK);
    CHECK(grl_allreduce_connect(a.h, handles) == GRL_OK);
    CHECK(grl_train_step_allreduce(a.h, 1, nullptr, nullptr) == GRL_OK);
    grl_metrics m;
    CHECK(grl_get_metrics(a.h, &m) == GRL_OK && std::isfinite(m.policy_loss));
    CHECK(grl_allreduce_disconnect(a.h) == GRL_OK);
    CHECK(grl_allreduce_disconnect(a.h) == GRL_OK);      // (nothing left to release)
    CHECK(grl_allreduce_init(a.h, 0, 1, handles) == GRL_OK);
    CHECK(grl_allreduce_init(a.h, 0, 1, handles) == GRL_ERR_STATE && last_error_has("grl_allreduce_init was already called on this handle"));
    CHECK(grl_allreduce_connect(a.h, handles) == GRL_OK);
    CHECK(grl_train_step_allreduce(a.h, 2, nullptr, nullptr) == GRL_OK);
    a.destroy();
  }
  {      // behaviour-cloning session: its launches move out of the handle's list at begin and die with the record; the handle is
         // destroyed with the session open (the buffer outlives the handle)
    std::vector<float> low(A, -1.f), high(A, 1.f), obs = ramp((size_t)CAP * OD, 97, 0.01f, -0.4f), act = ramp((size_t)CAP * A, 83, 0.02f, -0.8f);
    std::vector<int32_t> idx = {3, 17, 31, 0, 8, 21, -1, -1};
    grl_bc_config bc = {B, 1e-4f, 1e-8f, low.data(), high.data()};
    size_t bytes = 0;
    float loss[2];
    CHECK(grl_bc_query_sizes(b.h, &bc, &bytes) == GRL_OK && bytes > 0);
    Block first(bytes), second(bytes);
    CHECK(grl_bc_begin(b.h, &bc, first.get()) == GRL_OK);
    CHECK(grl_bc_train(b.h, obs.data(), act.data(), CAP, idx.data(), 1) == GRL_OK);
    CHECK(grl_bc_end(b.h) == GRL_OK);
    CHECK(grl_train_step(b.h, 1, nullptr, nullptr) == GRL_OK);      // the handle's own launches are where they were
    CHECK(grl_bc_begin(b.h, &bc, second.get()) == GRL_OK);
    CHECK(grl_bc_train(b.h, obs.data(), act.data(), CAP, idx.data(), 1) == GRL_OK);
    CHECK(grl_bc_get_losses(b.h, loss, 2) == 1 && std::isfinite(loss[0]));
    b.destroy();
  }
}

// ---------------------------------------------------------------------------------------------------- DQN / BDQ: the act forms
// layer_norm = 1: the launch-list greedy route, which stages the observations through pin_in
static void q_checks(int algo, int layer_norm) {
  const grl_config c = q_config(algo, layer_norm);
  const int D = c.q_branches, nq = D * c.q_bins;
  Handle h;
  h.create(c);
  std::vector<float> obs = ramp((size_t)NA * OD, 23, 0.1f, -1.0f), q1(nq), q2((size_t)NA * nq), q3(nq), b1(D), b2((size_t)NA * D), b3(D);
  CHECK(grl_act(h.h, obs.data(), 1, 0, nullptr, q1.data()) == GRL_OK);                  // the Q-value form
  CHECK(grl_act(h.h, obs.data(), NA, 0, nullptr, q2.data()) == GRL_OK);
  CHECK(grl_act(h.h, obs.data(), 1, 0, nullptr, q3.data()) == GRL_OK);
  CHECK(q1 == q3 && memcmp(q1.data(), q2.data(), (size_t)nq * 4) == 0 && std::isfinite(q1[0]));
  CHECK(grl_act(h.h, obs.data(), 1, GRL_ACT_GREEDY, nullptr, b1.data()) == GRL_OK);
  CHECK(grl_act(h.h, obs.data(), NA, GRL_ACT_GREEDY, nullptr, b2.data()) == GRL_OK);
  CHECK(grl_act(h.h, obs.data(), 1, GRL_ACT_GREEDY, nullptr, b3.data()) == GRL_OK);
  CHECK(b1 == b3 && memcmp(b1.data(), b2.data(), (size_t)D * 4) == 0);
  for (int d = 0; d < D; ++d) {      // the greedy bin is the arg-max of the Q-values of its branch
    int best = 0;
    for (int k = 1; k < c.q_bins; ++k)
      if (q1[(size_t)d * c.q_bins + k] > q1[(size_t)d * c.q_bins + best]) best = k;
    CHECK(b1[d] == (float)best);
  }
  CHECK(grl_observe(h.h, obs.data(), NA, GRL_OBSERVE_UPDATE_STATS) == GRL_OK);
  CHECK(grl_act(h.h, nullptr, NA, GRL_ACT_GREEDY | GRL_ACT_OBSERVED | GRL_ACT_RAW_OBS, nullptr, b2.data()) == GRL_OK);
  h.destroy();
}

// ---------------------------------------------------------------------------------------------------- auto-encoder: grl_encode
static void encode_checks() {
  grl_config c = base_config(GRL_ALGO_AE, 4096, 1);
  c.n_layers = 1; c.layers[0] = 1; c.layers[1] = 0; c.replay_capacity = 1; c.lr = 2e-4f;
  Handle h;
  h.create(c);
  std::vector<float> img = ramp((size_t)NA * 4096, 251, 0.004f, 0.f), e1(100), e2((size_t)NA * 100), e3(100);
  CHECK(grl_encode(h.h, img.data(), 1, e1.data()) == GRL_OK);
  CHECK(grl_encode(h.h, img.data(), NA, e2.data()) == GRL_OK);
  CHECK(grl_encode(h.h, img.data(), 1, e3.data()) == GRL_OK);
  CHECK(e1 == e3 && memcmp(e1.data(), e2.data(), 400) == 0 && std::isfinite(e1[0]));
  h.destroy();
}

// ---------------------------------------------------------------------------------------------------- creations that are refused
static void failed_creations() {
  grl_config c = sac_config();
  Block tiny(256);
  grl_handle h = nullptr;
  grl_buffers none = {tiny.get(), tiny.get(), nullptr, tiny.get()};
  CHECK(grl_create(&c, &none, &h) == GRL_ERR_INVALID && last_error_has("null buffers") && h == nullptr);
  // refused by the plan, after the configuration check has passed and the handle exists: 128x128 images at a batch whose image
  // buffer reaches 2^31 bytes (nothing is carved, so the arenas are never touched)
  c.extractor = GRL_EXTRACTOR_AUGMENTED; c.img_hw = 128; c.obs_dim = 0; c.batch_size = 65536;
  grl_buffers bufs = {tiny.get(), tiny.get(), tiny.get(), tiny.get()};
  CHECK(grl_create(&c, &bufs, &h) == GRL_ERR_INVALID && last_error_has("fewer than 2^31 bytes per buffer") && h == nullptr);
}

int main() {
  every_kind();
  ppo_checks();
  sac_checks();
  q_checks(GRL_ALGO_DQN, 0);
  q_checks(GRL_ALGO_BDQ, 0);
  q_checks(GRL_ALGO_DQN, 1);
  encode_checks();
  failed_creations();
  printf("%d checks, %d failed\n", n_checks, n_failed);
  return n_failed ? 1 : 0;
}
