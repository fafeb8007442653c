// td3_lifetime_check.cpp -- the life of a TD3 handle through include/grl.h alone: create, train (policy and critic-only updates, the
// caller's indices and normals and device draws), metrics, act, destroy; a handle destroyed without training; a refused create; the
// entry points a TD3 handle refuses.  A STAND-ALONE program for AddressSanitizer + UBSan + the leak checker
// (tests/test_td3_lifetime_sanitized.py links it with the emulation build of the library).  Every arena is a heap block of exactly
// the queried size: a launch that reads or writes past its buffers shows as a sanitizer report.
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

struct Block {      // exactly `bytes` bytes on the heap, zeroed
  size_t bytes;
  std::unique_ptr<char[]> p;
  explicit Block(size_t n) : bytes(n), p(new char[n]()) {}
  void* get() { return p.get(); }
};

static bool last_error_has(const char* text) { return strstr(grl_last_error(), text) != nullptr; }

struct Shape { int od, A, B, NA, cap, L, w[GRL_MAX_LAYERS]; int normalize; };

static grl_config config_of(const Shape& s) {
  grl_config c;
  memset(&c, 0, sizeof(c));
  c.algo = GRL_ALGO_TD3; c.extractor = GRL_EXTRACTOR_MLP; c.obs_dim = s.od; c.act_dim = s.A;
  c.n_layers = s.L;
  for (int l = 0; l < s.L; ++l) c.layers[l] = s.w[l];
  c.batch_size = s.B; c.act_batch = s.NA; c.replay_capacity = s.cap;
  c.normalize = s.normalize; c.gamma = 0.99f; c.lr = 3e-4f; c.tau = 0.005f;
  c.clip_obs = c.clip_reward = 10.f; c.norm_eps = 1e-8f; c.seed = 7;
  return c;
}
static grl_td3_config td3_of(int delay) {
  grl_td3_config t;
  memset(&t, 0, sizeof(t));
  t.policy_delay = delay; t.target_policy_noise = 0.2f; t.target_noise_clip = 0.5f;
  return t;
}

struct Handle {
  std::vector<Block> arenas;
  grl_handle h = nullptr;
  grl_sizes s;
  void create(const grl_config& c, const grl_td3_config& t) {
    CHECK(grl_td3_query_sizes(&c, &t, &s) == GRL_OK);
    for (size_t b : {s.state_bytes, s.grads_bytes, s.work_bytes, s.replay_bytes}) arenas.emplace_back(b);
    float* P = (float*)arenas[0].get();      // the parameter block opens the state arena: small values that are not zero
    unsigned r = 12345u;
    for (int64_t i = 0; i < s.n_params; ++i) { r = r * 1664525u + 1013904223u; P[i] = ((float)(r >> 8) / 16777216.f - 0.5f) * 0.4f; }
    grl_buffers bufs = {arenas[0].get(), arenas[1].get(), arenas[2].get(), arenas[3].get()};
    CHECK(grl_td3_create(&c, &t, &bufs, &h) == GRL_OK);
  }
  void destroy() { CHECK(grl_destroy(h) == GRL_OK); h = nullptr; }
};

static std::vector<float> ramp(size_t n, int mod, float scale, float shift) {
  std::vector<float> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = scale * (float)((i * 7 + 3) % (size_t)mod) + shift;
  return v;
}

static void fill_replay(Handle& H, const Shape& s, int n) {
  std::vector<float> obs = ramp((size_t)n * s.od, 23, 0.05f, -0.5f), nxt = ramp((size_t)n * s.od, 19, 0.06f, -0.5f);
  std::vector<float> act = ramp((size_t)n * s.A, 11, 0.18f, -0.9f), rew = ramp(n, 7, 0.3f, -1.f), done(n, 0.f);
  for (int i = 0; i < n; i += 5) done[i] = 1.f;
  CHECK(grl_replay_add(H.h, obs.data(), act.data(), rew.data(), nxt.data(), done.data(), n) == GRL_OK);
  CHECK(grl_replay_size(H.h) == (n < s.cap ? n : s.cap));
}

// create, train every form of an update, metrics, act, the statistics calls, destroy
static void full_life(const Shape& s, int delay, bool longest_call) {
  Handle H;
  H.create(config_of(s), td3_of(delay));
  CHECK(grl_param_count(H.h) == 2 * 3 * (2 * s.L + 2));
  CHECK(grl_td3_train(H.h, 1, nullptr, nullptr, 0) == GRL_ERR_STATE && last_error_has("empty"));
  fill_replay(H, s, s.cap + 3);      // (the ring wraps)
  std::vector<double> mean(s.od, 0.1), var(s.od, 0.7);
  CHECK(grl_set_obs_stats(H.h, mean.data(), var.data(), 2.0) == GRL_OK);
  const int n = 5;
  std::vector<int64_t> idx((size_t)n * s.B);
  for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int64_t)((i * 13 + 5) % (size_t)s.cap);
  std::vector<float> eps = ramp((size_t)n * s.B * s.A, 29, 0.15f, -2.1f);
  float m[GRL_TD3_MAX_UPDATES * GRL_TD3_METRICS];
  CHECK(grl_td3_train(H.h, n, idx.data(), eps.data(), 0) == GRL_OK);       // the caller's rows and normals
  CHECK(grl_td3_get_metrics(H.h, m, n * GRL_TD3_METRICS) == n);
  for (int u = 0; u < n; ++u) {
    CHECK(m[u * GRL_TD3_METRICS + 5] == (u % delay == 0 ? 1.f : 0.f));
    for (int k = 0; k < GRL_TD3_METRICS; ++k) CHECK(std::isfinite(m[u * GRL_TD3_METRICS + k]));
  }
  CHECK(grl_td3_get_metrics(H.h, m, n * GRL_TD3_METRICS - 1) == GRL_ERR_INVALID);
  CHECK(grl_td3_train(H.h, 7, nullptr, nullptr, 3) == GRL_OK);             // device draws, grouped
  CHECK(grl_td3_train(H.h, 2, idx.data(), nullptr, 10) == GRL_OK);         // rows handed over, normals drawn
  CHECK(grl_td3_train(H.h, 2, nullptr, eps.data(), 12) == GRL_OK);         // rows drawn, normals handed over
  CHECK(grl_td3_get_metrics(H.h, m, 2 * GRL_TD3_METRICS) == 2);
  CHECK(grl_profile_enable(H.h, 1) == GRL_OK);
  CHECK(grl_td3_train(H.h, 2, nullptr, nullptr, 0) == GRL_OK);
  CHECK(grl_profile_enable(H.h, 0) == GRL_OK);
  CHECK(grl_set_learning_rate(H.h, 1e-4f) == GRL_OK);
  CHECK(grl_reset_optimizer(H.h) == GRL_OK);
  if (longest_call) {      // the metrics block to its last row
    CHECK(grl_td3_train(H.h, GRL_TD3_MAX_UPDATES, nullptr, nullptr, 1) == GRL_OK);
    CHECK(grl_td3_get_metrics(H.h, m, GRL_TD3_MAX_UPDATES * GRL_TD3_METRICS) == GRL_TD3_MAX_UPDATES);
  }
  CHECK(grl_td3_train(H.h, GRL_TD3_MAX_UPDATES + 1, nullptr, nullptr, 0) == GRL_ERR_INVALID);
  // act: every row count up to act_batch, normalised and raw observations
  std::vector<float> obs = ramp((size_t)s.NA * s.od, 17, 0.07f, -0.5f), out((size_t)s.NA * s.A, 9.f);
  for (int k = 1; k <= s.NA; ++k) {
    CHECK(grl_act(H.h, obs.data(), k, GRL_ACT_DETERMINISTIC, nullptr, out.data()) == GRL_OK);
    CHECK(grl_act(H.h, obs.data(), k, GRL_ACT_RAW_OBS, nullptr, out.data()) == GRL_OK);
    for (int i = 0; i < k * s.A; ++i) CHECK(std::fabs(out[i]) <= 1.f);
  }
  CHECK(grl_act(H.h, obs.data(), s.NA + 1, GRL_ACT_DETERMINISTIC, nullptr, out.data()) == GRL_ERR_INVALID);
  CHECK(grl_act(H.h, nullptr, 1, GRL_ACT_OBSERVED, nullptr, out.data()) == GRL_ERR_STATE);
  CHECK(grl_act(H.h, obs.data(), 1, GRL_ACT_GREEDY, nullptr, out.data()) == GRL_ERR_STATE);
  // what a TD3 handle refuses, before anything moves
  CHECK(grl_train_step(H.h, 1, nullptr, nullptr) == GRL_ERR_STATE && last_error_has("TD3 handle"));
  CHECK(grl_compute_grads(H.h, nullptr, nullptr) == GRL_ERR_STATE);
  CHECK(grl_apply_grads(H.h, 1.f) == GRL_ERR_STATE);
  CHECK(grl_observe(H.h, obs.data(), 1, 0) == GRL_ERR_STATE);
  size_t bytes = 0;
  CHECK(grl_state_size(H.h, &bytes) == GRL_ERR_STATE);
  char handles[GRL_ALLREDUCE_HANDLE_BYTES];
  CHECK(grl_allreduce_init(H.h, 0, 1, handles) == GRL_ERR_STATE);
  grl_bc_config bc;
  memset(&bc, 0, sizeof(bc));
  CHECK(grl_bc_query_sizes(H.h, &bc, &bytes) == GRL_ERR_STATE);
  H.destroy();
}

int main() {
  const Shape shapes[] = {
      {20, 5, 8, 3, 32, 2, {16, 16, 0, 0}, 1},      // 16-byte gather rows, one-launch act, normalised
      {13, 3, 7, 2, 19, 3, {24, 17, 9, 0}, 0},      // nothing a multiple of 4
      {11, 1, 33, 1, 40, 1, {8, 0, 0, 0}, 3},       // one layer, one action component
      {30, 4, 16, 2, 24, 2, {300, 20, 0, 0}, 2},    // a width beyond 256: the act path's launch list
      {6, 2, 300, 4, 310, 2, {16, 16, 0, 0}, 0},    // two loss blocks
  };
  int k = 0;
  for (const Shape& s : shapes) { full_life(s, 1 + k % 3, k == 1); ++k; }      // (the longest call at the smallest shape)
  {      // destroyed without training
    Handle H;
    H.create(config_of(shapes[0]), td3_of(2));
    H.destroy();
  }
  {      // ... and with a filled ring and nothing else
    Handle H;
    H.create(config_of(shapes[1]), td3_of(2));
    fill_replay(H, shapes[1], 5);
    H.destroy();
  }
  {      // refused creations: nothing is left behind
    grl_sizes s;
    grl_handle h = nullptr;
    grl_config c = config_of(shapes[0]);
    grl_td3_config t = td3_of(0);
    CHECK(grl_td3_query_sizes(&c, &t, &s) == GRL_ERR_INVALID && last_error_has("policy_delay"));
    t = td3_of(2);
    t.target_noise_clip = -1.f;
    CHECK(grl_td3_query_sizes(&c, &t, &s) == GRL_ERR_INVALID && last_error_has("target_noise_clip"));
    t = td3_of(2);
    c.extractor = GRL_EXTRACTOR_NATURE;
    CHECK(grl_td3_query_sizes(&c, &t, &s) == GRL_ERR_INVALID && last_error_has("extractor"));
    c = config_of(shapes[0]);
    CHECK(grl_td3_query_sizes(&c, &t, &s) == GRL_OK);
    Block st(s.state_bytes), gr(s.grads_bytes), wk(s.work_bytes), rp(s.replay_bytes);
    grl_buffers bufs = {st.get(), gr.get(), wk.get(), nullptr};
    CHECK(grl_td3_create(&c, &t, &bufs, &h) == GRL_ERR_INVALID && h == nullptr);
    bufs.replay = rp.get();
    c.act_dim = 65;
    CHECK(grl_td3_create(&c, &t, &bufs, &h) == GRL_ERR_INVALID && h == nullptr);
    c = config_of(shapes[0]);
    CHECK(grl_create(&c, &bufs, &h) == GRL_ERR_INVALID && last_error_has("grl_td3_create") && h == nullptr);
    CHECK(grl_td3_create(&c, nullptr, &bufs, &h) == GRL_ERR_INVALID && h == nullptr);
  }
  printf("%d checks, %d failed\n", n_checks, n_failed);
  return n_failed ? 1 : 0;
}
