// session_lifetime_check.cpp -- the lifetime of a behaviour-cloning session (SAC handle) and of a GAIL session (TRPO handle)
// through include/grl.h alone, as a STAND-ALONE program for AddressSanitizer + UBSan (tests/test_session_lifetime_sanitized.py
// links it with the emulation build of the library).  Every arena and every session buffer is a heap block of exactly the
// queried size, so a plan that carves past its dry run, a record freed twice or a launch left behind shows as a sanitizer
// report.  Prints "<n> checks, 0 failed".
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
  std::unique_ptr<char[]> p;
  explicit Block(size_t bytes) : p(new char[bytes]()) {}
  void* get() { return p.get(); }
};

struct Handle {
  std::vector<Block> arenas;
  grl_handle h = nullptr;
  void create(const grl_config& c, const grl_trpo_config* t) {
    grl_sizes s;
    CHECK((t ? grl_trpo_query_sizes(&c, t, &s) : grl_query_sizes(&c, &s)) == GRL_OK);
    for (size_t b : {s.state_bytes, s.grads_bytes, s.work_bytes, s.replay_bytes}) arenas.emplace_back(b);
    float* P = (float*)arenas[0].get();      // the parameter block opens the state arena: small values that are not zero
    unsigned r = 12345u;
    for (int64_t i = 0; i < s.n_params; ++i) { r = r * 1664525u + 1013904223u; P[i] = ((float)(r >> 8) / 16777216.f - 0.5f) * 0.2f; }
    grl_buffers bufs = {arenas[0].get(), arenas[1].get(), arenas[2].get(), arenas[3].get()};
    CHECK((t ? grl_trpo_create(&c, t, &bufs, &h) : grl_create(&c, &bufs, &h)) == GRL_OK);
  }
};

static bool last_error_has(const char* text) { return strstr(grl_last_error(), text) != nullptr; }

static grl_config base_config(int obs_dim, int act_dim, int batch, int capacity) {
  grl_config c;
  memset(&c, 0, sizeof(c));
  c.extractor = GRL_EXTRACTOR_MLP; c.img_hw = 64; c.obs_channels = 2; c.n_direct = 1; c.obs_dim = obs_dim; c.act_dim = act_dim;
  c.n_layers = 2; c.layers[0] = c.layers[1] = 16;
  c.batch_size = batch; c.act_batch = 1; c.replay_capacity = capacity;
  c.gamma = 0.99f; c.lr = 3e-4f;
  return c;
}

// ---------------------------------------------------------------------------------------------------- behaviour cloning
static void bc_checks() {
  const int OD = 24, A = 4, B = 8, ROWS = 40;
  grl_config c = base_config(OD, A, B, 32);
  c.algo = GRL_ALGO_SAC; c.tau = 0.005f; c.clip_obs = c.clip_reward = 10.f; c.norm_eps = 1e-8f; c.target_entropy = -(float)A;
  std::vector<float> low(A, -1.f), high(A, 1.f), obs((size_t)ROWS * OD), act((size_t)ROWS * A);
  for (size_t i = 0; i < obs.size(); ++i) obs[i] = 0.01f * (float)(i % 97) - 0.4f;
  for (size_t i = 0; i < act.size(); ++i) act[i] = 0.02f * (float)(i % 83) - 0.8f;
  std::vector<int32_t> idx = {3, 17, 39, 0, 8, 21, -1, -1};
  grl_bc_config bc = {B, 1e-4f, 1e-8f, low.data(), high.data()};
  float loss[4];

  Handle a;
  a.create(c, nullptr);
  size_t bytes = 0;
  CHECK(grl_bc_query_sizes(a.h, &bc, &bytes) == GRL_OK && bytes > 0);
  {      // query, begin, one call, losses, end
    Block buf(bytes);
    CHECK(grl_bc_begin(a.h, &bc, buf.get()) == GRL_OK);
    CHECK(grl_bc_train(a.h, obs.data(), act.data(), ROWS, idx.data(), 1) == GRL_OK);
    CHECK(grl_bc_get_losses(a.h, loss, 4) == 1 && std::isfinite(loss[0]) && loss[0] > 0.f);
    CHECK(grl_bc_end(a.h) == GRL_OK);
  }
  {      // begin twice: the second is refused, the first stays usable
    Block buf(bytes), other(bytes);
    CHECK(grl_bc_begin(a.h, &bc, buf.get()) == GRL_OK);
    CHECK(grl_bc_begin(a.h, &bc, other.get()) == GRL_ERR_STATE && last_error_has("a behaviour-cloning session is open on this handle"));
    CHECK(grl_bc_eval(a.h, obs.data(), act.data(), ROWS, idx.data(), 1) == GRL_OK);
    CHECK(grl_bc_get_losses(a.h, loss, 4) == 1 && std::isfinite(loss[0]));
    CHECK(grl_bc_end(a.h) == GRL_OK);
  }
  {      // a bad bound is refused and leaves no session
    Block buf(bytes);
    std::vector<float> bad = high;
    bad[2] = low[2];
    grl_bc_config bcb = {B, 1e-4f, 1e-8f, low.data(), bad.data()};
    CHECK(grl_bc_begin(a.h, &bcb, buf.get()) == GRL_ERR_INVALID && last_error_has("bc: the action bounds must be finite with high > low (dimension 2)"));
    CHECK(grl_bc_end(a.h) == GRL_ERR_STATE && last_error_has("grl_bc_end needs an open session"));
  }
  {      // the handle is destroyed with a session open (the buffer outlives the handle)
    Block buf(bytes);
    CHECK(grl_bc_begin(a.h, &bc, buf.get()) == GRL_OK);
    CHECK(grl_bc_train(a.h, obs.data(), act.data(), ROWS, idx.data(), 1) == GRL_OK);
    CHECK(grl_destroy(a.h) == GRL_OK);
  }
}

// ---------------------------------------------------------------------------------------------------- GAIL
static void fill_rollout(grl_handle h, int T, int OD, int A) {
  std::vector<float> obs(OD), eps(A), out_act(A);
  for (int t = 0; t < T; ++t) {
    for (int j = 0; j < OD; ++j) obs[j] = 0.1f * (float)((t * 7 + j * 3) % 11) - 0.5f;
    for (int j = 0; j < A; ++j) eps[j] = 0.3f * (float)((t + j) % 5) - 0.6f;
    const float done = t == 0 ? 1.f : 0.f, rew = 0.05f * (float)t;
    float val, nlp;
    CHECK(grl_ppo_step(h, obs.data(), &done, eps.data(), out_act.data(), &val, &nlp) == GRL_OK);
    CHECK(grl_ppo_rewards(h, &rew, 1) == GRL_OK);
  }
}

static void gail_checks() {
  const int OD = 5, A = 2, T = 16, ROWS = 12, B = 4;
  grl_config c = base_config(OD, A, 128, T);
  c.algo = GRL_ALGO_TRPO;
  grl_trpo_config t;
  memset(&t, 0, sizeof(t));
  t.n_steps = T; t.n_vf_layers = 2; t.vf_layers[0] = t.vf_layers[1] = 16;
  t.cg_iters = 10; t.ls_steps = 10; t.fvp_stride = 5; t.vf_batch = 128;
  t.lam = 0.98f; t.max_kl = 0.01f; t.cg_damping = 1e-2f; t.adam_eps = 1e-8f;
  std::vector<float> low(A, -1.f), high(A, 1.f), obs((size_t)ROWS * OD), act((size_t)ROWS * A), last_obs(OD, 0.2f);
  for (size_t i = 0; i < obs.size(); ++i) obs[i] = 0.03f * (float)(i % 31) - 0.4f;
  for (size_t i = 0; i < act.size(); ++i) act[i] = 0.04f * (float)(i % 41) - 0.8f;
  std::vector<int32_t> gen = {0, 15, 7, 3}, exp = {11, 0, 5, -1};
  grl_gail_config g = {8, B, 1e-3f, 3e-4f, 1e-8f, low.data(), high.data()};
  const float last_done = 0.f;
  float losses[12];

  Handle a;
  a.create(c, &t);
  size_t bytes = 0;
  CHECK(grl_gail_query_sizes(a.h, &g, &bytes) == GRL_OK && bytes > 0);
  {      // query, begin, statistics, rewards on a full rollout, one update, losses, end
    Block buf(bytes);
    fill_rollout(a.h, T, OD, A);
    CHECK(grl_gail_begin(a.h, &g, buf.get()) == GRL_OK);
    std::vector<double> sum(OD, 1.5), sumsq(OD, 9.0), s2(OD), q2(OD);
    double count = 0.0;
    CHECK(grl_gail_set_stats(a.h, sum.data(), sumsq.data(), 6.0) == GRL_OK);
    CHECK(grl_gail_get_stats(a.h, s2.data(), q2.data(), &count) == GRL_OK && count == 6.0 && s2 == sum && q2 == sumsq);
    CHECK(grl_gail_rewards(a.h) == GRL_OK);
    CHECK(grl_ppo_finish(a.h, last_obs.data(), &last_done) == GRL_OK);
    CHECK(grl_gail_update(a.h, obs.data(), act.data(), ROWS, gen.data(), exp.data(), 1) == GRL_OK);
    CHECK(grl_gail_get_losses(a.h, losses, 12) == 1 && std::isfinite(losses[0]) && std::isfinite(losses[1]));
    CHECK(grl_gail_end(a.h) == GRL_OK);
  }
  {      // begin twice: the second is refused, the first stays usable (the finished rollout is still held)
    Block buf(bytes), other(bytes);
    CHECK(grl_gail_begin(a.h, &g, buf.get()) == GRL_OK);
    CHECK(grl_gail_begin(a.h, &g, other.get()) == GRL_ERR_STATE && last_error_has("a GAIL session is open on this handle"));
    CHECK(grl_gail_update(a.h, obs.data(), act.data(), ROWS, gen.data(), exp.data(), 1) == GRL_OK);
    CHECK(grl_gail_get_losses(a.h, losses, 12) == 1);
    CHECK(grl_gail_end(a.h) == GRL_OK);
  }
  {      // a bad bound is refused and leaves no session
    Block buf(bytes);
    std::vector<float> bad = high;
    bad[1] = INFINITY;
    grl_gail_config gb = {8, B, 1e-3f, 3e-4f, 1e-8f, low.data(), bad.data()};
    CHECK(grl_gail_begin(a.h, &gb, buf.get()) == GRL_ERR_INVALID && last_error_has("gail: the action bounds must be finite with high > low (dimension 1)"));
    CHECK(grl_gail_end(a.h) == GRL_ERR_STATE && last_error_has("grl_gail_end needs an open session"));
  }
  {      // the handle is destroyed with a session open
    Block buf(bytes);
    CHECK(grl_gail_begin(a.h, &g, buf.get()) == GRL_OK);
    CHECK(grl_gail_update(a.h, obs.data(), act.data(), ROWS, gen.data(), exp.data(), 1) == GRL_OK);
    CHECK(grl_destroy(a.h) == GRL_OK);
  }
}

int main() {
  bc_checks();
  gail_checks();
  printf("%d checks, %d failed\n", n_checks, n_failed);
  return n_failed ? 1 : 0;
}
