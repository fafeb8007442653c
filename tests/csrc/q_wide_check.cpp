// q_wide_check.cpp -- stand-alone check of the tile-table builder and the host forms of the two kernels of
// csrc/q_wide_kernels.h (tests/hostemu/q_wide_ref1.h) on ragged variables: 1, 255, 4097, 131 073 and 524 288 + 3 floats, each
// 16-byte aligned in the bucket as grl_ctx::add_var lays them out.  Built by tests/test_q_wide_sanitized.py with
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DGRL_HOSTEMU -I tests/hostemu
// Gradient bucket, parameters and moments are heap blocks that end with the last variable's last float and the partials array
// has one float per tile, so an access past either is a sanitizer report; the padding between variables carries a sentinel
// that must survive; the values are compared with a double-precision evaluation of clip_by_norm + TF-Adam.
#include <cmath>
#include <cstdio>
#include <vector>

#define GRL_ELEM_TYPES_ONLY
#include "../../deep-rl-grasping_amd/csrc/q_wide_kernels.h"

using namespace grl;

static unsigned g_state = 2463534242u;
static float rnd() {      // uniform in [-1, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) / 8388608.0f - 1.0f;
}

static int check(float gscale, float clip, float grad_scale) {
  const int64_t sizes[5] = {1, 255, 4097, 131073, 524288 + 3};
  std::vector<VarSeg> segs;
  int64_t off = 0;
  for (int v = 0; v < 5; ++v) {
    segs.push_back(VarSeg{off, sizes[v]});
    off += (sizes[v] + 3) / 4 * 4;
  }
  const int64_t total = segs[4].off + segs[4].n;      // no padding behind the last variable
  const std::vector<QwTile> tiles = qw_build_tiles(segs.data(), 5);
  int bad = 0;
  // ---- the table: every float of every variable in exactly one tile, no tile across two variables, one tile per small variable
  std::vector<int> cover((size_t)total, 0);
  for (size_t k = 0; k < tiles.size(); ++k) {
    const QwTile& t = tiles[k];
    const VarSeg& s = segs[t.var];
    if (t.n < 1 || t.n > QW_TILE || t.off < s.off || t.off + t.n > s.off + s.n || (t.off - s.off) % QW_TILE) ++bad;
    if ((int)k < t.p0 || (int)k >= t.p0 + t.np || t.np != (s.n + QW_TILE - 1) / QW_TILE) ++bad;
    if (tiles[t.p0].var != t.var || tiles[t.p0 + t.np - 1].var != t.var) ++bad;
    for (int i = 0; i < t.n; ++i) cover[(size_t)(t.off + i)] += 1;
  }
  for (int v = 0; v < 5; ++v) {
    for (int64_t i = 0; i < segs[v].n; ++i) if (cover[(size_t)(segs[v].off + i)] != 1) ++bad;
    for (int64_t i = segs[v].off + segs[v].n; i < (v < 4 ? segs[v + 1].off : total); ++i) if (cover[(size_t)i] != 0) ++bad;
  }
  if (tiles.size() != 1 + 1 + 2 + 33 + 129) ++bad;
  // ---- the kernels
  const float SENT = -12345.f;
  std::vector<float> g((size_t)total, SENT), p((size_t)total, SENT), m((size_t)total, SENT), vv((size_t)total, SENT);
  for (int v = 0; v < 5; ++v)
    for (int64_t i = 0; i < segs[v].n; ++i) {
      const size_t e = (size_t)(segs[v].off + i);
      g[e] = gscale * rnd(); p[e] = rnd(); m[e] = 0.01f * rnd(); vv[e] = 0.001f * (1.f + rnd());
    }
  const std::vector<float> g0 = g, p0 = p, m0 = m, v0 = vv;
  std::vector<float> partials(tiles.size(), SENT);
  DevScalars sc;
  memset(&sc, 0, sizeof(sc));
  sc.adam_alpha = 3e-4f;
  AdamArgs a;
  memset(&a, 0, sizeof(a));
  a.params = p.data(); a.grads = g.data(); a.m = m.data(); a.v = vv.data(); a.n_train = total; a.sc = &sc;
  a.grad_scale = grad_scale; a.eps = 1e-8f;
  hipLaunchKernelGGL(q_sumsq_kernel, dim3((unsigned)tiles.size()), dim3(256), 0, nullptr, (const float*)g.data(), tiles.data(), partials.data());
  hipLaunchKernelGGL(q_clip_adam_kernel, dim3((unsigned)tiles.size()), dim3(256), 0, nullptr, g.data(), tiles.data(),
                     (const float*)partials.data(), clip, a);
  int n_clipped = 0;
  for (int v = 0; v < 5; ++v) {
    double ss = 0;
    for (int64_t i = 0; i < segs[v].n; ++i) ss += (double)g0[(size_t)(segs[v].off + i)] * g0[(size_t)(segs[v].off + i)];
    const double scale = clip / std::max(sqrt(ss), (double)clip);
    n_clipped += scale < 1.0;
    for (int64_t i = 0; i < segs[v].n; ++i) {
      const size_t e = (size_t)(segs[v].off + i);
      const double gc = g0[e] * scale, gs = gc * grad_scale;
      const double mm = m0[e] + (gs - m0[e]) * 0.1, v2 = v0[e] + (gs * gs - v0[e]) * 0.001;
      const double pp = p0[e] - mm * 3e-4 / (sqrt(v2) + 1e-8);
      if (fabs(g[e] - gc) > 2e-4 * fabs(gc) + 1e-12) ++bad;
      // (the clip scale comes from a float32 sum of squares: up to ~1.3e-4 relative, twice that in g * g)
      if (fabs(m[e] - mm) > 3e-4 * (fabs(mm) + fabs(gs)) + 1e-12 || fabs(vv[e] - v2) > 3e-4 * fabs(v2) + 1e-12) ++bad;
      if (fabs(p[e] - pp) > 1e-6) ++bad;
    }
    for (int64_t i = segs[v].off + segs[v].n; i < (v < 4 ? segs[v + 1].off : total); ++i)
      if (g[(size_t)i] != SENT || p[(size_t)i] != SENT || m[(size_t)i] != SENT || vv[(size_t)i] != SENT) ++bad;
  }
  printf("gradient scale %g clip %g grad_scale %g: %zu tiles, %d of 5 variables clipped: %d mismatches\n", gscale, clip, grad_scale,
         tiles.size(), n_clipped, bad);
  return bad;
}

int main() {
  int bad = 0;
  bad += check(1.0f, 10.f, 1.f);        // the large variables are clipped, the small ones are not
  bad += check(1e-3f, 10.f, 1.f);       // nothing is clipped: scale exactly 1
  bad += check(1.0f, 20.f, 0.5f);       // two replicas: the sum clipped at clip / grad_scale, Adam on the mean
  return bad ? 1 : 0;
}
