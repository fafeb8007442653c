// q_act_ref1.h -- TEST-ONLY reference form of q_act_kernel (csrc/q_act.h): sequential loops over the same descriptor,
// included by that header ONLY in the g++ emulation build (-DGRL_HOSTEMU -I tests/hostemu, tests/conftest.py).
// Never part of libgrl.so.  No include guard: it is pasted once, inside namespace grl.
// Every layer sums k in order with fmaf and adds the bias last, as the emulation's GEMM reference does (igemm2_ref1.h), and
// the dueling combination is dueling_kernel's expression: the bins are the arg-max of the Q-values the emulated Q-value path
// of grl_act returns, bit for bit.
inline void qa_ref_layer(const float* x, int K, const float* w, const float* b, int N, bool relu, float* out) {
  for (int j = 0; j < N; ++j) {
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(x[k], w[(long)k * N + j], acc);
    const float v = acc + b[j];
    out[j] = relu ? fmaxf(v, 0.f) : v;
  }
}
inline void q_act_kernel(QActArgs a) {
  if (threadIdx.x != 0) return;
  const int br = blockIdx.y;
  for (int row = blockIdx.x * HT_RB; row < std::min(a.rows, (int)blockIdx.x * HT_RB + HT_RB); ++row) {
    float h[2][QA_MAXK], adv[QM_W], v = 0.f;
    const float* x = a.obs + (long)row * a.ld_obs;
    int K = a.obs_dim, cur = 0;
    for (int k = 0; k < a.Lc; ++k) {
      qa_ref_layer(x, K, a.trunk[k].w, a.trunk[k].b, a.trunk[k].n, true, h[cur]);
      x = h[cur]; K = a.trunk[k].n; cur ^= 1;
    }
    for (int pass = 0; pass < 2; ++pass) {      // the branch's tower, then the value tower, both on the trunk's output
      const QActTower& T = a.tw[pass == 0 ? br : a.D];
      float z[2][QA_MAXK];
      const float* zin = x;
      int kz = K, cz = 0;
      for (int l = 0; l < T.L; ++l) {
        qa_ref_layer(zin, kz, T.lay[l].w, T.lay[l].b, T.lay[l].n, true, z[cz]);
        zin = z[cz]; kz = T.lay[l].n; cz ^= 1;
      }
      if (pass == 0) qa_ref_layer(zin, kz, T.ow, T.ob, a.nb, false, adv);
      else qa_ref_layer(zin, kz, T.ow, T.ob, 1, false, &v);
    }
    float m = 0.f;
    for (int k = 0; k < a.nb; ++k) m += adv[k];
    m /= (float)a.nb;
    int best = 0;
    float best_q = v + adv[0] - m;
    for (int k = 1; k < a.nb; ++k) {
      const float val = v + adv[k] - m;
      if (qa_better(val, best_q)) { best_q = val; best = k; }
    }
    const float e = a.explore[(long)row * a.D + br];
    a.bins[(long)row * a.D + br] = e >= 0.f ? e : (float)best;
  }
  if (a.done) *a.done += 1u;
}
