// q_wide_ref1.h -- TEST-ONLY reference form of the kernels of csrc/q_wide_kernels.h (sequential loops over the same tile table),
// included by that header ONLY in the g++ emulation build (-DGRL_HOSTEMU -I tests/hostemu, tests/conftest.py).
// Never part of libgrl.so.  No include guard: it is pasted once, inside namespace grl.
inline void q_sumsq_kernel(const float* grads, const QwTile* tiles, float* partials) {
  if (threadIdx.x != 0) return;
  const QwTile tl = tiles[blockIdx.x];
  float ss = 0.f;
  for (int i = 0; i < tl.n; ++i) ss += grads[tl.off + i] * grads[tl.off + i];
  partials[blockIdx.x] = ss;
}

inline void q_clip_adam_kernel(float* grads, const QwTile* tiles, const float* partials, float clip, AdamArgs a) {
  if (threadIdx.x != 0) return;
  const QwTile tl = tiles[blockIdx.x];
  float sum = 0.f;
  for (int k = 0; k < tl.np; ++k) sum += partials[tl.p0 + k];
  const float sc = clip / fmaxf(sqrtf(sum), clip);
  const float alpha = a.sc->adam_alpha;
  for (int64_t e = tl.off; e < tl.off + tl.n; ++e) {
    const float g = grads[e] * sc;
    grads[e] = g;
    adam_elem(grad_scaled(g, a.grad_scale), a.params[e], a.m[e], a.v[e], alpha, a.eps);
  }
}
