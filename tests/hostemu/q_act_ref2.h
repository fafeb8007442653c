// q_act_ref2.h -- TEST-ONLY reference form of q_act_norm_kernel (csrc/q_act.h), the instantiation of the one-launch
// epsilon-greedy act that reads RAW observations and applies VecNormalize.normalize_obs itself: included by that header ONLY in
// the g++ emulation build (-DGRL_HOSTEMU -I tests/hostemu, tests/conftest.py), behind q_act_ref1.h.  Never part of libgrl.so.
// No include guard: it is pasted once, inside namespace grl.
// The rows of the workgroup are normalised element by element with norm_obs_act (csrc/elem_kernels.h: the float64 expression of
// the gather and of act_ingest_kernel, a NaN kept as np.clip keeps it) and handed to the sequential reference of the plain
// instantiation: the bins are those of q_act_kernel on the normalised rows, bit for bit.
inline void q_act_norm_kernel(QActArgs a, QActNorm nm) {
  if (threadIdx.x != 0) return;
  const int row0 = (int)blockIdx.x * HT_RB, row1 = std::min(a.rows, row0 + HT_RB);
  float* x = (float*)calloc((size_t)a.rows * a.obs_dim, sizeof(float));     // [rows, obs_dim]; only this workgroup's rows are filled
  for (int row = row0; row < row1; ++row)
    for (int e = 0; e < a.obs_dim; ++e)
      x[(size_t)row * a.obs_dim + e] = norm_obs_act(a.obs[(long)row * a.ld_obs + e], nm.mean[e], nm.stdv[e], nm.clip_obs);
  QActArgs b = a;
  b.obs = x; b.ld_obs = a.obs_dim;
  q_act_kernel(b);
  free(x);
}
