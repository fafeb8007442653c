// ln_kernels_ref1.h -- TEST-ONLY reference form of the kernels of csrc/ln_kernels.h: sequential loops over the same
// descriptors, included by that header ONLY in the g++ emulation build (-DGRL_HOSTEMU -I tests/hostemu, tests/conftest.py).
// Never part of libgrl.so.  No include guard: it is pasted once, inside namespace grl.
//
// ln_relu_fwd_ref / ln_relu_bwd_ref are the host forms (rows [row0, row1) of one descriptor); the *_kernel wrappers give them
// the kernels' names and grid so that the launchers of ln_kernels.h serve both builds.
inline void ln_relu_fwd_ref(const LnDesc& d, int row0, int row1) {
  const int H = d.H;
  const float inv = 1.0f / (float)H;
  for (int row = row0; row < row1; ++row) {
    const float* u = d.u + (long)row * H;
    float* z = d.z + (long)row * H;
    float s = 0.f;
    for (int c = 0; c < H; ++c) s += u[c];
    const float mean = s * inv;
    float q = 0.f;
    for (int c = 0; c < H; ++c) q += (u[c] - mean) * (u[c] - mean);      // two passes: deviations from the mean formed first
    const float rstd = ln_rstd(q * inv);
    for (int c = 0; c < H; ++c) z[c] = fmaxf(ln_y(ln_xhat(u[c], mean, rstd), d.gamma[c], d.beta[c]), 0.f);
    if (d.stat) { d.stat[2 * (long)row] = mean; d.stat[2 * (long)row + 1] = rstd; }
  }
}

// rows [row0, row1) are ONE block of the slab list (blk = row0 / LN_BWD_ROWS)
inline void ln_relu_bwd_ref(const LnDesc& d, int row0, int row1) {
  const int H = d.H;
  const float inv = 1.0f / (float)H;
  float* slab = d.slab + (long)(row0 / LN_BWD_ROWS) * 2 * H;
  for (int c = 0; c < 2 * H; ++c) slab[c] = 0.f;
  for (int row = row0; row < row1; ++row) {
    const float* u = d.u + (long)row * H;
    float* dz = d.dz + (long)row * H;
    const float mean = d.stat[2 * (long)row], rstd = d.stat[2 * (long)row + 1];
    float s1 = 0.f, s2 = 0.f;
    for (int c = 0; c < H; ++c) {
      const float xh = ln_xhat(u[c], mean, rstd);
      const float dy = ln_y(xh, d.gamma[c], d.beta[c]) > 0.f ? dz[c] : 0.f;
      slab[c] += dy;
      slab[H + c] += dy * xh;
      dz[c] = dy * d.gamma[c];      // g, until the row's two means are known
      s1 += dz[c];
      s2 += dz[c] * xh;
    }
    const float m1 = s1 * inv, m2 = s2 * inv;
    for (int c = 0; c < H; ++c) dz[c] = rstd * (dz[c] - m1 - ln_xhat(u[c], mean, rstd) * m2);
  }
}

template <int NPL>
inline void ln_relu_fwd_kernel(const LnDesc* descs, int rows) {
  if (threadIdx.x != 0) return;
  const int row0 = (int)blockIdx.x * LN_FWD_ROWS;
  if (row0 < rows) ln_relu_fwd_ref(descs[blockIdx.y], row0, min(row0 + LN_FWD_ROWS, rows));
}
template <int NPL>
inline void ln_relu_bwd_kernel(const LnDesc* descs, int rows) {
  if (threadIdx.x % 64 != 0) return;
  const int row0 = ((int)blockIdx.x * LN_BWD_WAVES + (int)threadIdx.x / 64) * LN_BWD_ROWS;
  if (row0 < rows) ln_relu_bwd_ref(descs[blockIdx.y], row0, min(row0 + LN_BWD_ROWS, rows));
}
