// ae_general_ref1.h -- TEST-ONLY reference form of aeg_tapsum_mse_kernel (csrc/ae_general.h): one sequential loop per workgroup
// over the same descriptor, included by that header ONLY in the g++ emulation build (-DGRL_HOSTEMU -I tests/hostemu).  Never
// part of libgrl.so.  No include guard: it is pasted once, inside namespace grl.  (The other kernels of ae_general.h use
// neither shared memory nor barriers: the emulation runs them as they are, thread after thread.)
inline void aeg_tapsum_mse_kernel(AegTapMseArgs a) {
  if (threadIdx.x != 0) return;
  float sd = 0.f, sg = 0.f;
  for (int t = 0; t < 256; ++t) {
    const long o = (long)blockIdx.x * 256 + t;
    if (o >= a.n_pix) break;
    const long n = o >> 12;
    const int oh = (int)((o >> 6) & 63), ow = (int)(o & 63);
    float s = 0.f;
    for (int kh = 0; kh < a.k; ++kh) {
      const int ih = oh + kh - a.lo;
      if (ih < 0 || ih > 63) continue;
      for (int kw = 0; kw < a.k; ++kw) {
        const int iw = ow + kw - a.lo;
        if (iw < 0 || iw > 63) continue;
        s += a.T[(long)(kh * a.k + kw) * a.ldT + (n << 10) + ((ih >> 1) << 5) + (iw >> 1)];
      }
    }
    const float ov = s + a.bias[0];
    a.out[o] = ov;
    const float d = ov - a.x[o];
    const float g = d * (2.f / (float)a.n_pix);
    a.gpad[(n * a.Gp + oh + a.hi) * a.Gp + ow + a.hi] = g;
    sd += d * d;
    sg += g;
  }
  a.partial[blockIdx.x] = sd;
  a.partial_g[blockIdx.x] = sg;
}
