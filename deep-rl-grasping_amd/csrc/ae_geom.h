// ae_geom.h -- host-only geometry of the auto-encoder's GENERAL route (plan_ae.inl: any three-layer, stride-2 encoder of
// encoders.py:85-124 on a 64 x 64 x 1 image): the supported domain, TensorFlow 'SAME' borders, the zero-bordered buffer
// layouts and the offset tables that are not built by grl_ctx::conv_fwd_tabs / conv_bwd_tabs.  Plain C++ (no HIP, no
// grl_ctx) so that tests/csrc/ae_general_check.cpp can sweep it under AddressSanitizer / UBSan.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace grl {

struct AeNet {
  int k[3], f[3], dim;
  float alpha;
  bool shipped() const {
    return k[0] == 7 && k[1] == 5 && k[2] == 3 && f[0] == 32 && f[1] == 32 && f[2] == 32 && dim == 100 && alpha == 0.1f;
  }
};
inline AeNet ae_shipped_net() { return AeNet{{7, 5, 3}, {32, 32, 32}, 100, 0.1f}; }
inline const char* ae_domain_text() {
  return "supported auto-encoders: three encoder layers of stride 2 on a 64x64x1 image, kernel_size 1..9, filters a multiple "
         "of 4 in 4..64, encoding_dim 1..1024, 0 <= alpha < 1";
}
inline bool ae_net_ok(const AeNet& n) {
  for (int l = 0; l < 3; ++l)
    if (n.k[l] < 1 || n.k[l] > 9 || n.f[l] < 4 || n.f[l] > 64 || (n.f[l] % 4)) return false;
  return n.dim >= 1 && n.dim <= 1024 && n.alpha >= 0.f && n.alpha < 1.f;
}

// TensorFlow 'SAME': out = ceil(in / s), total = max((out - 1) s + k - in, 0), low = total / 2 (the high side takes the odd one)
inline void ae_same_pad(int n_in, int k, int s, int* lo, int* hi) {
  const int out = (n_in + s - 1) / s;
  const int tot = (out - 1) * s + k - n_in > 0 ? (out - 1) * s + k - n_in : 0;
  *lo = tot / 2;
  *hi = tot - tot / 2;
}

// One convolution: input H x H x C (the up-sampled image for decoder layers), kernel k, stride S, output OH x OH x F; consumed as a
// 'valid' convolution over its input kept with a zero border of lo / hi pixels: Hp = H + lo + hi
struct AeConv {
  int H, C, k, S, OH, F, lo, hi;
  int Hp() const { return H + lo + hi; }
  int64_t bordered_elems(int B) const { return (int64_t)B * Hp() * Hp() * C; }
};
struct AeGeom {
  AeConv enc[3];   // conv2d_1..3
  AeConv dec[3];   // conv2d_4..6 (dec[2]: the one-channel output convolution)
};
inline AeGeom ae_geometry(const AeNet& n) {
  AeGeom g;
  for (int l = 0; l < 3; ++l) {
    AeConv& e = g.enc[l];
    e.H = 64 >> l; e.C = l == 0 ? 1 : n.f[l - 1]; e.k = n.k[l]; e.S = 2; e.OH = e.H / 2; e.F = n.f[l];
    ae_same_pad(e.H, e.k, 2, &e.lo, &e.hi);
    AeConv& d = g.dec[l];
    d.H = 16 << l; d.C = n.f[2 - l]; d.k = n.k[2 - l]; d.S = 1; d.OH = d.H; d.F = l == 2 ? 1 : n.f[1 - l];
    ae_same_pad(d.H, d.k, 1, &d.lo, &d.hi);
  }
  return g;
}

// output pixel (n, oh, ow) of an H x H x C tensor -> offset of its first channel in [B, H + lo + hi, H + lo + hi, C]
inline std::vector<int32_t> ae_bordered_rows(int B, int H, int lo, int hi, int C) {
  std::vector<int32_t> ct((size_t)B * H * H);
  const int Hp = H + lo + hi;
  for (int n = 0; n < B; ++n)
    for (int oh = 0; oh < H; ++oh)
      for (int ow = 0; ow < H; ++ow) ct[((size_t)n * H + oh) * H + ow] = ((n * Hp + oh + lo) * Hp + ow + lo) * C;
  return ct;
}

// The output convolution (k x k 'same', F0 -> 1 channel over the 2 x up-sampled d5 [B, 32, 32, F0]) in the backward pass works
// on the output gradient kept with a zero border: gpad [B, Gp, Gp], Gp = 64 + k - 1, the image at (hi, hi).  (out[o] = sum_t
// u[o + t - lo] W[t], so pixel p of u receives g[p - t + lo]: offsets -hi .. +lo around p.)
struct AeOutTabs {
  int Gp;                          // side of the bordered gradient image
  std::vector<int32_t> pix;        // [B * 1024]: pixel q = (n, qy, qx) of d5 -> offset of gradient pixel (2 qy, 2 qx)
  std::vector<int32_t> bwd_r;      // [4 k^2]: (sub-position s, tap) -> offset from pix[q]   (backward-data, reduction index)
  std::vector<int32_t> wg_i[4];    // [k^2] per sub-position: tap -> offset from pix[q]      (weight gradient, row index)
};
inline AeOutTabs ae_out_tabs(int B, int k) {
  int lo, hi;
  ae_same_pad(64, k, 1, &lo, &hi);
  AeOutTabs t;
  t.Gp = 64 + k - 1;
  t.pix.resize((size_t)B * 1024);
  for (int n = 0; n < B; ++n)
    for (int qy = 0; qy < 32; ++qy)
      for (int qx = 0; qx < 32; ++qx) t.pix[((size_t)n * 32 + qy) * 32 + qx] = (n * t.Gp + 2 * qy + hi) * t.Gp + 2 * qx + hi;
  t.bwd_r.resize((size_t)4 * k * k);
  for (int s = 0; s < 4; ++s) {
    t.wg_i[s].resize((size_t)k * k);
    for (int kh = 0; kh < k; ++kh)
      for (int kw = 0; kw < k; ++kw) {
        const int off = ((s >> 1) - kh + lo) * t.Gp + (s & 1) - kw + lo;
        t.bwd_r[(size_t)s * k * k + kh * k + kw] = off;
        t.wg_i[s][(size_t)kh * k + kw] = off;
      }
  }
  return t;
}

}  // namespace grl
