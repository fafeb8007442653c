// ae_general.h -- kernels of the auto-encoder's GENERAL route (plan_ae.inl, plan_ae_general): the pieces of the training step
// that ae_kernels.h writes for the shipped network only (7 x 7 output kernel, 49 taps, borders of 2 / 3 pixels), here with the
// kernel size and the borders as arguments.  The convolutions, dense layers and their gradients run on the implicit-GEMM
// kernels; up-sampling (upsample2_kernel / upsample2_bwd_kernel) and ae_finish_kernel of ae_kernels.h take any channel count
// as they are.  No atomics: every output element has one writer and every sum a fixed order.
#pragma once
#include "ae_kernels.h"

namespace grl {

// Opens a step (n_prep > 0) or an encode call (n_prep == 0).  Blocks [0, n_prep): the k x k x F0 output kernel repeated four
// times behind each other (the backward-data GEMM of the output convolution reduces over the four sub-positions of a 2 x 2
// up-sampling block, each with the whole kernel: Q = W6x4 [4 k^2, F0]).  The other blocks copy the one-channel 64 x 64 images
// into the interior of their zero-bordered buffer [N, Hp, Hp] (border `lo` in front; written once, kept zero).
__global__ __launch_bounds__(256) void aeg_prep_kernel(const float* __restrict__ W6, float* __restrict__ W6x4, int n_w, int n_prep,
                                                      const float* __restrict__ x, float* __restrict__ xp, long total, int lo,
                                                      int Hp) {
  if ((int)blockIdx.x < n_prep) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n_w) {
      const float v = W6[e];
#pragma unroll
      for (int s = 0; s < 4; ++s) W6x4[(long)s * n_w + e] = v;
    }
    return;
  }
  const long e = (long)(blockIdx.x - n_prep) * 256 + threadIdx.x;
  if (e >= total) return;
  const long n = e >> 12;
  const int y = (int)((e >> 6) & 63), c = (int)(e & 63);
  xp[(n * Hp + y + lo) * Hp + c + lo] = x[e];
}

// Output convolution k x k 'same' (TensorFlow borders: `lo` pixels in front), F0 -> 1 channel, behind the tap GEMM
// T[tap, q] = sum_c W[tap, c] d5[q, c] over the 32 x 32 pixels q of the layer in FRONT of the up-sampling:
//   out[n, oh, ow] = b + sum_{kh, kw} T[kh k + kw, (n, (oh + kh - lo) / 2, (ow + kw - lo) / 2)]     (taps outside the image skipped)
// -- ae_tapsum_kernel for any k.  Thread = output pixel; kh-major order.
__device__ __forceinline__ float aeg_tapsum(const float* __restrict__ T, long ldT, long o, int k, int lo) {
  const long n = o >> 12;
  const int oh = (int)((o >> 6) & 63), ow = (int)(o & 63);
  float s = 0.f;
  for (int kh = 0; kh < k; ++kh) {
    const int ih = oh + kh - lo;
    if (ih < 0 || ih > 63) continue;
    for (int kw = 0; kw < k; ++kw) {
      const int iw = ow + kw - lo;
      if (iw < 0 || iw > 63) continue;
      s += T[(long)(kh * k + kw) * ldT + (n << 10) + ((ih >> 1) << 5) + (iw >> 1)];
    }
  }
  return s;
}
__global__ __launch_bounds__(256) void aeg_tapsum_kernel(const float* __restrict__ T, long ldT, const float* __restrict__ bias,
                                                        float* __restrict__ out, long n_pix, int k, int lo) {
  const long o = (long)blockIdx.x * 256 + threadIdx.x;
  if (o >= n_pix) return;
  out[o] = aeg_tapsum(T, ldT, o, k, lo) + bias[0];
}

// The gather-sum and the MSE behind it as one launch (training steps): out, the loss term and the output gradient
// g = 2 (out - x) / n, stored into the zero-bordered gradient image gpad [N, Gp, Gp] at (oh + hi, ow + hi) -- the only form
// the backward launches read (ae_geom.h: AeOutTabs).  Per workgroup: sum of (out - x)^2 and of g (ae_finish_kernel adds them).
struct AegTapMseArgs {
  const float* T; long ldT; const float* bias; long n_pix;
  int k, lo, hi, Gp;
  float* out; const float* x; float* gpad; float* partial; float* partial_g;
};
__device__ __forceinline__ long aeg_pad_index(long o, int hi, int Gp) {
  const long n = o >> 12;
  return (n * Gp + ((o >> 6) & 63) + hi) * Gp + (o & 63) + hi;
}
#ifdef GRL_HOSTEMU
#include "ae_general_ref1.h"   // tests/hostemu: the emulation build only
#else
__global__ __launch_bounds__(256) void aeg_tapsum_mse_kernel(AegTapMseArgs a) {
  __shared__ float red[256], redg[256];
  const long o = (long)blockIdx.x * 256 + threadIdx.x;
  float dd = 0.f, g = 0.f;
  if (o < a.n_pix) {
    const float ov = aeg_tapsum(a.T, a.ldT, o, a.k, a.lo) + a.bias[0];
    a.out[o] = ov;
    const float d = ov - a.x[o];
    g = d * (2.f / (float)a.n_pix);
    a.gpad[aeg_pad_index(o, a.hi, a.Gp)] = g;
    dd = d * d;
  }
  red[threadIdx.x] = dd; redg[threadIdx.x] = g;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) { red[threadIdx.x] += red[threadIdx.x + off]; redg[threadIdx.x] += redg[threadIdx.x + off]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { a.partial[blockIdx.x] = red[0]; a.partial_g[blockIdx.x] = redg[0]; }
}
#endif

}  // namespace grl
