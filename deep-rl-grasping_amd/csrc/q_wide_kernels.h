// q_wide_kernels.h -- per-variable clip_by_norm + Adam of a DQN / BDQ handle whose variables are too large for one workgroup
// each (an MLP over a flattened image: a first kernel of 64 * 64 * C * H floats).  clip_by_norm_kernel gives every variable ONE
// 256-thread workgroup, which reads and rewrites it alone; here the bucket is cut into tiles of QW_TILE floats and both
// passes run one workgroup per tile:
//
//   q_sumsq_kernel      tile -> one float, the sum of squares of its gradients: 16-byte loads, per-thread sums over
//                       ascending addresses, a butterfly over the wave's lanes, the four wave sums added in order.  No atomics:
//                       the float goes to partials[tile].
//   q_clip_adam_kernel  tile -> adds the partials of ITS VARIABLE in index order (every tile of a variable forms the same
//                       bits), scale = clip / max(sqrt(sum), clip) as clip_by_norm_kernel writes it, the clipped gradient back
//                       to the bucket (what grl_get_gradients hands out), then TF-Adam with the expressions of
//                       adam_polyak_kernel (adam_elem on grad_scaled(g, grad_scale), step size from DevScalars).
//
// The tile table is built once on the host (qw_build_tiles): a tile never spans two variables, a variable of at most QW_TILE
// floats is one tile.  Bytes per update and variable of n floats: 4 n read by the first launch, 16 n read + 16 n written by
// the second (gradient, parameter, two moments) -- what clip_by_norm + adam moved, spread over n / QW_TILE workgroups.
#pragma once
#include <vector>
#include "elem_kernels.h"

namespace grl {

#define QW_TILE 4096        /* floats per tile: 256 threads x 4 quads */
#define QW_WIDE_MIN 131072  /* a handle is wide when a trainable variable has MORE floats than this */

struct QwTile {
  int64_t off;      // first float of the tile inside the gradient bucket (== inside params / adam_m / adam_v)
  int32_t n;        // floats of the tile, 1 ... QW_TILE
  int32_t var;      // index of its variable among the trainable ones
  int32_t p0, np;   // the partial sums of its variable: partials[p0 ... p0 + np)
};

// variable, offset, count: the tiles of every segment in order; the tiles of one variable are consecutive, so partials[k]
// belongs to tile k and a variable's partials are the run [p0, p0 + np)
inline std::vector<QwTile> qw_build_tiles(const VarSeg* segs, int n_seg) {
  std::vector<QwTile> tiles;
  for (int v = 0; v < n_seg; ++v) {
    const int32_t p0 = (int32_t)tiles.size();
    const int32_t np = (int32_t)((segs[v].n + QW_TILE - 1) / QW_TILE);
    for (int32_t k = 0; k < np; ++k) {
      const int64_t first = (int64_t)k * QW_TILE;
      const int64_t left = segs[v].n - first;
      tiles.push_back(QwTile{segs[v].off + first, (int32_t)(left < QW_TILE ? left : QW_TILE), v, p0, np});
    }
  }
  return tiles;
}

#ifndef GRL_QW_TYPES_ONLY
#ifdef GRL_HOSTEMU
#include "q_wide_ref1.h"   // tests/hostemu: the emulation build only
#else
typedef float qw_f4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) qw_f4* qw_gq;
typedef __attribute__((address_space(1))) qw_f4* qw_gqw;
typedef const __attribute__((address_space(1))) float* qw_g1;
typedef __attribute__((address_space(1))) float* qw_g1w;

// (every variable starts 16-byte aligned in the bucket and QW_TILE is a multiple of 4: a tile's quads are aligned; the last
//  quad of a variable whose size is no multiple of 4 is taken float by float -- the padding behind it is never touched)
__global__ __launch_bounds__(256) void q_sumsq_kernel(const float* __restrict__ grads, const QwTile* __restrict__ tiles,
                                                      float* __restrict__ partials) {
  __shared__ float wsum[4];
  const QwTile tl = tiles[blockIdx.x];
  const int t = threadIdx.x;
  const float* g = grads + tl.off;
  constexpr int NQ = QW_TILE / 1024;      // quads per thread
  float ss = 0.f;
  if (tl.n == QW_TILE) {      // a full tile: every load in flight before the first add; the adds in ascending j as below
    qw_f4 x[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) x[j] = *(qw_gq)(g + 4 * (j * 256 + t));
#pragma unroll
    for (int j = 0; j < NQ; ++j) { ss += x[j].x * x[j].x; ss += x[j].y * x[j].y; ss += x[j].z * x[j].z; ss += x[j].w * x[j].w; }
  } else {
    for (int j = 0; j < NQ; ++j) {
      const int i = 4 * (j * 256 + t);
      if (i + 4 <= tl.n) {
        const qw_f4 x = *(qw_gq)(g + i);
        ss += x.x * x.x; ss += x.y * x.y; ss += x.z * x.z; ss += x.w * x.w;
      } else {
        for (int e = i; e < tl.n; ++e) { const float x = ((qw_g1)g)[e]; ss += x * x; }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
  if ((t & 63) == 0) wsum[t >> 6] = ss;
  __syncthreads();
  if (t == 0) ((qw_g1w)partials)[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one quad: the gradient clipped in place, then adam_polyak_kernel's element update on grad_scaled(g, grad_scale)
__device__ __forceinline__ void qw_quad(qw_f4& g4, qw_f4& p4, qw_f4& m4, qw_f4& v4, float sc, float grad_scale, float alpha, float eps) {
  float ge[4] = {g4.x, g4.y, g4.z, g4.w}, pe[4] = {p4.x, p4.y, p4.z, p4.w}, me[4] = {m4.x, m4.y, m4.z, m4.w},
        ve[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    ge[w] *= sc;
    adam_elem(grad_scaled(ge[w], grad_scale), pe[w], me[w], ve[w], alpha, eps);
  }
  g4 = qw_f4{ge[0], ge[1], ge[2], ge[3]}; p4 = qw_f4{pe[0], pe[1], pe[2], pe[3]};
  m4 = qw_f4{me[0], me[1], me[2], me[3]}; v4 = qw_f4{ve[0], ve[1], ve[2], ve[3]};
}

__global__ __launch_bounds__(256) void q_clip_adam_kernel(float* __restrict__ grads, const QwTile* __restrict__ tiles,
                                                          const float* __restrict__ partials, float clip, AdamArgs a) {
  const QwTile tl = tiles[blockIdx.x];
  const int t = threadIdx.x;
  float sum = 0.f;
  for (int k = 0; k < tl.np; ++k) sum += ((qw_g1)partials)[tl.p0 + k];      // index order: the same bits in every tile of the variable
  const float sc = clip / fmaxf(sqrtf(sum), clip);
  const float alpha = a.sc->adam_alpha;
  float* g = grads + tl.off;
  float* p = a.params + tl.off; float* m = a.m + tl.off; float* v = a.v + tl.off;
  constexpr int NQ = QW_TILE / 1024;
  if (tl.n == QW_TILE) {      // a full tile: the four arrays' quads requested together, then the arithmetic, then the stores
    qw_f4 g4[NQ], p4[NQ], m4[NQ], v4[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int i = 4 * (j * 256 + t);
      g4[j] = *(qw_gq)(g + i); p4[j] = *(qw_gq)(p + i); m4[j] = *(qw_gq)(m + i); v4[j] = *(qw_gq)(v + i);
    }
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int i = 4 * (j * 256 + t);
      qw_quad(g4[j], p4[j], m4[j], v4[j], sc, a.grad_scale, alpha, a.eps);
      *(qw_gqw)(g + i) = g4[j]; *(qw_gqw)(p + i) = p4[j]; *(qw_gqw)(m + i) = m4[j]; *(qw_gqw)(v + i) = v4[j];
    }
    return;
  }
  for (int j = 0; j < NQ; ++j) {
    const int i = 4 * (j * 256 + t);
    if (i + 4 <= tl.n) {
      qw_f4 g4 = *(qw_gq)(g + i), p4 = *(qw_gq)(p + i), m4 = *(qw_gq)(m + i), v4 = *(qw_gq)(v + i);
      qw_quad(g4, p4, m4, v4, sc, a.grad_scale, alpha, a.eps);
      *(qw_gqw)(g + i) = g4; *(qw_gqw)(p + i) = p4; *(qw_gqw)(m + i) = m4; *(qw_gqw)(v + i) = v4;
    } else {
      for (int e = i; e < tl.n; ++e) {
        const float ge = ((qw_g1)g)[e] * sc;
        float pe = ((qw_g1)p)[e], me = ((qw_g1)m)[e], ve = ((qw_g1)v)[e];
        adam_elem(grad_scaled(ge, a.grad_scale), pe, me, ve, alpha, a.eps);
        ((qw_g1w)g)[e] = ge; ((qw_g1w)p)[e] = pe; ((qw_g1w)m)[e] = me; ((qw_g1w)v)[e] = ve;
      }
    }
  }
}
#endif
#endif  // GRL_QW_TYPES_ONLY

// the two launches (q_wide.hip); clip is the threshold on what the bucket holds (data parallel: clip / grad_scale on the sum)
void launch_q_sumsq(const float* grads, const QwTile* tiles, int n_tiles, float* partials, hipStream_t s);
void launch_q_clip_adam(float* grads, const QwTile* tiles, int n_tiles, const float* partials, float clip, const AdamArgs& a,
                        hipStream_t s);

}  // namespace grl
