// q_wide.hip -- the tiled clip_by_norm + Adam launches of wide DQN / BDQ handles (q_wide_kernels.h).  Launchers declared there.
#ifdef GRL_HOSTEMU
#include "hostemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#define GRL_ELEM_TYPES_ONLY     // (the element-wise kernels are compiled in engine.hip)
#include "q_wide_kernels.h"

namespace grl {

void launch_q_sumsq(const float* grads, const QwTile* tiles, int n_tiles, float* partials, hipStream_t s) {
  hipLaunchKernelGGL(q_sumsq_kernel, dim3(n_tiles), dim3(256), 0, s, grads, tiles, partials);
}
void launch_q_clip_adam(float* grads, const QwTile* tiles, int n_tiles, const float* partials, float clip, const AdamArgs& a,
                        hipStream_t s) {
  hipLaunchKernelGGL(q_clip_adam_kernel, dim3(n_tiles), dim3(256), 0, s, grads, tiles, partials, clip, a);
}

}  // namespace grl
