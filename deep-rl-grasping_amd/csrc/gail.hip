// gail.hip -- the kernels of a GAIL session (gail_kernels.h: the discriminator's input with its running statistics, the loss
// over generator and expert logits, the reward of a rollout).  Launchers declared there.
#ifdef GRL_HOSTEMU
#include "hostemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#define GRL_ELEM_TYPES_ONLY     // (the element-wise kernels are compiled in engine.hip)
#include "gail_kernels.h"

namespace grl {

void launch_gail_open(GailDev* dev, const float* obs, const float* act, const int32_t* gen_idx, const int32_t* exp_idx, hipStream_t s) {
  hipLaunchKernelGGL(gail_open_kernel, dim3(1), dim3(1), 0, s, dev, obs, act, gen_idx, exp_idx);
}
// (one thread per column of the input; the zero padding behind the action columns is never written)
void launch_gail_input(const GailInputArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gail_input_kernel, dim3((a.obs_dim + a.A + 255) / 256), dim3(256), 0, s, a);
}
void launch_gail_loss(const GailLossArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gail_loss_kernel, dim3(gail_loss_blocks(a.batch)), dim3(GAIL_LOSS_ROWS), 0, s, a);
}
void launch_gail_reward(const GailRewardArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gail_reward_kernel, dim3((a.T + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace grl
