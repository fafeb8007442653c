// ppo.hip -- the PPO2 kernels (ppo_kernels.h: one-launch act, policy tail, rewards, GAE, minibatch gather, tanh, loss, observe).
// Launchers declared there.
#ifdef GRL_HOSTEMU
#include "hostemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <algorithm>
#define GRL_ELEM_TYPES_ONLY     // (the element-wise kernels are compiled in engine.hip)
#include "ppo_kernels.h"

namespace grl {

void launch_ppo_act(const PpoActArgs& a, hipStream_t s) { hipLaunchKernelGGL(ppo_act_kernel, dim3(a.s.n, 2), dim3(256), 0, s, a); }
void launch_ppo_sample(const PpoSampleArgs& a, hipStream_t s) { hipLaunchKernelGGL(ppo_sample_kernel, dim3(a.n), dim3(256), 0, s, a); }
void launch_ppo_rewards(const float* rew_in, float* r_rew, PpoDev* dev, int n, int n_steps, hipStream_t s) {
  hipLaunchKernelGGL(ppo_rewards_kernel, dim3(1), dim3(256), 0, s, rew_in, r_rew, dev, n, n_steps);
}
void launch_gae(const GaeArgs& a, hipStream_t s) { hipLaunchKernelGGL(gae_kernel, dim3((a.n_envs + 63) / 64), dim3(64), 0, s, a); }
void launch_ppo_gather(const PpoGatherArgs& a, hipStream_t s) { hipLaunchKernelGGL(ppo_gather_kernel, dim3(a.mb + 1), dim3(256), 0, s, a); }
// (a workgroup walks its share of the largest tensor in steps of gridDim.x * 256 quads: at most 1024 workgroups per tensor)
static dim3 tanh_grid(int n_desc, int rows, int max_h) {
  const long quads = ((long)rows * max_h + 3) / 4;
  return dim3((unsigned)std::max<long>(1, std::min<long>(1024, (quads + 255) / 256)), n_desc);
}
void launch_tanh_fwd(const TanhDesc* descs, int n_desc, int rows, int max_h, hipStream_t s) {
  hipLaunchKernelGGL(tanh_fwd_kernel, tanh_grid(n_desc, rows, max_h), dim3(256), 0, s, descs, rows);
}
void launch_tanh_bwd(const TanhDesc* descs, int n_desc, int rows, int max_h, hipStream_t s) {
  hipLaunchKernelGGL(tanh_bwd_kernel, tanh_grid(n_desc, rows, max_h), dim3(256), 0, s, descs, rows);
}
void launch_ppo_loss(const PpoLossArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ppo_loss_kernel, dim3(ppo_loss_blocks(a.mb)), dim3(PPO_LOSS_ROWS), 0, s, a);
}
// (one thread per column of the normalised rows, the zero padding included)
void launch_ppo_observe(const PpoObserveArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ppo_observe_kernel, dim3((a.ldo + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace grl
