// td3.hip -- the TD3 kernels (td3_kernels.h: target-action smoothing, policy output forward / backward, loss).  Launchers declared there.
#ifdef GRL_HOSTEMU
#include "hostemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#define GRL_ELEM_TYPES_ONLY     // (the element-wise kernels are compiled in engine.hip)
#include "td3_kernels.h"

namespace grl {

void launch_td3_smooth(const Td3SmoothArgs& a, hipStream_t s) {
  const long n = (long)a.B * ((a.A + 1) / 2);
  hipLaunchKernelGGL(td3_smooth_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
}
void launch_td3_pi(const Td3PiArgs& a, hipStream_t s) {
  const long n = (long)a.rows * a.A;
  hipLaunchKernelGGL(td3_pi_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
}
void launch_td3_loss(const Td3LossArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(td3_loss_kernel, dim3(td3_loss_blocks(a.B)), dim3(PPO_LOSS_ROWS), 0, s, a);
}
void launch_td3_carry(Td3Dev* dev, const float* part, int nblk, int B, hipStream_t s) {
  hipLaunchKernelGGL(td3_carry_kernel, dim3(1), dim3(1), 0, s, dev, part, nblk, B);
}

}  // namespace grl
