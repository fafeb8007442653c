// trpo.hip -- the TRPO kernels (trpo_kernels.h: advantage standardisation, surrogate / KL loss, the scalar kernel, the tangent
// level of the Fisher product, the vectors of conjugate gradient and the line search, the value-loss gradient).
// Launchers declared there.
#ifdef GRL_HOSTEMU
#include "hostemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <algorithm>
#define GRL_ELEM_TYPES_ONLY     // (the element-wise kernels are compiled in engine.hip)
#define GRL_PPO_TYPES_ONLY      // (the PPO kernels in ppo.hip)
#include "trpo_kernels.h"

namespace grl {

static dim3 elem_grid(int64_t n) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (n + 255) / 256))); }

void launch_trpo_prep(const TrpoPrepArgs& a, hipStream_t s) { hipLaunchKernelGGL(trpo_prep_kernel, dim3(1), dim3(256), 0, s, a); }
void launch_trpo_loss(const TrpoLossArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(trpo_loss_kernel, dim3(trpo_loss_blocks(a.T)), dim3(TRPO_ROWS), 0, s, a);
}
void launch_trpo_scal(const TrpoScalArgs& a, hipStream_t s) { hipLaunchKernelGGL(trpo_scal_kernel, dim3(1), dim3(64), 0, s, a); }
void launch_trpo_tan(const TrpoTanArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(trpo_tan_kernel, elem_grid((int64_t)a.rows * a.H), dim3(256), 0, s, a);
}
void launch_trpo_vec(int kind, const TrpoVecArgs& a, hipStream_t s) {
  const dim3 red(trpo_vec_blocks(a.n)), el = elem_grid(a.n);      // (the reducing launches: one partial sum per workgroup)
  switch (kind) {
    case TRPO_V_CG_INIT: hipLaunchKernelGGL(trpo_cg_init_kernel, red, dim3(256), 0, s, a); break;
    case TRPO_V_DOT: hipLaunchKernelGGL(trpo_dot_kernel, red, dim3(256), 0, s, a); break;
    case TRPO_V_CG_X: hipLaunchKernelGGL(trpo_cg_x_kernel, red, dim3(256), 0, s, a); break;
    case TRPO_V_CG_P: hipLaunchKernelGGL(trpo_cg_p_kernel, red, dim3(256), 0, s, a); break;
    case TRPO_V_FVP_FIN: hipLaunchKernelGGL(trpo_fvp_fin_kernel, el, dim3(256), 0, s, a); break;
    case TRPO_V_STEP: hipLaunchKernelGGL(trpo_step_kernel, el, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL(trpo_theta_kernel, el, dim3(256), 0, s, a); break;
  }
}
void launch_trpo_copy(float* dst, const float* src, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(trpo_copy_kernel, elem_grid(n), dim3(256), 0, s, dst, src, n);
}
void launch_trpo_gather(const float* r_obs, float* x, int ldo, int stride, int n, hipStream_t s) {
  hipLaunchKernelGGL(trpo_gather_kernel, dim3(n), dim3(256), 0, s, r_obs, x, ldo, stride, n);
}
void launch_trpo_vf_loss(const float* v, int ld_v, const float* ret, float* dv, int ld_dv, int mb, PpoDev* dev, hipStream_t s) {
  hipLaunchKernelGGL(trpo_vf_loss_kernel, dim3((mb + 255) / 256), dim3(256), 0, s, v, ld_v, ret, dv, ld_dv, mb, dev);
}

}  // namespace grl
