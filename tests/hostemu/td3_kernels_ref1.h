// td3_kernels_ref1.h -- TEST-ONLY reference form of the loss kernel of csrc/td3_kernels.h: a sequential loop over the same argument
// block, included by that header ONLY in the g++ emulation build (-DGRL_HOSTEMU -I tests/hostemu, tests/conftest.py).
// Never part of libgrl.so.  No include guard: it is pasted once, inside namespace grl.
//
// The row-local arithmetic (td3_loss_row), the optimiser words (td3_open_apply) and the slab address (td3_part_of) are the
// header's own; what is restated here is the part a workgroup does together: the five batch sums of a block, plain sums in row
// order.  td3_smooth_kernel and td3_pi_kernel are element-wise and compile as they stand.
inline void td3_loss_kernel(Td3LossArgs a) {
  if (threadIdx.x != 0) return;
  const int blk = blockIdx.x;
  float dg[TD3_DIAG] = {0.f, 0.f, 0.f, 0.f, 0.f};
  const int b1 = min((blk + 1) * PPO_LOSS_ROWS, a.B);
  for (int b = blk * PPO_LOSS_ROWS; b < b1; ++b) {
    const Td3Row r = td3_loss_row(a, b);
    dg[0] += r.l1; dg[1] += r.l2; dg[2] += r.lp; dg[3] += r.q1; dg[4] += r.q2;
  }
  float* out = td3_part_of(a, blk, (int)gridDim.x);
  if (out)
    for (int k = 0; k < TD3_DIAG; ++k) out[k] = dg[k];
  if (blk == 0) td3_open_apply(a);
}
