// gail_kernels_ref1.h -- TEST-ONLY sequential form of what a workgroup of csrc/gail_kernels.h's loss launch does together,
// included by that header ONLY in the g++ emulation build (-DGRL_HOSTEMU -I tests/hostemu, tests/conftest.py).  Never part of
// libgrl.so.  No include guard: it is pasted once, inside namespace grl.
//
// The emulation runs the lanes of a workgroup one after the other, so nothing can meet in a cross-lane exchange.  Lane 0 walks
// the rows of its workgroup in order -- the row-local arithmetic (gail_loss_row) is the header's own -- and adds their shares of
// the six sums in row order; the other lanes return.  The input launch and the reward launch are lane-local: the emulation runs
// the header's own code.
inline void gail_loss_kernel(GailLossArgs a) {
  if (threadIdx.x != 0) return;
  const int blk = blockIdx.x, cur = a.dev->cur, n_e = a.dev->n_e;
  float s[GAIL_DIAG] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int r1 = min((blk + 1) * GAIL_LOSS_ROWS, 2 * a.batch);
  for (int r = blk * GAIL_LOSS_ROWS; r < r1; ++r) {
    const GailRowDiag o = gail_loss_row(a, r, n_e);
    for (int k = 0; k < GAIL_DIAG; ++k) s[k] += o.d[k];
  }
  if (cur < GRL_GAIL_MAX_UPDATES)
    for (int k = 0; k < GAIL_DIAG; ++k) a.diag[((long)cur * gridDim.x + blk) * GAIL_DIAG + k] = s[k];
  if (blk == 0) a.dev->cursor = cur + 1;
}
