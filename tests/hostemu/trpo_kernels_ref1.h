// trpo_kernels_ref1.h -- TEST-ONLY sequential forms of what a workgroup of csrc/trpo_kernels.h does together, included by that
// header ONLY in the g++ emulation build (-DGRL_HOSTEMU -I tests/hostemu, tests/conftest.py).  Never part of libgrl.so.  No
// include guard: it is pasted once, inside namespace grl.
//
// The emulation runs the lanes of a workgroup one after the other, so nothing can meet in LDS.  The kernels whose lanes share a
// range of elements (advantage standardisation, the dot products and vector updates of conjugate gradient) are written once in
// the header over TRPO_LANES / trpo_block_sum: here ONE lane walks the whole range in element order and the "block sum" is its
// own sum.  The loss launch, whose HIP form adds over a wavefront, is restated as a plain loop over the rows of the block.  The
// row-local arithmetic (trpo_loss_row / trpo_loss_row_j) and the single-lane scalar kernel are the header's own.
#define TRPO_LANES(t, nt)      \
  if (threadIdx.x != 0) return; \
  const int t = 0, nt = 1
inline float trpo_block_sum(float v) { return v; }
inline float trpo_block_max(float v) { return v; }

inline void trpo_loss_kernel(TrpoLossArgs a) {
  if (threadIdx.x != 0) return;
  if (a.mode && (a.dev->ls_accepted || a.dev->zero_grad)) return;
  const int blk = blockIdx.x;
  float dls[PPO_MAX_A] = {0.f}, s0 = 0.f, s1 = 0.f;
  const int b1 = min((blk + 1) * TRPO_ROWS, a.T);
  for (int b = blk * TRPO_ROWS; b < b1; ++b) {
    const TrpoRow r = trpo_loss_row(a, b);
    if (!a.mode)
      for (int j = 0; j < a.A; ++j) dls[j] += trpo_loss_row_j(a, b, j, r.w);
    s0 += r.surr; s1 += r.kl;
  }
  a.part[(long)blk * 2] = s0; a.part[(long)blk * 2 + 1] = s1;
  if (a.mode) return;
  for (int j = 0; j < a.A; ++j) a.dls_slab[(long)blk * a.A + j] = blk == 0 ? dls[j] + a.ent_coef : dls[j];
  if (blk == 0)
    for (int j = 0; j < a.A; ++j) a.logstd_old[j] = a.logstd[j];
}
