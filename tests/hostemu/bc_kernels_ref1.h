// bc_kernels_ref1.h -- TEST-ONLY sequential form of what the wavefront of csrc/bc_kernels.h's closing launch does together,
// included by that header ONLY in the g++ emulation build (-DGRL_HOSTEMU -I tests/hostemu, tests/conftest.py).  Never part of
// libgrl.so.  No include guard: it is pasted once, inside namespace grl.
//
// The emulation runs the lanes of a workgroup one after the other, so nothing can meet in a cross-lane exchange.  Lane 0 forms
// the 64 per-lane sums in row order and then adds them in the order of the HIP form's exchange (distances 32, 16, .. 1); the
// other lanes return 0 and leave the kernel at its `threadIdx.x != 0` test.  The gather, the loss launch and Adam are
// lane-local: the emulation runs the header's own code.
inline float bc_rows_sum(const float* row_loss, int batch) {
  if (threadIdx.x != 0) return 0.f;
  float lane[64];
  for (int t = 0; t < 64; ++t) {
    float s = 0.f;
    for (int b = t; b < batch; b += 64) s += row_loss[b];
    lane[t] = s;
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int t = 0; t < off; ++t) lane[t] += lane[t + off];
  return lane[0];
}
