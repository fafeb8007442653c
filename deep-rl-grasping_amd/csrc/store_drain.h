// store_drain.h -- 16-byte global stores whose cache policy is chosen at run time: plain, or WRITE-THROUGH (sc0 | sc1).
//
// A plain store leaves its line dirty in the XCD's L2 until the kernel boundary writes it back; a launch that ends with many
// megabytes of such lines makes its successor wait for that write-back.  A write-through store sends the bytes on while the
// launch is still computing, and the boundary finds nothing to flush.  The arithmetic is untouched: only the moment at which the
// bytes leave the L2 moves.  For tensors that a LATER launch reads, written as whole 128-byte lines by 16-byte stores (narrower
// write-through stores are one fabric write each and cost 3 - 12x per byte: those stay plain).
//
// GRL_TUNE store_drain=<mask> (engine.hip, README "Switches") selects the tensor groups of the SAC CNN plan that are stored this
// way; plan_sac.inl hands each kernel its bits.  The data-parallel exchange uses the same instruction for another reason (a
// store that another GPU may read while kernels are running): st_sys_quad.
#pragma once
#ifdef GRL_HOSTEMU
#include "hostemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

namespace grl {

// bits of GRL_TUNE store_drain
enum StoreDrain {
  SD_A12 = 1,       // layer-1 / layer-2 activations of the forward stack
  SD_A3 = 2,        // layer-3 activations (per-layer route only: the stack's 4-byte strided store stays plain)
  SD_G12 = 4,       // g2 (conv3_bwd) and g1 (conv2_bwd)
  SD_SLABS = 8,     // split-reduction slabs of the weight gradients (wgrad_conv and the dense riders of conv3_bwd)
  SD_IMAGES = 16,   // the next update's images, gathered by the riders of the head launch
  // (32: Adam moments, 64: parameters + Polyak targets -- no gain and a register cost in the reduction
  //  launch when compiled in, DESIGN.md 8: not built, the bits are ignored)
  SD_ALL = 31,
  SD_DEFAULT = SD_A12 | SD_G12 | SD_SLABS | SD_IMAGES     // profiles/r08_ab_store_drain.txt
};
// no group's buffer may reach this many bytes (32-bit byte offsets of the buffer instruction; plan_sac.inl checks the batch)
enum : int64_t { SD_MAX_BYTES = (int64_t)1 << 31 };

#ifdef GRL_HOSTEMU
static inline void st_quad_policy(float* base, int64_t ofs, const float (&v)[4], int drain) {
  (void)drain;
  for (int k = 0; k < 4; ++k) base[ofs + k] = v[k];
}
static inline void st_sys_quad(float* base, int64_t quad, const float (&v)[4]) { st_quad_policy(base, 4 * quad, v, 1); }
#else
typedef float sd_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sys_rsrc(const float* p) {
  const uint64_t a = (uint64_t)p;     // (made provably wave-uniform: no waterfall loop around the buffer instructions)
  const uint32_t lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)a), hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, 0x7fffffff, 0x00020000);
}
enum { SYS_SCOPE = 1 | 16 };     // buffer-instruction cache policy: sc0 | sc1
// v -> base[ofs .. ofs + 3] (floats; 16-byte aligned).  `base` and `drain` MUST be the same in every lane of the wave (a kernel
// argument, a descriptor field, a workgroup's tile origin) and ofs * 4 below SD_MAX_BYTES: the lanes differ in `ofs` only.
__device__ __forceinline__ void st_quad_policy(float* base, int64_t ofs, sd_f4 v, int drain) {
  typedef unsigned int sd_u4 __attribute__((ext_vector_type(4)));
  if (drain) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(sd_u4, v), sys_rsrc(base), (int)(ofs << 2), 0, SYS_SCOPE);
  else *(__attribute__((address_space(1))) sd_f4*)(base + ofs) = v;
}
__device__ __forceinline__ void st_sys_quad(float* base, int64_t quad, const float (&v)[4]) {
  st_quad_policy(base, 4 * quad, sd_f4{v[0], v[1], v[2], v[3]}, 1);
}
#endif

}  // namespace grl
