// philox.h -- device only: the counter-based generator of the kernels that draw on the device (surrogate.hip:
// the base noise of the surrogate; layout_force.h: the negative samples of an epoch of graph_layout.hip and
// graph_transform.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spmf {

// Philox4x32-10 (Salmon et al., SC'11): ten rounds on the counter c under the key k, the key advanced by the
// Weyl constants between the rounds.  A pure function of (c, k): who draws what is the caller's counter layout.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += 0x9E3779B9u;
    k.y += 0xBB67AE85u;
  }
  return c;
}

}  // namespace spmf
