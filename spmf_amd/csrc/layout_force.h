// layout_force.h -- device only: what graph_layout.hip and graph_transform.hip share, so that umap_transform stays
// the continuation of umap bit for bit: the row groups' shape, the force of one entry and of one negative, and the
// draw of a negative.  Each kernel keeps its own walk (a list per epoch / neighbours in registers), its own domain
// tag of the draws and its own rule for which drawn row counts.
#pragma once
#include "common.h"
#include "philox.h"

namespace spmf {

namespace {

constexpr int kRowLanes = 16;                              // lanes of the group that owns a row
constexpr int kRowsPerBlock = 256 / kRowLanes;

__device__ __forceinline__ bool finite2(float2 v) { return isfinite(v.x) && isfinite(v.y); }
// clamp to [-4, 4]; fmaxf / fminf return the other operand for a NaN (0 * inf of an overflowed distance)
__device__ __forceinline__ float clip4(float v) { return fminf(fmaxf(v, -4.f), 4.f); }

// a * d2^b for d2 > 0, capped where q / (1 + q) is 1 in fp32 anyway: an overflowed power stays out of inf / inf
__device__ __forceinline__ float a_pow_b(float a, float b, float d2) {
  return fminf(a * exp2f(b * log2f(d2)), 0x1p+60f);
}

// The attraction of yi towards yj along an entry of weight w, onto (fx, fy); nothing at distance 0.
__device__ __forceinline__ void attract(float2 yi, float2 yj, float w, float a, float b, float neg2b, float& fx,
                                        float& fy) {
  const float dx = yi.x - yj.x, dy = yi.y - yj.y;
  const float d2 = fmaf(dx, dx, dy * dy);
  if (d2 > 0.f) {
    const float q = a_pow_b(a, b, d2);
    const float c = neg2b * q / (d2 * (1.f + q));             // -2ab d2^(b-1) / (1 + a d2^b)
    fx = fmaf(w, clip4(c * dx), fx);
    fy = fmaf(w, clip4(c * dy), fy);
  }
}

// The repulsion of yi from the negative yr, onto (gx, gy); nothing at distance 0.
__device__ __forceinline__ void repel(float2 yi, float2 yr, float a, float b, float two_gamma_b, float& gx,
                                      float& gy) {
  const float dx = yi.x - yr.x, dy = yi.y - yr.y;
  const float d2 = fmaf(dx, dx, dy * dy);
  if (d2 > 0.f) {
    const float q = a_pow_b(a, b, d2);
    const float c = two_gamma_b / ((0.001f + d2) * (1.f + q));
    gx += clip4(c * dx);
    gy += clip4(c * dy);
  }
}

// Negative m of row `row32` in `epoch`: a row below n32, word m & 3 of the Philox block (row32, m >> 2, epoch, tag)
__device__ __forceinline__ uint32_t negative_row(uint32_t row32, int m, int epoch, uint32_t tag, uint32_t seed_lo,
                                                 uint32_t seed_hi, uint32_t n32) {
  const uint4 r4 = philox4x32_10(make_uint4(row32, (uint32_t)(m >> 2), (uint32_t)epoch, tag),
                                 make_uint2(seed_lo, seed_hi));
  const int k = m & 3;
  const uint32_t word = k == 0 ? r4.x : k == 1 ? r4.y : k == 2 ? r4.z : r4.w;
  return __umulhi(word, n32);
}

}  // namespace

}  // namespace spmf
