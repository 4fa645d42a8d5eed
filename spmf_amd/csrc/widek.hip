// widek.hip -- the sparse passes for latent dimensions above 64 (KP = 128, 256; gfx950, wave64).
//
// The reference's `latent_dim` defaults to `feature_dim` (poisson.py:103-104) and its own harness
// runs P = 50 (tests/spmf_test.py:21); the named configurations stop at K = 64, which is what the
// lane-group kernels of row_pass.hip / col_pass.hip are shaped for (a factor row = KP/4 lanes x
// float4, 64/(KP/4) stored entries per wave instruction).  Above that a factor row is still KP/4
// lanes x float4, which is the whole wave at KP = 256 and half of it at KP = 128: a wave holds
// NH = 256/KP row groups, one wave instruction gathers NH stored entries' rows as contiguous
// 4*KP-byte reads (group h takes entries e0 + NH*j + h), dot products fold over a group's lanes,
// and the per-entry scalar work (rate, log, reciprocal) is uniform inside a group.  The groups'
// partial sums meet through one cross-half exchange per row / item (xhalf_add; nothing at NH = 1).
// (KP = 128 as 64 lanes x float2 moves half the bytes per gather instruction: 0.76 against 0.5x ms
// per row pass on C2's matrix.)  Same algebra, same outputs, same accumulator layout as the
// lane-group kernels:
//
//   row_widek_kernel   z_b = xi_b sum_d x A'_d ; r = <z_b, V'_d> + phi_d ; sum x log r ;
//                      gz_b = sum_d (x/r) V'_d - veta - z_b ; fp64 scalars     (poisson.py:640-649,174-183)
//   col_widek_kernel   gV'_d += (x/r) z_b ; gA'_d += x xi_b gz_b ; gphi_d += x/r over the
//                      panel-CSC work items, float atomics; block 0 packs the row pass's fp64
//                      scalars into the accumulator tail
//
// Scope: Poisson likelihood with the linear decoder (likelihood code 0), modes 0 (full) and 1
// (encode only), canonical (col, val) / (pc_row, pc_val) entry arrays.  The log_transform /
// Bernoulli / mixed contexts and the deterministic mode stay at K <= 64 (spmf_ctx_create and
// spmf_ctx_set_deterministic say so).  Four gather instructions are in flight per wave.  This is the
// general form, not a tuned one: 2*KP*4 bytes gathered per stored entry and pass at the rate a
// wave-per-row loop reaches (C2's matrix: 6 - 11 TB/s against 16 for the lane-group kernels at K = 64, profiles/r05_widek_probe.txt).
#include "common.h"
#include "kernels.h"

namespace spmf {

namespace {

constexpr int kInFlight = 4;   // gather instructions issued back to back

__device__ __forceinline__ float4 ld4(const float* __restrict__ base, int row, int KP, int sub) {
  return *reinterpret_cast<const float4*>(base + (size_t)row * KP + sub * 4);
}
// <a, b> over the KP values of my row group, in every lane of the group.  Each KP keeps the association it has
// always summed in (z and every per-item partial sum are reproducible to the bit): q ascending and a butterfly
// over the wave at NH = 1, dot4 and the DPP fold of a half at NH = 2.
template <int NH>
__device__ __forceinline__ float group_dot(float4 a, float4 b) {
  if constexpr (NH == 2) {
    const float v = group_sum<16>(dot4(a, b));
    return v + __shfl_xor(v, 16);
  } else {
    return wave_sum(fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, 0.f)))));
  }
}
// + the other half's value (NH = 1: there is no other group)
template <int NH>
__device__ __forceinline__ float xhalf_add(float v) {
  if constexpr (NH == 2) v += __shfl_xor(v, 32);
  return v;
}
template <int NH>
__device__ __forceinline__ float4 xhalf_add(float4 v) {
  return make_float4(xhalf_add<NH>(v.x), xhalf_add<NH>(v.y), xhalf_add<NH>(v.z), xhalf_add<NH>(v.w));
}

}  // namespace

template <int KP>
__global__ __launch_bounds__(256) void row_widek_kernel(
    int64_t B, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, const float* __restrict__ row_scale, const float* __restrict__ Ap,
    const float* __restrict__ Vp, const float* __restrict__ phi, const double* __restrict__ dprep,
    float* __restrict__ z, float* __restrict__ gzs, double* __restrict__ dacc, int mode, int Dcols,
    int64_t dacc_stride) {
  constexpr int NH = 256 / KP, LPG = 64 / NH;   // row groups per wave, lanes of one
  if (gridDim.y > 1) {   // S draws per launch
    const size_t sd = blockIdx.y;
    Ap += sd * (size_t)Dcols * KP;
    Vp += sd * (size_t)Dcols * KP;
    phi += sd * (size_t)Dcols;
    dprep += sd * (size_t)kPrepSeg * (KP + 1);
    z += sd * (size_t)B * KP;
    gzs += sd * (size_t)B * KP;
    dacc += sd * (size_t)dacc_stride;
  }
  const bool encode_only = mode == 1;
  const int lane = threadIdx.x & 63, sub = lane % LPG, h = lane / LPG;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  float4 veta = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!encode_only)
    veta = make_float4((float)prep_sum(dprep, KP, sub * 4 + 0), (float)prep_sum(dprep, KP, sub * 4 + 1),
                       (float)prep_sum(dprep, KP, sub * 4 + 2), (float)prep_sum(dprep, KP, sub * 4 + 3));
  double ll_acc = 0.0, zsq_acc = 0.0, nnf_acc = 0.0;   // per lane: ll / nnf of this group's cells, zsq of group 0's k
  float4 zsum = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t b = wave; b < B; b += nwaves) {
    const int start = row_ptr[b], end = row_ptr[b + 1];
    const float xi = row_scale ? row_scale[b] : 1.f;
    // ---- sweep 1: z_b ---------------------------------------------------------------
    float4 zacc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = start; base < end; base += 64) {
      const int i = base + lane;
      const int c = i < end ? col[i] : 0;         // (slots behind the row's end: row 0, weight 0)
      const float x = i < end ? val[i] : 0.f;
      const int cnt = min(64, end - base);
      for (int e0 = 0; e0 < cnt; e0 += NH * kInFlight) {
        float4 a[kInFlight];
        float xe[kInFlight];
#pragma unroll
        for (int j = 0; j < kInFlight; ++j) {
          const int idx = e0 + NH * j + h, src = min(idx, 63);
          const int cj = __shfl(c, src);
          // (idx < cnt is wave-uniform at NH = 1 only: there the broadcast is skipped with it, which keeps that
          //  kernel's registers below its occupancy step; the halves of NH = 2 disagree about it, and a
          //  broadcast must not sit under a divergent condition)
          const float xs = (NH == 2 || idx < cnt) ? __shfl(x, src) : 0.f;
          xe[j] = idx < cnt ? xs : 0.f;
          a[j] = ld4(Ap, cj, KP, sub);
        }
#pragma unroll
        for (int j = 0; j < kInFlight; ++j) zacc = fma4(xe[j], a[j], zacc);
      }
    }
    zacc = xhalf_add<NH>(zacc);
    zacc.x *= xi; zacc.y *= xi; zacc.z *= xi; zacc.w *= xi;
    if (h == 0) reinterpret_cast<float4*>(z + (size_t)b * KP)[sub] = zacc;
    if (encode_only) continue;
    // ---- sweep 2: rates, log-likelihood, gz_b -------------------------------------
    float4 gz = make_float4(0.f, 0.f, 0.f, 0.f);
    float llrow = 0.f;
    for (int base = start; base < end; base += 64) {
      const int i = base + lane;
      const int c = i < end ? col[i] : 0;
      const float x = i < end ? val[i] : 0.f;
      const int cnt = min(64, end - base);
      for (int e0 = 0; e0 < cnt; e0 += NH * kInFlight) {
        float4 vv[kInFlight];
        float xe[kInFlight], ph[kInFlight];
#pragma unroll
        for (int j = 0; j < kInFlight; ++j) {
          const int idx = e0 + NH * j + h, src = min(idx, 63);
          const int cj = __shfl(c, src);
          const float xs = (NH == 2 || idx < cnt) ? __shfl(x, src) : 0.f;
          xe[j] = idx < cnt ? xs : 0.f;
          vv[j] = ld4(Vp, cj, KP, sub);
          ph[j] = phi[cj];
        }
#pragma unroll
        for (int j = 0; j < kInFlight; ++j) {
          const float r = group_dot<NH>(zacc, vv[j]) + ph[j];
          const bool on = xe[j] > 0.f, good = r > 0.f && r < INFINITY;   // uniform inside a group
          // (a cell with a non-positive rate: counted, weight +1 against the closed-form -1 -- row_pass.hip sweep2)
          const float cc = on ? (good ? xe[j] * __builtin_amdgcn_rcpf(r) : 1.f) : 0.f;
          if (on && good) llrow = fmaf(xe[j], logf(r), llrow);
          if (on && !good) nnf_acc += 1.0;
          gz = fma4(cc, vv[j], gz);
        }
      }
    }
    gz = xhalf_add<NH>(gz);
    if (h == 0) {
      float4 o;
      o.x = xi * (gz.x - veta.x - zacc.x);
      o.y = xi * (gz.y - veta.y - zacc.y);
      o.z = xi * (gz.z - veta.z - zacc.z);
      o.w = xi * (gz.w - veta.w - zacc.w);
      reinterpret_cast<float4*>(gzs + (size_t)b * KP)[sub] = o;
      if constexpr (NH == 2) {
        zsq_acc += (double)dot4(zacc, zacc);
      } else {   // (the association KP = 256 has always had: four squares, each added in fp64)
        zsq_acc += (double)(zacc.x * zacc.x);
        zsq_acc += (double)(zacc.y * zacc.y);
        zsq_acc += (double)(zacc.z * zacc.z);
        zsq_acc += (double)(zacc.w * zacc.w);
      }
      zsum = add4(zsum, zacc);
    }
    ll_acc += (double)llrow;
  }
  if (encode_only) return;
  // ---- one set of fp64 atomics per wave, into one of the kDaccRep replicas of the scalar block ----
  dacc += (size_t)(blockIdx.x % kDaccRep) * (kDaccHead + KP);
  // ll / nnf: every lane of a group carries that group's sum -- the lanes with sub == 0 hold the groups' values
  const double zq = wave_sum(zsq_acc);
  if (sub == 0) {
    atomicAdd(&dacc[0], ll_acc);
    if (nnf_acc != 0.0) atomicAdd(&dacc[2], nnf_acc);
  }
  if (lane == 0) atomicAdd(&dacc[1], zq);
  if (h == 0) {
    atomicAdd(&dacc[kDaccHead + sub * 4 + 0], (double)zsum.x);
    atomicAdd(&dacc[kDaccHead + sub * 4 + 1], (double)zsum.y);
    atomicAdd(&dacc[kDaccHead + sub * 4 + 2], (double)zsum.z);
    atomicAdd(&dacc[kDaccHead + sub * 4 + 3], (double)zsum.w);
  }
}

template <int KP>
__global__ __launch_bounds__(256) void col_widek_kernel(
    int D, int n_panels, int row_base, int blocks_per_panel, const int32_t* __restrict__ item_ptr,
    const int4* __restrict__ items, const int32_t* __restrict__ pc_row, const float* __restrict__ pc_val,
    const float* __restrict__ Vp, const float* __restrict__ phi, const float* __restrict__ z,
    const float* __restrict__ gzs, float* __restrict__ gAp, float* __restrict__ gVp, float* __restrict__ gphi,
    const int32_t* __restrict__ item_mid, int half_sel, int64_t Brows, int64_t acc_stride,
    const double* __restrict__ pack_dacc, float* __restrict__ pack_tail, int64_t dacc_stride) {
  constexpr int NH = 256 / KP, LPG = 64 / NH;
  if (pack_dacc && blockIdx.x == 0) {
    // the row pass's fp64 scalars -> (hi, lo) float pairs in the accumulator tail (col_pass.hip pack_block)
    const double* dacc = pack_dacc + (size_t)blockIdx.y * dacc_stride;
    float* tail = pack_tail + (size_t)blockIdx.y * acc_stride;
    for (int i = threadIdx.x; i < kDaccHead + KP; i += blockDim.x) fold_dacc(i, dacc, tail, KP);
    return;
  }
  if (gridDim.y > 1) {   // S draws per launch
    const size_t sd = blockIdx.y;
    Vp += sd * (size_t)D * KP;
    phi += sd * (size_t)D;
    z += sd * (size_t)Brows * KP;
    gzs += sd * (size_t)Brows * KP;
    gAp += sd * (size_t)acc_stride;
    gVp += sd * (size_t)acc_stride;
    gphi += sd * (size_t)acc_stride;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, sub = lane % LPG, h = lane / LPG;
  const int64_t L = (int64_t)blockIdx.x - (pack_dacc ? 1 : 0);
  const int p = (int)(L / blocks_per_panel), ib = (int)(L % blocks_per_panel);
  if (p >= n_panels) return;
  const int ilo = half_sel == 2 ? item_mid[p] : item_ptr[p];
  const int ihi = half_sel == 1 ? item_mid[p] : item_ptr[p + 1];
  const int it = ilo + ib * 4 + wid;               // one work item per wave
  if (it >= ihi) return;                            // wave-uniform
  const int4 im = items[it];
  const int d = im.z;
  const float4 vp = ld4(Vp, d, KP, sub);
  const float ph = phi[d];
  float4 gV = make_float4(0.f, 0.f, 0.f, 0.f), gA = gV;
  float gph = 0.f;
  const int end = im.x + im.y;
  for (int base = im.x; base < end; base += 64) {
    const int i = base + lane;
    const int rb = i < end ? pc_row[i] - row_base : 0;   // (slots behind the item's end: row 0, weight 0)
    const float x = i < end ? pc_val[i] : 0.f;
    const int cnt = min(64, end - base);
    for (int e0 = 0; e0 < cnt; e0 += NH * kInFlight) {
      float4 zz[kInFlight], gg[kInFlight];
      float xe[kInFlight];
#pragma unroll
      for (int j = 0; j < kInFlight; ++j) {
        const int idx = e0 + NH * j + h, src = min(idx, 63);
        const int b = __shfl(rb, src);
        const float xs = (NH == 2 || idx < cnt) ? __shfl(x, src) : 0.f;   // (as in the row kernel)
        xe[j] = idx < cnt ? xs : 0.f;
        zz[j] = ld4(z, b, KP, sub);
        gg[j] = ld4(gzs, b, KP, sub);
      }
#pragma unroll
      for (int j = 0; j < kInFlight; ++j) {
        const float r = group_dot<NH>(zz[j], vp) + ph;
        // (col_pass.hip: a cell the row pass counted as non-finite gets weight +1; padded slots stay weightless)
        const float xr = (r > 0.f && r < INFINITY) ? xe[j] * __builtin_amdgcn_rcpf(r) : (xe[j] > 0.f ? 1.f : 0.f);
        gV = fma4(xr, zz[j], gV);
        gA = fma4(xe[j], gg[j], gA);
        gph += xr;
      }
    }
  }
  gV = xhalf_add<NH>(gV);
  gA = xhalf_add<NH>(gA);
  gph = xhalf_add<NH>(gph);
  if (h == 0) {
    float* dv = gVp + (size_t)d * KP + sub * 4;
    float* da = gAp + (size_t)d * KP + sub * 4;
    if (gV.x != 0.f) atomicAdd(dv + 0, gV.x);
    if (gV.y != 0.f) atomicAdd(dv + 1, gV.y);
    if (gV.z != 0.f) atomicAdd(dv + 2, gV.z);
    if (gV.w != 0.f) atomicAdd(dv + 3, gV.w);
    if (gA.x != 0.f) atomicAdd(da + 0, gA.x);
    if (gA.y != 0.f) atomicAdd(da + 1, gA.y);
    if (gA.z != 0.f) atomicAdd(da + 2, gA.z);
    if (gA.w != 0.f) atomicAdd(da + 3, gA.w);
    if (lane == 0 && gph != 0.f) atomicAdd(&gphi[d], gph);
  }
}

namespace {
template <int KP>
void row_widek(int nb, const RowArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((row_widek_kernel<KP>), dim3(nb, a.S > 1 ? a.S : 1), dim3(256), 0, st, a.B, a.row_ptr, a.col,
                     a.val, a.row_scale, a.Ap, a.Vp, a.phi, a.dprep, a.z, a.gzs, a.dacc, a.mode, a.D,
                     a.dacc_stride);
}
template <int KP>
void col_widek(int64_t nb, int bpp, const ColArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((col_widek_kernel<KP>), dim3((unsigned)nb, a.S > 1 ? a.S : 1), dim3(256), 0, st, a.D,
                     a.n_panels, a.row_base, bpp, a.item_ptr, reinterpret_cast<const int4*>(a.items), a.pc_row,
                     a.pc_val, a.Vp, a.phi, a.z, a.gzs, a.gAp, a.gVp, a.gphi, a.item_mid, a.half_sel, a.B,
                     a.acc_stride, a.pack_dacc, a.pack_tail, a.dacc_stride);
}
}  // namespace

// false: not a shape this file covers (nothing launched)
bool launch_row_widek(int KP, const RowArgs& a, hipStream_t st) {
  if (a.logt != 0 || (a.mode != 0 && a.mode != 1) || a.det_slots) return false;
  const int64_t want = (a.B + 3) / 4;
  const int nb = (int)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
  return with_kp<256, 128>(KP, [&](auto kp) { row_widek<decltype(kp)::value>(nb, a, st); });
}

bool launch_col_widek(int KP, const ColArgs& a, hipStream_t st) {
  if (a.logt != 0 || a.det_part) return false;
  const int bpp = (a.max_items_per_panel + 3) / 4;
  if (bpp < 1) return false;
  const int64_t nb = (int64_t)a.n_panels * bpp + (a.pack_dacc ? 1 : 0);
  return with_kp<256, 128>(KP, [&](auto kp) { col_widek<decltype(kp)::value>(nb, bpp, a, st); });
}

}  // namespace spmf
