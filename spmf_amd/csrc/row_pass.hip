// row_pass.hip -- row-resident fused forward of the sparse Poisson energy
// (gfx950, wave64).
//
// Per stored row b of the batch (one wavefront per row, rows grid-strided):
//   sweep 1  z_b   = xi_b * sum_{d in nnz(b)} x_bd A'_d          encode,
//                                               poisson.py:640-649
//   sweep 2  r_bd  = <z_b, V'_d> + phi_d                          :174-177
//            ll   += x_bd log r_bd   (lgamma(x+1) is parameter free and is
//                                     pre-summed per batch)       :178-183
//            gz_b  = sum_d (x_bd/r_bd) V'_d - veta - z_b          d(x+z)/dz_b
//   out      z_b, xi_b*gz_b (the column pass needs exactly that product),
//            fp64: sum x log r, sum z^2, sum_b z_b, #non-finite cells.
//
// Lane layout: a gathered factor row is KP floats = LPN=KP/4 lanes x float4,
// so one wave instruction serves NPI=64/LPN stored entries; the LPN lanes of
// an entry fold their partial dot products with DPP adds.  The transcendental
// part (log, divide) runs once per 64 entries with one entry per lane: lane
// (grp,sub) keeps the dot product of iteration `sub`.  col/val are read as
// one coalesced 256-B wave load per 64 entries and distributed by
// ds_bpermute.  Gathers are issued in straight-line groups of up to four
// (padded entries ask for a row behind the table: dropped by the buffer range
// check, common.h GTable) so several L2 round trips are in
// flight per wave; rows of <= 128 entries keep col/val in registers for both
// sweeps.
//
// Short rows at K <= 32: only a row's LAST chunk can be partly filled, so the
// chunk in front of it is straight-line code over all LPN gather instructions,
// and the last chunk is dispatched ONCE per sweep, by a wave-uniform switch, to
// the arm for the T = ceil(entries / NPI) instructions that carry entries: T
// gathers, dot products and back-substitutions, no per-group guard and no padded
// instruction (RowCtx::sweep1_last / sweep2_last; DESIGN.md section 4 and
// profiles/r07_row_dispatch_ab.txt).  Long rows (> 128 entries) and K = 64 keep
// the guarded groups of four (RowCtx::sweep1 / sweep2).
//
// Stream loads: the entry words of the next row, the row pointers of the one
// after it and the dynamic tail's counter are asked for at ONE point of a row,
// behind its last gathers (issue_next in the row loop: why, and what it
// measured, is written there and in profiles/r06_stream_issue_ab.txt).
//
// Roofline: HBM traffic is 8 B per stored entry (+ an L2-served re-read for
// long rows) + 8*KP B per row written; the factor-row gathers (2 x 4*KP B per
// entry) are served by L2/Infinity Cache because A' and V' (D*KP*4 B each)
// stay resident.  Algorithmic bytes: DESIGN.md section 4.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "row_prefetch.h"

namespace spmf {

#ifndef ROW_MAX_BLOCKS
#define ROW_MAX_BLOCKS 4096
#endif
// share of a wave's rows that the counters hand out (the dynamic tail of the row loop, below)
#ifndef ROW_DYN_NUM
#define ROW_DYN_NUM 1
#define ROW_DYN_DEN 8
#endif
static_assert(ROW_MAX_BLOCKS <= spmf::kDetMaxBlocks,
              "the deterministic mode's per-workgroup slots (common.h kDetMaxBlocks) are sized for at most that many row-pass workgroups");
#ifndef ROW_GRP
#define ROW_GRP 4
#endif
#ifndef ROW_WAVES_PER_SIMD
#define ROW_WAVES_PER_SIMD 1
#endif
// The warm-up of a coming row's entry lines by scalar loads (issue_next in the row loop, K <= 32): 0 = none,
// L = 1 or 2 = the row whose vector load is L rows away.  (ROW_PREFETCH_WORDS, row_prefetch.h: words between two loads.)
#ifndef ROW_PREFETCH
#define ROW_PREFETCH 1
#endif
static_assert(ROW_PREFETCH >= 0 && ROW_PREFETCH <= 2, "ROW_PREFETCH: 0, or a lead of 1 or 2 rows");

namespace {

// The intercept phi_d is needed once per stored entry ("one entry per lane": 64 different
// cache lines per wave load).  tools/gather_rows_probe.hip: that third gather stream costs
// the row pass 0.35 ms of 1.9 on C3 (mode 6 vs mode 2); staged in LDS once per workgroup
// (4*D bytes, 80 KB at D = 20 000, two 512-thread workgroups per CU) it costs 0.1.
__device__ __forceinline__ float* lds_dyn() {
  extern __shared__ __attribute__((aligned(16))) float spmf_row_lds[];
  return spmf_row_lds;
}

// One stored entry: from the packed stream (col << 16 | count: half the bytes) when the batch
// carries one, from the canonical col / val arrays otherwise.  PACKED is a template parameter of the
// kernel (the resident-set launches have both forms).  load_entry only LOADS (into the row loop's pipeline registers, at its issue point);
// unpack_entry turns them into (column, count) where they are used, one row later -- arithmetic
// on the loaded word right away would put the wait for that load in front of it.
// FMT 0: canonical (col, val).  FMT 1: packed word.
//
// The entries of ONE row as a buffer (EntryRow: base = the row's first entry, size = its length; start and n are
// wave-uniform), so that every lane loads on every path: a lane behind the row's end is dropped by the address
// unit's range check (no memory operation; it returns 0), and unpack_entry, which is given the lane's `ok`,
// puts the padding entry in its place.  A load under a lane predicate is a branch on the exec mask instead, and
// behind the join of two paths that issued different numbers of loads the compiler waits for the longer count.
template <int FMT>
struct EntryRow {
  __amdgpu_buffer_rsrc_t a, b;
};
template <int FMT>
__device__ __forceinline__ EntryRow<FMT> entry_row(const int32_t* __restrict__ col, const float* __restrict__ val,
                                                   const uint32_t* __restrict__ ent, int start, int n) {
  EntryRow<FMT> r;
  start = __builtin_amdgcn_readfirstlane(start);
  n = __builtin_amdgcn_readfirstlane(n);
  if (FMT == 1) {
    r.a = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(ent + start), 0, n * 4, 0x00020000);
    r.b = r.a;
  } else {
    r.a = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(col + start), 0, n * 4, 0x00020000);
    r.b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(val + start), 0, n * 4, 0x00020000);
  }
  return r;
}
// entry i of the row (NT: read once, the non-temporal hint)
template <int FMT, bool NT>
__device__ __forceinline__ void load_entry(const EntryRow<FMT>& r, int i, int& ra, float& rb) {
  constexpr int AUX = NT ? 2 : 0;
  ra = (int)__builtin_amdgcn_raw_buffer_load_b32(r.a, i * 4, 0, AUX);
  rb = FMT == 1 ? 0.f : __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r.b, i * 4, 0, AUX));
}
template <int FMT>
__device__ __forceinline__ void unpack_entry(int ra, float rb, bool ok, int& c, float& x) {
  if (FMT == 1) {
    const uint32_t w = ok ? (uint32_t)ra : kPadWord;
    c = (int)(w >> 16);
    x = (float)(w & 0xffffu);
  } else {
    c = ok ? ra : kPadRow;
    x = ok ? rb : 0.f;
  }
}

// The warm-up of a coming row's entry lines: one word of every 64-byte half line that the first 128 entry words of the
// row span (which words: row_warm_word, row_prefetch.h), read through the constant address space from a wave-uniform
// address -- scalar loads, whose path into this XCD's L2 holds no miss slot of the vector cache.  The entry arrays
// are read-only for the kernel's lifetime.  The values are dead: warm_retire keeps them until a point where the scalar
// loads of the issue point have been waited for anyway, so that no wait is added.  A row without entries reads nothing.
template <int FMT>
struct RowWarm {
  static constexpr int N = (FMT == 1 ? 1 : 2) * kRowWarmLoads;
  uint32_t w[N] = {};
};
template <int FMT>
__device__ __forceinline__ void warm_issue(RowWarm<FMT>& r, const int32_t* __restrict__ col,
                                           const float* __restrict__ val, const uint32_t* __restrict__ ent, int start,
                                           int n) {
  typedef const __attribute__((address_space(4))) uint32_t* Words;
  if (n > 0) {   // wave-uniform
#pragma unroll
    for (int i = 0; i < kRowWarmLoads; ++i) {
      const int at = start + row_warm_word(i, n);
      if (FMT == 1) {
        r.w[i] = ((Words)ent)[at];
      } else {
        r.w[i] = ((Words)col)[at];
        r.w[kRowWarmLoads + i] = ((Words)val)[at];
      }
    }
  }
}
// (`behind`: a value that is there only behind the wait that covers them -- the consumer takes it as an operand too,
//  or the optimiser moves it, and with it the wait for the scalar loads, up to the loads)
template <int FMT>
__device__ __forceinline__ void warm_retire(const RowWarm<FMT>& r, int behind) {
#pragma unroll
  for (int i = 0; i < RowWarm<FMT>::N; ++i) asm volatile("" ::"s"(r.w[i]), "v"(behind));
}

// Lane `base/4 + IMM` 's value: ds_bpermute with the compile-time part of the source lane in the instruction's
// offset field (the row pass broadcasts from lanes (g0 + j) * NPI + grp and grp * LPN + g0 + j: one base
// register per form for the whole kernel instead of a shift / add per broadcast)
// (imm_lanes is a constant after the unrolled callers are inlined.  BASE false = the __shfl form: at K = 64 the
//  sixteen base + constant sums of a chunk get hoisted into registers the kernel does not have -- 132 instead of
//  76 bytes of scratch, C4's row launches 12.7 -> 13.2 ms -- so that instantiation keeps the shift per call)
template <bool BASE>
__device__ __forceinline__ int bperm_i(int base_bytes, int imm_lanes, int v) {
  if constexpr (BASE) return __builtin_amdgcn_ds_bpermute(base_bytes + imm_lanes * 4, v);
  else return __shfl(v, (base_bytes >> 2) + imm_lanes);
}
template <bool BASE>
__device__ __forceinline__ float bperm_f(int base_bytes, int imm_lanes, float v) {
  return __int_as_float(bperm_i<BASE>(base_bytes, imm_lanes, __float_as_int(v)));
}

// LIK: 0 Poisson / linear decoder, 1 Poisson / log_transform, 2 Bernoulli(logits) / linear
// LDSPHI: phi is read from the workgroup's LDS copy instead of global memory
template <int KP, int LIK, bool LDSPHI = false>
struct RowCtx {
  static constexpr int LPN = KP / 4;
  static constexpr int NPI = 64 / LPN;
  static constexpr int GRP = LPN < ROW_GRP ? LPN : ROW_GRP;  // gathers issued back to back
  // broadcasts through a base register: K <= 32; not the exp decoder's instantiations (they have no register to
  // spare either: 12 - 20 bytes of scratch with it)
  static constexpr bool BPI = LPN <= 8 && LIK != 1;
  GTable Ap, Vp;          // the gathered tables (common.h: slots behind a row's end are dropped by the range check)
  const float* phi;
  const uint8_t* ctype;   // LIK 3 (mixed): 1 = Bernoulli column
  int lane, sub, grp;
  int bp_grp, bp_row;     // byte addresses of lanes grp and grp * LPN (bperm_i / bperm_f)

  // z partial: zacc += sum over the chunk of x * A'_d
  template <int CNT>
  __device__ __forceinline__ void s1_group(int c, float x, int g0, float4& zacc) const {
    float4 a[CNT];
    float xv[CNT];
#pragma unroll
    for (int j = 0; j < CNT; ++j) {
      const int d = bperm_i<BPI>(bp_grp, (g0 + j) * NPI, c);
      xv[j] = bperm_f<BPI>(bp_grp, (g0 + j) * NPI, x);
      a[j] = gather4<LPN>(Ap, d, sub);
    }
#pragma unroll
    for (int j = 0; j < CNT; ++j) zacc = fma4(xv[j], a[j], zacc);
  }
  // (a chunk of nchunk entries under the per-group guard: long rows, and every row at K = 64)
  __device__ __forceinline__ void sweep1(int c, float x, int nchunk, float4& zacc) const {
#pragma unroll
    for (int g0 = 0; g0 < LPN; g0 += GRP) {
      if (g0 * NPI < nchunk) s1_group<GRP>(c, x, g0, zacc);  // wave-uniform
    }
  }

  // sweep-2 pieces of one group of GRP gather instructions of which CNT carry entries (an arm, below, passes its
  // whole count with g0 = 0)
  template <int CNT>
  __device__ __forceinline__ void s2_issue(int c, int g0, float4 (&vv)[LPN]) const {
#pragma unroll
    for (int j = 0; j < CNT; ++j) {
      const int d = bperm_i<BPI>(bp_grp, (g0 + j) * NPI, c);
      vv[g0 + j] = gather4<LPN>(Vp, d, sub);
    }
  }
  template <int CNT>
  __device__ __forceinline__ void s2_dots(int g0, const float4& z, float4 (&vv)[LPN], float& rmine) const {
#pragma unroll
    for (int j = 0; j < CNT; ++j) {
      const float dot = group_sum<LPN>(dot4(z, vv[g0 + j]));
      if (sub == g0 + j) rmine = dot;
    }
#pragma unroll
    for (int j = CNT; j < GRP; ++j) vv[g0 + j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  template <int CNT>
  __device__ __forceinline__ void s2_back(float cc, int g0, const float4 (&vv)[LPN],
                                          float4& gz) const {
#pragma unroll
    for (int j = 0; j < CNT; ++j) {
      const float cb = bperm_f<BPI>(bp_row, g0 + j, cc);    // the lane of the group that owns this gather's weight
      gz = fma4(cb, vv[g0 + j], gz);
    }
  }

  // ---- short rows at K <= 32: a chunk by the number T of its gather instructions that carry entries --------------
  // Only a row's LAST chunk can be partly filled; the chunk in front of it is T = LPN.  An arm is straight-line
  // code for one T: exactly T gathers, dot products and back-substitutions, no guard and no padded instruction in
  // it (the lanes behind the row's end in instruction T - 1 are still dropped by the range check).  The row loop
  // picks the arm ONCE per sweep with a wave-uniform switch (sweep1_last / sweep2_last).

  // sweep 1 of a chunk of T gather instructions, written in groups of GRP as everywhere.  (With no guard between
  // the groups the compiler asks for a later group's rows ahead of the first group's fma where it has the registers:
  // all eight of a full chunk at K = 32.  Holding it to four in flight with a scheduling barrier measured the same.)
  template <int T>
  __device__ __forceinline__ void s1_arm(int c, float x, float4& zacc) const {
    constexpr int WHOLE = T / GRP * GRP;
#pragma unroll
    for (int g0 = 0; g0 < WHOLE; g0 += GRP) s1_group<GRP>(c, x, g0, zacc);
    if constexpr (T > WHOLE) s1_group<T - WHOLE>(c, x, WHOLE, zacc);
  }
  // sweep 2 of a chunk of T gather instructions: the chunk asks for all of its V' rows before its first dot
  // product (asking for them ahead of sweep 1 or of its cross-group sum measured slower:
  // profiles/r05_row_v_ahead_ab.txt); `behind` runs behind the gathers, before they are waited for (the row
  // loop's issue_next in a row's last chunk).  Every arm consumes all of its gathers, so the arms of a switch meet
  // with what `behind` issued in flight and nothing else, and the waits inside an arm count T - 1 ... 0 on top of it.
  // (one fold per dot product: a transpose-reduce of the chunk's eight at K = 32 and the packed multiply / fma
  //  forms both measured no faster, profiles/r05_row_valu_ab.txt)
  template <int T, class Hook, class Landed>
  __device__ __forceinline__ void s2_arm(int c, float x, int nchunk, const float4& z, float4& gz, float& ll,
                                         double& nnf, Hook&& behind, Landed&& landed) const {
    float4 vv[LPN];
    float rmine = 0.f;
    s2_issue<T>(c, 0, vv);
    behind();
    if constexpr (T > 0) {
#pragma unroll
      for (int j = 0; j < T; ++j) {
        const float dot = group_sum<LPN>(dot4(z, vv[j]));
        if (sub == j) rmine = dot;
      }
      s2_cells<T>(c, x, nchunk, rmine, vv, gz, ll, nnf, landed);
    } else {
      landed(0);
    }
  }
  // f(integral constant T) for the wave-uniform t in 0 ... LPN
  template <class F>
  __device__ __forceinline__ static void by_count(int t, F&& f) {
    static_assert(LPN <= 8, "the arms are written out up to eight gather instructions per chunk");
#define SPMF_ROW_ARM(T_)                                            \
  case T_:                                                          \
    if constexpr (LPN >= T_) f(std::integral_constant<int, T_>{});  \
    break;
    switch (t) {
      SPMF_ROW_ARM(1) SPMF_ROW_ARM(2) SPMF_ROW_ARM(3) SPMF_ROW_ARM(4)
      SPMF_ROW_ARM(5) SPMF_ROW_ARM(6) SPMF_ROW_ARM(7) SPMF_ROW_ARM(8)
      default: f(std::integral_constant<int, 0>{}); break;   // an empty row
    }
#undef SPMF_ROW_ARM
  }
  // the number of gather instructions that carry entries of a chunk of n (wave-uniform)
  __device__ __forceinline__ static int count_of(int n) { return (int)((unsigned)(n + NPI - 1) / (unsigned)NPI); }
  __device__ __forceinline__ void sweep1_last(int c, float x, int nlast, float4& zacc) const {
    by_count(count_of(nlast), [&](auto t) __attribute__((always_inline)) {
      constexpr int T = decltype(t)::value;
      if constexpr (T > 0) s1_arm<T>(c, x, zacc);
    });
  }
  template <class Hook, class Landed>
  __device__ __forceinline__ void sweep2_last(int c, float x, int nlast, const float4& z, float4& gz, float& ll,
                                              double& nnf, Hook&& behind, Landed&& landed) const {
    by_count(count_of(nlast), [&](auto t) __attribute__((always_inline)) {
      s2_arm<decltype(t)::value>(c, x, nlast, z, gz, ll, nnf, behind, landed);
    });
  }

  // rates, log-likelihood and gz partial over one chunk, group by group under the per-group guard (long rows, and
  // every row at K = 64); `behind_last` runs behind the gathers of the chunk's last group, before they are waited
  // for (the row loop's issue_next in a long row's last chunk); `landed`: s2_cells
  template <class Hook, class Landed>
  __device__ __forceinline__ void sweep2(int c, float x, int nchunk, const float4& z, float4& gz, float& ll,
                                         double& nnf, Hook&& behind_last, Landed&& landed) const {
    float4 vv[LPN];
    float rmine = 0.f;
#pragma unroll
    for (int g0 = 0; g0 < LPN; g0 += GRP) {
      const bool occ = g0 * NPI < nchunk;                                     // wave-uniform
      if (occ) s2_issue<GRP>(c, g0, vv);
      if (g0 + GRP >= LPN) behind_last();
      if (occ) s2_dots<GRP>(g0, z, vv, rmine);
      else s2_dots<0>(g0, z, vv, rmine);
    }
    s2_cells(c, x, nchunk, rmine, vv, gz, ll, nnf, landed);
  }
  // the per-cell part of sweep 2 (one entry per lane) and the gz partial: over the CNT gather instructions of an
  // arm, or (CNT < 0, K = 64) group by group under the per-group guard.  `landed` is given a value of the chunk's last
  // dot product and of the broadcasts below: what waits for them has waited for every scalar load of the issue
  // point as well (the row loop retires its warm-up words there)
  template <int CNT = -1, class Landed>
  __device__ __forceinline__ void s2_cells(int c, float x, int nchunk, float rmine, const float4 (&vv)[LPN],
                                           float4& gz, float& ll, double& nnf, Landed&& landed) const {
    // one entry per lane: lane (grp,sub) owns slot sub*NPI+grp
    const int slot = sub * NPI + grp;
    const float xs = __shfl(x, slot);
    const int cs = __shfl(c, slot);
    landed(__float_as_int(rmine) ^ cs);
    float cc = 0.f;
    if (slot < nchunk && xs > 0.f) {
      if (LIK == 2 || LIK == 4 || (LIK == 3 && ctype[cs])) {
        // Bernoulli(logits = f(<z,V'>) + phi) (bernoulli.py:147-155): stored-cell part x*logit;
        // LIK 4: f = exp - 1 (saturating like the Poisson form)
        float ey = 1.f;
        const float fy = LIK == 4 ? expm1_dec(fminf(rmine, kYSat), ey) : rmine;
        const float lg = fy + (LDSPHI ? lds_dyn()[cs] : phi[cs]);
        if (lg > -INFINITY && lg < INFINITY) {
          ll = fmaf(xs, lg, ll);
          cc = LIK == 4 ? xs * ey : xs;              // d(x*logit)/d<z,V'>
        } else {
          nnf += 1.0;
        }
      } else {
        // linear decoder: r = <z,V'> + phi; log_transform: r = exp(<z,V'>) - 1 + phi
        float ey = 1.f;
        const float fy = LIK == 1 ? expm1_dec(fminf(rmine, kYSat), ey) : rmine;
        const float r = fy + (LDSPHI ? lds_dyn()[cs] : phi[cs]);
        if (r > 0.f && r < INFINITY) {
          ll = fmaf(xs, logf(r), ll);
          cc = xs * ey * __builtin_amdgcn_rcpf(r);   // d(x log r)/d<z,V'>
        } else {
          // the replacement rule (poisson.py:606-616) swaps the WHOLE log-pmf of this
          // cell for min-10 (spmf_nonfinite_patch; its lgamma(x+1) is taken back out of
          // the pre-summed constant there).  Its share of the closed-form / dense "-sum
          // over all cells of r" is cancelled with weight +1 here against the -1 every
          // cell gets there.  (No lgammaf in this kernel: inlined into the hot loop it
          // cost 20 % of the pass, 1.88 -> 2.25 ms on C3.)
          nnf += 1.0;
          cc = ey;
        }
      }
    }
    if constexpr (CNT >= 0) {
      s2_back<CNT>(cc, 0, vv, gz);
    } else {
#pragma unroll
      for (int g0 = 0; g0 < LPN; g0 += GRP) {
        if (g0 * NPI < nchunk) s2_back<GRP>(cc, g0, vv, gz);
      }
    }
  }
};

}  // namespace

// BT: threads per workgroup.  256: phi from global memory.  512 / 1024: phi staged in LDS
// (4*D bytes of dynamic LDS: two workgroups per CU up to D = 20 480, one up to 40 960),
// four waves per SIMD either way.  The 256-thread form is left to the compiler, except at K = 32, where it is held
// to four waves too: those five kernels sit at 128 - 134 registers unbounded, three waves for a handful of registers
// (all five fit 128 without scratch).
// Launch contract: blockDim.x == BT (the wave number is computed from BT), and B < 2^31 -- row numbers are 32-bit
// scalars inside, although the argument is int64_t (the host admits B * KP * 4 < 4 GiB only: api_ctx.hip).
template <int KP, int LIK, int BT = 256, int PACKED = 0>
__global__ __launch_bounds__(BT, BT == 256 && KP != 32 ? ROW_WAVES_PER_SIMD : 4) void row_pass_kernel(
    int64_t B, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, const float* __restrict__ row_scale,
    const float* __restrict__ Ap, const float* __restrict__ Vp, const float* __restrict__ phi,
    const double* __restrict__ dprep, float* __restrict__ z, float* __restrict__ gzs,
    double* __restrict__ dacc, int mode, const float* __restrict__ gzd,
    const uint8_t* __restrict__ ctype, int Dcols, int64_t dacc_stride,
    const uint32_t* __restrict__ ent, double* __restrict__ det_slots, int64_t det_stride, int dyn_tail) {
  if (gridDim.y > 1) {   // S draws per launch: tables, outputs and accumulators of draw blockIdx.y
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
  constexpr int LPN = KP / 4;
  constexpr bool LDSPHI = BT != 256;
  if (LDSPHI && !encode_only) {
    float* pl = lds_dyn();
    for (int i = threadIdx.x; i < Dcols; i += BT) pl[i] = phi[i];
    __syncthreads();
  }
  RowCtx<KP, LIK, LDSPHI> cx;
  cx.Ap = gtable(Ap, Dcols, KP);
  cx.Vp = gtable(Vp, Dcols, KP);
  cx.phi = phi;
  cx.ctype = ctype;
  cx.lane = threadIdx.x & 63;
  cx.sub = cx.lane % LPN;
  cx.grp = cx.lane / LPN;
  cx.bp_grp = cx.grp * 4;
  cx.bp_row = cx.grp * LPN * 4;
  const int lane = cx.lane, sub = cx.sub, grp = cx.grp;
  // The wave's number as a scalar (blockDim.x is BT): the row numbers a wave derives from it, and with them the
  // addresses of row_ptr[b], row_ptr[b + 1] and row_scale[b], are then wave-uniform for the compiler too, and a
  // row's bookkeeping is read by scalar loads -- three vector loads per row less in the in-order queue.
  const int wave = (int)blockIdx.x * (BT / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nwaves = (int)gridDim.x * (BT / 64);
  const int Bn = (int)B;   // row numbers fit 32 bits: B * KP * 4 < 4 GiB (checked by the host), and scalars are scarce here

  float4 veta4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!encode_only && (mode != 2 || LIK == 3 || !gzd))
    veta4 = make_float4((float)prep_sum(dprep, KP, sub * 4 + 0), (float)prep_sum(dprep, KP, sub * 4 + 1),
                        (float)prep_sum(dprep, KP, sub * 4 + 2), (float)prep_sum(dprep, KP, sub * 4 + 3));
  double ll_acc = 0.0, zsq_acc = 0.0, nnf_acc = 0.0;
  float4 zsum = make_float4(0.f, 0.f, 0.f, 0.f);

  // Which rows a wave takes.  Rows [0, B_static) are dealt out with a fixed stride (row w, w + nwaves, ...:
  // every wave the same count); the LAST eighth of a wave's share is not fixed: rows [B_static, B) are handed
  // out one at a time from sixteen counters (wave w draws from counter w % 16, which owns a sixteenth of that
  // range), so a wave that fell behind -- longer rows, a slower corner of the chip -- takes fewer of them and
  // the launch no longer ends with most waves waiting for the unluckiest one (the stored entries of a wave's
  // fixed share scatter by sqrt(rows per wave): +6.7 % at the largest of 4096 waves on the 8-GPU shard of
  // C3, +2.4 % on the whole matrix).  The counters are fp64 slot [kDaccDynSlot] of the sixteen replicas of the
  // scalar block (common.h: zeroed by the prep launch with everything else in it; the fold of the replicas skips
  // the slot, so its tail pair is always zero).
  // Off (B_static = B) in the deterministic mode -- which workgroup sums which rows must not depend on timing
  // there -- and for launches that share a step's scalar block with another row launch (dyn_tail = 0).
  int B_static = Bn;
  int dyn_lo = Bn, dyn_hi = Bn;
  unsigned int* dyn_ctr = nullptr;
  if (dyn_tail && !det_slots && !encode_only) {
    const int per_wave = Bn / nwaves;
    if (per_wave >= 8) {
      int fixed = per_wave - (per_wave * ROW_DYN_NUM) / ROW_DYN_DEN;
      if (fixed < 2) fixed = 2;
      B_static = fixed * nwaves;
      const int r = (int)(wave & (kDaccRep - 1));
      const int each = (Bn - B_static + kDaccRep - 1) / kDaccRep;
      dyn_lo = B_static + r * each;
      dyn_hi = dyn_lo + each < Bn ? dyn_lo + each : Bn;
      if (dyn_lo > Bn) dyn_lo = Bn;
      dyn_ctr = reinterpret_cast<unsigned int*>(dacc + (size_t)r * (kDaccHead + KP) + kDaccDynSlot);
    }
  }
  // the row after `cur` in this wave's sequence when it is a fixed one, else -1 (ask the counter)
  auto fixed_next = [&](int cur) -> int {
    if (cur >= Bn) return Bn;
    if (cur + nwaves < B_static) return cur + nwaves;
    return dyn_ctr ? -1 : Bn;
  };
  auto take_dynamic = [&]() -> int {          // (wave-uniform; the wait for the atomic is here)
    unsigned int k = 0;
    if (lane == 0) k = atomicAdd(dyn_ctr, 1u);
    k = (unsigned int)__builtin_amdgcn_readfirstlane((int)k);
    const int row = dyn_lo + (int)k;
    return row < dyn_hi ? row : Bn;
  };

  // The counter as a one-word buffer, so that the ask can be issued by every row on every path: a lane that is
  // not lane 0, and every lane of a row that has no ask to make, addresses the word BEHIND the counter, which the
  // address unit's range check drops (no memory operation; it returns 0).  The number of vector-memory operations
  // of a row's issue point then does not depend on the path (issue_next below).
  const __amdgpu_buffer_rsrc_t dyn_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      dyn_ctr ? dyn_ctr : reinterpret_cast<unsigned int*>(dacc), 0, dyn_ctr ? 4 : 0, 0x00020000);

  // Software pipeline across rows: while a row is processed, the first two 64-entry chunks of the next row and
  // the pointers of the row after next are in flight, so the row_ptr -> col/val dependent latency is off the
  // per-row critical path.
  // WHERE they are issued (issue_next): behind the row's LAST gathers, before those are waited for.  Vector-memory
  // operations return in issue order -- a counted s_waitcnt vmcnt(N) relies on it -- so a load in front of a
  // gather is waited for by the first wait on that gather: issued at the top of the row (as until round 5), the
  // entry words (HBM) and the counter's atomic stood in front of the row's first A' group.  Behind the last
  // gathers they are younger than every gather of the row and have its arithmetic tail (dot folds, log, rcp,
  // back-substitution, cross-group sums, stores) to land; they are first needed by the next row.
  // row_ptr and row_scale are read-only for the kernel's lifetime: read as constant memory, a load from a
  // wave-uniform address is a scalar load whatever the kernel stores elsewhere
  typedef const __attribute__((address_space(4))) int32_t* RowPtr;
  typedef const __attribute__((address_space(4))) float* RowScale;
  const RowPtr rptr = (RowPtr)row_ptr;
  const RowScale rscale = (RowScale)row_scale;
  int start = 0, end = 0, pc0 = 0, pc1 = 0, nstart = 0, nend = 0;
  float xi = 1.f, px0 = 0.f, px1 = 0.f, nxi = 1.f;
  // One more stage of lookahead for the warm-up (K <= 32, where the issue point stands behind the gathers): a row's
  // pointers are asked for one issue point before its lines are touched, and those are touched ROW_PREFETCH rows
  // ahead of the row's vector load.  (wstart, wend) is that pair; it feeds dead loads only, the rows themselves
  // still take their pointers from (nstart, nend) as before.  A row that a counter hands out has no number that
  // early and goes without (the pair stays 0, 0: nothing is read); so does each wave's first fixed row behind the
  // two of the prologue.  The entry loads of the issue point drop their non-temporal hint with it (issue_next).
  // Not the canonical format at K = 32: it retires two words per rung (two arrays), and with five rungs four of its
  // instances -- LIK 0 and 3 in both LDS forms -- already needed 12 bytes of scratch under the four-wave bound.  One
  // rule for the format at that K: the parent's loop.
  constexpr bool WARM = ROW_PREFETCH > 0 && KP <= 32 && (PACKED || KP < 32);
  int wstart = 0, wend = 0;
  int b = wave < B_static ? wave : Bn;
  int bn = fixed_next(b);
  if (bn < 0) bn = take_dynamic();
  int bnn = fixed_next(bn);
  if (bnn < 0) bnn = take_dynamic();
  if (b < Bn) {
    start = rptr[b];
    end = rptr[b + 1];
    xi = row_scale ? rscale[b] : 1.f;
    const EntryRow<PACKED> er = entry_row<PACKED>(col, val, ent, start, end - start);
    load_entry<PACKED, true>(er, lane, pc0, px0);
    load_entry<PACKED, true>(er, lane + 64, pc1, px1);
  }
  if (bn < Bn) {
    nstart = rptr[bn];
    nend = rptr[bn + 1];
    nxi = row_scale ? rscale[bn] : 1.f;
  }
  while (b < Bn) {
    const int n = end - start;
    int qc0 = 0, qc1 = 0, nnstart = 0, nnend = 0;
    float qx0 = 0.f, qx1 = 0.f, nnxi = 1.f;
    // the row three ahead: a fixed one, or a counter's next (asked for at the issue point, looked at when this
    // row is done)
    int bnnn = fixed_next(bnn);
    const bool dyn_ask = bnnn < 0;                  // wave-uniform
    unsigned int dyn_k = 0;
    // the row whose pointers the warm-up asks for now and uses at the next issue point: bnnn, which is bnn there
    // (a lead of one row), or the row behind it (a lead of two); -1 or Bn: none
    int wrow = bnnn;
    if (ROW_PREFETCH == 2 && wrow >= 0) wrow = fixed_next(wrow);
    int nwstart = 0, nwend = 0;
    RowWarm<PACKED> warm;
    // The row's issue point, run ONCE on every path through the row: the counter's ask, the two chunks of the
    // next row (whose pointers came a row ago; a wave's last rows load nothing) and the pointers of the
    // row after next (scalar loads).  Nothing here stands under a lane predicate.
    // (always_inline: at K <= 32 every arm of the last chunk's switch carries a copy)
    auto issue_next = [&]() __attribute__((always_inline)) {
      issue_fence(PACKED ? (const void*)ent : (const void*)col, val, row_ptr);
      dyn_k = (unsigned int)__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(1, dyn_rsrc, (dyn_ask && lane == 0) ? 0 : 4,
                                                                       0, 0);
      const EntryRow<PACKED> er = entry_row<PACKED>(col, val, ent, nstart, nend - nstart);
      // (no non-temporal hint on lines that the warm-up has brought in: with the hint the warm-up gains less than
      //  half as much, profiles/r09_row_prefetch_ab.txt; without the warm-up the hint makes no difference)
      load_entry<PACKED, !WARM>(er, lane, qc0, qx0);
      load_entry<PACKED, !WARM>(er, lane + 64, qc1, qx1);
      if (bnn < Bn) {
        nnstart = rptr[bnn];
        nnend = rptr[bnn + 1];
        nnxi = row_scale ? rscale[bnn] : 1.f;
      }
      // The warm-up rides in this batch of scalar loads and nowhere else: a scalar load in flight turns the next wait
      // on a ds_bpermute into a full lgkmcnt(0) (one counter, and scalar loads return out of order), which the row
      // pointers cause here in any case; at the top of a row it would park the wave in front of sweep 1.
      if constexpr (WARM) {
        warm_issue<PACKED>(warm, col, val, ent, wstart, wend - wstart);
        if (wrow >= 0 && wrow < Bn) {
          nwstart = rptr[wrow];
          nwend = rptr[wrow + 1];
        }
      }
      issue_fence(PACKED ? (const void*)ent : (const void*)col, val, row_ptr);
    };
    // Where the warm-up's dead words are let go: behind the first broadcasts that follow the issue point (s2_cells),
    // whose wait covers the scalar loads in any case -- no wait is added, and the words hold their registers for the
    // dot products only.  (The encode-only sweep has nothing behind its issue point: the next row's first broadcast
    // is that wait.)
    auto landed = [&](int behind) __attribute__((always_inline)) {
      if constexpr (WARM) warm_retire<PACKED>(warm, behind);
    };
    // K = 64 has no register for it (a chunk's V' rows alone are 64): its issue point stays at the top of the row
    constexpr bool BEHIND = KP <= 32;
    if constexpr (!BEHIND) issue_next();
    float4 zacc = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 gz = make_float4(0.f, 0.f, 0.f, 0.f);
    float llrow = 0.f;
    if (n <= 128) {
      // ---- short row: col/val stay in registers for both sweeps ----------
      int c0, c1;
      float x0, x1;
      unpack_entry<PACKED>(pc0, px0, lane < n, c0, x0);
      unpack_entry<PACKED>(pc1, px1, lane + 64 < n, c1, x1);
      const int n0 = min(n, 64);
      const int n1 = n - 64;
      // K <= 32: the row is one full chunk (n1 > 0: 64 entries, straight-line code) and its LAST chunk (cl, xl,
      // nl), the only one that can be partly filled, which each sweep dispatches once on its number of gather
      // instructions (RowCtx::sweep1_last / sweep2_last)
      const bool two = n1 > 0;                            // wave-uniform
      const int cl = two ? c1 : c0, nl = two ? n1 : n0;
      const float xl = two ? x1 : x0;
      if (mode != 2) {
        if constexpr (KP <= 32) {
          if (two) cx.template s1_arm<LPN>(c0, x0, zacc);
          cx.sweep1_last(cl, xl, nl, zacc);
        } else {
          cx.sweep1(c0, x0, n0, zacc);
          if (two) cx.sweep1(c1, x1, n1, zacc);
        }
        zacc = across_groups_sum4<LPN>(zacc);
        zacc.x *= xi; zacc.y *= xi; zacc.z *= xi; zacc.w *= xi;
        // (stored here, not in the row epilogue: profiles/r06_stream_issue_ab.txt)
        if (grp == 0) reinterpret_cast<float4*>(z)[(size_t)b * LPN + sub] = zacc;
      } else {
        zacc = gather4<LPN>(z, (int)b, sub);
      }
      if (encode_only) {
        if constexpr (BEHIND) { issue_next(); landed(0); }   // behind the last sweep-1 group
      } else {
        // The first of two chunks, then the row's last chunk with the issue point behind its gathers.
        // K <= 32: a chunk's sweep 2 asks for all of its V' rows before its first dot product (s2_arm); at
        // K = 64 a chunk's V' rows are 64 registers, and it gathers group by group.
        if constexpr (KP <= 32) {
          if (two) cx.template s2_arm<LPN>(c0, x0, 64, zacc, gz, llrow, nnf_acc, [] {}, [](int) {});
          cx.sweep2_last(cl, xl, nl, zacc, gz, llrow, nnf_acc, issue_next, landed);
        } else {
          // (K = 64: group by group, the issue point was at the top of the row)
          cx.sweep2(c0, x0, n0, zacc, gz, llrow, nnf_acc, [] {}, [](int) {});
          if (n1 > 0) cx.sweep2(c1, x1, n1, zacc, gz, llrow, nnf_acc, [] {}, [](int) {});
        }
      }
    } else {
      // ---- long row: stream the row twice (second read is L2 served) -----
      // Chunks 0 and 1 were loaded at the previous row's issue point; chunk i+2 is fetched while chunk i is
      // processed, so no chunk waits for its own col/val (14 chunks a row on C4).
      const EntryRow<PACKED> er = entry_row<PACKED>(col, val, ent, start, n);
      if (mode != 2) {
        int ra = pc0, ra1 = pc1;
        float rb = px0, rb1 = px1;
        for (int base = start; base < end; base += 64) {
          const int i2 = base + 128 + lane;
          int ra2;
          float rb2;
          load_entry<PACKED, false>(er, i2 - start, ra2, rb2);
          int c;
          float x;
          unpack_entry<PACKED>(ra, rb, base + lane < end, c, x);
          cx.sweep1(c, x, min(64, end - base), zacc);
          ra = ra1; rb = rb1; ra1 = ra2; rb1 = rb2;
        }
        zacc = across_groups_sum4<LPN>(zacc);
        zacc.x *= xi; zacc.y *= xi; zacc.z *= xi; zacc.w *= xi;
        if (grp == 0) reinterpret_cast<float4*>(z)[(size_t)b * LPN + sub] = zacc;
      } else {
        zacc = gather4<LPN>(z, (int)b, sub);
      }
      if (encode_only) {
        if constexpr (BEHIND) { issue_next(); landed(0); }   // behind the last sweep-1 group
      } else {
        int ra = pc0, ra1 = pc1;
        float rb = px0, rb1 = px1;
        for (int base = start; base < end; base += 64) {
          const int i2 = base + 128 + lane;
          int ra2;
          float rb2;
          load_entry<PACKED, false>(er, i2 - start, ra2, rb2);
          int c;
          float x;
          unpack_entry<PACKED>(ra, rb, base + lane < end, c, x);
          // (the row's last chunk, K <= 32, carries the issue point behind its last group's gathers)
          if (BEHIND && base + 64 >= end) cx.sweep2(c, x, end - base, zacc, gz, llrow, nnf_acc, issue_next, landed);
          else cx.sweep2(c, x, min(64, end - base), zacc, gz, llrow, nnf_acc, [] {}, [](int) {});
          ra = ra1; rb = rb1; ra1 = ra2; rb1 = rb2;
        }
      }
    }
    // rotate the pipeline registers
    const float xi_cur = xi;
    const int b_cur = b;
    start = nstart; end = nend; xi = nxi;
    pc0 = qc0; px0 = qx0; pc1 = qc1; px1 = qx1;
    nstart = nnstart; nend = nnend; nxi = nnxi;
    if constexpr (WARM) { wstart = nwstart; wend = nwend; }
    {
      // (read on every path: an answer left unread would stay "in flight" for the compiler's wait counting)
      const int row = dyn_lo + (int)(unsigned int)__builtin_amdgcn_readfirstlane((int)dyn_k);
      if (dyn_ask) bnnn = row < dyn_hi ? row : Bn;
    }
    b = bn; bn = bnn; bnn = bnnn;
    if (encode_only) continue;
    gz = across_groups_sum4<LPN>(gz);
    if (grp == 0) {
      zsq_acc += (double)dot4(zacc, zacc);
      zsum = add4(zsum, zacc);
      // minus the derivative of sum_d r_bd over ALL columns: closed form veta
      // (linear decoder) or the dense exp term of this row (log_transform)
      // (mixed: closed-form Poisson-column part veta PLUS the dense Bernoulli-column term)
      float4 dn = (mode == 2 && gzd) ? gather4<LPN>(gzd, (int)b_cur, sub) : veta4;
      if (LIK == 3 && mode == 2 && gzd) dn = add4(dn, veta4);
      // mode 3 (both sweeps, dense row term subtracted LATER by the dense kernel's epilogue,
      // gzs_b -= xi_b * sum_d E_bd V'_d): only the closed-form Poisson-column part is known here
      if (mode == 3 && LIK != 3) dn = make_float4(0.f, 0.f, 0.f, 0.f);
      float4 o;
      o.x = xi_cur * (gz.x - dn.x - zacc.x);
      o.y = xi_cur * (gz.y - dn.y - zacc.y);
      o.z = xi_cur * (gz.z - dn.z - zacc.z);
      o.w = xi_cur * (gz.w - dn.w - zacc.w);
      reinterpret_cast<float4*>(gzs)[(size_t)b_cur * LPN + sub] = o;
    }
    ll_acc += (double)llrow;
  }
  if (encode_only) return;

  // ---- block reduction, one set of fp64 atomics per block ---------------
  __shared__ double red[16];
  __shared__ double zred_static[BT == 256 ? 4 : 1][KP];
  // with phi in LDS the per-wave z sums reuse that region (phi is no longer needed once
  // every wave has left the row loop): keeps two 80 KB workgroups inside 160 KB
  if (LDSPHI) __syncthreads();
  double (*zred)[KP] = LDSPHI ? reinterpret_cast<double (*)[KP]>(lds_dyn()) : zred_static;
  const int wid = threadIdx.x >> 6;
  if (grp == 0) {
    zred[wid][sub * 4 + 0] = (double)zsum.x;
    zred[wid][sub * 4 + 1] = (double)zsum.y;
    zred[wid][sub * 4 + 2] = (double)zsum.z;
    zred[wid][sub * 4 + 3] = (double)zsum.w;
  }
  const double ll_b = block_sum(ll_acc, red);
  const double zq_b = block_sum(zsq_acc, red);
  const double nf_b = block_sum(nnf_acc, red);
  if (det_slots) {
    // deterministic mode: this workgroup's sums in its own slot; the pack block of the column pass adds
    // the slots up in workgroup order
    double* sl = det_slots + (size_t)blockIdx.y * det_stride;
    if (blockIdx.x == 0 && threadIdx.x == 0) sl[0] = (double)gridDim.x;
    sl += kDetMeta + (size_t)blockIdx.x * (kDaccHead + KP);
    if (threadIdx.x == 0) {
      sl[0] = ll_b;
      sl[1] = zq_b;
      sl[2] = nf_b;
      sl[3] = sl[4] = sl[5] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x < KP) {
      double t = 0.0;
      const int nw = blockDim.x >> 6;
      for (int i = 0; i < nw; ++i) t += zred[i][threadIdx.x];
      sl[kDaccHead + threadIdx.x] = t;
    }
    return;
  }
  dacc += (size_t)(blockIdx.x % kDaccRep) * (kDaccHead + KP);
  if (threadIdx.x == 0) {
    atomicAdd(&dacc[0], ll_b);
    atomicAdd(&dacc[1], zq_b);
    if (nf_b != 0.0) atomicAdd(&dacc[2], nf_b);
  }
  __syncthreads();
  if (threadIdx.x < KP) {
    double t = 0.0;
    const int nw = blockDim.x >> 6;
    for (int i = 0; i < nw; ++i) t += zred[i][threadIdx.x];
    atomicAdd(&dacc[kDaccHead + threadIdx.x], t);
  }
}

// false: the device does not grant the dynamic LDS this form needs (the caller then launches
// the 256-thread form, which reads phi from global memory)
template <int KP, int LIK, int BT, int PACKED>
static bool launch_row_lds_t(const RowArgs& a, hipStream_t st) {
  // (the encode-only sweep reads no phi: it takes this launch shape, not the LDS)
  const size_t lds = a.mode == 1 ? 0 : std::max((size_t)a.D * 4, (size_t)(BT / 64) * KP * sizeof(double));
  // opt in to more than 64 KB of dynamic LDS.  The attribute is per DEVICE (and this is one
  // instantiation per process), so the grant is remembered per device ordinal.
  constexpr int kMaxDev = 64;
  static size_t granted[kMaxDev] = {};
  if (lds > 64 * 1024) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) {
      (void)hipGetLastError();
      return false;
    }
    if (lds > __atomic_load_n(&granted[dev], __ATOMIC_RELAXED)) {
      if (hipFuncSetAttribute((const void*)row_pass_kernel<KP, LIK, BT, PACKED>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return false;
      }
      __atomic_store_n(&granted[dev], lds, __ATOMIC_RELAXED);
    }
  }
  const int64_t want = (a.B + (BT / 64) - 1) / (BT / 64);
  // exactly the resident set (two 512-thread or one 1024-thread workgroup per CU), rows
  // grid-strided: every workgroup stages phi once.  Measured on C3 / a 125k-row shard:
  // 1.587 / 0.211 ms, against 1.596 / 0.227 with twice and 1.621 / 0.247 with eight times
  // as many workgroups (each re-stages 4*D bytes before its first gather).
#ifndef ROW_LDS_CAP
#define ROW_LDS_CAP 1024
#endif
  const int64_t cap = (int64_t)ROW_LDS_CAP * 256 / BT;
  const int nb = (int)(want < 1 ? 1 : (want > cap ? cap : want));
  hipLaunchKernelGGL((row_pass_kernel<KP, LIK, BT, PACKED>), dim3(nb, a.S > 1 ? a.S : 1), dim3(BT), lds, st,
                     a.B, a.row_ptr, a.col, a.val, a.row_scale, a.Ap, a.Vp, a.phi, a.dprep, a.z,
                     a.gzs, a.dacc, a.mode, a.gzd, a.ctype, a.D, a.dacc_stride, a.ent, a.det_slots, a.det_stride, a.dyn_tail);
  return true;
}

// packed entry stream (spmf_counts.ent) when the batch carries one
template <int KP, int LIK, int BT>
static bool launch_row_lds(const RowArgs& a, hipStream_t st) {
  return a.ent ? launch_row_lds_t<KP, LIK, BT, 1>(a, st) : launch_row_lds_t<KP, LIK, BT, 0>(a, st);
}

template <int KP>
static bool launch_row_t(const RowArgs& a, hipStream_t st) {
  int64_t want = (a.B + 3) / 4;  // 4 waves (rows in flight) per 256-thread block
  int nb = (int)(want < 1 ? 1 : (want > ROW_MAX_BLOCKS ? ROW_MAX_BLOCKS : want));
  // phi from LDS: the sweep-2 forms of the Poisson likelihoods at the K of the named
  // configs, when 4*D bytes fit (and the batch is big enough to fill the wider blocks)
  if constexpr (KP >= 16) {
    if (a.mode == 1 && a.B >= 4096) {
      // sweep 1 alone (z from the encoder side) does not depend on the likelihood: the
      // resident-set launch of the 512-thread form, without the phi copy.  C4: 8.6 -> 6.4 ms
      // against the 256-thread grid (profiles/r03_sparse_pass_attempts.txt e25)
      if (launch_row_lds<KP, 0, 512>(a, st)) return true;
    }
    if (a.mode != 1 && a.logt >= 0 && a.logt <= 3 && a.B >= 4096) {
      // (likelihood codes 2 and 3, Bernoulli and mixed, since the end of round 3: their
      //  stored-cell sweep read phi one entry per lane from global memory, C5 0.61 ms)
      const size_t need = (size_t)a.D * 4;
      bool done = false;
      if (need <= 80 * 1024) {
        done = a.logt == 0   ? launch_row_lds<KP, 0, 512>(a, st)
               : a.logt == 1 ? launch_row_lds<KP, 1, 512>(a, st)
               : a.logt == 2 ? launch_row_lds<KP, 2, 512>(a, st)
                             : launch_row_lds<KP, 3, 512>(a, st);
      } else if (need <= 160 * 1024 - 1024) {
        done = a.logt == 0   ? launch_row_lds<KP, 0, 1024>(a, st)
               : a.logt == 1 ? launch_row_lds<KP, 1, 1024>(a, st)
               : a.logt == 2 ? launch_row_lds<KP, 2, 1024>(a, st)
                             : launch_row_lds<KP, 3, 1024>(a, st);
      }
      if (done) return true;
    }
  }
#define SPMF_ROW_LAUNCH(L_)                                                                    \
  hipLaunchKernelGGL((row_pass_kernel<KP, L_>), dim3(nb, a.S > 1 ? a.S : 1), dim3(256), 0, st, \
                     a.B, a.row_ptr, a.col, a.val, a.row_scale, a.Ap, a.Vp, a.phi, a.dprep, a.z, \
                     a.gzs, a.dacc, a.mode, a.gzd, a.ctype, a.D, a.dacc_stride, a.ent, a.det_slots, a.det_stride, a.dyn_tail)
  if (a.logt == 4) SPMF_ROW_LAUNCH(4);
  else if (a.logt == 3) SPMF_ROW_LAUNCH(3);
  else if (a.logt == 2) SPMF_ROW_LAUNCH(2);
  else if (a.logt == 1) SPMF_ROW_LAUNCH(1);
  else SPMF_ROW_LAUNCH(0);
#undef SPMF_ROW_LAUNCH
  return true;
}

bool launch_row_pass(int KP, const RowArgs& a, hipStream_t st) {
  if (KP > 64) return launch_row_widek(KP, a, st);   // widek.hip: a factor row is the whole wave
  bool ok = false;
  return with_kp<64>(KP, [&](auto kp) { ok = launch_row_t<decltype(kp)::value>(a, st); }) && ok;
}

}  // namespace spmf
