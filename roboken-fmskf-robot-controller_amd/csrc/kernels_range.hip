// kernels_range.hip -- range updates against surveyed anchors (fmskf_correct_range) of KF6 and
// EKF9 for gfx950.
//
// One lane per entry of a non-descending list.  A run -- the consecutive entries of one robot, a
// UWB burst -- is owned by the lane of its first entry (the lane whose predecessor has another
// robot): it gathers the robot's rows once through FixRows (list_rows.hpp), applies the run's
// entries in list order, each on the state the one before left (range_lane.hpp: the geometry on
// the current estimate, then the gated scalar update with a three-coefficient H), scatters the
// rows once and only if an entry was applied, calls nan_guard once and writes d2 and status of
// every entry of the run.  The other lanes of a run do nothing, except those whose entry lies
// FMSKF_RANGE_RUN_MAX or more places into the run: the entry that many places before them has
// the same robot, the owner stops before them, and they report themselves ignored.  So every
// entry's outputs are written exactly once.  No predict, and no robot that is not listed is read
// or written.
//
// The run loop is a real loop (not unrolled) whose body indexes x, P and the low parts with
// compile-time constants only: they stay in registers across the iterations.
//
// Cost: 16 B per entry (plus the predecessor words, which hit the same lines) and the pose fix's
// gather traffic per robot (kernels_fix.hip), whatever the run's length.
//
// The kernel takes its own argument struct (RangeArgs): nothing is added to the tick kernels'.
#include "range_lane.hpp"
#include "list_rows.hpp"

#pragma clang fp contract(off)

namespace fmskf {

struct RangeArgs {
  uint64_t n;      // robots of the handle
  uint64_t count;  // entries
  uint64_t pitch;  // the tiled arrays hold rows x pitch elements
  float *x, *P;
  float *thlo;  // EKF9: [N] heading low part
  float *lo;    // KF6 + FMSKF_CFG_COMP_POS: the tiled low-part rows
  const uint32_t *fixes;  // [count] x 16 B: robot, anchor, range_m, var_m2
  const float *anchors;   // [n_anchors] x 16 B: x, y, z, 0
  const float *sintab;    // the 513-entry TABLE512 sine table
  float *d2;              // [count] or null
  uint8_t *status;        // [count] or null
  unsigned long long *counters;  // [0]: states that went non-finite
  unsigned long long *ignored;   // ignored entries
  uint32_t n_anchors;
  float tag[3];
  float var, d2_max, d_min;
};

constexpr int kRunMax = (int)FMSKF_RANGE_RUN_MAX;

__device__ __forceinline__ void range_out(const RangeArgs &a, uint64_t k, float d2, uint32_t status) {
  if (a.d2) a.d2[k] = d2;
  if (a.status) a.status[k] = (uint8_t)status;
}

// NX: 6 (KF6) or 9 (EKF9, with the heading low part); COMP: KF6's position low parts; LIBM: the
// handle's sin / cos policy
template <int NX, bool COMP, bool LIBM, int CP, bool BIG>
__global__ __launch_bounds__(kBlock) void k_range(RangeArgs a) {
  using S = ListRows<NX, COMP, CP, BIG>;
  constexpr bool EKF = S::EKF;
  constexpr int CI = EKF ? 2 : -1;
  constexpr unsigned CXM = COMP ? kKf6CXM : 0u;
  constexpr unsigned long long CPM = COMP ? kKf6CPM : 0ull;
  const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= a.count) return;
  const uint4 *list = reinterpret_cast<const uint4 *>(a.fixes);
  uint4 f = list[k];
  const uint32_t robot = f.x;
  const uint32_t prev = k > 0 ? a.fixes[(k - 1) * 4] : 0u;
  uint32_t nign = 0;
  if (k > 0 && prev == robot) {
    // not the run's first entry: the owner covers it, unless it lies past the owner's reach
    if (k >= (uint64_t)kRunMax && a.fixes[(k - kRunMax) * 4] == robot) {
      range_out(a, k, 0.f, FMSKF_FIX_IGNORED);
      nign = 1;
    }
  } else if (robot >= a.n || (k > 0 && robot < prev)) {
    // a malformed run head: the whole run (what this lane owns of it) is ignored
    for (int j = 0; j < kRunMax; j++) {
      const uint64_t e = k + j;
      if (e >= a.count || (j > 0 && a.fixes[e * 4] != robot)) break;
      range_out(a, e, 0.f, FMSKF_FIX_IGNORED);
      nign++;
    }
  } else {
    const S rows(a, robot);
    float x[NX], P[S::NP], cl[S::NL] = {}, lo = 0.f;
    // gather and scatter stay loops of the kernel's own (list_rows.hpp ListRows)
#pragma unroll
    for (int j = 0; j < NX; j++) x[j] = rows.tx.ld(j);
#pragma unroll
    for (int j = 0; j < S::NP; j++) P[j] = rows.tp.ld(j);
    if constexpr (COMP) {
#pragma unroll
      for (int j = 0; j < S::NL; j++) cl[j] = rows.tl.ld(j);
    }
    if constexpr (EKF) lo = rows.th.ld();
    bool any = false;
#pragma unroll 1
    for (int j = 0; j < kRunMax; j++) {
      const uint64_t e = k + j;
      if (j > 0) {
        if (e >= a.count) break;
        f = list[e];
        if (f.x != robot) break;
      }
      float d2 = 0.f;
      uint32_t status = FMSKF_FIX_IGNORED;
      if (f.y < a.n_anchors) {
        const float4 an = reinterpret_cast<const float4 *>(a.anchors)[f.y];
        const float c = cos_p<LIBM>(x[2], a.sintab), s = sin_p<LIBM>(x[2], a.sintab);
        float H[3], d;
        if (range_geometry<COMP>(x[0], x[1], cl, c, s, a.tag, an.x, an.y, an.z, a.d_min, H, d)) {
          const float range = __builtin_bit_cast(float, f.z), var = __builtin_bit_cast(float, f.w);
          const float r = var > 0.f ? var : a.var;
          const bool apply = range_update<CI, CXM, CPM>(x, P, &lo, cl, H, range - d, r, a.d2_max, d2);
          if (apply) range_norm<CI, CXM, CPM>(x, P, &lo, cl);
          any = any || apply;
          status = apply ? FMSKF_GATE_ACCEPTED : FMSKF_GATE_REJECTED;
        } else {
          status = FMSKF_RANGE_NEAR;
        }
      } else {
        nign++;
      }
      range_out(a, e, d2, status);
    }
    if (any) {
#pragma unroll
      for (int j = 0; j < NX; j++) rows.tx.st(j, x[j]);
#pragma unroll
      for (int j = 0; j < S::NP; j++) rows.tp.st(j, P[j]);
      if constexpr (COMP) {
#pragma unroll
        for (int j = 0; j < S::NL; j++) rows.tl.st(j, cl[j]);
      }
      if constexpr (EKF) rows.th.st(lo);
      nan_guard(x, P, a.counters);
    }
  }
  if (nign) atomicAdd(a.ignored, (unsigned long long)nign);  // malformed lists only
}

int launch_range_fix(const DevState &s, const RangeDev &f, bool libm, hipStream_t st) {
  const ListRegime rg = list_regime(s);
  if (!rg.ok) return (int)hipErrorNotSupported;
  if (!f.fixes || !f.count || !f.ignored || !f.anchors || !f.n_anchors) return (int)hipErrorInvalidValue;
  RangeArgs a{s.n, f.count, s.pitch, (float *)s.x, (float *)s.P, s.thlo, s.xlo, f.fixes, f.anchors, s.sintab,
              f.d2, f.status, s.counters, f.ignored, f.n_anchors, {f.tag[0], f.tag[1], f.tag[2]},
              f.var, f.d2_max, f.d_min};
  with_list_regime(
      rg,
      [&](auto NX, auto COMP, auto CP, auto BIG, auto LIBM) {
        k_range<NX(), COMP(), LIBM(), CP(), BIG()><<<grid_for(a.count), kBlock, 0, st>>>(a);
      },
      libm);
  return (int)hipGetLastError();
}

}  // namespace fmskf
