// list_rows.hpp -- what the kernels that work on a list of robots share (kernels_fix.hip:
// fmskf_correct_pose; kernels_range.hip: fmskf_correct_range; kernels_select.hip: the subset get /
// set): the tiled state rows of one robot addressed per lane, the rows of a listed robot's whole
// state as one lane struct, the count of malformed entries, and the one launcher of the three
// kernels' forms.
//
// The state is tiled [ceil(N / 2048)][rows][2048] (fmskf_internal.hpp st_at) and a wave's listed
// robots lie in arbitrary tiles, so the wave-uniform per-chunk descriptors of the tick kernels do
// not apply.  Each array is one descriptor over the whole array (kernel arguments only, so it
// stays in SGPRs), the lane's row-0 byte offset is its voffset and row k the scalar offset
// k * 2048 * 4: one address register per array and the state's cache policy in the aux bits.  An
// array past 4 GiB (KF6 beyond 51 M robots, EKF9 beyond 23 M) cannot be reached through 32-bit
// offsets: the BIG form uses 64-bit lane addresses and non-temporal accesses (such a state is
// always streamed).
//
// ListRows, ThLo and count_ignored were lifted out of the three kernels in the spelling that
// leaves every kernel body the one it was (profiles/list_lane_bodies.json).
#pragma once
#include "kf6_lane.hpp"

namespace fmskf {

// ROWS tiled rows of one robot, addressed per lane
template <int ROWS, int CP, bool BIG>
struct FixRows {
  static constexpr uint32_t W = tile_w<float>();
  __amdgpu_buffer_rsrc_t r;
  uint32_t vo;
  float *p;
  __device__ __forceinline__ FixRows(float *base, uint64_t pitch, uint32_t robot) {
    const uint64_t e = (uint64_t)(robot / W) * ((uint64_t)ROWS * W) + robot % W;
    if constexpr (BIG) {
      p = base + e;
    } else {
      r = rsrc(base, (uint64_t)ROWS * pitch * sizeof(float));
      vo = (uint32_t)e * 4u;
    }
  }
  __device__ __forceinline__ float ld(int k) const {
    if constexpr (BIG) return __builtin_nontemporal_load(p + (size_t)k * W);
    else return ld_f32<CP>(r, vo, k * W * 4);
  }
  __device__ __forceinline__ void st(int k, float v) const {
    if constexpr (BIG) __builtin_nontemporal_store(v, p + (size_t)k * W);
    else st_f32<st_pol(CP)>(r, vo, k * W * 4, v);
  }
};

// the EKF9's heading low part of one robot ([N], not tiled), in the two forms of FixRows
template <int CP, bool BIG>
struct ThLo {
  float *thlo;
  uint64_t n;
  uint32_t robot;
  __device__ __forceinline__ float ld() const {
    if constexpr (BIG) return __builtin_nontemporal_load(thlo + robot);
    else return ld_f32<CP>(rsrc(thlo, n * sizeof(float)), robot * 4u, 0);
  }
  __device__ __forceinline__ void st(float v) const {
    if constexpr (BIG) __builtin_nontemporal_store(v, thlo + robot);
    else st_f32<st_pol(CP)>(rsrc(thlo, n * sizeof(float)), robot * 4u, 0, v);
  }
};

// The rows of one listed robot's whole state: x, P, KF6's position low parts (COMP) and the EKF9's
// heading low part (NX == 9).  A: a kernel's argument struct with n, pitch, x, P, thlo and lo.
// The kernel keeps x[NX], P[NP], cl[NL] and lo as locals of its own and gathers / scatters them
// with its own loops over tx, tp, tl and th, in that order.  Not members and member functions
// here: the arrays as members, or filled (k_fix, k_range) or stored (k_fix) by a member function,
// reach the compiler's alloca-to-vector step in another shape, and all 18 bodies of the kernel
// move (instruction order and register numbers; tools/body_compare.py).
template <int NX, bool COMP, int CP, bool BIG>
struct ListRows {
  static constexpr int NP = NX * (NX + 1) / 2, NL = COMP ? (int)kKf6LoRows : 1;
  static constexpr bool EKF = NX == 9;
  static_assert(!(EKF && COMP), "EKF9 with FMSKF_CFG_COMP_POS is not supported");
  const FixRows<NX, CP, BIG> tx;
  const FixRows<NP, CP, BIG> tp;
  const FixRows<NL, CP, BIG> tl;  // not COMP: never accessed
  const ThLo<CP, BIG> th;         // not EKF: never accessed
  template <class A>
  __device__ __forceinline__ ListRows(const A &a, uint32_t robot)
      : tx(a.x, a.pitch, robot), tp(a.P, a.pitch, robot), tl(COMP ? a.lo : a.x, a.pitch, robot),
        th{a.thlo, a.n, robot} {}
};

// the wave's lanes with a malformed entry counted into *ignored: one atomic, by the first of them
__device__ __forceinline__ void count_ignored(bool lane_bad, unsigned long long *ignored) {
  const unsigned long long bad = __ballot(lane_bad);
  if (bad && (threadIdx.x & 63) == __builtin_ctzll(bad)) atomicAdd(ignored, (unsigned long long)__popcll(bad));
}

// ---------------------------------------------------------------------------
// host side: the launch regime of a handle's list kernels
// ---------------------------------------------------------------------------
// ok: KF6 (plain, FMSKF_CFG_COMP_POS) or plain EKF9 with the tiled state; nt: the state's cache
// policy as the model's tick launcher chooses it; big: the 64-bit-address form, which the state's
// largest tiled array (P) needs past the reach of a 32-bit byte offset and FMSKF_LIST_BIG=1 (read
// once) forces
struct ListRegime {
  bool ok, ekf, comp, nt, big;
};
inline ListRegime list_regime(const DevState &s) {
  const bool force_big = FMSKF_ENV_INT("FMSKF_LIST_BIG", 0) != 0;
  const bool ekf = s.model == FMSKF_MODEL_EKF9, comp = s.xlo != nullptr;
  const bool ok = s.tile == tile_w<float>() && (ekf || s.model == FMSKF_MODEL_KF6) && !(ekf && (comp || !s.thlo));
  const bool big = force_big || (uint64_t)(ekf ? 45 : 21) * s.pitch * sizeof(float) > 0xFFFFFFFFull;
  return {ok, ekf, comp, state_nt(s.n * (ekf ? ekf9_state_bytes(false) : kf6_state_bytes(comp))), big};
}

// with_bools for a list kernel: f(NX, COMP, CP, BIG, bools...) with the regime as compile-time
// constants -- KF6, KF6 + FMSKF_CFG_COMP_POS and EKF9, each cached, non-temporal or BIG, and no
// other combination -- followed by a std::bool_constant per further bool
template <class F, class... Bs>
inline void with_list_regime(const ListRegime &r, F &&f, Bs... bs) {
  using std::integral_constant;
  auto form = [&](auto nx, auto comp) {
    with_bools(
        [&](auto... k) {
          if (r.big) f(nx, comp, integral_constant<int, kStateNT>{}, std::true_type{}, k...);
          else if (r.nt) f(nx, comp, integral_constant<int, kStateNT>{}, std::false_type{}, k...);
          else f(nx, comp, integral_constant<int, 0>{}, std::false_type{}, k...);
        },
        bs...);
  };
  if (r.ekf) form(integral_constant<int, 9>{}, std::false_type{});
  else if (r.comp) form(integral_constant<int, 6>{}, std::true_type{});
  else form(integral_constant<int, 6>{}, std::false_type{});
}

}  // namespace fmskf
