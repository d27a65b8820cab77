// kernels_fix.hip -- the absolute pose-fix update (fmskf_correct_pose) of KF6 and EKF9 for gfx950.
//
// One lane per fix of a sorted list: the lane reads its 16-byte fmskf_pose_fix and the `robot`
// word of the entry before it, and -- when the entry is well formed (robot < N and above its
// predecessor) -- gathers that robot's state rows, runs a measurement update with H = the first
// M rows of the identity (z = (px, py) or (px, py, theta)) and scatters the rows back.  No
// predict, and no robot that is not listed is read or written.
//
// The update is the tick's, instantiated for another H: kf_update_factor, NIS from w and D^-1 as
// the chi-square gate forms it (kf_nis), then kf_update_apply behind the per-lane
// decision -- with the EKF9's compensated heading (CI = 2, th_add / th_norm) and, for KF6 with
// FMSKF_CFG_COMP_POS, the position low parts (CXM / CPM) exactly where the models' own updates
// have them.  A rejected or ignored lane stores nothing.
//
// Addressing: per lane through FixRows (list_rows.hpp): one whole-array descriptor, the lane's
// row-0 byte offset as voffset, the row as a scalar offset; past 4 GiB the BIG form.
//
// Cost: the gathers are element-granular.  With `robot` ascending, a wave at density 1 touches
// each row's 256 contiguous bytes; at one robot in 32 every row load of a lane touches its own
// 128-byte line (DESIGN.md section 3 has the model and the measured numbers).
//
// The kernel takes its own argument struct (FixArgs): nothing is added to the tick kernels'.
#include "list_rows.hpp"

#pragma clang fp contract(off)

namespace fmskf {

struct FixArgs {
  uint64_t n;      // robots of the handle
  uint64_t count;  // fixes
  uint64_t pitch;  // the tiled arrays hold rows x pitch elements
  float *x, *P;
  float *thlo;  // EKF9: [N] heading low part
  float *lo;    // KF6 + FMSKF_CFG_COMP_POS: the tiled low-part rows
  const uint32_t *fixes;  // [count] x 16 B: robot, x_m, y_m, theta_rad
  float *nis;             // [count] or null
  uint8_t *status;        // [count] or null
  unsigned long long *counters;  // [0]: states that went non-finite
  unsigned long long *ignored;   // malformed entries
  float r[6];                    // packed lower triangle of the fix noise (3 x 3)
  float nis_max;
};

// H = the first MM rows of the identity
template <int NX, int MM>
struct MdFix {
  using T = float;
  static constexpr int N = NX, M = MM;
  __host__ __device__ static constexpr int h1(int a) { return a; }
  __host__ __device__ static constexpr int h2(int) { return -1; }
};

// NX: 6 (KF6) or 9 (EKF9, with the heading low part); MM: 2 or 3; COMP: KF6's position low parts
template <int NX, int MM, bool COMP, int CP, bool BIG>
__global__ __launch_bounds__(kBlock) void k_fix(FixArgs a) {
  using S = ListRows<NX, COMP, CP, BIG>;
  constexpr int NP = S::NP;
  constexpr bool EKF = S::EKF;
  using Md = MdFix<NX, MM>;
  const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool have = k < a.count;
  uint32_t robot = 0, prev = 0;
  float z[3] = {0.f, 0.f, 0.f};
  if (have) {
    const uint4 f = reinterpret_cast<const uint4 *>(a.fixes)[k];
    if (k > 0) prev = a.fixes[(k - 1) * 4];
    robot = f.x;
    z[0] = __builtin_bit_cast(float, f.y);
    z[1] = __builtin_bit_cast(float, f.z);
    z[2] = __builtin_bit_cast(float, f.w);
  }
  const bool ok = have && robot < a.n && (k == 0 || robot > prev);
  float nis = 0.f;
  uint32_t status = FMSKF_FIX_IGNORED;
  if (ok) {
    const S rows(a, robot);
    float x[NX], P[NP], cl[S::NL] = {}, lo = 0.f;
    // gather and scatter stay loops of the kernel's own (list_rows.hpp ListRows)
#pragma unroll
    for (int j = 0; j < NX; j++) x[j] = rows.tx.ld(j);
#pragma unroll
    for (int j = 0; j < NP; j++) P[j] = rows.tp.ld(j);
    if constexpr (COMP) {
#pragma unroll
      for (int j = 0; j < S::NL; j++) cl[j] = rows.tl.ld(j);
    }
    if constexpr (EKF) lo = rows.th.ld();
    // y = z - H x: a compensated state is hi + lo (as the EKF9's own heading innovation), the
    // heading innovation wrapped
    float y[MM], U[MM][NX], dinv[MM], w[MM];
    y[0] = COMP ? (z[0] - x[0]) - cl[0] : z[0] - x[0];
    y[1] = COMP ? (z[1] - x[1]) - cl[1] : z[1] - x[1];
    if constexpr (MM == 3) y[2] = EKF ? wrap_innov((z[2] - x[2]) - lo) : wrap_innov(z[2] - x[2]);
    kf_update_factor<Md, float, NX, MM, NP>(P, y, a.r, U, dinv, w);
    nis = kf_nis(w, dinv);
    const bool apply = nis <= a.nis_max;  // a NaN NIS never applies
    status = apply ? FMSKF_GATE_ACCEPTED : FMSKF_GATE_REJECTED;
    if (apply) {
      if constexpr (EKF) {
        kf_update_apply<Md, 2, float, NX, MM, NP>(x, P, U, dinv, w, &lo);
        th_norm(x[2], lo);
      } else if constexpr (COMP) {
        kf_update_apply<Md, -1, float, NX, MM, NP, kKf6CXM, kKf6CPM>(x, P, U, dinv, w, nullptr, cl);
      } else {
        kf_update_apply<Md, -1, float, NX, MM, NP>(x, P, U, dinv, w);
      }
#pragma unroll
      for (int j = 0; j < NX; j++) rows.tx.st(j, x[j]);
#pragma unroll
      for (int j = 0; j < NP; j++) rows.tp.st(j, P[j]);
      if constexpr (COMP) {
#pragma unroll
        for (int j = 0; j < S::NL; j++) rows.tl.st(j, cl[j]);
      }
      if constexpr (EKF) rows.th.st(lo);
      nan_guard(x, P, a.counters);
    }
  }
  if (have) {
    if (a.nis) a.nis[k] = nis;
    if (a.status) a.status[k] = (uint8_t)status;
  }
  count_ignored(have && !ok, a.ignored);
}

int launch_pose_fix(const DevState &s, const PoseFixDev &f, hipStream_t st) {
  const ListRegime rg = list_regime(s);
  if (!rg.ok) return (int)hipErrorNotSupported;
  if (!f.fixes || !f.count || !f.ignored || (f.m != 2 && f.m != 3)) return (int)hipErrorInvalidValue;
  FixArgs a{s.n, f.count, s.pitch, (float *)s.x, (float *)s.P, s.thlo, s.xlo, f.fixes, f.nis, f.status,
            s.counters, f.ignored, {}, f.nis_max};
  for (int k = 0; k < 6; k++) a.r[k] = f.r[k];
  with_list_regime(
      rg,
      [&](auto NX, auto COMP, auto CP, auto BIG, auto M3) {
        k_fix<NX(), M3() ? 3 : 2, COMP(), CP(), BIG()><<<grid_for(a.count), kBlock, 0, st>>>(a);
      },
      f.m == 3);
  return (int)hipGetLastError();
}

}  // namespace fmskf
