// range_lane.hpp -- one range measurement against a surveyed anchor as lane functions
// (fmskf_correct_range; kernels_range.hip): the antenna's geometry on the lane's current estimate
// and the scalar update whose H has three real, state-dependent coefficients on the states
// 0, 1, 2 (px, py, theta) -- kf_update_seq / kf_update_seq_gated only know selector rows.
//
// Canonical operation order (include/fmskf.h, the range section); fp32, every operation rounded
// on its own: the library is built with -ffp-contract=off and nothing here is an explicit fma,
// sqrt and the divisions are the correctly rounded ones.
#pragma once
#include "kf_generic.hpp"

#pragma clang fp contract(off)

namespace fmskf {

// The antenna against the anchor (ax, ay, az), on the position (px, py; plo: the low parts with
// COMP) and the heading's (c, s): the measurement row H (three coefficients) and the predicted
// distance d.  false: !(d >= d_min), the direction is undefined (a NaN d included) and H is not
// formed.
template <bool COMP>
__device__ __forceinline__ bool range_geometry(float px, float py, const float *plo, float c, float s,
                                               const float (&tag)[3], float ax, float ay, float az,
                                               float d_min, float (&H)[3], float &d) {
  const float rx = c * tag[0] - s * tag[1];
  const float ry = s * tag[0] + c * tag[1];
  const float dx = COMP ? ((px - ax) + plo[0]) + rx : (px - ax) + rx;
  const float dy = COMP ? ((py - ay) + plo[1]) + ry : (py - ay) + ry;
  const float dz = tag[2] - az;
  d = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
  if (!(d >= d_min)) return false;
  const float di = 1.0f / d;
  H[0] = dx * di;
  H[1] = dy * di;
  H[2] = (dy * rx - dx * ry) * di;
  return true;
}

// The scalar update with H = (H0, H1, H2, 0, ...): hp = H P (the high parts of P),
// S = H hp + r, si = 1 / S, g = y si, d2 = y g; applied when d2 <= d2_max (a NaN d2 never):
// x[j] += hp[j] g, P[i][j] -= (hp[i] si) hp[j].  A rejected measurement touches nothing.
// CI >= 0: state CI is compensated (x[CI] + *lo, th_add); CXM / CPM: the compensated states /
// packed P entries (slot_x, slot_p in clo), as in kf_update_seq.  Nothing is renormalised here
// (range_norm).
template <int CI, unsigned CXM, unsigned long long CPM, int N, int NP>
__device__ __forceinline__ bool range_update(float (&x)[N], float (&P)[NP], float *lo, float *clo,
                                             const float (&H)[3], float y, float r, float d2_max, float &d2) {
  float hp[N];
#pragma unroll
  for (int j = 0; j < N; j++) hp[j] = (H[0] * P[pk(0, j)] + H[1] * P[pk(1, j)]) + H[2] * P[pk(2, j)];
  const float S = ((H[0] * hp[0] + H[1] * hp[1]) + H[2] * hp[2]) + r;
  const float si = 1.0f / S;
  const float g = y * si;
  d2 = y * g;
  const bool apply = d2 <= d2_max;
  if (apply) {
#pragma unroll
    for (int j = 0; j < N; j++) {
      const float t = hp[j] * g;
      if (j == CI) th_add(x[j], *lo, t);
      else if ((CXM >> j) & 1u) th_add(x[j], clo[slot_x<CXM>(j)], t);
      else x[j] = x[j] + t;
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
      const float u = hp[i] * si;
#pragma unroll
      for (int j = 0; j <= i; j++) {
        const float t = u * hp[j];
        if ((CPM >> pk(i, j)) & 1ull) th_add(P[pk(i, j)], clo[slot_p<CXM, CPM>(pk(i, j))], -t);
        else P[pk(i, j)] = P[pk(i, j)] - t;
      }
    }
  }
  return apply;
}

// the compensated pairs renormalised after an applied entry: the state CI, then CXM / CPM
template <int CI, unsigned CXM, unsigned long long CPM, int N, int NP>
__device__ __forceinline__ void range_norm(float (&x)[N], float (&P)[NP], float *lo, float *clo) {
  if constexpr (CI >= 0) th_norm(x[CI], *lo);
  comp_norm<CXM, CPM>(x, P, clo);
}

}  // namespace fmskf
