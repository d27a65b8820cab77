// em_lane.hpp -- lane functions of the KF6 EM sufficient statistics (kernels_em.hip,
// fmskf_tick_many_em): the two sums the M-step of the EM algorithm for a linear-Gaussian model
// divides, taken over a smoothed window.
//
// With Pi = (P-[t+1])^-1, X = Pi Q and s = Q Pi (x_s[t+1] - x-[t+1]) -- all three formed by
// SmoothCarry::back (smooth_lane.hpp), which shows them through its tap -- the smoothed process
// noise of the step t -> t+1 is w = x_s[t+1] - F x_s[t] = s and
//   E[w w^T | all] = s s^T + (Q - Q Pi Q) + X^T P_s[t+1] X                    (sq, t = 0 .. T-2)
// which is the textbook s s^T + P_s[t+1] - F P_{t,t+1} - P_{t,t+1}^T F^T + F P_s[t] F^T with the
// lag-one covariance P_{t,t+1} = C P_s[t+1], written as a sum of three positive semidefinite terms:
// no cancellation while a prior is still the diffuse P0, as for the smoother's own recursion.  The
// measurement term of a measured tick is
//   v v^T + H P_s[t] H^T,  v = z - H x_s[t] (kf6_innov on x_s[t], heading wrapped)   (sr, t = 0 .. T-1)
// H selects the states (2, 5, 3, 4) (MdKF6::h1).
//
// Each tick's term is formed in fp32 like the smoother's numbers and added to an fp64 accumulator,
// so the sums do not lose accuracy with T.  The 31 accumulators do not fit next to the backward
// pass's registers at two waves per SIMD: 30 of them are per-lane LDS
// columns [30][256] of doubles, lane-major (a wave's 64 lanes read 64 consecutive doubles: no bank
// conflict), the 31st rides in two registers so that columns, sine table and reduction buffer stay
// inside 64 KiB of static LDS, two blocks per CU.  tests/em_ref.py restates the order in numpy.
#pragma once
#include "smooth_lane.hpp"
#include "window_lane.hpp"

#pragma clang fp contract(off)

namespace fmskf {

constexpr int kEmQ = 21, kEmR = 10, kEmAcc = kEmQ + kEmR, kEmLds = kEmAcc - 1;
constexpr int kEmTotal = 34;  // FMSKF_EM_TOTAL_LEN: n_trans, n_meas, left out, sq, sr

struct EmArgs {
  uint64_t n;
  TickIn in;
  Kf6Params prm;
  SmoothHist h;
  EmOut o;
};

// the lane's 31 sums: k < 21 sq (packed lower triangle), then sr
struct EmAcc {
  double *col;  // the lane's LDS column: accumulator k at col[k * kBlock]
  double last;  // accumulator kEmLds
  uint32_t n_meas;

  __device__ __forceinline__ void init(double *lds) {
    col = lds + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kEmLds; k++) col[k * kBlock] = 0.0;
    last = 0.0;
    n_meas = 0;
  }
  __device__ __forceinline__ void add(int k, float v) {
    if (k == kEmLds) last = last + (double)v;
    else col[k * kBlock] = col[k * kBlock] + (double)v;
  }
  __device__ __forceinline__ double get(int k) const { return k == kEmLds ? last : col[k * kBlock]; }

  // a measured tick t: v v^T + H P_s[t] H^T from the tick's smoothed estimate
  template <bool LIBM>
  __device__ __forceinline__ void measured(const Kf6In &m, const float *tab, const SmoothCarry<true> &c) {
    float v[4];
    kf6_innov<LIBM>(m, tab, c.x, v);
#pragma unroll
    for (int a = 0; a < 4; a++) {
#pragma unroll
      for (int b = 0; b <= a; b++)
        add(kEmQ + pk(a, b), dfma(v[a], v[b], c.P[pk(MdKF6::h1(a), MdKF6::h1(b))]));
    }
    n_meas++;
  }
};

// SmoothCarry::back's tap: the transition term of the step the call walks back over.
// gain() adds s s^T + X^T P_s[t+1] X, from the P_s[t+1] that back is about to overwrite: Y = P_s X
// column by column, each column's products added at once, so that no copy of the 21 values is held.
// noise() adds Q - Q Pi Q entry by entry as back forms it.
struct EmTap {
  EmAcc &acc;
  float s[6];
  __device__ __forceinline__ void resid(int i, float v) { s[i] = v; }
  __device__ __forceinline__ void gain(const float (&X)[6][6], const float (&Ps)[21]) {
#pragma unroll
    for (int j = 0; j < 6; j++) {
      float y[6];  // column j of P_s[t+1] X
#pragma unroll
      for (int l = 0; l < 6; l++) {
        float t = Ps[pk(l, 0)] * X[0][j];
#pragma unroll
        for (int k = 1; k < 6; k++) t = dfma(Ps[pk(l, k)], X[k][j], t);
        y[l] = t;
      }
#pragma unroll
      for (int i = j; i < 6; i++) {
        float t = s[i] * s[j];
#pragma unroll
        for (int l = 0; l < 6; l++) t = dfma(X[l][i], y[l], t);
        acc.add(pk(i, j), t);
      }
    }
  }
  __device__ __forceinline__ void noise(int i, int j, float v) { acc.add(pk(i, j), v); }
};

// The stores after tick 0 (ic: the lane's clamped robot, its chunk wave-uniform), then the block's
// partial totals (window_lane.hpp block_partials) of the lanes' fp64 values: zeros for a dead lane
// and for a robot left out, which counts in [2].  red: [wave][quantity].
__device__ __forceinline__ void em_store(const EmOut &o, uint64_t n, uint32_t ic, bool live, uint32_t n_trans,
                                         const EmAcc &c, double (*red)[kEmTotal]) {
  const uint32_t hb = gate_chunk(ic), li = ic - hb;
  const bool acc = o.accumulate != 0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < kEmAcc; k++) {
    const double v = c.get(k);
    bad = bad || !(__builtin_fabs(v) < __builtin_inf());
  }
  const double nan = __builtin_nan("");
  if (live) {
    if (o.n_meas) window_put<uint32_t>(o.n_meas, hb, n, li, acc, c.n_meas);
    if (o.sq) {
#pragma unroll
      for (int k = 0; k < kEmQ; k++)
        window_put<double>(o.sq + (uint64_t)k * o.pitch, hb, n, li, acc, bad ? nan : c.get(k));
    }
    if (o.sr) {
#pragma unroll
      for (int k = 0; k < kEmR; k++)
        window_put<double>(o.sr + (uint64_t)k * o.pitch, hb, n, li, acc, bad ? nan : c.get(kEmQ + k));
    }
  }
  if (o.partial) {
    const bool in = live && !bad;
    block_partials<kEmTotal>([&](int k) {
      const double v = k == 0 ? (double)n_trans : k == 1 ? (double)c.n_meas : k == 2 ? 1.0 : c.get(k - 3);
      return (k == 2 ? live && bad : in) ? v : 0.0;
    }, red, o.partial);
  }
}

}  // namespace fmskf
