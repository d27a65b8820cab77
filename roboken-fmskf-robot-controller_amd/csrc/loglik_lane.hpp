// loglik_lane.hpp -- lane functions of the KF6 innovation log-likelihood (kernels_loglik.hip,
// fmskf_tick_many_loglik): the per-robot accumulators a window of ticks carries in registers, the
// tick that feeds them, and the stores after the window's last tick.
//
// Per measured tick the update's factor phase (kf_generic.hpp kf_update_factor) already holds
// w = L^-1 y and dinv = 1 / D of S = H P H^T + R = L D L^T, so
//   NIS       = kf_nis(w, dinv)                (the gate's value, bit for bit)
//   log det S = -sum_a log dinv[a]
// and the window's sums need no transcendental per tick:
//   * sum NIS is a compensated fp32 pair, every addition a TwoSum (th_add);
//   * sum log dinv is kept as E * ln 2 + log pm: frexp splits every dinv[a] exactly into a mantissa
//     in [0.5, 1) and an exponent; the four mantissas are multiplied in the fixed order
//     ((m0 m1) m2) m3, that product into the running mantissa pm, pm is split again, and every
//     exponent goes to the int32 E.  Four fp32 roundings per measured tick, each 2^-24 relative to
//     a factor of the product, i.e. 2^-24 absolute in the log domain; one fp64 log per robot and
//     launch, at the store.  (T = 2^23 measured ticks of exponents up to 128 each fit the int32.)
//   * the innovation sums (MOM): y[a] and the rounded products y[i] y[j], i >= j, each a
//     compensated fp32 pair like the NIS, so their error does not grow with the window either.
// A dinv[a] that is not a positive finite number, or a NaN NIS, sets the lane's sticky `bad` flag.
//
// tests/loglik_ref.py restates the scheme in numpy.
#pragma once
#include "window_lane.hpp"

#pragma clang fp contract(off)

namespace fmskf {

struct LoglikArgs {
  Kf6Args k;
  LoglikOut o;
};

template <bool MOM>
struct LoglikAcc {
  float nis_hi = 0.f, nis_lo = 0.f;
  float pm = 1.f;
  int32_t E = 0;
  uint32_t n = 0;
  bool bad = false;
  float s_hi[MOM ? 4 : 1], s_lo[MOM ? 4 : 1], o_hi[MOM ? 10 : 1], o_lo[MOM ? 10 : 1];

  __device__ __forceinline__ LoglikAcc() {
    if constexpr (MOM) {
#pragma unroll
      for (int a = 0; a < 4; a++) s_hi[a] = s_lo[a] = 0.f;
#pragma unroll
      for (int k = 0; k < 10; k++) o_hi[k] = o_lo[k] = 0.f;
    }
  }

  // one measured tick, from the factor phase's values
  __device__ __forceinline__ void add(const float (&y)[4], const float (&w)[4], const float (&dinv)[4]) {
    const float v = kf_nis(w, dinv);
    th_add(nis_hi, nis_lo, v);
    bad = bad || v != v;
    float m[4];
#pragma unroll
    for (int a = 0; a < 4; a++) {
      bad = bad || !(dinv[a] > 0.f && dinv[a] < __builtin_inff());
      m[a] = __builtin_amdgcn_frexp_mantf(dinv[a]);
      E += __builtin_amdgcn_frexp_expf(dinv[a]);
    }
    pm = pm * (((m[0] * m[1]) * m[2]) * m[3]);
    E += __builtin_amdgcn_frexp_expf(pm);
    pm = __builtin_amdgcn_frexp_mantf(pm);
    n++;
    if constexpr (MOM) {
#pragma unroll
      for (int a = 0; a < 4; a++) th_add(s_hi[a], s_lo[a], y[a]);
#pragma unroll
      for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) th_add(o_hi[pk(i, j)], o_lo[pk(i, j)], y[i] * y[j]);
      }
    }
  }

  // the window's sums as stored: NaN for a robot left out
  __device__ __forceinline__ double nis_sum() const {
    return bad ? __builtin_nan("") : (double)nis_hi + (double)nis_lo;
  }
  // 0 - (...): a window without a measured tick stores +0
  __device__ __forceinline__ double logdet_sum() const {
    return bad ? __builtin_nan("") : 0.0 - ((double)E * 0.69314718055994530942 + log((double)pm));
  }
};

// One tick: the gated tick's sequence (kf6_lane.hpp kf6_tick1) with the accumulators in place of
// the decision -- kf6_innov, kf_update_factor, the sums, kf_update_apply, which is kf_update bit
// for bit -- then kf6_tick1's plain predict.
template <class O, bool MOM>
__device__ __forceinline__ void loglik_tick1(const Kf6In &m, const float *tab, const Kf6Params &prm, float (&x)[6],
                                             float (&P)[21], LoglikAcc<MOM> &acc) {
  if (!O::VALID || m.valid) {
    float y[4], U[4][6], dinv[4], w[4];
    kf6_innov<O::LIBM>(m, tab, x, y);
    kf_update_factor<MdKF6>(P, y, prm.r, U, dinv, w);
    acc.add(y, w, dinv);
    kf_update_apply<MdKF6>(x, P, U, dinv, w);
  }
  const float dt = prm.dt;
  x[0] = dfma(dt, x[3], x[0]);
  x[1] = dfma(dt, x[4], x[1]);
  x[2] = wrap_pi(dfma(dt, x[5], x[2]));
  kf_predict_cov<MdKF6>(P, [&](int, int) { return dt; }, prm.q);
}

// The stores after the last tick (ic: the lane's clamped robot, its chunk wave-uniform), then the
// block's partial totals (window_lane.hpp block_partials) of the lanes' fp64 values: zeros for a
// dead lane and for a robot left out, which counts in [3].  red: [wave][quantity].
template <bool MOM>
__device__ __forceinline__ void loglik_store(const LoglikOut &o, uint64_t n, uint32_t ic, bool live,
                                             const LoglikAcc<MOM> &c, double (*red)[4]) {
  const uint32_t hb = gate_chunk(ic), li = ic - hb;
  const bool acc = o.accumulate != 0;
  const double nis = c.nis_sum(), ld = c.logdet_sum();
  if (live) {
    if (o.n_meas) window_put<uint32_t>(o.n_meas, hb, n, li, acc, c.n);
    if (o.nis_sum) window_put<double>(o.nis_sum, hb, n, li, acc, nis);
    if (o.logdet_sum) window_put<double>(o.logdet_sum, hb, n, li, acc, ld);
    if constexpr (MOM) {
      if (o.innov_sum) {
#pragma unroll
        for (int a = 0; a < 4; a++)
          window_put<double>(o.innov_sum + (uint64_t)a * o.pitch, hb, n, li, acc, (double)c.s_hi[a] + (double)c.s_lo[a]);
      }
      if (o.innov_outer) {
#pragma unroll
        for (int k = 0; k < 10; k++)
          window_put<double>(o.innov_outer + (uint64_t)k * o.pitch, hb, n, li, acc,
                             (double)c.o_hi[k] + (double)c.o_lo[k]);
      }
    }
  }
  if (o.partial) {
    const bool in = live && !c.bad;
    const double v[4] = {in ? (double)c.n : 0.0, in ? nis : 0.0, in ? ld : 0.0, live && c.bad ? 1.0 : 0.0};
    block_partials<4>([&](int k) { return v[k]; }, red, o.partial);
  }
}

}  // namespace fmskf
