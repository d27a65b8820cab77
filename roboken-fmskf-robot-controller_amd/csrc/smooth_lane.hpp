// smooth_lane.hpp -- lane functions of the KF6 fixed-interval smoother (kernels_smooth.hip): the
// history of per-tick priors the forward pass writes and the backward pass reads, and the backward
// recursion of the smoothed estimate.
//
// The backward pass is the Rauch-Tung-Striebel recursion in a form without cancellation.  With
// (x-[t], P-[t]) the prior of tick t, (x+[t], P+[t]) its filtered state, Pi = (P-[t+1])^-1 and
// C = P+[t] F^T Pi the smoother gain, P-[t+1] = F P+[t] F^T + Q gives C = F^-1 (I - Q Pi) and
//   x_s[t] = x+[t] + F^-1 (I - Q Pi) (x_s[t+1] - x-[t+1])
//   P_s[t] = F^-1 (Q - Q Pi Q + (I - Q Pi) P_s[t+1] (I - Q Pi)^T) F^-T
// (P+ + C (P_s[t+1] - P-[t+1]) C^T with P+ - C P-[t+1] C^T = F^-1 (Q - Q Pi Q) F^-T; F^-1 = I - dt E
// exactly, since F = I + dt E with E E = 0).  P_s[t] is a sum of two positive semidefinite terms
// and needs neither P+[t] nor the tick's inputs; x_s[t] stays anchored to the forward pass's own
// x+[t], which is rebuilt from the prior and the inputs with the forward update's arithmetic.
// Pi is applied through an LDL^T factor of P-[t+1] (6 x 6, no square roots, like the update's).
//
// Why not the adjoint (Bryson-Frazier) form x_s = x+ - P+ lambda, P_s = P+ - P+ Lambda P+, which
// needs no 6 x 6 factor: while a robot's covariance is still the diffuse P0 (heading variance 1)
// and its ticks are invalid, P+ = P- = P0 and the smoothed heading variance (1e-6) is the
// difference of two numbers near 1.  In fp32 that form returned variances off by 6e-6, negative
// for one robot in two that starts on an invalid tick (tests/smooth_ref.py, the window straight
// from reset()); so does the textbook P+ + C (P_s - P-) C^T.  The form above deviates 2e-9 there.
//
// fp32 throughout, explicit fused multiply-adds in ascending-index sums like kf_generic.hpp;
// tests/smooth_ref.py restates the order in numpy.
#pragma once
#include "kf6_lane.hpp"

#pragma clang fp contract(off)

namespace fmskf {

// The history (fmskf_internal.hpp SmoothHist): tick t's priors laid out like the state itself.
// One tick's slice of 2^20 robots is 113 MB, so the offset of a slice is 64-bit scalar arithmetic
// folded into the descriptor base; within a slice one descriptor per tile, a scalar offset per
// row, a 32-bit lane offset below 8 KiB.  Written once and read once, and larger than the
// Infinity Cache for any window worth smoothing: non-temporal both ways (kStateNT).
struct SmoothFwdArgs {
  Kf6Args k;
  SmoothHist h;
};
struct SmoothBwdArgs {
  uint64_t n;
  TickIn in;
  Kf6Params prm;
  SmoothHist h;
  SmoothOut o;
};

// ic: the lane's clamped robot (its tile is wave-uniform, kf6_load_state); live: the lane stores
__device__ __forceinline__ void hist_store(const SmoothHist &h, uint32_t t, uint32_t ic, bool live,
                                           const float (&x)[6], const float (&P)[21]) {
  constexpr uint32_t W = tile_w<float>();
  constexpr int SP = st_pol(kStateNT);
  const uint32_t tl = (uint32_t)__builtin_amdgcn_readfirstlane(ic / W);
  const uint32_t c = (ic - tl * W) * 4u;
  const auto rx = rsrc(h.x + (uint64_t)t * h.sx + (uint64_t)tl * (6 * W), 6 * W * 4);
  const auto rp = rsrc(h.P + (uint64_t)t * h.sp + (uint64_t)tl * (21 * W), 21 * W * 4);
  if (live) {
#pragma unroll
    for (int k = 0; k < 6; k++) st_f32<SP>(rx, c, k * W * 4, x[k]);
#pragma unroll
    for (int k = 0; k < 21; k++) st_f32<SP>(rp, c, k * W * 4, P[k]);
  }
}
__device__ __forceinline__ void hist_load(const SmoothHist &h, uint32_t t, uint32_t ic, float (&x)[6],
                                          float (&P)[21]) {
  constexpr uint32_t W = tile_w<float>();
  const uint32_t tl = (uint32_t)__builtin_amdgcn_readfirstlane(ic / W);
  const uint32_t c = (ic - tl * W) * 4u;
  const auto rx = rsrc(h.x + (uint64_t)t * h.sx + (uint64_t)tl * (6 * W), 6 * W * 4);
  const auto rp = rsrc(h.P + (uint64_t)t * h.sp + (uint64_t)tl * (21 * W), 21 * W * 4);
#pragma unroll
  for (int k = 0; k < 6; k++) x[k] = ld_f32<kStateNT>(rx, c, k * W * 4);
#pragma unroll
  for (int k = 0; k < 21; k++) P[k] = ld_f32<kStateNT>(rp, c, k * W * 4);
}

// ROWS dense rows of tick t at base + (t * ROWS + k) * pitch: a descriptor per row over the
// block's chunk (hb its first robot, wave-uniform; li the lane's slot), so neither the tick nor
// the row enters a 32-bit offset at any pitch; coalesced per row, non-temporal
template <int ROWS>
__device__ __forceinline__ void smooth_store(float *base, uint32_t t, uint64_t pitch, uint64_t n, uint32_t hb,
                                             uint32_t li, bool live, const float (&v)[ROWS]) {
  float *row = base + (uint64_t)t * ROWS * pitch + hb;
  if (live) {
#pragma unroll
    for (int k = 0; k < ROWS; k++)
      st_f32<st_pol(kStateNT)>(rsrc(row + (uint64_t)k * pitch, (n - hb) * 4), li * 4u, 0, v[k]);
  }
}

// P = L D L^T of a packed symmetric 6 x 6 (the recurrence of kf_update_factor: E = L D is the
// pre-division value): L unit lower (set below the diagonal only), dinv = 1 / D
__device__ __forceinline__ void smooth_ldl6(const float (&P)[21], float (&L)[6][6], float (&dinv)[6]) {
  float E[6][6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int j = 0; j <= i; j++) {
      float s = P[pk(i, j)];
#pragma unroll
      for (int k = 0; k < j; k++) s = dfma(-L[i][k], E[j][k], s);
      if (i == j) {
        dinv[i] = 1.0f / s;
      } else {
        E[i][j] = s;
        L[i][j] = s * dinv[j];
      }
    }
  }
}
// v <- P^-1 v: forward substitution, the scaling, back substitution
__device__ __forceinline__ void smooth_solve6(const float (&L)[6][6], const float (&dinv)[6], float (&v)[6]) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    float s = v[i];
#pragma unroll
    for (int k = 0; k < i; k++) s = dfma(-L[i][k], v[k], s);
    v[i] = s;
  }
#pragma unroll
  for (int i = 0; i < 6; i++) v[i] = v[i] * dinv[i];
#pragma unroll
  for (int i = 4; i >= 0; i--) {
    float s = v[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) s = dfma(-L[k][i], v[k], s);
    v[i] = s;
  }
}

// What SmoothCarry::back shows of its intermediates to a caller that needs them (em_lane.hpp: the
// EM statistics are built from them); the smoother itself passes this one, whose calls are empty
struct SmoothNoTap {
  // s = Q Pi (x_s[t+1] - x-[t+1]), component i
  __device__ __forceinline__ void resid(int, float) {}
  // X = Pi Q, with Ps still P_s[t+1]
  __device__ __forceinline__ void gain(const float (&)[6][6], const float (&)[21]) {}
  // (Q - Q Pi Q)(i, j), j <= i
  __device__ __forceinline__ void noise(int, int, float) {}
};

// The smoothed estimate of the tick behind the current one, carried down the window.  WP: P_s
// exists (the call forms it)
template <bool WP>
struct SmoothCarry {
  float x[6];
  float P[WP ? 21 : 1];

  // the window's last tick: its filtered state, the heading wrapped into [-pi, pi)
  __device__ __forceinline__ void start(const float (&xf)[6], const float (&Pf)[21]) {
#pragma unroll
    for (int k = 0; k < 6; k++) x[k] = xf[k];
    x[2] = wrap_pi(x[2]);
    if constexpr (WP) {
#pragma unroll
      for (int k = 0; k < 21; k++) P[k] = Pf[k];
    }
  }

  // From tick t+1 (held) to tick t, as far as the prior of t+1 (x1, P1) takes it: P becomes
  // P_s[t]; e = F^-1 (I - Q Pi) (x_s[t+1] - x-[t+1]), the heading difference wrapped as the
  // innovation is.  The x path is the same operations with and without P_s.
  __device__ __forceinline__ void back(const float (&x1)[6], const float (&P1)[21], const float *Q, float dt,
                                       float (&e)[6]) {
    SmoothNoTap tap;
    back(x1, P1, Q, dt, e, tap);
  }
  template <class Tap>
  __device__ __forceinline__ void back(const float (&x1)[6], const float (&P1)[21], const float *Q, float dt,
                                       float (&e)[6], Tap &tap) {
    float L[6][6], dinv[6], d[6], pd[6];
    smooth_ldl6(P1, L, dinv);
#pragma unroll
    for (int i = 0; i < 6; i++) pd[i] = d[i] = x[i] - x1[i];
    pd[2] = d[2] = wrap_innov(d[2]);
    smooth_solve6(L, dinv, pd);
#pragma unroll
    for (int i = 0; i < 6; i++) {
      float s = Q[pk(i, 0)] * pd[0];
#pragma unroll
      for (int k = 1; k < 6; k++) s = dfma(Q[pk(i, k)], pd[k], s);
      tap.resid(i, s);
      e[i] = d[i] - s;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
      for (int k = 0; k < 6; k++)
        if (MdKF6::pat(i, k)) e[i] = dfma(-dt, e[k], e[i]);
    }
    if constexpr (WP) {
      float X[6][6];  // Pi Q, column by column
#pragma unroll
      for (int j = 0; j < 6; j++) {
        float c[6];
#pragma unroll
        for (int k = 0; k < 6; k++) c[k] = Q[pk(k, j)];
        smooth_solve6(L, dinv, c);
#pragma unroll
        for (int k = 0; k < 6; k++) X[k][j] = c[k];
      }
      tap.gain(X, P);
      float A[6][6];  // I - Q Pi = I - X^T
#pragma unroll
      for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j < 6; j++) A[i][j] = (i == j ? 1.0f : 0.0f) - X[j][i];
      }
      float M[6][6];  // A P_s[t+1]
#pragma unroll
      for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int l = 0; l < 6; l++) {
          float s = A[i][0] * P[pk(0, l)];
#pragma unroll
          for (int k = 1; k < 6; k++) s = dfma(A[i][k], P[pk(k, l)], s);
          M[i][l] = s;
        }
      }
      float G[21];  // Q - Q Pi Q + A P_s[t+1] A^T
#pragma unroll
      for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
          float s = Q[pk(i, 0)] * X[0][j];
#pragma unroll
          for (int k = 1; k < 6; k++) s = dfma(Q[pk(i, k)], X[k][j], s);
          s = Q[pk(i, j)] - s;
          tap.noise(i, j, s);
#pragma unroll
          for (int l = 0; l < 6; l++) s = dfma(M[i][l], A[j][l], s);
          G[pk(i, j)] = s;
        }
      }
      float T1[6][6];  // F^-1 G
#pragma unroll
      for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j < 6; j++) {
          float s = G[pk(i, j)];
#pragma unroll
          for (int k = 0; k < 6; k++)
            if (MdKF6::pat(i, k)) s = dfma(-dt, G[pk(k, j)], s);
          T1[i][j] = s;
        }
      }
#pragma unroll
      for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
          float s = T1[i][j];
#pragma unroll
          for (int k = 0; k < 6; k++)
            if (MdKF6::pat(j, k)) s = dfma(-dt, T1[i][k], s);
          P[pk(i, j)] = s;
        }
      }
    }
  }

  // x_s[t] = x+[t] + e, the heading wrapped into [-pi, pi)
  __device__ __forceinline__ void finish(const float (&xf)[6], const float (&e)[6]) {
#pragma unroll
    for (int k = 0; k < 6; k++) x[k] = xf[k] + e[k];
    x[2] = wrap_pi(x[2]);
  }
};

// The filtered state of a tick from a copy of its prior (x, P) and its inputs, in place: the
// forward update itself (kf6_innov, kf_update: the forward pass's bits).  Returns whether the tick
// was measured.  The callers copy the prior themselves, since they keep it for the next tick down
// ("What the window calls share", on why the copy is not made in here).
template <class O>
__device__ __forceinline__ bool smooth_filtered(const Kf6Params &prm, const float *stab, const Kf6In &m,
                                                float (&xf)[6], float (&Pf)[21]) {
  const bool meas = !O::VALID || m.valid;
  if (meas) {
    float y[4];
    kf6_innov<O::LIBM>(m, stab, xf, y);
    kf_update<MdKF6>(xf, Pf, y, prm.r);
  }
  return meas;
}

}  // namespace fmskf
