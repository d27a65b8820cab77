// window_lane.hpp -- what the kernels that replay a window of KF6 ticks and return sums over it
// share (kernels_loglik.hip, kernels_em.hip): the store of one per-robot value, the block's partial
// fleet totals and their fold.
//
// The fleet total is deterministic: every block reduces its lanes' fp64 values in a fixed tree and
// writes one partial per quantity (block_partials); k_window_fold, one block, adds the partials in
// block order.  No floating-point atomics.  tests/loglik_ref.py and tests/em_ref.py restate the
// tree in numpy (fleet_fold).
#pragma once
#include "kf6_lane.hpp"

#pragma clang fp contract(off)

namespace fmskf {

// one value of a per-robot plane (or of a row of a multi-row plane) at the lane's slot of its
// 256-robot chunk: overwritten, or with the call's accumulate flag old + new
template <typename T>
__device__ __forceinline__ void window_put(T *plane, uint32_t hb, uint64_t n, uint32_t li, bool acc, T v) {
  if (acc) v = ld_chunk<T, 0>(plane, hb, n, li) + v;
  st_chunk<T, st_pol(0)>(plane, hb, n, li, v);
}

// The block's partial totals of K quantities.  value(k): the lane's fp64 value of quantity k (zero
// for a lane that does not count).  A fixed butterfly inside each wave, d = 1, 2, .. 32 -- every
// lane ends with the same sum, since a + b is b + a -- then the four waves' sums added in wave
// order, one thread per quantity: partial[k * gridDim.x + blockIdx.x].  red: [wave][quantity].
template <int K, class V>
__device__ __forceinline__ void block_partials(V value, double (*red)[K], double *partial) {
  static_assert(K <= kBlock && kBlock == 4 * 64, "one thread per quantity, four waves");
  double v[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    v[k] = value(k);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v[k] = v[k] + __shfl_xor(v[k], d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) red[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    partial[(uint64_t)k * gridDim.x + blockIdx.x] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// total[k] = (old +) the nb block partials of quantity k added in block order from 0.0, k < K: the
// block stages CHUNK partials of each quantity in LDS (coalesced loads), thread k adds its row in
// order.  The order of the additions is the contract, the chunk only sizes the LDS.
template <int K, uint32_t CHUNK>
__global__ __launch_bounds__(kBlock) void k_window_fold(const double *partial, uint32_t nb, double *total,
                                                        uint32_t accumulate) {
  __shared__ double buf[K][CHUNK];
  double s = 0.0;
  for (uint32_t b0 = 0; b0 < nb; b0 += CHUNK) {
    const uint32_t m = min(CHUNK, nb - b0);
    for (uint32_t idx = threadIdx.x; idx < K * CHUNK; idx += kBlock) {
      const uint32_t k = idx / CHUNK, j = idx % CHUNK;
      if (j < m) buf[k][j] = partial[(uint64_t)k * nb + b0 + j];
    }
    __syncthreads();
    if (threadIdx.x < K) {
      for (uint32_t j = 0; j < m; j++) s = s + buf[threadIdx.x][j];
    }
    __syncthreads();
  }
  if (threadIdx.x < K) total[threadIdx.x] = accumulate ? total[threadIdx.x] + s : s;
}

}  // namespace fmskf
