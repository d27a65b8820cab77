// list_rows.hpp -- the tiled state rows of one robot addressed per lane, for the kernels that
// work on a list of robots (kernels_fix.hip: fmskf_correct_pose; kernels_range.hip:
// fmskf_correct_range; kernels_select.hip: the subset get / set).
//
// The state is tiled [ceil(N / 2048)][rows][2048] (fmskf_internal.hpp st_at) and a wave's listed
// robots lie in arbitrary tiles, so the wave-uniform per-chunk descriptors of the tick kernels do
// not apply.  Each array is one descriptor over the whole array (kernel arguments only, so it
// stays in SGPRs), the lane's row-0 byte offset is its voffset and row k the scalar offset
// k * 2048 * 4: one address register per array and the state's cache policy in the aux bits.  An
// array past 4 GiB (KF6 beyond 51 M robots, EKF9 beyond 23 M) cannot be reached through 32-bit
// offsets: the BIG form uses 64-bit lane addresses and non-temporal accesses (such a state is
// always streamed).
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

// the largest tiled array of a KF6 / EKF9 state (P) within reach of a 32-bit byte offset?
inline bool rows_big(bool ekf, uint64_t pitch) {
  return (uint64_t)(ekf ? 45 : 21) * pitch * sizeof(float) > 0xFFFFFFFFull;
}

}  // namespace fmskf
