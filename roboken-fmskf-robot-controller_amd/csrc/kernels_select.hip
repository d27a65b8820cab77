// kernels_select.hip -- robots selected by their state (fmskf_select) and the state of listed
// robots read or overwritten (fmskf_get_state_subset / fmskf_set_state_subset), KF6 and EKF9 for
// gfx950.
//
// fmskf_select writes the selected robots in ascending order, so an atomic append will not do, and
// no block waits on another block of its launch (no look-back, no spin flags): four launches.
//   k_sel_flag    one lane per robot, 256-robot blocks, the tiled rows addressed as the tick
//                 kernels address them (TileRows: one wave-uniform descriptor per block, a scalar
//                 offset per row).  Only the rows the requested criteria need are loaded -- a
//                 compile-time choice for NONFINITE (27 / 54 rows) and POS_VAR (packed P rows 0
//                 and 2), a wave-uniform one for the gate word -- with the cache policy of the
//                 model's tick launcher.  Writes the reason byte of every robot and the block's
//                 count (ballots, then four wave counts through LDS).
//   k_sel_chunks  the sum of every 256 block counts (2^30 robots: 2^22 counts, 2^14 sums)
//   k_sel_top     one block: the exclusive scan of the chunk sums, in place, and *count
//   k_sel_emit    block b of a chunk sums the counts of the blocks before it in the chunk (at most
//                 255 words), adds the chunk's offset, re-reads its flags, ranks the selected
//                 lanes (ballot + mbcnt in the wave, the waves through LDS) and stores robot and
//                 reason where the index is below `capacity`.  A block that selected nothing
//                 leaves after one load.
//
// The subset kernel is one lane per listed robot, addressed per lane through FixRows
// (list_rows.hpp) as the pose-fix kernel; a malformed entry (robot >= N, or not above its
// predecessor) is skipped and counted.
//
// Every kernel takes an argument struct of its own: nothing is added to the tick kernels'.
#include "list_rows.hpp"

#pragma clang fp contract(off)

namespace fmskf {

struct SelArgs {
  uint64_t n;
  float *x, *P;
  SelectDev d;
  uint32_t nb;  // 256-robot blocks
  uint32_t nc;  // chunks of kSelChunk block counts
};

static_assert(kSelChunk == kBlock, "one block count per lane of a chunk's block");

__device__ __forceinline__ uint32_t lane_rank(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the sum of v over the block's 256 lanes, in every lane (two barriers)
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *lds4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();  // lds4 may still be read from an earlier use
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds4[0] + lds4[1] + lds4[2] + lds4[3];
}

// NX: 6 (KF6) or 9 (EKF9); SP: the FMSKF_SEL_NONFINITE / FMSKF_SEL_POS_VAR bits of the call
template <int NX, uint32_t SP, int CP>
__global__ __launch_bounds__(kBlock) void k_sel_flag(SelArgs a) {
  constexpr int NP = NX * (NX + 1) / 2;
  __shared__ uint32_t wcnt[kBlock / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < a.n;
  const uint32_t t = tile_slot(a.n);
  uint32_t reason = 0;
  float p00 = 0.f, p11 = 0.f;
  if constexpr ((SP & FMSKF_SEL_NONFINITE) != 0) {
    const TileRows<float, NX, CP> tx(a.x, t);
    const TileRows<float, NP, CP> tp(a.P, t);
    uint32_t mag = 0;  // the largest |bits|: NaN and Inf are those at or above the Inf pattern
#pragma unroll
    for (int k = 0; k < NX; k++) mag = max(mag, __builtin_bit_cast(uint32_t, tx.ld(k)) & 0x7FFFFFFFu);
#pragma unroll
    for (int k = 0; k < NP; k++) {
      const float v = tp.ld(k);
      if (k == 0) p00 = v;
      if (k == 2) p11 = v;
      mag = max(mag, __builtin_bit_cast(uint32_t, v) & 0x7FFFFFFFu);
    }
    if (mag >= 0x7F800000u) reason |= FMSKF_SEL_NONFINITE;
  } else if constexpr ((SP & FMSKF_SEL_POS_VAR) != 0) {
    const TileRows<float, NP, CP> tp(a.P, t);
    p00 = tp.ld(0);
    p11 = tp.ld(2);
  }
  if constexpr ((SP & FMSKF_SEL_POS_VAR) != 0) {
    const float s = p00 + p11;
    if (s > a.d.pos_var_min) reason |= FMSKF_SEL_POS_VAR;  // a NaN sum does not select
  }
  if (a.d.criteria & FMSKF_SEL_GATE_RUN) {
    if constexpr (NX == 6) {
      const uint32_t w = live ? a.d.gate_word[i] : 0u;
      if (((w >> kGateRunShift) & kGateRunMax) >= a.d.run_min) reason |= FMSKF_SEL_GATE_RUN;
    } else {
      const uint64_t w = live ? a.d.rowgate_word[i] : 0ull;
      bool hit = false;
#pragma unroll
      for (int r = 0; r < FMSKF_EKF9_ROWS; r++)
        hit |= ((a.d.row_mask >> r) & 1u) && ((uint32_t)(w >> (kRowGateRunShift + 8 * r)) & kRowGateRunMax) >= a.d.run_min;
      if (hit) reason |= FMSKF_SEL_GATE_RUN;
    }
  }
  if (!live) reason = 0;
  if (live) a.d.flag[i] = (uint8_t)reason;
  const unsigned long long m = __ballot(reason != 0);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) a.d.blk[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// chunk c: the sum of block counts [c * 256, c * 256 + 256)
__global__ __launch_bounds__(kBlock) void k_sel_chunks(SelArgs a) {
  __shared__ uint32_t lds4[kBlock / 64];
  const uint32_t b = blockIdx.x * kSelChunk + threadIdx.x;
  const uint32_t s = block_sum(b < a.nb ? a.d.blk[b] : 0u, lds4);
  if (threadIdx.x == 0) a.d.chunk[blockIdx.x] = s;
}

// one block: chunk sums -> their exclusive scan, in place; the total to *count.  Lane t owns the
// contiguous span of ceil(nc / 256) sums (64 at the 2^30-robot cap).
__global__ __launch_bounds__(kBlock) void k_sel_top(SelArgs a) {
  __shared__ uint32_t part[kBlock];
  const uint32_t span = (a.nc + kBlock - 1) / kBlock;
  const uint32_t lo = min(threadIdx.x * span, a.nc), hi = min(lo + span, a.nc);
  uint32_t s = 0;
  for (uint32_t c = lo; c < hi; c++) s += a.d.chunk[c];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {  // 256 partial sums: a serial scan by one lane
    uint32_t run = 0;
    for (int k = 0; k < kBlock; k++) {
      const uint32_t v = part[k];
      part[k] = run;
      run += v;
    }
    *a.d.count = run;
  }
  __syncthreads();
  uint32_t run = part[threadIdx.x];
  for (uint32_t c = lo; c < hi; c++) {
    const uint32_t v = a.d.chunk[c];
    a.d.chunk[c] = run;
    run += v;
  }
}

__global__ __launch_bounds__(kBlock) void k_sel_emit(SelArgs a) {
  __shared__ uint32_t lds4[kBlock / 64], wcnt[kBlock / 64];
  const uint32_t b = blockIdx.x;
  if (a.d.blk[b] == 0) return;  // block-uniform
  // the selected robots of the blocks before this one: the chunk's offset, then the counts of the
  // chunk's earlier blocks
  const uint32_t first = b & ~(kSelChunk - 1);
  const uint32_t before = block_sum(first + threadIdx.x < b ? a.d.blk[first + threadIdx.x] : 0u, lds4);
  const uint64_t i = (uint64_t)b * kBlock + threadIdx.x;
  const uint32_t reason = i < a.n ? a.d.flag[i] : 0u;
  const unsigned long long m = __ballot(reason != 0);
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wcnt[w] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t waves = 0;
#pragma unroll
  for (uint32_t k = 0; k < kBlock / 64; k++) waves += k < w ? wcnt[k] : 0u;
  const uint64_t at = (uint64_t)a.d.chunk[b / kSelChunk] + before + waves + lane_rank(m);
  if (reason != 0 && at < a.d.capacity) {
    a.d.robots[at] = (uint32_t)i;
    if (a.d.reason) a.d.reason[at] = (uint8_t)reason;
  }
}

template <int NX, int CP>
static void launch_flag(const SelArgs &a, hipStream_t st) {
  const dim3 g(a.nb);
  switch (a.d.criteria & (FMSKF_SEL_NONFINITE | FMSKF_SEL_POS_VAR)) {
    case 0: k_sel_flag<NX, 0, CP><<<g, kBlock, 0, st>>>(a); break;
    case FMSKF_SEL_NONFINITE: k_sel_flag<NX, FMSKF_SEL_NONFINITE, CP><<<g, kBlock, 0, st>>>(a); break;
    case FMSKF_SEL_POS_VAR: k_sel_flag<NX, FMSKF_SEL_POS_VAR, CP><<<g, kBlock, 0, st>>>(a); break;
    default: k_sel_flag<NX, FMSKF_SEL_NONFINITE | FMSKF_SEL_POS_VAR, CP><<<g, kBlock, 0, st>>>(a); break;
  }
}

int launch_select(const DevState &s, const SelectDev &d, hipStream_t st) {
  const ListRegime rg = list_regime(s);
  if (!rg.ok) return (int)hipErrorNotSupported;
  const bool ekf = rg.ekf, nt = rg.nt;
  if (!d.flag || !d.blk || !d.chunk || !d.count || (d.capacity && !d.robots)) return (int)hipErrorInvalidValue;
  if ((d.criteria & FMSKF_SEL_GATE_RUN) && !(ekf ? (const void *)d.rowgate_word : (const void *)d.gate_word))
    return (int)hipErrorInvalidValue;
  SelArgs a{s.n, (float *)s.x, (float *)s.P, d, 0, 0};
  a.nb = grid_for(s.n).x;
  a.nc = (a.nb + kSelChunk - 1) / kSelChunk;
  if (ekf) nt ? launch_flag<9, kStateNT>(a, st) : launch_flag<9, 0>(a, st);
  else nt ? launch_flag<6, kStateNT>(a, st) : launch_flag<6, 0>(a, st);
  k_sel_chunks<<<a.nc, kBlock, 0, st>>>(a);
  k_sel_top<<<1, kBlock, 0, st>>>(a);
  if (d.capacity) k_sel_emit<<<a.nb, kBlock, 0, st>>>(a);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// the state of listed robots
// ---------------------------------------------------------------------------
struct SubArgs {
  uint64_t n;
  uint64_t pitch;
  float *x, *P;
  float *thlo;  // EKF9: [N] heading low part
  float *lo;    // KF6 + FMSKF_CFG_COMP_POS: the tiled low-part rows
  SubsetDev d;
};

// NX: 6 (KF6) or 9 (EKF9, one low row: the heading's); COMP: KF6's five position low rows;
// SET: the caller's columns are written into the state, with fmskf_set_state's restarts of the low
// parts; otherwise the state is read into the caller's columns
template <int NX, bool COMP, int CP, bool BIG, bool SET>
__global__ __launch_bounds__(kBlock) void k_subset(SubArgs a) {
  constexpr int NP = NX * (NX + 1) / 2;
  constexpr bool EKF = NX == 9;
  static_assert(!(EKF && COMP), "EKF9 with FMSKF_CFG_COMP_POS is not supported");
  const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t cnt = a.d.count;
  const bool have = k < cnt;
  uint32_t robot = 0, prev = 0;
  if (have) {
    robot = a.d.robots[k];
    if (k > 0) prev = a.d.robots[k - 1];
  }
  const bool ok = have && robot < a.n && (k == 0 || robot > prev);
  if (ok) {
    float *ux = a.d.x ? a.d.x + k : nullptr, *up = a.d.p ? a.d.p + k : nullptr, *ul = a.d.lo ? a.d.lo + k : nullptr;
    if (ux) {
      const FixRows<NX, CP, BIG> tx(a.x, a.pitch, robot);
      float v[NX];  // every load in flight before the first store
#pragma unroll
      for (int j = 0; j < NX; j++) v[j] = SET ? ux[(size_t)j * cnt] : tx.ld(j);
#pragma unroll
      for (int j = 0; j < NX; j++) {
        if constexpr (SET) tx.st(j, v[j]);
        else ux[(size_t)j * cnt] = v[j];
      }
    }
    if (up) {
      const FixRows<NP, CP, BIG> tp(a.P, a.pitch, robot);
      float v[NP];
#pragma unroll
      for (int j = 0; j < NP; j++) v[j] = SET ? up[(size_t)j * cnt] : tp.ld(j);
#pragma unroll
      for (int j = 0; j < NP; j++) {
        if constexpr (SET) tp.st(j, v[j]);
        else up[(size_t)j * cnt] = v[j];
      }
    }
    if constexpr (COMP) {
      // set: a given x or P restarts the position low parts at 0, a given lo replaces that
      if (SET ? (ux || up || ul) : ul != nullptr) {
        const FixRows<(int)kKf6LoRows, CP, BIG> tl(a.lo, a.pitch, robot);
#pragma unroll
        for (int j = 0; j < (int)kKf6LoRows; j++) {
          if constexpr (SET) tl.st(j, ul ? ul[(size_t)j * cnt] : 0.f);
          else ul[(size_t)j * cnt] = tl.ld(j);
        }
      }
    }
    if constexpr (EKF) {
      // set: a given x restarts the heading low part at 0, a given lo replaces that
      if (SET ? (ux || ul) : ul != nullptr) {
        const ThLo<CP, BIG> th{a.thlo, a.n, robot};
        if constexpr (SET) th.st(ul ? *ul : 0.f);
        else *ul = th.ld();
      }
    }
  }
  count_ignored(have && !ok, a.d.ignored);
}

int launch_state_subset(const DevState &s, const SubsetDev &d, hipStream_t st) {
  const ListRegime rg = list_regime(s);
  if (!rg.ok) return (int)hipErrorNotSupported;
  if (!d.robots || !d.count || !d.ignored) return (int)hipErrorInvalidValue;
  if (d.lo && !rg.ekf && !rg.comp) return (int)hipErrorInvalidValue;
  const SubArgs a{s.n, s.pitch, (float *)s.x, (float *)s.P, s.thlo, s.xlo, d};
  with_list_regime(
      rg,
      [&](auto NX, auto COMP, auto CP, auto BIG, auto SET) {
        k_subset<NX(), COMP(), CP(), BIG(), SET()><<<grid_for(a.d.count), kBlock, 0, st>>>(a);
      },
      d.set);
  return (int)hipGetLastError();
}

}  // namespace fmskf
