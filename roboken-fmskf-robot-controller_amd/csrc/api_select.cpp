// api_select.cpp -- fmskf_select (robots selected by their state, as an ascending list) and
// fmskf_get_state_subset / fmskf_set_state_subset (the state of listed robots): argument checks,
// the host list's validation, staging, the launches of kernels_select.hip.
#include "api_ctx.hpp"

using namespace fmskf;
using namespace fmskf::capi;

namespace {

// the checks and the launch shared by the subset get and set; x / p / lo are the caller's
void state_subset(fmskf_ctx *h, const uint32_t *robots, uint64_t count, const float *x, const float *p,
                  const float *lo, uint32_t mem, bool set) {
  check_handle(h);
  check_list_model(h, set ? "fmskf_set_state_subset is" : "fmskf_get_state_subset is");
  if (mem != FMSKF_MEM_HOST && mem != FMSKF_MEM_DEVICE) fail(FMSKF_EINVAL, "bad mem flag");
  const uint32_t lrows = h->s.thlo ? 1u : h->s.xlo ? kKf6LoRows : 0u;
  if (lo && !lrows) fail(FMSKF_EINVAL, "this model keeps no low-part rows");
  if (count == 0) return;
  if (!robots) fail(FMSKF_EINVAL, "null robot list");
  const uint64_t n = h->s.n;
  // a strictly ascending list of robots below N has at most N entries
  if (count > n) fail(FMSKF_EINVAL, "more listed robots than robots");
  const bool host = mem == FMSKF_MEM_HOST;
  if (!host && ((uintptr_t)robots & 3) != 0) fail(FMSKF_EINVAL, "a device robot list must be 4-byte aligned");
  if (host) {
    if (h->capturing) fail(FMSKF_EINVAL, "a host robot list cannot be captured");
    for (uint64_t k = 0; k < count; k++) {
      if (robots[k] >= n) fail(FMSKF_EINVAL, "robot list: robot >= N");
      if (k && robots[k] <= robots[k - 1]) fail(FMSKF_EINVAL, "robot list: not strictly ascending");
    }
  }
  if (!x && !p && !lo) return;
  DeviceGuard g(h->cfg.device);
  const uint32_t nx = h->d.nx, np = nx * (nx + 1) / 2;
  const size_t bx = x ? (size_t)nx * count * 4 : 0, bp = p ? (size_t)np * count * 4 : 0,
               bl = lo ? (size_t)lrows * count * 4 : 0;
  SubsetDev d{};
  d.count = count;
  d.ignored = h->subset_ignored;
  d.set = set;
  const void *list = robots, *sx = x, *sp = p, *sl = lo;
  Stager sg(h, mem);
  sg.add(&list, (size_t)count * 4);
  if (set) {
    sg.add(&sx, bx);
    sg.add(&sp, bp);
    sg.add(&sl, bl);
  }
  sg.run();
  d.robots = (const uint32_t *)list;
  char *res = nullptr;
  if (host && !set) {  // the planes gathered into device scratch, then copied out
    res = (char *)h->out_for(bx + bp + bl);
    d.x = x ? (float *)res : nullptr;
    d.p = p ? (float *)(res + bx) : nullptr;
    d.lo = lo ? (float *)(res + bx + bp) : nullptr;
  } else {
    d.x = (float *)sx;
    d.p = (float *)sp;
    d.lo = (float *)sl;
  }
  h->time_begin();
  launch_check(launch_state_subset(h->s, d, h->stream), "state subset kernel launch");
  h->time_end();
  if (set && x) h->ens_shift_ok = false;
  if (res) {
    copy_out(h, (void *)x, d.x, bx, mem);
    copy_out(h, (void *)p, d.p, bp, mem);
    copy_out(h, (void *)lo, d.lo, bl, mem);
  }
  finish_out(h, mem);
}

}  // namespace

extern "C" {

int fmskf_select(fmskf_handle h, const fmskf_select_params *prm, uint32_t *robots, uint8_t *reason,
                 uint64_t capacity, uint64_t *count, uint32_t mem) {
  return guarded([&] {
    check_handle(h);
    check_list_model(h, "fmskf_select is");
    if (!prm) fail(FMSKF_EINVAL, "null select parameters");
    const uint32_t all = FMSKF_SEL_NONFINITE | FMSKF_SEL_POS_VAR | FMSKF_SEL_GATE_RUN;
    if ((prm->criteria & ~all) || !(prm->criteria & all)) fail(FMSKF_EINVAL, "criteria: FMSKF_SEL_* bits, at least one");
    if ((prm->criteria & FMSKF_SEL_POS_VAR) && prm->pos_var_min != prm->pos_var_min)
      fail(FMSKF_EINVAL, "pos_var_min is NaN");
    const bool ekf = h->cfg.model == FMSKF_MODEL_EKF9, run = (prm->criteria & FMSKF_SEL_GATE_RUN) != 0;
    if (run && (prm->run_min < 1 || prm->run_min > 255)) fail(FMSKF_EINVAL, "run_min must be 1..255");
    if (ekf && run) {
      if (!prm->row_mask || (prm->row_mask & ~0x3Fu)) fail(FMSKF_EINVAL, "row_mask must be a nonzero subset of 0x3F");
    } else if (prm->row_mask) {
      fail(FMSKF_EINVAL, "row_mask goes with FMSKF_SEL_GATE_RUN on EKF9 only");
    }
    if (run && !(ekf ? h->rowgate_on : h->gate_on))
      fail(FMSKF_EINVAL, ekf ? "FMSKF_SEL_GATE_RUN needs a row gate (fmskf_set_row_gate)"
                             : "FMSKF_SEL_GATE_RUN needs a gate (fmskf_set_gate)");
    if (mem != FMSKF_MEM_HOST && mem != FMSKF_MEM_DEVICE) fail(FMSKF_EINVAL, "bad mem flag");
    if (!count) fail(FMSKF_EINVAL, "null count");
    if (capacity && !robots) fail(FMSKF_EINVAL, "null robots with capacity > 0");
    if (h->capturing) fail(FMSKF_EINVAL, "fmskf_select cannot be captured");
    const bool host = mem == FMSKF_MEM_HOST;
    if (!host && (((uintptr_t)count & 7) != 0 || ((uintptr_t)robots & 3) != 0))
      fail(FMSKF_EINVAL, "device count must be 8-byte, robots 4-byte aligned");
    DeviceGuard g(h->cfg.device);
    const uint64_t n = h->s.n;
    const size_t nb = (size_t)((n + kBlock - 1) / kBlock), nc = (nb + kSelChunk - 1) / kSelChunk;
    if (!h->sel_flag) {  // scratch sized by N, on first use
      h->sel_flag = h->alloc<uint8_t>(n);
      h->sel_blk = h->alloc<uint32_t>(nb);
      h->sel_chunk = h->alloc<uint32_t>(nc);
    }
    SelectDev d{};
    d.criteria = prm->criteria;
    d.pos_var_min = prm->pos_var_min;
    d.run_min = prm->run_min;
    d.row_mask = prm->row_mask;
    d.gate_word = h->gate_on ? h->gate.word : nullptr;
    d.rowgate_word = h->rowgate_on ? h->rowgate.word : nullptr;
    d.flag = h->sel_flag;
    d.blk = h->sel_blk;
    d.chunk = h->sel_chunk;
    // a list holds at most N robots, whatever the capacity
    const uint64_t cap = std::min<uint64_t>(capacity, n);
    d.capacity = cap;
    char *res = nullptr;
    if (host) {  // device scratch: count, robots [cap], reason [cap]
      res = (char *)h->out_for(8 + (size_t)cap * 5);
      d.count = (uint64_t *)res;
      d.robots = cap ? (uint32_t *)(res + 8) : nullptr;
      d.reason = cap && reason ? (uint8_t *)(res + 8 + (size_t)cap * 4) : nullptr;
    } else {
      d.count = count;
      d.robots = robots;
      d.reason = reason;
    }
    h->time_begin();
    launch_check(launch_select(h->s, d, h->stream), "select kernel launch");
    h->time_end();
    if (host) {  // the count first: only the list's entries are copied out
      uint64_t total = 0;
      copy_out_sync(h, &total, res, 8, mem);
      const uint64_t got = std::min<uint64_t>(total, cap);
      if (got) {
        copy_out(h, robots, d.robots, (size_t)got * 4, mem);
        copy_out(h, reason, d.reason, (size_t)got, mem);
        finish_out(h, mem);
      }
      *count = total;
    }
  });
}

int fmskf_get_state_subset(fmskf_handle h, const uint32_t *robots, uint64_t count, float *x, float *p_packed,
                           float *lo, uint32_t mem) {
  return guarded([&] { state_subset(h, robots, count, x, p_packed, lo, mem, false); });
}

int fmskf_set_state_subset(fmskf_handle h, const uint32_t *robots, uint64_t count, const float *x,
                           const float *p_packed, const float *lo, uint32_t mem) {
  return guarded([&] { state_subset(h, robots, count, x, p_packed, lo, mem, true); });
}

}  // extern "C"
