// api_fix.cpp -- fmskf_correct_pose: absolute pose fixes for a listed subset of robots
// (argument checks, the host list's validation, staging, the launch of kernels_fix.hip).
#include "api_ctx.hpp"

using namespace fmskf;
using namespace fmskf::capi;

extern "C" {

int fmskf_correct_pose(fmskf_handle h, const fmskf_pose_fix *fixes, uint64_t count,
                       const fmskf_pose_fix_params *prm, float *nis, uint8_t *status, uint32_t mem) {
  return guarded([&] {
    check_handle(h);
    check_list_model(h, "pose fixes are");
    if (!prm) fail(FMSKF_EINVAL, "null fix parameters");
    if (prm->flags & ~FMSKF_FIX_HEADING) fail(FMSKF_EINVAL, "unknown FMSKF_FIX_* flags");
    const uint32_t m = (prm->flags & FMSKF_FIX_HEADING) ? 3u : 2u;
    for (uint32_t i = 0; i < m; i++)
      for (uint32_t j = 0; j <= i; j++) {
        const double v = prm->r[i * (i + 1) / 2 + j];
        if (!isfinite(v) || (i == j && !(v > 0.0))) fail(FMSKF_EINVAL, "fix noise must be finite with a positive diagonal");
      }
    if (!(prm->nis_max > 0.0f)) fail(FMSKF_EINVAL, "nis_max must be > 0 (+INFINITY: no gate)");
    if (mem != FMSKF_MEM_HOST && mem != FMSKF_MEM_DEVICE) fail(FMSKF_EINVAL, "bad mem flag");
    if (count == 0) return;
    if (!fixes) fail(FMSKF_EINVAL, "null fix list");
    const uint64_t n = h->s.n;
    // a strictly ascending list of robots below N has at most N entries
    if (count > n) fail(FMSKF_EINVAL, "more fixes than robots");
    const bool host = mem == FMSKF_MEM_HOST;
    if (!host && ((uintptr_t)fixes & 15) != 0) fail(FMSKF_EINVAL, "a device fix list must be 16-byte aligned");
    if (host) {
      if (h->capturing) fail(FMSKF_EINVAL, "a host fix list cannot be captured");
      for (uint64_t k = 0; k < count; k++) {
        if (fixes[k].robot >= n) fail(FMSKF_EINVAL, "fix list: robot >= N");
        if (k && fixes[k].robot <= fixes[k - 1].robot) fail(FMSKF_EINVAL, "fix list: robot not strictly ascending");
      }
    }
    DeviceGuard g(h->cfg.device);
    PoseFixDev f{};
    f.count = count;
    f.ignored = h->fix_ignored;
    for (int k = 0; k < 6; k++) f.r[k] = (float)prm->r[k];  // narrowed to the model's element type
    f.nis_max = prm->nis_max;
    f.m = m;
    const void *list = fixes;
    Stager sg(h, mem);
    sg.add(&list, (size_t)count * sizeof(fmskf_pose_fix));
    sg.run();
    f.fixes = (const uint32_t *)list;
    EntryOut out(h, nis, status, count, mem);
    f.nis = out.value;
    f.status = out.status;
    h->time_begin();
    launch_check(launch_pose_fix(h->s, f, h->stream), "pose fix kernel launch");
    h->time_end();
    out.deliver();
  });
}

}  // extern "C"
