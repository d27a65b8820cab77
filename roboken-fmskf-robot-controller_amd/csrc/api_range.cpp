// api_range.cpp -- range updates against surveyed anchors: the handle's anchor table
// (fmskf_set_anchors / fmskf_get_anchors) and fmskf_correct_range (argument checks, the host
// list's validation, staging, the launch of kernels_range.hip).
#include "api_ctx.hpp"

using namespace fmskf;
using namespace fmskf::capi;

extern "C" {

int fmskf_set_anchors(fmskf_handle h, const float *xyz, uint32_t count) {
  return guarded([&] {
    check_handle(h);
    if (count > FMSKF_RANGE_ANCHORS_MAX) fail(FMSKF_EINVAL, "more anchors than FMSKF_RANGE_ANCHORS_MAX");
    if (count && !xyz) fail(FMSKF_EINVAL, "null anchor coordinates");
    if (h->capturing) fail(FMSKF_EINVAL, "anchors changed inside a graph capture");
    for (uint32_t k = 0; k < 3 * count; k++)
      if (!isfinite(xyz[k])) fail(FMSKF_EINVAL, "anchor coordinates must be finite");
    std::vector<float> rows((size_t)count * 4, 0.f);  // 16-byte rows: x, y, z, 0
    for (uint32_t k = 0; k < count; k++)
      for (int c = 0; c < 3; c++) rows[(size_t)k * 4 + c] = xyz[(size_t)k * 3 + c];
    DeviceGuard g(h->cfg.device);
    // ordered on the handle's stream behind the calls that read the old table; the source is a
    // pinned input slot (16 KiB at most), released by the event behind this copy
    if (count) {
      char *pin = h->pinned_in();
      memcpy(pin, rows.data(), rows.size() * sizeof(float));
      hip_check(hipMemcpyAsync(h->anchors, pin, rows.size() * sizeof(float), hipMemcpyHostToDevice, h->stream),
                "anchor upload");
    }
    h->anchors_host.swap(rows);
    h->n_anchors = count;
  });
}

int fmskf_get_anchors(fmskf_handle h, float *xyz, uint32_t capacity, uint32_t *count) {
  return guarded([&] {
    check_handle(h);
    if (capacity && !xyz) fail(FMSKF_EINVAL, "null anchor buffer");
    const uint32_t m = std::min(capacity, h->n_anchors);
    for (uint32_t k = 0; k < m; k++)
      for (int c = 0; c < 3; c++) xyz[(size_t)k * 3 + c] = h->anchors_host[(size_t)k * 4 + c];
    if (count) *count = h->n_anchors;
  });
}

int fmskf_correct_range(fmskf_handle h, const fmskf_range_fix *fixes, uint64_t count,
                        const fmskf_range_params *prm, float *d2, uint8_t *status, uint32_t mem) {
  return guarded([&] {
    check_handle(h);
    check_list_model(h, "range updates are");
    if (!prm) fail(FMSKF_EINVAL, "null range parameters");
    if (prm->flags || prm->reserved) fail(FMSKF_EINVAL, "range flags and reserved must be 0");
    if (!isfinite(prm->var_m2) || !(prm->var_m2 > 0.0f)) fail(FMSKF_EINVAL, "var_m2 must be finite and > 0");
    if (!(prm->d2_max > 0.0f)) fail(FMSKF_EINVAL, "d2_max must be > 0 (+INFINITY: no gate)");
    if (!isfinite(prm->d_min) || !(prm->d_min > 0.0f)) fail(FMSKF_EINVAL, "d_min must be finite and > 0");
    for (int c = 0; c < 3; c++)
      if (!isfinite(prm->tag[c])) fail(FMSKF_EINVAL, "the tag offset must be finite");
    if (mem != FMSKF_MEM_HOST && mem != FMSKF_MEM_DEVICE) fail(FMSKF_EINVAL, "bad mem flag");
    if (h->n_anchors == 0) fail(FMSKF_EINVAL, "no anchors set (fmskf_set_anchors)");
    if (count == 0) return;
    if (!fixes) fail(FMSKF_EINVAL, "null range list");
    const uint64_t n = h->s.n;
    // a non-descending list of robots below N with runs of at most FMSKF_RANGE_RUN_MAX
    if (count > (uint64_t)FMSKF_RANGE_RUN_MAX * n) fail(FMSKF_EINVAL, "more ranges than FMSKF_RANGE_RUN_MAX per robot");
    const bool host = mem == FMSKF_MEM_HOST;
    if (!host && ((uintptr_t)fixes & 15) != 0) fail(FMSKF_EINVAL, "a device range list must be 16-byte aligned");
    if (host) {
      if (h->capturing) fail(FMSKF_EINVAL, "a host range list cannot be captured");
      uint64_t run = 0;
      for (uint64_t k = 0; k < count; k++) {
        if (fixes[k].robot >= n) fail(FMSKF_EINVAL, "range list: robot >= N");
        if (k && fixes[k].robot < fixes[k - 1].robot) fail(FMSKF_EINVAL, "range list: robot descending");
        run = (k && fixes[k].robot == fixes[k - 1].robot) ? run + 1 : 1;
        if (run > FMSKF_RANGE_RUN_MAX) fail(FMSKF_EINVAL, "range list: more than FMSKF_RANGE_RUN_MAX entries of one robot");
        if (fixes[k].anchor >= h->n_anchors) fail(FMSKF_EINVAL, "range list: anchor index outside the table");
      }
    }
    DeviceGuard g(h->cfg.device);
    RangeDev f{};
    f.count = count;
    f.anchors = h->anchors;
    f.n_anchors = h->n_anchors;
    f.ignored = h->range_ignored;
    for (int c = 0; c < 3; c++) f.tag[c] = prm->tag[c];
    f.var = prm->var_m2;
    f.d2_max = prm->d2_max;
    f.d_min = prm->d_min;
    const void *list = fixes;
    Stager sg(h, mem);
    sg.add(&list, (size_t)count * sizeof(fmskf_range_fix));
    sg.run();
    f.fixes = (const uint32_t *)list;
    EntryOut out(h, d2, status, count, mem);
    f.d2 = out.value;
    f.status = out.status;
    h->time_begin();
    launch_check(launch_range_fix(h->s, f, h->cfg.trig == FMSKF_TRIG_LIBM, h->stream), "range kernel launch");
    h->time_end();
    out.deliver();
  });
}

}  // extern "C"
