// l5dh_counters_host.cpp -- host side of the counter space (the l5dh_counters_* entry points of
// include/l5dhist.h): the int64 values a context owns (l5dh_ctx::Counters) and the drivers of
// its batched add, its range calls and its rollup.  The kernels are in l5dh_counters.hip.
#include <algorithm>
#include <cerrno>
#include <memory>
#include <new>
#include <string>

#include "l5dh_ctx.hpp"

using namespace l5dh;

namespace {

using Counters = l5dh_ctx::Counters;

constexpr size_t CNT_MAX_BATCH = (size_t)1 << 30;

int no_counters(l5dh_ctx* c, const char* what) {
  return fail(c, -EINVAL, std::string(what) + ": the context has no counters");
}

int check_max(l5dh_ctx* c, const char* what, uint32_t max_counters) {
  static_assert(L5DH_MAX_COUNTERS == CNT_MAX, "the header's constant is the kernel's");
  static_assert(L5DH_NO_GROUP == CNT_NO_GROUP, "the header's constant is the kernel's");
  if (max_counters < 1 || max_counters > L5DH_MAX_COUNTERS)
    return fail(c, -EINVAL, std::string(what) + ": max_counters must be in [1, 2^24]");
  return 0;
}

int check_cnt_range(l5dh_ctx* c, const char* what, uint32_t first, uint32_t count) {
  if ((uint64_t)first + count > c->cnt->max) return fail(c, -EINVAL, std::string(what) + ": counter range out of bounds");
  return 0;
}

// A zeroed block of `max` values.
int new_values(l5dh_ctx* c, const char* what, uint32_t max, DevBuf& v) {
  if (!v.alloc((size_t)max * 8)) {
    (void)hipGetLastError();
    return fail(c, -ENOMEM, std::string(what) + ": hipMalloc of the values failed");
  }
  HIPCHK(c, hipMemsetAsync(v.p, 0, v.cap, c->stream));
  return 0;
}

// Wait until what has been enqueued so far has run (the caller's buffers are free again).
int wait_here(l5dh_ctx* c) {
  HIPCHK(c, hipEventRecord(c->ev_copy, c->stream));
  HIPCHK(c, hipEventSynchronize(c->ev_copy));
  return 0;
}

}  // namespace

namespace l5dh {

int counters_check(l5dh_ctx* c) {
  Counters& k = *c->cnt;
  uint64_t dropped = 0;
  HIPCHK(c, hipMemcpyAsync(&dropped, k.stats.as<uint64_t>() + CS_DROPPED, 8, hipMemcpyDeviceToHost, c->stream));
  if (int r = sync_stream(c)) return r;
  if (dropped != k.dropped_reported) {
    k.dropped_reported = dropped;
    return fail(c, -EINVAL, "counter id >= max_counters in a counters batch (those adds were dropped)");
  }
  return 0;
}

}  // namespace l5dh

extern "C" {

int l5dh_counters_open(l5dh_ctx* c, uint32_t max_counters) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (c->cnt) return fail(c, -EEXIST, "counters_open: the context already has counters");
  if (int r = check_max(c, "counters_open", max_counters)) return r;
  std::unique_ptr<Counters> k(new (std::nothrow) Counters());
  if (!k) return fail(c, -ENOMEM, "counters_open: out of host memory");
  if (set_counters_attributes() != hipSuccess) return fail(c, -EIO, "counters_open: the kernels' attributes");
  if (!k->stats.alloc(CS_WORDS * 8) || !k->status.alloc(4)) {
    (void)hipGetLastError();
    return fail(c, -ENOMEM, "counters_open: hipMalloc of the status words failed");
  }
  int r;
  if ((r = new_values(c, "counters_open", max_counters, k->values))) return r;
  HIPCHK(c, hipMemsetAsync(k->stats.p, 0, k->stats.cap, c->stream));
  if ((r = sync_stream(c))) return r;
  k->max = max_counters;
  c->cnt = std::move(k);
  return 0;
}

int l5dh_counters_close(l5dh_ctx* c) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (!c->cnt) return no_counters(c, "counters_close");
  if (int r = sync_stream(c)) return r;  // (before anything is freed)
  c->cnt.reset();
  return 0;
}

int l5dh_counters_resize(l5dh_ctx* c, uint32_t max_counters) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (!c->cnt) return no_counters(c, "counters_resize");
  Counters& k = *c->cnt;
  int r;
  if ((r = check_max(c, "counters_resize", max_counters))) return r;
  if (max_counters < k.max)
    return fail(c, -EINVAL,
                "counters_resize: " + std::to_string(max_counters) + " is below the space's " + std::to_string(k.max));
  if (max_counters == k.max) return 0;
  DevBuf v;
  if ((r = new_values(c, "counters_resize", max_counters, v))) return r;
  HIPCHK(c, hipMemcpyAsync(v.p, k.values.p, (size_t)k.max * 8, hipMemcpyDeviceToDevice, c->stream));
  if ((r = sync_stream(c))) return r;  // (before the old block is freed)
  k.values.swap(v);
  k.max = max_counters;
  return 0;
}

int l5dh_counters_add(l5dh_ctx* c, const uint32_t* ids, const int32_t* deltas, size_t n) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (!c->cnt) return no_counters(c, "counters_add");
  if (n > CNT_MAX_BATCH) return fail(c, -EINVAL, "counters_add: a batch larger than 2^30 adds");
  if (n && !ids) return fail(c, -EINVAL, "counters_add: null ids");
  if (n == 0) return 0;
  Counters& k = *c->cnt;
  // device inputs are stream ordered on a caller's stream; otherwise the call returns once
  // nothing of the caller's memory is still to be read
  const bool dev = direct(ids, 4) || (deltas && direct(deltas, 4));
  const bool host = !direct(ids, 4) || (deltas && !direct(deltas, 4));
  int r;
  {
    KTimer kt(c, L5DH_K_COPY);
    if ((r = stage_in(c, ids, n, 4, k.stage_ids)) || (r = stage_in(c, deltas, n, 4, k.stage_deltas))) return r;
  }
  if (host && (r = wait_here(c))) return r;  // (host buffers: their copies have completed)
  {
    KTimer kt(c, L5DH_K_COUNTERS);
    HIPCHK(c, launch_cnt_add(ids, deltas, n, k.values.as<int64_t>(), k.max, k.stats.as<uint64_t>(), c->G_max,
                             (c->variant & 8) != 0, c->stream));
  }
  if (dev && c->stream == c->own_stream) return wait_here(c);
  return 0;
}

int l5dh_counters_read(l5dh_ctx* c, uint32_t first, uint32_t count, int64_t* out) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (!c->cnt) return no_counters(c, "counters_read");
  if (int r = check_cnt_range(c, "counters_read", first, count)) return r;
  if (count && !out) return fail(c, -EINVAL, "counters_read: null out");
  if (count == 0) return 0;
  HIPCHK(c, hipMemcpyAsync(out, c->cnt->values.as<int64_t>() + first, (size_t)count * 8, hipMemcpyDefault, c->stream));
  return sync_stream(c);
}

int l5dh_counters_write(l5dh_ctx* c, uint32_t first, uint32_t count, const int64_t* values) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (!c->cnt) return no_counters(c, "counters_write");
  if (int r = check_cnt_range(c, "counters_write", first, count)) return r;
  if (count == 0) return 0;
  int64_t* dst = c->cnt->values.as<int64_t>() + first;
  if (values)
    HIPCHK(c, hipMemcpyAsync(dst, values, (size_t)count * 8, hipMemcpyDefault, c->stream));
  else
    HIPCHK(c, hipMemsetAsync(dst, 0, (size_t)count * 8, c->stream));
  return sync_stream(c);
}

int l5dh_counters_rollup(l5dh_ctx* c, uint32_t first, uint32_t count, const uint32_t* group, uint32_t ngroups,
                         int64_t* g_out) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (!c->cnt) return no_counters(c, "counters_rollup");
  Counters& k = *c->cnt;
  int r;
  if ((r = check_cnt_range(c, "counters_rollup", first, count))) return r;
  if (ngroups < 1 || ngroups > L5DH_MAX_COUNTERS) return fail(c, -EINVAL, "counters_rollup: ngroups must be in [1, 2^24]");
  if (!g_out) return fail(c, -EINVAL, "counters_rollup: null g_out");
  if (count && !group) return fail(c, -EINVAL, "counters_rollup: null group map");
  StagedOut<int64_t> out;
  if ((r = stage_in(c, group, count, 4, k.stage_group)) || (r = out.begin(c, g_out, ngroups, k.stage_out))) return r;
  uint32_t* status = k.status.as<uint32_t>();
  uint32_t hs = 0;
  {
    KTimer kt(c, L5DH_K_COUNTERS);
    HIPCHK(c, launch_cnt_rollup(k.values.as<const int64_t>() + first, count, group, ngroups, out.dev, status,
                                std::max(1, c->num_cu), c->stream));
  }
  // the status word, read after the kernel: the call's one wait
  HIPCHK(c, hipMemcpyAsync(&hs, status, 4, hipMemcpyDeviceToHost, c->stream));
  if ((r = out.end(c)) || (r = sync_stream(c))) return r;
  if (hs != 0xFFFFFFFFu)
    return fail(c, -EINVAL,
                "counters_rollup: group[" + std::to_string(hs) + "] is neither a group below " + std::to_string(ngroups) +
                    " nor L5DH_NO_GROUP");
  return 0;
}

int l5dh_counters_values(l5dh_ctx* c, const int64_t** device_ptr, uint32_t* max_counters) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (!c->cnt) return no_counters(c, "counters_values");
  if (device_ptr) *device_ptr = c->cnt->values.as<const int64_t>();
  if (max_counters) *max_counters = c->cnt->max;
  return 0;
}

int l5dh_counters_move(l5dh_ctx* from, l5dh_ctx* to) {
  if (!from || !to || from == to) return -EINVAL;
  // the two locks in address order
  l5dh_ctx* a = from < to ? from : to;
  l5dh_ctx* b = from < to ? to : from;
  std::lock_guard<std::mutex> ga(a->mu), gb(b->mu);
  if (!from->cnt) return no_counters(from, "counters_move");
  if (to->cnt) return fail(to, -EEXIST, "counters_move: the target already has counters");
  if (from->device != to->device) return fail(to, -EINVAL, "counters_move: the contexts are on different devices");
  hipSetDevice(to->device);
  int r;
  // queued adds have run; ids dropped and not yet reported are the target's to report
  if ((r = sync_stream(from))) return r;
  to->cnt = std::move(from->cnt);
  return 0;
}

int l5dh_counters_info(l5dh_ctx* c, uint32_t* max_counters, uint64_t* adds, uint64_t* lds_adds, uint64_t* global_adds,
                       uint64_t* dropped) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (!c->cnt) return no_counters(c, "counters_info");
  uint64_t s[CS_WORDS] = {0};
  HIPCHK(c, hipMemcpyAsync(s, c->cnt->stats.p, sizeof(s), hipMemcpyDeviceToHost, c->stream));
  if (int r = sync_stream(c)) return r;
  if (max_counters) *max_counters = c->cnt->max;
  if (adds) *adds = s[CS_ADDS];
  if (lds_adds) *lds_adds = s[CS_LDS];
  if (global_adds) *global_adds = s[CS_GLOBAL];
  if (dropped) *dropped = s[CS_DROPPED];
  return 0;
}

}  // extern "C"
