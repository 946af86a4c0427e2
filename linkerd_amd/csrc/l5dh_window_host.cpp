// l5dh_window_host.cpp -- host side of the sliding window (the l5dh_window_* entry points of
// include/l5dhist.h): the ring of ended intervals a context owns (l5dh_ctx::Window) and the
// drivers of its push and query.  The kernels are in l5dh_window.hip; the export passes a
// push runs are the sparse export's (l5dh_import.hip).
#include <algorithm>
#include <cerrno>
#include <memory>
#include <new>
#include <string>

#include "l5dh_ctx.hpp"

using namespace l5dh;

namespace {

using Window = l5dh_ctx::Window;

// A block of at least `bytes` in `fresh` when `have` is too small: the slot's own buffer
// stays as it is until every allocation of the push has succeeded.
int win_room(l5dh_ctx* c, const DevBuf& have, size_t bytes, DevBuf& fresh) {
  if (have.cap >= bytes) return 0;
  if (!fresh.alloc((bytes + 4095) & ~(size_t)4095)) {
    (void)hipGetLastError();
    return fail(c, -ENOMEM, "window_push: hipMalloc of a slot's buffers failed");
  }
  return 0;
}

// The interval of series [0, count) into the ring's next slot.  The caller holds the lock.
int do_window_push(l5dh_ctx* c, uint32_t count, l5dh_summary* series_out) {
  Window& w = *c->win;
  Window::Slot& s = w.slot[w.head];
  int r = live_begin(c);
  if (r) return r;
  uint64_t total = 0;
  uint64_t* offs = nullptr;
  if (count) {
    // the entry count: the one host wait before the slot's buffers are sized
    auto rows = [&](uint32_t* cnt) { return export_sparse_count(state(c), 0, count, cnt, c->stream); };
    if ((r = count_scan(c, count, c->xs_cnt, c->xs_offs, c->xs_tmp, rows, &total))) return r;
    offs = c->xs_offs.as<uint64_t>();
  }
  // room for the interval: the slot's buffers are reused when large enough, else replaced --
  // after every allocation has succeeded, so a failure leaves the ring as it was
  DevBuf n_off, n_ent, n_tot;
  if ((r = win_room(c, s.row_off, ((size_t)count + 1) * 8, n_off)) || (r = win_room(c, s.entries, (size_t)total * 8, n_ent)) ||
      (r = win_room(c, s.totals, (size_t)count * 8, n_tot)))
    return r;
  StagedOut<Summary88> summ;
  if ((r = summ.begin(c, series_out, count, c->stage_summ))) return r;
  if (n_off.p) s.row_off.swap(n_off);  // (the stream is idle: every entry point ends in a wait)
  if (n_ent.p) s.entries.swap(n_ent);
  if (n_tot.p) s.totals.swap(n_tot);
  s.count = 0;  // (not a valid interval until the pass below has completed)
  s.n_entries = s.seq = 0;
  if (count) {
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, hipMemcpyAsync(s.row_off.p, offs, ((size_t)count + 1) * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, export_sparse_write(state(c), 0, count, offs, s.entries.as<BucketEntry>(), s.totals.as<int64_t>(),
                                  c->stream));
    // the interval's summaries and the reset of the same range, from the same state
    if ((r = rows_of_range(c, 0, count, summ.dev, 1))) return r;
  }
  if ((r = summ.end(c)) || (r = sync_stream(c))) return r;
  s.count = count;
  s.n_entries = total;
  s.seq = ++w.pushes;
  w.head = (w.head + 1) % w.slots;
  w.filled = std::min(w.filled + 1, w.slots);
  return 0;
}

// The summed rows of series [first, first + count) over the `last` most recent slots (+ the
// open interval).  The caller holds the lock and has checked the arguments; count > 0.
int do_window_query(l5dh_ctx* c, uint32_t first, uint32_t count, uint32_t last, int include_open, l5dh_summary* out,
                    int32_t* counts_out, int64_t* totals_out) {
  Window& w = *c->win;
  int r;
  if (include_open && (r = live_begin(c))) return r;
  StagedOut<Summary88> summ;
  StagedOut<int32_t> cnt;
  StagedOut<int64_t> tot;
  // (the copies are not timed here, as in l5dh_summarize_dense and l5dh_le)
  if ((r = summ.begin(c, out, count, c->stage_summ)) || (r = cnt.begin(c, counts_out, (size_t)count * NB, c->stage_counts)) ||
      (r = tot.begin(c, totals_out, count, c->stage_totals)))
    return r;
  WinSlots ws{};
  ws.n = last;
  for (uint32_t k = 0; k < last; ++k) {  // slot k of the call: the k-th most recent push
    const Window::Slot& s = w.slot[(w.head + w.slots - 1 - k) % w.slots];
    ws.row_off[k] = s.row_off.as<const uint64_t>();
    ws.entries[k] = s.entries.as<const BucketEntry>();
    ws.totals[k] = s.totals.as<const int64_t>();
    ws.seq[k] = s.seq;
    ws.count[k] = s.count;
  }
  uint32_t* status = w.status.as<uint32_t>();
  uint32_t hs = 0;
  {
    KTimer kt(c, L5DH_K_WINDOW);
    HIPCHK(c, hipMemsetAsync(status, 0xFF, 4, c->stream));
    HIPCHK(c, launch_win_sum(ws, w.born.as<const uint64_t>(), state(c), first, count, include_open, tables(c), cnt.dev,
                             tot.dev, summ.dev, status, c->stream));
  }
  // the status word, read after the kernel: the call's one wait
  HIPCHK(c, hipMemcpyAsync(&hs, status, 4, hipMemcpyDeviceToHost, c->stream));
  if ((r = summ.end(c)) || (r = cnt.end(c)) || (r = tot.end(c)) || (r = sync_stream(c))) return r;
  if (hs != 0xFFFFFFFFu)
    return fail(c, -ERANGE, "window_query: a bucket sum of series " + std::to_string(hs) + " exceeds 2^31 - 1");
  return 0;
}

int no_window(l5dh_ctx* c, const char* what) { return fail(c, -EINVAL, std::string(what) + ": the context has no window"); }

}  // namespace

extern "C" {

int l5dh_window_open(l5dh_ctx* c, uint32_t slots) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  static_assert(L5DH_WINDOW_MAX == WIN_MAX, "the header's constant is the kernel's");
  if (c->win) return fail(c, -EEXIST, "window_open: the context already has a window");
  if (slots < 1 || slots > L5DH_WINDOW_MAX) return fail(c, -EINVAL, "window_open: slots must be in [1, 64]");
  std::unique_ptr<Window> w(new (std::nothrow) Window());
  if (!w) return fail(c, -ENOMEM, "window_open: out of host memory");
  w->slots = slots;
  w->slot.reset(new (std::nothrow) Window::Slot[slots]);
  if (!w->slot || !w->born.alloc((size_t)c->S * 8) || !w->status.alloc(4)) {
    (void)hipGetLastError();
    return fail(c, -ENOMEM, "window_open: hipMalloc of the ring failed");
  }
  w->born_n = c->S;
  HIPCHK(c, hipMemsetAsync(w->born.p, 0, (size_t)c->S * 8, c->stream));
  if (int r = sync_stream(c)) return r;
  c->win = std::move(w);
  return 0;
}

int l5dh_window_close(l5dh_ctx* c) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (!c->win) return no_window(c, "window_close");
  if (int r = sync_stream(c)) return r;  // (before anything is freed)
  c->win.reset();
  return 0;
}

int l5dh_window_push(l5dh_ctx* c, uint32_t count, l5dh_summary* series_out) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (!c->win) return no_window(c, "window_push");
  if (int r = check_range(c, 0, count)) return r;
  static_assert(sizeof(l5dh_summary) == sizeof(Summary88), "l5dh_summary layout");
  return do_window_push(c, count, series_out);
}

int l5dh_window_query(l5dh_ctx* c, uint32_t first, uint32_t count, uint32_t last, int include_open, l5dh_summary* out,
                      int32_t* counts_out, int64_t* totals_out) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (!c->win) return no_window(c, "window_query");
  if (int r = check_range(c, first, count)) return r;
  if (last > c->win->filled)
    return fail(c, -EINVAL,
                "window_query: last = " + std::to_string(last) + ", the ring holds " + std::to_string(c->win->filled) +
                    " intervals");
  if (last == 0 && !include_open) return fail(c, -EINVAL, "window_query: last = 0 without the open interval");
  if (count == 0) return 0;
  return do_window_query(c, first, count, last, include_open, out, counts_out, totals_out);
}

int l5dh_window_forget(l5dh_ctx* c, uint32_t first, uint32_t count) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (!c->win) return no_window(c, "window_forget");
  if (int r = check_range(c, first, count)) return r;
  HIPCHK(c, launch_win_born(c->win->born.as<uint64_t>(), first, count, c->win->pushes, c->stream));
  return sync_stream(c);
}

int l5dh_window_move(l5dh_ctx* from, l5dh_ctx* to) {
  if (!from || !to || from == to) return -EINVAL;
  // the two locks in address order
  l5dh_ctx* a = from < to ? from : to;
  l5dh_ctx* b = from < to ? to : from;
  std::lock_guard<std::mutex> ga(a->mu), gb(b->mu);
  if (!from->win) return no_window(from, "window_move");
  if (to->win) return fail(to, -EEXIST, "window_move: the target already has a window");
  if (from->device != to->device) return fail(to, -EINVAL, "window_move: the contexts are on different devices");
  Window& w = *from->win;
  for (uint32_t k = 0; k < w.slots; ++k)
    if (w.slot[k].count > to->S)
      return fail(to, -EINVAL,
                  "window_move: a slot holds " + std::to_string(w.slot[k].count) + " series, the target " +
                      std::to_string(to->S));
  hipSetDevice(to->device);
  int r;
  if ((r = sync_stream(from))) return r;
  // the forget marks, extended with zeros to the target's series count
  DevBuf born;
  if (!born.alloc((size_t)to->S * 8)) {
    (void)hipGetLastError();
    return fail(to, -ENOMEM, "window_move: hipMalloc of the forget marks failed");
  }
  const size_t keep = std::min<size_t>(w.born_n, to->S);
  HIPCHK(to, hipMemsetAsync(born.p, 0, (size_t)to->S * 8, to->stream));
  HIPCHK(to, hipMemcpyAsync(born.p, w.born.p, keep * 8, hipMemcpyDeviceToDevice, to->stream));
  if ((r = sync_stream(to))) return r;
  w.born.swap(born);
  w.born_n = to->S;
  to->win = std::move(from->win);
  return 0;
}

int l5dh_window_info(l5dh_ctx* c, uint32_t* slots, uint32_t* filled, uint64_t* pushes, uint64_t* entries,
                     uint64_t* bytes) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (!c->win) return no_window(c, "window_info");
  const Window& w = *c->win;
  uint64_t ne = 0, nb = w.born.cap + w.status.cap;
  for (uint32_t k = 0; k < w.slots; ++k) {
    const Window::Slot& s = w.slot[k];
    ne += s.n_entries;
    nb += s.row_off.cap + s.entries.cap + s.totals.cap;
  }
  if (slots) *slots = w.slots;
  if (filled) *filled = w.filled;
  if (pushes) *pushes = w.pushes;
  if (entries) *entries = ne;
  if (bytes) *bytes = nb;
  return 0;
}

}  // extern "C"
