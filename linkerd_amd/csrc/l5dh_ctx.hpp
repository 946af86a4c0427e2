// l5dh_ctx.hpp -- private to the host side (l5dh_engine.cpp, l5dh_queries.cpp,
// l5dh_fleet.cpp, l5dh_window_host.cpp, l5dh_counters_host.cpp): the context behind the C-ABI's opaque l5dh_ctx, the owner of its
// device memory, and the helpers the files share (defined in l5dh_engine.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/l5dhist.h"
#include "l5dh_counters.hpp"
#include "l5dh_import.hpp"
#include "l5dh_influx.hpp"
#include "l5dh_kernels.hpp"
#include "l5dh_le.hpp"
#include "l5dh_merge.hpp"
#include "l5dh_quant.hpp"
#include "l5dh_render.hpp"
#include "l5dh_rollup.hpp"
#include "l5dh_top.hpp"
#include "l5dh_window.hpp"

namespace l5dh {

// Move-only owner of one hipMalloc block.  Freed with the context (after ~l5dh_ctx has
// synchronized the stream); whoever frees earlier -- ensure(), release() callers --
// synchronizes the context's stream first.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { swap(o); }  // (move-only: the copies are implicitly deleted)
  DevBuf& operator=(DevBuf&& o) noexcept { return swap(o), *this; }  // (o then frees the old block)
  ~DevBuf() { release(); }
  void swap(DevBuf& o) { std::swap(p, o.p), std::swap(cap, o.cap); }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
  }
  // A fixed allocation (l5dh_open): at least 256 bytes.
  bool alloc(size_t bytes) {
    release();
    bytes = bytes < 256 ? 256 : bytes;
    if (hipMalloc(&p, bytes) != hipSuccess) p = nullptr;
    cap = p ? bytes : 0;
    return p != nullptr;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

// A DevBuf of one element type: reads as the T* it replaces.
template <class T>
struct DevArr : DevBuf {
  operator T*() const { return as<T>(); }
};

}  // namespace l5dh

struct l5dh_ctx {
  template <class T>
  using Arr = l5dh::DevArr<T>;
  using DevBuf = l5dh::DevBuf;

  std::mutex mu;
  int device = 0;
  int num_cu = 256;
  uint32_t S = 0, F = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t side = nullptr;       // cold-tile accumulation runs here beside the hot tiles
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipStream_t stream = nullptr;
  std::string last_error;

  // tables
  Arr<int32_t> d_lim_pad, d_mid, d_base;
  Arr<uint32_t> d_lut;
  Arr<uint2> d_lut2;
  // state
  Arr<uint32_t> d_counts;
  Arr<int64_t> d_total, d_sumfix;
  Arr<uint8_t> d_dirty;
  Arr<uint32_t> d_err;
  // scratch
  Arr<uint32_t> d_tile_tot;  // [F] tile totals (snapshot plan)
  Arr<uint4> d_cold_item;
  DevBuf split_item;  // big-tile half chunk items (sized per snapshot)
  Arr<uint32_t> d_hot_list;
  Arr<uint8_t> d_tile_flags;
  Arr<uint32_t> d_header;
  Arr<uint32_t> d_enc_base;  // [F] sparse export: each tile's first word of the unpacked encoding
  Arr<uint32_t> d_enc_h0;    // [F] sparse export: words reserved for half 0 of a big or dirty tile
  Arr<uint32_t> d_enc_dw;    // [2F] sparse export: words of each half of a dirty tile's state rows
  uint32_t* h_header = nullptr;      // pinned: [PIN_ERR] ingest error count (written by k_rfix1), [PIN_BIG] big tiles of the last plan
  uint32_t* h_header_dev = nullptr;  // its device-side address
  Arr<uint32_t> d_kest;   // [2F] sampled ids per (tile, half) key of the batch being binned
  Arr<uint32_t> d_kprev;  // [2F] exact records per key of the previous batch (region sizes)
  int G_max = 256;
  // segments: binned batches awaiting the snapshot
  struct Seg {
    DevBuf rec32, rec16;
    Arr<uint32_t> meta;  // [meta_layout(F).words()]
    size_t n = 0;
  };
  Seg segs[l5dh::MAX_SEG];
  int nseg = 0;
  int max_seg = 4;
  uint32_t direct_max = l5dh::DIRECT_MAX;  // direct tiles per batch (0: none)
  uint32_t direct_div = 1;           // direct tiles average >= 1/direct_div records per 8K samples
  uint32_t region_pct = 100;         // region capacity scale (L5DH_PARAM_REGION_PCT)
  uint64_t fold_last = 0;            // samples of the last batch folded at ingest (one-tile spaces)
  DevBuf stage_series, stage_values, stage_summ, stage_counts, stage_totals, stage_in_counts, stage_in_totals;
  // staging ring: small ingest batches are concatenated on the device and binned together
  DevBuf ring_series, ring_values;
  size_t ring_fill = 0;
  size_t ring_cap = 0;  // samples (0: every batch is binned at once)
  hipEvent_t ev_copy = nullptr;
  // asynchronous ingest: ticket t's inputs are consumed when tick_ev[t % NTICK] (recorded
  // for a ticket >= t, stream order) completes
  static constexpr int NTICK = 64;
  hipEvent_t tick_ev[NTICK] = {};
  uint64_t tick_of[NTICK] = {};
  uint64_t tick_next = 0, tick_done = 0;
  uint32_t err_reported = 0;  // invalid-id reports already returned (h_header[PIN_ERR] is the device's count)
  // fleet merge (RCCL)
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  DevBuf merge_counts, merge_totals, recv_counts, recv_totals;
  // sparse reduce-scatter (l5dh_merge.hip): this rank's encoding, the received slices
  DevBuf m_words, m_offs, m_enc, m_tmp, m_sizes, r_words, r_offs, r_enc;
  DevBuf m_unpacked, m_roff;  // the sparse export: rows' encodings at their tiles' places, each row's first word
  size_t m_unpacked_words = 0;  // (the unpacked encoding's size: a bound of the packed one)
  bool m_sparse = false;      // the last export was sparse (reduce-scatter through the collective)
  size_t m_tmp_bytes = 0;
  std::vector<uint64_t> m_to, m_from;  // words to / from every rank
  uint64_t m_dense_bytes = 0, m_encoded_bytes = 0, m_sent_bytes = 0;
  bool rccl_1rank = false;  // run the collective in a 1-rank communicator too (an identity otherwise skipped)
  bool loopback = false;    // l5dh_comm_init_loopback: the collectives are device copies among the group's contexts
  // label rollups (l5dh_rollup.hip): the staged map, the plan's arrays, the partial rows, staged outputs
  DevBuf ru_group, ru_u32, ru_u64, ru_members, ru_igroup, ru_mlist, ru_partial, ru_tmp, ru_summ, ru_counts, ru_totals;
  DevBuf le_stage, le_sums_stage;  // cumulative `le` buckets (l5dh_le.hip): staged outputs
  DevBuf q_stage;                  // configurable quantiles (l5dh_quant.hip): staged output
  DevBuf rd_qlabels;               // the device renderer's quantile labels, formatted on the host
  // top-k selection (l5dh_top.hip): staged external rows and group map, the K = 1 quantile values,
  // the two list buffers of the tournament, staged outputs (ids, summaries, quantile values), the count
  DevBuf top_vals, top_group, top_q, top_list_a, top_list_b, top_ids, top_summ, top_qout, top_n;
  // state import and sparse export (l5dh_import.hip): status words, staged CSR inputs, the clean
  // tiles' flags and list; the export's row counts, offsets, scan scratch and staged entries
  DevBuf imp_status, imp_series, imp_off, imp_entries, imp_tflag, imp_list;
  DevBuf xs_cnt, xs_offs, xs_tmp, xs_entries;
  // the device renderers (l5dh_render.hip, l5dh_influx.hip; one call at a time uses them): staged
  // names, values and output; the two passes' scratch -- row lengths, their scan's offsets and
  // scratch, the rows' slots (rd_avg) and the flag words of either renderer (rd_flags)
  DevBuf rd_index, rd_koff, rd_kbytes, rd_loff, rd_lbytes, rd_vals, rd_sums, rd_le, rd_out;
  DevBuf rd_len, rd_offs, rd_avg, rd_flags, rd_tmp;
  DevBuf rd_kinds, rd_counters, rd_gauges;  // the staged kinds and values of the JSON, scalar and InfluxDB calls
  // the InfluxDB renderer: what its table has beyond the arrays staged above
  DevBuf ifx_line, ifx_field, ifx_hoff, ifx_hbytes, ifx_toff, ifx_tbytes, ifx_host;
  // the sliding window (l5dh_window_host.cpp): a ring of ended intervals, each slot the CSR of
  // one sparse export (row_off [count + 1], 8-byte entries, totals [count]) with the series
  // it covers and its push number; born [born_n] u64: the push number at which a series'
  // history starts (l5dh_window_forget); the query's status word
  struct Window {
    struct Slot {
      DevBuf row_off, entries, totals;
      uint32_t count = 0;
      uint64_t seq = 0, n_entries = 0;
    };
    uint32_t slots = 0, filled = 0, head = 0;  // head: the slot the next push writes
    uint64_t pushes = 0;
    std::unique_ptr<Slot[]> slot;
    DevBuf born, status;
    uint32_t born_n = 0;
  };
  std::unique_ptr<Window> win;  // (freed after ~l5dh_ctx has drained the stream, as every device buffer)
  // the counter space (l5dh_counters_host.cpp): values [max] int64, the kernels' statistics words
  // (stats [CS_WORDS] u64), the rollup's status word, the staged inputs of an add and of a rollup
  struct Counters {
    DevBuf values, stats, status;
    uint32_t max = 0;
    uint64_t dropped_reported = 0;  // dropped ids already returned by l5dh_sync
    DevBuf stage_ids, stage_deltas, stage_vals, stage_group, stage_out;
  };
  std::unique_ptr<Counters> cnt;
  uint32_t rollup_item = l5dh::RU_ITEM_DEFAULT;  // members per work item (L5DH_PARAM_ROLLUP_ITEM)
  uint32_t variant = 0;  // L5DH_PARAM_VARIANT: result-preserving kernel variants (A/B timing)
  // params
  uint32_t cold_limit = l5dh::COLD_LIMIT_MAX;
  uint32_t hot_chunk = 1u << 18;  // records per big-tile item (u32 LDS bins, one half-tile per workgroup)
  bool timing = false;
  struct Ev {
    int kid;
    hipEvent_t a, b;
  };
  std::vector<Ev> pending_ev;
  std::vector<hipEvent_t> ev_pool;
  double k_ms[L5DH_K_NKERNELS] = {0};
  int64_t k_n[L5DH_K_NKERNELS] = {0};

  // Drains the stream, then destroys the events, the communicator, the pinned header
  // and the streams; the device buffers free themselves after it (no hipFree runs before
  // the stream has been synchronized).  Copes with a half-built context (l5dh_open).
  ~l5dh_ctx();
};

namespace l5dh {

// The context's lock with its device made current: the preamble of an entry point
// that touches the GPU.
struct CtxLock {
  std::lock_guard<std::mutex> g;
  explicit CtxLock(l5dh_ctx* c) : g(c->mu) { hipSetDevice(c->device); }
};

int fail(l5dh_ctx* c, int code, const std::string& msg);
int hipfail(l5dh_ctx* c, hipError_t e, const char* what);

#define HIPCHK(c, expr)                                \
  do {                                                 \
    hipError_t _e = (expr);                            \
    if (_e != hipSuccess) return hipfail((c), _e, #expr); \
  } while (0)

struct KTimer {  // a timed scope on the context's stream (L5DH_PARAM_TIMING)
  l5dh_ctx* c;
  int kid;
  hipEvent_t a = nullptr;
  KTimer(l5dh_ctx* c_, int kid_);
  ~KTimer();
};

int sync_stream(l5dh_ctx* c);
bool is_device_ptr(const void* p);
// Grows only; the stream is synchronized before the old block is freed.
int ensure(l5dh_ctx* c, DevBuf& b, size_t bytes);
Tables tables(l5dh_ctx* c);
State state(l5dh_ctx* c);
int flush_ring(l5dh_ctx* c);
// Aggregate every pending segment.  final_mode: emit summaries/counts for the
// whole series space into `out` (fused path); otherwise fold into state.  encode: the
// fleet merge's sparse export (out.words / out.roff / out.totals; out.enc is set here).
int aggregate(l5dh_ctx* c, int final_mode, int reset, Outputs out, bool encode = false);
// Fold the pending segments into the state rows.
int fold(l5dh_ctx* c);

// ---- staging: a caller's array is used in place when it is device memory the kernels
// can address, otherwise through a staging buffer of the context.  Alignment: 8 bytes
// for everything (the kernels' 64-bit accesses) except the rollup's u32 group map, 4.
// The helpers carry no timer: each caller keeps its own KTimer scopes.
inline bool direct(const void* p, size_t align) { return is_device_ptr(p) && (uintptr_t)p % align == 0; }

// Input: p becomes the address the kernel reads -- unchanged when direct (or null, or
// empty: never read), else `stage`, with the copy enqueued.
template <class T>
int stage_in(l5dh_ctx* c, const T*& p, size_t count, size_t align, DevBuf& stage) {
  if (!p || !count || direct(p, align)) return 0;
  if (int r = ensure(c, stage, count * sizeof(T))) return r;
  HIPCHK(c, hipMemcpyAsync(stage.p, p, count * sizeof(T), hipMemcpyDefault, c->stream));
  p = stage.as<const T>();
  return 0;
}

// Output of `count` elements T at the caller's `user` (nullable: an optional output).
template <class T>
struct StagedOut {
  void* user = nullptr;
  T* dev = nullptr;  // where the kernel writes (null: no output)
  size_t bytes = 0;
  bool staged() const { return dev && dev != user; }
  // First half: dev = user when direct, else `stage` grown to hold the output.
  int begin(l5dh_ctx* c, void* user_, size_t count, DevBuf& stage, size_t align = 8) {
    if (!user_ || !count) return 0;
    user = user_;
    bytes = count * sizeof(T);
    if (direct(user, align)) {
      dev = static_cast<T*>(user);
      return 0;
    }
    if (int r = ensure(c, stage, bytes)) return r;
    dev = stage.as<T>();
    return 0;
  }
  // An accumulating output: the caller's old values go to the staging buffer first.
  int load(l5dh_ctx* c) const {
    if (staged()) HIPCHK(c, hipMemcpyAsync(dev, user, bytes, hipMemcpyDefault, c->stream));
    return 0;
  }
  // Second half: the copy back to the caller, if staged.
  int end(l5dh_ctx* c) const {
    if (staged()) HIPCHK(c, hipMemcpyAsync(user, dev, bytes, hipMemcpyDefault, c->stream));
    return 0;
  }
};

// ---- the steps the drivers of the live queries share; no timer either ----
// The state rows made current: the ring binned, the pending segments folded.
int live_begin(l5dh_ctx* c);
// The per-series snapshot (summ_dev, nullable) and reset of [first, first + count), from
// the state rows.
int rows_of_range(l5dh_ctx* c, uint32_t first, uint32_t count, Summary88* summ_dev, int reset);
// -EINVAL unless [first, first + count) lies within the series space.
int check_range(l5dh_ctx* c, uint32_t first, uint32_t count);
// l5dh_sync's share of the counter space (l5dh_counters_host.cpp), after the stream has been
// drained: -EINVAL once for ids dropped since the last such report.
int counters_check(l5dh_ctx* c);

// n elements of a small host or device array to the host: one copy, and one wait if it
// was device memory.
template <class T>
int fetch_small(l5dh_ctx* c, const T* p, size_t n, T* host_dst) {
  if (!is_device_ptr(p)) {
    memcpy(host_dst, p, n * sizeof(T));
    return 0;
  }
  HIPCHK(c, hipMemcpyAsync(host_dst, p, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  return sync_stream(c);
}

// ---- count, scan, total: the step the sparse export, the window push and the text passes
// share.  Sizes cnt [n + 1] u32, offs [n + 1] u64 and the scan's scratch; then, in one
// L5DH_K_HOT scope, runs count(cnt) -- the caller's launches that fill cnt[0 .. n) -- and the
// fleet merge's exclusive scan, which leaves offs[n] the total.  total non-null: read back
// here, with a host wait of its own; null: the caller reads offs[n] with whatever else
// shares its wait.
template <class Count>
int count_scan(l5dh_ctx* c, uint32_t n, DevBuf& cnt, DevBuf& offs, DevBuf& tmp, Count&& count, uint64_t* total = nullptr) {
  int r;
  size_t tmp_bytes = 0;
  HIPCHK(c, merge_count(n, nullptr, nullptr, nullptr, &tmp_bytes, c->stream));
  if ((r = ensure(c, cnt, ((size_t)n + 1) * 4)) || (r = ensure(c, offs, ((size_t)n + 1) * 8)) ||
      (r = ensure(c, tmp, tmp_bytes)))
    return r;
  {
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, count(cnt.as<uint32_t>()));
    HIPCHK(c, merge_count(n, cnt.as<uint32_t>(), offs.as<uint64_t>(), tmp.p, &tmp_bytes, c->stream));
  }
  if (!total) return 0;
  HIPCHK(c, hipMemcpyAsync(total, offs.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, c->stream));
  return sync_stream(c);
}

}  // namespace l5dh
