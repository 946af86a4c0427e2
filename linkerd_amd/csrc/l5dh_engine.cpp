// l5dh_engine.cpp -- host side of the MI355X histogram engine: the context's
// lifetime, ingest, snapshot, and their part of the C-ABI declared in
// include/l5dhist.h (the query families' entry points are in l5dh_queries.cpp,
// the fleet merge's in l5dh_fleet.cpp).
//
// One context = one GPU = one shard of the series space (l5dh_ctx.hpp).  It owns:
//   * the constant tables, built once per process on the host (l5dh_tables.cpp)
//   * dense state    counts[S][1800] u32, total[S] i64, sumfix[S] i64, dirty[F]
//   * a log of binned ingest segments (u16 records, one contiguous range per
//     (tile, half) key, + the segment's metadata)
//   * scratch for the snapshot plan, staging buffers for host-side arguments
// Ingest partitions a batch by series tile at once, in two levels and with no
// counting pass (README steps 3-4): the regions are sized from the previous
// batch's exact key counts and a sample of this one; level 1 scatters the samples
// into super-tile bins (u32 records) and gives the <= 255 heaviest ("direct")
// tiles their final u16 records itself; level 2 gives the other tiles theirs; a
// region that overflows is redone with exact sizes.  A one-tile space is folded
// into its state rows at ingest instead.  Snapshot plans over the pending
// segments, accumulates each tile in LDS-private histograms and emits summaries
// in the same pass (the fused path), or folds into state first (range path).
#include <algorithm>
#include <cerrno>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "l5dh_ctx.hpp"

using namespace l5dh;

namespace {

constexpr size_t MAX_BATCH = ((size_t)1 << 30) - 65536;  // samples per binned piece (k_bin1 tags bit 31)

hipEvent_t ev_get(l5dh_ctx* c) {
  if (!c->ev_pool.empty()) {
    hipEvent_t e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  hipEventCreate(&e);
  return e;
}

void collect_timing(l5dh_ctx* c) {
  for (auto& e : c->pending_ev) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
      c->k_ms[e.kid] += ms;
      c->k_n[e.kid] += 1;
    }
    c->ev_pool.push_back(e.a);
    c->ev_pool.push_back(e.b);
  }
  c->pending_ev.clear();
}

// Device-visible address of page-locked host memory (hipHostMalloc / registered),
// or nullptr for device or pageable memory.
const void* host_mapped_ptr(const void* p) {
  if (!p) return nullptr;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  if (a.type != hipMemoryTypeHost || !a.devicePointer) return nullptr;
  return static_cast<const char*>(a.devicePointer) + (static_cast<const char*>(p) - static_cast<const char*>(a.hostPointer));
}

Plan plan(l5dh_ctx* c) {
  return Plan{c->d_tile_tot, c->d_enc_base, c->d_enc_h0, c->d_enc_dw, c->d_cold_item,
              c->split_item.as<uint2>(), c->d_hot_list, c->d_tile_flags, c->d_header,
              c->h_header_dev + PIN_BIG};
}

Segs segs_view(l5dh_ctx* c) {
  Segs s{};
  s.n = c->nseg;
  for (int j = 0; j < c->nseg; ++j) {
    s.rec16[j] = c->segs[j].rec16.as<const uint16_t>();
    s.meta[j] = c->segs[j].meta;
  }
  return s;
}

int do_ingest(l5dh_ctx* c, const uint32_t* series, const float* values, size_t n);

}  // namespace

// ---- helpers shared with l5dh_queries.cpp and l5dh_fleet.cpp (declared in l5dh_ctx.hpp) ----
namespace l5dh {

int fail(l5dh_ctx* c, int code, const std::string& msg) {
  c->last_error = msg;
  return code;
}

int hipfail(l5dh_ctx* c, hipError_t e, const char* what) {
  c->last_error = std::string(what) + ": " + hipGetErrorString(e);
  return -EIO;
}

KTimer::KTimer(l5dh_ctx* c_, int kid_) : c(c_), kid(kid_) {
  if (c->timing) {
    a = ev_get(c);
    hipEventRecord(a, c->stream);
  }
}

KTimer::~KTimer() {
  if (a) {
    hipEvent_t b = ev_get(c);
    hipEventRecord(b, c->stream);
    c->pending_ev.push_back({kid, a, b});
  }
}

int sync_stream(l5dh_ctx* c) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  collect_timing(c);
  return 0;
}

bool is_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

int ensure(l5dh_ctx* c, DevBuf& b, size_t bytes) {
  if (b.cap >= bytes) return 0;
  if (b.p) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.release();
  }
  size_t cap = std::max(bytes, (size_t)4096);
  cap = (cap + 4095) & ~(size_t)4095;
  hipError_t e = hipMalloc(&b.p, cap);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, -ENOMEM, std::string("hipMalloc staging: ") + hipGetErrorString(e));
  }
  b.cap = cap;
  return 0;
}

Tables tables(l5dh_ctx* c) { return Tables{c->d_lim_pad, c->d_mid, c->d_base, c->d_lut, c->d_lut2, c->d_lut2 + LUT2_N}; }

State state(l5dh_ctx* c) { return State{c->d_counts, c->d_total, c->d_sumfix, c->d_dirty, c->S, c->F}; }

int aggregate(l5dh_ctx* c, int final_mode, int reset, Outputs out, bool encode) {
  if (!final_mode && c->nseg == 0) return 0;
  Segs sv = segs_view(c);
  size_t recs = 0;
  for (int j = 0; j < c->nseg; ++j) recs += c->segs[j].n;
  // big-tile items: hot_chunk records, fewer when the pending records would leave CUs
  // idle (>= 2 items per CU when the records allow)
  uint32_t hc = c->hot_chunk;
  {
    const size_t fill = recs / (2 * (size_t)std::max(1, c->num_cu));
    hc = (uint32_t)std::min<size_t>(hc, std::max<size_t>(16384, (fill + 1023) & ~(size_t)1023));
  }
  if (int r = ensure(c, c->split_item, (recs / hc + 2 * (size_t)c->F + 2) * 8)) return r;
  Plan pl = plan(c);
  // a resetting snapshot of every series into dense rows: clean big tiles count
  // straight into their output rows (no copy of state rows in k_hot_finish), and those
  // whose halves are one item each are written by their items alone (TF_SOLO)
  const int direct_out = final_mode && reset && out.counts && out.first == 0 && out.count == (uint32_t)c->S;
  // the sparse export (the fleet merge's reduce-scatter): row encodings, no dense rows
  if (encode && !(final_mode && reset && out.first == 0 && out.count == (uint32_t)c->S && !out.counts && !out.summ))
    return fail(c, -EINVAL, "internal: the sparse export is a whole-range resetting export");
  {
    KTimer kt(c, L5DH_K_SCAN);
    // (the sparse export: the dirty tiles' state-row words first, for their encoding ranges)
    if (encode) HIPCHK(c, launch_enc_dirty(state(c), pl, c->stream));
    HIPCHK(c, launch_plan(sv, c->F, final_mode, c->cold_limit, hc, c->d_dirty, direct_out, encode ? 1 : 0, pl,
                          c->stream));
  }
  if (encode) {  // the unpacked encoding's size comes from the plan (one host wait)
    uint32_t words = 0;
    HIPCHK(c, hipMemcpyAsync(&words, c->d_header + plan_header(c->F).enc_words(), 4, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int r = ensure(c, c->m_unpacked, (size_t)words * 4 + 16)) return r;
    c->m_unpacked_words = words;
    out.enc = c->m_unpacked.as<uint32_t>();
  }
  // The accumulate kernels are persistent and read their item counts from the plan
  // header on the device, so no host round trip separates them from the plan: the
  // launches get upper bounds (a big tile holds > cold_limit records).
  const uint32_t hot = (uint32_t)std::min<size_t>(c->F, recs / ((size_t)c->cold_limit + 1));
  const uint32_t split_items = (uint32_t)std::min<size_t>(0xFFFFFFF0u, recs / hc + 2 * (size_t)hot);
  State st = state(c);
  Tables tb = tables(c);
  if (hot) {
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, launch_hot_init(pl, hot, st, out, direct_out, c->stream));
  }
  bool joined = true;
  {
    // the big tiles first (on at most half the CUs), the cold tiles on the side stream
    // concurrently (disjoint tiles and series; the side stream joins back after
    // k_hot_finish, which touches only big tiles: it runs under the cold kernel)
    KTimer kt(c, L5DH_K_ACCUM);
    // The two streams cost ~20 us of idle GPU (the fork's and the join's barrier packets);
    // they pay only when there are big tiles, so the last plan the host has seen picks the
    // order (a hint: either order is correct; k_plan_b writes it to a mapped host word)
    const bool big_seen = __atomic_load_n(c->h_header + PIN_BIG, __ATOMIC_RELAXED) != 0u;
    if (split_items && big_seen) {
      HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
      HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
      HIPCHK(c, launch_accum_split(sv, pl, split_items, st, tb, out, direct_out, hc, c->stream));
      HIPCHK(c, launch_accum_cold(sv, pl, DEV_COUNT, st, tb, out, final_mode, reset, c->side));
      HIPCHK(c, hipEventRecord(c->ev_join, c->side));
      joined = false;
    } else {
      if (split_items) HIPCHK(c, launch_accum_split(sv, pl, split_items, st, tb, out, direct_out, hc, c->stream));
      HIPCHK(c, launch_accum_cold(sv, pl, DEV_COUNT, st, tb, out, final_mode, reset, c->stream));
    }
    // (timed with the accumulate: with two streams it runs under the cold kernel)
    if (hot) HIPCHK(c, launch_hot_finish(pl, hot, st, tb, out, final_mode, reset, direct_out, c->stream));
    if (!joined) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
  }
  c->nseg = 0;
  return 0;
}

// Bin the staging ring as one batch.
int flush_ring(l5dh_ctx* c) {
  if (!c->ring_fill) return 0;
  const size_t n = c->ring_fill;
  c->ring_fill = 0;
  return do_ingest(c, c->ring_series.as<const uint32_t>(), c->ring_values.as<const float>(), n);
}

int fold(l5dh_ctx* c) {
  Outputs none{nullptr, nullptr, 0, 0, nullptr};
  return aggregate(c, 0, 0, none);
}

int live_begin(l5dh_ctx* c) {
  int r;
  if ((r = flush_ring(c)) || (r = fold(c))) return r;
  return 0;
}

int rows_of_range(l5dh_ctx* c, uint32_t first, uint32_t count, Summary88* summ_dev, int reset) {
  HIPCHK(c, launch_rows(state(c), nullptr, nullptr, tables(c), Outputs{summ_dev, nullptr, first, count, nullptr}, reset,
                        nullptr, c->stream));
  return 0;
}

int check_range(l5dh_ctx* c, uint32_t first, uint32_t count) {
  if ((uint64_t)first + count > c->S) return fail(c, -EINVAL, "series range out of bounds");
  return 0;
}

}  // namespace l5dh

namespace {

// Invalid series ids: k_rbin1 (k_fold1) adds to the device counter d_err (never
// reset); k_rfix1 (a copy, after k_fold1) puts it into the pinned, mapped h_header[PIN_ERR].  The host value only grows, so comparing it with the number of
// reports already returned needs no synchronization.
int check_err(l5dh_ctx* c) {
  const uint32_t seen = __atomic_load_n(c->h_header + PIN_ERR, __ATOMIC_ACQUIRE);
  if (seen != c->err_reported) {
    c->err_reported = seen;
    return fail(c, -EINVAL, "series id >= max_series in an ingest batch (those samples were dropped)");
  }
  return 0;
}

int do_ingest(l5dh_ctx* c, const uint32_t* series, const float* values, size_t n) {
  if (n == 0) return 0;
  if (n > MAX_BATCH) return fail(c, -EINVAL, "batch piece larger than 2^30 samples");
  if (c->nseg >= c->max_seg) {
    int r = fold(c);
    if (r) return r;
  }
  const uint32_t* ds = series;
  const float* dv = values;
  if (!is_device_ptr(series) || !is_device_ptr(values)) {
    int r;
    if ((r = ensure(c, c->stage_series, n * 4))) return r;
    if ((r = ensure(c, c->stage_values, n * 4))) return r;
    KTimer kt(c, L5DH_K_COPY);
    HIPCHK(c, hipMemcpyAsync(c->stage_series.p, series, n * 4, hipMemcpyDefault, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->stage_values.p, values, n * 4, hipMemcpyDefault, c->stream));
    ds = c->stage_series.as<const uint32_t>();
    dv = c->stage_values.as<const float>();
  }
  const bool vec = ((uintptr_t)ds % 16 == 0) && ((uintptr_t)dv % 16 == 0);
  if (c->F == 1) {  // one tile: fold the batch into its state rows now (no records, no segment)
    KTimer kt(c, L5DH_K_BIN);
    // one item per CU when the batch allows (each item clears and flushes its LDS rows:
    // C1's fold 0.040 ms at two items per CU, 0.033 at one, 0.044 at four;
    // profiles/r06_fold_items_ab.txt)
    const size_t fill = n / (size_t)std::max(1, c->num_cu);
    const uint32_t chunk =
        (uint32_t)std::min<size_t>(c->hot_chunk & ~3u, std::max<size_t>(16384, (fill + 1023) & ~(size_t)1023));
    HIPCHK(c, launch_fold1(ds, dv, n, chunk, state(c), tables(c), c->d_err, vec, (c->variant & 1) != 0, c->stream));
    c->fold_last = n;
    HIPCHK(c, hipMemcpyAsync(c->h_header + PIN_ERR, c->d_err, 4, hipMemcpyDeviceToHost, c->stream));
    return 0;
  }
  auto& sg = c->segs[c->nseg];
  // region buffers: the plan sizes the regions from the previous batch and a sample
  // of this one, with slack; a plan that does not fit is scaled to these sizes (an
  // overflowing region is then redone with exact sizes, which always fit)
  // rec32: the super-tile bins' records; rec16: the direct keys' regions in [0, dlim16)
  // (planned, so possibly oversized) and level 2's regions after them, with room for
  // level 2's exact layout in any case (N + 7 per key of padding)
  const size_t cap32 = n + n / 2 + ((size_t)1 << 19);
  const size_t cap16 = 2 * n + n / 8 + (size_t)128 * c->F + 4096;
  const size_t dlim16 = (cap16 - (n + (size_t)16 * c->F + 1024)) & ~(size_t)7;  // (level-2 regions 16-B aligned)
  {
    int r = ensure(c, sg.rec32, (cap32 + 16) * 4);  // readers load whole 16-B groups
    if (!r) r = ensure(c, sg.rec16, (cap16 + 16) * 2);
    if (r) return r;
  }
  // slabs: one workgroup per CU at most, >= 8K samples each, 16-B aligned starts
  int G = (int)std::min<size_t>((size_t)c->G_max, (n + 8191) / 8192);
  if (G < 1) G = 1;
  size_t per = (n + G - 1) / G;
  per = (per + 3) & ~(size_t)3;
  G = (int)((n + per - 1) / per);
  IngestArgs a{};
  a.series = ds;
  a.values = dv;
  a.n = n;
  a.per = per;
  a.G = G;
  a.num_cu = c->num_cu;
  a.S = c->S;
  a.F = c->F;
  a.tb = tables(c);
  a.sumfix = c->d_sumfix;
  a.err = c->d_err;
  a.err_host = c->h_header_dev + PIN_ERR;
  a.kest = c->d_kest;
  a.kprev = c->d_kprev;
  a.meta = sg.meta;
  a.rec32 = sg.rec32.as<uint32_t>();
  a.rec16 = sg.rec16.as<uint16_t>();
  a.cap32 = cap32;
  a.cap16 = cap16;
  a.dlim16 = dlim16;
  a.thr_min = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, n / (8192ull * c->direct_div)), 0xFFFFFFFFull);
  const uint32_t FS = (c->F + 63) / 64;
  // + the trash bin (and 8 spare bins)
  a.dmax = std::min<uint32_t>(c->direct_max, ((uint32_t)BIN1_BINS - 9 - FS) / 2);
  a.pct = c->region_pct;
  a.vec = vec;
  {
    KTimer kt(c, L5DH_K_SCAN);
    // variant bit 2 (measurement): forget the previous batch's exact key counts, so every
    // batch is planned as a first interval is -- from its sample alone
    if (c->variant & 4) HIPCHK(c, hipMemsetAsync(c->d_kprev, 0, (size_t)2 * c->F * 4, c->stream));
    HIPCHK(c, launch_ingest(a, 0, c->stream));
  }
  {
    KTimer kt(c, L5DH_K_BIN);
    HIPCHK(c, launch_ingest(a, 1, c->stream));
  }
  {
    KTimer kt(c, L5DH_K_BIN2);
    HIPCHK(c, launch_ingest(a, 3, c->stream));
  }
  sg.n = n;
  c->nseg++;
  return 0;  // (k_rfix1 wrote the invalid-id count to h_header[PIN_ERR])
}

// Wait until the caller's buffers of this call have been read by the device.
int wait_inputs(l5dh_ctx* c) {
  HIPCHK(c, hipEventRecord(c->ev_copy, c->stream));
  HIPCHK(c, hipEventSynchronize(c->ev_copy));
  return 0;
}

// Asynchronous ingest: the inputs of ticket t are consumed once its event completes.
int issue_ticket(l5dh_ctx* c, uint64_t* ticket) {
  const uint64_t t = ++c->tick_next;
  const int slot = (int)(t % l5dh_ctx::NTICK);
  if (!c->tick_ev[slot]) HIPCHK(c, hipEventCreateWithFlags(&c->tick_ev[slot], hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->tick_ev[slot], c->stream));
  c->tick_of[slot] = t;
  *ticket = t;
  return 0;
}

int wait_ticket(l5dh_ctx* c, uint64_t t) {
  if (t <= c->tick_done) return 0;
  if (t > c->tick_next) return fail(c, -EINVAL, "unknown ingest ticket");
  const int slot = (int)(t % l5dh_ctx::NTICK);
  // the slot holds t or a later ticket (recorded later on the same stream)
  HIPCHK(c, hipEventSynchronize(c->tick_ev[slot]));
  c->tick_done = std::max(c->tick_done, c->tick_of[slot]);
  return 0;
}

int ingest_impl(l5dh_ctx* c, const uint32_t* series, const float* values, size_t n, uint64_t* ticket = nullptr) {
  if (ticket) *ticket = c->tick_next;  // nothing new to wait for (n == 0)
  if (n == 0) return 0;
  const bool dev = is_device_ptr(series) && is_device_ptr(values);
  // caller-stream contexts are stream ordered for device inputs; otherwise the
  // call returns once nothing of the caller's memory is still to be read, or, in
  // the asynchronous form, with a ticket to wait for
  const bool wait = (!dev || c->stream == c->own_stream) && !ticket;
  if (c->ring_cap && n <= c->ring_cap / 2) {
    int r;
    if (c->ring_fill + n > c->ring_cap && (r = flush_ring(c))) return r;
    if ((r = ensure(c, c->ring_series, c->ring_cap * 4 + 64)) || (r = ensure(c, c->ring_values, c->ring_cap * 4 + 64)))
      return r;
    {
      KTimer kt(c, L5DH_K_COPY);
      uint32_t* rs = c->ring_series.as<uint32_t>() + c->ring_fill;
      float* rv = c->ring_values.as<float>() + c->ring_fill;
      // pinned host batches: one zero-copy kernel (variant bit 1: DMA copies instead)
      const void* hs = dev || (c->variant & 2) ? nullptr : host_mapped_ptr(series);
      const void* hv = hs ? host_mapped_ptr(values) : nullptr;
      if (hs && hv) {
        HIPCHK(c, launch_fetch_host(static_cast<const uint32_t*>(hs), static_cast<const uint32_t*>(hv), rs,
                                    reinterpret_cast<uint32_t*>(rv), n, c->stream));
      } else {
        HIPCHK(c, hipMemcpyAsync(rs, series, n * 4, hipMemcpyDefault, c->stream));
        HIPCHK(c, hipMemcpyAsync(rv, values, n * 4, hipMemcpyDefault, c->stream));
      }
    }
    c->ring_fill += n;
    if (ticket) return issue_ticket(c, ticket);
    return wait ? wait_inputs(c) : 0;
  }
  int r = flush_ring(c);
  if (r) return r;
  // batches are binned in pieces below 2^30 samples (k_bin1 tags direct-tile
  // destinations in bit 31)
  for (size_t o = 0; o < n; o += MAX_BATCH) {
    const size_t m = std::min(n - o, MAX_BATCH);
    if ((r = do_ingest(c, series + o, values + o, m))) return r;
  }
  if (ticket) return issue_ticket(c, ticket);
  return wait ? wait_inputs(c) : 0;
}

bool full_range(l5dh_ctx* c, uint32_t first, uint32_t count) { return first == 0 && count == c->S; }

int do_snapshot(l5dh_ctx* c, uint32_t first, uint32_t count, l5dh_summary* out, int32_t* counts_out, int reset) {
  if (int r = check_range(c, first, count)) return r;
  if (count == 0) return 0;
  int r = flush_ring(c);
  if (r) return r;
  StagedOut<Summary88> summ;
  StagedOut<int32_t> cnt;
  if ((r = summ.begin(c, out, count, c->stage_summ)) || (r = cnt.begin(c, counts_out, (size_t)count * NB, c->stage_counts)))
    return r;
  Outputs o{summ.dev, cnt.dev, first, count, nullptr};
  // (a one-tile space folds every batch into its state rows at ingest: no segments, so its
  // snapshot is the state rows' -- one k_rows launch instead of the plan and accumulate
  // kernels; C1 in profiles/r06_one_tile_snapshot_ab.txt)
  if (full_range(c, first, count) && c->F > 1) {
    if ((r = aggregate(c, 1, reset, o))) return r;
  } else {
    if ((r = fold(c))) return r;
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, launch_rows(state(c), nullptr, nullptr, tables(c), o, reset, nullptr, c->stream));
  }
  {
    KTimer kt(c, L5DH_K_COPY);
    if ((r = summ.end(c)) || (r = cnt.end(c))) return r;
  }
  // The one entry point that may return without a host wait (every other one ends in
  // sync_stream): direct outputs on a caller stream are stream ordered (as device inputs
  // of l5dh_ingest), so the caller's later work on that stream sees them
  if (!summ.staged() && !cnt.staged() && c->stream != c->own_stream) return 0;
  return sync_stream(c);
}

}  // namespace

l5dh_ctx::~l5dh_ctx() {
  hipSetDevice(device);
  if (stream) hipStreamSynchronize(stream);  // before anything is freed
  for (auto& e : pending_ev) {
    hipEventDestroy(e.a);
    hipEventDestroy(e.b);
  }
  for (auto e : ev_pool) hipEventDestroy(e);
  for (hipEvent_t e : tick_ev)
    if (e) hipEventDestroy(e);
  for (hipEvent_t e : {ev_fork, ev_join, ev_copy})
    if (e) hipEventDestroy(e);
  if (comm) ncclCommDestroy(comm);
  if (h_header) hipHostFree(h_header);
  if (side) hipStreamDestroy(side);
  if (own_stream) hipStreamDestroy(own_stream);
}  // (the device buffers free themselves here)

// ============================================================================
// C-ABI
// ============================================================================
extern "C" {

int l5dh_abi_version(void) { return L5DH_ABI_VERSION; }

const int32_t* l5dh_limits(size_t* n) {
  const HostLimits& h = host_limits();
  if (n) *n = h.ok ? NL : 0;
  return h.ok ? h.L : nullptr;
}

int l5dh_open(l5dh_ctx** out, uint32_t max_series, uint32_t device_mask) {
  if (!out) return -EINVAL;
  *out = nullptr;
  if (max_series == 0 || max_series > L5DH_MAX_SERIES) return -EINVAL;
  if (device_mask == 0 || (device_mask & (device_mask - 1))) return -EINVAL;  // exactly one device
  const HostLimits& hl = host_limits();
  if (!hl.ok) return -EIO;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    return -ENODEV;
  }
  int dev = __builtin_ctz(device_mask);
  if (dev >= ndev) return -ENODEV;
  auto* c = new (std::nothrow) l5dh_ctx();
  if (!c) return -ENOMEM;
  c->device = dev;
  c->S = max_series;
  // staging ring: 64 samples per series, between 2^20 and 2^26 samples (4 MB .. 256 MB per array)
  c->ring_cap = std::min<size_t>(std::max<size_t>((size_t)max_series * 64, (size_t)1 << 20), (size_t)1 << 26);
  c->F = (max_series + TILE - 1) / TILE;
  auto bail = [&](int code) {
    delete c;
    return code;
  };
  if (hipSetDevice(dev) != hipSuccess) return bail(-EIO);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess) c->num_cu = prop.multiProcessorCount;
  // one slab per CU: the level-1 kernel holds one 1024-thread workgroup per CU (LDS-bound)
  c->G_max = std::max(1, std::min(c->num_cu, 512));
  if (set_ingest_attributes() != hipSuccess || set_snapshot_attributes() != hipSuccess) return bail(-EIO);
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) return bail(-EIO);
  if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess) return bail(-EIO);
  if (hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming) != hipSuccess)
    return bail(-EIO);
  c->stream = c->own_stream;
  const size_t S = c->S, F = c->F;
  bool ok = c->d_lim_pad.alloc(LIM_PAD * 4) && c->d_mid.alloc(NB * 4) && c->d_base.alloc(ROW * 4) &&
            c->d_lut.alloc(LUT_N * 4) && c->d_lut2.alloc(LUT2_N * 16) && c->d_counts.alloc(S * ROW * 4) &&
            c->d_total.alloc(S * 8) && c->d_sumfix.alloc(S * 8) && c->d_dirty.alloc(F) && c->d_err.alloc(4) &&
            c->d_tile_tot.alloc(F * 4) && c->d_cold_item.alloc((F + 1) * 16) && c->d_hot_list.alloc(F * 4) &&
            c->d_header.alloc(plan_header((uint32_t)F).words() * 4) && c->d_tile_flags.alloc(F) &&
            c->d_enc_base.alloc(F * 4) && c->d_enc_h0.alloc(F * 4) && c->d_enc_dw.alloc(2 * F * 4) &&
            c->d_kest.alloc(2 * F * 4) && c->d_kprev.alloc(2 * F * 4);
  const size_t meta_bytes = (size_t)meta_layout((uint32_t)F).words() * 4;
  for (int j = 0; ok && j < MAX_SEG; ++j)  // (zeroed: the header's redo counters only grow)
    ok = c->segs[j].meta.alloc(meta_bytes) && hipMemset(c->segs[j].meta, 0, meta_bytes) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    return bail(-ENOMEM);
  }
  if (hipHostMalloc((void**)&c->h_header, PIN_WORDS * 4, hipHostMallocMapped) != hipSuccess) return bail(-ENOMEM);
  memset(c->h_header, 0, PIN_WORDS * 4);
  if (hipHostGetDevicePointer((void**)&c->h_header_dev, c->h_header, 0) != hipSuccess) return bail(-ENOMEM);
  // constant tables (built on the host once per process: l5dh_tables.cpp)
  const HostTables* ht = nullptr;
  if (host_tables(&ht) != 0) return bail(-EIO);
  if (hipMemcpy(c->d_lut, ht->lut, sizeof(ht->lut), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->d_lut2, ht->lut2, sizeof(ht->lut2), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->d_lim_pad, ht->lim_pad, sizeof(ht->lim_pad), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->d_mid, ht->mid, sizeof(ht->mid), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->d_base, ht->base, sizeof(ht->base), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(c->d_dirty, 0, F) != hipSuccess || hipMemset(c->d_sumfix, 0, S * 8) != hipSuccess ||
      hipMemset(c->d_err, 0, 4) != hipSuccess || hipMemset(c->d_kest, 0, 2 * F * 4) != hipSuccess ||
      hipMemset(c->d_kprev, 0, 2 * F * 4) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
    return bail(-EIO);
  *out = c;
  return 0;
}

int l5dh_close(l5dh_ctx* c) {
  if (!c) return -EINVAL;
  delete c;
  return 0;
}

int l5dh_ingest(l5dh_ctx* c, const uint32_t* series, const float* values, size_t n) {
  if (!c) return -EINVAL;
  if (n && (!series || !values)) return -EINVAL;
  CtxLock g(c);
  // 0 = the batch was accepted; a deferred invalid-id report never rides on a later
  // batch's status (l5dh_sync returns it), so a caller never re-sends an accepted batch
  return ingest_impl(c, series, values, n);
}

int l5dh_ingest_async(l5dh_ctx* c, const uint32_t* series, const float* values, size_t n, uint64_t* ticket) {
  if (!c || !ticket) return -EINVAL;
  if (n && (!series || !values)) return -EINVAL;
  CtxLock g(c);
  return ingest_impl(c, series, values, n, ticket);  // (deferred id errors: l5dh_sync)
}

int l5dh_ingest_wait(l5dh_ctx* c, uint64_t ticket) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  return wait_ticket(c, ticket);
}

int l5dh_snapshot(l5dh_ctx* c, uint32_t first, uint32_t count, l5dh_summary* out, int32_t* counts_out, int reset) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  return do_snapshot(c, first, count, out, counts_out, reset);
}

int l5dh_export_state(l5dh_ctx* c, uint32_t first, uint32_t count, int32_t* counts, int64_t* totals, int reset) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (int r = check_range(c, first, count)) return r;
  if (count == 0) return 0;
  int r = flush_ring(c);
  if (r) return r;
  const bool fused = full_range(c, first, count) && reset;  // the fleet merge's export: one aggregate pass
  if (!fused && (r = fold(c))) return r;
  StagedOut<int32_t> cnt;
  StagedOut<int64_t> tot;
  if ((r = cnt.begin(c, counts, (size_t)count * NB, c->stage_counts)) || (r = tot.begin(c, totals, count, c->stage_totals)))
    return r;
  if (fused) {
    // pending records and state go straight into the caller's dense rows and
    // totals (no fold into state, no second pass), and the state is left clean
    if ((r = aggregate(c, 1, 1, Outputs{nullptr, cnt.dev, first, count, tot.dev}))) return r;
  } else {
    Outputs o{nullptr, cnt.dev, first, count, nullptr};
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, launch_rows(state(c), nullptr, nullptr, tables(c), o, reset, tot.dev, c->stream));
  }
  if ((r = cnt.end(c)) || (r = tot.end(c))) return r;  // (the copies are not timed here)
  return sync_stream(c);
}

int l5dh_summarize_dense(l5dh_ctx* c, const int32_t* counts, const int64_t* totals, size_t n, l5dh_summary* out) {
  if (!c || (n && (!counts || !out))) return -EINVAL;
  if (n == 0) return 0;
  if (n > 0xFFFFFFFFull) return -EINVAL;
  CtxLock g(c);
  int r;
  // (totals too must be 8-byte aligned to be read in place, like every int64 array)
  StagedOut<Summary88> summ;
  if ((r = stage_in(c, counts, n * NB, 8, c->stage_in_counts)) || (r = stage_in(c, totals, n, 8, c->stage_in_totals)) ||
      (r = summ.begin(c, out, n, c->stage_summ)))
    return r;
  Outputs o{summ.dev, nullptr, 0, (uint32_t)n, nullptr};
  {
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, launch_rows(state(c), counts, totals, tables(c), o, 0, nullptr, c->stream));
  }
  if ((r = summ.end(c))) return r;  // (the copies are not timed here)
  return sync_stream(c);
}

int l5dh_peek(l5dh_ctx* c, uint32_t series, l5dh_bucket_count* out, size_t cap, size_t* n_out) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (series >= c->S) return fail(c, -EINVAL, "series id out of range");
  int r = live_begin(c);
  if (r) return r;
  uint8_t dirty = 0;
  std::vector<uint32_t> row(ROW, 0);
  HIPCHK(c, hipMemcpyAsync(&dirty, c->d_dirty + (series >> TILE_SHIFT), 1, hipMemcpyDeviceToHost, c->stream));
  if ((r = sync_stream(c))) return r;
  if (dirty) {
    HIPCHK(c, hipMemcpyAsync(row.data(), c->d_counts + (size_t)series * ROW, NB * 4, hipMemcpyDeviceToHost,
                             c->stream));
    if ((r = sync_stream(c))) return r;
  }
  const HostLimits& hl = host_limits();
  size_t k = 0;
  for (int b = 0; b < NB; ++b) {
    const int32_t cnt = (int32_t)row[b];
    if (cnt > 0) {
      if (out && k < cap) {
        out[k].lower = b == 0 ? 0 : hl.L[b - 1];
        out[k].upper = b < NL ? hl.L[b] : INT_MAXV;
        out[k].count = cnt;
      }
      ++k;
    }
  }
  if (n_out) *n_out = k;
  return 0;
}

int l5dh_sync(l5dh_ctx* c) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  int r;
  if ((r = flush_ring(c)) || (r = sync_stream(c))) return r;
  if ((r = check_err(c))) return r;
  return c->cnt ? counters_check(c) : 0;
}

int l5dh_set_stream(l5dh_ctx* c, void* s) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  int r = sync_stream(c);
  if (r) return r;
  c->stream = s == L5DH_OWN_STREAM ? c->own_stream : static_cast<hipStream_t>(s);
  return 0;
}

int l5dh_wait_event(l5dh_ctx* c, void* ev) {
  if (!c || !ev) return -EINVAL;
  CtxLock g(c);
  HIPCHK(c, hipStreamWaitEvent(c->stream, static_cast<hipEvent_t>(ev), 0));
  return 0;
}

int l5dh_set_param(l5dh_ctx* c, int param, int64_t v) {
  if (!c) return -EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  switch (param) {
    case L5DH_PARAM_TIMING:
      c->timing = v != 0;
      return 0;
    case L5DH_PARAM_COLD_LIMIT:
      if (v < 0 || v > (int64_t)COLD_LIMIT_MAX) return fail(c, -EINVAL, "cold limit must be in [0, 65535]");
      c->cold_limit = (uint32_t)v;
      return 0;
    case L5DH_PARAM_HOT_CHUNK:
      // <= 2^20: an item's records index LDS bins in u32 (and stay far below 2^32)
      if (v < 1024 || v > (1ll << 20)) return fail(c, -EINVAL, "hot chunk must be in [1024, 2^20]");
      c->hot_chunk = (uint32_t)v;
      return 0;
    case L5DH_PARAM_MAX_SEGMENTS:
      if (v < 1 || v > MAX_SEG) return fail(c, -EINVAL, "max segments must be in [1, 8]");
      if (c->nseg > v) {
        hipSetDevice(c->device);
        int r = fold(c);
        if (r) return r;
      }
      c->max_seg = (int)v;
      return 0;
    case L5DH_PARAM_DIRECT_MAX:
      if (v < 0 || v > DIRECT_MAX) return fail(c, -EINVAL, "direct tiles must be in [0, 255]");
      c->direct_max = (uint32_t)v;
      return 0;
    case L5DH_PARAM_DIRECT_DIV:
      if (v < 1 || v > 65536) return fail(c, -EINVAL, "direct divisor must be in [1, 65536]");
      c->direct_div = (uint32_t)v;
      return 0;
    case L5DH_PARAM_STAGE_SAMPLES: {
      if (v < 0 || v > (int64_t)MAX_BATCH) return fail(c, -EINVAL, "staging ring must be in [0, 2^30 - 65536] samples");
      hipSetDevice(c->device);
      int r = flush_ring(c);  // staged samples are binned before the ring changes size
      if (r) return r;
      if ((size_t)v * 4 + 64 > c->ring_series.cap) {  // the next small batch allocates the new size
        if ((r = sync_stream(c))) return r;
        c->ring_series.release();
        c->ring_values.release();
      }
      c->ring_cap = ((size_t)v + 3) & ~(size_t)3;
      return 0;
    }
    case L5DH_PARAM_VARIANT:
      if (v < 0 || v > 31) return fail(c, -EINVAL, "variant bits must be in [0, 31]");
      c->variant = (uint32_t)v;
      return 0;
    case L5DH_PARAM_REGION_PCT:
      if (v < 1 || v > 1000) return fail(c, -EINVAL, "region capacity percent must be in [1, 1000]");
      c->region_pct = (uint32_t)v;
      return 0;
    case L5DH_PARAM_ROLLUP_ITEM:
      if (v < 1 || v > (int64_t)RU_ITEM_DEFAULT) return fail(c, -EINVAL, "rollup item must be in [1, 64] members");
      c->rollup_item = (uint32_t)v;
      return 0;
    case L5DH_PARAM_MERGE_RCCL_1RANK:
      c->rccl_1rank = v != 0;
      return 0;
    case L5DH_PARAM_MAX_SLABS:
      if (v < 1 || v > 512) return fail(c, -EINVAL, "slabs must be in [1, 512]");
      c->G_max = (int)v;
      return 0;
    default:
      return fail(c, -EINVAL, "unknown parameter");
  }
}

int l5dh_kernel_time(l5dh_ctx* c, int kid, double* ms, int64_t* launches, int reset_after) {
  if (!c || kid < 0 || kid >= L5DH_K_NKERNELS) return -EINVAL;
  CtxLock g(c);
  int r = sync_stream(c);
  if (r) return r;
  if (ms) *ms = c->k_ms[kid];
  if (launches) *launches = c->k_n[kid];
  if (reset_after) {
    c->k_ms[kid] = 0;
    c->k_n[kid] = 0;
  }
  return 0;
}

int l5dh_device(l5dh_ctx* c, int* dev) {
  if (!c || !dev) return -EINVAL;
  *dev = c->device;
  return 0;
}

uint32_t l5dh_max_series(l5dh_ctx* c) { return c ? c->S : 0; }

int l5dh_pin_alloc(size_t bytes, void** out) {
  if (!out || bytes == 0) return -EINVAL;
  if (hipHostMalloc(out, bytes, 0) != hipSuccess) {
    (void)hipGetLastError();
    *out = nullptr;
    return -ENOMEM;
  }
  return 0;
}

int l5dh_pin_free(void* p) {
  if (!p) return -EINVAL;
  return hipHostFree(p) == hipSuccess ? 0 : -EINVAL;
}

const char* l5dh_last_error(l5dh_ctx* c) { return c ? c->last_error.c_str() : "null context"; }

int l5dh_tile_totals(l5dh_ctx* c, uint64_t* out, size_t n) {
  if (!c || !out) return -EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  if (n < c->F) return fail(c, -EINVAL, "tile totals: the output holds fewer than ceil(max_series / 32) entries");
  hipSetDevice(c->device);
  int r;
  if ((r = flush_ring(c))) return r;
  if (c->F == 1) {  // folded at ingest: the batch's samples (invalid ids included)
    out[0] = c->fold_last;
    return sync_stream(c);
  }
  std::vector<uint32_t> k(2 * (size_t)c->F);
  HIPCHK(c, hipMemcpyAsync(k.data(), c->d_kprev, k.size() * 4, hipMemcpyDeviceToHost, c->stream));
  if ((r = sync_stream(c))) return r;
  for (uint32_t t = 0; t < c->F; ++t) out[t] = (uint64_t)k[2 * t] + k[2 * t + 1];
  return 0;
}

int l5dh_partition_redos(l5dh_ctx* c, uint64_t* level1, uint64_t* level2, uint64_t* level2_counted) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  int r;
  if ((r = flush_ring(c))) return r;
  const MetaLayout L = meta_layout(c->F);
  static_assert(H_NOVR2 == H_NOVR1 + 1 && H_NCNT2 == H_NOVR1 + 3, "header words read together");
  uint32_t h[MAX_SEG][4] = {};
  if (c->F > 1)
    for (int j = 0; j < MAX_SEG; ++j)
      HIPCHK(c, hipMemcpyAsync(h[j], c->segs[j].meta + L.hdr() + H_NOVR1, 16, hipMemcpyDeviceToHost, c->stream));
  if ((r = sync_stream(c))) return r;
  uint64_t a = 0, b = 0, k = 0;
  for (int j = 0; j < MAX_SEG; ++j) {
    a += h[j][0];
    b += h[j][1];
    k += h[j][3];
  }
  if (level1) *level1 = a;
  if (level2) *level2 = b;
  if (level2_counted) *level2_counted = k;
  return 0;
}

}  // extern "C"
