// l5dh_queries.cpp -- host side of the query families over the bucket rows: label rollups,
// cumulative `le` buckets, quantiles, top-k, state import (dense and sparse), the sparse
// export and the device renderer -- their drivers and their C-ABI entry points (declared in
// include/l5dhist.h).  The context, ingest and the snapshot are in l5dh_engine.cpp, as are
// the helpers of l5dh_ctx.hpp that the drivers here are written in.
#include <cerrno>
#include <cstring>
#include <string>

#include "l5dh_ctx.hpp"
#include "l5dh_fmt.hpp"

using namespace l5dh;

namespace {

// ---- label rollups -------------------------------------------------------------
// Per-group sums of the live state rows of series [first, first + count) (ext ==
// nullptr; then also the per-series snapshot / reset of the same state) or of external
// dense rows ext[count][1798].  The caller holds the lock and has checked the arguments.
int do_rollup(l5dh_ctx* c, uint32_t first, uint32_t count, const int32_t* ext, const int64_t* ext_totals,
              const uint32_t* group, uint32_t G, l5dh_summary* g_out, int32_t* g_counts_out, int64_t* g_totals_out,
              l5dh_summary* series_out, int reset) {
  int r;
  const bool live = ext == nullptr;
  if (live && (r = live_begin(c))) return r;
  RollupWork w{};
  w.count = count;
  w.G = G;
  w.first = first;
  w.item = c->rollup_item;
  w.caps = rollup_caps(count, G, w.item);
  w.tmp_bytes = rollup_tmp_bytes(G);
  const size_t G1 = (size_t)G + 1;
  if ((r = ensure(c, c->ru_u32, (4 * G1 + RH_WORDS) * 4)) || (r = ensure(c, c->ru_u64, 2 * G1 * 8)) ||
      (r = ensure(c, c->ru_members, ((size_t)count + 1) * 4)) || (r = ensure(c, c->ru_igroup, w.caps.items * 4)) ||
      (r = ensure(c, c->ru_mlist, (w.caps.multi + 1) * 4)) ||
      (r = ensure(c, c->ru_partial, (w.caps.slots + 1) * (size_t)RU_PROW * 8)) ||
      (r = ensure(c, c->ru_tmp, w.tmp_bytes)))
    return r;
  {
    KTimer kt(c, L5DH_K_COPY);
    // (the u32 map is the one argument that needs 4-byte alignment only; live: ext_totals is null)
    if ((r = stage_in(c, group, count, 4, c->ru_group)) ||
        (r = stage_in(c, ext, (size_t)count * NB, 8, c->stage_in_counts)) ||
        (r = stage_in(c, ext_totals, count, 8, c->stage_in_totals)))
      return r;
  }
  w.group = group;
  uint32_t* u = c->ru_u32.as<uint32_t>();
  w.cnt = u;
  w.nitems = u + G1;
  w.cursor = u + 2 * G1;
  w.pbase = u + 3 * G1;
  w.hdr = u + 4 * G1;
  w.moff = c->ru_u64.as<uint64_t>();
  w.ioff = w.moff + G1;
  w.members = c->ru_members.as<uint32_t>();
  w.igroup = c->ru_igroup.as<uint32_t>();
  w.mlist = c->ru_mlist.as<uint32_t>();
  w.partial = c->ru_partial.as<uint64_t>();
  w.tmp = c->ru_tmp.p;
  StagedOut<Summary88> g_summ, s_summ;
  StagedOut<int32_t> g_cnt;
  StagedOut<int64_t> g_tot;
  if ((r = g_summ.begin(c, g_out, G, c->ru_summ)) || (r = g_cnt.begin(c, g_counts_out, (size_t)G * NB, c->ru_counts)) ||
      (r = g_tot.begin(c, g_totals_out, G, c->ru_totals)) || (r = s_summ.begin(c, series_out, count, c->stage_summ)))
    return r;
  RollupOut o{g_summ.dev, g_cnt.dev, g_tot.dev};
  {
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, launch_rollup(w, state(c), ext, ext_totals, tables(c), o, c->stream));
  }
  // the device's findings (an invalid map entry, a bucket sum out of range) end the call
  // here, before the snapshot that would reset the range
  uint32_t hdr[RH_WORDS];
  HIPCHK(c, hipMemcpyAsync(hdr, w.hdr, sizeof(hdr), hipMemcpyDeviceToHost, c->stream));
  if ((r = sync_stream(c))) return r;
  if (hdr[RH_BOUNDS]) return fail(c, -EIO, "internal: a rollup workspace bound was hit");
  if (hdr[RH_BADIDX] != 0xFFFFFFFFu)
    return fail(c, -EINVAL,
                "rollup: group[" + std::to_string(hdr[RH_BADIDX]) + "] is neither < ngroups nor L5DH_NO_GROUP");
  if (hdr[RH_RANGE] != 0xFFFFFFFFu)
    return fail(c, -ERANGE, "rollup: a bucket sum of group " + std::to_string(hdr[RH_RANGE]) + " exceeds 2^31 - 1");
  if (live && count && (s_summ.dev || reset)) {
    KTimer kt(c, L5DH_K_HOT);
    if ((r = rows_of_range(c, first, count, s_summ.dev, reset))) return r;
  }
  {
    KTimer kt(c, L5DH_K_COPY);
    if ((r = g_summ.end(c)) || (r = g_cnt.end(c)) || (r = g_tot.end(c)) || (r = s_summ.end(c))) return r;
  }
  return sync_stream(c);
}

// ---- cumulative `le` buckets -----------------------------------------------------
// The cuts of a call, on the host and checked: K in [1, LE_MAX], each cut in [1, NL],
// strictly ascending.  A device array is fetched first (one small copy and wait).
int le_fetch_cuts(l5dh_ctx* c, const uint32_t* cuts, uint32_t ncuts, LeCuts& out) {
  if (ncuts < 1 || ncuts > LE_MAX) return fail(c, -EINVAL, "le: ncuts must be in [1, 64]");
  if (!cuts) return fail(c, -EINVAL, "le: null cuts");
  memset(&out, 0, sizeof(out));
  if (int r = fetch_small(c, cuts, ncuts, out.c)) return r;
  for (uint32_t k = 0; k < ncuts; ++k) {
    if (out.c[k] < 1 || out.c[k] > (uint32_t)NL)
      return fail(c, -EINVAL, "le: cuts[" + std::to_string(k) + "] is outside [1, 1797]");
    if (k && out.c[k] <= out.c[k - 1])
      return fail(c, -EINVAL, "le: cuts[" + std::to_string(k) + "] does not ascend strictly");
  }
  return 0;
}

// Cumulative counts at the cuts of the live state rows of series [first, first + count)
// (ext == nullptr; then also the per-series snapshot / reset of the same state) or of
// external dense rows ext[count][1798].  The caller holds the lock and has checked the
// arguments; count > 0.
int do_le(l5dh_ctx* c, uint32_t first, uint32_t count, const int32_t* ext, const int64_t* ext_totals,
          const LeCuts& cuts, uint32_t K, uint64_t* le_out, int64_t* sums_out, int accumulate,
          l5dh_summary* series_out, int reset) {
  int r;
  const bool live = ext == nullptr;
  if (live && (r = live_begin(c))) return r;
  StagedOut<uint64_t> le;
  StagedOut<int64_t> sums;
  StagedOut<Summary88> s_summ;
  // (the copies are not timed here, as in l5dh_summarize_dense and l5dh_export_state)
  if ((r = stage_in(c, ext, (size_t)count * NB, 8, c->stage_in_counts)) ||
      (r = stage_in(c, ext_totals, count, 8, c->stage_in_totals)) ||
      (r = le.begin(c, le_out, (size_t)count * (K + 1), c->le_stage)) ||
      (r = sums.begin(c, sums_out, count, c->le_sums_stage)) ||
      (r = s_summ.begin(c, series_out, count, c->stage_summ)))
    return r;
  // (an accumulating host output: its old values are staged in)
  if (accumulate && ((r = le.load(c)) || (r = sums.load(c)))) return r;
  {
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, launch_le(state(c), first, count, ext, ext_totals, cuts, K, le.dev, sums.dev, accumulate, c->stream));
    // the per-series snapshot and the reset of the same range, from the same state
    if (live && (s_summ.dev || reset) && (r = rows_of_range(c, first, count, s_summ.dev, reset))) return r;
  }
  if ((r = le.end(c)) || (r = sums.end(c)) || (r = s_summ.end(c))) return r;
  return sync_stream(c);
}

// ---- configurable quantiles ---------------------------------------------------------
// The quantiles of a call, on the host and checked: K in [1, Q_MAX], each q in [0, 1]
// (NaN fails both comparisons).  A device array is fetched first (one small copy and wait).
int quant_fetch_q(l5dh_ctx* c, const double* q, uint32_t nq, QuantQ& out) {
  if (nq < 1 || nq > Q_MAX) return fail(c, -EINVAL, "quantiles: nq must be in [1, 64]");
  if (!q) return fail(c, -EINVAL, "quantiles: null q");
  memset(&out, 0, sizeof(out));
  if (int r = fetch_small(c, q, nq, out.q)) return r;
  for (uint32_t k = 0; k < nq; ++k)
    if (!(out.q[k] >= 0.0 && out.q[k] <= 1.0))
      return fail(c, -EINVAL, "quantiles: q[" + std::to_string(k) + "] is not in [0, 1]");
  return 0;
}

// The quantiles of the live state rows of series [first, first + count) (ext == nullptr;
// then also the per-series snapshot / reset of the same state) or of external dense rows
// ext[count][1798].  The caller holds the lock and has checked the arguments; count > 0.
int do_quant(l5dh_ctx* c, uint32_t first, uint32_t count, const int32_t* ext, const QuantQ& qs, uint32_t K,
             int64_t* q_out, l5dh_summary* series_out, int reset) {
  int r;
  const bool live = ext == nullptr;
  if (live && (r = live_begin(c))) return r;
  StagedOut<int64_t> qo;
  StagedOut<Summary88> s_summ;
  // (the copies are not timed here, as in l5dh_summarize_dense and l5dh_le)
  if ((r = stage_in(c, ext, (size_t)count * NB, 8, c->stage_in_counts)) ||
      (r = qo.begin(c, q_out, (size_t)count * K, c->q_stage)) ||
      (r = s_summ.begin(c, series_out, count, c->stage_summ)))
    return r;
  {
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, launch_quant(state(c), first, count, ext, qs, K, tables(c).mid, qo.dev, c->stream));
    // the per-series snapshot and the reset of the same range, from the same state
    if (live && (s_summ.dev || reset) && (r = rows_of_range(c, first, count, s_summ.dev, reset))) return r;
  }
  if ((r = qo.end(c)) || (r = s_summ.end(c))) return r;
  return sync_stream(c);
}

// ---- top-k selection ------------------------------------------------------------------
// What to rank by and whom: the checked arguments the two entry points share.
struct TopQuery {
  int by;             // 0 .. 10: the summary field; L5DH_BY_QUANTILE: percentile(q) of the live row
  double q;
  int order;          // L5DH_TOP_LARGEST / L5DH_TOP_SMALLEST
  int64_t min_count;
  const uint32_t* group;  // nullable
  uint32_t g, k;
};

// -EINVAL for everything a selection can be asked wrongly, before anything is enqueued.
// by_max: the largest `by` the entry point takes.
int top_check(l5dh_ctx* c, const TopQuery& t, int by_max, const void* ids_out, const void* n_out) {
  if (t.k < 1 || t.k > L5DH_TOP_LIMIT) return fail(c, -EINVAL, "top: k must be in [1, 1024]");
  if (t.by < 0 || t.by > by_max) return fail(c, -EINVAL, "top: unknown `by` for this call");
  if (t.order != L5DH_TOP_LARGEST && t.order != L5DH_TOP_SMALLEST) return fail(c, -EINVAL, "top: order must be 0 or 1");
  if (t.min_count < 0) return fail(c, -EINVAL, "top: min_count must be >= 0");
  if (t.by == L5DH_BY_QUANTILE && !(t.q >= 0.0 && t.q <= 1.0)) return fail(c, -EINVAL, "top: q is not in [0, 1]");
  if (!ids_out || !n_out) return fail(c, -EINVAL, "top: null ids_out or n_out");
  return 0;
}

// A u32 to the caller's host or device word.
int top_put_n(l5dh_ctx* c, uint32_t* n_out, uint32_t v) {
  if (!is_device_ptr(n_out)) {
    *n_out = v;
    return 0;
  }
  HIPCHK(c, hipMemcpyAsync(n_out, &v, 4, hipMemcpyHostToDevice, c->stream));
  return sync_stream(c);
}

// The k best of `count` rows: the live state rows of series [first, first + count) (ext ==
// nullptr; then also the K = 1 quantile pass, the per-series snapshot and the reset of the
// same state) or external summaries ext[count] (first == 0).  The caller holds the lock and
// has checked the arguments; 0 < count <= TOP_MAX_ROWS.
int do_top(l5dh_ctx* c, uint32_t first, uint32_t count, const Summary88* ext, const TopQuery& t, uint32_t* ids_out,
           l5dh_summary* top_out, int64_t* q_out, uint32_t* n_out, l5dh_summary* series_out, int reset) {
  int r;
  const bool live = ext == nullptr;
  const bool byq = t.by == L5DH_BY_QUANTILE;
  const uint32_t kp = top_kp(t.k);
  if (live && (r = live_begin(c))) return r;
  StagedOut<Summary88> s_summ, top;
  StagedOut<uint32_t> ids;
  StagedOut<int64_t> qo;
  const uint32_t* group = t.group;
  // (the copies are not timed here, as in l5dh_summarize_dense and l5dh_quantiles)
  if ((r = stage_in(c, ext, count, 8, c->top_vals)) || (r = stage_in(c, group, count, 4, c->top_group)) ||
      (r = ensure(c, c->top_list_a, top_bytes_a(count, kp))) || (r = ensure(c, c->top_list_b, top_bytes_b(count, kp))) ||
      (r = ensure(c, c->top_n, 4)) || (r = ids.begin(c, ids_out, t.k, c->top_ids, 4)) ||
      (r = top.begin(c, top_out, t.k, c->top_summ)) || (r = qo.begin(c, byq ? q_out : nullptr, t.k, c->top_qout)))
    return r;
  // the rows ranked: the external ones, or the live range's summaries in series_out's
  // (staged) buffer, or in the same staging buffer as scratch
  Summary88* live_rows = nullptr;
  if (live) {
    if ((r = s_summ.begin(c, series_out, count, c->stage_summ))) return r;
    live_rows = s_summ.dev;
    if (!live_rows) {
      if ((r = ensure(c, c->stage_summ, (size_t)count * sizeof(Summary88)))) return r;
      live_rows = c->stage_summ.as<Summary88>();
    }
    if (byq && (r = ensure(c, c->top_q, (size_t)count * 8))) return r;
  }
  TopArgs a{};
  a.summ = live ? live_rows : ext;
  a.qv = byq ? c->top_q.as<const int64_t>() : nullptr;
  a.group = group;
  a.g = t.g;
  a.n = count;
  a.first = first;
  a.by = (uint32_t)t.by;
  a.smallest = t.order == L5DH_TOP_SMALLEST;
  a.min_count = t.min_count;
  a.k = t.k;
  a.list_a = c->top_list_a.as<TopItem>();
  a.list_b = c->top_list_b.as<TopItem>();
  a.ids_out = ids.dev;
  a.top_out = top.dev;
  a.q_out = qo.dev;
  a.n_out = c->top_n.as<uint32_t>();
  a.n_out2 = is_device_ptr(n_out) ? n_out : nullptr;
  {
    KTimer kt(c, L5DH_K_HOT);
    if (live) {
      if (byq) {  // the existing kernel with K = 1, before any reset
        QuantQ qs;
        memset(&qs, 0, sizeof(qs));
        qs.q[0] = t.q;
        HIPCHK(c, launch_quant(state(c), first, count, nullptr, qs, 1, tables(c).mid, c->top_q.as<int64_t>(), c->stream));
      }
      // the per-series summaries and the reset of the same range, from the same state
      if ((r = rows_of_range(c, first, count, live_rows, reset))) return r;
    }
    HIPCHK(c, launch_top(a, c->stream));
  }
  // the number of winners: what the host copies back of staged outputs, and no more
  uint32_t m = 0;
  HIPCHK(c, hipMemcpyAsync(&m, a.n_out, 4, hipMemcpyDeviceToHost, c->stream));
  if ((r = sync_stream(c))) return r;
  if (m > t.k) return fail(c, -EIO, "internal: top-k count out of range");
  if (!a.n_out2) *n_out = m;
  if (m && ids.staged()) HIPCHK(c, hipMemcpyAsync(ids.user, ids.dev, (size_t)m * 4, hipMemcpyDefault, c->stream));
  if (m && top.staged())
    HIPCHK(c, hipMemcpyAsync(top.user, top.dev, (size_t)m * sizeof(Summary88), hipMemcpyDefault, c->stream));
  if (m && qo.staged()) HIPCHK(c, hipMemcpyAsync(qo.user, qo.dev, (size_t)m * 8, hipMemcpyDefault, c->stream));
  if ((r = s_summ.end(c))) return r;
  return sync_stream(c);
}

// ---- state import and sparse export -------------------------------------------------
// The status words of an import, read in one copy and one wait.
int imp_read_status(l5dh_ctx* c, uint32_t (&hs)[IS_WORDS]) {
  HIPCHK(c, hipMemcpyAsync(hs, c->imp_status.p, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
  return sync_stream(c);
}

// Dense rows into series [first, first + count).  The caller holds the lock and has checked
// the range; count > 0.  Nothing is flushed or folded: the ring's samples and the pending
// segments are summed onto the rows by whichever snapshot comes next.
int do_import_dense(l5dh_ctx* c, uint32_t first, uint32_t count, const int32_t* counts, const int64_t* totals) {
  int r;
  if ((r = ensure(c, c->imp_status, IS_WORDS * 4))) return r;
  // (the copies are not timed here, as in l5dh_summarize_dense and l5dh_export_state)
  if ((r = stage_in(c, counts, (size_t)count * NB, 8, c->stage_in_counts)) ||
      (r = stage_in(c, totals, count, 8, c->stage_in_totals)))
    return r;
  uint32_t* status = c->imp_status.as<uint32_t>();
  {
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, import_status_init(status, c->stream));
    HIPCHK(c, import_dense(state(c), first, count, counts, totals, status, c->stream));
  }
  uint32_t hs[IS_WORDS];
  if ((r = imp_read_status(c, hs))) return r;
  if (hs[IS_BAD] == IS_NONE && hs[IS_RANGE] == IS_NONE) return 0;
  {  // the same rows out again: the state reads as it did before the call
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, import_dense_undo(state(c), first, count, counts, totals, c->stream));
  }
  if ((r = sync_stream(c))) return r;
  if (hs[IS_BAD] != IS_NONE)
    return fail(c, -EINVAL, "import_state: a negative count in the row of series " + std::to_string(hs[IS_BAD]));
  return fail(c, -ERANGE, "import_state: a bucket sum of series " + std::to_string(hs[IS_RANGE]) + " exceeds 2^31 - 1");
}

// CSR rows into the state.  The caller holds the lock; n > 0.
int do_import_sparse(l5dh_ctx* c, const uint32_t* series, uint32_t first, size_t n, const uint64_t* row_off,
                     const BucketEntry* entries, const int64_t* totals) {
  int r;
  if (!row_off) return fail(c, -EINVAL, "import_sparse: null row_off");
  if (n > c->S) return fail(c, -EINVAL, "import_sparse: more rows than series");
  if (!series && (uint64_t)first + n > c->S) return fail(c, -EINVAL, "series range out of bounds");
  // the entry count: row_off[n] (a device array: one small copy and wait)
  uint64_t n_entries = 0;
  if ((r = fetch_small(c, row_off + n, 1, &n_entries))) return r;
  if (n_entries && !entries) return fail(c, -EINVAL, "import_sparse: null entries");
  // more entries than n full rows: some row's offsets are wrong -- the check finds the least
  // such row from the offsets alone (no entry is staged or read)
  const bool offsets_only = n_entries > (uint64_t)n * NB;
  if (offsets_only) entries = nullptr;
  if ((r = ensure(c, c->imp_status, IS_WORDS * 4)) || (r = ensure(c, c->imp_tflag, (size_t)c->F * 4)) ||
      (r = ensure(c, c->imp_list, (size_t)c->F * 4)))
    return r;
  if ((r = stage_in(c, series, n, 4, c->imp_series)) || (r = stage_in(c, row_off, n + 1, 8, c->imp_off)) ||
      (r = stage_in(c, entries, (size_t)n_entries, 8, c->imp_entries)) ||
      (r = stage_in(c, totals, n, 8, c->stage_in_totals)))
    return r;
  const SparseRows rows{series, first, (uint32_t)n, row_off, entries, totals, n_entries};
  uint32_t* status = c->imp_status.as<uint32_t>();
  uint32_t hs[IS_WORDS];
  {
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, import_status_init(status, c->stream));
    HIPCHK(c, import_sparse_check(rows, c->S, status, c->stream));
  }
  // no state is touched before the host has read the check's findings
  if ((r = imp_read_status(c, hs))) return r;
  if (hs[IS_BAD] != IS_NONE)
    return fail(c, -EINVAL,
                "import_sparse: row " + std::to_string(hs[IS_BAD]) +
                    " is invalid (offsets, series id, bucket order or range, or a count above 2^31 - 1)");
  if (offsets_only) return fail(c, -EIO, "internal: import_sparse offsets");
  {
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, import_sparse(state(c), rows, c->imp_tflag.as<uint32_t>(), c->imp_list.as<uint32_t>(), status, c->stream));
  }
  if ((r = imp_read_status(c, hs))) return r;
  if (hs[IS_RANGE] == IS_NONE) return 0;
  {
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, import_sparse_undo(state(c), rows, c->stream));
  }
  if ((r = sync_stream(c))) return r;
  return fail(c, -ERANGE, "import_sparse: a bucket sum of series " + std::to_string(hs[IS_RANGE]) + " exceeds 2^31 - 1");
}

// The CSR of the non-empty buckets of series [first, first + count).  The caller holds the
// lock and has checked the arguments; count > 0.
int do_export_sparse(l5dh_ctx* c, uint32_t first, uint32_t count, uint64_t* row_off, BucketEntry* entries, size_t cap,
                     size_t* n_entries, int64_t* totals, int reset) {
  int r = live_begin(c);
  if (r) return r;
  // the entry count: one host wait, before anything of the caller's is written
  uint64_t total = 0;
  auto rows = [&](uint32_t* cnt) { return export_sparse_count(state(c), first, count, cnt, c->stream); };
  if ((r = count_scan(c, count, c->xs_cnt, c->xs_offs, c->xs_tmp, rows, &total))) return r;
  const uint64_t* offs = c->xs_offs.as<uint64_t>();
  *n_entries = (size_t)total;
  if (!entries) return 0;  // a size query
  if (cap < total)
    return fail(c, -ERANGE, "export_sparse: " + std::to_string(total) + " entries, room for " + std::to_string(cap));
  StagedOut<BucketEntry> ent;
  StagedOut<int64_t> tot;
  if ((r = ent.begin(c, entries, (size_t)total, c->xs_entries)) || (r = tot.begin(c, totals, count, c->stage_totals)))
    return r;
  {
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, export_sparse_write(state(c), first, count, offs, ent.dev, tot.dev, c->stream));
    // the reset of the same range, from the same state
    if (reset && (r = rows_of_range(c, first, count, nullptr, reset))) return r;
  }
  HIPCHK(c, hipMemcpyAsync(row_off, offs, ((size_t)count + 1) * 8, hipMemcpyDefault, c->stream));
  if ((r = ent.end(c)) || (r = tot.end(c))) return r;  // (the copies are not timed here)
  return sync_stream(c);
}

// ---- the device renderer -----------------------------------------------------------
// Bytes of a name array that is not used in place: its offsets' last entry (the write
// pass, the only reader of the bytes, runs after every offset was found ascending).
int rd_stage_bytes(l5dh_ctx* c, const uint8_t*& bytes, const uint64_t* off, size_t n, DevBuf& stage) {
  if (direct(bytes, 1)) return 0;
  uint64_t last = 0;
  if (int r = fetch_small(c, off + n, 1, &last)) return r;
  if (last && !bytes) return fail(c, -EINVAL, "render: null name bytes under non-empty offsets");
  return stage_in(c, bytes, (size_t)last, 1, stage);
}

// A finding of the passes: its flag word holds the least row that has it (0xFFFFFFFF:
// none), and the call fails with `code` and the text before + the row + after.
struct Finding {
  int word, code;
  const char *before, *after;
};
constexpr uint32_t TEXT_FLAG_WORDS = RF_WORDS > IF_WORDS ? RF_WORDS : IF_WORDS;  // rd_flags serves either renderer

// In the order of precedence.
const Finding RENDER_FINDINGS[] = {
    {RF_KIND, -EINVAL, "render: the kind of row ", " is not one the call prints"},
    {RF_BADIDX, -EINVAL, "render: index of row ", " is not < nvalues"},
    {RF_BADOFF, -EINVAL, "render: key_off or lab_off descends at row ", ""},
    {RF_LONG, -EINVAL, "render: key and label text of row ", " exceed 2^25 bytes"},
    {RF_RANGE, -ERANGE, "render: avg or gauge of row ", " is outside +-[2^-64, 2^64), 0, NaN, Infinity"},
    {RF_MISMATCH, -EIO, "internal: the render passes disagree on the length of row ", ""},
};
const Finding INFLUX_FINDINGS[] = {
    {IF_KIND, -EINVAL, "render_influx: the kind of row ", " is none of the three"},
    {IF_FIELD, -EINVAL, "render_influx: field of row ", " is above 10"},
    {IF_BADIDX, -EINVAL, "render_influx: index of row ", " is not < the count of its kind"},
    {IF_LINE, -EINVAL, "render_influx: line of row ", " is not < nlines, or descends"},
    {IF_KEYOFF, -EINVAL, "render_influx: key_off descends at row ", ""},
    {IF_LINEOFF, -EINVAL, "render_influx: head_off or tail_off descends at the line of row ", ""},
    {IF_LONG, -EINVAL, "render_influx: head, host, tail and key of row ", " exceed 2^25 bytes"},
    {IF_RANGE, -ERANGE, "render_influx: avg of row ", " is outside +-[2^-64, 2^64), 0, NaN, Infinity"},
    {IF_MISMATCH, -EIO, "internal: the render_influx passes disagree on the length of row ", ""},
};

template <size_t N>
int findings(l5dh_ctx* c, const Finding (&table)[N], const uint32_t* f) {
  for (const Finding& t : table)
    if (f[t.word] != 0xFFFFFFFFu) return fail(c, t.code, t.before + std::to_string(f[t.word]) + t.after);
  return 0;
}

// The two passes of a text over n > 0 rows, from the flag words' 0xFF to the second reading
// of the findings.  name: the call's, for the messages; lengths(len, flags) and
// write(offs, out, flags) launch the renderer's passes over inputs the caller staged.  The
// caller holds the lock and has checked the arguments.  braces: the rows' text is the
// inside of one JSON object -- it goes from out + 1, `{` goes to out[0] and `}` over the
// last entry's comma (no entry at all: `{}`).
template <size_t N, class Lengths, class Write>
int text_passes(l5dh_ctx* c, const char* name, const Finding (&table)[N], size_t n, Lengths&& lengths, Write&& write,
                bool braces, uint8_t* out, size_t cap, size_t* len) {
  int r;
  if ((r = ensure(c, c->rd_flags, TEXT_FLAG_WORDS * 4))) return r;
  uint32_t* flags = c->rd_flags.as<uint32_t>();
  auto count = [&](uint32_t* row_len) {
    const hipError_t e = hipMemsetAsync(flags, 0xFF, TEXT_FLAG_WORDS * 4, c->stream);
    return e != hipSuccess ? e : lengths(row_len, flags);
  };
  if ((r = count_scan(c, (uint32_t)n, c->rd_len, c->rd_offs, c->rd_tmp, count))) return r;
  const uint64_t* offs = c->rd_offs.as<uint64_t>();
  // the device's findings and the text's length: one host wait, before anything is written
  uint32_t hf[TEXT_FLAG_WORDS];
  uint64_t total = 0;
  HIPCHK(c, hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&total, offs + n, 8, hipMemcpyDeviceToHost, c->stream));
  if ((r = sync_stream(c)) || (r = findings(c, table, hf))) return r;
  const uint64_t rows_total = total;
  if (braces) total = total ? total + 1 : 2;
  if (len) *len = (size_t)total;
  if (!out) return 0;  // a size query
  if (cap < total)
    return fail(c, -ERANGE,
                std::string(name) + ": the text takes " + std::to_string(total) + " bytes, cap is " + std::to_string(cap));
  StagedOut<uint8_t> o;
  if ((r = o.begin(c, out, (size_t)total, c->rd_out, 1))) return r;
  {
    KTimer kt(c, L5DH_K_HOT);
    if (rows_total) HIPCHK(c, write(offs, o.dev + (braces ? 1 : 0), flags));
    if (braces) {
      HIPCHK(c, hipMemsetAsync(o.dev, '{', 1, c->stream));
      HIPCHK(c, hipMemsetAsync(o.dev + total - 1, '}', 1, c->stream));
    }
  }
  {
    KTimer kt(c, L5DH_K_COPY);
    if ((r = o.end(c))) return r;
    HIPCHK(c, hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, c->stream));
  }
  if ((r = sync_stream(c))) return r;
  return findings(c, table, hf);
}

// A render call over n > 0 rows: stages the names, then the passes; rows holds device
// pointers (the caller staged the values).  braces: text_passes', and names' label text is
// not read.
template <class Rows>
int do_render(l5dh_ctx* c, const l5dh_names* names, size_t n, size_t nvalues, const Rows& rows, uint8_t* out, size_t cap,
              size_t* len, bool braces = false) {
  int r;
  RenderNames nm{names->index, names->key_off, names->key_bytes, braces ? nullptr : names->lab_off,
                 braces ? nullptr : names->lab_bytes};
  {
    KTimer kt(c, L5DH_K_COPY);
    if ((r = rd_stage_bytes(c, nm.key_bytes, names->key_off, n, c->rd_kbytes)) ||
        (nm.lab_off && (r = rd_stage_bytes(c, nm.lab_bytes, names->lab_off, n, c->rd_lbytes))) ||
        (r = stage_in(c, nm.index, n, 4, c->rd_index)) || (r = stage_in(c, nm.key_off, n + 1, 8, c->rd_koff)) ||
        (r = stage_in(c, nm.lab_off, n + 1, 8, c->rd_loff)))
      return r;
  }
  return text_passes(
      c, "render", RENDER_FINDINGS, n,
      [&](uint32_t* row_len, uint32_t* flags) {
        return render_lengths(nm, (uint32_t)n, (uint32_t)nvalues, rows, row_len, flags, c->stream);
      },
      [&](const uint64_t* offs, uint8_t* dst, uint32_t* flags) {
        return render_write(nm, (uint32_t)n, rows, offs, dst, flags, c->stream);
      },
      braces, out, cap, len);
}

// The arguments both render calls share.  0: go on; 1: n == 0, done; negative: an error.
int rd_check(l5dh_ctx* c, const l5dh_names* names, size_t n, const void* values, size_t nvalues, size_t* len) {
  if (len) *len = 0;
  if (!names || !names->key_off || !names->lab_off) return fail(c, -EINVAL, "render: null names, key_off or lab_off");
  if (n == 0) return 1;
  if (nvalues == 0 || !values) return fail(c, -EINVAL, "render: no values for the rows");
  if (n > 0xFFFFFFF0ull || nvalues > 0xFFFFFFFFull) return fail(c, -EINVAL, "render: more than 2^32 - 16 rows");
  return 0;
}

// The kind arrays of a call (k holds the caller's pointers and counts): staged where they
// are not used in place, and the n rows' slots sized.  No timer: the caller's.
int rd_stage_kinds(l5dh_ctx* c, KindRows& k, size_t n) {
  int r;
  if ((r = stage_in(c, k.kinds, n, 1, c->rd_kinds)) || (r = stage_in(c, k.summaries, (size_t)k.nsummaries, 8, c->rd_vals)) ||
      (r = stage_in(c, k.counters, (size_t)k.ncounters, 8, c->rd_counters)) ||
      (r = stage_in(c, k.gauges, (size_t)k.ngauges, 4, c->rd_gauges)) || (r = ensure(c, c->rd_avg, n * RENDER_AVG_SLOT)))
    return r;
  k.slot = c->rd_avg.as<uint8_t>();
  return 0;
}

// The arguments the JSON and the scalar call share, and their staged values.  0: go on;
// 1: n == 0; negative: an error.
int rd_kind_check(l5dh_ctx* c, const l5dh_names* names, const uint8_t* kinds, size_t n, bool labels, KindRows& k,
                  size_t nsummaries, size_t ncounters, size_t ngauges, size_t* len) {
  if (len) *len = 0;
  if (!names || !names->key_off || (labels && !names->lab_off))
    return fail(c, -EINVAL, labels ? "render: null names, key_off or lab_off" : "render: null names or key_off");
  if ((nsummaries && !k.summaries) || (ncounters && !k.counters) || (ngauges && !k.gauges))
    return fail(c, -EINVAL, "render: a null value array with a count above 0");
  if (n == 0) return 1;
  if (!kinds) return fail(c, -EINVAL, "render: null kinds");
  if (n > 0xFFFFFFF0ull || nsummaries > 0xFFFFFFFFull || ncounters > 0xFFFFFFFFull || ngauges > 0xFFFFFFFFull)
    return fail(c, -EINVAL, "render: more than 2^32 - 16 rows");
  k.kinds = kinds;
  k.nsummaries = (uint32_t)nsummaries;
  k.ncounters = (uint32_t)ncounters;
  k.ngauges = (uint32_t)ngauges;
  KTimer kt(c, L5DH_K_COPY);
  return rd_stage_kinds(c, k, n);
}

// ---- the InfluxDB renderer -----------------------------------------------------------
// The passes over n > 0 rows.  The caller holds the lock and has checked the arguments; r
// holds the caller's pointers and counts, staged here where they are not used in place.
int do_render_influx(l5dh_ctx* c, InfluxRows r, size_t n, uint8_t* out, size_t cap, size_t* len) {
  int rc;
  const size_t nl = r.nlines;
  const uint64_t *koff = r.key_off, *hoff = r.head_off, *toff = r.tail_off;  // (the caller's: rd_stage_bytes reads their ends)
  {
    KTimer kt(c, L5DH_K_COPY);
    if ((rc = rd_stage_bytes(c, r.key_bytes, koff, n, c->rd_kbytes)) ||
        (rc = rd_stage_bytes(c, r.head_bytes, hoff, nl, c->ifx_hbytes)) ||
        (rc = rd_stage_bytes(c, r.tail_bytes, toff, nl, c->ifx_tbytes)) ||
        (rc = stage_in(c, r.line, n, 4, c->ifx_line)) || (rc = stage_in(c, r.field, n, 1, c->ifx_field)) ||
        (rc = stage_in(c, r.index, n, 4, c->rd_index)) || (rc = stage_in(c, r.key_off, n + 1, 8, c->rd_koff)) ||
        (rc = stage_in(c, r.head_off, nl + 1, 8, c->ifx_hoff)) || (rc = stage_in(c, r.tail_off, nl + 1, 8, c->ifx_toff)) ||
        (rc = stage_in(c, r.host, (size_t)r.host_len, 1, c->ifx_host)) ||
        (rc = rd_stage_kinds(c, r.k, n)))
      return rc;
  }
  return text_passes(
      c, "render_influx", INFLUX_FINDINGS, n,
      [&](uint32_t* row_len, uint32_t* flags) { return influx_lengths(r, (uint32_t)n, row_len, flags, c->stream); },
      [&](const uint64_t* offs, uint8_t* dst, uint32_t* flags) {
        return influx_write(r, (uint32_t)n, offs, dst, flags, c->stream);
      },
      false, out, cap, len);
}

}  // namespace

extern "C" {

int l5dh_rollup(l5dh_ctx* c, uint32_t first, uint32_t count, const uint32_t* group, uint32_t ngroups,
                l5dh_summary* g_out, int32_t* g_counts_out, int64_t* g_totals_out, l5dh_summary* series_out,
                int reset) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (int r = check_range(c, first, count)) return r;
  if (ngroups == 0 || ngroups > L5DH_MAX_SERIES) return fail(c, -EINVAL, "rollup: ngroups must be in [1, 2^20]");
  if (!group) return fail(c, -EINVAL, "rollup: null group map");
  return do_rollup(c, first, count, nullptr, nullptr, group, ngroups, g_out, g_counts_out, g_totals_out, series_out,
                   reset);
}

int l5dh_rollup_dense(l5dh_ctx* c, const int32_t* counts, const int64_t* totals, size_t n, const uint32_t* group,
                      uint32_t ngroups, l5dh_summary* g_out, int32_t* g_counts_out, int64_t* g_totals_out) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (n > 0xFFFFFFF0ull) return fail(c, -EINVAL, "rollup: more than 2^32 - 16 dense rows");
  if (ngroups == 0 || ngroups > L5DH_MAX_SERIES) return fail(c, -EINVAL, "rollup: ngroups must be in [1, 2^20]");
  if (!group) return fail(c, -EINVAL, "rollup: null group map");
  if (n && !counts) return fail(c, -EINVAL, "rollup: null dense rows");
  // (n == 0: the kernels never read a row; a non-null marker selects the dense source)
  static const int32_t none = 0;
  return do_rollup(c, 0, (uint32_t)n, n ? counts : &none, n ? totals : nullptr, group, ngroups, g_out, g_counts_out,
                   g_totals_out, nullptr, 0);
}

int l5dh_le_cuts(const double* bounds, size_t n, uint32_t* cuts, int64_t* le) { return le_cuts(bounds, n, cuts, le); }

int l5dh_le(l5dh_ctx* c, uint32_t first, uint32_t count, const uint32_t* cuts, uint32_t ncuts, uint64_t* le_out,
            int64_t* sums_out, int accumulate, l5dh_summary* series_out, int reset) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (int r = check_range(c, first, count)) return r;
  LeCuts lc;
  if (int r = le_fetch_cuts(c, cuts, ncuts, lc)) return r;
  if (count == 0) return 0;
  if (!le_out) return fail(c, -EINVAL, "le: null output");
  return do_le(c, first, count, nullptr, nullptr, lc, ncuts, le_out, sums_out, accumulate, series_out, reset);
}

int l5dh_le_dense(l5dh_ctx* c, const int32_t* counts, const int64_t* totals, size_t n, const uint32_t* cuts,
                  uint32_t ncuts, uint64_t* le_out, int64_t* sums_out, int accumulate) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (n > 0xFFFFFFFFull) return fail(c, -EINVAL, "le: more than 2^32 - 1 dense rows");
  LeCuts lc;
  if (int r = le_fetch_cuts(c, cuts, ncuts, lc)) return r;
  if (n == 0) return 0;
  if (!counts || !le_out) return fail(c, -EINVAL, "le: null dense rows or output");
  return do_le(c, 0, (uint32_t)n, counts, totals, lc, ncuts, le_out, sums_out, accumulate, nullptr, 0);
}

int l5dh_quantiles(l5dh_ctx* c, uint32_t first, uint32_t count, const double* q, uint32_t nq, int64_t* q_out,
                   l5dh_summary* series_out, int reset) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (int r = check_range(c, first, count)) return r;
  QuantQ qs;
  if (int r = quant_fetch_q(c, q, nq, qs)) return r;
  if (count == 0) return 0;
  if (!q_out) return fail(c, -EINVAL, "quantiles: null output");
  return do_quant(c, first, count, nullptr, qs, nq, q_out, series_out, reset);
}

int l5dh_quantiles_dense(l5dh_ctx* c, const int32_t* counts, size_t n, const double* q, uint32_t nq, int64_t* q_out) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (n > 0xFFFFFFFFull) return fail(c, -EINVAL, "quantiles: more than 2^32 - 1 dense rows");
  QuantQ qs;
  if (int r = quant_fetch_q(c, q, nq, qs)) return r;
  if (n == 0) return 0;
  if (!counts || !q_out) return fail(c, -EINVAL, "quantiles: null dense rows or output");
  return do_quant(c, 0, (uint32_t)n, counts, qs, nq, q_out, nullptr, 0);
}

int l5dh_top(l5dh_ctx* c, uint32_t first, uint32_t count, int by, double q, int order, int64_t min_count,
             const uint32_t* group, uint32_t g, uint32_t k, uint32_t* ids_out, l5dh_summary* top_out, int64_t* q_out,
             uint32_t* n_out, l5dh_summary* series_out, int reset) {
  if (!c) return -EINVAL;
  CtxLock lk(c);
  static_assert(L5DH_TOP_LIMIT == TOP_LIMIT && L5DH_BY_QUANTILE == TOP_BY_QUANTILE && L5DH_BY_AVG == TOP_BY_FIELDS - 1,
                "the header's constants are the kernels'");
  const TopQuery t{by, q, order, min_count, group, g, k};
  if (int r = top_check(c, t, L5DH_BY_QUANTILE, ids_out, n_out)) return r;
  if (int r = check_range(c, first, count)) return r;
  if (count == 0) return top_put_n(c, n_out, 0);
  return do_top(c, first, count, nullptr, t, ids_out, top_out, q_out, n_out, series_out, reset);
}

int l5dh_top_summaries(l5dh_ctx* c, const l5dh_summary* values, size_t n, int by, int order, int64_t min_count,
                       const uint32_t* group, uint32_t g, uint32_t k, uint32_t* ids_out, l5dh_summary* top_out,
                       uint32_t* n_out) {
  if (!c) return -EINVAL;
  CtxLock lk(c);
  const TopQuery t{by, 0.0, order, min_count, group, g, k};
  if (int r = top_check(c, t, L5DH_BY_AVG, ids_out, n_out)) return r;
  if (n > TOP_MAX_ROWS) return fail(c, -EINVAL, "top: more than 2^24 rows");
  if (n == 0) return top_put_n(c, n_out, 0);
  if (!values) return fail(c, -EINVAL, "top: null values");
  static_assert(sizeof(l5dh_summary) == sizeof(Summary88), "l5dh_summary layout");
  return do_top(c, 0, (uint32_t)n, reinterpret_cast<const Summary88*>(values), t, ids_out, top_out, nullptr, n_out,
                nullptr, 0);
}

int l5dh_import_state(l5dh_ctx* c, uint32_t first, uint32_t count, const int32_t* counts, const int64_t* totals) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (int r = check_range(c, first, count)) return r;
  if (count == 0) return 0;
  if (!counts) return fail(c, -EINVAL, "import_state: null counts");
  return do_import_dense(c, first, count, counts, totals);
}

int l5dh_export_sparse(l5dh_ctx* c, uint32_t first, uint32_t count, uint64_t* row_off, l5dh_bucket_entry* entries,
                       size_t cap, size_t* n_entries, int64_t* totals, int reset) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (int r = check_range(c, first, count)) return r;
  if (!n_entries) return fail(c, -EINVAL, "export_sparse: null n_entries");
  if (entries && !row_off) return fail(c, -EINVAL, "export_sparse: null row_off");
  if (count == 0) {
    *n_entries = 0;
    if (entries) {  // (an empty range still has its row_off[0] = 0)
      const uint64_t zero = 0;
      HIPCHK(c, hipMemcpyAsync(row_off, &zero, 8, hipMemcpyDefault, c->stream));
      return sync_stream(c);
    }
    return 0;
  }
  static_assert(sizeof(l5dh_bucket_entry) == sizeof(BucketEntry), "l5dh_bucket_entry layout");
  return do_export_sparse(c, first, count, row_off, reinterpret_cast<BucketEntry*>(entries), cap, n_entries, totals,
                          reset);
}

int l5dh_import_sparse(l5dh_ctx* c, const uint32_t* series, uint32_t first, size_t n, const uint64_t* row_off,
                       const l5dh_bucket_entry* entries, const int64_t* totals) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (n == 0) return 0;
  return do_import_sparse(c, series, first, n, row_off, reinterpret_cast<const BucketEntry*>(entries), totals);
}

int l5dh_format_double(double x, char* out, size_t* len) {
  if (!out || !len) return -EINVAL;
  const int n = fmt::format_double(x, out);
  *len = n < 0 ? 0 : (size_t)n;
  return n < 0 ? -ERANGE : 0;
}

int l5dh_format_float(float x, char* out, size_t* len) {
  if (!out || !len) return -EINVAL;
  const int n = fmt::format_float(x, out);
  *len = n < 0 ? 0 : (size_t)n;
  return n < 0 ? -ERANGE : 0;
}

int l5dh_format_long(int64_t v, char* out, size_t* len) {
  if (!out || !len) return -EINVAL;
  *len = (size_t)fmt::format_long(v, out);
  return 0;
}

int l5dh_format_ulong(uint64_t v, char* out, size_t* len) {
  if (!out || !len) return -EINVAL;
  *len = (size_t)fmt::format_ulong(v, out);
  return 0;
}

int l5dh_render_summaries(l5dh_ctx* c, const l5dh_names* names, size_t n, const l5dh_summary* values, size_t nvalues,
                          uint8_t* out, size_t cap, size_t* len) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  int r = rd_check(c, names, n, values, nvalues, len);
  if (r) return r < 0 ? r : 0;
  const Summary88* v = reinterpret_cast<const Summary88*>(values);
  {
    KTimer kt(c, L5DH_K_COPY);
    if ((r = stage_in(c, v, nvalues, 8, c->rd_vals))) return r;
  }
  if ((r = ensure(c, c->rd_avg, n * RENDER_AVG_SLOT))) return r;
  return do_render(c, names, n, nvalues, SummaryRows{v, c->rd_avg.as<uint8_t>()}, out, cap, len);
}

int l5dh_render_le(l5dh_ctx* c, const l5dh_names* names, size_t n, const uint64_t* le_rows, const int64_t* sums,
                   size_t nvalues, const int64_t* le, uint32_t ncuts, uint8_t* out, size_t cap, size_t* len) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (len) *len = 0;
  if (ncuts < 1 || ncuts > L5DH_LE_MAX) return fail(c, -EINVAL, "render: ncuts must be in [1, 64]");
  int r = rd_check(c, names, n, le_rows, nvalues, len);
  if (r) return r < 0 ? r : 0;
  if (!le) return fail(c, -EINVAL, "render: null le labels");
  {
    KTimer kt(c, L5DH_K_COPY);
    if ((r = stage_in(c, le_rows, nvalues * ((size_t)ncuts + 1), 8, c->rd_vals)) ||
        (r = stage_in(c, sums, nvalues, 8, c->rd_sums)) || (r = stage_in(c, le, (size_t)ncuts, 8, c->rd_le)))
      return r;
  }
  return do_render(c, names, n, nvalues, LeRows{le_rows, sums, le, ncuts}, out, cap, len);
}

int l5dh_render_quantiles(l5dh_ctx* c, const l5dh_names* names, size_t n, const int64_t* q_rows, size_t nvalues,
                          const double* q, uint32_t nq, uint8_t* out, size_t cap, size_t* len) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (len) *len = 0;
  QuantQ qs;
  int r = quant_fetch_q(c, q, nq, qs);
  if (r) return r;
  // the K labels, formatted once per call: Double.toString(q[k]), its length in the slot's last byte
  uint8_t labels[Q_MAX * RENDER_QLABEL_SLOT] = {0};
  static_assert(L5DH_DOUBLE_CHARS < RENDER_QLABEL_SLOT, "a label and its length share a slot");
  for (uint32_t k = 0; k < nq; ++k) {
    uint8_t* slot = labels + (size_t)k * RENDER_QLABEL_SLOT;
    const int m = fmt::format_double(qs.q[k], reinterpret_cast<char*>(slot));
    if (m < 0)
      return fail(c, -ERANGE, "render: q[" + std::to_string(k) + "] is outside +-[2^-64, 2^64), 0, NaN, Infinity");
    slot[RENDER_QLABEL_SLOT - 1] = (uint8_t)m;
  }
  r = rd_check(c, names, n, q_rows, nvalues, len);
  if (r) return r < 0 ? r : 0;
  const uint8_t* lab = labels;
  {
    KTimer kt(c, L5DH_K_COPY);
    if ((r = stage_in(c, q_rows, nvalues * (size_t)nq, 8, c->rd_vals)) ||
        (r = stage_in(c, lab, (size_t)nq * RENDER_QLABEL_SLOT, 1, c->rd_qlabels)))
      return r;
  }
  // (labels lives on this frame: do_render returns only after the stream has drained)
  return do_render(c, names, n, nvalues, QuantRows{q_rows, lab, nq}, out, cap, len);
}

int l5dh_render_json(l5dh_ctx* c, const l5dh_names* names, const uint8_t* kinds, size_t n, const l5dh_summary* summaries,
                     size_t nsummaries, const int64_t* counters, size_t ncounters, const float* gauges, size_t ngauges,
                     uint8_t* out, size_t cap, size_t* len) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  KindRows k{nullptr, reinterpret_cast<const Summary88*>(summaries), counters, gauges, 0u, 0u, 0u, nullptr};
  int r = rd_kind_check(c, names, kinds, n, false, k, nsummaries, ncounters, ngauges, len);
  if (r < 0) return r;
  if (r == 1) {  // the empty document
    if (len) *len = 2;
    if (!out) return 0;
    if (cap < 2) return fail(c, -ERANGE, "render: the text takes 2 bytes, cap is " + std::to_string(cap));
    HIPCHK(c, hipMemcpyAsync(out, "{}", 2, hipMemcpyDefault, c->stream));
    return sync_stream(c);
  }
  return do_render(c, names, n, 0, JsonRows{k}, out, cap, len, true);
}

int l5dh_render_scalars(l5dh_ctx* c, const l5dh_names* names, const uint8_t* kinds, size_t n, const int64_t* counters,
                        size_t ncounters, const float* gauges, size_t ngauges, uint8_t* out, size_t cap, size_t* len) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  KindRows k{nullptr, nullptr, counters, gauges, 0u, 0u, 0u, nullptr};
  int r = rd_kind_check(c, names, kinds, n, true, k, 0, ncounters, ngauges, len);
  if (r) return r < 0 ? r : 0;
  return do_render(c, names, n, 0, ScalarRows{k}, out, cap, len);
}

int l5dh_render_influx(l5dh_ctx* c, const l5dh_influx_names* names, size_t n, size_t nlines, const uint8_t* host,
                       size_t host_len, const l5dh_summary* summaries, size_t nsummaries, const int64_t* counters,
                       size_t ncounters, const float* gauges, size_t ngauges, uint8_t* out, size_t cap, size_t* len) {
  if (!c) return -EINVAL;
  CtxLock g(c);
  if (len) *len = 0;
  if (!names) return fail(c, -EINVAL, "render_influx: null names");
  if (n && (!names->line || !names->kinds || !names->field || !names->index || !names->key_off || !names->key_bytes ||
            !names->head_off || !names->head_bytes || !names->tail_off || !names->tail_bytes))
    return fail(c, -EINVAL, "render_influx: a null array of names");
  if (host_len && !host) return fail(c, -EINVAL, "render_influx: null host with a length above 0");
  if (host_len > 65535) return fail(c, -EINVAL, "render_influx: host_len above 65535");
  if ((nsummaries && !summaries) || (ncounters && !counters) || (ngauges && !gauges))
    return fail(c, -EINVAL, "render_influx: a null value array with a count above 0");
  if (n > 0xFFFFFFF0ull || nlines > 0xFFFFFFF0ull || nsummaries > 0xFFFFFFFFull || ncounters > 0xFFFFFFFFull ||
      ngauges > 0xFFFFFFFFull)
    return fail(c, -EINVAL, "render_influx: more than 2^32 - 16 rows or lines");
  if (n == 0) return 0;
  static_assert(sizeof(l5dh_summary) == sizeof(Summary88), "l5dh_summary layout");
  InfluxRows r{};
  r.k.kinds = names->kinds;
  r.k.summaries = reinterpret_cast<const Summary88*>(summaries);
  r.k.counters = counters;
  r.k.gauges = gauges;
  r.k.nsummaries = (uint32_t)nsummaries;
  r.k.ncounters = (uint32_t)ncounters;
  r.k.ngauges = (uint32_t)ngauges;
  r.line = names->line;
  r.field = names->field;
  r.index = names->index;
  r.key_off = names->key_off;
  r.key_bytes = names->key_bytes;
  r.head_off = names->head_off;
  r.head_bytes = names->head_bytes;
  r.tail_off = names->tail_off;
  r.tail_bytes = names->tail_bytes;
  r.host = host;
  r.host_len = (uint32_t)host_len;
  r.nlines = (uint32_t)nlines;
  return do_render_influx(c, r, n, out, cap, len);
}

}  // extern "C"
