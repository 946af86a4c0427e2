/*
 * l5dhist.h -- C-ABI of the MI355X latency-histogram engine (drop-in boundary).
 *
 * The boundary replaces the per-Stat arithmetic behind
 * io.buoyant.telemetry.Metric.Stat (reference: telemetry/core/src/main/scala/
 * io/buoyant/telemetry/Metric.scala:22-70) with a batched, device-resident
 * engine.  A JNI shim binds these symbols one-to-one; the
 * Scala side keeps Metric.Stat / HistogramSummary unchanged so exporters
 * (Prometheus, InfluxDB, admin metrics.json) consume the summaries as-is.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Any data pointer may be host memory
 *    (pageable or from l5dh_pin_alloc) or device memory (hipMalloc on the
 *    context's device); the library detects which.
 *  - Status codes: 0 = OK, negative errno otherwise (-EINVAL, -ENOMEM, -EIO,
 *    -ENODEV, -ERANGE).  The HIP/RCCL error text of the last failure is kept in
 *    l5dh_last_error(ctx).  No C++ exception crosses the ABI.
 *  - Every entry point taking a context is thread-safe (one lock per context).
 *  - The library never retains a caller pointer after a call returns, except
 *    buffers from l5dh_pin_alloc, which it owns.
 *
 * Series ids are dense uint32 ids assigned when a Stat is created
 * (reference: MetricsTree.mkStat, MetricsTree.scala:85-93), 0 <= id < max_series.
 */
#ifndef L5DHIST_H
#define L5DHIST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L5DH_ABI_VERSION 3 /* 3: count-free partition (no bin-mode / split-min tunables); id errors from l5dh_sync only */
#define L5DH_NLIMITS 1797  /* BucketedHistogram.scala:42 (0.5% error => 1797 limits) */
#define L5DH_NBUCKETS 1798 /* counts = limits.length + 1 (upstream finagle-stats) */
#define L5DH_MAX_SERIES (1u << 20) /* per context (= per GPU); shard wider fleets */

typedef struct l5dh_ctx l5dh_ctx;

/* Metric.HistogramSummary (Metric.scala:76-88): same fields, same order, 88 B. */
typedef struct {
  int64_t count;
  int64_t min;
  int64_t max;
  int64_t sum;
  int64_t p50;
  int64_t p90;
  int64_t p95;
  int64_t p99;
  int64_t p9990;
  int64_t p9999;
  double avg;
} l5dh_summary;

/* finagle-core BucketAndCount(lowerLimit, upperLimit, count) */
typedef struct {
  int32_t lower;
  int32_t upper;
  int32_t count;
} l5dh_bucket_count;

/* Tunables for l5dh_set_param */
enum {
  L5DH_PARAM_TIMING = 1,      /* 1: record HIP events around every kernel launch */
  L5DH_PARAM_COLD_LIMIT = 2,  /* max records for the single-pass tile path (<= 65535) */
  L5DH_PARAM_HOT_CHUNK = 3,   /* max records per work item on the big-tile path, 1024..2^20 (fewer when CUs would idle) */
  L5DH_PARAM_MAX_SEGMENTS = 4, /* binned ingest batches kept before folding (1..8) */
  L5DH_PARAM_DIRECT_MAX = 6,   /* tiles whose final records level 1 writes directly (0..255) */
  L5DH_PARAM_DIRECT_DIV = 7,   /* direct tiles hold >= 1/div records per 8K samples of the batch */
  L5DH_PARAM_STAGE_SAMPLES = 9, /* device staging ring for small batches, in samples (0: off) */
  L5DH_PARAM_MAX_SLABS = 10,   /* ingest slabs (workgroups of the level-1 kernel), 1..512 */
  L5DH_PARAM_MERGE_RCCL_1RANK = 11, /* 1: run the RCCL collective even in a 1-rank communicator (tests) */
  L5DH_PARAM_REGION_PCT = 13,  /* capacity of the partition's regions in percent of the prediction (1..1000,
                                  default 100); a region that overflows is redone with exact sizes, so values
                                  below 100 exercise that path (tests) and cost time, never results */
  L5DH_PARAM_ROLLUP_ITEM = 14, /* members per work item of a rollup (1..64, default 64; a group of more than
                                  1024 items' worth takes longer items); small values cut test-sized groups
                                  into several items (tests) and cost time, never results */
  L5DH_PARAM_VARIANT = 12      /* kernel variant bits for same-context A/B timing (0: the default kernels;
                                  every variant computes the same results; bit 0: one-tile folds in u16 bins;
                                  bit 1: DMA copies of pinned host batches; bit 2: every ingest batch's
                                  capacity plan made as for a first interval, from its sample alone;
                                  bit 3: l5dh_counters_add without the LDS claim table, one global atomic
                                  per add; other bits are ignored) */
};

/* Fleet-merge modes for l5dh_merge */
enum {
  L5DH_MERGE_REDUCE_SCATTER = 0, /* rank r receives the summed rows of its series slice */
  L5DH_MERGE_ALL_REDUCE = 1      /* every rank receives all summed rows */
};
#define L5DH_UNIQUE_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */

/* Kernel ids for l5dh_kernel_time */
enum {
  L5DH_K_COUNT = 0,  /* (unused: the partition has no counting pass) */
  L5DH_K_SCAN = 1,   /* the batch sample, the partition plans and the snapshot plan */
  L5DH_K_BIN = 2,    /* level-1 partition by super-tile and direct half-tile (+ its redo) */
  L5DH_K_ACCUM = 3,  /* LDS-private tile histograms + fused summary / dense flush */
  L5DH_K_HOT = 4,    /* big-tile init/finish and row summaries */
  L5DH_K_COPY = 5,   /* H2D/D2H staging copies */
  L5DH_K_BIN2 = 6,   /* level-2 partition (super-tile regions -> 16-bit per-key records, + its redo) */
  L5DH_K_MERGE = 7,  /* the RCCL collective of l5dh_merge */
  L5DH_K_WINDOW = 8, /* the sliding window's sum over its slots (l5dh_window_query) */
  L5DH_K_COUNTERS = 9, /* the counter space's batched add and rollup (l5dh_counters_add, l5dh_counters_rollup) */
  L5DH_K_NKERNELS = 10
};

/* Reference: BucketedHistogram() per Stat (MetricsTree.scala:88).  Opens a
 * context owning device state for max_series series on the single device
 * selected by device_mask (exactly one bit set; bit i = HIP device i). */
int l5dh_open(l5dh_ctx** out, uint32_t max_series, uint32_t device_mask);
int l5dh_close(l5dh_ctx* ctx);

/* Reference: BucketedHistogram.DefaultLimits (BucketedHistogram.scala:42-46).
 * Returns the 1797 limits (static storage); *n receives 1797. */
const int32_t* l5dh_limits(size_t* n);

/* Reference: Metric.Stat.add(Float) (Metric.scala:30-33), batched: adds
 * values[i] to series series[i] for i < n.  Integer-only effect, so order
 * independent.
 *
 * Small batches (n <= half the staging ring, L5DH_PARAM_STAGE_SAMPLES) are
 * appended to a device staging ring and binned together when it fills or at
 * the next snapshot / peek / export / merge / sync; larger batches are binned
 * at once.  The call does not wait for the binning kernels: host buffers may
 * be reused as soon as it returns (their copy has completed); device buffers
 * may be reused once it returns when the context runs on its own stream, and
 * in stream order when it runs on a caller stream (l5dh_set_stream).
 *
 * Returns 0 once the batch is accepted (queued), otherwise an error and nothing
 * of the batch was queued.  Samples with out-of-range ids are dropped; the kernels
 * detect them asynchronously and l5dh_sync reports -EINVAL for them (a
 * later ingest never carries an earlier batch's error: an error from l5dh_ingest
 * means this batch was not queued -- or, for a batch above 2^30 samples, only its
 * leading 2^30-sample pieces were); all valid samples are ingested. */
int l5dh_ingest(l5dh_ctx* ctx, const uint32_t* series, const float* values, size_t n);

/* The same without waiting for the copy of host buffers: *ticket identifies the
 * call, and the caller keeps the buffers unchanged until l5dh_ingest_wait(ctx,
 * ticket) returns (a JNI thread double-buffers its pinned staging this way, so
 * the PCIe copy of one buffer overlaps the filling of the other).  Tickets grow;
 * waiting for a ticket also completes every earlier one.  Device buffers follow
 * l5dh_ingest's rules, with the ticket standing for "consumed". */
int l5dh_ingest_async(l5dh_ctx* ctx, const uint32_t* series, const float* values, size_t n, uint64_t* ticket);
int l5dh_ingest_wait(l5dh_ctx* ctx, uint64_t ticket);

/* Reference: Metric.Stat.snapshot() + reset() per Stat as driven by
 * AdminMetricsExportTelemeter.snapshotHistograms (AdminMetricsExportTelemeter.scala:154-162),
 * batched over series [first, first+count).  out (nullable) receives one
 * l5dh_summary per series (Metric.scala:53-67); counts_out (nullable)
 * receives [count][1798] int32 bucket counts (what reset()/peek return, dense).
 * reset != 0 clears those series afterwards, atomically with the snapshot.
 * The call returns once the outputs are written, except when every output given
 * is device memory and the context runs on a caller stream (l5dh_set_stream):
 * then the outputs are stream ordered on that stream (no host wait). */
int l5dh_snapshot(l5dh_ctx* ctx, uint32_t first, uint32_t count, l5dh_summary* out,
                  int32_t* counts_out, int reset);

/* Reference: Metric.Stat.peek (Metric.scala:35-37) -> Seq[BucketAndCount].
 * Writes up to cap non-empty buckets of one series; *n_out = number of
 * non-empty buckets (may exceed cap). */
int l5dh_peek(l5dh_ctx* ctx, uint32_t series, l5dh_bucket_count* out, size_t cap, size_t* n_out);

/* Dense export of current state for the fleet merge (sample-sharded config):
 * counts [count][1798] int32 and totals [count] int64 (nullable).  reset as
 * in l5dh_snapshot. */
int l5dh_export_state(l5dh_ctx* ctx, uint32_t first, uint32_t count, int32_t* counts,
                      int64_t* totals, int reset);

/* Summaries of externally held dense state (e.g. after an RCCL reduce-scatter
 * of exported counts): counts [n][1798] int32, totals [n] int64.  Domain: every
 * count in [0, 2^31 - 1] (upstream's Int counts; negative counts are outside the
 * contract and not checked) and any row sum -- a row's count may pass 2^32 (up to
 * 1798 (2^31 - 1)); it and the percentile targets are carried in 64 bits. */
int l5dh_summarize_dense(l5dh_ctx* ctx, const int32_t* counts, const int64_t* totals, size_t n,
                         l5dh_summary* out);

/* Label rollups: the histogram of a union of series is the element-wise integer sum
 * of their bucket rows, so a group's summary is exact -- what ONE Stat would report
 * had it received every member's samples (Metric.scala:53-67 over the summed counts).
 * group[i] names the group of series first + i: a value < ngroups, or L5DH_NO_GROUP
 * (the series is in no group); anything else is -EINVAL, found on the device and
 * reported by this call (nothing is reset then).  Per group g < ngroups the outputs
 * (each nullable) receive: g_out[g] the summary, g_counts_out[g][1798] the summed
 * bucket counts, g_totals_out[g] the summed exact sums (an int64 that wraps like a
 * Java long).  A group without members, or whose members are all empty, gets a zero
 * row, total 0 and the all-zero summary.  A bucket sum above 2^31 - 1 (what an int32
 * row, and upstream's Int counts, can hold) is detected, never wrapped: the call
 * returns -ERANGE, l5dh_last_error names the first such group, the outputs are
 * unspecified and nothing is reset.  count == 0 (n == 0) still writes ngroups empty
 * results.  ngroups is in [1, L5DH_MAX_SERIES]. */
#define L5DH_NO_GROUP 0xFFFFFFFFu

/* Live state.  Under ONE hold of the context lock: staged samples are binned
 * and pending segments folded; the rows of series [first, first+count) are
 * summed per group into g_* (each nullable; ngroups rows); then, if
 * series_out is given and/or reset != 0, the per-series snapshot of the same
 * range is taken from the same state (series_out: count l5dh_summary,
 * nullable) and the range is cleared -- so the rollup, the per-series
 * summaries and the reset all see exactly the same samples. */
int l5dh_rollup(l5dh_ctx* ctx, uint32_t first, uint32_t count, const uint32_t* group, uint32_t ngroups,
                l5dh_summary* g_out, int32_t* g_counts_out, int64_t* g_totals_out,
                l5dh_summary* series_out, int reset);

/* External dense rows: counts [n][1798] int32, totals [n] int64 (nullable: 0) --
 * the inputs of l5dh_summarize_dense, e.g. the slice a rank received from l5dh_merge. */
int l5dh_rollup_dense(l5dh_ctx* ctx, const int32_t* counts, const int64_t* totals, size_t n,
                      const uint32_t* group, uint32_t ngroups,
                      l5dh_summary* g_out, int32_t* g_counts_out, int64_t* g_totals_out);

/* Exact cumulative `le` buckets (Prometheus `<name>_bucket{le="..."}` counters): unlike
 * quantiles, they can be summed and divided outside the process (sum by (le),
 * histogram_quantile, "share of requests under 250 ms").  Bucket b of a row holds the
 * samples with L[b-1] <= (long)value < L[b] (L = l5dh_limits; bucket 0: (long)value < 1;
 * bucket 1797: the overflow).  A cut c in [1, 1797] stands for the first c buckets: the
 * count at the cut is counts[0] + ... + counts[c-1], carried in 64 bits, which is
 * exactly the number of samples with (long)value <= L[c-1] - 1 -- so the cut's label is
 * le = L[c-1] - 1, exact for the truncated value the histogram records.
 *
 * l5dh_le_cuts (host only, no context): each bound B is snapped DOWN to the largest such
 * le <= floor(B), so no reported bucket ever claims more than it holds:
 * cuts[i] = #{ j : L[j] - 1 <= floor(B) } clipped to [1, 1797], le[i] = L[cuts[i]-1] - 1
 * (cuts / le: each nullable).  Bounds 1, 2, 5, 10, 25, 50, 100 are exact (cuts 2, 3, 6,
 * 11, 26, 51, 101); 250 -> cut 193, le 250; 500 -> cut 262, le 497; 1000 -> cut 332,
 * le 997; +Inf and anything >= L[1796] - 1 give cut 1797.  NaN or B < 0 is -EINVAL
 * (nothing is written).  Nothing is deduplicated: bounds that snap to one cut yield
 * equal cuts, and the caller drops them (l5dh_le wants strictly ascending cuts). */
#define L5DH_LE_MAX 64 /* cuts per call */
int l5dh_le_cuts(const double* bounds, size_t n, uint32_t* cuts, int64_t* le);

/* Live state.  Under ONE hold of the context lock: staged samples are binned and
 * pending segments folded; per series i of [first, first+count) the counts at the
 * ncuts cuts and then the row's count (the `+Inf` bucket, always the last column) go to
 * le_out[i][0..ncuts] (uint64 [count][ncuts+1]) and the row's exact sum to sums_out[i]
 * (nullable); then, if series_out is given and/or reset != 0, the per-series snapshot
 * of the same range is taken from the same state (series_out: count l5dh_summary,
 * nullable) and the range is cleared -- the buckets, the summaries and the reset all
 * see exactly the same samples.
 * accumulate != 0 adds the results to what le_out / sums_out hold (sums_out wraps like
 * a Java long): a caller keeps lifetime counters across resetting intervals this way.
 * Every pointer may be host or device memory (cuts included); an accumulating host
 * output has its old values copied to the device first.
 * -EINVAL, with nothing written and nothing reset: ncuts outside [1, L5DH_LE_MAX], a cut
 * outside [1, 1797], cuts not strictly ascending, a bad range, a null cuts / le_out. */
int l5dh_le(l5dh_ctx* ctx, uint32_t first, uint32_t count, const uint32_t* cuts, uint32_t ncuts,
            uint64_t* le_out /* [count][ncuts+1] */, int64_t* sums_out /* [count], nullable */,
            int accumulate, l5dh_summary* series_out /* nullable */, int reset);

/* The same over external dense rows: counts [n][1798] int32, totals [n] int64 (nullable:
 * 0) -- the inputs and the domain of l5dh_summarize_dense (every count in [0, 2^31 - 1],
 * any row sum).  E.g. the g_counts of a rollup: cumulative buckets are linear, so these
 * are the members' summed buckets. */
int l5dh_le_dense(l5dh_ctx* ctx, const int32_t* counts, const int64_t* totals /* nullable */, size_t n,
                  const uint32_t* cuts, uint32_t ncuts, uint64_t* le_out, int64_t* sums_out, int accumulate);

/* Exact configurable quantiles: the inverse of the `le` buckets -- not "how many samples lie
 * at or below this value" but "which value is the q-quantile", for any q in [0, 1] (p25 and
 * p75 of a box plot, the p99.5 of an SLO, the p99.99 of a rollup group), without the dense
 * rows leaving the device.  Upstream BucketedHistogram.percentile(q): for a row with bucket
 * counts c[0..1797] and num = c[0] + ... + c[1797] (64 bits),
 *   target = Math.round(q * (double)num)      one FP64 product, JDK-8 Math.round
 *   target == 0 -> 0                          q = 0, an empty row, or q * num < 0.5
 *   else the midpoint of the first bucket whose running count >= target (the overflow
 *   bucket reports Int.MaxValue).
 * For q = 0.5, 0.9, 0.95, 0.99, 0.999, 0.9999 this is the summary's field; for q = 1 and a
 * non-empty row it is max; q = 0 gives 0, which is not min.  The order of the q is free and
 * duplicates are legal.
 *
 * l5dh_quantiles: live state.  Under ONE hold of the context lock: staged samples are binned
 * and pending segments folded; per series i of [first, first+count) the nq values go to
 * q_out[i][0..nq-1] (int64 [count][nq]); then, if series_out is given and/or reset != 0, the
 * per-series snapshot of the same range is taken from the same state (series_out: count
 * l5dh_summary, nullable) and the range is cleared -- the quantiles, the summaries and the
 * reset all see exactly the same samples.  Every pointer may be host or device memory (q
 * included).  count == 0 returns 0 and writes nothing.
 * -EINVAL, with nothing written and nothing reset: nq outside [1, L5DH_Q_MAX], a q that is
 * NaN, < 0 or > 1 (upstream's AssertionError; found on the host before anything is
 * enqueued), a bad range, a null q / q_out. */
#define L5DH_Q_MAX 64 /* quantiles per call */
int l5dh_quantiles(l5dh_ctx* ctx, uint32_t first, uint32_t count, const double* q, uint32_t nq,
                   int64_t* q_out /* [count][nq] */, l5dh_summary* series_out /* nullable */, int reset);

/* The same over external dense rows: counts [n][1798] int32 -- the inputs and the domain of
 * l5dh_summarize_dense (every count in [0, 2^31 - 1], any row sum).  E.g. the g_counts of a
 * rollup: the exact quantiles of the members' union. */
int l5dh_quantiles_dense(l5dh_ctx* ctx, const int32_t* counts, size_t n, const double* q, uint32_t nq,
                         int64_t* q_out /* [n][nq] */);

/* Exact top-k: WHICH series are the worst -- the k rows with the largest (or smallest) value
 * of one summary field, or of any quantile, selected where the numbers are: a full engine's
 * summaries never leave the device, k ids and k summaries do.
 *
 * Candidates: row i is a candidate iff its count >= min_count and (group == NULL or group[i]
 * == g).  Every other map value, L5DH_NO_GROUP included, means "not a member" -- nothing about
 * the map is an error, so the group map of a rollup can be passed as it is.  min_count = 0
 * admits empty rows (a live series of a clean tile has the all-zero summary).
 * Key: `by` names the field by its index in l5dh_summary; fields 0..9 compare as signed int64,
 * avg in the IEEE total order of its bits (-NaN < -Inf < ... < -0.0 < +0.0 < ... < +Inf < +NaN:
 * external garbage still has one answer).  L5DH_BY_QUANTILE (live state only) ranks by
 * BucketedHistogram.percentile(q) of the row, exactly what l5dh_quantiles returns for that q.
 * Order: by key descending (L5DH_TOP_LARGEST) or ascending (L5DH_TOP_SMALLEST); equal keys by
 * ascending id in both.  The id is first + i for the live call, the row index i for the
 * external one.  *n_out = min(k, number of candidates); ids_out[0 .. *n_out), top_out[0 ..
 * *n_out) (the winners' whole summaries) and q_out[0 .. *n_out) (their quantile values; by ==
 * L5DH_BY_QUANTILE only, ignored otherwise) are written and nothing beyond them.  The answer is
 * a pure function of the inputs: the same on every run, for host and for device pointers.
 *
 * l5dh_top: live state.  Under ONE hold of the context lock: staged samples are binned and
 * pending segments folded; for L5DH_BY_QUANTILE the quantile of every series of the range is
 * taken; the per-series snapshot of [first, first + count) is taken from the same state
 * (series_out: count l5dh_summary, nullable) and, with reset != 0, the range is cleared; the
 * selection then runs over those summaries or quantile values -- the ranking, series_out and
 * the reset all see exactly the same samples.
 * l5dh_top_summaries: external summaries values[n] (e.g. the g_out of a rollup: "the worst
 * routers").  Reads no engine state: it holds the context lock only to use its stream and
 * scratch.
 * Every pointer may be host or device memory.  count == 0 (n == 0) sets *n_out = 0.
 * -EINVAL, found on the host before anything is enqueued, with nothing written and nothing
 * reset: k outside [1, L5DH_TOP_LIMIT]; `by` outside the enum, or L5DH_BY_QUANTILE in
 * l5dh_top_summaries; order not 0 or 1; min_count < 0; q NaN or outside [0, 1] with
 * L5DH_BY_QUANTILE (q is ignored otherwise); a bad range; n > 2^24; a null ids_out or n_out;
 * a null values with n > 0. */
#define L5DH_TOP_LIMIT 1024 /* k per call */
enum {
  L5DH_BY_COUNT = 0,
  L5DH_BY_MIN = 1,
  L5DH_BY_MAX = 2,
  L5DH_BY_SUM = 3,
  L5DH_BY_P50 = 4,
  L5DH_BY_P90 = 5,
  L5DH_BY_P95 = 6,
  L5DH_BY_P99 = 7,
  L5DH_BY_P9990 = 8,
  L5DH_BY_P9999 = 9,
  L5DH_BY_AVG = 10,     /* = the field's index in l5dh_summary */
  L5DH_BY_QUANTILE = 11 /* live state only: percentile(q) */
};
enum { L5DH_TOP_LARGEST = 0, L5DH_TOP_SMALLEST = 1 };
int l5dh_top(l5dh_ctx* ctx, uint32_t first, uint32_t count, int by, double q, int order, int64_t min_count,
             const uint32_t* group /* [count], nullable */, uint32_t g, uint32_t k,
             uint32_t* ids_out /* [k] */, l5dh_summary* top_out /* [k], nullable */,
             int64_t* q_out /* [k], nullable; by == QUANTILE */, uint32_t* n_out,
             l5dh_summary* series_out /* [count], nullable */, int reset);
int l5dh_top_summaries(l5dh_ctx* ctx, const l5dh_summary* values, size_t n, int by, int order, int64_t min_count,
                       const uint32_t* group /* [n], nullable */, uint32_t g, uint32_t k,
                       uint32_t* ids_out, l5dh_summary* top_out /* nullable */, uint32_t* n_out);

/* State import and sparse export: the way INTO the bucket rows, and the CSR form of the way
 * out.  Rows that left an engine -- l5dh_export_state / l5dh_export_sparse output, the slice
 * of a merge, the g_counts of a rollup, the non-empty buckets of a peek -- enter another one:
 * a larger engine that takes over (growth), an aggregator above the process, a restart.
 *
 * An import makes every target series report exactly what it would report had it also
 * received the samples behind the imported row: counts[b] += row[b] for every bucket, the
 * exact sum += totals[i] (an int64 that wraps like a Java long), and everything downstream
 * (snapshot, peek, rollup, le, export, merge) sees the union.  Samples ingested before or
 * after the call -- those still in the staging ring or in pending segments included -- are
 * unaffected.  Domain: every imported count in [0, 2^31 - 1].  A bucket sum above 2^31 - 1 is
 * -ERANGE, found on the device and never wrapped, l5dh_last_error naming the least such
 * series.  A failing import leaves the observable state exactly as it was (l5dh_export_state
 * of the whole engine is byte-identical before and after), the call's valid rows included.
 * Every data pointer may be host or device memory.
 *
 * l5dh_import_state: counts [count][1798] int32 and totals [count] int64 (nullable: 0) -- what
 * l5dh_export_state writes -- into series [first, first+count).  -EINVAL: a range out of
 * bounds (found on the host), a negative count (found on the device; l5dh_last_error names
 * the least such series). */
typedef struct {
  uint32_t bucket; /* < 1798 */
  uint32_t count;  /* 1 .. 2^31 - 1 in an export; an imported 0 is legal and adds nothing */
} l5dh_bucket_entry; /* 8 B */
int l5dh_import_state(l5dh_ctx* ctx, uint32_t first, uint32_t count, const int32_t* counts, const int64_t* totals);

/* CSR of the non-empty buckets of series [first, first+count) (staged samples are binned and
 * pending segments folded first): row_off [count+1] with row_off[0] = 0, row i's entries at
 * entries[row_off[i] .. row_off[i+1]) in ascending bucket order, totals [count] (nullable) the
 * rows' exact sums.  *n_entries always receives the exact entry count (= row_off[count]).
 * entries == NULL is a size query: nothing else is written, nothing is reset.  cap <
 * *n_entries is -ERANGE: nothing else is written, nothing is reset.  reset as in
 * l5dh_export_state: the range is cleared afterwards, under the same hold of the lock. */
int l5dh_export_sparse(l5dh_ctx* ctx, uint32_t first, uint32_t count, uint64_t* row_off,
                       l5dh_bucket_entry* entries, size_t cap, size_t* n_entries, int64_t* totals, int reset);

/* n CSR rows (row_off [n+1], entries, totals [n] nullable: 0): row i goes to series[i]
 * (strictly ascending, each < max_series); series == NULL: to first + i.  The rows are checked
 * on the device before any state is touched; each of these is -EINVAL, l5dh_last_error naming
 * the least offending row: row_off not ascending from 0; an entry with bucket >= 1798; buckets
 * not strictly ascending within a row; a count above 2^31 - 1; series not strictly ascending,
 * or >= max_series.  first + n > max_series (series == NULL) is -EINVAL, found on the host. */
int l5dh_import_sparse(l5dh_ctx* ctx, const uint32_t* series, uint32_t first, size_t n, const uint64_t* row_off,
                       const l5dh_bucket_entry* entries, const int64_t* totals);

/* Sliding windows: exact summaries over the last W ended intervals ("p99 over the last five
 * minutes").  A window is a ring of at most L5DH_WINDOW_MAX slots that belongs to a context;
 * a slot holds, in device memory, the sparse rows (the CSR of l5dh_export_sparse) and exact
 * totals of one ended interval.  The histogram of a union of intervals is the element-wise
 * integer sum of their bucket rows, so a series' window summary is byte for byte what ONE
 * Stat would report had it received every sample the series received in those intervals.
 * Every data pointer may be host or device memory; every call holds the context's lock.
 *
 * l5dh_window_open: slots in [1, L5DH_WINDOW_MAX], else -EINVAL; -EEXIST if the context
 * already has a window.  l5dh_window_close frees the ring (-EINVAL without one); l5dh_close
 * frees it too.
 *
 * l5dh_window_push ends the interval of series [0, count): l5dh_export_sparse(0, count, ...,
 * reset = 1) with the ring's next slot as destination, under one hold of the lock, and
 * series_out (nullable: count l5dh_summary) the interval's summaries from the same state, as
 * l5dh_snapshot(0, count, ..., reset = 1) would report them.  The oldest slot is overwritten
 * once the ring is full.  A slot remembers its count: a series at or beyond it has an empty
 * row in that slot.  Pushes are numbered from 1.  When an allocation fails the call returns
 * -ENOMEM, resets nothing and leaves the ring as it was.
 *
 * l5dh_window_query sums, per series of [first, first + count), the rows of the `last` most
 * recent slots and, with include_open != 0, the open interval's live row (staged samples are
 * binned and pending segments folded first, as in l5dh_le; the open interval is not changed).
 * Per series the outputs (each nullable) receive: out the summary, counts_out [count][1798]
 * the summed dense row, totals_out the summed exact sum (an int64 that wraps like a Java
 * long) -- what every other row source returns, so they feed l5dh_top_summaries,
 * l5dh_render_summaries, l5dh_quantiles_dense, l5dh_le_dense and l5dh_rollup_dense
 * unchanged.  last == 0 with include_open equals l5dh_snapshot(first, count, ..., reset = 0)
 * byte for byte.  -EINVAL, found on the host before anything is enqueued: no window, a range
 * out of bounds, last above the number of filled slots, last == 0 without include_open.  A
 * bucket sum above 2^31 - 1 is -ERANGE, found on the device and never wrapped (also when
 * the sum passes 2^32), l5dh_last_error naming the least such series; ring and state are
 * untouched and the outputs unspecified.
 *
 * l5dh_window_forget makes series [first, first + count) start their history now: a query
 * ignores, for those series, every slot pushed so far (a pruned id's past stays out of the
 * next Stat that gets the id).  The open interval is not touched.
 *
 * l5dh_window_move hands the whole ring of `from` to `to`, a context on the same device
 * that has none (-EEXIST) and holds at least as many series as the largest slot count
 * (-EINVAL): pointers move, nothing is copied but the per-series forget marks, extended with
 * zeros to `to`'s series count.  The two locks are taken in address order.
 *
 * l5dh_window_info (every pointer nullable): the ring's slots, the filled ones, the pushes so
 * far, the entries (8 B each) the filled slots hold, and the device bytes the ring owns. */
#define L5DH_WINDOW_MAX 64
int l5dh_window_open(l5dh_ctx* ctx, uint32_t slots);
int l5dh_window_close(l5dh_ctx* ctx);
int l5dh_window_push(l5dh_ctx* ctx, uint32_t count, l5dh_summary* series_out /* [count], nullable */);
int l5dh_window_query(l5dh_ctx* ctx, uint32_t first, uint32_t count, uint32_t last, int include_open,
                      l5dh_summary* out, int32_t* counts_out, int64_t* totals_out);
int l5dh_window_forget(l5dh_ctx* ctx, uint32_t first, uint32_t count);
int l5dh_window_move(l5dh_ctx* from, l5dh_ctx* to);
int l5dh_window_info(l5dh_ctx* ctx, uint32_t* slots, uint32_t* filled, uint64_t* pushes, uint64_t* entries,
                     uint64_t* bytes);

/* Counters on the device: Metric.Counter (Metric.scala:14-20, an AtomicLong behind
 * incr(delta: Int)), batched.  A context may own a counter space: int64 values
 * [max_counters] in device memory, all zero when opened; nothing is allocated before.  Every
 * sum is a two's-complement sum that wraps like a Java long, so the order of adds never
 * shows.  Every data pointer may be host or device memory (at any 4-byte alignment for ids,
 * deltas and the group map, 8-byte for the values); every call holds the context's lock.
 * Arguments are checked on the host before anything is enqueued, and a failing call changes
 * nothing: -EINVAL for a null context, a context without counters, a range outside the
 * space, max_counters outside [1, L5DH_MAX_COUNTERS], ngroups outside [1,
 * L5DH_MAX_COUNTERS], n above 2^30.
 *
 * l5dh_counters_open: -EEXIST if the context already has counters.  l5dh_counters_close
 * frees the space; l5dh_close frees it too.  l5dh_counters_resize grows only (a smaller size
 * is -EINVAL): the values are kept and the new ones are 0.
 *
 * l5dh_counters_add: values[ids[i]] += deltas[i] for i < n (deltas == NULL: 1 each).  It
 * follows l5dh_ingest's contract: it returns once the batch is queued, host buffers are free
 * again when it returns, device buffers are stream ordered on a caller stream
 * (l5dh_set_stream) and free when it returns otherwise.  An id >= max_counters is dropped --
 * never applied, never an address -- and counted: the next l5dh_sync returns -EINVAL (once)
 * for them, and l5dh_counters_info's *dropped holds their number.  Every valid add is
 * applied.
 *
 * l5dh_counters_read / l5dh_counters_write: values [first, first + count) to out / from
 * values (NULL: zeros), ordered with the adds queued before.  count == 0 does nothing.
 *
 * l5dh_counters_rollup: label rollups of counters ("requests per router"): g_out[g] for g <
 * ngroups receives the wrapping sum of the counters first + i, i < count, with group[i] == g
 * -- l5dh_rollup's map: a value < ngroups or L5DH_NO_GROUP.  Any other value is -EINVAL,
 * found on the device and reported by this call, l5dh_last_error naming the least such index;
 * that entry counts as no group.  A group without members gives 0; count == 0 still writes
 * ngroups zeros.
 *
 * l5dh_counters_values: the live array, for a renderer on the same context and stream
 * (l5dh_render_json, l5dh_render_scalars, l5dh_render_influx take it as `counters`), so a
 * scrape copies nothing.  Valid until the next resize, move or close.
 *
 * l5dh_counters_move hands the space of `from` to `to`, a context on the same device that
 * has none (-EEXIST): the pointer moves, nothing is copied.  The two locks are taken in
 * address order.
 *
 * l5dh_counters_info (every pointer nullable): the space's size and what the add kernels
 * counted since it was opened: *adds the adds applied, of which *lds_adds went through a
 * workgroup's LDS claim table and *global_adds took a global atomic of their own (*adds ==
 * *lds_adds + *global_adds), and *dropped the invalid ids. */
#define L5DH_MAX_COUNTERS (1u << 24)
int l5dh_counters_open(l5dh_ctx* ctx, uint32_t max_counters);
int l5dh_counters_close(l5dh_ctx* ctx);
int l5dh_counters_resize(l5dh_ctx* ctx, uint32_t max_counters);
int l5dh_counters_add(l5dh_ctx* ctx, const uint32_t* ids, const int32_t* deltas /* nullable: 1 */, size_t n);
int l5dh_counters_read(l5dh_ctx* ctx, uint32_t first, uint32_t count, int64_t* out);
int l5dh_counters_write(l5dh_ctx* ctx, uint32_t first, uint32_t count, const int64_t* values /* nullable: 0 */);
int l5dh_counters_rollup(l5dh_ctx* ctx, uint32_t first, uint32_t count, const uint32_t* group, uint32_t ngroups,
                         int64_t* g_out);
int l5dh_counters_values(l5dh_ctx* ctx, const int64_t** device_ptr, uint32_t* max_counters);
int l5dh_counters_move(l5dh_ctx* from, l5dh_ctx* to);
int l5dh_counters_info(l5dh_ctx* ctx, uint32_t* max_counters, uint64_t* adds, uint64_t* lds_adds,
                       uint64_t* global_adds, uint64_t* dropped);

/* Java number texts, as the exporters print them (host only, no context): Long.toString,
 * the unsigned 64-bit decimal (the `le` counts) and Double.toString as JDK 8 prints it
 * (FloatingDecimal: not the shortest round-trip form of later JDKs; 2.82879384806159e17
 * prints as 2.82879384806159008E17).  out receives *len characters, no terminator.
 * l5dh_format_double handles +-0.0, NaN, +-Infinity and finite 2^-64 <= |x| < 2^64 --
 * everything sum / count of two int64 can be; any other value is -ERANGE (*len = 0): it
 * is never printed wrongly.  A null out or len is -EINVAL.
 * l5dh_format_float is Float.toString of JDK 8 (the same digit loop with the float's 24
 * significant bits, fewer for a subnormal) and handles every float: the formatter's
 * 192-bit integer covers the whole float range.  It keeps the contract all the same: a
 * value it could not print exactly would be -ERANGE (*len = 0), never a wrong text. */
#define L5DH_DOUBLE_CHARS 26
#define L5DH_FLOAT_CHARS 16
#define L5DH_LONG_CHARS 20
int l5dh_format_double(double x, char* out /* >= L5DH_DOUBLE_CHARS */, size_t* len);
int l5dh_format_float(float x, char* out /* >= L5DH_FLOAT_CHARS */, size_t* len);
int l5dh_format_long(int64_t v, char* out /* >= L5DH_LONG_CHARS */, size_t* len);
int l5dh_format_ulong(uint64_t v, char* out /* >= L5DH_LONG_CHARS */, size_t* len);

/* The Prometheus exposition of Stats, rendered on the device: the text is produced where
 * the numbers are, and one buffer goes to whoever answers the scrape.  A name table holds
 * what does not vary per scrape, fixed when a Stat is registered: row j < n prints element
 * index[j] (index == NULL: j) of the value arrays under the escaped metric key
 * key_bytes[key_off[j] .. key_off[j+1]) and the already-escaped text between the braces
 * lab_bytes[lab_off[j] .. lab_off[j+1]) -- `a="b", c="d"`, possibly empty.  key_off and
 * lab_off hold n + 1 ascending entries.  With lab = "" for an empty inner text, else
 * `{inner}`, and an extra label appended as `{inner, quantile="0.5"}` (`{quantile="0.5"}`
 * for an empty inner text), every line is `name[lab] value\n`.
 *
 * l5dh_render_summaries prints per row, from values[index[j]] (nvalues elements):
 *   key_count lab N / key_sum lab N / key_avg lab D, then eight lines key{.. quantile="q"} N
 *   for q = 0, 0.5, 0.9, 0.95, 0.99, 0.999, 0.9999, 1 (min, p50, p90, p95, p99, p9990,
 *   p9999, max) -- N as l5dh_format_long, D as l5dh_format_double.
 * l5dh_render_le prints per row, from le_rows[index[j]][0..ncuts] (what l5dh_le wrote) and
 * sums[index[j]] (sums == NULL: 0), with the ncuts labels le[k]:
 *   ncuts lines key_hist_bucket{.. le="<le[k]>"} n, one with le="+Inf" carrying the last
 *   column, key_hist_sum lab s, key_hist_count lab <the last column> -- n as
 *   l5dh_format_ulong.
 * l5dh_render_quantiles prints per row, from q_rows[index[j]][0..nq-1] (what l5dh_quantiles
 * wrote; int64 [nvalues][nq]):
 *   nq lines key{.. quantile="<l5dh_format_double(q[k])>"} N -- 0.75, 0.995, 1.0E-4 -- N as
 *   l5dh_format_long.  The labels are formatted once per call on the host; q is checked as
 *   l5dh_quantiles checks it (-EINVAL), and a q outside l5dh_format_double's domain (a
 *   positive q below 2^-64) is -ERANGE, both before anything is enqueued.
 *
 * Every data pointer (the five arrays of the table included) may be host or device
 * memory.  *len always receives the exact length of the text.  out == NULL is a size
 * query (returns 0); out != NULL with cap < *len is -ERANGE and nothing is written;
 * n == 0 writes nothing, sets *len = 0 and returns 0.  -EINVAL: ncuts outside
 * [1, L5DH_LE_MAX], nq outside [1, L5DH_Q_MAX], a null names, key_off, lab_off, le or q,
 * nvalues == 0 (or null values) with n > 0.  Found on the device and reported by the call, l5dh_last_error naming the
 * first such row, the output then unspecified: index[j] >= nvalues, offsets that descend,
 * a row whose key and label text exceed 2^25 bytes (-EINVAL); an avg outside
 * l5dh_format_double's domain (-ERANGE).  The calls read no engine state: they hold the
 * context lock only to use its stream and scratch, and return once out is written. */
typedef struct {
  const uint32_t* index;     /* [n], nullable: row j prints element j */
  const uint64_t* key_off;   /* [n + 1] */
  const uint8_t* key_bytes;
  const uint64_t* lab_off;   /* [n + 1] */
  const uint8_t* lab_bytes;
} l5dh_names;
int l5dh_render_summaries(l5dh_ctx* ctx, const l5dh_names* names, size_t n, const l5dh_summary* values,
                          size_t nvalues, uint8_t* out, size_t cap, size_t* len);
int l5dh_render_le(l5dh_ctx* ctx, const l5dh_names* names, size_t n, const uint64_t* le_rows,
                   const int64_t* sums /* nullable: 0 */, size_t nvalues, const int64_t* le, uint32_t ncuts,
                   uint8_t* out, size_t cap, size_t* len);
int l5dh_render_quantiles(l5dh_ctx* ctx, const l5dh_names* names, size_t n, const int64_t* q_rows /* [nvalues][nq] */,
                          size_t nvalues, const double* q, uint32_t nq, uint8_t* out, size_t cap, size_t* len);

/* A whole scrape on the device: the flat compact /admin/metrics.json document and the
 * counter and gauge lines of the Prometheus exposition.  A row has a kind, kinds[j], and
 * each kind its own value array; index[j] (index == NULL: j) counts within the row's kind:
 *   L5DH_KIND_COUNTER  counters[index[j]]   int64, printed as l5dh_format_long
 *   L5DH_KIND_GAUGE    gauges[index[j]]     float, printed as l5dh_format_float
 *   L5DH_KIND_STAT     summaries[index[j]]  l5dh_render_json only
 *
 * l5dh_render_json writes one JSON object, byte for byte what jackson writes for
 * AdminMetricsExportTelemeter's flat compact form: `{`, per row its entries
 * `"<key><sfx>":<number>` separated by `,`, `}`.  key is the name already escaped as
 * JsonGenerator.writeFieldName escapes it (UTF-8, without the quotes).  There is no label
 * text: names->lab_off and names->lab_bytes are not read and may be NULL.  A counter and a
 * gauge have one entry (sfx empty); a non-finite gauge is quoted ("NaN", "Infinity",
 * "-Infinity").  A stat always has `.count`, and only when count > 0 also .max .min .p50
 * .p90 .p95 .p99 .p9990 .p9999 .sum (longs) and .avg (l5dh_format_double, quoted when
 * non-finite), in that order.  Without any entry (n == 0) the document is `{}`.
 * l5dh_render_scalars writes one line `key[{inner}] <value>\n` per row, the line grammar of
 * the calls above; a gauge is never quoted here.  n == 0 writes nothing.
 *
 * The contract is that of the render calls above: host or device memory for every data
 * pointer, *len the exact length, out == NULL a size query, cap < *len -ERANGE with nothing
 * written, no engine state read.  A value array may be NULL only with a count of 0; a
 * non-null count with a null array, a null names, key_off or kinds (n > 0) and, for
 * l5dh_render_scalars, a null lab_off are -EINVAL.  Found on the device, l5dh_last_error
 * naming the first such row: a kind that is none of the above, or L5DH_KIND_STAT in
 * l5dh_render_scalars (-EINVAL); index[j] >= the count of the row's kind, which a row of a
 * kind without values always is (-EINVAL); offsets that descend, a key above 2^25 bytes
 * (-EINVAL); an avg outside l5dh_format_double's domain (-ERANGE). */
#define L5DH_KIND_COUNTER 0
#define L5DH_KIND_GAUGE 1
#define L5DH_KIND_STAT 2
int l5dh_render_json(l5dh_ctx* ctx, const l5dh_names* names, const uint8_t* kinds /* [n] */, size_t n,
                     const l5dh_summary* summaries, size_t nsummaries, const int64_t* counters, size_t ncounters,
                     const float* gauges, size_t ngauges, uint8_t* out, size_t cap, size_t* len);
int l5dh_render_scalars(l5dh_ctx* ctx, const l5dh_names* names, const uint8_t* kinds /* [n] */, size_t n,
                        const int64_t* counters, size_t ncounters, const float* gauges, size_t ngauges, uint8_t* out,
                        size_t cap, size_t* len);

/* The InfluxDB line protocol body (/admin/metrics/influxdb) on the device.  A line is a
 * measurement head followed by the fields of every metric under one parent, sorted
 * together by key, so the rows of this table are FIELDS in the order they are printed,
 * beside a small table of lines.  Row j < n belongs to line l = line[j] (non-decreasing,
 * < nlines) and prints
 *   ( first row of its line ? head[l] host tail[l] : `,` )  key  `=`  value  ( last row ? `\n` : nothing )
 * where a row is first when j == 0 or line[j-1] != l, and last when j == n-1 or
 * line[j+1] != l; a line id without rows prints nothing.  head[l] is
 * head_bytes[head_off[l] .. head_off[l+1]), the text up to and including `host=`;
 * host the request's Host value, host_len bytes (0: none); tail[l] the text after it up
 * to and including the space; key the whole field key, suffix included
 * (`request_latency_ms_p999`).  The value is the element index[j] of the array of the
 * row's kind, kinds[j]:
 *   L5DH_KIND_COUNTER  counters[index[j]]   as l5dh_format_long
 *   L5DH_KIND_GAUGE    gauges[index[j]]     as l5dh_format_float, never quoted
 *   L5DH_KIND_STAT     field field[j] (0 .. 10: count, min, max, sum, p50, p90, p95, p99,
 *                      p9990, p9999, avg -- the L5DH_BY_ numbering) of summaries[index[j]]:
 *                      a long, or avg as l5dh_format_double; printed whatever the count is
 * The text is byte for byte what InfluxDbTelemeter writes when the table is built as
 * linkerd_amd/render_influx.py builds it.
 *
 * The contract is that of l5dh_render_json: host or device memory for every data pointer,
 * host included; *len the exact length; out == NULL a size query; cap < *len -ERANGE with
 * nothing written; n == 0 writes nothing and sets *len = 0; no engine state read.
 * -EINVAL before anything is enqueued: a null names or, with n > 0, a null array of it; a
 * null host with host_len > 0; host_len > 65535; a non-null count with a null value
 * array; n or nlines above 2^32 - 16.  Found on the device, l5dh_last_error naming the
 * least such row and the output then unspecified: a kind that is none of the three;
 * field[j] > 10 on a stat row; index[j] >= the count of the row's kind; line[j] >= nlines
 * or line[j] < line[j-1]; key_off descending at the row, head_off or tail_off descending at
 * its line; pieces (head, host, tail and key) above 2^25 bytes (all -EINVAL); an avg
 * outside l5dh_format_double's domain (-ERANGE). */
typedef struct {
  const uint32_t* line;      /* [n] */
  const uint8_t* kinds;      /* [n] */
  const uint8_t* field;      /* [n] */
  const uint32_t* index;     /* [n] */
  const uint64_t* key_off;   /* [n + 1] */
  const uint8_t* key_bytes;
  const uint64_t* head_off;  /* [nlines + 1] */
  const uint8_t* head_bytes;
  const uint64_t* tail_off;  /* [nlines + 1] */
  const uint8_t* tail_bytes;
} l5dh_influx_names;
int l5dh_render_influx(l5dh_ctx* ctx, const l5dh_influx_names* names, size_t n, size_t nlines, const uint8_t* host,
                       size_t host_len, const l5dh_summary* summaries, size_t nsummaries, const int64_t* counters,
                       size_t ncounters, const float* gauges, size_t ngauges, uint8_t* out, size_t cap, size_t* len);

/* Fleet merge over RCCL (xGMI): sample-sharded series (config C4) summed across
 * contexts on different GPUs.  One communicator per context, one rank per GPU:
 *  - multi-process (or one thread per context): rank 0 calls l5dh_comm_unique_id,
 *    the caller distributes the L5DH_UNIQUE_ID_BYTES bytes, every rank calls
 *    l5dh_comm_init_rank (collective: all ranks must call it);
 *  - one process holding several GPUs (e.g. a JVM): l5dh_comm_init_all over its
 *    contexts (distinct devices; rank i = ctxs[i]).
 * Every context of a communicator has the same max_series. */
int l5dh_comm_unique_id(void* id_out /* L5DH_UNIQUE_ID_BYTES */);
int l5dh_comm_init_rank(l5dh_ctx* ctx, const void* id, int nranks, int rank);
int l5dh_comm_init_all(l5dh_ctx** ctxs, int n);
/* Test transport: n contexts on ONE device form an n-rank group whose collectives are
 * device copies and reductions among their buffers (no RCCL), so the multi-rank merge
 * code -- per-destination slices, the size all-gather, the payload exchange, the
 * in-place local slice, the decode -- runs on a single GPU.  Such a group merges
 * through l5dh_merge_all only.  At most 64 ranks for every communicator kind
 * (the sparse reduce-scatter's sources): larger groups are rejected here, before
 * any merge consumes an interval. */
int l5dh_comm_init_loopback(l5dh_ctx** ctxs, int n);
int l5dh_comm_destroy(l5dh_ctx* ctx);

/* Reference: the snapshot of a series whose samples arrived on several hosts
 * must see their merged counts (AdminMetricsExportTelemeter.scala:154-162,
 * Metric.scala:39-67).  Collective (every rank of the communicator calls it):
 * each rank's pending samples and state are exported (whole range, reset), the
 * int32 counts [S][1798] and int64 totals [S] are summed with one RCCL
 * reduce-scatter (or all-reduce), and the rank summarizes the rows it received:
 * series [*first, *first + *count) (reduce-scatter: slice r of ceil(S/nranks)
 * rows; all-reduce: all S).  The reduce-scatter moves the rows sparse: each rank
 * sends each other rank the non-empty buckets of that rank's slice (one u32 per
 * bucket: bucket << 21 | count; larger counts take a second word) and the words per
 * row, and the totals go by one int64 reduce-scatter (l5dh_merge_bytes); the
 * all-reduce moves them dense.  out (nullable) receives *count l5dh_summary,
 * counts_out / totals_out (nullable) the summed rows.  Each output must hold
 * ceil(S/nranks) rows (reduce-scatter) or S rows (all-reduce).  Integer sums:
 * bit-exact and independent of the reduction order.  Unlike a rollup, the merge adds
 * the ranks' bucket counts in 32 bits and checks no range: a merged bucket above
 * 2^32 - 1 wraps silently (above 2^31 - 1 it no longer fits the int32 counts_out).
 * The merged row's count is exact for the buckets as merged.  The export consumes the
 * rank's interval (as a resetting snapshot does) before the collective runs: if
 * the collective then fails (-EIO, l5dh_last_error), that interval is lost -- the
 * same outcome as a snapshot whose outputs are discarded. */
int l5dh_merge(l5dh_ctx* ctx, int mode, l5dh_summary* out, int32_t* counts_out, int64_t* totals_out,
               uint32_t* first, uint32_t* count);
/* The same for all contexts of an l5dh_comm_init_all communicator, from one
 * thread (the collectives are grouped).  Arrays are indexed like ctxs; any of
 * the output arrays (or their entries) may be NULL. */
int l5dh_merge_all(l5dh_ctx** ctxs, int n, int mode, l5dh_summary** outs, int32_t** counts_outs,
                   int64_t** totals_outs, uint32_t* firsts, uint32_t* counts);

/* Records per 32-series tile of the last binned ingest batch (out: >= ceil(max_series
 * / 32) entries; staged samples are binned first).  The load a series-sharded fleet
 * plans its next ranges from (linkerd_amd/fleet.py plan_shards). */
int l5dh_tile_totals(l5dh_ctx* ctx, uint64_t* out, size_t n);

/* Partition passes redone since l5dh_open because a capacity-planned region overflowed
 * (any pointer nullable): *level1 / *level2 = redos of the level-1 / level-2 partition
 * (each costs about one more pass of that level; results are exact either way).
 * *level2_counted = batches whose level-2 regions were known not to fit after level 1
 * (a moved load, a first interval): their first level-2 pass only counted the keys
 * (about 0.4 of a pass) and the second wrote exact regions -- not counted as redos. */
int l5dh_partition_redos(l5dh_ctx* ctx, uint64_t* level1, uint64_t* level2, uint64_t* level2_counted);

/* Bytes of the last l5dh_merge / l5dh_merge_all on this context (any pointer nullable):
 * *dense = the dense rows + totals a reduce-scatter would move ([S][1798] int32 +
 * [S] int64), *encoded = this rank's sparse encoding of them (non-empty buckets,
 * words per row, totals), *sent = what it sent to the other ranks. */
int l5dh_merge_bytes(l5dh_ctx* ctx, uint64_t* dense, uint64_t* encoded, uint64_t* sent);

/* Bin staged samples, wait for queued work; returns -EINVAL (once) if the device
 * found invalid series ids in any batch ingested since the last such report. */
int l5dh_sync(l5dh_ctx* ctx);
/* Run the context's work on an external hipStream_t, e.g. the caller's current
 * stream (torch's), so the context's kernels are ordered with the caller's work
 * on it; NULL selects the device's legacy default (null) stream.
 * L5DH_OWN_STREAM restores the context's own stream (the default). */
#define L5DH_OWN_STREAM ((void*)(intptr_t)-1)
int l5dh_set_stream(l5dh_ctx* ctx, void* hip_stream);
/* Order the context's next work after a caller's hipEvent_t (recorded on whatever
 * stream produced the device inputs, e.g. a torch.cuda.Event): the context's
 * stream waits for it on the device, the host does not. */
int l5dh_wait_event(l5dh_ctx* ctx, void* hip_event);
int l5dh_set_param(l5dh_ctx* ctx, int param, int64_t value);
/* Accumulated device time (ms) and launch count of one kernel id since the
 * last reset (requires L5DH_PARAM_TIMING=1). reset_after != 0 zeroes it. */
int l5dh_kernel_time(l5dh_ctx* ctx, int kernel_id, double* ms, int64_t* launches, int reset_after);
int l5dh_device(l5dh_ctx* ctx, int* hip_device);
uint32_t l5dh_max_series(l5dh_ctx* ctx);

/* Pinned host staging for the JNI side's per-thread DirectByteBuffers. */
int l5dh_pin_alloc(size_t bytes, void** out);
int l5dh_pin_free(void* p);

const char* l5dh_last_error(l5dh_ctx* ctx);
int l5dh_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
