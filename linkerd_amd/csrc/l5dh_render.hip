// l5dh_render.hip -- the text of a scrape, produced where the numbers are.
//
// A row's block is a list of lines, each
//     open key sfx [ `{` inner [`, `] ext ev `"` `}` ] sep number end
// with key / inner the row's name bytes, sfx / ext / ev small constant texts (or, for ev,
// an `le` label or a quantile's label) and number a Java long, an unsigned 64-bit decimal or
// a text formatted once per row (the avg's Double.toString, a gauge's Float.toString).
// open, sep and end are the block's grammar: nothing, a space and a newline for the
// Prometheus lines that prometheus.py's write_metrics, write_rollup_metrics,
// write_histogram_metrics, write_quantile_metrics and write_scalar_metrics print; `"`,
// `":` and `,` for the entries of admin_metrics.py's write_flat_json.  The number of
// lines is the row's: a JSON stat row has one entry, or eleven when its count is above 0.
//
//   k_rd_len    a lane per row: checks the row (kind, index, offsets, name length), formats
//               its avg or gauge once into the row's slot, and adds up the lines' lengths from
//               the name lengths and the digit counts.
//   (scan)      the fleet merge's exclusive u32 -> u64 scan (merge_count).
//   k_rd_write  a wave per row (one-wave workgroups striding over the rows).  Lane t lays
//               out line t: a wave scan of the line lengths gives its place, and the lane
//               writes the line's own small pieces (sfx, braces, ext, numbers).  The wave
//               then copies key and inner into every line together (their first 64 bytes
//               from registers).  A row of at most TEXT_STAGE bytes is built in LDS at the
//               destination's offset within 16 bytes and leaves through stage_flush; a
//               longer row is built by the same code straight in the output.  Only row j's
//               wave writes row j's bytes.
//
// The slot, the stage's way out, `put`, the kinds and the write pass's sizes are
// l5dh_textout.hpp's, shared with l5dh_influx.hip.  A Rows struct of l5dh_render.hpp has
// its Block here (block_of); render_lengths and render_write are one template each,
// instantiated below for the five Rows.
#include "l5dh_device.hpp"
#include "l5dh_textout.hpp"

namespace l5dh {
namespace {

constexpr uint32_t RD_LINES_MAX = LE_MAX + 3;     // K buckets, +Inf, _sum, _count
static_assert(Q_MAX <= RD_LINES_MAX && 11u <= RD_LINES_MAX, "a block's lines have their places in LDS");

enum { NUM_LONG = 0, NUM_ULONG = 1, NUM_TEXT = 2 };

struct Line {
  const char* sfx;      // after the key
  uint32_t sfx_n;
  const char* ext;      // the extra label up to its value's opening quote (ext_n == 0: none)
  uint32_t ext_n;
  const char* ev;       // the extra label's value, or null: the long ev_num
  uint32_t ev_n;
  int64_t ev_num;
  uint32_t kind;        // NUM_*
  uint64_t v;           // NUM_LONG (its bits) / NUM_ULONG
  const uint8_t* text;  // NUM_TEXT
  uint32_t text_n;
};

__device__ __forceinline__ uint32_t num_len(const Line& L) {
  return L.kind == NUM_TEXT ? L.text_n : (uint32_t)(L.kind == NUM_LONG ? fmt::long_digits((int64_t)L.v) : fmt::ulong_digits(L.v));
}
__device__ __forceinline__ uint32_t ev_len(const Line& L) { return L.ev ? L.ev_n : (uint32_t)fmt::long_digits(L.ev_num); }

// A block's grammar: what precedes the key (open_n bytes: none or one), what stands between
// the name part and the number (sep_n bytes: one or two), what ends the line, and whether
// a row has label text at all (false: lab_off and lab_bytes are never read).
struct PromGrammar {
  static constexpr bool labels = true;
  static constexpr uint32_t open_n = 0u, sep_n = 1u;
  static constexpr uint8_t open = 0, sep0 = ' ', sep1 = 0, end = '\n';
};
struct JsonGrammar {
  static constexpr bool labels = false;
  static constexpr uint32_t open_n = 1u, sep_n = 2u;
  static constexpr uint8_t open = '"', sep0 = '"', sep1 = ':', end = ',';
};

// Bytes of the line up to its inner text (open, key, sfx, `{`) and in all.
template <class G>
__device__ __forceinline__ uint32_t line_head(uint32_t klen, uint32_t ilen, const Line& L) {
  return G::open_n + klen + L.sfx_n + ((ilen || L.ext_n) ? 1u : 0u);
}
template <class G>
__device__ __forceinline__ uint32_t line_len(uint32_t klen, uint32_t ilen, const Line& L) {
  uint32_t n = line_head<G>(klen, ilen, L) + ilen;
  if (L.ext_n) n += (ilen ? 2u : 0u) + L.ext_n + ev_len(L) + 1u;  // [`, `] ext ev `"`
  if (ilen || L.ext_n) n += 1u;                                    // `}`
  return n + G::sep_n + num_len(L) + 1u;                           // sep number end
}

// The lane's own pieces of its line at dst + pos: everything but key and inner.  Writes
// inside [pos, pos + line_len) only, and ends exactly there.
template <class G>
__device__ __forceinline__ void line_write(uint8_t* dst, uint32_t pos, uint32_t klen, uint32_t ilen, const Line& L) {
  if (G::open_n) dst[pos] = G::open;
  uint32_t p = put(dst, pos + G::open_n + klen, L.sfx, L.sfx_n);
  if (ilen || L.ext_n) dst[p++] = '{';
  p += ilen;
  if (L.ext_n) {
    if (ilen) {
      dst[p++] = ',';
      dst[p++] = ' ';
    }
    p = put(dst, p, L.ext, L.ext_n);
    if (L.ev)
      p = put(dst, p, L.ev, L.ev_n);
    else
      p += (uint32_t)fmt::format_long(L.ev_num, dst + p);
    dst[p++] = '"';
  }
  if (ilen || L.ext_n) dst[p++] = '}';
  dst[p++] = G::sep0;
  if (G::sep_n > 1u) dst[p++] = G::sep1;
  if (L.kind == NUM_TEXT)
    p = put(dst, p, L.text, L.text_n);
  else if (L.kind == NUM_LONG)
    p += (uint32_t)fmt::format_long((int64_t)L.v, dst + p);
  else
    p += (uint32_t)fmt::format_ulong(L.v, dst + p);
  dst[p] = G::end;
}

// ---- the blocks ---------------------------------------------------------------------
// A block has its grammar G and K_MAX (its rows' K lies in [1, K_MAX]; 0: they have none);
// kind_ok(j): row j is of a kind the call prints;
// values(j, nvalues): the number of values the row indexes; prepare(j, idx): the length pass's own work for
// the row (false: out of the formatter's domain); nlines(j, idx) and line(j, idx, t, L).
// Summary: _count, _sum, _avg, then QUANTILES' eight lines (min, p50, .., p9999, max).
struct SummaryBlock {
  using G = PromGrammar;
  static constexpr uint32_t K_MAX = 0u;
  SummaryRows r;
  __device__ __forceinline__ bool kind_ok(uint32_t) const { return true; }
  __device__ __forceinline__ uint32_t values(uint32_t, uint32_t nvalues) const { return nvalues; }
  __device__ __forceinline__ uint32_t nlines(uint32_t, uint32_t) const { return 11u; }
  // The avg's text.
  __device__ __forceinline__ bool prepare(uint32_t j, uint32_t idx) const {
    return slot_write(r.avg + (size_t)j * RENDER_AVG_SLOT, r.v[idx].avg) >= 0;
  }
  __device__ __forceinline__ void line(uint32_t j, uint32_t idx, uint32_t t, Line& L) const {
    // Summary88's words: count, min, max, sum, p50, p90, p95, p99, p9990, p9999
    const uint32_t field = t == 0 ? 0u : (t == 1 ? 3u : (t == 3 ? 1u : (t == 10 ? 2u : t)));
    L.sfx = t == 0 ? "_count" : (t == 1 ? "_sum" : "_avg");
    L.sfx_n = t == 0 ? 6u : (t < 3 ? 4u : 0u);
    L.ext = "quantile=\"";
    L.ext_n = t < 3 ? 0u : 10u;
    const char* q = "0      0.5    0.9    0.95   0.99   0.999  0.9999 1";  // 7 bytes apart
    const uint32_t qi = t < 3 ? 0u : t - 3u;
    L.ev = q + 7u * qi;
    L.ev_n = (0x16544331u >> (4u * qi)) & 15u;  // their lengths: 1 3 3 4 4 5 6 1
    L.ev_num = 0;
    const SlotText avg = slot_read(r.avg + (size_t)j * RENDER_AVG_SLOT);
    L.kind = t == 2 ? NUM_TEXT : NUM_LONG;
    L.v = t == 2 ? 0ull : (uint64_t)reinterpret_cast<const int64_t*>(r.v + idx)[field];
    L.text = avg.p;
    L.text_n = t == 2 ? avg.n : 0u;
  }
};

// Histogram: K `_hist_bucket` lines with le="<label>", the le="+Inf" line, _hist_sum, _hist_count.
struct LeBlock {
  using G = PromGrammar;
  static constexpr uint32_t K_MAX = LE_MAX;
  LeRows r;
  __device__ __forceinline__ bool kind_ok(uint32_t) const { return true; }
  __device__ __forceinline__ uint32_t values(uint32_t, uint32_t nvalues) const { return nvalues; }
  __device__ __forceinline__ uint32_t nlines(uint32_t, uint32_t) const { return r.K + 3u; }
  __device__ __forceinline__ bool prepare(uint32_t, uint32_t) const { return true; }
  __device__ __forceinline__ void line(uint32_t, uint32_t idx, uint32_t t, Line& L) const {
    const uint32_t K = r.K;
    const uint64_t* row = r.le_rows + (size_t)idx * (K + 1u);
    L.sfx = t <= K ? "_hist_bucket" : (t == K + 1u ? "_hist_sum" : "_hist_count");
    L.sfx_n = t <= K ? 12u : (t == K + 1u ? 9u : 11u);
    L.ext = "le=\"";
    L.ext_n = t <= K ? 4u : 0u;
    L.ev = t == K ? "+Inf" : nullptr;
    L.ev_n = t == K ? 4u : 0u;
    L.ev_num = t < K ? r.le[t] : 0;
    L.kind = t == K + 1u ? NUM_LONG : NUM_ULONG;
    L.v = t == K + 1u ? (r.sums ? (uint64_t)r.sums[idx] : 0ull) : row[t < K ? t : K];
    L.text = nullptr;
    L.text_n = 0u;
  }
};

// Configured quantiles: K lines with quantile="<label>", the label the quantile's
// Double.toString -- bytes the host formatted once per call, in global memory.
struct QuantileBlock {
  using G = PromGrammar;
  static constexpr uint32_t K_MAX = Q_MAX;
  QuantRows r;
  __device__ __forceinline__ bool kind_ok(uint32_t) const { return true; }
  __device__ __forceinline__ uint32_t values(uint32_t, uint32_t nvalues) const { return nvalues; }
  __device__ __forceinline__ uint32_t nlines(uint32_t, uint32_t) const { return r.K; }
  __device__ __forceinline__ bool prepare(uint32_t, uint32_t) const { return true; }
  __device__ __forceinline__ void line(uint32_t, uint32_t idx, uint32_t t, Line& L) const {
    const uint8_t* slot = r.labels + (size_t)t * RENDER_QLABEL_SLOT;
    L.sfx = "";
    L.sfx_n = 0u;
    L.ext = "quantile=\"";
    L.ext_n = 10u;
    L.ev = reinterpret_cast<const char*>(slot);
    L.ev_n = slot[RENDER_QLABEL_SLOT - 1];
    L.ev_num = 0;
    L.kind = NUM_LONG;
    L.v = (uint64_t)r.q_rows[(size_t)idx * r.K + t];
    L.text = nullptr;
    L.text_n = 0u;
  }
};

// What the JSON and the scalar block share: the count of a row's kind, and the row's text
// (a gauge's Float.toString, a stat's avg) in its slot -- between quotes when `quote` and
// the value is not finite, as jackson writes such a number.
struct KindBlock {
  KindRows r;
  __device__ __forceinline__ bool kind_ok(uint32_t j, bool stats) const {
    const uint8_t k = r.kinds[j];
    return kind_known(k) && (stats || k != KIND_STAT);
  }
  __device__ __forceinline__ uint32_t values(uint32_t j) const { return kind_count(r, r.kinds[j]); }
  __device__ __forceinline__ bool slot_text(uint32_t j, uint32_t idx, bool quote) const {
    const uint8_t k = r.kinds[j];
    if (k == KIND_COUNTER) return true;
    uint8_t* slot = r.slot + (size_t)j * RENDER_AVG_SLOT;
    int n;
    bool finite;
    if (k == KIND_GAUGE) {
      const float x = r.gauges[idx];
      uint32_t bits;
      __builtin_memcpy(&bits, &x, 4);
      finite = (bits & 0x7F800000u) != 0x7F800000u;
      n = slot_write(slot, x);
    } else {
      if (r.summaries[idx].count <= 0) return true;  // (the avg is printed only above 0: nlines)
      const double x = r.summaries[idx].avg;
      uint64_t bits;
      __builtin_memcpy(&bits, &x, 8);
      finite = (bits & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
      n = slot_write(slot, x);
    }
    if (quote && !finite && n > 0) {  // (NaN, Infinity, -Infinity) a byte to the right, between the quotes
      for (int i = n; i > 0; --i) slot[i] = slot[i - 1];
      slot[0] = slot[n + 1] = '"';
      slot[SLOT_LEN] = (uint8_t)(n + 2);
    }
    return n >= 0;
  }
  __device__ __forceinline__ void slot_line(uint32_t j, Line& L) const {
    const SlotText s = slot_read(r.slot + (size_t)j * RENDER_AVG_SLOT);
    L.kind = NUM_TEXT;
    L.v = 0ull;
    L.text = s.p;
    L.text_n = s.n;
  }
  __device__ __forceinline__ void plain(Line& L) const {  // no sfx, no extra label, no number yet
    L.sfx = "";
    L.sfx_n = 0u;
    L.ext = "";
    L.ext_n = 0u;
    L.ev = "";
    L.ev_n = 0u;
    L.ev_num = 0;
    L.kind = NUM_LONG;
    L.v = 0ull;
    L.text = nullptr;
    L.text_n = 0u;
  }
};

// /admin/metrics.json, flat and compact: a counter's or a gauge's entry; a stat's `.count`
// and, only when count > 0, STAT_FIELDS' nine longs and `.avg`.
struct JsonBlock {
  using G = JsonGrammar;
  static constexpr uint32_t K_MAX = 0u;
  KindBlock b;
  __device__ __forceinline__ bool kind_ok(uint32_t j) const { return b.kind_ok(j, true); }
  __device__ __forceinline__ uint32_t values(uint32_t j, uint32_t) const { return b.values(j); }
  __device__ __forceinline__ bool prepare(uint32_t j, uint32_t idx) const { return b.slot_text(j, idx, true); }
  __device__ __forceinline__ uint32_t nlines(uint32_t j, uint32_t idx) const {
    return b.r.kinds[j] == KIND_STAT && b.r.summaries[idx].count > 0 ? 11u : 1u;
  }
  __device__ __forceinline__ void line(uint32_t j, uint32_t idx, uint32_t t, Line& L) const {
    b.plain(L);
    const uint8_t k = b.r.kinds[j];
    if (k == KIND_COUNTER) {
      L.v = (uint64_t)b.r.counters[idx];
    } else if (k == KIND_GAUGE) {
      b.slot_line(j, L);
    } else {
      const char* sfx = ".count .max   .min   .p50   .p90   .p95   .p99   .p9990 .p9999 .sum   .avg";  // 7 bytes apart
      L.sfx = sfx + 7u * t;
      L.sfx_n = (uint32_t)(0x44664444446ull >> (4u * t)) & 15u;  // their lengths: 6 4 4 4 4 4 4 6 6 4 4
      // Summary88's words: count, min, max, sum, p50, p90, p95, p99, p9990, p9999
      const uint32_t field = t == 0 ? 0u : (t == 1 ? 2u : (t == 2 ? 1u : (t == 9 ? 3u : t + 1u)));
      if (t == 10)
        b.slot_line(j, L);
      else
        L.v = (uint64_t)reinterpret_cast<const int64_t*>(b.r.summaries + idx)[field];
    }
  }
};

// The counter and gauge lines of the Prometheus exposition: one line per row.
struct ScalarBlock {
  using G = PromGrammar;
  static constexpr uint32_t K_MAX = 0u;
  KindBlock b;
  __device__ __forceinline__ bool kind_ok(uint32_t j) const { return b.kind_ok(j, false); }
  __device__ __forceinline__ uint32_t values(uint32_t j, uint32_t) const { return b.values(j); }
  __device__ __forceinline__ bool prepare(uint32_t j, uint32_t idx) const { return b.slot_text(j, idx, false); }
  __device__ __forceinline__ uint32_t nlines(uint32_t, uint32_t) const { return 1u; }
  __device__ __forceinline__ void line(uint32_t j, uint32_t idx, uint32_t, Line& L) const {
    b.plain(L);
    if (b.r.kinds[j] == KIND_COUNTER)
      L.v = (uint64_t)b.r.counters[idx];
    else
      b.slot_line(j, L);
  }
};

// ---- length pass ------------------------------------------------------------------
template <class Block>
__global__ __launch_bounds__(256) void k_rd_len(RenderNames nm, uint32_t n, uint32_t nvalues, Block blk,
                                                uint32_t* __restrict__ len, uint32_t* __restrict__ flags) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint32_t idx = nm.index ? nm.index[j] : j;
  const uint64_t k0 = nm.key_off[j], k1 = nm.key_off[j + 1];
  constexpr bool labels = Block::G::labels;
  const uint64_t i0 = labels ? nm.lab_off[j] : 0ull, i1 = labels ? nm.lab_off[j + 1] : 0ull;
  bool ok = true;
  if (!blk.kind_ok(j)) {
    atomicMin(flags + RF_KIND, j);
    ok = false;
  } else if (idx >= blk.values(j, nvalues)) {
    atomicMin(flags + RF_BADIDX, j);
    ok = false;
  }
  if (k1 < k0 || i1 < i0) {
    atomicMin(flags + RF_BADOFF, j);
    ok = false;
  } else if (k1 - k0 > RENDER_NAME_MAX || i1 - i0 > RENDER_NAME_MAX || (k1 - k0) + (i1 - i0) > RENDER_NAME_MAX) {
    atomicMin(flags + RF_LONG, j);
    ok = false;
  }
  if (ok && !blk.prepare(j, idx)) {
    atomicMin(flags + RF_RANGE, j);
    ok = false;
  }
  uint32_t total = 0u;
  if (ok) {
    const uint32_t klen = (uint32_t)(k1 - k0), ilen = (uint32_t)(i1 - i0), nl = blk.nlines(j, idx);
    for (uint32_t t = 0; t < nl; ++t) {
      Line L;
      blk.line(j, idx, t, L);
      total += line_len<typename Block::G>(klen, ilen, L);
    }
  }
  len[j] = total;
}

// ---- write pass -------------------------------------------------------------------
// len bytes of src at dst, the wave together; pre = src[lane] (lanes < len).
__device__ __forceinline__ void emit(uint8_t* dst, const uint8_t* __restrict__ src, uint32_t len, uint8_t pre,
                                     uint32_t lane) {
  if (lane < len) dst[lane] = pre;
  for (uint32_t i = lane + 64u; i < len; i += 64u) dst[i] = src[i];
}

// Builds the row at dst (LDS or the output: the same code, inlined for each).  False: the
// lines add up to another length than rowlen, and nothing was written.
template <class Block>
__device__ __forceinline__ bool build_row(uint8_t* dst, const Block& blk, uint32_t j, uint32_t idx,
                                          const uint8_t* __restrict__ key, uint32_t klen,
                                          const uint8_t* __restrict__ inner, uint32_t ilen, uint32_t rowlen,
                                          uint32_t* lpos, uint32_t* ipos, uint32_t lane) {
  using G = typename Block::G;
  const uint32_t nl = blk.nlines(j, idx);
  // every line's place first: nothing is written before the total is known to match
  uint32_t cursor = 0u;
  for (uint32_t base = 0; base < nl; base += 64u) {  // (wave-uniform bounds)
    const uint32_t t = base + lane;
    Line L;
    uint32_t ln = 0u;
    if (t < nl) {
      blk.line(j, idx, t, L);
      ln = line_len<G>(klen, ilen, L);
    }
    const uint32_t incl = wave_incl_scan32(ln);
    if (t < nl) {
      lpos[t] = cursor + incl - ln;
      ipos[t] = cursor + incl - ln + line_head<G>(klen, ilen, L);
    }
    cursor += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  }
  if (cursor != rowlen) return false;
  __syncthreads();  // (one wave: orders lpos / ipos)
  for (uint32_t base = 0; base < nl; base += 64u) {
    const uint32_t t = base + lane;
    if (t < nl) {
      Line L;
      blk.line(j, idx, t, L);
      line_write<G>(dst, lpos[t], klen, ilen, L);
    }
  }
  const uint8_t kpre = lane < klen ? key[lane] : (uint8_t)0, ipre = lane < ilen ? inner[lane] : (uint8_t)0;
  for (uint32_t t = 0; t < nl; ++t) {
    emit(dst + lpos[t] + G::open_n, key, klen, kpre, lane);
    emit(dst + ipos[t], inner, ilen, ipre, lane);
  }
  return true;
}

template <class Block>
__global__ __launch_bounds__(64) void k_rd_write(RenderNames nm, uint32_t n, Block blk,
                                                 const uint64_t* __restrict__ offs, uint8_t* __restrict__ out,
                                                 uint32_t* __restrict__ flags) {
  __shared__ uint4 stage4[TEXT_STAGE / 16 + 1];  // (+16 bytes: the destination's offset within 16)
  __shared__ uint32_t lpos[RD_LINES_MAX], ipos[RD_LINES_MAX];
  const uint32_t lane = threadIdx.x;
  for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {  // (wave-uniform)
    const uint32_t idx = nm.index ? nm.index[j] : j;
    constexpr bool labels = Block::G::labels;
    const uint64_t k0 = nm.key_off[j], i0 = labels ? nm.lab_off[j] : 0ull, o0 = offs[j];
    const uint32_t klen = (uint32_t)(nm.key_off[j + 1] - k0), ilen = labels ? (uint32_t)(nm.lab_off[j + 1] - i0) : 0u;
    const uint32_t rowlen = (uint32_t)(offs[j + 1] - o0);
    const uint8_t* key = nm.key_bytes + k0;
    const uint8_t* inner = nm.lab_bytes + i0;
    uint8_t* gdst = out + o0;
    bool ok;
    if (rowlen <= TEXT_STAGE) {
      const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(gdst) & 15u);
      uint8_t* sdst = reinterpret_cast<uint8_t*>(stage4) + skew;
      ok = build_row(sdst, blk, j, idx, key, klen, inner, ilen, rowlen, lpos, ipos, lane);
      __syncthreads();
      if (ok) stage_flush(gdst, sdst, rowlen, skew, lane);
    } else {
      ok = build_row(gdst, blk, j, idx, key, klen, inner, ilen, rowlen, lpos, ipos, lane);
    }
    if (!ok && lane == 0) atomicMin(flags + RF_MISMATCH, j);
    __syncthreads();  // the stage and the places are reused by the next row
  }
}

// ---- Rows to Block ------------------------------------------------------------------
inline SummaryBlock block_of(const SummaryRows& r) { return {r}; }
inline LeBlock block_of(const LeRows& r) { return {r}; }
inline QuantileBlock block_of(const QuantRows& r) { return {r}; }
inline JsonBlock block_of(const JsonRows& r) { return {KindBlock{r.k}}; }
inline ScalarBlock block_of(const ScalarRows& r) { return {KindBlock{r.k}}; }

template <class Block>
bool k_in_range(const Block& blk) {
  if constexpr (Block::K_MAX > 0u) return blk.r.K >= 1u && blk.r.K <= Block::K_MAX;
  return true;
}

}  // namespace

template <class Rows>
hipError_t render_lengths(const RenderNames& nm, uint32_t n, uint32_t nvalues, const Rows& rows, uint32_t* len,
                          uint32_t* flags, hipStream_t st) {
  using Block = decltype(block_of(rows));
  const Block blk = block_of(rows);
  if (!k_in_range(blk)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rd_len<Block>, dim3((n + 255u) / 256u), dim3(256), 0, st, nm, n, nvalues, blk, len, flags);
  return hipGetLastError();
}

template <class Rows>
hipError_t render_write(const RenderNames& nm, uint32_t n, const Rows& rows, const uint64_t* offs, uint8_t* out,
                        uint32_t* flags, hipStream_t st) {
  using Block = decltype(block_of(rows));
  const Block blk = block_of(rows);
  if (!k_in_range(blk)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rd_write<Block>, dim3(n < TEXT_GRID_MAX ? n : TEXT_GRID_MAX), dim3(64), 0, st, nm, n, blk, offs, out,
                     flags);
  return hipGetLastError();
}

#define L5DH_RENDER_ROWS(R)                                                                                             \
  template hipError_t render_lengths(const RenderNames&, uint32_t, uint32_t, const R&, uint32_t*, uint32_t*, hipStream_t); \
  template hipError_t render_write(const RenderNames&, uint32_t, const R&, const uint64_t*, uint8_t*, uint32_t*, hipStream_t);
L5DH_RENDER_ROWS(SummaryRows) L5DH_RENDER_ROWS(LeRows) L5DH_RENDER_ROWS(QuantRows) L5DH_RENDER_ROWS(JsonRows) L5DH_RENDER_ROWS(ScalarRows)
#undef L5DH_RENDER_ROWS

}  // namespace l5dh
