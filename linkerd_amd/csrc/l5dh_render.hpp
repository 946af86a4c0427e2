// l5dh_render.hpp -- the Prometheus exposition of Stats, rendered on the device
// (l5dh_render.hip): per row of a name table the summary block, the `_hist` block or the
// configured quantiles' block, byte for byte what linkerd_amd/prometheus.py prints; the
// counter and gauge lines of the same exposition (the scalar block), and the entries of
// the flat compact /admin/metrics.json document (the JSON block), byte for byte
// linkerd_amd/admin_metrics.py's write_flat_json.
#pragma once

#include "l5dh_kernels.hpp"
#include "l5dh_le.hpp"
#include "l5dh_quant.hpp"

namespace l5dh {

// The name table (device pointers): row j prints element index[j] (null: j) of the value
// arrays under the escaped key key_bytes[key_off[j] .. key_off[j+1]) and the escaped text
// between the braces lab_bytes[lab_off[j] .. lab_off[j+1]) (may be empty).
struct RenderNames {
  const uint32_t* index;
  const uint64_t* key_off;
  const uint8_t* key_bytes;
  const uint64_t* lab_off;  // (the JSON block has no label text: it reads neither lab_off nor lab_bytes)
  const uint8_t* lab_bytes;
};

// The flag words of a call: each the least row with that finding (0xFFFFFFFF: none).
enum {
  RF_BADIDX = 0,    // index[j] >= nvalues (the JSON and scalar blocks: the count of the row's kind)
  RF_BADOFF = 1,    // key_off or lab_off descends at row j
  RF_RANGE = 2,     // the row's avg (or gauge) is outside the formatter's domain
  RF_LONG = 3,      // key + label text above RENDER_NAME_MAX bytes (a row would pass 2^32 bytes)
  RF_MISMATCH = 4,  // the write pass laid a row out to another length than the length pass (internal)
  RF_KIND = 5,      // kinds[j] is not a kind the call prints
  RF_WORDS = 8
};
// 67 lines (L5DH_LE_MAX cuts) of a name this long, their fixed text and numbers stay below 2^32.
constexpr uint64_t RENDER_NAME_MAX = 1ull << 25;
// per row: the avg's or the gauge's text (26 bytes at most, 28 between quotes), its length in the
// last byte (the layout is l5dh_textout.hpp's)
constexpr uint32_t RENDER_AVG_SLOT = 32;

// The values of a call (device pointers).
struct SummaryRows {
  const Summary88* v;  // [nvalues]
  uint8_t* avg;        // [n][RENDER_AVG_SLOT]: written by the length pass, read by the write pass
};
struct LeRows {
  const uint64_t* le_rows;  // [nvalues][K + 1]
  const int64_t* sums;      // [nvalues], nullable: 0
  const int64_t* le;        // [K] the labels
  uint32_t K;
};
constexpr uint32_t RENDER_QLABEL_SLOT = 32;  // per quantile: its Double.toString (26 bytes at most), the length last
struct QuantRows {
  const int64_t* q_rows;  // [nvalues][K]
  const uint8_t* labels;  // [K][RENDER_QLABEL_SLOT]: formatted once per call on the host
  uint32_t K;
};

// The JSON and the scalar block: a row's kind selects its value array, and index[j] counts
// within that kind.  A null array has count 0.
enum : uint8_t { KIND_COUNTER = 0, KIND_GAUGE = 1, KIND_STAT = 2 };  // = L5DH_KIND_*
struct KindRows {
  const uint8_t* kinds;      // [n]
  const Summary88* summaries;
  const int64_t* counters;
  const float* gauges;
  uint32_t nsummaries, ncounters, ngauges;
  uint8_t* slot;             // [n][RENDER_AVG_SLOT]: the gauge's or the avg's text, as SummaryRows::avg
};
struct JsonRows { KindRows k; };    // entries `"key sfx":number,` (the caller writes the braces)
struct ScalarRows { KindRows k; };  // lines `key[{inner}] number\n`; a stat row is RF_KIND

// Both passes are templates over the Rows struct of the call, instantiated in
// l5dh_render.hip for the five above; hipErrorInvalidValue: LeRows' K outside [1, LE_MAX],
// QuantRows' outside [1, Q_MAX].
// Length pass: len[j] = bytes of row j's block for j < n (a row with a finding: 0, and its
// flag word is lowered).  flags must hold 0xFFFFFFFF words.  (JsonRows, ScalarRows: nvalues
// is not read, the counts are the rows'.)
template <class Rows>
hipError_t render_lengths(const RenderNames& nm, uint32_t n, uint32_t nvalues, const Rows& rows, uint32_t* len,
                          uint32_t* flags, hipStream_t st);
// Write pass: row j's block at out + offs[j] (offs: the exclusive prefix of len, offs[n] the
// total).  Only launched when the length pass raised no flag: it trusts the table.
template <class Rows>
hipError_t render_write(const RenderNames& nm, uint32_t n, const Rows& rows, const uint64_t* offs, uint8_t* out,
                        uint32_t* flags, hipStream_t st);

}  // namespace l5dh
