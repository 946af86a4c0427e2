// l5dh_influx.hpp -- the InfluxDB line protocol body, rendered on the device
// (l5dh_influx.hip): byte for byte what linkerd_amd/influxdb.py's write_metrics prints,
// from a table whose rows are the FIELDS in the order they are printed
// (linkerd_amd/render_influx.py builds it).
#pragma once

#include "l5dh_render.hpp"

namespace l5dh {

// The table (device pointers).  Row j < n of line l = line[j] prints
//   ( first row of l ? head[l] host tail[l] : `,` )  key  `=`  value  ( last row of l ? `\n` : nothing )
// first: j == 0 or line[j-1] != l; last: j == n-1 or line[j+1] != l.
struct InfluxRows {
  KindRows k;                // the rows' kinds [n], the three value arrays and their counts, the slots
  const uint32_t* line;      // [n] non-decreasing, < nlines
  const uint8_t* field;      // [n] a stat row's word of Summary88 (0 .. 10); not read for other kinds
  const uint32_t* index;     // [n] the element of the row's kind's value array
  const uint64_t* key_off;   // [n + 1]
  const uint8_t* key_bytes;
  const uint64_t* head_off;  // [nlines + 1]
  const uint8_t* head_bytes;
  const uint64_t* tail_off;  // [nlines + 1]
  const uint8_t* tail_bytes;
  const uint8_t* host;       // [host_len]
  uint32_t host_len, nlines;
};

// The flag words of a call: each the least row with that finding (0xFFFFFFFF: none).
enum {
  IF_KIND = 0,      // kinds[j] is none of the three
  IF_FIELD = 1,     // field[j] > 10 on a stat row
  IF_BADIDX = 2,    // index[j] >= the count of the row's kind
  IF_LINE = 3,      // line[j] >= nlines, or line[j] < line[j-1]
  IF_KEYOFF = 4,    // key_off descends at row j
  IF_LINEOFF = 5,   // head_off or tail_off descends at row j's line
  IF_LONG = 6,      // the row's pieces (head, host, tail, key) exceed RENDER_NAME_MAX bytes
  IF_RANGE = 7,     // the row's avg is outside the formatter's domain
  IF_MISMATCH = 8,  // the write pass laid a row out to another length than the length pass (internal)
  IF_WORDS = 12
};

// Length pass: len[j] = bytes of row j's pieces, prefix and suffix included (a row with a
// finding: 0, and its flag word is lowered).  flags must hold 0xFFFFFFFF words.  One
// exclusive scan of len then gives every byte's place.
hipError_t influx_lengths(const InfluxRows& r, uint32_t n, uint32_t* len, uint32_t* flags, hipStream_t st);
// Write pass: row j's bytes at out + offs[j] (offs: the exclusive prefix of len, offs[n] the
// total).  Only launched when the length pass raised no flag: it trusts the table.
hipError_t influx_write(const InfluxRows& r, uint32_t n, const uint64_t* offs, uint8_t* out, uint32_t* flags,
                        hipStream_t st);

}  // namespace l5dh
