// l5dh_textout.hpp -- device-only: what the text kernels of l5dh_render.hip and
// l5dh_influx.hip share.  Either has a length pass (a lane per row) that formats a row's
// gauge or avg once into the row's slot, and a write pass of one-wave workgroups that builds
// a unit of text (a row / a chunk of 64 rows) in LDS and stores it 16 aligned bytes at a time.
// Everything is forced inline: an out-of-line formatter once cost render_summaries 8 %.
#pragma once

#include "l5dh_fmt.hpp"
#include "l5dh_render.hpp"

namespace l5dh {

constexpr uint32_t TEXT_STAGE = 4096;          // bytes of a unit built in LDS
constexpr uint32_t TEXT_GRID_MAX = 256 * 32;   // one-wave workgroups of a write pass

template <class S>
__device__ __forceinline__ uint32_t put(uint8_t* dst, uint32_t p, const S* __restrict__ s, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) dst[p + i] = (uint8_t)s[i];
  return p + n;
}

// The wave stores the len bytes it built at sdst (LDS, at offset skew = gdst & 15 of a
// 16-byte aligned stage) to gdst: a head up to the output's first 16-byte boundary, an
// aligned 16-byte body, a tail.  The caller has synchronized after building.
__device__ __forceinline__ void stage_flush(uint8_t* gdst, const uint8_t* sdst, uint32_t len, uint32_t skew,
                                            uint32_t lane) {
  const uint32_t head = min(len, (16u - skew) & 15u);
  if (lane < head) gdst[lane] = sdst[lane];
  const uint32_t body = (len - head) >> 4;
  const uint4* s4 = reinterpret_cast<const uint4*>(sdst + head);  // (skew + head is a multiple of 16, or body == 0)
  uint4* g4 = reinterpret_cast<uint4*>(gdst + head);
  for (uint32_t i = lane; i < body; i += 64u) g4[i] = s4[i];
  const uint32_t done = head + (body << 4);
  if (done + lane < len) gdst[done + lane] = sdst[done + lane];  // (< 16 bytes)
}

__device__ __forceinline__ bool kind_known(uint8_t k) { return k == KIND_COUNTER || k == KIND_GAUGE || k == KIND_STAT; }
// The values a row of a known kind indexes.
__device__ __forceinline__ uint32_t kind_count(const KindRows& r, uint8_t k) {
  return k == KIND_COUNTER ? r.ncounters : (k == KIND_GAUGE ? r.ngauges : r.nsummaries);
}

// A row's slot: RENDER_AVG_SLOT bytes of scratch, written by the length pass and read by
// the write pass.  The text begins at the slot's first byte, its length is in byte SLOT_LEN.
// (The beginning is fixed, not stored: a stored one is a load the text's own loads wait
// for.  A version with a stored beginning and a `put` without __restrict__ made render_influx
// 2 % slower; the two were not measured apart.)  A block may lengthen the text by two bytes
// (the JSON block's quotes).
constexpr uint32_t SLOT_LEN = RENDER_AVG_SLOT - 1;
static_assert(fmt::DOUBLE_CHARS + 3 <= (int)RENDER_AVG_SLOT && fmt::FLOAT_CHARS <= fmt::DOUBLE_CHARS,
              "the text, two more bytes and the length share a slot");

// x's Float.toString (a float) or Double.toString (a double) into the slot; its length,
// or below 0: x is outside the formatter's domain (the slot then reads as empty).
template <class T>
__device__ __forceinline__ int slot_write(uint8_t* slot, T x) {
  int n;
  if constexpr (sizeof(T) == 4)
    n = fmt::format_float(x, slot);
  else
    n = fmt::format_double(x, slot);
  slot[SLOT_LEN] = (uint8_t)(n < 0 ? 0 : n);
  return n;
}

struct SlotText {
  const uint8_t* p;
  uint32_t n;
};
__device__ __forceinline__ SlotText slot_read(const uint8_t* slot) { return {slot, slot[SLOT_LEN]}; }

}  // namespace l5dh
