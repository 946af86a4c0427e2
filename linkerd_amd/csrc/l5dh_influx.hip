// l5dh_influx.hip -- the InfluxDB line protocol body, produced where the numbers are.
//
// The rows of the table are the fields of the text in the order they are printed
// (l5dh_influx.hpp); a row carries its line's head, the host and the tail when it is the
// first of its line, a comma otherwise, and the newline when it is the last.  So the text
// is the concatenation of the rows, and lines are no entity of either pass: a line of
// 10^5 fields is 10^5 rows like any others.
//
//   k_ifx_len    a lane per row: checks the row (kind, field, index, line, offsets, piece
//                lengths), formats its gauge or avg once into the row's slot, and adds up
//                the row's pieces.
//   (scan)       the fleet merge's exclusive u32 -> u64 scan (merge_count): every byte's place.
//   k_ifx_write  a wave per chunk of 64 consecutive rows (one-wave workgroups striding over
//                the chunks), a lane per row.  The chunk's bytes are the contiguous range
//                [offs[j0], offs[j0 + 64)) whatever line boundaries fall inside it.  Each
//                lane lays its row out again and writes its own small pieces (`,` `=` the
//                number, the newline, and every text piece of at most IFX_COOP bytes); the
//                wave then copies the longer pieces together, one after the other.  A
//                chunk of at most TEXT_STAGE bytes is built in LDS at the destination's
//                offset within 16 bytes and leaves through stage_flush; a longer chunk is
//                built by the same code straight in the output.  Only chunk c's wave writes
//                chunk c's bytes.
//
// The slot, the stage's way out, `put`, the kinds and the write pass's sizes are
// l5dh_textout.hpp's, shared with l5dh_render.hip.
#include "l5dh_device.hpp"
#include "l5dh_influx.hpp"
#include "l5dh_textout.hpp"

namespace l5dh {
namespace {

constexpr uint32_t IFX_ROWS = 64;            // rows of a chunk: a lane each
constexpr uint32_t IFX_COOP = 48;            // a text piece above this many bytes is copied by the wave together
constexpr uint32_t AVG_FIELD = 10;           // Summary88's last word: the avg, a double

// A row of a table the length pass found valid, laid out: its pieces and their lengths.
struct Row {
  bool first, last;     // of its line
  bool text;            // the value is the slot's text vtext (a gauge, an avg); else the long v
  uint32_t hlen, tlen;  // the line's head and tail (first rows only, else 0)
  uint32_t klen, vlen;
  uint64_t h0, t0, k0;  // where head, tail and key begin in their byte arrays
  int64_t v;
  const uint8_t* vtext;
};

__device__ __forceinline__ void row_layout(const InfluxRows& r, uint32_t n, uint32_t j, Row& R) {
  const uint32_t l = r.line[j];
  R.first = j == 0 || r.line[j - 1] != l;
  R.last = j == n - 1 || r.line[j + 1] != l;
  R.k0 = r.key_off[j];
  R.klen = (uint32_t)(r.key_off[j + 1] - R.k0);
  R.h0 = R.t0 = 0ull;
  R.hlen = R.tlen = 0u;
  if (R.first) {
    R.h0 = r.head_off[l];
    R.hlen = (uint32_t)(r.head_off[l + 1] - R.h0);
    R.t0 = r.tail_off[l];
    R.tlen = (uint32_t)(r.tail_off[l + 1] - R.t0);
  }
  const uint8_t k = r.k.kinds[j];
  const uint32_t idx = r.index[j];
  R.v = 0;
  R.vtext = nullptr;
  if (k == KIND_COUNTER) {
    R.text = false;
    R.v = r.k.counters[idx];
  } else if (k == KIND_STAT && r.field[j] != AVG_FIELD) {
    R.text = false;
    R.v = reinterpret_cast<const int64_t*>(r.k.summaries + idx)[r.field[j]];
  } else {
    R.text = true;
  }
  if (R.text) {
    const SlotText s = slot_read(r.k.slot + (size_t)j * RENDER_AVG_SLOT);
    R.vtext = s.p;
    R.vlen = s.n;
  } else {
    R.vlen = (uint32_t)fmt::long_digits(R.v);
  }
}

// Bytes before the key: head, host and tail, or the comma.
__device__ __forceinline__ uint32_t row_pre(const Row& R, uint32_t host_len) {
  return R.first ? R.hlen + host_len + R.tlen : 1u;
}
__device__ __forceinline__ uint32_t row_len(const Row& R, uint32_t host_len) {
  return row_pre(R, host_len) + R.klen + 1u + R.vlen + (R.last ? 1u : 0u);
}

// ---- length pass ------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ifx_len(InfluxRows r, uint32_t n, uint32_t* __restrict__ len,
                                                 uint32_t* __restrict__ flags) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint8_t k = r.k.kinds[j];
  const uint32_t idx = r.index[j], l = r.line[j];
  bool ok = true;
  if (!kind_known(k)) {
    atomicMin(flags + IF_KIND, j);
    ok = false;
  } else {
    if (k == KIND_STAT && r.field[j] > AVG_FIELD) {
      atomicMin(flags + IF_FIELD, j);
      ok = false;
    }
    if (idx >= kind_count(r.k, k)) {
      atomicMin(flags + IF_BADIDX, j);
      ok = false;
    }
  }
  const bool line_ok = l < r.nlines && !(j > 0 && r.line[j - 1] > l);
  if (!line_ok) {
    atomicMin(flags + IF_LINE, j);
    ok = false;
  }
  const uint64_t k0 = r.key_off[j], k1 = r.key_off[j + 1];
  uint64_t klen = 0ull, hlen = 0ull, tlen = 0ull, hostlen = 0ull;
  if (k1 < k0) {
    atomicMin(flags + IF_KEYOFF, j);
    ok = false;
  } else {
    klen = k1 - k0;
  }
  if (line_ok && (j == 0 || r.line[j - 1] != l)) {  // the line's first row reads its offsets
    const uint64_t h0 = r.head_off[l], h1 = r.head_off[l + 1], t0 = r.tail_off[l], t1 = r.tail_off[l + 1];
    if (h1 < h0 || t1 < t0) {
      atomicMin(flags + IF_LINEOFF, j);
      ok = false;
    } else {
      hlen = h1 - h0;
      tlen = t1 - t0;
      hostlen = r.host_len;
    }
  }
  constexpr uint64_t M = RENDER_NAME_MAX;  // (each below M first: their sum cannot wrap)
  if (ok && (klen > M || hlen > M || tlen > M || klen + hlen + tlen + hostlen > M)) {
    atomicMin(flags + IF_LONG, j);
    ok = false;
  }
  if (ok && (k == KIND_GAUGE || (k == KIND_STAT && r.field[j] == AVG_FIELD))) {
    uint8_t* slot = r.k.slot + (size_t)j * RENDER_AVG_SLOT;
    const int m = k == KIND_GAUGE ? slot_write(slot, r.k.gauges[idx]) : slot_write(slot, r.k.summaries[idx].avg);
    if (m < 0) {
      atomicMin(flags + IF_RANGE, j);
      ok = false;
    }
  }
  uint32_t total = 0u;
  if (ok) {
    Row R;
    row_layout(r, n, j, R);
    total = row_len(R, r.host_len);
  }
  len[j] = total;
}

// ---- write pass -------------------------------------------------------------------
// The wave copies, one after the other, the piece src[0 .. len) of every lane that wants
// it to dst + at (that lane's values).  Convergent: the whole wave calls it.
__device__ __forceinline__ void copy_together(uint8_t* dst, bool want, uint32_t at, const uint8_t* src, uint32_t len,
                                              uint32_t lane) {
  unsigned long long m = __ballot(want);
  const uint64_t s = reinterpret_cast<uint64_t>(src);
  while (m) {  // (wave-uniform)
    const int from = __ffsll((long long)m) - 1;
    m &= m - 1ull;
    const uint32_t p = __shfl(at, from, 64), ln = __shfl(len, from, 64);
    const uint8_t* sp = reinterpret_cast<const uint8_t*>(((uint64_t)__shfl((uint32_t)(s >> 32), from, 64) << 32) |
                                                         __shfl((uint32_t)s, from, 64));
    for (uint32_t i = lane; i < ln; i += 64u) dst[p + i] = sp[i];
  }
}

// Builds the chunk at dst (LDS or the output: the same code, inlined for each): lane t's row
// at dst + pos.  Writes inside [pos, pos + row_len) only.
__device__ __forceinline__ void build_chunk(uint8_t* dst, const InfluxRows& r, const Row& R, bool valid, uint32_t pos,
                                            uint32_t lane) {
  const uint32_t host_len = r.host_len, pre = row_pre(R, host_len);
  const uint8_t* head = r.head_bytes + R.h0;
  const uint8_t* tail = r.tail_bytes + R.t0;
  const uint8_t* key = r.key_bytes + R.k0;
  if (valid) {
    if (R.first) {
      if (R.hlen <= IFX_COOP) put(dst, pos, head, R.hlen);
      if (host_len <= IFX_COOP) put(dst, pos + R.hlen, r.host, host_len);
      if (R.tlen <= IFX_COOP) put(dst, pos + R.hlen + host_len, tail, R.tlen);
    } else {
      dst[pos] = ',';
    }
    uint32_t p = pos + pre;
    if (R.klen <= IFX_COOP) put(dst, p, key, R.klen);
    p += R.klen;
    dst[p++] = '=';
    if (R.text)
      put(dst, p, R.vtext, R.vlen);
    else
      fmt::format_long(R.v, dst + p);
    if (R.last) dst[p + R.vlen] = '\n';
  }
  const bool lead = valid && R.first;
  copy_together(dst, lead && R.hlen > IFX_COOP, pos, head, R.hlen, lane);
  copy_together(dst, lead && host_len > IFX_COOP, pos + R.hlen, r.host, host_len, lane);
  copy_together(dst, lead && R.tlen > IFX_COOP, pos + R.hlen + host_len, tail, R.tlen, lane);
  copy_together(dst, valid && R.klen > IFX_COOP, pos + pre, key, R.klen, lane);
}

__global__ __launch_bounds__(64) void k_ifx_write(InfluxRows r, uint32_t n, const uint64_t* __restrict__ offs,
                                                  uint8_t* __restrict__ out, uint32_t* __restrict__ flags) {
  __shared__ uint4 stage4[TEXT_STAGE / 16 + 1];  // (+16 bytes: the destination's offset within 16)
  const uint32_t lane = threadIdx.x;
  const uint32_t nchunks = (n + IFX_ROWS - 1u) / IFX_ROWS;
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {  // (wave-uniform)
    const uint32_t j0 = c * IFX_ROWS, j = j0 + lane;
    const bool valid = j < n;
    const uint64_t o0 = offs[j0], o1 = offs[min(j0 + IFX_ROWS, n)];
    const uint32_t chunklen = (uint32_t)(o1 - o0);  // (64 rows of at most 2^25 + 29 bytes)
    Row R{};
    uint32_t pos = 0u;
    bool differs = false;
    if (valid) {
      row_layout(r, n, j, R);
      const uint64_t o = offs[j];
      pos = (uint32_t)(o - o0);
      differs = (uint64_t)row_len(R, r.host_len) != offs[j + 1] - o;
    }
    // nothing of a chunk is written unless every row's layout is the length pass's
    const unsigned long long bad = __ballot(differs);
    if (bad) {
      if (lane == 0) atomicMin(flags + IF_MISMATCH, j0 + (uint32_t)__ffsll((long long)bad) - 1u);
      continue;
    }
    uint8_t* gdst = out + o0;
    if (chunklen <= TEXT_STAGE) {
      const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(gdst) & 15u);
      uint8_t* sdst = reinterpret_cast<uint8_t*>(stage4) + skew;
      build_chunk(sdst, r, R, valid, pos, lane);
      __syncthreads();
      stage_flush(gdst, sdst, chunklen, skew, lane);
      __syncthreads();  // the stage is reused by the next chunk
    } else {
      build_chunk(gdst, r, R, valid, pos, lane);
    }
  }
}

}  // namespace

hipError_t influx_lengths(const InfluxRows& r, uint32_t n, uint32_t* len, uint32_t* flags, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ifx_len, dim3((n + 255u) / 256u), dim3(256), 0, st, r, n, len, flags);
  return hipGetLastError();
}

hipError_t influx_write(const InfluxRows& r, uint32_t n, const uint64_t* offs, uint8_t* out, uint32_t* flags,
                        hipStream_t st) {
  if (n == 0) return hipSuccess;
  const uint32_t nchunks = (n + IFX_ROWS - 1u) / IFX_ROWS;
  hipLaunchKernelGGL(k_ifx_write, dim3(nchunks < TEXT_GRID_MAX ? nchunks : TEXT_GRID_MAX), dim3(64), 0, st, r, n, offs, out,
                     flags);
  return hipGetLastError();
}

}  // namespace l5dh
