// l5dh_fleet.cpp -- the fleet merge of the C-ABI (include/l5dhist.h): every rank's
// pending samples and state exported (dense rows, or sparse row encodings for the
// reduce-scatter), exchanged over RCCL or among a loopback group's contexts on one
// device, and this rank's rows summarized.  Context and shared helpers: l5dh_ctx.hpp.
#include <algorithm>
#include <cerrno>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "l5dh_ctx.hpp"

using namespace l5dh;

namespace {

int ncclfail(l5dh_ctx* c, ncclResult_t e, const char* what) {
  c->last_error = std::string(what) + ": " + ncclGetErrorString(e);
  return -EIO;
}

#define NCCLCHK(c, expr)                                     \
  do {                                                       \
    ncclResult_t _e = (expr);                                \
    if (_e != ncclSuccess) return ncclfail((c), _e, #expr);  \
  } while (0)

uint32_t merge_per(const l5dh_ctx* c) { return (c->S + c->nranks - 1) / c->nranks; }

// Phase 1: pending samples + state -> dense rows [Sp][1798] and totals [Sp] (the
// fused whole-range export with reset), pad rows zero.
bool merge_skips_collective(const l5dh_ctx* c);

int merge_export(l5dh_ctx* c, int mode) {
  if (!c->comm && !c->loopback)
    return fail(c, -EINVAL, "no communicator: call l5dh_comm_init_rank or l5dh_comm_init_all first");
  int r = flush_ring(c);
  if (r) return r;
  const size_t Sp = (size_t)merge_per(c) * c->nranks;
  // the reduce-scatter through the collective exports SPARSE: each row's encoding straight
  // from the accumulate kernels' bins (no dense rows, no re-read), words and first word per
  // row; the all-reduce and a 1-rank communicator that skips the collective export dense rows
  c->m_sparse = mode == L5DH_MERGE_REDUCE_SCATTER && !merge_skips_collective(c);
  if ((r = ensure(c, c->merge_totals, Sp * 8)) || (r = ensure(c, c->m_words, (Sp + 1) * 4))) return r;
  int64_t* tot = c->merge_totals.as<int64_t>();
  uint32_t* words = c->m_words.as<uint32_t>();
  if (Sp > c->S) HIPCHK(c, hipMemsetAsync(tot + c->S, 0, (Sp - c->S) * 8, c->stream));
  HIPCHK(c, hipMemsetAsync(words + c->S, 0, (Sp + 1 - c->S) * 4, c->stream));
  if (c->m_sparse) {
    if ((r = ensure(c, c->m_roff, Sp * 4))) return r;
    Outputs o{nullptr, nullptr, 0, c->S, tot, words, nullptr, c->m_roff.as<uint32_t>()};
    return aggregate(c, 1, 1, o, true);
  }
  if ((r = ensure(c, c->merge_counts, Sp * NB * 4))) return r;
  int32_t* cnt = c->merge_counts.as<int32_t>();
  if (Sp > c->S) HIPCHK(c, hipMemsetAsync(cnt + (size_t)c->S * NB, 0, (Sp - c->S) * NB * 4, c->stream));
  return aggregate(c, 1, 1, Outputs{nullptr, cnt, 0, c->S, tot, words, nullptr, nullptr});
}

// Phase 2 (reduce-scatter): the rows are exchanged sparse (l5dh_merge.hip) -- per
// destination rank, the non-empty buckets of its slice plus the words per row --
// and the totals by one int64 reduce-scatter.  A 1-rank communicator skips it (an
// identity) unless L5DH_PARAM_MERGE_RCCL_1RANK forces it, with the encoding sent to
// itself through RCCL.  Steps: pack (local: the export's row encodings in row order),
// sizes (collective: an all-gather of the words-to matrix), receive buffers (local,
// one host wait), payload (collective).  l5dh_merge_all groups each collective step
// over its contexts.  The forcing parameter applies to an RCCL communicator only: a
// 1-rank loopback group has no transport that could carry the slice to itself (its
// copies skip p == q), so it always takes the identity.
bool merge_skips_collective(const l5dh_ctx* c) { return c->nranks == 1 && (!c->rccl_1rank || c->loopback); }

int merge_pack_step(l5dh_ctx* c) {
  const uint32_t per = merge_per(c);
  const uint32_t Sp = per * (uint32_t)c->nranks;
  const int W = c->nranks;
  int r;
  KTimer kt(c, L5DH_K_MERGE);
  c->m_tmp_bytes = 0;  // (the scans of every slice fit the storage of this, the longest one)
  HIPCHK(c, merge_count(Sp, nullptr, nullptr, nullptr, &c->m_tmp_bytes, c->stream));
  if ((r = ensure(c, c->m_words, ((size_t)Sp + 1) * 4)) || (r = ensure(c, c->m_offs, ((size_t)Sp + 1) * 8)) ||
      (r = ensure(c, c->m_tmp, c->m_tmp_bytes)) || (r = ensure(c, c->m_sizes, (size_t)W * W * 8)))
    return r;
  uint32_t* words = c->m_words.as<uint32_t>();
  uint64_t* offs = c->m_offs.as<uint64_t>();
  HIPCHK(c, merge_count(Sp, words, offs, c->m_tmp.p, &c->m_tmp_bytes, c->stream));  // (words: the export's)
  // this rank's row of the size matrix (for the all-gather) written on the device: the
  // slice sizes reach the host with the matrix, in the receive step's one host wait
  HIPCHK(c, merge_sizes_row(offs, per, W, c->m_sizes.as<uint64_t>() + (size_t)c->rank * W, c->stream));
  // (the packed encoding is no larger than the unpacked one)
  if ((r = ensure(c, c->m_enc, c->m_unpacked_words * 4 + 16))) return r;
  // the export's row encodings packed in row order (one contiguous slice per destination)
  HIPCHK(c, merge_pack(c->m_unpacked.as<const uint32_t>(), c->m_roff.as<const uint32_t>(), offs,
                       (uint32_t)std::min<size_t>(Sp, c->S), c->m_enc.as<uint32_t>(), c->stream));
  c->m_dense_bytes = (uint64_t)Sp * (NB * 4 + 8);
  return 0;
}

int merge_sizes_step(l5dh_ctx* c) {
  const int W = c->nranks;
  uint64_t* m = c->m_sizes.as<uint64_t>();
  NCCLCHK(c, ncclAllGather(m + (size_t)c->rank * W, m, (size_t)W, ncclUint64, c->comm, c->stream));
  return 0;
}

int merge_recv_step(l5dh_ctx* c) {
  const uint32_t per = merge_per(c);
  const int W = c->nranks;
  std::vector<uint64_t> mat((size_t)W * W);
  HIPCHK(c, hipMemcpyAsync(mat.data(), c->m_sizes.p, mat.size() * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->m_from.assign(W, 0);
  c->m_to.assign(W, 0);
  uint64_t all = 0, mine = 0;
  for (int s = 0; s < W; ++s) all += (c->m_from[s] = mat[(size_t)s * W + c->rank]);
  for (int q = 0; q < W; ++q) mine += (c->m_to[q] = mat[(size_t)c->rank * W + q]);
  c->m_encoded_bytes = mine * 4 + (uint64_t)per * W * (4 + 8);  // entries + words per row + totals
  int r;
  if ((r = ensure(c, c->r_enc, (size_t)all * 4 + 16)) || (r = ensure(c, c->r_words, (size_t)W * per * 4)) ||
      (r = ensure(c, c->r_offs, (size_t)W * per * 8)) || (r = ensure(c, c->recv_totals, (size_t)per * 8)))
    return r;
  uint64_t sent = 0;
  for (int q = 0; q < W; ++q)
    if (q != c->rank) sent += 4 * c->m_to[q] + 4ull * per + 8ull * per;
  c->m_sent_bytes = sent;
  return 0;
}

int merge_payload_step(l5dh_ctx* c) {
  const uint32_t per = merge_per(c);
  const int W = c->nranks;
  const uint32_t* enc = c->m_enc.as<const uint32_t>();
  const uint32_t* words = c->m_words.as<const uint32_t>();
  uint32_t* renc = c->r_enc.as<uint32_t>();
  uint32_t* rwords = c->r_words.as<uint32_t>();
  KTimer kt(c, L5DH_K_MERGE);
  uint64_t at = 0, rat = 0;
  for (int q = 0; q < W; ++q) {
    // (the local slice is read in place, except in a forced 1-rank exchange)
    if (q != c->rank || W == 1) {
      if (c->m_to[q]) NCCLCHK(c, ncclSend(enc + at, c->m_to[q], ncclUint32, q, c->comm, c->stream));
      NCCLCHK(c, ncclSend(words + (size_t)q * per, per, ncclUint32, q, c->comm, c->stream));
      if (c->m_from[q]) NCCLCHK(c, ncclRecv(renc + rat, c->m_from[q], ncclUint32, q, c->comm, c->stream));
      NCCLCHK(c, ncclRecv(rwords + (size_t)q * per, per, ncclUint32, q, c->comm, c->stream));
    }
    at += c->m_to[q];
    rat += c->m_from[q];
  }
  NCCLCHK(c, ncclReduceScatter(c->merge_totals.p, c->recv_totals.p, per, ncclInt64, ncclSum, c->comm, c->stream));
  return 0;
}

int merge_dense_allreduce(l5dh_ctx* c) {
  const size_t Sp = (size_t)merge_per(c) * c->nranks;
  KTimer kt(c, L5DH_K_MERGE);
  c->m_dense_bytes = c->m_encoded_bytes = Sp * (NB * 4 + 8);
  c->m_sent_bytes = c->nranks > 1 ? 2 * c->m_dense_bytes * (c->nranks - 1) / c->nranks : 0;
  NCCLCHK(c, ncclAllReduce(c->merge_counts.p, c->merge_counts.p, Sp * NB, ncclInt32, ncclSum, c->comm, c->stream));
  NCCLCHK(c, ncclAllReduce(c->merge_totals.p, c->merge_totals.p, Sp, ncclInt64, ncclSum, c->comm, c->stream));
  return 0;
}

// Phase 3: the rows this rank receives -- decoded from every source and summarized
// (reduce-scatter), or the all-reduced dense rows summarized -- and the copies.
int merge_finish(l5dh_ctx* c, int mode, l5dh_summary* out, int32_t* counts_out, int64_t* totals_out, uint32_t* first,
                 uint32_t* count) {
  const uint32_t per = merge_per(c);
  const bool rs = mode == L5DH_MERGE_REDUCE_SCATTER;
  const bool sparse = rs && !merge_skips_collective(c);
  const uint32_t f = rs ? (uint32_t)std::min<uint64_t>((uint64_t)c->rank * per, c->S) : 0u;
  const uint32_t n = rs ? std::min<uint32_t>(per, c->S - f) : c->S;
  if (first) *first = f;
  if (count) *count = n;
  if (n == 0) return sync_stream(c);
  int r;
  StagedOut<Summary88> summ;
  if ((r = summ.begin(c, out, n, c->stage_summ))) return r;
  const int32_t* rows = c->merge_counts.as<const int32_t>();
  const int64_t* tots = c->merge_totals.as<const int64_t>();
  if (sparse) {
    const int W = c->nranks;
    if (W > MERGE_MAX_RANKS) return fail(c, -EINVAL, "fleet merge: more than 64 ranks");
    StagedOut<int32_t> drows;  // the decoded rows: to the caller's memory, or staged
    if ((r = drows.begin(c, counts_out, (size_t)n * NB, c->recv_counts))) return r;
    // the received slices are contiguous in r_enc / r_words, source by source; this
    // rank's own slice (not sent) is copied to its place there, and one scan of the
    // [W][per] word counts gives every source's row offsets
    KTimer kt(c, L5DH_K_MERGE);
    uint32_t* renc = c->r_enc.as<uint32_t>();
    uint32_t* rwords = c->r_words.as<uint32_t>();
    if (W > 1) {
      uint64_t a0 = 0, rat = 0;
      for (int k = 0; k < c->rank; ++k) {
        a0 += c->m_to[k];
        rat += c->m_from[k];
      }
      if (c->m_to[c->rank])
        HIPCHK(c, hipMemcpyAsync(renc + rat, c->m_enc.as<const uint32_t>() + a0, c->m_to[c->rank] * 4,
                                 hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(rwords + (size_t)c->rank * per, c->m_words.as<const uint32_t>() + (size_t)c->rank * per,
                               (size_t)per * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    uint64_t* roffs = c->r_offs.as<uint64_t>();
    HIPCHK(c, merge_offsets(rwords, (uint32_t)((size_t)W * per), roffs, c->m_tmp.p, c->m_tmp_bytes, c->stream));
    const MergeRecv src{renc, rwords, roffs, per, W};
    tots = c->recv_totals.as<const int64_t>();
    HIPCHK(c, merge_decode(src, n, tots, tables(c), drows.dev, summ.dev, c->stream));
    KTimer kc(c, L5DH_K_COPY);  // (overlaps the MERGE scope above, which ends with this block)
    if ((r = summ.end(c)) || (r = drows.end(c))) return r;
    // (a plain copy, not staging: see below)
    if (totals_out) HIPCHK(c, hipMemcpyAsync(totals_out, tots, (size_t)n * 8, hipMemcpyDefault, c->stream));
    return sync_stream(c);
  }
  if (rs) {  // a 1-rank communicator, collective skipped: the exported rows are the sums
    c->m_dense_bytes = (uint64_t)per * (NB * 4 + 8);
    c->m_encoded_bytes = c->m_dense_bytes;
    c->m_sent_bytes = 0;
  }
  if (out) {
    KTimer kt(c, L5DH_K_HOT);
    HIPCHK(c, launch_rows(state(c), rows, tots, tables(c), Outputs{summ.dev, nullptr, 0, n, nullptr}, 0, nullptr,
                          c->stream));
  }
  {
    KTimer kt(c, L5DH_K_COPY);
    if ((r = summ.end(c))) return r;
    // (not staging: plain copies out of the engine's own merge buffers to wherever the
    // caller's pointers live)
    if (counts_out) HIPCHK(c, hipMemcpyAsync(counts_out, rows, (size_t)n * NB * 4, hipMemcpyDefault, c->stream));
    if (totals_out) HIPCHK(c, hipMemcpyAsync(totals_out, tots, (size_t)n * 8, hipMemcpyDefault, c->stream));
  }
  return sync_stream(c);
}

// The loopback group's collectives (l5dh_comm_init_loopback: n contexts on one device):
// the same encode / size / receive / payload steps as over RCCL, with each exchange
// done by device copies (all streams drained first) and the reductions by one kernel
// reading every rank's buffer.
int sync_all(l5dh_ctx** cs, int n) {
  for (int i = 0; i < n; ++i) HIPCHK(cs[i], hipStreamSynchronize(cs[i]->stream));
  return 0;
}

int loop_collectives(l5dh_ctx** cs, int n, int mode) {
  int r;
  const int W = n;
  const uint32_t per = merge_per(cs[0]);
  if (mode != L5DH_MERGE_REDUCE_SCATTER) {  // dense all-reduce: the sum into rank 0's rows, copied to the others
    const size_t Sp = (size_t)per * W;
    if ((r = sync_all(cs, n))) return r;
    std::vector<const int32_t*> rows(W);
    std::vector<const int64_t*> tots(W);
    for (int i = 0; i < W; ++i) {
      rows[i] = cs[i]->merge_counts.as<const int32_t>();
      tots[i] = cs[i]->merge_totals.as<const int64_t>();
    }
    l5dh_ctx* c0 = cs[0];
    HIPCHK(c0, merge_loop_sum_i32(rows.data(), W, c0->merge_counts.as<int32_t>(), Sp * NB, c0->stream));
    HIPCHK(c0, merge_loop_sum_i64(tots.data(), W, c0->merge_totals.as<int64_t>(), Sp, c0->stream));
    HIPCHK(c0, hipStreamSynchronize(c0->stream));
    for (int i = 1; i < W; ++i) {
      HIPCHK(cs[i], hipMemcpyAsync(cs[i]->merge_counts.p, c0->merge_counts.p, Sp * NB * 4, hipMemcpyDeviceToDevice,
                                   cs[i]->stream));
      HIPCHK(cs[i], hipMemcpyAsync(cs[i]->merge_totals.p, c0->merge_totals.p, Sp * 8, hipMemcpyDeviceToDevice,
                                   cs[i]->stream));
    }
    for (int i = 0; i < W; ++i) {
      cs[i]->m_dense_bytes = cs[i]->m_encoded_bytes = Sp * (NB * 4 + 8);
      cs[i]->m_sent_bytes = 2 * cs[i]->m_dense_bytes * (W - 1) / W;
    }
    return sync_all(cs, n);
  }
  if (merge_skips_collective(cs[0])) return 0;  // one rank: merge_finish's identity over the dense export
  for (int i = 0; i < n; ++i)
    if ((r = merge_pack_step(cs[i]))) return r;
  if ((r = sync_all(cs, n))) return r;
  {  // all-gather of the size rows: one copy launch per destination
    for (int j = 0; j < n; ++j) {
      LoopCopies l{};
      for (int i = 0; i < n; ++i)
        if (i != j) {
          l.src[l.n] = reinterpret_cast<const uint32_t*>(cs[i]->m_sizes.as<const uint64_t>() + (size_t)i * W);
          l.dst[l.n] = reinterpret_cast<uint32_t*>(cs[j]->m_sizes.as<uint64_t>() + (size_t)i * W);
          l.words[l.n++] = (uint64_t)W * 2;
        }
      HIPCHK(cs[j], merge_loop_copy(l, cs[j]->stream));
    }
  }
  for (int i = 0; i < n; ++i)
    if ((r = merge_recv_step(cs[i]))) return r;
  if ((r = sync_all(cs, n))) return r;
  for (int q = 0; q < W; ++q) {  // destination q receives every other source's slice q (one copy launch)
    l5dh_ctx* d = cs[q];
    uint64_t rat = 0;
    LoopCopies l{};
    for (int p = 0; p < W; ++p) {
      l5dh_ctx* sp = cs[p];
      if (p != q) {
        uint64_t at = 0;
        for (int k = 0; k < q; ++k) at += sp->m_to[k];
        if (sp->m_to[q]) {
          l.src[l.n] = sp->m_enc.as<const uint32_t>() + at;
          l.dst[l.n] = d->r_enc.as<uint32_t>() + rat;
          l.words[l.n++] = sp->m_to[q];
        }
        l.src[l.n] = sp->m_words.as<const uint32_t>() + (size_t)q * per;
        l.dst[l.n] = d->r_words.as<uint32_t>() + (size_t)p * per;
        l.words[l.n++] = per;
      }
      rat += d->m_from[p];
    }
    HIPCHK(d, merge_loop_copy(l, d->stream));
    std::vector<const int64_t*> tots(W);  // the totals' reduce-scatter: slice q summed over the sources
    for (int p = 0; p < W; ++p) tots[p] = cs[p]->merge_totals.as<const int64_t>() + (size_t)q * per;
    HIPCHK(d, merge_loop_sum_i64(tots.data(), W, d->recv_totals.as<int64_t>(), per, d->stream));
  }
  return sync_all(cs, n);
}

// The collective steps of one merge over contexts `cs` (one, or every context of an
// l5dh_comm_init_all communicator): each collective step is grouped over them.
int merge_collectives(l5dh_ctx** cs, int n, int mode) {
  if (cs[0]->loopback) return loop_collectives(cs, n, mode);
  int r = 0;
  if (mode != L5DH_MERGE_REDUCE_SCATTER) {
    NCCLCHK(cs[0], ncclGroupStart());
    for (int i = 0; i < n && !r; ++i) {
      hipSetDevice(cs[i]->device);
      if (!merge_skips_collective(cs[i])) r = merge_dense_allreduce(cs[i]);
    }
    const ncclResult_t ge = ncclGroupEnd();
    if (r) return r;
    return ge == ncclSuccess ? 0 : ncclfail(cs[0], ge, "ncclGroupEnd");
  }
  if (merge_skips_collective(cs[0])) return 0;
  for (int i = 0; i < n; ++i) {
    hipSetDevice(cs[i]->device);
    if ((r = merge_pack_step(cs[i]))) return r;
  }
  NCCLCHK(cs[0], ncclGroupStart());
  for (int i = 0; i < n && !r; ++i) {
    hipSetDevice(cs[i]->device);
    r = merge_sizes_step(cs[i]);
  }
  ncclResult_t ge = ncclGroupEnd();
  if (r) return r;
  if (ge != ncclSuccess) return ncclfail(cs[0], ge, "ncclGroupEnd");
  for (int i = 0; i < n; ++i) {
    hipSetDevice(cs[i]->device);
    if ((r = merge_recv_step(cs[i]))) return r;
  }
  NCCLCHK(cs[0], ncclGroupStart());
  for (int i = 0; i < n && !r; ++i) {
    hipSetDevice(cs[i]->device);
    r = merge_payload_step(cs[i]);
  }
  ge = ncclGroupEnd();
  if (r) return r;
  return ge == ncclSuccess ? 0 : ncclfail(cs[0], ge, "ncclGroupEnd");
}

}  // namespace

extern "C" {

int l5dh_comm_unique_id(void* id_out) {
  if (!id_out) return -EINVAL;
  static_assert(sizeof(ncclUniqueId) == L5DH_UNIQUE_ID_BYTES, "unique id size");
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return -EIO;
  memcpy(id_out, &id, sizeof(id));
  return 0;
}

int l5dh_comm_init_rank(l5dh_ctx* c, const void* id, int nranks, int rank) {
  if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return -EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  if (c->comm || c->loopback) return fail(c, -EINVAL, "context already has a communicator");
  // (the sparse reduce-scatter holds one source per rank: checked before any merge runs)
  if (nranks > MERGE_MAX_RANKS) return fail(c, -EINVAL, "fleet merge: more than 64 ranks");
  hipSetDevice(c->device);
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof(uid));
  ncclComm_t comm = nullptr;
  NCCLCHK(c, ncclCommInitRank(&comm, nranks, uid, rank));
  c->comm = comm;
  c->nranks = nranks;
  c->rank = rank;
  return 0;
}

int l5dh_comm_init_all(l5dh_ctx** ctxs, int n) {
  if (!ctxs || n < 1 || n > MERGE_MAX_RANKS) return -EINVAL;
  std::vector<int> devs(n);
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i] || ctxs[i]->comm || ctxs[i]->loopback || ctxs[i]->S != ctxs[0]->S) return -EINVAL;
    devs[i] = ctxs[i]->device;
  }
  std::vector<ncclComm_t> comms(n, nullptr);
  const ncclResult_t e = ncclCommInitAll(comms.data(), n, devs.data());
  if (e != ncclSuccess) {
    ctxs[0]->last_error = std::string("ncclCommInitAll: ") + ncclGetErrorString(e);
    return -EIO;
  }
  for (int i = 0; i < n; ++i) {
    std::lock_guard<std::mutex> g(ctxs[i]->mu);
    ctxs[i]->comm = comms[i];
    ctxs[i]->nranks = n;
    ctxs[i]->rank = i;
  }
  return 0;
}

int l5dh_comm_init_loopback(l5dh_ctx** ctxs, int n) {
  if (!ctxs || n < 1 || n > MERGE_MAX_RANKS) return -EINVAL;
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i] || ctxs[i]->comm || ctxs[i]->loopback || ctxs[i]->S != ctxs[0]->S ||
        ctxs[i]->device != ctxs[0]->device)
      return -EINVAL;
    for (int j = 0; j < i; ++j)
      if (ctxs[j] == ctxs[i]) return -EINVAL;
  }
  for (int i = 0; i < n; ++i) {
    std::lock_guard<std::mutex> g(ctxs[i]->mu);
    ctxs[i]->loopback = true;
    ctxs[i]->nranks = n;
    ctxs[i]->rank = i;
  }
  return 0;
}

int l5dh_comm_destroy(l5dh_ctx* c) {
  if (!c) return -EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  if (c->comm) {
    hipSetDevice(c->device);
    int r = sync_stream(c);
    if (r) return r;
    ncclCommDestroy(c->comm);
  }
  c->loopback = false;
  c->comm = nullptr;
  c->nranks = 1;
  c->rank = 0;
  return 0;
}

int l5dh_merge(l5dh_ctx* c, int mode, l5dh_summary* out, int32_t* counts_out, int64_t* totals_out, uint32_t* first,
               uint32_t* count) {
  if (!c || (mode != L5DH_MERGE_REDUCE_SCATTER && mode != L5DH_MERGE_ALL_REDUCE)) return -EINVAL;
  CtxLock g(c);
  if (c->loopback) return fail(c, -EINVAL, "a loopback group merges through l5dh_merge_all");
  int r;
  if ((r = merge_export(c, mode))) return r;
  if ((r = merge_collectives(&c, 1, mode))) return r;
  return merge_finish(c, mode, out, counts_out, totals_out, first, count);
}

int l5dh_merge_all(l5dh_ctx** ctxs, int n, int mode, l5dh_summary** outs, int32_t** counts_outs, int64_t** totals_outs,
                   uint32_t* firsts, uint32_t* counts) {
  if (!ctxs || n < 1 || (mode != L5DH_MERGE_REDUCE_SCATTER && mode != L5DH_MERGE_ALL_REDUCE)) return -EINVAL;
  for (int i = 0; i < n; ++i)
    if (!ctxs[i] || !(ctxs[i]->comm || ctxs[i]->loopback) || ctxs[i]->loopback != ctxs[0]->loopback ||
        ctxs[i]->nranks != n || ctxs[i]->rank != i)
      return -EINVAL;
  std::vector<std::unique_lock<std::mutex>> locks;
  for (int i = 0; i < n; ++i) locks.emplace_back(ctxs[i]->mu);  // in rank order
  int r;
  for (int i = 0; i < n; ++i) {
    hipSetDevice(ctxs[i]->device);
    if ((r = merge_export(ctxs[i], mode))) return r;
  }
  if ((r = merge_collectives(ctxs, n, mode))) return r;
  for (int i = 0; i < n; ++i) {
    hipSetDevice(ctxs[i]->device);
    if ((r = merge_finish(ctxs[i], mode, outs ? outs[i] : nullptr, counts_outs ? counts_outs[i] : nullptr,
                          totals_outs ? totals_outs[i] : nullptr, firsts ? firsts + i : nullptr,
                          counts ? counts + i : nullptr)))
      return r;
  }
  return 0;
}

int l5dh_merge_bytes(l5dh_ctx* c, uint64_t* dense, uint64_t* encoded, uint64_t* sent) {
  if (!c) return -EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  if (dense) *dense = c->m_dense_bytes;
  if (encoded) *encoded = c->m_encoded_bytes;
  if (sent) *sent = c->m_sent_bytes;
  return 0;
}

}  // extern "C"
