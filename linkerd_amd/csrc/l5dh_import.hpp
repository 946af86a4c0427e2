// l5dh_import.hpp -- state import (dense and sparse rows) and the public sparse export
// (l5dh_import.hip): the way INTO the bucket rows, and the CSR form of the way out.
#pragma once

#include "l5dh_kernels.hpp"

namespace l5dh {

struct BucketEntry {  // = l5dh_bucket_entry: one non-empty bucket of a row
  uint32_t bucket, count;
};
static_assert(sizeof(BucketEntry) == 8, "l5dh_bucket_entry layout");

// Status words of an import (u32, on the device; the host reads them in one copy):
// the least offender each, IS_NONE while there is none.
enum : uint32_t {
  IS_BAD = 0,     // an input outside the domain: the least series (dense) / row (sparse)
  IS_RANGE = 1,   // a bucket sum above 2^31 - 1: the least series
  IS_NCLEAN = 2,  // clean tiles the sparse rows touch (the zero pass' list length)
  IS_WORDS = 4
};
constexpr uint32_t IS_NONE = 0xFFFFFFFFu;
// IS_BAD = IS_RANGE = IS_NONE, IS_NCLEAN = 0
hipError_t import_status_init(uint32_t* status, hipStream_t st);

// Dense rows ext[count][1798] (+ ext_total, nullable: 0) into series [first, first + count).
// One wave per series of the range widened to tile boundaries: in a clean tile the imported
// rows are stored and every other row zeroed (total likewise), in a dirty one the imported
// rows are read, added and written; then, in a second launch, the range's tiles are marked
// dirty.  A count above 2^31 - 1 (a negative int32) lowers status[IS_BAD], a bucket sum
// above 2^31 - 1 status[IS_RANGE], to the least such series; the rows are written all the
// same (modulo 2^32), and import_dense_undo takes exactly them out again.
hipError_t import_dense(State state, uint32_t first, uint32_t count, const int32_t* ext, const int64_t* ext_total,
                        uint32_t* status, hipStream_t st);
hipError_t import_dense_undo(State state, uint32_t first, uint32_t count, const int32_t* ext,
                             const int64_t* ext_total, hipStream_t st);

// CSR rows: row i (entries[row_off[i] .. row_off[i + 1])) belongs to series[i] (series ==
// nullptr: first + i).  n <= S rows, n_entries = row_off[n] as the host read it.
struct SparseRows {
  const uint32_t* series;
  uint32_t first, n;
  const uint64_t* row_off;
  const BucketEntry* entries;  // (nullptr: import_sparse_check reads the offsets and ids only)
  const int64_t* totals;       // nullable: 0
  uint64_t n_entries;
};
// Reads only.  status[IS_BAD] = the least row with: an offset that descends, passes
// n_entries or (row 0) does not start at 0; more than 1798 entries; a bucket >= 1798; buckets
// not strictly ascending; a count above 2^31 - 1; a series id >= S or not above its
// predecessor's.  A row whose offsets are wrong has none of its entries read.
hipError_t import_sparse_check(SparseRows rows, uint32_t S, uint32_t* status, hipStream_t st);
// Checked rows into the state: the clean tiles they touch are listed (tflag [F] and list [F]
// are scratch) and zeroed whole, rows and totals; every entry is a read-add-write of its
// bucket (no two entries share an address); the touched tiles are marked dirty in a last
// launch.  status[IS_RANGE] as in import_dense; import_sparse_undo subtracts the same entries.
hipError_t import_sparse(State state, SparseRows rows, uint32_t* tflag, uint32_t* list, uint32_t* status,
                         hipStream_t st);
hipError_t import_sparse_undo(State state, SparseRows rows, hipStream_t st);

// Sparse export of the state rows of series [first, first + count) (folded state):
// export_sparse_count writes each row's non-empty buckets to rowcnt[i] (a row of a clean tile:
// 0, not read); after the exclusive scan of rowcnt into offs (merge_count),
// export_sparse_write places row i's entries at entries[offs[i] ..) in ascending bucket
// order and its exact sum in totals[i] (nullable).
hipError_t export_sparse_count(State state, uint32_t first, uint32_t count, uint32_t* rowcnt, hipStream_t st);
hipError_t export_sparse_write(State state, uint32_t first, uint32_t count, const uint64_t* offs,
                               BucketEntry* entries, int64_t* totals, hipStream_t st);

}  // namespace l5dh
