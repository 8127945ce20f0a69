// long_records.hpp -- the host side of the record launches: the record engine, with the batch's
// long records on the sequence-parallel tiles (segments.hip) when long_route.hpp says so.
#pragma once

#include "enet_crypto.h"
#include "enet_internal.hpp"

namespace enet {

// Both set the text enet_last_error() returns on this thread (capi.cpp owns it) and give the
// ABI's return code; hip_status clears the text on hipSuccess.
int fail(int code, const char* what);
int hip_status(hipError_t e, const char* what);

inline bool hints_uniform(const enet_records* r) { return hints_uniform(r->count, r->max_len_hint, r->total_bytes_hint); }

hipMemPool_t scratch_pool();      // the current device's library-private pool (nullptr: none)
void set_seg_min(int64_t bytes);  // enet_set_seg_min, argument checked
uint64_t seg_batches();           // enet_seg_batches

// The record engine over the batch, with its long records on the tiles first where
// choose_long_route wants them.  r->order may name any r->count records of a larger batch: the
// tiles' claim bytes are kept per position of the launch, not per record index, so no bound on
// the indices is needed (or known: the order is device memory, and this call does not synchronise).
int run_records(int mode, const enet_records* r, RecParams& p, hipStream_t st, const char* what);

}  // namespace enet
