// request_batch.h — what the batch-of-requests verbs share (tas_request_batch.hip,
// gas_fit_requests.hip): the requests arrive as a CSR whose offsets are a host array.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pas_internal.h"

namespace pas {

// S: the longest request the batched prioritize sorts in one workgroup's LDS; longer ones
// take the single-request path.
constexpr int kRequestCap = 2048;

// The longest request of the batch.
int32_t request_longest(int32_t n_requests, const int32_t* req_off);
// gridDim.y of the one-lane-per-position kernels (gridDim.x = the requests): workgroups of
// `tpb` positions over the longest request, at most 65 535 (the kernels stride past that).
unsigned request_chunks(int32_t longest, int tpb);
// A host array copied to the device on s; wait: and waited for, so that the array may change
// when the call returns (else the caller keeps it until it has synchronized s).
int upload_host(pas_ctx* ctx, void* dst, const void* src, size_t bytes, bool wait,
                hipStream_t s);

}  // namespace pas
