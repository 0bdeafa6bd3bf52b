// host_staging.h — the arrays of one host-pointer entry point in the context's scratch (every
// file with host forms: pas_api.hip, tas_ingest.hip, name_table.hip, span_pool.hip,
// gas_cards.hip, gas_annotations.hip, gas_node_strings.hip, gas_render.hip; the _device forms
// and the _launch functions stage nothing).
#pragma once

#include <algorithm>
#include <cassert>

#include "pas_internal.h"

namespace pas {

// A host form states each array once: in (uploaded), out (fetched) or work (device only), with
// the caller's device pointer, the host pointer and the element count.  upload() then sizes
// ctx->scratch for all of them (ensure_scratch may free and reallocate, so the device pointers
// are only filled in here), lays them out in declaration order, each rounded up to 256 bytes,
// and copies the inputs; fetch() copies the outputs and synchronizes ctx->stream.  A copy is
// skipped when its byte count is 0 or its host pointer is null, and in no other case.  Every
// stated array gets a device pointer of its own, even at count 0 (at least 256 bytes);
// in_opt / out_opt state an optional argument, whose device pointer is null when the host
// pointer is (what the _launch functions read as "not given").  No heap allocation per call.
class Staging {
 public:
  explicit Staging(pas_ctx* ctx) : ctx_(ctx) {}
  pas_ctx* ctx() const { return ctx_; }
  template <typename T>
  void in(T*& d, const T* host, size_t count) { add(&d, host, count, kIn, false); }
  template <typename T>
  void in_opt(T*& d, const T* host, size_t count) { add(&d, host, count, kIn, true); }
  template <typename T>  // (a record's read-only field)
  void in(const T*& d, const T* host, size_t count) {
    add(const_cast<T**>(&d), host, count, kIn, false);
  }
  template <typename T>
  void out(T*& d, T* host, size_t count) { add(&d, host, count, kOut, false); }
  template <typename T>
  void out_opt(T*& d, T* host, size_t count) { add(&d, host, count, kOut, true); }
  template <typename T>
  void work(T*& d, size_t count) { add(&d, static_cast<const T*>(nullptr), count, kWork, false); }
  // The n byte spans of a host form (checked: check_host_spans), two arrays: d gets the byte
  // total now and the device pointers at upload().  n == 0 states both arrays empty.
  void in_spans(ByteSpans& d, int64_t n, const int64_t* off, const char* bytes) {
    d.n_bytes = n > 0 ? off[n] : 0;
    in(d.off, off, n > 0 ? (size_t)n + 1 : 0);
    in(d.bytes, bytes, (size_t)d.n_bytes);
  }

  int upload() {
    size_t total = 0;
    for (int i = 0; i < n_; ++i) total += room(buf_[i]);
    if (int rc = ensure_scratch(ctx_, total)) return rc;
    char* p = static_cast<char*>(ctx_->scratch);
    for (int i = 0; i < n_; ++i) {
      *buf_[i].dev = room(buf_[i]) ? p : nullptr;
      p += room(buf_[i]);
    }
    for (int i = 0; i < n_; ++i)
      if (const Buf& b = buf_[i]; b.role == kIn && b.bytes && b.host)
        PAS_HIP(ctx_, hipMemcpyAsync(*b.dev, b.host, b.bytes, hipMemcpyHostToDevice, ctx_->stream));
    return PAS_OK;
  }

  // The first error of the output copies (in the order stated) and the synchronize; a failed
  // copy ends the copies, not the synchronize (the earlier ones write the caller's arrays).
  hipError_t fetch() {
    hipError_t e = hipSuccess;
    for (int i = 0; i < n_ && e == hipSuccess; ++i)
      if (const Buf& b = buf_[i]; b.role == kOut && b.bytes && b.host)
        e = hipMemcpyAsync(const_cast<void*>(b.host), *b.dev, b.bytes, hipMemcpyDeviceToHost,
                           ctx_->stream);
    const hipError_t es = hipStreamSynchronize(ctx_->stream);
    return e != hipSuccess ? e : es;
  }
  // fetch() as a status, for the forms whose results are the last thing that can fail
  int fetch_results(const std::string& fn) {
    const hipError_t e = fetch();
    return e == hipSuccess ? PAS_OK : check_hip(ctx_, e, (fn + ": copy of the results").c_str());
  }

 private:
  enum Role { kIn, kOut, kWork };
  struct Buf {
    void** dev;
    const void* host;
    size_t bytes;
    Role role;
    bool opt;
  };
  static size_t room(const Buf& b) {  // 0: an optional array that was not given
    return b.opt && !b.host ? 0 : (std::max(b.bytes, size_t(1)) + 255) & ~size_t(255);
  }
  template <typename T>
  void add(T** d, const T* host, size_t count, Role role, bool opt) {
    assert(n_ < kMax);
    buf_[n_++] = Buf{reinterpret_cast<void**>(d), host, sizeof(T) * count, role, opt};
  }
  static constexpr int kMax = 16;
  pas_ctx* ctx_;
  Buf buf_[kMax];
  int n_ = 0;
};

// The pod batch of a GAS host form stated to st (three arrays): req [P][C][Q], req_mask [P][C]
// and n_containers [P].
inline void stage_pods(Staging& st, PodBatch& d, int32_t n_pods, int32_t max_containers,
                       const int64_t* req, const uint32_t* req_mask,
                       const int32_t* n_containers) {
  const size_t P = (size_t)n_pods, C = (size_t)max_containers;
  d.n_pods = n_pods;
  d.max_containers = max_containers;
  st.in(d.req, req, P * C * (size_t)st.ctx()->gas.n_res);
  st.in(d.mask, req_mask, P * C);
  st.in(d.n_containers, n_containers, P);
}

}  // namespace pas
