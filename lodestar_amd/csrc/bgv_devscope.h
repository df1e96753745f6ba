// DevScope: the owner of a one-shot call's device memory ("allocate some buffers, enqueue on one
// stream, read back, free").  Host-only; it reaches the device through its policy alone, so it
// compiles without the HIP headers when given another policy (tests/native/devscopesim.cpp).
//
//   * a buffer from alloc() is freed exactly once when the scope ends, on every path, in
//     allocation order;
//   * before the first free, and before the function returns, the stream is drained: the work
//     queued on it may still read host memory of the function, write the caller's output or use
//     the buffers.  On the success path the function's own sync() (whose status it returns) is
//     that drain and no second one is issued; on a failure path the destructor drains and
//     ignores the status;
//   * sync() leaves the scope drained and no longer guarding: a function that queues more work
//     after it says so with enqueued() (a chunk loop, a second phase), or the destructor frees
//     without a drain;
//   * release() hands a buffer out of the scope (it was committed to longer-lived state).
#pragma once
#include <stddef.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "../../include/blsgpu.h"

// The default policy: hipMalloc, hipFree, hipStreamSynchronize (defined in bgv_ctx.h).  A policy
// has a stream_t and three static functions: bool alloc(void**, size_t bytes), void free(void*),
// bool sync(stream_t).
struct HipDevApi;

template <class Api = HipDevApi>
class DevScope {
 public:
  using stream_t = typename Api::stream_t;
  explicit DevScope(stream_t stream) : stream_(stream) {}
  DevScope(const DevScope&) = delete;
  DevScope& operator=(const DevScope&) = delete;
  ~DevScope() {
    // pending work matters when something it may touch is about to go away
    if (pending_ && (guard_ || !bufs_.empty())) (void)Api::sync(stream_);
    for (void* p : bufs_) Api::free(p);
  }

  // count elements of T (bytes for a void pointer); BGV_OK or -BGV_E_DEVICE (*p is null then)
  template <class T>
  int alloc(T** p, size_t count) {
    using E = std::conditional_t<std::is_void<T>::value, char, T>;
    void* q = nullptr;
    *p = nullptr;
    if (!Api::alloc(&q, count * sizeof(E))) return -BGV_E_DEVICE;
    bufs_.push_back(q);
    pending_ = true;  // the caller is about to queue work on it
    *p = static_cast<T*>(q);
    return BGV_OK;
  }

  // Work was queued that the scope cannot know of: after a sync(), or on host memory of the
  // function while the scope owns no buffer.  The scope drains the stream even with nothing to free.
  void enqueued() { pending_ = guard_ = true; }

  // The function's explicit synchronize; its status is the call's.
  int sync() {
    const bool ok = Api::sync(stream_);
    pending_ = false;
    return ok ? BGV_OK : -BGV_E_DEVICE;
  }

  // Another owner of the same stream synchronized it since this scope's last alloc() / enqueued().
  void drained() { pending_ = false; }

  template <class T>
  T* release(T* p) {
    bufs_.erase(std::remove(bufs_.begin(), bufs_.end(), static_cast<void*>(p)), bufs_.end());
    return p;
  }

 private:
  stream_t stream_;
  std::vector<void*> bufs_;
  bool pending_ = false, guard_ = false;
};
