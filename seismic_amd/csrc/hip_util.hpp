// hip_util.hpp — what the launchers in the .hip files share: the HIP error check, a grow-only device buffer, the
// per-replica state made on first use, and what the other files see of device_index.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "device_types.hpp"
#include "host_index.hpp"

namespace sgpu {

#define HIP_TRY(expr)                                                                                         \
  do {                                                                                                        \
    hipError_t e_ = (expr);                                                                                   \
    if (e_ != hipSuccess)                                                                                     \
      return fail(SGPU_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// device_index.hip: the device a replica lives on and its index as the kernels see it
int device_index_device(const DeviceIndex* d);
const DevView& device_index_view(const DeviceIndex* d);

// Device memory that is recycled from call to call and only ever grows.
struct DeviceBuffer {
  void* p = nullptr;
  uint64_t bytes = 0;

  template <class T>
  T* as() const { return static_cast<T*>(p); }
  // At least `want` bytes (never fewer than 16). A buffer that is too small is freed first, after `stream` - where the
  // work that may still use it was enqueued - has been synchronised. `what` names the use in the SGPU_ENOMEM message.
  sgpu_status reserve(hipStream_t stream, uint64_t want, const char* what) {
    if (p && bytes >= want) return SGPU_OK;
    if (p) {
      (void)hipStreamSynchronize(stream);
      release();
    }
    want = std::max<uint64_t>(want, 16);
    if (hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return fail(SGPU_ENOMEM, "out of device memory %s (%llu bytes)", what, (unsigned long long)want);
    }
    bytes = want;
    return SGPU_OK;
  }
  void release() {   // (the caller has synchronised whatever used it)
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// The state of type T that `replica` keeps in `slots` (one pointer per replica, null until its first use), made under
// `mu` on first use: init(T*, device) fills a new T, free_state(T*) takes a half-made one back - the error it failed
// with stays the thread's last error. SGPU_EDEVICE: not uploaded / no such replica.
template <class T, class Init, class Free>
sgpu_status replica_state(sgpu_index* idx, std::mutex& mu, std::vector<T*>& slots, uint32_t replica, Init init, Free free_state,
                          T** out) {
  std::lock_guard<std::mutex> lk(mu);
  if (replica >= idx->replicas.size())
    return fail(SGPU_EDEVICE, "index is not uploaded to a device (call sgpu_index_upload) / replica out of range");
  if (slots.size() != idx->replicas.size()) slots.resize(idx->replicas.size(), nullptr);
  if (!slots[replica]) {
    T* fresh = new (std::nothrow) T();
    if (!fresh) return fail(SGPU_ENOMEM, "out of host memory");
    sgpu_status st;
    try {
      st = init(fresh, device_index_device(idx->replicas[replica]));
    } catch (const std::bad_alloc&) {
      st = fail(SGPU_ENOMEM, "out of host memory");
    }
    if (st != SGPU_OK) {
      const std::string msg = last_error();
      free_state(fresh);
      last_error() = msg;
      return st;
    }
    slots[replica] = fresh;
  }
  *out = slots[replica];
  return SGPU_OK;
}

}  // namespace sgpu
