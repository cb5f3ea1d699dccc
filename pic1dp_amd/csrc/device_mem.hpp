// device_mem.hpp -- DeviceMem, the one owner of a CONTEXT's device and pinned host memory (pic1dp_ctx::mem): every
// allocation is recorded where it is made -- at create() or lazily, in whichever unit -- and destroy() releases them all
// in one call.  The context's members stay raw pointers (the kernel argument structs copy them).
// tests/test_device_mem_host.py holds every other allocation of the product against a short list of named exceptions.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace pic1dp_host {

class DeviceMem {
 public:
  DeviceMem() = default;
  DeviceMem(const DeviceMem &) = delete;
  DeviceMem &operator=(const DeviceMem &) = delete;
  ~DeviceMem() { release_all(); }

  // *slot <- n elements of device memory / of pinned host memory (uninitialised)
  template <class T>
  hipError_t alloc(T **slot, size_t n) { return take(reinterpret_cast<void **>(slot), sizeof(T) * n, false); }
  template <class T>
  hipError_t alloc_pinned(T **slot, size_t n) { return take(reinterpret_cast<void **>(slot), sizeof(T) * n, true); }
  // a grow-only buffer gets a new size: the old one (device or pinned, as it was allocated; may be null) is freed first
  template <class T>
  hipError_t regrow(T **slot, size_t n, bool pinned = false) {
    for (size_t i = 0; i < held.size(); ++i)
      if (held[i].p == static_cast<void *>(*slot)) {
        free_one(held[i]);
        held.erase(held.begin() + static_cast<long>(i));
        break;
      }
    *slot = nullptr;
    return take(reinterpret_cast<void **>(slot), sizeof(T) * n, pinned);
  }
  // a buffer that lives for one call (capi_select.cpp: a selection's result, a gather's indices) goes back before the call
  // returns: freed, forgotten, *slot null.  The standing allocation of the context is what it was before the call.
  template <class T>
  void release(T **slot) {
    for (size_t i = 0; i < held.size(); ++i)
      if (held[i].p == static_cast<void *>(*slot)) {
        free_one(held[i]);
        held.erase(held.begin() + static_cast<long>(i));
        break;
      }
    *slot = nullptr;
  }
  // device memory allocated elsewhere (hipMalloc) becomes this owner's
  void adopt(void *p) {
    if (p) held.push_back(Held{p, false});
  }
  // everything (the device whose memory this is must be current)
  void release_all() {
    for (size_t i = held.size(); i-- > 0;) free_one(held[i]);
    held.clear();
  }

 private:
  struct Held {
    void *p;
    bool pinned;
  };
  std::vector<Held> held;
  static void free_one(const Held &h) {
    if (h.pinned)
      (void)hipHostFree(h.p);
    else
      (void)hipFree(h.p);
  }
  hipError_t take(void **slot, size_t bytes, bool pinned) {
    void *p = nullptr;
    const hipError_t e = pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
    held.push_back(Held{p, pinned});
    *slot = p;
    return hipSuccess;
  }
};

}  // namespace pic1dp_host
