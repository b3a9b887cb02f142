// dev_mem.hpp — the one owner of a handle's device memory.  Plain C++17, no HIP include: the four
// functions below are the only way to the allocator, defined once in abi.hip (hipMalloc / hipFree / hipHostMalloc /
// hipHostFree, and the process-wide counters rl_debug_device_memory reads) — a test links its own over malloc.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

void *rl_device_alloc(uint64_t bytes);             // throws when the allocation fails
void rl_device_free(void *p, uint64_t bytes);      // `bytes` as allocated; never throws
void *rl_host_alloc(uint64_t bytes, bool mapped);  // pinned host memory; `mapped`: visible to the device as well
void rl_host_free(void *p);

// Every pointer DevMem hands out is a plain T*: what the kernel-visible structs (TrajDev, EnvStateDev, ReplayDev, the
// *Args structs) hold are views, and a view that points elsewhere — into the middle of a buffer, into another owner's
// memory — is nobody's to free.  The destructor frees what was allocated here and nothing else.
class DevMem {
 public:
  DevMem() = default;
  DevMem(DevMem &&o) noexcept : recs_(std::move(o.recs_)) { o.recs_.clear(); }
  DevMem &operator=(DevMem &&o) noexcept {
    if (this != &o) {
      clear();
      recs_ = std::move(o.recs_);
      o.recs_.clear();
    }
    return *this;
  }
  DevMem(const DevMem &) = delete;
  DevMem &operator=(const DevMem &) = delete;
  ~DevMem() { clear(); }

  // `count` elements of device memory (0 counts as 1: never a null result)
  template <class T>
  T *alloc(uint64_t count) {
    return static_cast<T *>(record(DEVICE, (count ? count : 1) * sizeof(T)));
  }
  // ... of pinned host memory
  template <class T>
  T *alloc_host(uint64_t count, bool mapped) {
    return static_cast<T *>(record(mapped ? HOST_MAPPED : HOST, (count ? count : 1) * sizeof(T)));
  }
  // Grow-only: nothing happens while `p` holds `count` elements (a null `p` holds none).  Otherwise `p` is freed and
  // nulled BEFORE the new allocation: when that throws, `p` is null and unrecorded, and the next call starts afresh.
  // Contents are not kept.  Returns whether it reallocated.
  template <class T>
  bool ensure(T *&p, uint64_t count) {
    if (count_of(p) >= count) return false;
    release(p);
    p = alloc<T>(count);
    return true;
  }
  // elements behind a pointer allocated here; 0 for null and for pointers this owner does not know
  template <class T>
  uint64_t count_of(const T *p) const {
    const Rec *r = find(p);
    return r ? r->bytes / sizeof(T) : 0;
  }
  // frees `p` if it was allocated here, and nulls it either way
  template <class T>
  void release(T *&p) {
    if (const Rec *r = find(p)) {
      free_rec(*r);
      recs_.erase(recs_.begin() + (r - recs_.data()));
    }
    p = nullptr;
  }

 private:
  enum Kind : uint8_t { DEVICE, HOST, HOST_MAPPED };
  struct Rec {
    void *p;
    uint64_t bytes;
    Kind kind;
  };
  std::vector<Rec> recs_;

  const Rec *find(const void *p) const {
    if (p != nullptr)
      for (const Rec &r : recs_)
        if (r.p == p) return &r;
    return nullptr;
  }
  void *record(Kind kind, uint64_t bytes) {
    recs_.push_back(Rec{nullptr, bytes, kind});  // (the record first: a push_back failing after the allocation loses it)
    try {
      recs_.back().p = kind == DEVICE ? rl_device_alloc(bytes) : rl_host_alloc(bytes, kind == HOST_MAPPED);
    } catch (...) {
      recs_.pop_back();
      throw;
    }
    return recs_.back().p;
  }
  static void free_rec(const Rec &r) {
    if (r.kind == DEVICE) rl_device_free(r.p, r.bytes);
    else rl_host_free(r.p);
  }
  void clear() {
    for (const Rec &r : recs_) free_rec(r);
    recs_.clear();
  }
};
