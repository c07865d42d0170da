// agx_mem.hpp -- owners of device and pinned host memory.
//
// Buf<T, Backend> holds n elements of T from a backend that supplies
//   error, ok                          the error type and its success value
//   alloc(void**, size_t bytes)        -> error
//   free(void*)
//   copy_in(void* dst, const void* src, size_t bytes) -> error   (from pageable host memory)
// It is move-only; what it holds is freed by reset(), by the next alloc() and by the
// destructor.  The template names nothing of HIP (tests/cpp/host_mem.cpp instantiates it
// over malloc / free); the two backends of the library follow under __HIPCC__.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

namespace agx {

template <class T, class Backend>
class Buf {
 public:
  using error = typename Backend::error;
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_; n_ = o.n_;
      o.p_ = nullptr; o.n_ = 0;
    }
    return *this;
  }
  ~Buf() { reset(); }

  void reset() {
    if (p_) Backend::free(p_);
    p_ = nullptr; n_ = 0;
  }
  // frees what is held, then n elements (uninitialised); empty if the backend fails
  error alloc(size_t n) {
    reset();
    void* p = nullptr;
    const error e = Backend::alloc(&p, sizeof(T) * n);
    if (e == Backend::ok) { p_ = static_cast<T*>(p); n_ = n; }
    return e;
  }
  // at least n elements: grows only (the contents are not kept); *grew: it reallocated
  error reserve(size_t n, bool* grew) {
    *grew = n > n_;
    return *grew ? alloc(n) : Backend::ok;
  }
  // n elements copied from the host; n == 0 leaves the owner empty
  error upload(const T* src, size_t n) {
    if (n == 0) { reset(); return Backend::ok; }
    const error e = alloc(n);
    return e == Backend::ok ? Backend::copy_in(p_, src, sizeof(T) * n) : e;
  }
  error upload(const std::vector<T>& v) { return upload(v.data(), v.size()); }

  T* get() const { return p_; }
  size_t size() const { return n_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

}  // namespace agx

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
namespace agx {
struct DevMem {
  using error = hipError_t;
  static constexpr error ok = hipSuccess;
  static error alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
  static error copy_in(void* dst, const void* src, size_t bytes) {
    return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
  }
};
struct PinnedMem {
  using error = hipError_t;
  static constexpr error ok = hipSuccess;
  static error alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes); }
  static void free(void* p) { (void)hipHostFree(p); }
  static error copy_in(void* dst, const void* src, size_t bytes) {
    memcpy(dst, src, bytes);
    return hipSuccess;
  }
};
template <class T> using DevBuf = Buf<T, DevMem>;
template <class T> using PinnedBuf = Buf<T, PinnedMem>;
}  // namespace agx
#endif
