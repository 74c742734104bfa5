// loik_devmem.hpp -- the one owner of device and pinned host memory (host only; includes no HIP).
//
// The rule of the host layer:
//   * a buffer that lives exactly as long as the handle and never changes size is an arena allocation (alloc_dev) behind a raw
//     typed pointer;
//   * every other owned buffer -- one that is freed, replaced or regrown before the handle goes -- is an OwnedBuf member
//     (DevBuf<T> / PinBuf<T> in loik_host.hip) of the struct that uses it.
// Nothing is freed by naming it in loikb_destroy: a member frees itself when its struct goes.
//
// Policy: static bool allocate(void** out, size_t bytes)   -- false: nothing was allocated
//         static void free(void* p, size_t bytes)          -- bytes: what allocate was given for p (the policies count live bytes)
//
// regrow  frees first, then allocates: the only order that fits for a buffer of gigabytes.  A failure leaves the buffer empty.
// replace allocates first, then frees: a failure leaves the old buffer, its size and its contents as they were.
// Neither keeps the contents across a growth, and neither ever shrinks a buffer.
#pragma once
#include <cstddef>

namespace loikb {

template <class Policy, class T = void>
class OwnedBuf {
 public:
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  OwnedBuf(OwnedBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept
  {
    if (this != &o) { release(); swap(o); }
    return *this;
  }
  ~OwnedBuf() { release(); }

  // a launch site names the member as it named the raw pointer; a buffer of another element type is read through as<U>()
  operator T*() const { return static_cast<T*>(p_); }
  template <class U> U* as() const { return static_cast<U*>(p_); }
  size_t bytes() const { return bytes_; }

  bool regrow(size_t bytes)
  {
    if (bytes <= bytes_) return true;
    release();
    if (!Policy::allocate(&p_, bytes)) { p_ = nullptr; return false; }
    bytes_ = bytes;
    return true;
  }
  bool replace(size_t bytes)
  {
    if (bytes <= bytes_) return true;
    void* p = nullptr;
    if (!Policy::allocate(&p, bytes)) return false;
    release();
    p_ = p; bytes_ = bytes;
    return true;
  }
  // frees the buffer; returns the bytes freed (0: it was empty)
  size_t release()
  {
    const size_t freed = bytes_;
    if (p_) Policy::free(p_, bytes_);
    p_ = nullptr; bytes_ = 0;
    return freed;
  }
  void swap(OwnedBuf& o) noexcept
  {
    void* p = p_; p_ = o.p_; o.p_ = p;
    const size_t n = bytes_; bytes_ = o.bytes_; o.bytes_ = n;
  }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

}  // namespace loikb
