// The one owner of device memory in libtsearch: a move-only buffer that knows its size in bytes and whether the pointer is
// its own.  Nothing from HIP: the allocator is the policy `Mem` (host.h supplies the HIP one and the alias DevArray<T>), so
// tests/dev_array_check.cpp runs all of it on the CPU, over malloc, under the host sanitizers.
//   Mem::alloc(void** p, size_t bytes) -> 0 or a failure code;  Mem::free(void* p);  Mem::zero(void* p, size_t bytes) -> 0 or a code
#pragma once
#include <cstddef>

namespace ts {

template <class T, class Mem>
class DevArrayOf {
    T* p_ = nullptr;
    size_t bytes_ = 0;
    bool owned_ = false;

public:
    DevArrayOf() = default;
    DevArrayOf(const DevArrayOf&) = delete;
    DevArrayOf& operator=(const DevArrayOf&) = delete;
    DevArrayOf(DevArrayOf&& o) noexcept : p_(o.p_), bytes_(o.bytes_), owned_(o.owned_) { o.drop(); }
    DevArrayOf& operator=(DevArrayOf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; bytes_ = o.bytes_; owned_ = o.owned_;
            o.drop();
        }
        return *this;
    }
    ~DevArrayOf() { reset(); }

    operator T*() const { return p_; }
    template <class U> U* as() const { return (U*)p_; }      // for byte offsets and the kernels' own element types
    size_t bytes() const { return bytes_; }

    // frees what it owns; a borrowed pointer is only forgotten
    void reset() {
        if (p_ && owned_) Mem::free((void*)p_);
        drop();
    }
    // holds memory that belongs to someone else (a view's rows, rows attached by the caller)
    void borrow(T* p, size_t bytes) {
        reset();
        p_ = p;
        bytes_ = bytes;
    }
    // An owned buffer of at least `bytes` is kept; otherwise the old one is freed FIRST, then the new one allocated (old and
    // new never exist together: some of these are gigabytes).  On failure the buffer is empty and the code is returned; the
    // next call tries again.
    int need(size_t bytes) {
        if (p_ && owned_ && bytes_ >= bytes) return 0;
        reset();
        void* p = nullptr;
        const int e = Mem::alloc(&p, bytes);
        if (e) return e;
        p_ = (T*)p;
        bytes_ = bytes;
        owned_ = true;
        return 0;
    }
    // ... a fresh allocation zeroed, a kept one left as it is.  *zeroing: the failure was the zeroing, not the allocation.
    int need_zeroed(size_t bytes, bool* zeroing = nullptr) {
        if (zeroing) *zeroing = false;
        if (p_ && owned_ && bytes_ >= bytes) return 0;
        int e = need(bytes);
        if (e) return e;
        e = Mem::zero((void*)p_, bytes);
        if (e) {
            reset();
            if (zeroing) *zeroing = true;
        }
        return e;
    }

private:
    void drop() { p_ = nullptr; bytes_ = 0; owned_ = false; }
};

// Two buffers that are sized together, re-made: both are released before either is allocated (the same peak-memory rule),
// and a failure leaves both empty.
template <class A, class B>
inline int remake(A& a, size_t a_bytes, B& b, size_t b_bytes) {
    a.reset();
    b.reset();
    int e = a.need(a_bytes);
    if (!e) e = b.need(b_bytes);
    if (e) {
        a.reset();
        b.reset();
    }
    return e;
}

}  // namespace ts
