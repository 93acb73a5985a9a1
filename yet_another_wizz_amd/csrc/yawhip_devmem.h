// Who owns device memory: every hipMalloc'd array of the library belongs to one DevPtr (a member of the handle, layout or
// workspace it lives as long as, or a local of the function that needs it for one call), and what an owner goes out of scope
// with, or is release()d with, is freed -- no unit keeps a list of pointers to free. This header is the only place that calls
// hipMalloc / hipFree. Private: never installed, not part of the C ABI.
#ifndef YAWHIP_DEVMEM_H
#define YAWHIP_DEVMEM_H
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>

#pragma GCC visibility push(hidden)

namespace yawhip_detail {

// Move-only owner of one hipMalloc'd array of T. Reads as a plain T * wherever one is expected (kernel launches, copies,
// pointer arithmetic); null while it owns nothing.
template <typename T>
class DevPtr {
    T *p = nullptr;

public:
    DevPtr() = default;
    DevPtr(DevPtr &&o) noexcept : p(std::exchange(o.p, nullptr)) {}
    DevPtr &operator=(DevPtr &&o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
        }
        return *this;
    }
    DevPtr(const DevPtr &) = delete;
    DevPtr &operator=(const DevPtr &) = delete;
    ~DevPtr() { release(); }

    // `count` elements and `extra_bytes` behind them (what it held before is freed first); empty after a failure
    hipError_t alloc(size_t count, size_t extra_bytes = 0) {
        release();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T) + extra_bytes);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    operator T *() const { return p; }
};

// Grow-only device workspace: reserve(n, slack) keeps what it has while n fits, else allocates n + slack elements anew.
template <typename T>
struct DevBuf {
    DevPtr<T> ptr;
    size_t cap = 0;

    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : ptr(std::move(o.ptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        ptr = std::move(o.ptr);
        cap = std::exchange(o.cap, 0);
        return *this;
    }

    hipError_t reserve(size_t n, size_t slack = 0) {
        if (n <= cap) return hipSuccess;
        cap = 0;
        const hipError_t e = ptr.alloc(n + slack);
        if (e == hipSuccess) cap = n + slack;
        return e;
    }
    void release() {
        ptr.release();
        cap = 0;
    }
};

// workgroups of 256 threads that cover n elements (the launches of the host units that own such memory)
inline unsigned grid_for(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace yawhip_detail

#pragma GCC visibility pop
#endif
