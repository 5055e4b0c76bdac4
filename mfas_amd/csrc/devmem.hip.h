// devmem.hip.h — who owns device memory on the host side (host only, plain C++17; the translation unit has included the HIP runtime):
// DevBuf<T>, the ONE place that calls hipMalloc / hipFree.  A population's buffers and every function's scratch are DevBufs, so nothing is
// freed by hand and a capacity cannot disagree with its pointer.  It never zeroes, never synchronises, never touches a stream: those
// stay visible where the buffer is used.  Kernels receive .get().  No DevBuf has static storage duration (it would outlive the runtime).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#ifdef MFAS_TEST_HOOKS      // the test-hooks variant counts the live allocations of the process (tests/test_gpu_devmem.py); never in the product library
#include <atomic>
static std::atomic<int64_t> g_devbuf_live{0};
extern "C" int64_t mfas_test_live_allocations(void) { return g_devbuf_live.load(); }
#define DEVBUF_LIVE(d) (void)(g_devbuf_live += (d))
#else
#define DEVBUF_LIVE(d) (void)0
#endif

template <typename T>
struct DevBuf {
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    T* get() const { return p_; }
    size_t size() const { return n_; }       // elements it was allocated for
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) {
            (void)hipFree(p_);
            DEVBUF_LIVE(-1);
        }
        p_ = nullptr; n_ = 0;
    }
    // exactly n elements, whatever it held (n = 0: empty); empty after a failure
    hipError_t alloc(size_t n) {
        reset();
        void* q = nullptr;
        const hipError_t e = n ? hipMalloc(&q, sizeof(T) * n) : hipSuccess;
        if (e == hipSuccess && n) {
            p_ = static_cast<T*>(q); n_ = n;
            DEVBUF_LIVE(+1);
        }
        return e;
    }
    // grow-only: nothing within the capacity; else the old block goes FIRST (the two never coexist) and a failure leaves it empty
    hipError_t reserve(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }
    // a copy of v (an empty list stays a null pointer)
    hipError_t upload(const std::vector<T>& v) {
        const hipError_t e = alloc(v.size());
        return e != hipSuccess || v.empty() ? e : hipMemcpy(p_, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
    }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
#undef DEVBUF_LIVE
