// sphx_common.hpp -- host-side plumbing shared by the C-ABI translation units: error reporting
// (message + MEX-style id, the analogue of mexErrMsgIdAndTxt in sph_physics_mex.c:41-46), HIP call
// checking and a small RAII device buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sphx.h"

#define SPHX_EXPORT extern "C" __attribute__((visibility("default")))

namespace sphx {

struct Error : std::runtime_error {
    int code;
    std::string id;
    Error(int c, std::string i, const std::string &msg) : std::runtime_error(msg), code(c), id(std::move(i)) {}
};

void set_last_error(int code, const std::string &id, const std::string &msg);
int report(const Error &e);
int report_unknown(const std::exception &e);

inline void require(bool cond, const char *id, const char *msg)
{
    if (!cond) throw Error(SPHX_ERR_ARG, id, msg);
}

#define SPHX_HIP(expr)                                                                             \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            throw ::sphx::Error(SPHX_ERR_DEVICE, "SPHX:HIP",                                       \
                                std::string(#expr) + ": " + hipGetErrorString(_e));               \
    } while (0)

// Fails loudly when no HIP device is usable -- there is no CPU fallback by design.
void ensure_device();

// Device memory comes from a small caching pool: the stateless MEX-surface calls allocate a dozen arrays each and
// hipMalloc/hipFree (100+ us apiece, the free synchronising the device) dominated them -- 10.7 ms per step of the
// six-calls-per-step loop at 5 760 particles.  Whoever returns a block must have synchronised the work using it
// (every owner here does: the stateless calls before their scope ends, contexts before they are destroyed).
void *pool_alloc(size_t bytes);
void pool_free(void *p, size_t bytes);
// Diagnostics (sphx_pool_stats / sphx_pool_scrub, include/sphx.h).  A block comes back from the pool as it was returned:
// nothing clears it, so whoever takes one must write every element before it reads or returns it -- results must not depend
// on what a block held before (tests/test_gpu_pool_history.py holds the library to that).  pool_stats: cached bytes, cached
// blocks, and the pool_alloc calls served from the cache (hits) and by hipMalloc (misses) since process start; no HIP call.
// pool_scrub: fills every cached free block of the current device with `word` under the pool's lock, waits for the device
// and returns the number of blocks filled; the allocation path is untouched.  Not while a stream is capturing.
void pool_stats(uint64_t out[4]);
uint64_t pool_scrub(uint32_t word);
// Poison at free (sphx_pool_poison_on_free / sphx_pool_poison_stats, test support; off by default, and then pool_free is
// unchanged and makes no HIP call).  On: a block entering the cache is first filled with `word` on a non-blocking stream the
// pool owns, and that stream alone is waited for under the pool's lock -- no later owner can be overwritten by a late fill,
// while work the former owner left in flight races with the fill and shows in the bytes it produces.  A filled block is
// handed out before older blocks of its class, so the next taker of that size is the one that meets the former owner.  The invariant this
// makes visible: a block returns to the pool only after every stream that was given it has been waited for
// (tests/test_gpu_live_neighbours.py).  Blocks that go straight to hipFree are not filled, nor are blocks freed on a thread
// that is inside one of the library's stream captures (a CaptureScope): those are counted in out[1], the fills in out[0].
void pool_poison_on_free(bool on, uint32_t word);
void pool_poison_stats(uint64_t out[2]);
// Marks the calling thread as inside a hipStreamBeginCapture / hipStreamEndCapture pair of the library for its lifetime.
struct CaptureScope {
    CaptureScope();
    ~CaptureScope();
    CaptureScope(const CaptureScope &) = delete;
    CaptureScope &operator=(const CaptureScope &) = delete;
};

template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    explicit DevBuf(size_t n) { alloc(n); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_), owned_(o.owned_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p_ = o.p_; n_ = o.n_; owned_ = o.owned_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void alloc(size_t n)
    {
        release();
        n_ = n;
        if (n) p_ = static_cast<T *>(pool_alloc(n * sizeof(T)));
    }
    // n elements of memory somebody else owns (a member's block of a batch-wide array, see sphx_batch)
    void alias(T *p, size_t n)
    {
        release();
        p_ = p;
        n_ = n;
        owned_ = false;
    }
    void release()
    {
        if (p_ && owned_) pool_free(p_, n_ * sizeof(T));
        p_ = nullptr;
        n_ = 0;
        owned_ = true;
    }
    void zero(hipStream_t s = nullptr)
    {
        if (n_) SPHX_HIP(hipMemsetAsync(p_, 0, n_ * sizeof(T), s));
    }
    void upload(const T *host, size_t n, hipStream_t s = nullptr)
    {
        if (n) SPHX_HIP(hipMemcpyAsync(p_, host, n * sizeof(T), hipMemcpyHostToDevice, s));
    }
    void download(T *host, size_t n, hipStream_t s = nullptr) const
    {
        if (n) SPHX_HIP(hipMemcpyAsync(host, p_, n * sizeof(T), hipMemcpyDeviceToHost, s));
    }
    T *get() const { return p_; }
    size_t size() const { return n_; }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
    bool owned_ = true;
};

inline unsigned div_up(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

}  // namespace sphx

#define SPHX_TRY try {
#define SPHX_CATCH                                                                                 \
    }                                                                                              \
    catch (const ::sphx::Error &e) { return ::sphx::report(e); }                                   \
    catch (const std::exception &e) { return ::sphx::report_unknown(e); }
