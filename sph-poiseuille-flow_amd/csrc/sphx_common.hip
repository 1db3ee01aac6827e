// sphx_common.hip -- error state, device selection, version.
#include "sphx_common.hpp"

#include <map>
#include <mutex>
#include <unordered_map>
#include <utility>

namespace sphx {

static thread_local std::string g_err_msg;
static thread_local std::string g_err_id;

void set_last_error(int code, const std::string &id, const std::string &msg)
{
    (void)code;
    g_err_id = id;
    g_err_msg = msg;
}

int report(const Error &e)
{
    set_last_error(e.code, e.id, e.what());
    return e.code;
}

int report_unknown(const std::exception &e)
{
    set_last_error(SPHX_ERR_DEVICE, "SPHX:Internal", e.what());
    return SPHX_ERR_DEVICE;
}

namespace {

size_t pool_class(size_t bytes)
{  // power of two below 1 MiB, whole MiB above: few distinct sizes, at most 2x slack on small blocks
    size_t c = 256;
    if (bytes <= (1u << 20)) {
        while (c < bytes) c <<= 1;
        return c;
    }
    return (bytes + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
}

struct Pool {
    std::mutex m;
    std::multimap<std::pair<int, size_t>, void *> free_blocks;  // (device, class) -> block
    std::unordered_map<void *, int> owner;                      // block -> the device it was allocated on
    size_t cached = 0;
    uint64_t hits = 0, misses = 0;  // pool_alloc calls served from the cache / sent to hipMalloc, since process start
    // poison at free (sphx_pool_poison_on_free, test support): off by default, and then pool_free makes no HIP call
    bool poison = false;
    uint32_t poison_word = 0;
    uint64_t poisoned = 0, poison_skipped = 0;                  // blocks filled / fills skipped inside a capture, since process start
    std::unordered_map<int, hipStream_t> poison_streams;        // device -> the pool's own non-blocking stream, made on first use
    static constexpr size_t kMaxCached = (size_t)4 << 30;
    void trim()
    {
        for (auto &kv : free_blocks) { owner.erase(kv.second); (void)hipFree(kv.second); }
        free_blocks.clear();
        cached = 0;
    }
    ~Pool() { /* process exit: the runtime reclaims device memory; HIP may already be torn down */ }
};

Pool &pool()
{
    static Pool *p = new Pool();  // never destroyed: DevBufs in static storage may outlive any static pool
    return *p;
}

thread_local int g_capturing = 0;  // CaptureScope depth of this thread

// Fill a block on its way into the cache with the poison word, on the pool's own stream of the block's device, and wait for
// that stream alone (the pool's lock is held): the fill has ended before any later owner can take the block.  Work the
// former owner left in flight on its own streams is not waited for -- it races with the fill, which is what the mode is for.
void poison_block(Pool &P, void *p, size_t cls, int dev)
{
    if (g_capturing) { ++P.poison_skipped; return; }
    int cur = 0;
    SPHX_HIP(hipGetDevice(&cur));
    if (cur != dev) SPHX_HIP(hipSetDevice(dev));
    hipError_t e = hipSuccess;
    auto it = P.poison_streams.find(dev);
    if (it == P.poison_streams.end()) {
        hipStream_t st = nullptr;
        e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (e == hipSuccess) it = P.poison_streams.emplace(dev, st).first;
    }
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)p, (int)P.poison_word, cls / sizeof(uint32_t), it->second);
    if (e == hipSuccess) e = hipStreamSynchronize(it->second);
    if (cur != dev) (void)hipSetDevice(cur);
    SPHX_HIP(e);
    ++P.poisoned;
}

}  // namespace

CaptureScope::CaptureScope() { ++g_capturing; }
CaptureScope::~CaptureScope() { --g_capturing; }

void *pool_alloc(size_t bytes)
{
    const size_t cls = pool_class(bytes);
    int dev = 0;
    SPHX_HIP(hipGetDevice(&dev));
    Pool &P = pool();
    {
        std::lock_guard<std::mutex> lk(P.m);
        auto it = P.free_blocks.find({dev, cls});
        if (it != P.free_blocks.end()) {
            void *p = it->second;
            P.free_blocks.erase(it);
            P.cached -= cls;
            ++P.hits;
            return p;
        }
        ++P.misses;
    }
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, cls);
    if (e != hipSuccess) {  // give the cache back and try once more
        (void)hipGetLastError();
        {
            std::lock_guard<std::mutex> lk(P.m);
            P.trim();
        }
        e = hipMalloc(&p, cls);
    }
    SPHX_HIP(e);
    {
        std::lock_guard<std::mutex> lk(P.m);
        P.owner[p] = dev;
    }
    return p;
}

void pool_free(void *p, size_t bytes)
{
    if (!p) return;
    const size_t cls = pool_class(bytes);
    Pool &P = pool();
    std::lock_guard<std::mutex> lk(P.m);
    // a block goes back under the device that allocated it, whatever device is current now
    auto it = P.owner.find(p);
    if (it == P.owner.end() || P.cached + cls > Pool::kMaxCached) {
        if (it != P.owner.end()) P.owner.erase(it);
        (void)hipFree(p);
        return;
    }
    const std::pair<int, size_t> key{it->second, cls};
    if (P.poison) {
        try {
            poison_block(P, p, cls, it->second);
        } catch (const Error &) { /* pool_free runs in destructors: a fill that failed leaves the block as it was returned */
            (void)hipGetLastError();
        }
        // ... and goes to the FRONT of its class: the next request of that size gets the block released last, so a neighbour
        // takes a block released too early while its former owner is still at work, not an older one out of a warm cache
        P.free_blocks.insert(P.free_blocks.lower_bound(key), {key, p});
    } else {
        P.free_blocks.insert({key, p});
    }
    P.cached += cls;
}

void pool_stats(uint64_t out[4])
{
    Pool &P = pool();
    std::lock_guard<std::mutex> lk(P.m);
    out[0] = P.cached;
    out[1] = P.free_blocks.size();
    out[2] = P.hits;
    out[3] = P.misses;
}

void pool_poison_on_free(bool on, uint32_t word)
{
    Pool &P = pool();
    std::lock_guard<std::mutex> lk(P.m);
    P.poison = on;
    P.poison_word = word;
}

void pool_poison_stats(uint64_t out[2])
{
    Pool &P = pool();
    std::lock_guard<std::mutex> lk(P.m);
    out[0] = P.poisoned;
    out[1] = P.poison_skipped;
}

uint64_t pool_scrub(uint32_t word)
{
    Pool &P = pool();
    std::lock_guard<std::mutex> lk(P.m);
    if (P.free_blocks.empty()) return 0;  // nothing cached: no HIP call at all
    int dev = 0;
    SPHX_HIP(hipGetDevice(&dev));
    uint64_t n = 0;
    // a free block is nobody's (whoever returned it had synchronised its work): the fill races with nothing, and it ends
    // before the lock is released, so no pool_alloc can hand out a block that is still being filled
    for (auto it = P.free_blocks.lower_bound({dev, 0}); it != P.free_blocks.end() && it->first.first == dev; ++it, ++n)
        SPHX_HIP(hipMemsetD32Async((hipDeviceptr_t)it->second, (int)word, it->first.second / sizeof(uint32_t), nullptr));
    if (n) SPHX_HIP(hipDeviceSynchronize());
    return n;
}

void ensure_device()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        throw Error(SPHX_ERR_DEVICE, "SPHX:NoDevice",
                    "libsphx: no HIP device available (this library has no CPU fallback)");
    }
}

}  // namespace sphx

SPHX_EXPORT const char *sphx_version(void) { return "sphx 0.1 (gfx950)"; }
SPHX_EXPORT const char *sphx_last_error(void) { return sphx::g_err_msg.c_str(); }
SPHX_EXPORT const char *sphx_last_error_id(void) { return sphx::g_err_id.c_str(); }

SPHX_EXPORT int sphx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

SPHX_EXPORT int sphx_set_device(int device)
{
    SPHX_TRY
    sphx::ensure_device();
    SPHX_HIP(hipSetDevice(device));
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_pool_stats(uint64_t out[4])
{
    SPHX_TRY
    sphx::require(out != nullptr, "SPHX:Pool:args", "sphx_pool_stats: out must not be NULL");
    sphx::pool_stats(out);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_pool_scrub(uint32_t word, uint64_t *n_blocks)
{
    SPHX_TRY
    const uint64_t n = sphx::pool_scrub(word);
    if (n_blocks) *n_blocks = n;
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_pool_poison_on_free(int on, uint32_t word)
{
    SPHX_TRY
    sphx::pool_poison_on_free(on != 0, word);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_pool_poison_stats(uint64_t out[2])
{
    SPHX_TRY
    sphx::require(out != nullptr, "SPHX:Pool:args", "sphx_pool_poison_stats: out must not be NULL");
    sphx::pool_poison_stats(out);
    return SPHX_OK;
    SPHX_CATCH
}
