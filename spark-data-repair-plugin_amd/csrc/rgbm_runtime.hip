// rgbm_runtime.hip -- what every translation unit of librepairgbm.so stands on, host side only: the thread-local error text, the caching
// device-memory pool (rgbm_host.h) with its guard and trace kernels, the page-locked staging of large host -> HBM copies, and the entry
// points of include/rgbm.h that belong to no table and no model (version, devices, error text, page-locked host memory, the caches).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "rgbm_host.h"

#define RGBM_VERSION 220   // numerics spec v2.2: float32 (g, h) as LightGBM computes them, exact integer histogram sums on a fixed-point grid chosen per class tree and boosting iteration (rgbm_numerics.h)

namespace {

thread_local std::string g_err;
}  // namespace
std::string& rgh::last_error() { return g_err; }

// ---- caching device-memory pool (rgbm_host.h)
namespace {
struct PoolBlock { void* p; size_t bytes; unsigned long long stamp; };
struct DevPool {
    std::mutex mu;
    std::multimap<std::pair<int, size_t>, PoolBlock> free_blocks;     // (device, bytes) -> block
    size_t cached = 0; unsigned long long clock = 0;
    size_t cap() {
        static const size_t c = [] { const char* e = getenv("RGBM_POOL_MB"); long long mb = e ? atoll(e) : 65536; return (size_t)std::max<long long>(mb, 0) << 20; }();
        return c;
    }
    // drop the least recently freed blocks until at most `keep` bytes stay cached (mu held)
    void trim_locked(size_t keep) {
        while (cached > keep && !free_blocks.empty()) {
            auto victim = free_blocks.begin();
            for (auto it = free_blocks.begin(); it != free_blocks.end(); ++it) if (it->second.stamp < victim->second.stamp) victim = it;
            int cur = 0; (void)hipGetDevice(&cur);
            if (cur != victim->first.first) (void)hipSetDevice(victim->first.first);
            (void)hipFree(victim->second.p);
            if (cur != victim->first.first) (void)hipSetDevice(cur);
            cached -= victim->second.bytes;
            free_blocks.erase(victim);
        }
    }
    ~DevPool() { /* process exit: the driver reclaims device memory; HIP may already be shut down here */ }
};
DevPool& pool() { static DevPool* p = new DevPool(); return *p; }
}  // namespace

// RGBM_GUARD=1 (debugging): every buffer sits between two 2 MB guard zones filled with 0xC3, and so is the slack between the bytes asked
// for and the end of the pool block; pool_free checks that nobody wrote there and says so on stderr.  A kernel that READS out of
// bounds sees the same 0xC3 bytes in every process instead of a neighbour's live data.  The first allocation says "[rgbm guard] on" on
// stderr, after checking the check itself (guard_self_check); RGBM_POISON=1 (DevBuf::alloc, rgbm_host.h) says "[rgbm poison] on".
bool rgh::guard_on() { static const bool g = getenv("RGBM_GUARD") != nullptr; return g; }
bool rgh::poison_on() {
    static const bool p = [] { const bool on = getenv("RGBM_POISON") != nullptr; if (on) fprintf(stderr, "[rgbm poison] on\n"); return on; }();
    return p;
}
namespace {
using rgh::guard_on;
constexpr size_t GUARD = 2u << 20;
std::mutex g_guard_mu; std::map<void*, size_t> g_guard_bytes;
__global__ void k_guard_check(const unsigned char* p, size_t n, unsigned long long* bad /* [0] count, [1] first offset */) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        if (p[i] != 0xC3) { atomicAdd(&bad[0], 1ull); atomicMin(&bad[1], (unsigned long long)i); }
}
// RGBM_TRACE (debugging): wrapping 64-bit sum of a buffer's words
__global__ void k_trace_sum(const unsigned long long* p, size_t nwords, unsigned long long* out) {
    unsigned long long a = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (size_t)gridDim.x * blockDim.x) a += p[i] * (2 * (unsigned long long)i + 1);
    atomicAdd(out, a);
}
void* pool_alloc_raw(size_t bytes, size_t* block_bytes, int* device);
void pool_free_raw(void* p, size_t block_bytes, int device);
}  // namespace

void rgh::trace_sum(const void* src, size_t bytes, unsigned long long* d_out, hipStream_t s) {
    hipLaunchKernelGGL(k_trace_sum, dim3(2048), dim3(256), 0, s, (const unsigned long long*)src, bytes / 8, d_out);
}

namespace {
// a buffer of `bytes` bytes between its two zones, the slack of the pool block included in the second
void* guarded_alloc(size_t bytes, size_t* block_bytes, int* device) {
    unsigned char* raw = static_cast<unsigned char*>(pool_alloc_raw(bytes + 2 * GUARD, block_bytes, device));
    if (hipMemset(raw, 0xC3, GUARD) != hipSuccess || hipMemset(raw + GUARD + bytes, 0xC3, *block_bytes - GUARD - bytes) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
        throw std::runtime_error("RGBM_GUARD: hipMemset failed");
    return raw + GUARD;
}

// The zone check: how many bytes of the two zones around the buffer of `bytes` bytes at raw + GUARD no longer hold 0xC3, and the first of them
// (an offset into its zone).  Blocking, on the null stream.
struct ZoneHit { const char* what; bool front; unsigned long long count, first; };
void guard_check_zones(const unsigned char* raw, size_t bytes, size_t block_bytes, ZoneHit (&hits)[2]) {
    static thread_local unsigned long long* d_bad = nullptr;
    if (!d_bad && hipMalloc(&d_bad, 16) != hipSuccess) { d_bad = nullptr; throw std::runtime_error("RGBM_GUARD: hipMalloc failed"); }
    const struct { const unsigned char* q; size_t n; const char* what; } zones[2] = {{raw, GUARD, "front guard"},
                                                                                      {raw + GUARD + bytes, block_bytes - GUARD - bytes, "slack + back guard"}};
    for (int z = 0; z < 2; ++z) {
        unsigned long long h[2] = {0ull, ~0ull};
        bool ok = hipMemcpy(d_bad, h, 16, hipMemcpyHostToDevice) == hipSuccess;
        hipLaunchKernelGGL(k_guard_check, dim3(1024), dim3(256), 0, nullptr, zones[z].q, zones[z].n, d_bad);
        ok = ok && hipGetLastError() == hipSuccess && hipMemcpy(h, d_bad, 16, hipMemcpyDeviceToHost) == hipSuccess;
        if (!ok) throw std::runtime_error("RGBM_GUARD: the zone check did not run");
        hits[z] = ZoneHit{zones[z].what, z == 0, h[0], h[1]};
    }
}

// First use in guard mode: the check must see a byte that IS overwritten, or a clean run says nothing.  One byte just past the end of a small
// buffer is cleared from the host (inside the buffer's own back zone, so inside its own allocation); the check has to count that byte alone.
void guard_self_check() {
    const size_t bytes = 192;
    size_t block = 0; int dev = 0;
    unsigned char* p = static_cast<unsigned char*>(guarded_alloc(bytes, &block, &dev));
    ZoneHit hits[2];
    const bool wrote = hipMemset(p + bytes, 0, 1) == hipSuccess;
    try { guard_check_zones(p - GUARD, bytes, block, hits); }
    catch (...) { pool_free_raw(p - GUARD, block, dev); throw; }
    pool_free_raw(p - GUARD, block, dev);
    if (!wrote || hits[0].count != 0 || hits[1].count != 1 || hits[1].first != 0) {
        char b[256];
        snprintf(b, sizeof(b), "RGBM_GUARD: self-check failed (one byte cleared past a %zu-byte buffer; the check counts %llu in front, %llu behind, first at %lld)",
                 bytes, hits[0].count, hits[1].count, (long long)hits[1].first);
        throw std::runtime_error(b);
    }
    fprintf(stderr, "[rgbm guard] on, self-check ok\n");
}
}  // namespace

void* rgh::pool_alloc(size_t bytes, size_t* block_bytes, int* device) {
    if (!guard_on()) return pool_alloc_raw(bytes, block_bytes, device);
    static std::once_flag self_check;                   // (a check that throws runs again with the next allocation)
    std::call_once(self_check, guard_self_check);
    void* p = guarded_alloc(bytes, block_bytes, device);
    { std::lock_guard<std::mutex> lk(g_guard_mu); g_guard_bytes[p] = bytes; }
    return p;
}

void rgh::pool_free(void* p, size_t block_bytes, int device) {
    if (!p) return;
    if (!guard_on()) { pool_free_raw(p, block_bytes, device); return; }
    size_t bytes = 0;
    { std::lock_guard<std::mutex> lk(g_guard_mu); auto it = g_guard_bytes.find(p); if (it != g_guard_bytes.end()) { bytes = it->second; g_guard_bytes.erase(it); } }
    unsigned char* raw = static_cast<unsigned char*>(p) - GUARD;
    ZoneHit hits[2] = {};
    try { guard_check_zones(raw, bytes, block_bytes, hits); }
    catch (const std::exception& e) { fprintf(stderr, "[rgbm guard] buffer of %zu bytes (block %zu): not checked (%s)\n", bytes, block_bytes, e.what()); }
    for (const ZoneHit& h : hits)
        if (h.count) fprintf(stderr, "[rgbm guard] buffer of %zu bytes (block %zu): %llu byte(s) of the %s were overwritten, first at offset %lld from the buffer's %s\n",
                             bytes, block_bytes, h.count, h.what, h.front ? (long long)h.first - (long long)GUARD : (long long)h.first, h.front ? "start" : "end");
    pool_free_raw(raw, block_bytes, device);
}

namespace {
void* pool_alloc_raw(size_t bytes, size_t* block_bytes, int* device) {
    int dev = 0; (void)hipGetDevice(&dev);
    *device = dev;
    DevPool& P = pool();
    // round up so that nearly equal requests can share blocks: 256 B below 1 MB, 2 MB above
    const size_t want = bytes < (1u << 20) ? ((bytes + 255) & ~(size_t)255) : ((bytes + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1));
    if (P.cap() > 0) {
        std::lock_guard<std::mutex> lk(P.mu);
        auto it = P.free_blocks.lower_bound(std::make_pair(dev, want));
        // a request never swallows a much larger block (up to 8x its size, 4x below 1 MB)
        if (it != P.free_blocks.end() && it->first.first == dev && it->first.second <= want * (want >= (1u << 20) ? 8 : 4)) {
            void* p = it->second.p; *block_bytes = it->second.bytes;
            P.cached -= it->second.bytes;
            P.free_blocks.erase(it);
            return p;
        }
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess && P.cap() > 0) {       // out of memory with blocks parked in the pool: give them back and retry once
        (void)hipGetLastError();
        { std::lock_guard<std::mutex> lk(P.mu); P.trim_locked(0); }
        e = hipMalloc(&p, want);
    }
    if (e != hipSuccess) { (void)hipGetLastError(); char b[256]; snprintf(b, sizeof(b), "hipMalloc of %zu bytes failed: %s", want, hipGetErrorString(e)); throw rgh::device_oom(b); }
    *block_bytes = want;
    return p;
}

void pool_free_raw(void* p, size_t block_bytes, int device) {
    if (!p) return;
    DevPool& P = pool();
    if (P.cap() == 0 || block_bytes > P.cap()) {
        int cur = 0; (void)hipGetDevice(&cur);
        if (cur != device) (void)hipSetDevice(device);
        (void)hipFree(p);
        if (cur != device) (void)hipSetDevice(cur);
        return;
    }
    std::lock_guard<std::mutex> lk(P.mu);
    P.free_blocks.emplace(std::make_pair(device, block_bytes), PoolBlock{p, block_bytes, ++P.clock});
    P.cached += block_bytes;
    if (P.cached > P.cap()) P.trim_locked(P.cap());
}

}  // namespace

void rgh::pool_trim(size_t keep_bytes) { DevPool& P = pool(); std::lock_guard<std::mutex> lk(P.mu); P.trim_locked(keep_bytes); }

// Host -> HBM copy of a caller-owned block.  A pageable block handed to hipMemcpy is staged by the driver through one small
// bounce buffer (measured 4-7 GB/s for the 735 MB of the 10M x 16 tables); page-locking it in place (hipHostRegister) costs more
// than it saves for a one-off copy (4.4 GB/s).  So the library stages it itself: two page-locked 32 MB buffers kept for the
// life of the process, filled by a few host threads while the copy engine drains the other one.  Blocks that already are
// pinned (rgbm_host_alloc, or registered by the caller) go straight to the copy engine.  RGBM_NO_PIN=1: plain hipMemcpy.
namespace {
struct StageRing {
    std::mutex mu; void* buf[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr}; hipStream_t s = nullptr; int device = -1; bool ok = false;
    static constexpr size_t CHUNK = 32u << 20;
    bool ready(int dev) {
        if (ok && device == dev) return true;
        if (ok) return false;                                        // ring belongs to another device: plain copy for this one
        if (hipHostMalloc(&buf[0], CHUNK, hipHostMallocDefault) != hipSuccess || hipHostMalloc(&buf[1], CHUNK, hipHostMallocDefault) != hipSuccess ||
            hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        device = dev; ok = true;
        return true;
    }
};
StageRing& stage_ring() { static StageRing* r = new StageRing(); return *r; }
}  // namespace

void rgh::upload_pinned(void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return;
    hipPointerAttribute_t attr; memset(&attr, 0, sizeof(attr));
    const bool pinned = hipPointerGetAttributes(&attr, src) == hipSuccess && attr.type == hipMemoryTypeHost;
    if (!pinned) (void)hipGetLastError();
    int dev = 0; (void)hipGetDevice(&dev);
    StageRing& R = stage_ring();
    if (pinned || bytes < (8u << 20) || getenv("RGBM_NO_PIN") != nullptr) { HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return; }
    std::lock_guard<std::mutex> lk(R.mu);
    if (!R.ready(dev)) { HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return; }
    const int nthr = (int)std::min<size_t>(8, std::max<size_t>(1, std::thread::hardware_concurrency() / 2));
    size_t off = 0; int i = 0;
    while (off < bytes) {
        const size_t n = std::min(StageRing::CHUNK, bytes - off);
        const int b = i & 1;
        if (i >= 2) HIPCHK(hipEventSynchronize(R.ev[b]));            // the copy engine is done with this buffer
        std::vector<std::thread> th;
        const size_t per = (n + nthr - 1) / nthr;
        for (int t = 1; t < nthr; ++t) {
            const size_t o = per * t; if (o >= n) break;
            th.emplace_back([=, &R]() { memcpy((char*)R.buf[b] + o, (const char*)src + off + o, std::min(per, n - o)); });
        }
        memcpy(R.buf[b], (const char*)src + off, std::min(per, n));
        for (auto& t : th) t.join();
        HIPCHK(hipMemcpyAsync((char*)dst + off, R.buf[b], n, hipMemcpyHostToDevice, R.s));
        HIPCHK(hipEventRecord(R.ev[b], R.s));
        off += n; ++i;
    }
    HIPCHK(hipStreamSynchronize(R.s));
}

extern "C" {

RGBM_EXPORT int rgbm_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
RGBM_EXPORT const char* rgbm_last_error(void) { return g_err.c_str(); }
RGBM_EXPORT int rgbm_version(void) { return RGBM_VERSION; }
RGBM_EXPORT int rgbm_release_cache(void) {
    return rgh::guarded([&]() {
        rgh::pool_trim(0);
        rgh::release_host_staging();
        return RGBM_OK;
    });
}

RGBM_EXPORT int rgbm_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return rgh::fail(RGBM_ERR_ARG, "rgbm_host_alloc: bad argument");
    return rgh::guarded([&]() {
        void* p = nullptr;
        HIPCHK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        *out = p;
        return RGBM_OK;
    });
}

RGBM_EXPORT void rgbm_host_free(void* p) { if (p) (void)hipHostFree(p); }

}  // extern "C"
