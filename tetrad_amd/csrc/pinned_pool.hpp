// pinned_pool.hpp -- (host) the process-wide pool of page-locked host memory.
#pragma once

// ---------------------------------------------------------------------------------------------
// Pinned host memory pool (process-wide: blocks handed to a caller may outlive any context).
// Result arrays that live in such a block are written by the copy engine directly (no staging, no
// host pass); blocks are recycled because pinning pages costs about as much as a resolve call.
// ---------------------------------------------------------------------------------------------
struct PinnedPool {
    std::mutex mu;
    std::map<uintptr_t, size_t> live;              // base -> bytes of blocks handed out
    std::multimap<size_t, void *> idle;            // bytes -> base of cached blocks
    size_t idle_bytes = 0;
    static constexpr size_t IDLE_CAP = (size_t)4 << 30;
    static size_t round_up(size_t b)
    {
        size_t g = (size_t)1 << 16;
        while (g < b && g < ((size_t)1 << 24)) g <<= 1;         // 64 KiB .. 16 MiB: powers of two
        if (g >= b) return g;
        const size_t step = (size_t)1 << 24;                   // beyond: multiples of 16 MiB
        return (b + step - 1) / step * step;
    }
    int alloc(size_t bytes, void **out)
    {
        const size_t want = round_up(bytes ? bytes : 1);
        std::lock_guard<std::mutex> g(mu);
        try {
            auto it = idle.lower_bound(want);
            if (it != idle.end() && it->first <= want * 2) {
                void *p = it->second;
                const size_t sz = it->first;
                idle.erase(it);
                idle_bytes -= sz;
                live[(uintptr_t)p] = sz;
                *out = p;
                return TQ_OK;
            }
            void *p = nullptr;
            if (hipHostMalloc(&p, want, hipHostMallocPortable) != hipSuccess || !p) return TQ_ERR_OOM;
            live[(uintptr_t)p] = want;
            *out = p;
            return TQ_OK;
        } catch (...) {
            return TQ_ERR_OOM;
        }
    }
    int release(void *p)
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = live.find((uintptr_t)p);
        if (it == live.end()) return TQ_ERR_INVALID_ARG;
        const size_t sz = it->second;
        live.erase(it);
        bool cached = false;
        if (idle_bytes + sz <= IDLE_CAP) {
            try {
                idle.emplace(sz, p);
                idle_bytes += sz;
                cached = true;
            } catch (...) {
            }
        }
        if (!cached) (void)hipHostFree(p);
        return TQ_OK;
    }
    bool owns(const void *p, size_t bytes)
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = live.upper_bound((uintptr_t)p);
        if (it == live.begin()) return false;
        --it;
        return (uintptr_t)p + bytes <= it->first + it->second;
    }
};

PinnedPool &pool()
{
    static PinnedPool *p = new PinnedPool();       // never destroyed: blocks may be alive at exit
    return *p;
}

// true when [p, p+bytes) is page-locked memory the copy engine can write asynchronously
bool is_pinned(const void *p, size_t bytes)
{
    if (!p) return false;
    if (pool().owns(p, bytes)) return true;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();                               // unregistered memory: clear the sticky error
        return false;
    }
    return a.type == hipMemoryTypeHost;
}
