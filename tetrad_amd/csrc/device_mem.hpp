// device_mem.hpp -- (host) owners of device and page-locked memory, of events, streams and pool blocks, the two-piece
// staging ring, and the struct of one resident site layout.
//
// Nothing here synchronises: a caller that regrows a buffer the device may still read waits for the device first.  (The
// one exception is the staging ring, which waits for its own two copies before it gives its pieces back.)
// Nothing here selects a device either: the owner of a buffer does, before the buffer's first and last use.
#pragma once

// Move-only owner of one block of `cap()` elements, device (hipMalloc) or page-locked host memory (hipHostMalloc);
// converts to the bare pointer wherever one is expected.
template <typename T, bool PINNED>
class OwnedBuf {
    T *p_ = nullptr;
    size_t cap_ = 0;

public:
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf &) = delete;
    OwnedBuf &operator=(const OwnedBuf &) = delete;
    OwnedBuf(OwnedBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept
    {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(cap_, o.cap_);
        }
        return *this;
    }
    ~OwnedBuf() { reset(); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t cap() const { return cap_; }
    void reset()
    {
        if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    // frees what it held, then allocates n elements; a failure leaves it empty
    hipError_t alloc(size_t n)
    {
        reset();
        const hipError_t e = PINNED ? hipHostMalloc((void **)&p_, n * sizeof(T), hipHostMallocDefault)
                                    : hipMalloc((void **)&p_, n * sizeof(T));
        if (e == hipSuccess) cap_ = n;
        else p_ = nullptr;
        return e;
    }
    // the grow-only idiom: nothing while n fits, else alloc(n) -- the old contents are gone
    hipError_t grow(size_t n) { return n <= cap_ ? hipSuccess : alloc(n); }
};
template <typename T> using DevBuf = OwnedBuf<T, false>;
template <typename T> using PinnedBuf = OwnedBuf<T, true>;

// Move-only owner of one handle that FREE gives back: the base of Event, Stream and PoolBuf.  Converts to the bare handle.
template <typename H, auto FREE>
class Handle {
protected:
    H h_ = nullptr;

public:
    Handle() = default;
    Handle(Handle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Handle &operator=(Handle &&o) noexcept
    {
        if (this != &o) {
            reset();
            std::swap(h_, o.h_);
        }
        return *this;
    }
    ~Handle() { reset(); }
    operator H() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
    void reset()
    {
        if (h_) (void)FREE(h_);
        h_ = nullptr;
    }
};
// one event, without timing unless it is asked for
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t create(bool timing = false)
    {
        reset();
        return timing ? hipEventCreate(&h_) : hipEventCreateWithFlags(&h_, hipEventDisableTiming);
    }
};
// one non-blocking stream (destroyed with work queued, it goes once that work is done)
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    hipError_t create()
    {
        reset();
        return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking);
    }
};
// one block of n elements out of the page-locked pool (pinned_pool.hpp); alloc answers with a TQ_* code
inline int pool_release(void *p) { return pool().release(p); }
template <typename T>
struct PoolBuf : Handle<T *, pool_release> {
    int alloc(size_t n)
    {
        this->reset();
        return pool().alloc(n * sizeof(T), (void **)&this->h_);
    }
};

// A small host array on its way to the device without a wait for the stream: two page-locked pieces in turn, each with
// the event behind the H2D copy that last read it.  The caller fills next() and issues its hipMemcpyAsync from it, then
// calls sent(); the host waits only for the copy that read this piece two turns ago, so the next call can hand its
// array over while this copy is queued.  The one rule of release, whoever releases: the pool hands a released block to
// any caller, so reset() and the destructor first wait for both copies.
template <typename T>
struct StagingRing {
    PoolBuf<T> piece[2];
    Event ev[2];
    int turn = 1;                   // the piece handed out last
    ~StagingRing() { reset(); }
    // pieces of n elements and their events, where absent: TQ_ERR_OOM without a piece, TQ_ERR_HIP without an event
    int ensure(size_t n)
    {
        for (int i = 0; i < 2; ++i) {
            if (!piece[i] && piece[i].alloc(n) != TQ_OK) return TQ_ERR_OOM;
            if (!ev[i] && ev[i].create() != hipSuccess) return TQ_ERR_HIP;
        }
        return TQ_OK;
    }
    hipError_t next(T *&p) { p = piece[turn ^= 1]; return hipEventSynchronize(ev[turn]); }
    hipError_t sent(hipStream_t stream) { return hipEventRecord(ev[turn], stream); }
    void reset()
    {
        for (Event &e : ev) if (e) (void)hipEventSynchronize(e);
        for (int i = 0; i < 2; ++i) { piece[i].reset(); ev[i].reset(); }
    }
};

// One resident site layout (tetrad_hip.hip, "Data layout in HBM"): rows, nibbles, the optional nibbles with 4 = missing,
// uint4 planes and the 12-byte plane records with runbeg behind them.  The arrays are allocated for capSp sites per row
// and hold the current Sp <= capSp of them.  One rule for runbeg, whichever set and whatever the current width: it sits
// behind the allocation's capacity, planes3 + T * capW * 3 -- the builders and the kernels receive that pointer, so where
// it points inside the allocation is invisible to them.
struct SiteSet {
    DevBuf<uint8_t> rows, nib, nib5;
    DevBuf<uint4> planes;
    DevBuf<uint32_t> planes3;
    int64_t Sp = 0, W = 0;          // current sites per row, plane records per row (Sp / 32)
    int64_t capSp = 0;              // sites per row the arrays were allocated for

    void reset()
    {
        rows.reset(); nib.reset(); nib5.reset(); planes.reset(); planes3.reset();
        Sp = W = capSp = 0;
    }
    // the one copy of the size formulas; a failure leaves the set empty
    hipError_t alloc(int64_t T, int64_t cap, bool with_nib5)
    {
        reset();
        const int64_t capW = cap / 32;
        hipError_t e = rows.alloc((size_t)(T * cap));
        if (e == hipSuccess) e = nib.alloc((size_t)(T * cap / 2));
        if (e == hipSuccess && with_nib5) e = nib5.alloc((size_t)(T * cap / 2));
        if (e == hipSuccess) e = planes.alloc((size_t)(T * capW));
        if (e == hipSuccess) e = planes3.alloc((size_t)(T * capW * 3 + capW));
        if (e == hipSuccess) capSp = cap;
        else reset();
        return e;
    }
    void set_sites(int64_t sp) { Sp = sp; W = sp / 32; }
    uint32_t *runbeg(int64_t T) const { return planes3 + (size_t)T * (size_t)(capSp / 32) * 3; }
    // the layout fields of a DevData (T and inv are the caller's)
    void fill(DevData &d, int64_t T) const
    {
        d.rows = rows;
        d.nib = nib;
        d.nib5 = nib5;
        d.planes = planes;
        d.planes3 = planes3;
        d.runbeg = runbeg(T);
        d.pitch = Sp;
        d.W = W;
        d.ntiles = (int32_t)(Sp / TILE);
    }
};
