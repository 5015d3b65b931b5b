// device_mem.hpp -- (host) owners of device and page-locked memory, and the struct of one resident site layout.
//
// Nothing here synchronises: a caller that regrows a buffer the device may still read waits for the device first.
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
