// split_table.hpp -- (host) what the accumulators over sets of trees share: the staged chunk of
// prepared trees of tq_cons, tq_tbe and tq_rf, and the device split table with its host companion of tq_cons and tq_rf.
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace, behind `fail`, TQ_HIP
// and StreamOrder).  The kernels are those of consensus.hpp.
#pragma once

// the arguments every tq_*_add over a set of trees takes
int tree_set_args(tq_ctx *ctx, const char *who, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride)
{
    if (R < 0 || stride < 0 || (R > 0 && (!parents || !n_nodes)))
        return fail(ctx, TQ_ERR_INVALID_ARG, "%s: NULL pointer or negative size", who);
    return TQ_OK;
}

// recs[R][cons_stride(T)] = the prepared records of R trees: every tree is validated before the caller counts the first
int prepare_trees(tq_ctx *ctx, const char *who, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride,
                  int64_t T, std::vector<int32_t> &recs)
{
    const int64_t S = cons_stride(T);
    recs.assign((size_t)R * S, 0);
    for (int64_t r = 0; r < R; ++r) {
        if (n_nodes[r] > stride)
            return fail(ctx, TQ_ERR_INVALID_ARG, "%s: tree %lld: n_nodes exceeds the stride", who, (long long)r);
        const std::string err = cons_prepare(parents + r * stride, n_nodes[r], T, &recs[(size_t)r * S]);
        if (!err.empty()) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: tree %lld: %s", who, (long long)r, err.c_str());
    }
    return TQ_OK;
}

// One chunk of prepared trees on its way through tq_cons_mask_kernel: the page-locked staging buffer, the records, and
// the masks and keys the kernel writes.  The owner waits for the chunk before it stages the next one.
struct TreeChunk {
    int32_t T = 0, W = 0, G = 1;    // taxa, words of a mask, lanes that share a mask
    uint64_t tail = 0;              // valid bits of word W - 1
    int64_t chunk_trees = 0, chunks = 0;
    PinnedBuf<int32_t> p_trees;
    DevBuf<int32_t> d_trees;
    DevBuf<uint64_t> d_masks, d_keys;

    void shape(int64_t taxa)
    {
        T = (int32_t)taxa;
        W = (int32_t)((taxa + 63) / 64);
        tail = (taxa & 63) ? (uint64_t(1) << (taxa & 63)) - 1 : ~uint64_t(0);
        while (G < W) G *= 2;
    }
    int64_t nodes() const { return T - 2; }
    // as many trees as `scratch_bytes` (device + page-locked) hold, 1..most: per tree the masks, the keys, the record and
    // what the owner keeps beside them.  The device buffers; an owner allocates all its device memory, then
    // alloc_host() of its parts and its own page-locked memory (the order of the accumulators before they shared this:
    // with page-locked blocks between the device blocks a read of the tree distances measured 7 % slower,
    // profiles/bit_tile/README.md)
    hipError_t alloc(int64_t scratch_bytes, int64_t extra_bytes_per_tree, int64_t most = CONS_CHUNK_MAX)
    {
        const int64_t stride = cons_stride(T);
        const int64_t per_tree = nodes() * W * 8 + nodes() * 8 + stride * 4 + extra_bytes_per_tree;
        chunk_trees = std::max<int64_t>(1, std::min<int64_t>({CONS_CHUNK_MAX, scratch_bytes / per_tree, most}));
        hipError_t e = d_trees.alloc((size_t)(chunk_trees * stride));
        if (e == hipSuccess) e = d_masks.alloc((size_t)(chunk_trees * nodes() * W));
        if (e == hipSuccess) e = d_keys.alloc((size_t)(chunk_trees * nodes()));
        return e;
    }
    hipError_t alloc_host() { return p_trees.alloc((size_t)(chunk_trees * cons_stride(T))); }
    // the chunk's part of the kernel arguments, for n trees; keys of the full hash until a table says otherwise
    void fill(ConsArgs &p, int64_t n) const
    {
        p.trees = d_trees; p.masks = d_masks; p.keys = d_keys;
        p.items = n * nodes();
        p.T = T; p.W = W; p.G = G; p.hash_bits = 64; p.tail = tail;
    }
    // n <= chunk_trees records into the (free) staging buffer, to the device and through the mask kernel on `st`; a
    // launch failure shows in the owner's hipGetLastError
    hipError_t stage(int64_t n, const int32_t *recs, hipStream_t st, const ConsArgs &p)
    {
        const size_t bytes = (size_t)(n * cons_stride(T)) * 4;
        memcpy(p_trees, recs, bytes);
        const hipError_t e = hipMemcpyAsync(d_trees, p_trees, bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) hipLaunchKernelGGL(tq_cons_mask_kernel, dim3((unsigned)n), dim3(CONS_THREADS), 0, st, p);
        return e;
    }
};

// The split table of an accumulator: on the device the hash table of consensus.hpp, which numbers the distinct splits
// (its entries) from 0, on the host the exact map of the host back end, which with a context holds the splits that lost
// a hash collision on the device.  Both together never hold more than max_splits.
struct SplitTable {
    int64_t max_splits = 0;
    ConsMap host;
    bool overflow = false;          // more distinct splits than max_splits were offered: unusable until a reset
    // device back end
    int32_t W = 0;
    int hash_bits = 64;
    int64_t slots = 0, gather_cap = 0;
    DevBuf<unsigned long long> d_slot_key, d_count;
    DevBuf<int32_t> d_slot_idx;
    DevBuf<uint64_t> d_rep, d_gather;
    PinnedBuf<uint64_t> p_gather;
    DevBuf<unsigned int> d_ctr;
    PinnedBuf<unsigned int> p_ctr;  // the counters behind the last chunk
    DevBuf<uint32_t> d_unres;
    int64_t dev_entries = 0;        // entries of the device table after the last finished chunk
    int64_t unresolved = 0;

    // the device side for masks of `words` words and chunks of at most chunk_items (tree, node) pairs; max_splits is set.
    // Device buffers here, the page-locked ones in alloc_host(), as TreeChunk
    hipError_t alloc(const tq_ctx *ctx, int32_t words, int64_t chunk_items)
    {
        W = words;
        hash_bits = ctx->opt.cons_hash_bits;
        slots = 64;
        while (slots < 2 * max_splits) slots *= 2;
        gather_cap = std::max<int64_t>(1, CONS_GATHER_BYTES / (W * 8));
        hipError_t e = d_unres.alloc((size_t)chunk_items);
        if (e == hipSuccess) e = d_slot_key.alloc((size_t)slots);
        if (e == hipSuccess) e = d_slot_idx.alloc((size_t)slots);
        if (e == hipSuccess) e = d_rep.alloc((size_t)max_splits * W);
        if (e == hipSuccess) e = d_count.alloc((size_t)max_splits);
        if (e == hipSuccess) e = d_ctr.alloc(CONS_CTR_WORDS);
        if (e == hipSuccess) e = d_gather.alloc((size_t)gather_cap * W);
        return e;
    }
    hipError_t alloc_host()
    {
        const hipError_t e = p_gather.alloc((size_t)gather_cap * W);
        return e == hipSuccess ? p_ctr.alloc(CONS_CTR_WORDS) : e;
    }
    // the table's part of the kernel arguments
    void fill(ConsArgs &p) const
    {
        p.hash_bits = hash_bits;
        p.slot_key = d_slot_key; p.slot_idx = d_slot_idx; p.rep = d_rep; p.count = d_count; p.ctr = d_ctr;
        p.unres = d_unres; p.slot_mask = slots - 1; p.max_splits = max_splits;
    }
    // empty device table (also the reset): keys CONS_EMPTY (all bits set), slot entries -1, counts and counters 0
    int clear(tq_ctx *ctx)
    {
        TQ_HIP(ctx, hipMemset(d_slot_key, 0xFF, (size_t)slots * 8));
        TQ_HIP(ctx, hipMemset(d_slot_idx, 0xFF, (size_t)slots * 4));
        TQ_HIP(ctx, hipMemset(d_count, 0, (size_t)max_splits * 8));
        TQ_HIP(ctx, hipMemset(d_ctr, 0, CONS_CTR_WORDS * 4));
        TQ_HIP(ctx, hipDeviceSynchronize());
        return TQ_OK;
    }
    // everything a reset forgets; with a context behind clear(), and the hash width is read again
    void forget(const tq_ctx *ctx)
    {
        if (ctx) hash_bits = ctx->opt.cons_hash_bits;
        host.clear();
        dev_entries = unresolved = 0;
        overflow = false;
    }
    int overflowed(tq_ctx *ctx, const char *who)
    {
        overflow = true;
        return fail(ctx, TQ_ERR_INVALID_ARG, "%s: more than max_splits = %lld distinct splits; reset the accumulator", who,
                    (long long)max_splits);
    }
    // on `st` behind the chunk's kernels: no unresolved item yet / the counters to the host
    hipError_t begin_chunk(hipStream_t st) { return hipMemsetAsync(d_ctr + CONS_CTR_UNRES, 0, 4, st); }
    hipError_t end_chunk(hipStream_t st) { return hipMemcpyAsync(p_ctr, d_ctr, CONS_CTR_WORDS * 4, hipMemcpyDeviceToHost, st); }
    // Waits for the last chunk (masks in d_masks), reads its counters and hands its unresolved masks to the host:
    // on_mask(u, m) for the u-th unresolved item of the chunk, false when the map is full.  `nun` = how many there were.
    template <class OnMask>
    int drain(tq_ctx *ctx, const char *who, StreamOrder &order, const uint64_t *d_masks, int64_t &nun, OnMask on_mask)
    {
        nun = 0;
        if (!order.pending) return TQ_OK;
        TQ_HIP(ctx, order.sync());
        dev_entries = std::min<int64_t>((int64_t)p_ctr[CONS_CTR_CLAIMS], max_splits);
        if (p_ctr[CONS_CTR_OVERFLOW]) return overflowed(ctx, who);
        nun = (int64_t)p_ctr[CONS_CTR_UNRES];
        hipStream_t st = order.last;
        std::vector<uint64_t> m((size_t)W);
        for (int64_t first = 0; first < nun; first += gather_cap) {
            const int64_t n = std::min<int64_t>(gather_cap, nun - first);
            hipLaunchKernelGGL(tq_cons_gather_kernel, dim3((unsigned)((n * W + CONS_THREADS - 1) / CONS_THREADS)),
                               dim3(CONS_THREADS), 0, st, (const uint32_t *)d_unres, first, n, d_masks, W, d_gather.get());
            TQ_LAUNCHED(ctx, who);
            TQ_HIP(ctx, hipMemcpyAsync(p_gather, d_gather, (size_t)n * W * 8, hipMemcpyDeviceToHost, st));
            TQ_HIP(ctx, hipStreamSynchronize(st));
            for (int64_t e = 0; e < n; ++e) {
                m.assign(p_gather + e * W, p_gather + (e + 1) * W);
                if (!on_mask(first + e, m)) return overflowed(ctx, who);
            }
        }
        unresolved += nun;
        if (dev_entries + (int64_t)host.size() > max_splits) return overflowed(ctx, who);
        return TQ_OK;
    }
};
