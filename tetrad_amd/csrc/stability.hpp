// stability.hpp -- quartet frequencies of a set of trees and the per-taxon sums of the leaf stability index
// (DESIGN.md section 28).  No reference counterpart.
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace, behind qdist.hpp, whose
// codes, planes and encode kernel it reuses unchanged).
//
// One rule, executed on the host and on the device, integers only.  Over the N trees held, for a quartet row (a, b, c, d)
// as given:
//   counts    n_k = the trees whose `qd_code` of the row is k (0 = ab|cd, 1 = ac|bd, 2 = ad|bc), n_3 = N - n_0 - n_1 - n_2
//             (unresolved); the row u16 [4] = (n_0, n_1, n_2, n_3) sums to N <= 8192.
//   measures  `ls_row`: top = max(n_0, n_1, n_2), second = the second largest of the three (= top when the largest is
//             tied), dif = top - second, res = n_0 + n_1 + n_2.
//   acc       u64 [T][4] = (quartets, res, top, dif): the sums over every scored row that holds taxon t; a row given twice
//             counts twice.
// A permutation of the taxa inside a row permutes n_0..n_2 and moves none of top, dif, res; any chunking of quartets, any
// launch shape and any order of score calls add the same integers.
//
//   tq_ls_count_kernel    behind tq_qd_encode_kernel on the planes [N][3][cw] of a chunk.  One workgroup of 256 threads per
//                         group of LS_GROUP_WORDS = 16 consecutive plane words (128 bytes of every plane row, 1 024
//                         quartets); a wave owns 4 of the words, lane l of it quartet 64 w + l of each.  The trees are
//                         walked in tiles of LS_TILE: all threads stage [tile][3][16 words] into LDS (words past cw and
//                         trees past N as zero), then per staged tree and plane a lane reads its wave's word (one LDS
//                         address per wave: a broadcast), takes bit l and adds it to one of three u32 registers per word.
//                         Behind the last tile a lane with a quartet < nq stores the counts row as one 8-byte vector store
//                         (where a counts array was asked for) and adds (1, res, top, dif) to the four taxa of its row in
//                         a per-workgroup LDS accumulator u64 [T][4] with LDS integer atomics; after a barrier the threads
//                         add every non-zero entry to the global acc with the u64 integer atomicAdd.
// All LDS is dynamic (staging tile + accumulator, sized by T: 6 KiB + 32 T bytes), so small T keeps its occupancy and
// the base stays 16-byte aligned.  u64 in LDS: no overflow bound has to be argued.
// No float, no inline assembly, no loop that waits on another lane or workgroup; every loop is bounded by N, T, the
// words of a group or a constant.
#pragma once

constexpr int LS_THREADS = 256;
constexpr int LS_GROUP_WORDS = 16;          // plane words a workgroup owns
constexpr int LS_WAVE_WORDS = LS_GROUP_WORDS / (LS_THREADS / 64);
constexpr int LS_TILE = 16;                 // trees staged per pass (unmeasured): 16 x 3 x 16 words = 6 KiB, 3 words a thread
constexpr int LS_TILE_WORDS = LS_TILE * 3 * LS_GROUP_WORDS;

struct LsRow {
    uint32_t res, top, dif;
};

// the measures of one counts row
__host__ __device__ __forceinline__ LsRow ls_row(uint32_t n0, uint32_t n1, uint32_t n2)
{
    const uint32_t hi01 = n0 > n1 ? n0 : n1, lo01 = n0 > n1 ? n1 : n0;
    LsRow r;
    r.top = hi01 > n2 ? hi01 : n2;
    const uint32_t second = hi01 > n2 ? (lo01 > n2 ? lo01 : n2) : hi01;
    r.dif = r.top - second;
    r.res = n0 + n1 + n2;
    return r;
}

// Host execution: the planes P [N][3][cw] of `nq` quartets q (u32 [nq][4]) summed along the trees, a loop over the bits;
// counts (u16 [nq][4]) may be NULL
inline void ls_host_count(const uint64_t *P, int64_t N, int64_t cw, const uint32_t *q, int64_t nq, uint16_t *counts, uint64_t *acc)
{
    for (int64_t i = 0; i < nq; ++i) {
        const int64_t w = i >> 6;
        const int b = (int)(i & 63);
        uint32_t n[3] = {0, 0, 0};
        for (int64_t t = 0; t < N; ++t)
            for (int k = 0; k < 3; ++k) n[k] += (uint32_t)((P[(t * 3 + k) * cw + w] >> b) & 1u);
        const LsRow r = ls_row(n[0], n[1], n[2]);
        if (counts) {
            counts[4 * i] = (uint16_t)n[0];
            counts[4 * i + 1] = (uint16_t)n[1];
            counts[4 * i + 2] = (uint16_t)n[2];
            counts[4 * i + 3] = (uint16_t)((uint32_t)N - r.res);
        }
        for (int k = 0; k < 4; ++k) {
            uint64_t *a = acc + 4 * (size_t)q[4 * i + k];
            a[0] += 1;
            a[1] += r.res;
            a[2] += r.top;
            a[3] += r.dif;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Device path
// ---------------------------------------------------------------------------------------------
struct LsCountArgs {
    const uint4 *quartets;      // [nq] four distinct taxa < T each
    const uint64_t *planes;     // [N][3][cw]
    uint2 *counts;              // [nq] rows of u16 x 4, or NULL
    unsigned long long *acc;    // [T][4]
    int64_t nq;                 // quartets of the chunk
    int32_t cw;                 // words of the chunk, (nq + 63) / 64
    int32_t N;                  // trees
    uint32_t T;
};

// grid ((cw + 15) / 16); dynamic LDS (LS_TILE_WORDS + 4 T) * 8 bytes
__global__ __launch_bounds__(LS_THREADS) void tq_ls_count_kernel(LsCountArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_ls[];
    unsigned long long *s_tile = s_ls;                      // [LS_TILE][3][LS_GROUP_WORDS]
    unsigned long long *s_acc = s_ls + LS_TILE_WORDS;       // [T][4]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nacc = a.T * 4;
    const int64_t w0 = (int64_t)blockIdx.x * LS_GROUP_WORDS;
    for (uint32_t i = tid; i < nacc; i += LS_THREADS) s_acc[i] = 0;

    uint32_t n[LS_WAVE_WORDS][3];
#pragma unroll
    for (int k = 0; k < LS_WAVE_WORDS; ++k) n[k][0] = n[k][1] = n[k][2] = 0;

    for (int32_t t0 = 0; t0 < a.N; t0 += LS_TILE) {
        __syncthreads();                                    // the tile of the pass before has been read
#pragma unroll
        for (int i = 0; i < LS_TILE_WORDS / LS_THREADS; ++i) {
            const uint32_t e = tid + (uint32_t)i * LS_THREADS;      // = (row of the tile) * 16 + word: 128-byte row segments
            const int64_t row = (int64_t)t0 * 3 + (e >> 4), w = w0 + (e & 15u);
            s_tile[e] = (row < (int64_t)a.N * 3 && w < a.cw) ? a.planes[row * a.cw + w] : 0ull;
        }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < LS_TILE; ++t)
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int k = 0; k < LS_WAVE_WORDS; ++k)
                    n[k][p] += (uint32_t)(s_tile[(t * 3 + p) * LS_GROUP_WORDS + wave * LS_WAVE_WORDS + k] >> lane) & 1u;
    }
    __syncthreads();                                        // s_acc is zero everywhere (also with no tree at all)

#pragma unroll
    for (int k = 0; k < LS_WAVE_WORDS; ++k) {
        const int64_t q = (w0 + wave * LS_WAVE_WORDS + k) * 64 + lane;
        if (q >= a.nq) continue;
        const LsRow r = ls_row(n[k][0], n[k][1], n[k][2]);
        if (a.counts) a.counts[q] = make_uint2(n[k][0] | (n[k][1] << 16), n[k][2] | (((uint32_t)a.N - r.res) << 16));
        const uint4 x = a.quartets[q];
        const uint32_t taxa[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned long long *s = s_acc + 4 * taxa[j];
            atomicAdd(s, 1ull);
            if (r.res) atomicAdd(s + 1, (unsigned long long)r.res);
            if (r.top) atomicAdd(s + 2, (unsigned long long)r.top);
            if (r.dif) atomicAdd(s + 3, (unsigned long long)r.dif);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < nacc; i += LS_THREADS) {     // integer adds: exact in any order
        const unsigned long long v = s_acc[i];
        if (v) atomicAdd(&a.acc[i], v);
    }
}
