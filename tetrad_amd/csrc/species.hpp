// species.hpp -- species-tree mode: per-species base counts and pooled count matrices of species quartets
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace).  DESIGN.md section 12.
#pragma once

// A species quartet (A, B, C, D) pools the full-mode count matrices of every lineage quartet (i in A, j in B, k in C,
// l in D).  The reference worker masks a site of a lineage quartet when a base is missing or the four bases are equal
// (resolve_quartets.py:216-223), so the pooled matrix factors over sites:
//   M[64x + 16y + 4z + w] = sum_s a_s[x] b_s[y] c_s[z] d_s[w],   bins x = y = z = w set to 0,
// where a_s[x] is the number of lineages of species A with base x at site s (a missing base counts nowhere).

// Species table, two layouts of the same counts: tab[k][s] = {n_A, n_C, n_G, n_T} of species k at site s, one byte
// each (a species holds <= 255 lineages), for the VALU form; tab8[k][x][s] = the count of base x as one byte (per-base
// planes), for the MFMA form.  0 for the pad sites s >= S.  One thread per (species, site); members[offsets[k] .. offsets[k+1]) are the
// samples of species k.  Reads the resident nibble rows with 4 = missing (common.hpp nib_offset / nib_shift).
__global__ void __launch_bounds__(256)
tq_species_table_kernel(const uint8_t *__restrict__ nib5, int64_t Sp, int64_t S, const int32_t *__restrict__ members,
                        const int32_t *__restrict__ offsets, int32_t K, uint32_t *__restrict__ tab,
                        uint8_t *__restrict__ tab8)
{
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)K * Sp) return;
    const int64_t k = gid / Sp, s = gid - k * Sp;
    uint32_t c = 0;
    if (s < S) {
        const int64_t off = nib_offset(s);
        const int sh = nib_shift(s);
        for (int32_t m = offsets[k]; m < offsets[k + 1]; ++m) {
            const uint32_t code = (nib5[(int64_t)members[m] * (Sp / 2) + off] >> sh) & 0xFu;
            c += code < 4 ? 1u << (8 * code) : 0u;
        }
    }
    tab[gid] = c;
#pragma unroll
    for (int x = 0; x < 4; ++x) tab8[(k * 4 + x) * Sp + s] = (uint8_t)((c >> (8 * x)) & 0xFFu);
}

// Allele mode (option species_alleles): the same table, both layouts, built from the IUPAC source
// matrix seqarr u8[T][S0] instead of the resident rows, with every sample as two haplotype lineages.  A cell adds 2 to
// its base when it is A / C / G / T (or an already recoded 0..3), 1 to each of its two bases when it is a two-base code
// (the table of tq_boot_build_kernel: R = G/A, K = G/T, S = G/C, Y = T/C, W = T/A, M = C/A) and nothing otherwise (N,
// gap, three-base codes).  No coin is drawn: the pooled matrix of these counts is the sum over haplotype quartets.
// {n_A, n_C, n_G, n_T} packed as in tab; the host admits at most 127 samples per species, so a byte holds 2n.
__device__ __forceinline__ uint32_t species_allele_counts(uint8_t v)
{
    constexpr uint32_t A = 1u, C = 1u << 8, G = 1u << 16, T = 1u << 24;
    switch (v) {
    case 0: case 65: return 2 * A;
    case 1: case 67: return 2 * C;
    case 2: case 71: return 2 * G;
    case 3: case 84: return 2 * T;
    case 82: return G + A;
    case 75: return G + T;
    case 83: return G + C;
    case 89: return T + C;
    case 87: return T + A;
    case 77: return C + A;
    default: return 0;
    }
}

// One thread per (species, padded site), as tq_species_table_kernel.  src_col[s] = the source column of replicate site
// s, the map tq_boot_perm_kernel left for the resident replicate (s < S <= its capacity, src_col[s] < S0).  Plain
// vector stores; no atomics, no LDS.
__global__ void __launch_bounds__(256)
tq_species_allele_table_kernel(const uint8_t *__restrict__ seqarr, int64_t S0, const uint32_t *__restrict__ src_col,
                               int64_t S, int64_t Sp, const int32_t *__restrict__ members,
                               const int32_t *__restrict__ offsets, int32_t K, uint32_t *__restrict__ tab,
                               uint8_t *__restrict__ tab8)
{
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)K * Sp) return;
    const int64_t k = gid / Sp, s = gid - k * Sp;
    uint32_t c = 0;
    if (s < S) {
        const uint8_t *col = seqarr + src_col[s];
        for (int32_t m = offsets[k]; m < offsets[k + 1]; ++m) c += species_allele_counts(col[(int64_t)members[m] * S0]);
    }
    tab[gid] = c;
#pragma unroll
    for (int x = 0; x < 4; ++x) tab8[(k * 4 + x) * Sp + s] = (uint8_t)((c >> (8 * x)) & 0xFFu);
}

// The row's own range rule: S x n_A n_B n_C n_D < 2^32.  The host refuses a call whose four largest species break it;
// a row that repeats a species can still break it, and such a row gets zero counts (TQ_FLAG_ZERO_DATA) instead of
// counts wrapped modulo 2^32.
__device__ __forceinline__ bool species_row_in_range(const int32_t *__restrict__ offsets, uint4 sq, int64_t S)
{
    const uint64_t p = (uint64_t)(offsets[sq.x + 1] - offsets[sq.x]) * (uint64_t)(offsets[sq.y + 1] - offsets[sq.y]) *
                       (uint64_t)(offsets[sq.z + 1] - offsets[sq.z]) * (uint64_t)(offsets[sq.w + 1] - offsets[sq.w]);
    return (uint64_t)S < (1ull << 32) && (uint64_t)S * p < (1ull << 32);
}

// Row write shared by both forms: the four waves' partial counts part[v][bin] are summed (u32, modulo 2^32), the
// invariant bins (x, x, x, x) -- lanes 0, 21, 42, 63, component w = x -- are masked, as every lineage quartet's site with
// four equal bases is (resolve_quartets.py:218), and wave 0 writes the row with 16-byte vector stores.
template <int NW>
__device__ __forceinline__ void species_write_row(uint32_t (*part)[256], int wave, int lane, uint32_t *cm_row)
{
    if (wave != 0) return;
    uint4 r = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int v = 0; v < NW; ++v) {
        const uint4 p = reinterpret_cast<const uint4 *>(part[v])[lane];
        r.x += p.x;
        r.y += p.y;
        r.z += p.z;
        r.w += p.w;
    }
    if (lane == 0) r.x = 0;
    if (lane == 21) r.y = 0;
    if (lane == 42) r.z = 0;
    if (lane == 63) r.w = 0;
    reinterpret_cast<uint4 *>(cm_row)[lane] = r;
}

// Pooled count kernel (VALU form): one workgroup of four waves per species quartet.  Lane l owns bins 4l .. 4l+3, i.e.
// (x, y, z) = (l >> 4, (l >> 2) & 3, l & 3) and w = 0..3; each wave walks a quarter of the sites, reading the four
// species' table entries with uniform (scalar) loads.  Per site and lane: three byte extracts, two 24-bit multiplies
// and four 24-bit multiply-adds.  All arithmetic is u32 modulo 2^32; the host's range rule (S x product of the four
// largest species sizes < 2^32) makes every bin's true value fit, so the sums are exact and independent of order.
// The four waves' partial sums meet in LDS; wave 0 writes the row of the count slab (u32 [Q][256], the layout the scan
// kernels write for tq_svd_dev) with 16-byte vector stores.  A row with a species id >= K gets zero counts (the score
// kernel flags it TQ_FLAG_BAD_INDEX).
constexpr int SPECIES_WAVES = 4;
constexpr int SPECIES_UNROLL = 16;          // sites per uniform load group (S is walked in multiples of it: the pad is 0)

__global__ void __launch_bounds__(WAVE * SPECIES_WAVES)
tq_species_pool_kernel(const uint32_t *__restrict__ tab, int64_t Sp, int64_t S, const uint32_t *__restrict__ squartets,
                       int64_t Q, int32_t K, const int32_t *__restrict__ offsets, uint32_t *__restrict__ cm)
{
    __shared__ __attribute__((aligned(16))) uint32_t part[SPECIES_WAVES][256];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sx = 8 * (lane >> 4), sy = 8 * ((lane >> 2) & 3), sz = 8 * (lane & 3);
    // the sites [0, Su) in SPECIES_UNROLL steps, dealt to the waves in contiguous pieces (Su <= Sp: the pad reads 0)
    const int64_t Su = (S + SPECIES_UNROLL - 1) / SPECIES_UNROLL * SPECIES_UNROLL;
    const int64_t per = ((Su + SPECIES_WAVES - 1) / SPECIES_WAVES + SPECIES_UNROLL - 1) / SPECIES_UNROLL * SPECIES_UNROLL;
    const int64_t s_lo = per * wave < Su ? per * wave : Su;
    const int64_t s_hi = s_lo + per < Su ? s_lo + per : Su;
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
        const uint4 sq = reinterpret_cast<const uint4 *>(squartets)[q];
        const uint32_t Ku = (uint32_t)K;
        uint32_t acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
        if ((sq.x < Ku) & (sq.y < Ku) & (sq.z < Ku) & (sq.w < Ku) && species_row_in_range(offsets, sq, S)) {
            const uint32_t *ta = tab + (int64_t)sq.x * Sp, *tb = tab + (int64_t)sq.y * Sp;
            const uint32_t *tc = tab + (int64_t)sq.z * Sp, *td = tab + (int64_t)sq.w * Sp;
            auto site = [&](uint32_t pa, uint32_t pb, uint32_t pc, uint32_t pd) {
                const uint32_t abc = __umul24(__umul24((pa >> sx) & 0xFFu, (pb >> sy) & 0xFFu), (pc >> sz) & 0xFFu);
                acc0 += __umul24(abc, pd & 0xFFu);
                acc1 += __umul24(abc, (pd >> 8) & 0xFFu);
                acc2 += __umul24(abc, (pd >> 16) & 0xFFu);
                acc3 += __umul24(abc, pd >> 24);
            };
            // (the loop vectoriser would turn the uniform loads into lane-spread ones moved by readlane / writelane)
#pragma clang loop vectorize(disable)
            for (int64_t s0 = s_lo; s0 < s_hi; s0 += SPECIES_UNROLL) {
                // 16-byte groups (rows start 8 KiB aligned, s0 is a multiple of 16): one scalar x4 load per species
#pragma unroll
                for (int j = 0; j < SPECIES_UNROLL / 4; ++j) {
                    const uint4 a = reinterpret_cast<const uint4 *>(ta + s0)[j], b = reinterpret_cast<const uint4 *>(tb + s0)[j];
                    const uint4 c = reinterpret_cast<const uint4 *>(tc + s0)[j], d = reinterpret_cast<const uint4 *>(td + s0)[j];
                    site(a.x, b.x, c.x, d.x);
                    site(a.y, b.y, c.y, d.y);
                    site(a.z, b.z, c.z, d.z);
                    site(a.w, b.w, c.w, d.w);
                }
            }
        }
        reinterpret_cast<uint4 *>(part[wave])[lane] = make_uint4(acc0, acc1, acc2, acc3);
        __syncthreads();
        species_write_row<SPECIES_WAVES>(part, wave, lane, cm + q * 256);
        __syncthreads();
    }
}

// Pooled count kernel (MFMA form, the default when every species holds <= 11 lineages): the pooled matrix is an integer
// GEMM over sites, M[4x+y][4z+w] = sum_s U[s][4x+y] V[s][4z+w] with U[s] = a_s (x) b_s and V[s] = c_s (x) d_s, so one
// v_mfma_i32_16x16x64_i8 adds 64 sites: lane l supplies row l & 15 of U^T (i.e. (x, y)) and column l & 15 of V (i.e.
// (z, w)) for the 16 sites of group g = l >> 4 of the step.  Which byte of the 16 holds which site does not matter as
// long as both operands use the same order (they do: both are built by the same code from the same table rows).  i8
// operands need n_A n_B <= 127 and n_C n_D <= 127, hence the size bound.  Per 64-site step a wave stages the 4 species
// x 4 bases x 64 sites of tab8 (1 KiB) in its own LDS piece -- lane l loads chunk (species l >> 4, base (l >> 2) & 3,
// site group l & 3) -- then each lane reads its four 16-byte chunks and multiplies them pairwise, two sites per
// v_pk_mul_lo_u16: the even bytes as they are, the odd bytes with one factor shifted into the high byte (every product
// is <= 127, so no product reaches the next byte).  The kernel is bound by the LDS reads (4 KiB per wave and step; with
// u16 counts it was 8 KiB and twice as slow).  One wave's LDS writes and reads are not reordered, so the
// piece needs no barrier.  The i32 accumulators (D layout: lane l, register r = bin 64 (l >> 4) + 16 r + (l & 15)) are
// drained into u32 sums every SPECIES_DRAIN steps, far below 2^31 (a step adds at most 64 x 127 x 127 < 2^20).
constexpr int SPECIES_MFMA_MAX = 11;        // largest species size the i8 operands take (11 x 11 = 121 <= 127)
constexpr int64_t SPECIES_DRAIN = 1024;

typedef int species_v4i __attribute__((ext_vector_type(4)));
typedef unsigned short species_us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t species_pk_mul(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(species_us2, a) * __builtin_bit_cast(species_us2, b));
}

// byte-wise products of four counts packed in a and b (each product <= 127)
__device__ __forceinline__ uint32_t species_bytes_mul(uint32_t a, uint32_t b)
{
    return species_pk_mul(a & 0x00FF00FFu, b & 0x00FF00FFu) | species_pk_mul(a & 0xFF00FF00u, (b >> 8) & 0x00FF00FFu);
}

__device__ __forceinline__ species_v4i species_frag(uint4 a, uint4 b)
{
    species_v4i f;
    f[0] = (int)species_bytes_mul(a.x, b.x);
    f[1] = (int)species_bytes_mul(a.y, b.y);
    f[2] = (int)species_bytes_mul(a.z, b.z);
    f[3] = (int)species_bytes_mul(a.w, b.w);
    return f;
}

__global__ void __launch_bounds__(WAVE * SPECIES_WAVES)
tq_species_mfma_kernel(const uint8_t *__restrict__ tab8, int64_t Sp, int64_t S, const uint32_t *__restrict__ squartets,
                       int64_t Q, int32_t K, const int32_t *__restrict__ offsets, uint32_t *__restrict__ cm)
{
    __shared__ uint4 stage[SPECIES_WAVES][WAVE];            // per wave: 64 chunks of 16 bytes
    __shared__ __attribute__((aligned(16))) uint32_t part[SPECIES_WAVES][256];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, i = lane & 15;
    // the chunks this lane's operands are made of: U = (A, x = i >> 2) x (B, y = i & 3), V = (C, z) x (D, w), group g
    const int cA = 4 * (i >> 2) + g, cB = 16 + 4 * (i & 3) + g, cC = 32 + 4 * (i >> 2) + g, cD = 48 + 4 * (i & 3) + g;
    uint4 *my = stage[wave];
    const int64_t steps = (S + 63) / 64;                    // 64-site steps (<= Sp / 64: the pad reads 0)
    const int64_t per = (steps + SPECIES_WAVES - 1) / SPECIES_WAVES;
    const int64_t st_lo = per * wave < steps ? per * wave : steps;
    const int64_t st_hi = st_lo + per < steps ? st_lo + per : steps;
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
        const uint4 sq = reinterpret_cast<const uint4 *>(squartets)[q];
        const uint32_t Ku = (uint32_t)K;
        uint32_t tot[4] = {0, 0, 0, 0};
        if ((sq.x < Ku) & (sq.y < Ku) & (sq.z < Ku) & (sq.w < Ku) && species_row_in_range(offsets, sq, S)) {
            const uint32_t ld_sp = lane >> 4 == 0 ? sq.x : lane >> 4 == 1 ? sq.y : lane >> 4 == 2 ? sq.z : sq.w;
            const uint4 *src = reinterpret_cast<const uint4 *>(tab8 + ((int64_t)ld_sp * 4 + ((lane >> 2) & 3)) * Sp +
                                                               16 * (lane & 3));
            uint4 n0 = make_uint4(0, 0, 0, 0);                  // the next step's chunk, loaded one step ahead
            if (st_lo < st_hi) n0 = src[4 * st_lo];
            for (int64_t d0 = st_lo; d0 < st_hi; d0 += SPECIES_DRAIN) {
                const int64_t d1 = d0 + SPECIES_DRAIN < st_hi ? d0 + SPECIES_DRAIN : st_hi;
                species_v4i acc = {0, 0, 0, 0};
                for (int64_t st = d0; st < d1; ++st) {
                    my[lane] = n0;
                    const int64_t nx = st + 1 < st_hi ? st + 1 : st;
                    n0 = src[4 * nx];
                    __builtin_amdgcn_wave_barrier();        // the other lanes' chunks: no code motion across it
                    const species_v4i u = species_frag(my[cA], my[cB]);
                    const species_v4i v = species_frag(my[cC], my[cD]);
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(u, v, acc, 0, 0, 0);
                    __builtin_amdgcn_wave_barrier();        // this step's reads stay before the next step's writes
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) tot[r] += (uint32_t)acc[r];
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][64 * g + 16 * r + i] = tot[r];
        __syncthreads();
        species_write_row<SPECIES_WAVES>(part, wave, lane, cm + q * 256);
        __syncthreads();
    }
}
