/*
 * tetrad_hip.h -- C ABI of the MI355X (gfx950) quartet-invariant engine.
 *
 * This is the drop-in boundary for tetrad's per-chunk worker.  Each entry point
 * cites the reference interface it replaces (paths relative to the reference
 * checkout).  The reference is pure Python, so "the FFI a maintainer would
 * bind" is ctypes; the binding is shown in INTEGRATION.md and shipped as
 * tetrad_amd/_lib.py.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.
 *   - every function returns TQ_OK (0) or a negative TQ_ERR_* code; it never
 *     throws and never aborts.  tq_last_error() returns a human-readable
 *     message for the last failure on that context (or the last failure of
 *     tq_create when ctx is NULL).
 *   - one context per (process, device).  A context is not thread-safe;
 *     distinct contexts are independent.  The library keeps no host pointer
 *     after a call returns.
 *   - host-buffer entry points (tq_set_data, tq_resolve, tq_resolve_to_host,
 *     tq_resolve_debug) are synchronous: results are in the caller's arrays on
 *     return.  Inside, kernels and copies run on the context's own streams and the
 *     result D2H of one piece overlaps the kernels of the next.  *_dev entry points
 *     take device pointers, enqueue on the given HIP stream and return without
 *     synchronising.
 *   - stream rule: the *_dev entry points of one context share its device scratch (count slab,
 *     ordering and singular-value scratch, the replicate's layout).  The library orders them in CALL
 *     order whatever their streams: a call on another stream than the previous *_dev call first makes
 *     its stream wait for that call's work, and a host-buffer call waits for every *_dev call made
 *     before it.  What the library cannot see is the caller's own use of the OUTPUT arrays of a *_dev
 *     call: read them on the stream they were produced on, or after synchronising with it.
 */
#ifndef TETRAD_HIP_H
#define TETRAD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tq_ctx tq_ctx;

enum {
    TQ_OK = 0,
    TQ_ERR_INVALID_ARG = -1,   /* NULL pointer, negative size, taxon index >= T ... */
    TQ_ERR_NO_DEVICE = -2,     /* no HIP device / device is not usable             */
    TQ_ERR_HIP = -3,           /* a HIP runtime call failed (see tq_last_error)    */
    TQ_ERR_NO_DATA = -4,       /* tq_resolve* before tq_set_data                   */
    TQ_ERR_LOCUS_ORDER = -5,   /* subsample requested but a locus id re-appears
                                  after its run ended (see tq_set_data)            */
    TQ_ERR_OOM = -6
};

/* per-quartet flag bits written by tq_resolve* */
enum {
    TQ_FLAG_ZERO_DATA = 1,     /* no site counted: scores are 0.001, topology 0.
                                  (reference: unseeded np.random.randint(3),
                                  resolve_quartets.py:230-232)                      */
    TQ_FLAG_DEGENERATE = 2,    /* two lowest scores within 1e-9 * sigma_max: argmin is
                                  decided by SVD rounding noise in any implementation */
    TQ_FLAG_BAD_INDEX = 4,     /* a taxon index was >= T; row treated as zero-data   */
    TQ_FLAG_NO_CONVERGENCE = 8, /* a singular-value iteration hit its sweep cap; the row holds the
                                  unconverged values (reference: np.linalg.svd raises LinAlgError,
                                  resolve_quartets.py:242; the Python mirror raises it too)   */
    TQ_FLAG_INVALID_DIAGNOSTIC = 16 /* the row was made while a timing-diagnostic mode was set (tq_set_option
                                  "scan_method" 2..5 or "phases" 1 / 2): it is NOT a result.  Set on every row of
                                  such a call; a call without a flags array fails while such a mode is set; the
                                  Python mirror raises.                                        */
};

/* Create / destroy a context bound to HIP device `device_id`.
 * Replaces: the per-engine process state of the reference (an ipyparallel
 * engine that re-opens the HDF5 file on every call, resolve_quartets.py:33-35). */
int tq_create(tq_ctx **out, int device_id);
void tq_destroy(tq_ctx *ctx);
const char *tq_last_error(const tq_ctx *ctx);

/* Upload one replicate's genotype matrix and locus column (H2D once per
 * replicate, not once per chunk).
 * Replaces: `tmparr = io5["tmparr"][:]; tmpmap = io5["tmpmap"][:]`
 *           (resolve_quartets.py:33-35) and the `tmpmap[:, 0]` argument of
 *           resolve_quartets.py:221,223.
 *   tmparr  u8 [T,S] row-major; 0..3 = A,C,G,T; anything > 3 (78 = N) is missing
 *   locus   u32, element i at locus[i * locus_stride]  (pass tmpmap and stride 2
 *           to use tmpmap[:,0] without a copy)
 * Subsample mode requires every locus id to occupy one contiguous run of sites
 * (always true for the reference's writers: write_database.py:138-149,
 * jit/resample.py:58) and no id equal to 0xFFFFFFFF; otherwise tq_resolve*
 * with subsample != 0 returns TQ_ERR_LOCUS_ORDER.                                  */
int tq_set_data(tq_ctx *ctx, const uint8_t *tmparr, int64_t T, int64_t S,
                const uint32_t *locus, int64_t locus_stride);

/* Bootstrap replicates built on the device.
 * tq_set_source uploads, once per project, what the reference keeps in its HDF5 database for
 * resampling: `seqarr` (u8 [T,S0], ASCII bases incl. IUPAC two-base codes, N/'-' = missing;
 * write_database.py:157-159) and `spans` (i64 [nloci,2], [start,end) columns of each locus;
 * jit/get_spans.py:11-48).
 * tq_bootstrap replaces resample_tmp_database (run_inference.py:99-143): loci `lidxs` (host,
 * i64 [nloci], values in [0,nloci); the reference draws them with rng.choice(nloci, nloci,
 * replace=True) at :117) are concatenated with their columns shuffled (jit/resample.py:20-64),
 * IUPAC codes are resolved at random per cell (jit/resolve_ambigs.py:12-36), bases are recoded
 * 0..3 (:133-136) and the device layout is rebuilt -- the result is the resident replicate, as if
 * tq_set_data had been called with the resampled tmparr/tmpmap.  The two seeds take the place of
 * the two rng.integers(2**31) draws (:120,:123); the streams behind them are this engine's own
 * (counter-based), so replicates are distributed like the reference's, not identical to them.
 * *out_S receives the replicate's number of sites.
 * tq_get_data copies the resident replicate back in the reference's layout (tmparr u8 [T,S] with
 * 0..3 and 78 = missing; tmpmap u32 [S,2] = {locus ordinal, site index}); tq_data_shape gives T,S. */
int tq_set_source(tq_ctx *ctx, const uint8_t *seqarr, int64_t T, int64_t S0,
                  const int64_t *spans, int64_t nloci);
int tq_bootstrap(tq_ctx *ctx, const int64_t *lidxs, int64_t n, uint64_t seed_shuffle,
                 uint64_t seed_ambig, int64_t *out_S);
/* Same, enqueued on `stream` without waiting (the replicate length is computed on the host from the
 * spans): the replicate of iteration k+1 is built right behind the kernels of iteration k.  It is a
 * *_dev call under the stream rule above: the library orders it behind the *_dev calls made before it
 * and every later call of this context -- *_dev on any stream, or host-buffer -- behind it; the caller
 * adds no event (tests/test_gpu_stream_rule.py holds the build back and checks each consumer).          */
int tq_bootstrap_async(tq_ctx *ctx, const int64_t *lidxs, int64_t n, uint64_t seed_shuffle,
                       uint64_t seed_ambig, int64_t *out_S, void *stream);
int tq_get_data(tq_ctx *ctx, uint8_t *tmparr, uint32_t *tmpmap);
int tq_data_shape(tq_ctx *ctx, int64_t *T, int64_t *S);

/* Resolve Q quartets (host buffers, synchronous).
 * Replaces: new_infer_resolved_quartets(tmparr, tmpmap, quartets, subsample_snps)
 *           (resolve_quartets.py:191-265), which returns (quartets, rstat, rscor).
 *   quartets u32 [Q,4]  taxon indices (returned unchanged by the reference, :265)
 *   rstat    u32 [Q,2]  out: [:,0] topology 0/1/2 (argmin of scores, :251),
 *                            [:,1] number of counted sites (:226,:264)
 *   rscor    f64 [Q,3]  out: invariant score of the three flattenings (:246-248)
 *   flags    u8  [Q]    out, may be NULL: TQ_FLAG_* bits                           */
int tq_resolve(tq_ctx *ctx, const uint32_t *quartets, int64_t Q, int subsample,
               uint32_t *rstat, double *rscor, uint8_t *flags);

/* Page-locked host memory from a process-wide pool (blocks are recycled: pinning pages costs about
 * as much as a resolve call).  Result arrays (and quartet arrays) that live in such a block -- or in
 * any other page-locked memory -- are read / written by the copy engine directly, asynchronously under
 * the kernels; pageable arrays work too, through pinned staging pieces and one host memcpy per piece.
 * Blocks are independent of any context and may outlive it.  No reference counterpart (the reference
 * returns fresh NumPy arrays, resolve_quartets.py:253-265; the ctypes binding wraps such blocks as NumPy
 * arrays).                                                                                       */
int tq_host_alloc(int64_t bytes, void **out);
int tq_host_free(void *p);

/* Quartets already on the device, results to host arrays (synchronous): what bench.py times as one
 * step -- inputs resident in HBM, result D2H inside the step.
 * Replaces: the same function as tq_resolve.                                                     */
int tq_resolve_to_host(tq_ctx *ctx, const uint32_t *d_quartets, int64_t Q, int subsample,
                       uint32_t *rstat, double *rscor, uint8_t *flags);

/* Same, device pointers in and out, asynchronous on `stream` (a hipStream_t; NULL = the
 * default stream).                                                                        */
int tq_resolve_dev(tq_ctx *ctx, const uint32_t *d_quartets, int64_t Q, int subsample,
                   uint32_t *d_rstat, double *d_rscor, uint8_t *d_flags, void *stream);

/* Full-mode quartet generation on the device: resolves the quartets whose
 * lexicographic ranks are [first_rank, first_rank+Q) among C(T,4), i.e. what
 * islice(combinations(range(T),4), start, end) yields (combinations.py:40-55),
 * without any quartet H2D.  d_quartets (u32[Q,4], may be NULL) receives them.
 * TQ_ERR_INVALID_ARG when the range does not end at or below C(T,4), or T > 145 056
 * (see tq_unrank).                                                                 */
int tq_resolve_range_dev(tq_ctx *ctx, uint64_t first_rank, int64_t Q, int subsample,
                         uint32_t *d_quartets, uint32_t *d_rstat, double *d_rscor,
                         uint8_t *d_flags, void *stream);

/* The two stages of tq_resolve_dev as separate calls, for callers that ship results in pieces (the
 * multi-GPU path gathers and copies piece i while piece i+1 is computed):
 *   tq_scan_dev  orders and scans quartets [0,Q) into the context's count slab (Q <= option "batch");
 *   tq_svd_dev   turns rows [q0, q0+n) of that scanned batch into results; d_rstat / d_rscor / d_flags
 *                point at the outputs OF ROW q0 (so pieces can live in separate slabs).
 * Both enqueue on `stream`.  Replaces: the two halves of new_infer_resolved_quartets
 * (resolve_quartets.py:208-226 and :236-251).                                                    */
int tq_scan_dev(tq_ctx *ctx, const uint32_t *d_quartets, int64_t Q, int subsample, void *stream);
int tq_svd_dev(tq_ctx *ctx, int64_t q0, int64_t n, uint32_t *d_rstat, double *d_rscor,
               uint8_t *d_flags, void *stream);

/* Random-mode quartet generation on the device: unranks host-sampled
 * lexicographic ranks (combinations.py:94-114) into d_quartets.  The ranks are on
 * the device and are not checked: each must be below C(T,4).  T > 145 056 is
 * TQ_ERR_INVALID_ARG (see tq_unrank).                                              */
int tq_unrank_dev(tq_ctx *ctx, const uint64_t *d_ranks, int64_t Q, uint32_t *d_quartets,
                  void *stream);

/* Opt-in quartet sampler on the device: Q DISTINCT quartets drawn uniformly from the C(T,4) of the resident
 * (or source) matrix, in random order, written to d_quartets (u32[Q,4]) and -- if d_ranks is not NULL -- their
 * lexicographic ranks to d_ranks (u64[Q]).  Same distribution as
 * random_combination_sample_via_index (combinations.py:109-114: rng.choice(C(T,4), size, replace=False)
 * + unranking) but NOT the project Generator's stream (a keyed permutation of the rank space,
 * counter-based): for runs that do not need to reproduce a reference run's sample.  Element i of the sample
 * depends on (seed, T, i) alone (a call with a smaller Q returns a prefix); tests/rank_model.py states it in
 * Python integers.  TQ_ERR_INVALID_ARG when Q > C(T,4) or T > 145 056 (see tq_unrank).            */
int tq_sample_quartets_dev(tq_ctx *ctx, uint64_t seed, int64_t Q, uint64_t *d_ranks,
                           uint32_t *d_quartets, void *stream);

/* Kernel-level outputs for parity tests (host buffers, synchronous); any of the
 * debug pointers may be NULL.
 * Replaces: subsample_chunk_to_matrices / full_chunk_to_matrices
 *           (resolve_quartets.py:42-104) -> cmats u32[Q,3,16,16];
 *           np.linalg.svd(...)[1] (:242) -> svds f64[Q,3,16] (descending);
 *           np.linalg.matrix_rank (:243) -> ranks i32[Q,3].                        */
int tq_resolve_debug(tq_ctx *ctx, const uint32_t *quartets, int64_t Q, int subsample,
                     uint32_t *rstat, double *rscor, uint8_t *flags,
                     uint32_t *cmats, double *svds, int32_t *ranks);

/* HIP-event timing of the two resolve kernels, on the stream they were launched on.
 * tq_timing_enable(ctx, 1) makes every subsequent resolve call record HIP events
 * around its kernels; tq_timing_read synchronises those events, returns the summed
 * kernel milliseconds and the number of resolve calls since the last reset, and resets. */
int tq_timing_enable(tq_ctx *ctx, int on);
int tq_timing_read(tq_ctx *ctx, double *kernel_ms, int64_t *launches);
/* Same, split by kernel: total = scan + svd milliseconds summed over the `calls` resolve calls
 * made since the last read (a resolve call launches one scan + one SVD kernel per batch).     */
int tq_timing_read_split(tq_ctx *ctx, double *total_ms, double *scan_ms, double *svd_ms, int64_t *calls);
/* Same, per kernel: ms[0] ordering (key + radix sort), ms[1] site scan, ms[2] bidiagonalisation (or the
 * whole Jacobi kernel with svd_method 0), ms[3] bidiagonal QR, ms[4] scores; entries beyond n_ms are
 * not written, entries beyond 4 are set to 0.                                                    */
int tq_timing_read_kernels(tq_ctx *ctx, double *ms, int n_ms, int64_t *calls);

/* Tuning / diagnostic knobs (value 0 = library default unless noted).  Returns TQ_OK or an error.
 * Names: nrep, waves_per_cu, wg_min_quartets (batches below it -- default 4096 -- are scanned by the one-wave-per-quartet kernel:
 * small calls are latency-bound), batch (quartets per internal batch, default 2^23; device scratch is about
 * 3.2 KB per quartet of the largest batch resolved so far), order, scan_wg (waves per scan workgroup: 1, 2, 4, 8, 16), scan_method (-1 auto), svd_method (0 Jacobi,
 * 1 Householder+QR), bidiag_layout (1, default: the bidiagonalisation deals a matrix 2 x 2 over four lanes; 0: four column
 * groups), xcd_remap (1: scan workgroups of one XCD take a contiguous part of the sorted order),
 * svd_wpc (blocks per CU of the singular-value grids, 0 = one pass per block), svd_chunk (quartets per
 * pass of the singular-value stage = per result-copy piece, default 2^18), svd_streams (1 or 2: chunks alternate
 * between two streams so that one chunk's tail is filled by the next chunk; default 2), share_c (1: scan variant that also shares row c inside a
 * workgroup; measured slower, off), park_t (1, default: transposed, bank-conflict-free pattern park of the set-bit walk; 0: lane-
 * contiguous park), scan_pair (1: two quartets per wavefront; measured slower, off), count_invariant (1: sites whose four bases
 * are equal are counted too -- what the reference's count kernels do when their caller's mask leaves such a site open,
 * resolve_quartets.py:59-64; one-wave kernel), bdsqr_maxit (QR sweeps per singular value before TQ_FLAG_NO_CONVERGENCE,
 * default 60), bdsqr_stats (1: count rotation steps / issued lane-slots, read with tq_debug_fetch which = 3), phases
 * (timing diagnostics), species_method (-1 auto, 0 VALU, 1 MFMA form of the species-mode pooled counts), species_alleles
 * (0 / 1: species mode reads both alleles of the IUPAC source, see the species section below).  scan_method 2..5 and phases 1 / 2 are timing diagnostics whose rows are wrong: every row of a
 * call made under them carries TQ_FLAG_INVALID_DIAGNOSTIC and a call without a flags array fails.  scan_method 6 = the
 * bank-private counter kernel (scan_pb.hpp; an A/B form, slower).  batch is clamped to 2^31 - 1.
 * scan_dp (1, default: full-mode batches -- subsample = 0 -- of at least dp_min_quartets go to the joint-histogram scan,
 * scan_dp.hpp: two quartets that share their first three taxa per wavefront, one LDS atomic per site and pair; the same rows,
 * bit for bit; 0: always one quartet per wavefront), dp_min_quartets (default 32 768; smaller batches are not sorted and hold
 * few pairs), scan_f4 (-1, default: in subsample mode the cooperative scan streams a wavefront's own rows as 12-byte
 * {missing, bit 0, bit 1} records only and makes the pattern of a counted site inside the histogram walk, scan_f4.hpp =
 * SURVEY 8 row f4; 1: in full mode too (slower there); 0: the nibble-code kernel of rounds 1-3 everywhere; NOTE: 0 is a value
 * of its own for this option, the default is -1).
 * site_pack (-1, default; read by tq_set_data): the subsample-mode scans read a second resident copy of the matrix in which
 * every 32-site lane word holds whole loci and the 64 words of a step hold the same number of them (tq_pack_sites below), so
 * a wavefront's set-bit walk makes that many trips per step instead of the most any of 64 arbitrary windows holds; the same
 * rows, bit for bit.  -1: built when the predicted instruction count of the scan falls (dense matrices; not for sparse
 * RAD-like ones, where the walk is short anyway and only the extra steps would cost -- no second copy is made then);
 * 1: always built; 0: never built, and a copy already built is no longer used (-1 / 1 set after tq_set_data take effect
 * with the next one).  Full mode, species mode and tq_get_data use the natural layout.
 * NOTE: 0 is a value of its own for this option, the default is -1.
 * boot_pack (0, default; read by tq_bootstrap / tq_bootstrap_async): whether a device-built bootstrap replicate gets a
 * packed copy too.  0: the replicate keeps the natural layout only, and a packed copy left by tq_set_data goes stale;
 * 1: every replicate is packed -- the host plans the packed order from the widths of the drawn loci (no work per site, no
 * device round trip: the call stays asynchronous), the packed start of every draw goes to the device with the locus indices
 * and two more kernels build the copy right behind the natural one on the same stream; the same rows, bit for bit;
 * -1: packed when the automatic rule of site_pack = -1 took the packed layout for the SOURCE (decided once, in
 * tq_set_source, on the loci of the source with a two-base IUPAC code counted as present: a replicate resamples those
 * loci, so their statistics are the replicate's).  site_pack = 0 keeps its meaning: no packed copy is read, and none is
 * built for replicates either.                                                                                      */
int tq_set_option(tq_ctx *ctx, const char *name, int64_t value);

/* Test hook: copy the scratch of the last resolve call to the host.  which = 0: count slab
 * u32[n][256] of the last scan batch; 1: bidiagonals f64[3m][32] (d[16], e[16]); 2: singular values
 * f64[3m][16] (unsorted, sign bit = not converged), m = quartets of the last singular-value chunk; 3: the 8 u64 counters
 * of option bdsqr_stats; 4: two i64 about the packed layout set of option site_pack: its padded site count (0 = none is
 * resident) and 1 if a subsample-mode scan issued now would read it; 5: the site order of the packed copy of the current
 * device-built replicate (option boot_pack) as u32[that padded site count] -- entry p = the replicate's site at packed
 * position p or 0xFFFFFFFF for a pad, what tq_pack_sites gives for the replicate's tmpmap -- TQ_ERR_INVALID_ARG when the
 * current packed copy was not built by tq_bootstrap or is stale; 6: three i64 about the most recent scan launch of the
 * context, recorded where the launch is decided: the kernel form (0 none yet, 1 tq_scan_kernel, 2 tq_scan_wg_kernel,
 * 3 tq_scan_wg2_kernel, 4 tq_scan_f4_kernel, 5 tq_scan_pb_kernel, 6 tq_scan_dp_kernel), T * pitch of the layout set it
 * read (the cooperative forms 2-6 address that set with 32-bit byte offsets and are chosen only below 0xFFFF0000) and 1
 * if that set was the packed one, else 0.  No reference counterpart.                                                */
int tq_debug_fetch(tq_ctx *ctx, int which, void *dst, int64_t bytes);

/* Test hook: the scan kernel the library would launch, for n rows of options and batch shape (host code: no context, no
 * device).  rows i64[n][22]: the options scan_pair, scan_wg, scan_method, scan_f4, scan_dp, park_t, share_c,
 * count_invariant, waves_per_cu, nrep, order, wg_min_quartets, dp_min_quartets as the context holds them (defaults
 * resolved: tq_set_option's 0 = default is not applied here), pb_ok (1: the start-up probe of tq_scan_pb_kernel passed, as
 * on every device so far; -1: it failed), xcd_remap, the CU count; then T, the padded sites per row of the layout set
 * the scan reads, the same of the natural set, Q, subsample, and 1 if the quartets arrive in sorted order.
 * plans i64[n][12]: the kernel form (as tq_debug_fetch which = 6), the kernel's template arguments SUB, METHOD, NW, SHC,
 * PARK_T, NREP (0 where the form's kernel has no such argument), quartets per workgroup, threads per workgroup, grid
 * (0: the one-wave form sizes it by the occupancy query at launch), xcd_chunk, and the row of the library's table of
 * scan instantiations that holds this kernel (-1: none is built -- a launch would fail).  *n_kernels (may be NULL)
 * gets the number of rows of that table.  It is the function the launch itself calls.
 * No reference counterpart.                                                                                          */
int tq_scan_plan(const int64_t *rows, int64_t n, int64_t *plans, int64_t *n_kernels);

/* Test hook: run the bidiagonal-QR kernel (tq_bdsqr_kernel) alone on nmat bidiagonals given on the host -- de f64[nmat][32]
 * as tq_debug_fetch(which = 1) hands them out, in ANY order: lane i of wave w gets matrix 64 w + i -- and return the singular
 * values sv f64[nmat][16] (unsorted; may be NULL), per matrix its rotation steps | sweeps << 16 (work u32[nmat]; may be NULL)
 * and the mean duration of `reps` launches in ms.  Used to measure what ordering the matrices into waves is worth
 * (tools/bdsqr_order.py).  No reference counterpart.                                                                */
int tq_debug_bdsqr(tq_ctx *ctx, const double *de, int64_t nmat, double *sv, uint32_t *work, int reps, double *ms);

/* Text for the consumers right after the hot path (host code, no device involved).
 * tq_format_tsv writes the rows the reference appends to <name>.quartets_<rep>.tsv
 *   (run_inference.py:233-234: pd.concat([rqrts, rscor, rstat], axis=1).to_csv(sep="\t",
 *   float_format='%.6f', index=False, header=False)): "a\tb\tc\td\ts0\ts1\ts2\ttopo\tnsnps\n".
 * tq_format_qmc writes the wQMC input lines "a,b|c,d:weight\n" of iter_qmc_formatted
 *   (run_inference.py:254-305) for the rows that pass min_snps (:258,:275) and min_ratio (:300), with the
 *   weight strategies 0..3 (:280-297) computed, as the reference does, from the scores as they read
 *   back from the TSV (rounded to 6 decimals); *n_lines = lines written.  The reference then shuffles
 *   the file with `shuf` (:326-327); that is left to the caller.
 * Both return TQ_OK with *written = bytes produced (no terminating 0), TQ_ERR_OOM with *written = a
 * buffer size that is sufficient when `cap` was too small, TQ_ERR_INVALID_ARG otherwise.            */
int tq_format_tsv(const uint32_t *quartets, const uint32_t *rstat, const double *rscor, int64_t Q,
                  char *out, int64_t cap, int64_t *written);
int tq_format_qmc(const uint32_t *quartets, const uint32_t *rstat, const double *rscor, int64_t Q,
                  int weights, int64_t min_snps, double min_ratio, char *out, int64_t cap,
                  int64_t *written, int64_t *n_lines);

/* The site order of the packed layout (option site_pack; host code, no device involved): src[p] = the site of the matrix
 * that packed position p holds, or 0xFFFFFFFF for a pad (missing in every taxon).  Every site appears once; the sites of a
 * locus (a run of equal ids in `locus`, read with stride `locus_stride`) stay adjacent and in order; a locus of at most 32
 * sites lies inside one 32-site word, a longer one starts a word and fills consecutive words; words come by falling number
 * of loci; the length is a multiple of 2048.  *packed_sites = that length; src (cap entries) is filled when cap suffices,
 * so a first call with cap = 0 sizes the buffer.  With tmparr u8[T][S] (may be NULL) the automatic rule is evaluated too:
 * *pays = 1 when tq_set_data would build the packed copy under site_pack = -1, and estimate[0..4] = predicted vector
 * instructions per quartet of the natural and of the packed layout, walk trips per quartet of the two, and the relative gain
 * in instructions lowered by two standard errors of the sample (the rule takes the packed layout from 0.03 on).  pays and
 * estimate may be NULL.  TQ_ERR_LOCUS_ORDER when a locus id is 0xFFFFFFFF or does not form one run.                  */
int tq_pack_sites(const uint8_t *tmparr, int64_t T, int64_t S, const uint32_t *locus, int64_t locus_stride, uint32_t *src,
                  int64_t cap, int64_t *packed_sites, int32_t *pays, double *estimate);

/* The reference's quartet sample, stream-identical and faster (host code): what
 * `Generator.choice(pop, size, replace=False)` (combinations.py:113) returns when size > pop // 50 and
 * pop > 10 000 -- NumPy's tail shuffle of arange(pop) -- drawn from the SAME NumPy bit generator, passed as the
 * address NumPy publishes in `rng.bit_generator.ctypes.bit_generator` (caller holds `bit_generator.lock`).
 * The Generator is left in the state NumPy's own call would leave it in.  pop <= 2^32 - 2.        */
int tq_numpy_choice_tail(void *np_bitgen, uint64_t pop, int64_t size, int64_t *out);

/* Lexicographic unranking on the host (no device involved): quartets[i] = the 4-combination of range(T) with
 * rank ranks[i] (or first_rank + i when ranks is NULL), i.e. _index_to_combination (combinations.py:94-106) for
 * every sampled index / islice(combinations(range(T), 4), first_rank, first_rank + Q) (combinations.py:40-55).
 * Ranks are 64-bit: C(T,4) is below 2^64 up to T = 145 056, and every call that takes or makes ranks (this one,
 * tq_unrank_dev, tq_resolve_range_dev, tq_sample_quartets_dev, tq_qd_score_ranks, tq_ls_score_ranks) refuses a larger T
 * with TQ_ERR_INVALID_ARG and one message ("C(T,4) does not fit 64 bits").  TQ_ERR_INVALID_ARG too when a rank is
 * >= C(T,4) or the range [first_rank, first_rank + Q) does not end at or below C(T,4) (tested without forming the sum,
 * which wraps near 2^64); the message is read with tq_last_error(NULL).                              */
int tq_unrank(const uint64_t *ranks, uint64_t first_rank, int64_t Q, int64_t T, uint32_t *quartets);

/* The rows tq_format_qmc would write, as arrays (no text round trip): splits u32[n,4] = "a,b|c,d" and weights f64[n]
 * (the value of the line's "%.5f" text), n = *n_rows <= Q; splits / weights must hold Q rows.  Input for tq_qmc_tree.  */
int tq_qmc_splits(const uint32_t *quartets, const uint32_t *rstat, const double *rscor, int64_t Q, int weights,
                  int64_t min_snps, double min_ratio, uint32_t *splits, double *weights_out, int64_t *n_rows);

/* Quartet supertree (host code, no device involved): weighted Quartet MaxCut over `n` resolved quartets
 * splits u32[n,4] = "a,b|c,d" (the taxa of a wQMC input line, run_inference.py:264-305), weights f64[n] or
 * NULL (all 1), taxa 0..ntaxa-1.  Writes the unrooted tree as newick with the taxon numbers as tip labels
 * ("((0,1),(2,3),4);"), *written = its length (TQ_ERR_OOM with the needed size when cap is too small).
 * Takes the place of: `bin/max-cut-tree qrtt=.. weights=on|off otre=..` as called by run_qmc
 * (run_inference.py:146-166).  That binary ships without source and is never run or read here: this is an
 * implementation from the published method, and parity with it is UNPINNED by construction.        */
int tq_qmc_tree(const uint32_t *splits, const double *weights, int64_t n, int64_t ntaxa, uint64_t seed,
                char *out, int64_t cap, int64_t *written);

/* Quartet concordance on a fixed tree.  Replaces: prepare_fixed_tree + set_quartet_data +
 * the counting half of set_quartet_stats (tetrad/src/concordance.py:97-244), which re-read every quartets TSV line by
 * line; here the rows are counted where they are -- host arrays, or device arrays right behind tq_svd_dev.
 *   tq_conc_create  tree as a parent array: nodes 0..T-1 are the taxa (tips), nodes >= T internal, parent[root] = -1;
 *                   4 <= T <= 4096.  A root of degree 2 is dissolved (unrooted, as toytree's .unroot()), unary nodes
 *                   are suppressed; edges = the nontrivial splits of that tree (both sides >= 2 taxa).  min_snps is
 *                   taken as max(1, min_snps).  `ctx` may be NULL: then only tq_conc_add works.  The context must
 *                   outlive the accumulator; messages go to tq_last_error(ctx) (tq_last_error(NULL) without one).
 *   tq_conc_add     host rows (no device involved), synchronous: quartets u32[n,4], rstat u32[n,2] {topology, nsnps},
 *                   rscor f64[n,3], flags u8[n] or NULL.
 *   tq_conc_add_dev the same rows as device pointers, enqueued on `stream` (hipStream_t, NULL = default stream),
 *                   allocation-free; calls on different streams are ordered in call order (the accumulator's slab).
 *   tq_conc_read    waits for the device adds and returns the sums of every add since create / reset, any output may be
 *                   NULL: edge_counts i64[E][6] = {nqrts, conc, disc1, disc2, nu, nsnps sum}, edge_sums f64[E][2] =
 *                   {weight sum, score sum}, masks u64[E][W] = taxa on one side of each edge (bit x of word x/64),
 *                   tip_counts i64[T][2] = {QFc, QFd}, *skipped = rows counted nowhere (taxon >= T, repeated taxon,
 *                   topology > 2, flags TQ_FLAG_BAD_INDEX or TQ_FLAG_INVALID_DIAGNOSTIC).  E, W: tq_conc_shape.   */
typedef struct tq_conc tq_conc;
int tq_conc_create(tq_conc **out, const int32_t *parent, int64_t n_nodes, int64_t T, int64_t min_snps, double min_ratio,
                   tq_ctx *ctx);
void tq_conc_destroy(tq_conc *acc);
int tq_conc_reset(tq_conc *acc);
int tq_conc_add(tq_conc *acc, const uint32_t *quartets, const uint32_t *rstat, const double *rscor, const uint8_t *flags,
                int64_t n);
int tq_conc_add_dev(tq_conc *acc, const uint32_t *d_quartets, const uint32_t *d_rstat, const double *d_rscor,
                    const uint8_t *d_flags, int64_t n, void *stream);
int tq_conc_shape(const tq_conc *acc, int64_t *T, int64_t *n_edges, int64_t *mask_words);
int tq_conc_read(tq_conc *acc, int64_t *edge_counts, double *edge_sums, uint64_t *masks, int64_t *tip_counts,
                 int64_t *skipped);

/* Exact quartet supertree: Quartet MaxCut level by level with integer graph weights, the passes
 * over the quartets on the device next to the resolved rows.  A second path beside tq_qmc_splits + tq_qmc_tree, which
 * stay as they are; the host and the device execution of it give the same newick string, bit for bit, for any row
 * order and any split of the rows over several adds.
 *   Row rule: the filters, split and weight of tq_qmc_splits (weights 0-3, min_snps taken as max(1, min_snps), scores
 *   as their "%.6f" text reads back); the weight is kept as the integer k = weight x 10^5 rounded as "%.5f" rounds.
 *   Skipped (counted, kept nowhere): a row the filters drop, a taxon >= ntaxa, a repeated taxon, topology > 2, flags
 *   TQ_FLAG_BAD_INDEX / TQ_FLAG_INVALID_DIAGNOSTIC, k == 0, a weight that is not finite or >= 4e9.
 *   tq_stree_create  capacity_rows = rows that may be added between two resets (kept or not), < 2^31.  `ctx` NULL: host
 *                    back end only, 1 <= ntaxa <= 65535.  With a context: 4 <= ntaxa <= 1024, all device and page-locked
 *                    memory is allocated here (56 bytes per row of capacity, 24 x ntaxa^2 bytes of each kind for a level's
 *                    matrices).  The context must outlive the accumulator; messages go to tq_last_error(ctx).
 *   tq_stree_add     host rows, synchronous; arrays as tq_conc_add.  More rows than the capacity: TQ_ERR_INVALID_ARG,
 *                    nothing is added.
 *   tq_stree_add_dev the same rows as device pointers, enqueued on `stream`, allocation-free; calls on different streams
 *                    are ordered in call order.  Host and device rows do not mix in one accumulator (until a reset).
 *   tq_stree_graph   the root graph of the rows added so far, any output may be NULL: G / B u64[ntaxa][ntaxa] symmetric,
 *                    G[u][v] = sum of k over the kept rows that have u and v on different sides of their split, B[u][v] =
 *                    the same for rows that pair u with v; kept / skipped rows; *sum_k = sum of k (2^64 - 1 when larger).
 *   tq_stree_rows    the kept rows: splits u32[kept][4] = "a,b|c,d", k u64[kept] (either may be NULL), *n = kept.  Host
 *                    rows come in the order added, device rows in any order.
 *   tq_stree_build   the tree of the rows added so far as newick with the taxon numbers as tip labels, *written = its
 *                    length (TQ_ERR_OOM with the needed size when cap is too small), *levels = levels of the recursion.
 *                    Device rows: the passes run on `stream`, two synchronisations of it per level.  Refused
 *                    (TQ_ERR_INVALID_ARG) when 6 x sum of k >= 2^53.  The rows stay: build may be repeated with any seed.
 *   tq_stree_level_stats  of the last build: *n_levels (at most 64 are kept), out f64[n_levels][6] = {open nodes, live
 *                    quartets, cells of one matrix, graph pass ms, host search ms, partition pass ms} (wall clock of the
 *                    calling thread, synchronisation included).
 *   tq_stree_set_search  the rule of the cut search of the following builds: 0 (default) = the multi-start search on
 *                    the cells as doubles, run on the host; 1 = "exact", the all-integer rule of DESIGN.md section 16,
 *                    which device rows run in a kernel (only side bytes and a cut byte per node come back, still two
 *                    synchronisations per level) and host rows on the host, with the same newick string from both.
 *                    Anything else: TQ_ERR_INVALID_ARG, the rule stays.  May be called between builds.
 *   tq_stree_fit     quartet fit of R trees against the kept rows.  Trees as tq_cons_add takes
 *                    them: parents i32[R][stride], n_nodes i64[R] (each <= stride), tips 0..ntaxa-1 = the taxa, every
 *                    taxon of the accumulator in every tree.  Every tree is validated first: one bad tree gives
 *                    TQ_ERR_INVALID_ARG with its index in the message and nothing is written.  With D(x, y) = the depth
 *                    of the lowest common ancestor of tips x and y, a kept row a,b|c,d is satisfied when D(a,b) + D(c,d)
 *                    is strictly the largest of the three pair sums, violated when one of the two others is, unresolved
 *                    when the largest is not unique (a polytomy); the class does not depend on the rooting, on a root of
 *                    degree 2 or on unary nodes.  out u64[R][6] = {k_satisfied, k_violated, k_unresolved, n_satisfied,
 *                    n_violated, n_unresolved}: the k sum to the accumulator's sum of k, the n to its kept rows, and the
 *                    host and the device execution agree bit for bit.  Host rows (or none, or no context) run on the
 *                    host.  Device rows run tq_fit_table_kernel and tq_fit_kernel on `stream`, ordered behind the adds,
 *                    with one synchronisation before returning.  Unlike the adds this call MAY ALLOCATE: the first fit
 *                    of an accumulator allocates the table region (device) and staging for the parent arrays and the
 *                    results (device and page-locked, 16 x ntaxa + 48 bytes per tree); both only grow and are freed
 *                    with the accumulator.  The rows stay: fits and builds may alternate in any order.  Refused
 *                    (TQ_ERR_INVALID_ARG) when the sum of k does not fit in 64 bits (tq_stree_graph then reports
 *                    2^64 - 1); the 2^53 limit of tq_stree_build does not apply.  R = 0 and no kept rows (all zeros) are
 *                    valid.
 *   tq_stree_nni_scan  the quartet-fit weights of every nearest-neighbour interchange of one tree, in one pass over the
 *                    kept rows.  The tree is a parent array as tq_stree_fit takes one (validated
 *                    first, the same messages, as "tree 0"; a bad tree writes nothing) and is held as prepared: root of
 *                    degree >= 3, no unary nodes, children ordered by their smallest taxon, internal nodes in BFS order.
 *                    Edge e is the edge above the e-th internal non-root node v; *n_edges <= ntaxa - 3 of them.  With u =
 *                    parent(v) the edge is eligible when v has two children and u three neighbours (eligible u8[E]).  Its
 *                    corners u64[E][4][W], W = ceil(ntaxa / 64), bit x of word x / 64: X1, X2 = the taxa below the
 *                    children of v, Y1, Y2 = the two other subtrees at u, within a side the corner with the smaller
 *                    smallest taxon first; zeros when not eligible.  w u64[E][3]: the sum of k over the kept rows with
 *                    one taxon in each corner that display X1 X2 | Y1 Y2 (the tree's split), X1 Y1 | X2 Y2 (alternative
 *                    1) and X1 Y2 | X2 Y1 (alternative 2); zeros when not eligible.  The neighbour tree of alternative j
 *                    has k_satisfied - w[e][0] + w[e][j], k_violated + w[e][0] - w[e][j] and the same k_unresolved.  Any
 *                    output may be NULL.  Host rows (or none, or no context) run on the host; device rows run
 *                    tq_nni_table_kernel and tq_nni_kernel on `stream` behind the adds, with one synchronisation, and
 *                    give the same numbers bit for bit.  The first scan on device rows ALLOCATES (2 ntaxa^2 + 44 ntaxa
 *                    bytes on the device, 40 ntaxa page-locked), freed with the accumulator.  Refused when the sum of k
 *                    does not fit in 64 bits.  No kept rows (all zeros) is valid.  The rows stay.
 *   tq_stree_polish  local search from that tree: one round = one scan, then for every eligible edge the alternative with
 *                    the larger weight (a tie: alternative 1), a candidate when that weight exceeds w[e][0]; candidates by
 *                    gain descending, then edge ascending; an edge is accepted when neither of its two nodes belongs to an
 *                    edge accepted before it in the round; all accepted interchanges are applied (the root stays) and
 *                    k_satisfied rises by exactly the sum of their gains.  Stops when a scan finds no candidate
 *                    (*converged = 1) or after max_rounds rounds (0..65536; 0 only rewrites the tree).  out / cap /
 *                    *written as tq_stree_build: newick with numeric tips from the prepared rooting, children by smallest
 *                    taxon.  trace u64[max_rounds][2] = {interchanges applied, sum of gains} per round that moved, *rounds
 *                    = those rounds; trace, rounds and converged may be NULL.  The selection runs on the host for both
 *                    back ends: the same string and trace from both.  One synchronisation of `stream` per round.
 * Option "fit_scratch_bytes" (tq_set_option, default 64 MiB, read at an accumulator's first fit): bound of the table
 * region.  Trees per chunk = max(1, bytes / (2 ntaxa^2)); chunks run one after the other on the call's stream.  Results
 * never depend on it.
 * Option "stree_lds" (tq_set_option): 1 (default) = the graph pass sums in private LDS counters where a level's cells fit
 * (at most 8128 per matrix), 0 = global integer atomics only.  Both are exact.
 * Option "stree_search_dev": 1 (default) = device rows run the rule "exact" in tq_stree_search_kernel, 0 = the matrices
 * are copied out and the same rule runs on the host (A/B; the same string).                                            */
typedef struct tq_stree tq_stree;
int tq_stree_create(tq_stree **out, int64_t ntaxa, int64_t capacity_rows, int weights, int64_t min_snps, double min_ratio,
                    tq_ctx *ctx);
void tq_stree_destroy(tq_stree *acc);
int tq_stree_reset(tq_stree *acc);
int tq_stree_add(tq_stree *acc, const uint32_t *quartets, const uint32_t *rstat, const double *rscor, const uint8_t *flags,
                 int64_t n);
int tq_stree_add_dev(tq_stree *acc, const uint32_t *d_quartets, const uint32_t *d_rstat, const double *d_rscor,
                     const uint8_t *d_flags, int64_t n, void *stream);
int tq_stree_graph(tq_stree *acc, uint64_t *G, uint64_t *B, int64_t *kept, int64_t *skipped, uint64_t *sum_k);
int tq_stree_rows(tq_stree *acc, uint32_t *splits, uint64_t *k, int64_t *n);
int tq_stree_build(tq_stree *acc, uint64_t seed, void *stream, char *out, int64_t cap, int64_t *written, int64_t *levels);
int tq_stree_level_stats(const tq_stree *acc, int64_t *n_levels, double *out);
int tq_stree_set_search(tq_stree *acc, int search);
int tq_stree_fit(tq_stree *acc, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride, void *stream,
                 uint64_t *out);
int tq_stree_nni_scan(tq_stree *acc, const int32_t *parent, int64_t n_nodes, void *stream, int64_t *n_edges,
                      uint8_t *eligible, uint64_t *corners, uint64_t *w);
int tq_stree_polish(tq_stree *acc, const int32_t *parent, int64_t n_nodes, int64_t max_rounds, void *stream, char *out,
                    int64_t cap, int64_t *written, uint64_t *trace, int64_t *rounds, int *converged);

/* Test hook: the exact cut search alone on a batch of nodes.  sizes i32[n_nodes] (4..65535 on the host, 4..1024 on the
 * device), G and B the nodes' upper triangles one after the other (node of n taxa: n (n - 1) / 2 cells, cell (u < v) at
 * u n - u (u + 1) / 2 + v - u - 1; 6 x the sum of a node's B cells / 2 must stay below 2^53), node_seeds u64[n_nodes].
 * Out: side u8[sum of sizes] (zero for a node without a cut), cut u8[n_nodes], rounds i32[n_nodes] (may be NULL) = the
 * Dinkelbach rounds run, 0 for n = 4 and for a node without B.  ctx NULL: the host execution; otherwise the batch is
 * uploaded and tq_stree_search_kernel runs it in one launch.  No reference counterpart.                                */
int tq_stree_search(tq_ctx *ctx, int64_t n_nodes, const int32_t *sizes, const uint64_t *G, const uint64_t *B,
                    const uint64_t *node_seeds, uint8_t *side, uint8_t *cut, int32_t *rounds);

/* Majority-rule consensus: how many trees of a set contain each split, counted exactly, the
 * consensus tree built from the counts, and the counts written onto the edges of a given tree (the computation behind
 * the reference's `tetrad consensus`, cli_consensus.py:87-132).  The host and the device execution return identical
 * arrays and strings.
 *   Trees are parent arrays as tq_conc_create takes them (tips 0..T-1 = the taxa, parent[root] = -1; a root of degree 2
 *   is dissolved, unary nodes are suppressed; multifurcations allowed), 4 <= T <= 4096.  A split is an internal edge
 *   with at least 2 taxa on both sides; its mask is the side without taxon 0, bit x of word x / 64 of W = ceil(T / 64)
 *   u64 words.  Table order: count descending, then the mask ascending as one integer (word W - 1 most significant).
 *   tq_cons_create  max_splits = distinct splits the table may hold (1..2^26).  `ctx` NULL: host back end.  With a
 *                   context all device and page-locked memory is allocated here: the table (max_splits x (W + 3) x 8
 *                   bytes) and one chunk of trees within the option "cons_scratch_bytes".  The context must outlive the
 *                   accumulator; messages go to tq_last_error(ctx).
 *   tq_cons_add     parents i32[R][stride], n_nodes i64[R] (each <= stride).  Every tree is validated first: one bad
 *                   tree is TQ_ERR_INVALID_ARG naming its index, and nothing is added.  Device back end: the kernels
 *                   run on `stream` (hipStream_t, NULL = default stream) chunk by chunk; the call returns with the last
 *                   chunk in flight.  Adds on different streams are ordered in call order.
 *   tq_cons_shape   T, W, trees added, distinct splits (any may be NULL; asking for the splits waits for device work).
 *   tq_cons_read    masks u64[nsplits][W], counts i64[nsplits] in table order (either may be NULL); waits for device work.
 *   tq_cons_tree    the consensus as newick: walking the table, a split is accepted when count >= min_count (>= 1) and
 *                   it is compatible with every accepted split (disjoint, or one side inside the other).  The root holds
 *                   the maximal sides and the uncovered tips (taxon 0 among them), children are ordered by their
 *                   smallest taxon, tips are taxon numbers, an accepted side carries the integer percent
 *                   (200 count + ntrees) / (2 ntrees) as its label, no branch lengths.  *written = the length
 *                   (TQ_ERR_OOM with the needed size when cap is too small).
 *   tq_cons_support the splits of one given tree, masks ascending: counts_out i64[E] = the split's count in the table
 *                   (0 when absent), masks_out u64[E][W] (either may be NULL, room for T - 3 splits), *n_edges = E.
 *   tq_cons_stats   out i64[6] = {trees per chunk, chunks launched, entries of the device table, entries of the host
 *                   map, splits that lost a hash collision and were counted on the host, hash bits}; since create / reset.
 *   More distinct splits than max_splits: TQ_ERR_INVALID_ARG from the add or the read that notices, and from every call
 *   after it until tq_cons_reset; nothing is ever written out of bounds.
 * Options (tq_set_option): "cons_hash_bits" 1..64 (default 64; read at create / reset) cuts the table key, so that the
 * collision path can be exercised: results never depend on it.  "cons_scratch_bytes" (default 256 MiB; read at create)
 * bounds the device and page-locked memory of one chunk of trees.                                                       */
typedef struct tq_cons tq_cons;
int tq_cons_create(tq_cons **out, int64_t T, int64_t max_splits, tq_ctx *ctx);
void tq_cons_destroy(tq_cons *acc);
int tq_cons_reset(tq_cons *acc);
int tq_cons_add(tq_cons *acc, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride, void *stream);
int tq_cons_shape(tq_cons *acc, int64_t *T, int64_t *W, int64_t *ntrees, int64_t *nsplits);
int tq_cons_read(tq_cons *acc, uint64_t *masks, int64_t *counts);
int tq_cons_tree(tq_cons *acc, int64_t min_count, char *out, int64_t cap, int64_t *written);
int tq_cons_support(tq_cons *acc, const int32_t *parent, int64_t n_nodes, int64_t *counts_out, uint64_t *masks_out,
                    int64_t *n_edges);
int tq_cons_stats(tq_cons *acc, int64_t *out);

/* Transfer bootstrap supports (TBE; Lemoine et al. 2018): for every branch of one reference tree
 * and every replicate tree, the number of taxa that must be moved to turn the branch's bipartition into the closest
 * bipartition of the replicate, summed over the replicates.  Integers only; the host and the device execution return
 * identical arrays.  No reference counterpart.
 *   Trees are parent arrays as tq_cons_add takes them (a root of degree 2 is dissolved, unary nodes are suppressed,
 *   multifurcations allowed), 4 <= T <= 4096.
 *   Branches: the splits of the reference tree (an internal edge with at least 2 taxa on both sides), mask = the side
 *   without taxon 0 in W = ceil(T / 64) u64 words, ordered by the mask ascending as one integer (the order of
 *   tq_cons_support), E <= T - 3 of them; p[b] = min(|mask|, T - |mask|) >= 2, the light side.
 *   Distance of two bipartitions with masks x, y: d = popcount(x xor y) over the W words, delta = min(d, T - d); the
 *   same whichever side either mask names.
 *   Transfer index phi(b, t) = the minimum of delta over every edge of replicate t, the edges above tips included: a tip
 *   of the light side gives p - 1, so phi = min(p[b] - 1, min over the internal splits of t of delta).  A star gives
 *   p - 1 for every branch, a replicate that contains the branch gives 0.  No argmin is reported.
 *   Accumulated: ntrees and phi_sum[b] = the sum of phi(b, t), u64; any chunking and order of adds gives the same sums.
 *   Support: TBE(b) = 1 - phi_sum[b] / (ntrees (p[b] - 1)), taken by the caller; the integer percent, rounded half up,
 *   is (200 (N q - s) + N q) / (2 N q) with q = p - 1, N = ntrees, s = phi_sum.
 *   tq_tbe_create   the reference tree ref_parent i32[n_nodes]; a bad tree is TQ_ERR_INVALID_ARG, a star is valid with
 *                   E = 0.  `ctx` NULL: host back end.  With a context all device and page-locked memory is allocated
 *                   here: the branch masks, p and phi_sum, and one chunk of trees (records, masks, phi rows) within the
 *                   option "cons_scratch_bytes", read here as tq_cons_create reads it.  The context must outlive the
 *                   accumulator; messages go to tq_last_error(ctx).
 *   tq_tbe_reset    keeps the reference tree, zeroes ntrees and phi_sum (waits for device work).
 *   tq_tbe_add      parents i32[R][stride], n_nodes i64[R] (each <= stride).  Every tree is validated first: one bad
 *                   tree is TQ_ERR_INVALID_ARG naming its index, and nothing is added.  R = 0 is a no-op.  Device back
 *                   end: the kernels run on `stream` (hipStream_t, NULL = default stream) chunk by chunk.  phi_out
 *                   NULL: the call returns with the last chunk in flight.  phi_out u16[R][E]: the call waits for its
 *                   chunks and writes phi(b, t) of every replicate of the call.  Adds on different streams are ordered
 *                   in call order.
 *   tq_tbe_shape    T, W, E, trees added (any may be NULL).
 *   tq_tbe_read     masks u64[E][W], p i64[E], phi_sum u64[E] (any may be NULL); waits for device work.
 *   tq_tbe_stats    out i64[2] = {trees per chunk (0 on the host), chunks launched since create / reset}.           */
typedef struct tq_tbe tq_tbe;
int tq_tbe_create(tq_tbe **out, int64_t T, const int32_t *ref_parent, int64_t n_nodes, tq_ctx *ctx);
void tq_tbe_destroy(tq_tbe *acc);
int tq_tbe_reset(tq_tbe *acc);
int tq_tbe_add(tq_tbe *acc, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride, void *stream,
               uint16_t *phi_out);
int tq_tbe_shape(tq_tbe *acc, int64_t *T, int64_t *W, int64_t *E, int64_t *ntrees);
int tq_tbe_read(tq_tbe *acc, uint64_t *masks, int64_t *p, uint64_t *phi_sum);
int tq_tbe_stats(tq_tbe *acc, int64_t *out);

/* All-pairs Robinson-Foulds distances of a set of trees: which trees of a bootstrap set, of N
 * restarts or of two search rules agree, and by how much.  Integers only; the host and the device execution return
 * identical arrays.  No reference counterpart.
 *   Trees are parent arrays as tq_cons_add takes them (a root of degree 2 is dissolved, unary nodes are suppressed,
 *   multifurcations allowed), 4 <= T <= 4096.  A split is an internal edge with at least 2 taxa on both sides, its mask
 *   the side without taxon 0 in W = ceil(T / 64) u64 words; two splits are the same when all W words are.
 *   nsplits[i]    the splits of tree i: 0 for a star, at most T - 3.
 *   shared[i][j]  the splits both trees hold; shared[i][i] = nsplits[i].
 *   rf[i][j]      nsplits[i] + nsplits[j] - 2 shared[i][j]: the size of the symmetric difference, the unnormalised
 *                 Robinson-Foulds distance of unrooted trees (right for polytomies too).
 *   The matrices are symmetric, N x N over the trees in the order they were added.  No result depends on the chunking
 *   of trees or columns, the order of adds, streams or the option "cons_hash_bits".
 *   tq_rf_create   max_trees 1..8192, max_splits 1..2^26 distinct splits.  `ctx` NULL: host back end (an exact map gives
 *                  every tree an ascending id list; shared = a merge of two lists).  With a context all device and
 *                  page-locked memory is allocated here: a split table of max_splits entries, ids u32[max_trees][T - 2],
 *                  the two u32 matrices of max_trees^2 each, one chunk of trees and the bit rows of one chunk of columns,
 *                  each within the option "cons_scratch_bytes"; "cons_hash_bits" is read here and at reset.  A failed
 *                  allocation is TQ_ERR_OOM / TQ_ERR_HIP with a message and frees everything.  The context must outlive
 *                  the accumulator; messages go to tq_last_error(ctx).
 *   tq_rf_reset    forgets the trees and the splits (waits for device work).
 *   tq_rf_add      parents i32[R][stride], n_nodes i64[R] (each <= stride).  Every tree is validated first: one bad tree
 *                  is TQ_ERR_INVALID_ARG naming its index, more than max_trees trees in all is TQ_ERR_INVALID_ARG, and
 *                  nothing is added.  R = 0 is a no-op.  Device back end: the kernels run on `stream` (hipStream_t, NULL
 *                  = default stream) chunk by chunk and the call returns with the last chunk in flight; adds on different
 *                  streams are ordered in call order.  More than max_splits distinct splits: TQ_ERR_INVALID_ARG, at the
 *                  add or at the next call that waits, and the accumulator refuses everything until a reset.
 *   tq_rf_shape    T, W, trees added, distinct splits seen (waits), columns of the last read (any may be NULL).
 *   tq_rf_read     nsplits i32[N], shared u32[N][N], rf u32[N][N] (any may be NULL); waits.  May be called any number of
 *                  times, between adds too.  Device back end: a column is a split of at least two trees; the bit rows
 *                  B[N][columns] are built a chunk of columns at a time and shared += B B^T by tq_rf_gemm_kernel.
 *   tq_rf_stats    out i64[8] = {trees per chunk, tree chunks launched since create / reset, columns of the last read,
 *                  column words per chunk, column chunks of the last read, splits resolved on the host after a hash
 *                  collision, hash bits in use, entries of the device table}; on the host only the columns count.
 *   tq_rf_word_shared  the word rule of the product, popcount(x & y): the one definition tq_rf_gemm_kernel compiles.  */
typedef struct tq_rf tq_rf;
int tq_rf_create(tq_rf **out, int64_t T, int64_t max_trees, int64_t max_splits, tq_ctx *ctx);
void tq_rf_destroy(tq_rf *acc);
int tq_rf_reset(tq_rf *acc);
int tq_rf_add(tq_rf *acc, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride, void *stream);
int tq_rf_shape(tq_rf *acc, int64_t *T, int64_t *W, int64_t *ntrees, int64_t *nsplits, int64_t *columns);
int tq_rf_read(tq_rf *acc, int32_t *nsplits, uint32_t *shared, uint32_t *rf);
int tq_rf_stats(tq_rf *acc, int64_t *out);
uint32_t tq_rf_word_shared(uint64_t x, uint64_t y);

/* All-pairs quartet distances of a set of trees: for every pair of trees the number of quartets
 * both resolve alike, both resolve differently, only one resolves, neither resolves -- the ruler of the quartet
 * supertrees themselves, and one that a single misplaced taxon moves little.  Integers only; the host and the device
 * execution return identical arrays.  No reference counterpart.
 *   Trees are parent arrays as tq_stree_fit takes them (a root of degree 2 is dissolved, unary nodes are suppressed,
 *   multifurcations allowed), 4 <= T <= 1024 on both back ends.  D(x, y) is the depth of the lowest common ancestor of
 *   tips x and y.  The code of four distinct taxa (a, b, c, d), in any order, in a tree: with m0 = D(a,b) + D(c,d),
 *   m1 = D(a,c) + D(b,d), m2 = D(a,d) + D(b,c) it is 0, 1 or 2 when m0, m1 or m2 is strictly the largest and 3
 *   (unresolved) otherwise.
 *   same[i][j]    quartets scored so far that trees i and j both resolve, with the same code.
 *   both[i][j]    quartets scored so far that both resolve; both[i][i] = the quartets tree i resolves.
 *   Both are exact u64 sums, symmetric, N x N over the trees in the order they were added.  No result depends on the
 *   launch shape, the chunking of trees or quartets, the k split, streams, the order of score calls or the order of the
 *   taxa inside a quartet.
 *   tq_qd_create   max_trees 1..8192.  `ctx` NULL: host back end.  With a context all device and page-locked memory is
 *                  allocated here: tables max_trees T^2 u16, the parent records max_trees 2 T i32 (device and
 *                  page-locked), two u64 matrices of max_trees^2, and one chunk of quartets -- per quartet 16 bytes of
 *                  taxa and 8 of rank on the device, 16 page-locked, and 3 bits of plane row for each of max_trees --
 *                  within the option "qdist_scratch_bytes" (tq_set_option, default 256 MiB, 0 = default, read here).  A
 *                  failed allocation is TQ_ERR_OOM / TQ_ERR_HIP with a message and frees everything.  The context must
 *                  outlive the accumulator; messages go to tq_last_error(ctx).
 *   tq_qd_add      parents i32[R][stride], n_nodes i64[R] (each <= stride).  Every tree is validated first, with the
 *                  messages of tq_stree_fit: one bad tree is TQ_ERR_INVALID_ARG naming its index, more than max_trees
 *                  trees in all is TQ_ERR_INVALID_ARG, and nothing of the call is added.  The tables of the new trees are
 *                  built (tq_fit_table_kernel on `stream`) and kept.  Refused once anything has been scored, until a
 *                  clear or reset.  R = 0 is a no-op.
 *   tq_qd_score    quartets i32[Q][4]: the host checks every quartet (taxa distinct and < T); one bad quartet is
 *                  TQ_ERR_INVALID_ARG naming its index and nothing is scored.  Device back end: chunk by chunk on
 *                  `stream` (hipStream_t, NULL = default stream) tq_qd_encode_kernel writes three bit planes per tree and
 *                  tq_qd_gemm_kernel adds their product; the call returns with the last chunk in flight.
 *   tq_qd_score_ranks  ranks u64[Q], or NULL for the Q consecutive ranks from first_rank: lexicographic ranks of
 *                  4-combinations as in tq_resolve_range_dev, unranked by tq_unrank_kernel.  A rank >= C(T,4) is
 *                  TQ_ERR_INVALID_ARG naming its index and nothing is scored.  Q = 0 and an accumulator without trees are
 *                  valid no-ops (of both score calls).
 *   Calls on different streams are ordered in call order.  Option "qdist_kslices" (0 = auto, read at every score): the
 *   number of slices the words of a chunk are split into across workgroups of the product; auto aims at about 4
 *   workgroups per compute unit, never more slices than staged word chunks (of 8 words).
 *   tq_qd_clear    zeroes the counts and keeps the trees.   tq_qd_reset  forgets everything.  Both wait.
 *   tq_qd_shape    T, trees held, quartets scored since create / clear / reset (any may be NULL).
 *   tq_qd_read     same u64[N][N], both u64[N][N] (either may be NULL); waits.  May be called between score calls.
 *   tq_qd_stats    out i64[6] = {quartets per chunk, quartet chunks launched since create / reset, k slices of the last
 *                  launch (0 on the host), tree tables built since create / reset, table form (0 host, 1 LDS, 2 through
 *                  L2), plane words per chunk}.
 *   tq_qd_word_counts  the word rule of the product: same = popc(x0 & y0) + popc(x1 & y1) + popc(x2 & y2), both =
 *                  popc((x0 | x1 | x2) & (y0 | y1 | y2)); the one definition tq_qd_gemm_kernel compiles.  */
typedef struct tq_qd tq_qd;
int tq_qd_create(tq_qd **out, int64_t T, int64_t max_trees, tq_ctx *ctx);
void tq_qd_destroy(tq_qd *acc);
int tq_qd_reset(tq_qd *acc);
int tq_qd_clear(tq_qd *acc);
int tq_qd_add(tq_qd *acc, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride, void *stream);
int tq_qd_score(tq_qd *acc, const int32_t *quartets, int64_t Q, void *stream);
int tq_qd_score_ranks(tq_qd *acc, const uint64_t *ranks, uint64_t first_rank, int64_t Q, void *stream);
int tq_qd_shape(tq_qd *acc, int64_t *T, int64_t *ntrees, uint64_t *q_total);
int tq_qd_read(tq_qd *acc, uint64_t *same, uint64_t *both);
int tq_qd_stats(tq_qd *acc, int64_t *out);
void tq_qd_word_counts(uint64_t x0, uint64_t x1, uint64_t x2, uint64_t y0, uint64_t y1, uint64_t y2, uint32_t *same,
                       uint32_t *both);

/* Quartet frequencies of a set of trees and the sums of the leaf stability index (Thorley &
 * Wilkinson 1999, on quartets because the trees are unrooted): which taxa the trees disagree about.  Integers only; the
 * host and the device execution return identical arrays.  No reference counterpart.
 *   Trees, their limits and the code of a quartet in a tree are those of tq_qd above.  Over the N trees held, for a
 *   quartet row (a, b, c, d) as given:
 *   counts        u16[4] = (n_0, n_1, n_2, n_3): the trees with code 0 = ab|cd, 1 = ac|bd, 2 = ad|bc, and n_3 = N - n_0 -
 *                 n_1 - n_2 unresolved.  A row sums to N.
 *   top, second   the largest and the second largest of n_0..n_2 (equal when the largest is tied); dif = top - second,
 *                 res = n_0 + n_1 + n_2.
 *   acc[t][4]     u64 (quartets, res, top, dif): the sums over every scored row that holds taxon t; a row given twice
 *                 counts twice.  The order of the taxa inside a row permutes n_0..n_2 and moves nothing of acc.  No result
 *                 depends on the launch shape, the chunking of quartets, streams or the order of score calls.
 *   tq_ls_create  limits, refusals and back ends as tq_qd_create.  With a context everything is allocated here: tables and
 *                 parent records as tq_qd_create, acc, and one chunk of quartets within "qdist_scratch_bytes" -- per
 *                 quartet what tq_qd_create takes plus a counts row of 8 bytes on the device and 8 page-locked.  A failed
 *                 allocation is TQ_ERR_OOM / TQ_ERR_HIP with a message and frees everything.
 *   tq_ls_add     as tq_qd_add, under its own name.  Refused once anything has been scored, until a clear or reset: N is
 *                 the denominator of every scored row.
 *   tq_ls_score   quartets i32[Q][4], checked as tq_qd_score checks them; repeated rows are allowed.  `counts` u16[Q][4] or
 *                 NULL.  Device back end: chunk by chunk on `stream` tq_qd_encode_kernel writes the planes and
 *                 tq_ls_count_kernel sums them along the trees.  With counts NULL the call returns with the last chunk
 *                 in flight; with an array the rows come back chunk by chunk through the page-locked staging and the call
 *                 returns once the array is filled.
 *   tq_ls_score_ranks  ranks u64[Q], or NULL for the Q consecutive ranks from first_rank; checked as tq_qd_score_ranks.
 *                 Q = 0 and an accumulator without trees are valid no-ops of both score calls: counts is not written.
 *   tq_ls_clear   zeroes acc and the quartet total and keeps the trees.   tq_ls_reset  forgets everything.  Both wait.
 *   tq_ls_shape   T, trees held, quartet rows scored since create / clear / reset (any may be NULL).
 *   tq_ls_read    out u64[T][4]; waits.  May be called between score calls.
 *   tq_ls_stats   out i64[7] = {quartets per chunk, quartet chunks launched since create / reset, tree tables built since
 *                 create / reset, table form (0 host, 1 LDS, 2 through L2), plane words per chunk, workgroups of the last
 *                 count launch (0 on the host), trees per staged tile of tq_ls_count_kernel}.  */
typedef struct tq_ls tq_ls;
int tq_ls_create(tq_ls **out, int64_t T, int64_t max_trees, tq_ctx *ctx);
void tq_ls_destroy(tq_ls *acc);
int tq_ls_reset(tq_ls *acc);
int tq_ls_clear(tq_ls *acc);
int tq_ls_add(tq_ls *acc, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride, void *stream);
int tq_ls_score(tq_ls *acc, const int32_t *quartets, int64_t Q, uint16_t *counts, void *stream);
int tq_ls_score_ranks(tq_ls *acc, const uint64_t *ranks, uint64_t first_rank, int64_t Q, uint16_t *counts, void *stream);
int tq_ls_shape(tq_ls *acc, int64_t *T, int64_t *ntrees, uint64_t *q_total);
int tq_ls_read(tq_ls *acc, uint64_t *out);
int tq_ls_stats(tq_ls *acc, int64_t *out);

/* Species-tree mode: quartets of SPECIES resolved from pooled lineages, as SVDquartets' species
 * mode does.  No reference counterpart: the reference only plans a sample-to-clade table (`imap`, schema.py:50-51,
 * cli.py:8, parsed at write_database.py:198-201) and would use it to select samples.
 *   Pooling: the count matrix of species quartet (A, B, C, D) is the sum, over every lineage quartet (i in A, j in B,
 *   k in C, l in D), of the full-mode count matrix the reference worker builds for (i, j, k, l)
 *   (full_chunk_to_matrices with the mask of resolve_quartets.py:216-223: sites with a missing base or four equal bases
 *   are masked).  Equivalently sum_s a_s (x) b_s (x) c_s (x) d_s with the four bins (x,x,x,x) set to 0, where a_s[x] =
 *   lineages of A with base x at site s.  nsnps = the sum of the 256 bins; the other flattenings, ranks, scores,
 *   topology and flags come from the singular-value stage of tq_resolve, unchanged.  Full mode only: the reference's
 *   subsample mode picks a site per locus and LINEAGE quartet, which does not factor over sites.
 *   Range: bins and nsnps are u32 (resolve_quartets.py:88).  A species call is refused (TQ_ERR_INVALID_ARG) when
 *   S x (product of the four largest species sizes) >= 2^32; a row that repeats a species can still exceed that for
 *   its own lineage product: the host call refuses it, the device call gives it zero counts (TQ_FLAG_ZERO_DATA).
 *   Kernel forms (option "species_method"): 1 = MFMA (v_mfma_i32_16x16x64_i8, species of <= 11 lineages: i8 operands),
 *   0 = VALU (any size), -1 (default) = MFMA when every species of the map holds <= 11 lineages, else VALU.  Both give
 *   the same bits.
 *   tq_set_species  species_of i32[T]: species id in [0,K) per sample, -1 = left out; T must equal the resident (or
 *                   source) T, K >= 4, at most 255 lineages per species.  Replaces any earlier map.  The per-species
 *                   base counts (K x S x 8 bytes on the device) are rebuilt after every tq_set_data / tq_bootstrap* on
 *                   the stream of the next species call.
 *   tq_resolve_species  squartets u32[Q,4] species ids (host buffers, synchronous; any Q, in pieces of option "batch",
 *                   result D2H under the kernels as tq_resolve); outputs as tq_resolve.  An id >= K: TQ_ERR_INVALID_ARG.
 *   tq_resolve_species_dev  device pointers, enqueued on `stream` (the stream rule above); an id >= K gives the row
 *                   TQ_FLAG_BAD_INDEX (zero data).
 *   tq_resolve_species_debug  also the pooled cmats u32[Q,3,16,16], svds f64[Q,3,16], ranks i32[Q,3] (any may be NULL).
 * Species calls fail with TQ_ERR_NO_DATA without data or without a map, TQ_ERR_INVALID_ARG when the map's T differs from
 * the resident replicate's.
 *
 * Both alleles (option "species_alleles" = 1; 0, the default, is everything above): every sample
 * of the SOURCE matrix (tq_set_source: seqarr u8[T,S0]) is two haplotype lineages, and the per-species base counts are
 * built straight from it through the site map of the resident replicate instead of from the coin-resolved rows:
 *   a cell A / C / G / T (or an already recoded 0..3) adds 2 to its base; a two-base code adds 1 to each of its bases
 *   (R = G,A  K = G,T  S = G,C  Y = T,C  W = T,A  M = C,A: the table tq_bootstrap resolves by coin); every other byte
 *   (N, gap, three-base codes) adds nothing.  The pooled matrix, with the same formula as above, is then the sum over
 *   haplotype quartets = 16 x the expectation of the coin-resolved lineage-quartet matrix; seed_ambig has no influence.
 *   Which sites: those of the resident replicate, which must have been built by tq_bootstrap(_async) from the current
 *   source (the original matrix is the replicate of lidxs = 0..nloci-1).  Resident data from tq_set_data, or a
 *   tq_set_source newer than the replicate, make every species call fail with TQ_ERR_NO_DATA, as does no source at all.
 *   Sizes count in lineages = 2 x samples wherever a size rule applies: the call is refused when S x (product of the
 *   four largest 2n) >= 2^32; a species holds at most 127 samples (2n <= 255, one byte per base); the MFMA form
 *   (automatic choice and species_method 1) takes 2n <= 11, i.e. at most 5 samples per species; a row's own product
 *   is taken over its 2n (host call: refused, device call: zero counts and TQ_FLAG_ZERO_DATA).  All of it is checked
 *   by the species call, since the option can be set after the map.  Setting the option to another value makes the
 *   next species call rebuild the counts on its stream; any value other than 0 / 1 is refused.                        */
int tq_set_species(tq_ctx *ctx, const int32_t *species_of, int64_t T, int64_t K);
int tq_resolve_species(tq_ctx *ctx, const uint32_t *squartets, int64_t Q, uint32_t *rstat, double *rscor,
                       uint8_t *flags);
int tq_resolve_species_dev(tq_ctx *ctx, const uint32_t *d_squartets, int64_t Q, uint32_t *d_rstat, double *d_rscor,
                           uint8_t *d_flags, void *stream);
int tq_resolve_species_debug(tq_ctx *ctx, const uint32_t *squartets, int64_t Q, uint32_t *rstat, double *rscor,
                             uint8_t *flags, uint32_t *cmats, double *svds, int32_t *ranks);

/* Site-pattern classes and ABBA-BABA D tests.  No reference counterpart in tetrad itself: the
 * class counts are what ipyrad's `baba` tool made of tetrad's count matrices.
 *   Rule: a pattern is four bases (x0, x1, x2, x3) in the order of the quartet's four taxa; its class is its
 *   restricted-growth string (position 0 gets label 0, every base not seen before the next label) and the 15 strings in
 *   lexicographic order number the classes: 0000 0001 0010 0011 0012 0100 0101 0102 0110 0111 0112 0120 0121 0122 0123.
 *   A class row is u32[16]: slots 0..14 the class counts, slot 15 their sum = the number of counted sites (rstat[:,1]
 *   of the same quartet).  Class 0 is zero unless option "count_invariant" is set.  With roles (P1, P2, P3, O) in
 *   positions 0..3, BBAA is class 3, BABA class 6 and ABBA class 8.  Permuting the four positions permutes the classes,
 *   so every role assignment of a taxon set is read off the row of its ASCENDING quartet.
 *   tq_pattern_class_table  out u8[256]: the class of pattern 64 x0 + 16 x1 + 4 x2 + x3 (host code, no context).
 *   tq_patterns        sets u32[Q,4], host buffers, synchronous; validated as tq_resolve validates its quartets, and a
 *                      row that is not strictly ascending is refused (TQ_ERR_INVALID_ARG naming the row) before anything
 *                      is launched.  classes u32[Q,16].  Q = 0 is valid.
 *   tq_patterns_dev    device pointers, enqueued on `stream` (the stream rule above): scan batches of at most option
 *                      "batch", each followed by the class kernel at the batch's offset.  The rows are the caller's
 *                      responsibility, as in tq_resolve_dev (an index >= T gives a row of zeros).
 *                      d_sets and d_classes must be 16-byte aligned (rows are read and written as 16-byte words):
 *                      a misaligned pointer is refused with TQ_ERR_INVALID_ARG before anything is launched.
 *   tq_patterns_species / tq_patterns_species_dev  the same on species quartets (ascending species ids) after
 *                      tq_set_species: the class counts of the pooled lineage combinations.  Refused when a species
 *                      resolve call would be.
 *   All four are refused (TQ_ERR_INVALID_ARG) while a timing-diagnostic mode is set (scan_method 2..5, phases 1 / 2):
 *   there is no flags array to mark the rows with.
 *   Timing (tq_timing_enable): a pattern call counts as one call of tq_timing_read* and records the marks of its scan
 *   (ordering, site scan; species: table, pooled counts); the class kernel runs behind the last mark, so its time is in
 *   none of the figures and the timing indices stay as they are.  Time it with events of your own around the call.
 *   tq_dstat_accumulate_dev  one replicate of N tests added on `stream`: test t reads a = classes[set_of[t]][ia[t]] and
 *                      b = classes[set_of[t]][ib[t]] (set_of u32[N], ia / ib u8[N] in 0..14: the classes that play ABBA
 *                      and BABA for the test) and, unless a + b = 0, adds d = (a - b) / (a + b) to its row of
 *                      acc f64[N][4] = {n, sum of d, sum of d * d, d of the last replicate added}.  Every operation is
 *                      rounded once (no fused multiply-add), replicates are added one after another by the same thread:
 *                      the result depends on the replicate order only and equals the host execution bit for bit.  A test
 *                      whose set_of >= n_sets or whose class index is above 14 is skipped without touching memory.
 *   tq_dstat_accumulate  the host execution (no context; messages go to tq_last_error(NULL)); such a test is refused
 *                      (TQ_ERR_INVALID_ARG) and nothing is added.                                                     */
int tq_pattern_class_table(uint8_t *out);
int tq_patterns(tq_ctx *ctx, const uint32_t *sets, int64_t Q, int subsample, uint32_t *classes);
int tq_patterns_dev(tq_ctx *ctx, const uint32_t *d_sets, int64_t Q, int subsample, uint32_t *d_classes, void *stream);
int tq_patterns_species(tq_ctx *ctx, const uint32_t *ssets, int64_t Q, uint32_t *classes);
int tq_patterns_species_dev(tq_ctx *ctx, const uint32_t *d_ssets, int64_t Q, uint32_t *d_classes, void *stream);
int tq_dstat_accumulate(const uint32_t *classes, int64_t n_sets, const uint32_t *set_of, const uint8_t *ia,
                        const uint8_t *ib, int64_t N, double *acc);
int tq_dstat_accumulate_dev(tq_ctx *ctx, const uint32_t *d_classes, int64_t n_sets, const uint32_t *d_set_of,
                            const uint8_t *d_ia, const uint8_t *d_ib, int64_t N, double *d_acc, void *stream);

/* Site-pattern classes per block of sites and the block-jackknife D test.  The error estimate of
 * D that ADMIXTOOLS, Dsuite and ipyrad's `baba` use; no reference counterpart in tetrad itself.
 *   Rule (full mode only): a site is counted for a set when none of its four bases is missing and, unless option
 *   "count_invariant" is set, the four are not all equal; its class is the one of section 18.  block_starts i64[B + 1]
 *   in HOST memory: block j = sites [block_starts[j], block_starts[j + 1]) of the resident replicate, with
 *   0 <= block_starts[0], a strictly increasing sequence, block_starts[B] <= S and 1 <= B <= 4096.  Sites outside every
 *   block count nowhere; blocks need not respect loci.  A block row is u32[16]: the class counts of the block's sites
 *   and their sum.  When the blocks tile [0, S) the sum of a set's block rows equals the row tq_patterns(subsample = 0)
 *   writes, bit for bit.  There is no subsample form (its one-SNP-per-locus choice is not a per-block function).
 *   tq_patterns_blocks      sets u32[Q,4], host buffers, synchronous; classes u32[Q][B][16].  Validated as tq_patterns
 *                      validates (NULL, negative Q, no data, an index >= T, a row not strictly ascending) plus the
 *                      block rule, all before anything is launched.  Q = 0 is valid.  Works in chunks of whole sets of
 *                      at most option "batch" items of Q * B.
 *   tq_patterns_blocks_dev  d_sets / d_classes device pointers (16-byte aligned: a misaligned pointer is refused with
 *                      TQ_ERR_INVALID_ARG before anything is launched), enqueued on `stream` under the stream rule
 *                      above, so it is ordered behind a tq_bootstrap_async that rebuilds the layout.  The rows are the
 *                      caller's responsibility (an index >= T gives rows of zeros).  block_starts is read before the call
 *                      returns and reaches the device without a synchronisation of the caller's stream: it is copied
 *                      into one of two page-locked staging pieces of the context (the host waits only for the copy that
 *                      used that piece two calls earlier) and from there, asynchronously on `stream`, into a device array
 *                      of the context.
 *   Both read the natural layout always (never the packed set of site_pack / boot_pack) and no option but
 *   "count_invariant" and, in the host form, "batch": not scan_method, not phases, no scan option.  Neither records a
 *   timing mark or counts as a call of tq_timing_read*.
 *   tq_dstat_jackknife_dev  one thread per test, enqueued on `stream`: test t reads the B block rows of set set_of[t],
 *                      a_j = row_j[ia[t]], b_j = row_j[ib[t]], m_j = a_j + b_j, and OVERWRITES its row of
 *                      out f64[N][4] = {g, theta, theta_J, var}: the delete-one-block jackknife with block weight m_j
 *                      (Busing, Meijer & van der Leeden 1999).  A = sum a_j, Bs = sum b_j, n = A + Bs, g = blocks with
 *                      m_j > 0 (integers).  n = 0: {0, NaN, NaN, NaN}.  theta = (A - Bs) / n.  g < 2: {g, theta, NaN,
 *                      NaN}.  Over the blocks with m_j > 0 in block order: r = n - m_j, theta_-j = ((A - a_j) - (Bs - b_j))
 *                      / r, sJ += (r / n) theta_-j; theta_J = g theta - sJ.  Then h = n / m_j, tau = h theta - (h - 1)
 *                      theta_-j, e = tau - theta_J, sV += (e e) / (h - 1); var = sV / g.  Every floating operation is one
 *                      correctly rounded double operation in that order (no fused multiply-add), so the result equals
 *                      the host execution bit for bit.  Standard error = sqrt(var), Z = D / standard error: the
 *                      caller's.  A test whose set_of >= n_sets or whose class index is above 14 is skipped without
 *                      touching memory.  1 <= B <= 4096.
 *   tq_dstat_jackknife  the host execution (no context; messages go to tq_last_error(NULL)); such a test, or B outside
 *                      1..4096, is refused (TQ_ERR_INVALID_ARG) and nothing is written.                               */
int tq_patterns_blocks(tq_ctx *ctx, const uint32_t *sets, int64_t Q, const int64_t *block_starts, int64_t B,
                       uint32_t *classes);
int tq_patterns_blocks_dev(tq_ctx *ctx, const uint32_t *d_sets, int64_t Q, const int64_t *block_starts, int64_t B,
                           uint32_t *d_classes, void *stream);
int tq_dstat_jackknife(const uint32_t *bclasses, int64_t n_sets, int64_t B, const uint32_t *set_of, const uint8_t *ia,
                       const uint8_t *ib, int64_t N, double *out);
int tq_dstat_jackknife_dev(tq_ctx *ctx, const uint32_t *d_bclasses, int64_t n_sets, int64_t B, const uint32_t *d_set_of,
                           const uint8_t *d_ia, const uint8_t *d_ib, int64_t N, double *d_out, void *stream);

/* Pooled site-pattern classes of SPECIES sets per block of sites: the block rows of section 20
 * for the species map of tq_set_species, so that tq_dstat_jackknife* give the block-jackknife D test between populations.
 *   Rule: for a species set (A, B, C, D) and a site s let a[x], b[x], c[x], d[x] (x = 0..3) be the lineages of each
 *   species with base x at s (a missing base counts nowhere; option "species_alleles": two lineages per sample).  The
 *   pooled count of class k at s is the sum of a[x0] b[x1] c[x2] d[x3] over the patterns (x0, x1, x2, x3) of class k:
 *   the number of lineage quartets (i in A, j in B, k in C, l in D) that show the class there.  Class 0 (xxxx) is always
 *   0, under either value of "count_invariant", as the invariant bins of the pooled matrix are; slot 15 is the sum of
 *   slots 1..14.  A block row is these counts summed over the block's sites; blocks and block_starts as above.  When
 *   the blocks tile [0, S) the sum of a set's block rows equals the row tq_patterns_species writes, bit for bit.  The
 *   counts are computed from the per-species base counts of the resident replicate (15 sums of products per site,
 *   inverted once per row), not from 256 bins; u32, exact under the range rule of species mode.
 *   tq_patterns_blocks_species      ssets u32[Q,4], host buffers, synchronous; classes u32[Q][B][16].  Refuses whatever
 *                      the species calls refuse (no data, no map, a map for another T, the range rule S x product of the
 *                      four largest species sizes >= 2^32, allele mode without a replicate built from the source), then
 *                      NULL, negative Q, the block rule, an id >= K and a row not strictly ascending, all before
 *                      anything is launched.  Q = 0 is valid.  Chunks by option "batch" as tq_patterns_blocks does.
 *   tq_patterns_blocks_species_dev  d_ssets / d_classes device pointers (16-byte aligned or refused before anything is
 *                      launched), enqueued on `stream` under the stream rule above: ordered behind a tq_bootstrap_async
 *                      that rebuilds the layout, and the species table follows the replicate without a tq_set_species
 *                      in between.  The rows are the caller's responsibility: an id >= K gives a row of zeros, and so
 *                      does a row that repeats species so that S x its own lineage product reaches 2^32.  block_starts
 *                      travels as in tq_patterns_blocks_dev.
 *   Neither reads scan_method, phases, count_invariant or species_method (only a species_method the map's sizes do not
 *   allow is refused, as by every species call); neither touches the count slab, records a timing mark or counts as a
 *   call of tq_timing_read*.
 *   tq_pooled_site_classes  host-only, no context: the rule for ONE site.  packed[4] = the four species' counts, each
 *                      {n_A, n_C, n_G, n_T} as bytes 0..3 of a word; out[16] = the class row of that site, computed by
 *                      the function the kernel runs (arithmetic modulo 2^32; counts up to 255^4 fit).               */
int tq_patterns_blocks_species(tq_ctx *ctx, const uint32_t *ssets, int64_t Q, const int64_t *block_starts, int64_t B,
                               uint32_t *classes);
int tq_patterns_blocks_species_dev(tq_ctx *ctx, const uint32_t *d_ssets, int64_t Q, const int64_t *block_starts, int64_t B,
                                   uint32_t *d_classes, void *stream);
int tq_pooled_site_classes(const uint32_t packed[4], uint32_t out[16]);

/* Five-taxon site-pattern classes per block of sites and the block jackknife on sums of slots: what
 * DFOIL (Pease & Hahn 2015) and partitioned D (Eaton & Ree 2013) are read from.  No reference counterpart in tetrad itself.
 *   Rule (full mode only): a set is five taxa t0 < t1 < t2 < t3 < t4 with bases x0..x4 at a site.  The site is counted
 *   when none of the five is missing and they take exactly two distinct values; its class is
 *   k = sum over i = 1..4 of [x_i != x_0] 2^(i - 1), in 1..15 (unpolarised: every role assignment is a relabelling on the
 *   host).  Invariant sites and sites with three or four bases count nowhere; "count_invariant" is not read.  A block
 *   row is u32[16]: slot k = the count of class k for k = 1..15, slot 0 = the sum of slots 1..15.  block_starts and B as
 *   in tq_patterns_blocks.
 *   tq_quintet_class_table  host-only: out u8[1024], index 256 x0 + 64 x1 + 16 x2 + 4 x3 + x4; 0 = not counted, else the
 *                      class 1..15, from the function the kernel's masks are checked against at compile time.
 *   tq_patterns_quintet_blocks      sets5 u32[Q,5], host buffers, synchronous; classes u32[Q][B][16].  Validated as
 *                      tq_patterns_blocks validates (NULL, negative Q, no data, an index >= T, a row not strictly
 *                      ascending, the block rule), all before anything is launched.  Q = 0 is valid.  Chunks by option
 *                      "batch" as tq_patterns_blocks does.
 *   tq_patterns_quintet_blocks_dev  d_sets5 (4-byte aligned) / d_classes (16-byte aligned; either misaligned is refused
 *                      before anything is launched) device pointers, enqueued on `stream` under the stream rule above, so
 *                      ordered behind a tq_bootstrap_async that rebuilds the layout.  The rows are the caller's
 *                      responsibility (an index >= T gives rows of zeros).  block_starts travels as in
 *                      tq_patterns_blocks_dev.
 *   Both read the natural layout always and no option but, in the host form, "batch"; neither records a timing mark or
 *   counts as a call of tq_timing_read*.
 *   tq_dstat_jackknife_masks_dev  one thread per test, one launch on `stream`: the jackknife of tq_dstat_jackknife_dev,
 *                      operation for operation (one definition serves both), with a_j = the sum of the slots of block
 *                      row j whose bit is set in lmask[t] and b_j the same for rmask[t] (u16 arrays; bit k = slot k).
 *                      a_j + b_j <= 15 (2^32 - 1), n < 2^48: every integer is exact.  OVERWRITES out f64[N][4] =
 *                      {g, theta, theta_J, var}.  A test is valid when bit 0 is clear in both masks, both are non-empty
 *                      and they are disjoint; an invalid test, or one whose set_of >= n_sets, is skipped without
 *                      touching memory.  1 <= B <= 4096.  Works on any u32[.][B][16] rows, the four-taxon ones included.
 *   tq_dstat_jackknife_masks  the host execution (no context; messages go to tq_last_error(NULL)); an invalid test, or B
 *                      outside 1..4096, is refused (TQ_ERR_INVALID_ARG) and nothing is written.                       */
int tq_quintet_class_table(uint8_t out[1024]);
int tq_patterns_quintet_blocks(tq_ctx *ctx, const uint32_t *sets5, int64_t Q, const int64_t *block_starts, int64_t B,
                               uint32_t *classes);
int tq_patterns_quintet_blocks_dev(tq_ctx *ctx, const uint32_t *d_sets5, int64_t Q, const int64_t *block_starts, int64_t B,
                                   uint32_t *d_classes, void *stream);
int tq_dstat_jackknife_masks(const uint32_t *bclasses, int64_t n_sets, int64_t B, const uint32_t *set_of,
                             const uint16_t *lmask, const uint16_t *rmask, int64_t N, double *out);
int tq_dstat_jackknife_masks_dev(tq_ctx *ctx, const uint32_t *d_bclasses, int64_t n_sets, int64_t B,
                                 const uint32_t *d_set_of, const uint16_t *d_lmask, const uint16_t *d_rmask, int64_t N,
                                 double *d_out, void *stream);

/* Pooled five-taxon site-pattern classes of SPECIES sets per block of sites: the block rows of
 * section 22 for the species map of tq_set_species, so that tq_dstat_jackknife_masks* give DFOIL and partitioned D between
 * populations.
 *   Rule: a species set is five ids k0 < k1 < k2 < k3 < k4; n_i[x] (x = 0..3) is the number of lineages of species k_i
 *   with base x at a site (a missing base counts nowhere; option "species_alleles": two lineages per sample).  The pooled
 *   count of class k = 1..15 at the site is the number of lineage quintets, one lineage per species in position order,
 *   whose five bases take exactly two values and whose class (tq_quintet_class_table) is k.  With M the positions i >= 1
 *   whose bit i - 1 is set in k, Mc the other positions and d(T) = sum over x of the product over i in T of n_i[x], it
 *   equals d(Mc) d(M) - d({0,1,2,3,4}).  Invariant sites and sites with three or four bases count nowhere;
 *   "count_invariant" is not read.  A block row is u32[16]: slot k = the count of class k summed over the block's sites,
 *   slot 0 = the sum of slots 1..15; blocks and block_starts as in tq_patterns_blocks.  u32, exact under the range rule
 *   S x product of the five largest species sizes < 2^32 (sizes in lineages).
 *   tq_patterns_quintet_blocks_species      ssets5 u32[Q,5], host buffers, synchronous; classes u32[Q][B][16].  Refuses
 *                      NULL and negative Q, whatever the species calls refuse (no data, no map, a map for another T, the
 *                      range rule of four species, allele mode without a replicate built from the source), the range rule
 *                      of five species above, the block rule, an id >= K and a row not strictly ascending, all before
 *                      anything is launched.  Q = 0 is valid.  Chunks by option "batch" as tq_patterns_blocks does.
 *   tq_patterns_quintet_blocks_species_dev  d_ssets5 (4-byte aligned) / d_classes (16-byte aligned; either misaligned is
 *                      refused before anything is launched) device pointers, enqueued on `stream` under the stream rule
 *                      above: ordered behind a tq_bootstrap_async that rebuilds the layout, and the species table follows
 *                      the replicate without a tq_set_species in between.  The rows are the caller's responsibility: an
 *                      id >= K gives a row of zeros, and so does a row that repeats species so that S x its own lineage
 *                      product reaches 2^32.  block_starts travels as in tq_patterns_blocks_dev.
 *   Neither reads scan_method, phases, count_invariant or species_method (only a species_method the map's sizes do not
 *   allow is refused, as by every species call); neither touches the count slab, records a timing mark or counts as a
 *   call of tq_timing_read*.  tq_dstat_jackknife_masks* take the rows as they are: a_j + b_j <= 15 (2^32 - 1).
 *   tq_pooled_quintet_site_classes  host-only, no context: the rule for ONE site.  packed[5] = the five species' counts
 *                      in position order, each {n_A, n_C, n_G, n_T} as bytes 0..3 of a word; out[16] = the class row of
 *                      that site, computed by the functions the kernel runs (arithmetic modulo 2^32; counts up to 255^4
 *                      x 255 that fit u32 are exact).                                                                 */
int tq_patterns_quintet_blocks_species(tq_ctx *ctx, const uint32_t *ssets5, int64_t Q, const int64_t *block_starts, int64_t B,
                                       uint32_t *classes);
int tq_patterns_quintet_blocks_species_dev(tq_ctx *ctx, const uint32_t *d_ssets5, int64_t Q, const int64_t *block_starts,
                                           int64_t B, uint32_t *d_classes, void *stream);
int tq_pooled_quintet_site_classes(const uint32_t packed[5], uint32_t out[16]);

/* Site concordance factors per branch of a fixed tree: sCF / sDF1 / sDF2 / sN of Minh, Hahn &
 * Lanfear 2020 from the class rows above.  No reference counterpart in tetrad itself.
 *   Rule: a row is a set (a, b, c, d) with its class row u32[16] as the pattern calls write it.  The tree gives the
 *   row's edge and its resolution r there exactly as the concordance accumulator does (a row induced on no edge counts
 *   nowhere; a taxon >= T or a repeated taxon sends it to `skipped`).  n0, n1, n2 = classes 3, 6, 8: the sites that
 *   support resolution 0, 1, 2 of the row as given; inf = n0 + n1 + n2.  conc = n_r, d1 = n of the lower of the two
 *   other indices, d2 = n of the remaining one.  inf = 0: the edge's nq_zero += 1 and nothing else.  Otherwise nq += 1,
 *   sum_x += x and fx_x += floor(x * 2^32 / inf) for x = conc, d1, d2.  Every sum is an unsigned 64-bit integer, so
 *   host adds, device adds and any order of addition agree bit for bit.  sCF = 100 fx_conc / (nq 2^32).
 *   tq_scf_create   tree as tq_conc_create takes it (4 <= T <= 4096, same unrooting, edges and edge order).  `ctx` may
 *                   be NULL: then only tq_scf_add works.  The context must outlive the accumulator; messages go to
 *                   tq_last_error(ctx) (tq_last_error(NULL) without one).
 *   tq_scf_add      host rows, synchronous: sets u32[n,4], classes u32[n,16] (slot 15 is not read).  n = 0 is valid.
 *   tq_scf_add_dev  the same rows as device pointers, enqueued on `stream` (hipStream_t, NULL = default stream),
 *                   allocation-free; calls on different streams are ordered in call order.  d_sets and d_classes must be
 *                   16-byte aligned: a misaligned pointer is refused with TQ_ERR_INVALID_ARG before anything is launched.
 *   tq_scf_read     waits for the device adds and returns the sums of every add since create / reset, any output may be
 *                   NULL: edge_counts i64[E][8] = {nq, nq_zero, sum_conc, sum_d1, sum_d2, fx_conc, fx_d1, fx_d2} (the
 *                   u64 sums as their bit patterns), masks u64[E][W] and the edge order as tq_conc_read gives them for
 *                   the same tree, *skipped.  E, W: tq_scf_shape.                                                     */
typedef struct tq_scf tq_scf;
int tq_scf_create(tq_scf **out, const int32_t *parent, int64_t n_nodes, int64_t T, tq_ctx *ctx);
void tq_scf_destroy(tq_scf *acc);
int tq_scf_reset(tq_scf *acc);
int tq_scf_add(tq_scf *acc, const uint32_t *sets, const uint32_t *classes, int64_t n);
int tq_scf_add_dev(tq_scf *acc, const uint32_t *d_sets, const uint32_t *d_classes, int64_t n, void *stream);
int tq_scf_shape(const tq_scf *acc, int64_t *T, int64_t *n_edges, int64_t *mask_words);
int tq_scf_read(tq_scf *acc, int64_t *edge_counts, uint64_t *masks, int64_t *skipped);

/* All-pairs taxon counts per block of sites, and neighbour joining.  No reference counterpart.
 *   Rule (full mode, every site counts; "count_invariant" is not read): for taxa i, j and the sites of a block, both = the
 *   sites present (tmparr <= 3) in i and in j, diff = of those the sites whose bases differ, ts = of the differing ones
 *   the transitions (A<->G, C<->T with A, C, G, T = 0..3), tv = diff - ts.  A pair row is u32[4] = (both, diff, ts, tv);
 *   row (i, i) is (sites present in i, 0, 0, 0); the matrix is symmetric.  Blocks and block_starts exactly as
 *   tq_patterns_blocks takes them (host memory, B + 1 strictly increasing boundaries inside [0, S], 1 <= B <= 4096; sites
 *   outside every block count nowhere).  Output u32[B][T][T][4].  Exact integers: host and device, any option value, any
 *   stream give the same array.
 *   tq_taxon_counts        host buffer, synchronous.  Reads the resident replicate in the natural layout always.  Refuses
 *                     NULL, no data and the block rule before anything is launched.  Works in chunks of whole blocks
 *                     whose rows fit option "taxdist_scratch_bytes" (default 256 MiB, 0 = default, negative refused; one
 *                     block where a block alone exceeds it).
 *   tq_taxon_counts_dev    d_out a device pointer, 16-byte aligned or refused; enqueued on `stream` under the stream rule
 *                     above, so it is ordered behind a tq_bootstrap_async.  block_starts is read before the call returns;
 *                     the work items made of it reach the device through two page-locked staging pieces in turn, without
 *                     a synchronisation of the caller's stream (the host waits only for the copy that used the piece two
 *                     launches earlier; a launch holds 65 535 work items).
 *   tq_taxon_counts_host   the same rule on tmparr u8[T][S] (a cell above 3 is missing), no context: T >= 2, S >= 1, the
 *                     block rule against S; messages go to tq_last_error(NULL).
 *   tq_taxon_counts_stats  out i64[5], of the last counts call of the context: tile pairs, work items, u64 words of a work
 *                     item (option "taxdist_slice_words", a multiple of 8, 0 = default; no result depends on it), blocks
 *                     per chunk, chunks.
 *   Neither counts call records a timing mark or counts as a call of tq_timing_read*.
 *   tq_nj_tree   neighbour joining, host code, no context.  dist f64[T][T], T >= 3; refused when an off-diagonal entry is
 *                not finite or dist[i][j] != dist[j][i] (the message names the pair); the diagonal is ignored, negative
 *                entries are allowed.  Nodes 0..T-1 are the taxa, new nodes T, T+1, ...; the active list is kept in
 *                ascending id.  A round with n > 3 active nodes: r_i = the sum of d(i, k) over the active k != i in ascending
 *                id; Q(i, j) = ((n - 2) d(i, j) - r_i) - r_j; the smallest Q is joined, ties to the lexicographically
 *                lowest (i, j), i < j; l_i = 0.5 d(i, j) + (r_i - r_j) / (2 (n - 2)), l_j = d(i, j) - l_i, d(u, k) = 0.5
 *                ((d(i, k) + d(j, k)) - d(i, j)).  With n = 3 the active i < j < k become children of node 2T - 3 with l_i =
 *                0.5 ((d_ij + d_ik) - d_jk), l_j = 0.5 ((d_ij + d_jk) - d_ik), l_k = 0.5 ((d_ik + d_jk) - d_ij).  Every
 *                floating operation is one correctly rounded double operation in that order.  parent i32[2T - 2]
 *                (parent[root] = -1), length f64[2T - 2] (the root's is 0; negative lengths are returned as computed). */
int tq_taxon_counts(tq_ctx *ctx, const int64_t *block_starts, int64_t B, uint32_t *out);
int tq_taxon_counts_dev(tq_ctx *ctx, const int64_t *block_starts, int64_t B, uint32_t *d_out, void *stream);
int tq_taxon_counts_host(const uint8_t *tmparr, int64_t T, int64_t S, const int64_t *block_starts, int64_t B, uint32_t *out);
int tq_taxon_counts_stats(tq_ctx *ctx, int64_t *out);
int tq_nj_tree(const double *dist, int64_t T, int32_t *parent, double *length);

/* Device facts used by bench.py: writes CU count, wave slots used by the resolve
 * kernel per CU and the padded row pitch in bytes.                                 */
int tq_device_info(tq_ctx *ctx, int32_t *num_cu, int32_t *waves_per_cu, int64_t *row_pitch);

#ifdef __cplusplus
}
#endif
#endif /* TETRAD_HIP_H */
