// tetrad_hip.hip -- MI355X (gfx950 / CDNA4) quartet-invariant engine.
//
// Hand-written HIP for the per-quartet hot path of eaton-lab/tetrad
// (reference: tetrad/src/resolve_quartets.py:191-265 and the count kernels
// :42-104).  Not a translation: the reference is an interpreted per-quartet
// loop around a serial site scan and six LAPACK calls; here one 64-lane
// wavefront owns a quartet during the site scan (four neighbours of the sorted
// order form a workgroup that shares what depends on their common taxa a,b),
// four lanes own a matrix during bidiagonalisation and one lane owns it during
// the QR iteration.
//
// Data layout in HBM (built once per replicate by tq_set_data / tq_bootstrap):
//   rows    u8   [T][Sp]   base code 0..3 per site, missing/pad -> 0  (Sp = S rounded up to 2048;
//                          inside each 2048-site step the bytes sit in two 1 KiB panels, row_offset())
//   nib     u8   [T][Sp/2] the same codes, two per byte (nib_offset())
//   nib5    u8   [T][Sp/2] the same with 4 for a missing cell (rows d1, d2 of the joint-histogram scan)
//   planes  u32x4[T][W]    per 32 sites: {missing bits, base bit 0, base bit 1, run-begin bits}, W = Sp/32
//   planes3 u32x3[T][W]    compact copy {missing, bit 0, bit 1}; runbeg u32 [W] run-begin bits, stored once
//   and, when it pays, a second rows / nib / planes / planes3 + runbeg set in the packed site order (pack.hpp)
//
// Kernels (each in its own header of this directory, all included below into one translation unit):
//   pinned_pool.hpp (host) the process-wide pool of page-locked blocks (tq_host_alloc, result and array staging)
//   device_mem.hpp (host) DevBuf / PinnedBuf, the owners of every device and page-locked block; Event / Stream / PoolBuf,
//                 the owners of every event, stream and pool block; StagingRing; and SiteSet, one layout set
//   prepare.hpp   layout build, lexicographic unranking, sort keys
//   pack.hpp      (host) packed site order for the subsample-mode scans: whole loci per lane word (option site_pack)
//   scan.hpp      tq_scan_wg_kernel / tq_scan_kernel: site scan -> 256 pattern counts per quartet (nibble codes + plane
//                 records; the one-wave-per-quartet kernel of small calls)
//   scan_f4.hpp   tq_scan_f4_kernel: the cooperative scan on 12-byte plane records only (default of subsample mode)
//   scan_dp.hpp   tq_scan_dp_kernel: two quartets that share three taxa per wave, one joint histogram (default of full mode
//                 from 32 768 quartets on); unit list from the sorted order
//   scan_pb.hpp   tq_scan_pb_kernel: bank-private counters (A/B form)
//   scan_plan.hpp (host) choose_scan: which of the scan kernels takes a batch, and its grid
//   hqr.hpp       tq_bidiag_kernel + tq_bdsqr_kernel + tq_score_kernel: singular values (default)
//   jacobi.hpp    tq_svd_kernel: one-sided Jacobi singular values in registers (alternative)
//   bootstrap.hpp tq_boot_*: bootstrap replicate built on the device
//   concordance.hpp tq_conc_kernel + tq_conc_fold_kernel: quartet concordance counters of resolved rows on a fixed tree
//   scf.hpp         tq_scf_kernel (tables, geometry and fold of concordance.hpp): site concordance sums of class rows
//   supertree.hpp tq_stree_*_kernel: rows -> weighted splits, graph and partition passes of the exact quartet supertree
//   fit.hpp       tq_fit_*_kernel: LCA-depth tables of candidate trees, quartet fit of the supertree's kept rows against them
//   nni.hpp       tq_nni_*_kernel: the quartet-fit weights of every nearest-neighbour interchange of a tree in one row pass; the polish search
//   consensus.hpp tq_cons_*_kernel: split masks of many trees, exact split counts in a hash table (majority-rule consensus)
//   split_table.hpp (host) TreeChunk and SplitTable: the staged chunk of trees and the split table that the accumulators
//                 of consensus.hpp, tbe.hpp and treedist.hpp share (included below StreamOrder, not with the kernels)
//   bit_tile.hpp  bit_tile_product: the 64 x 64 tile product on bit rows inside the product kernels of the next three
//   tbe.hpp       tq_tbe_kernel: transfer distances of a reference tree's branches to every node of many trees (TBE)
//   treedist.hpp  tq_rf_*_kernel: split ids, bit rows and their product: all-pairs Robinson-Foulds distances of a tree set
//   qdist.hpp     tq_qd_*_kernel: quartet topology planes of every tree and their product: all-pairs quartet distances of a tree set
//   stability.hpp tq_ls_count_kernel: the same planes summed along the trees: quartet frequencies and leaf stability sums
//   species.hpp   tq_species_table_kernel / tq_species_allele_table_kernel (base counts per species from the resident
//                 rows / from both alleles of the IUPAC source) + tq_species_mfma_kernel / tq_species_pool_kernel: pooled
//                 count matrices of species quartets (species mode; MFMA form, VALU form)
//   pattern_blocks.hpp the class masks of a quartet's block rows + tq_jackknife_kernel: the block jackknife of D
//   quintet_blocks.hpp tq_quintet_blocks_kernel: five-taxon class rows per block of sites + the mask form of
//                 tq_jackknife_kernel: the block jackknife on sums of slots (DFOIL, partitioned D)
//   species_blocks.hpp, species_quintet_blocks.hpp the arithmetic of pooled four- and five-species block rows (species table)
//   block_rows.hpp tq_block_rows_kernel<Rule>: the per-block class-row kernel, its plane walk and table walk, and the
//                 rules of quartets, species and species quintets on the arithmetic of the headers above
//   taxdist.hpp   tq_taxon_counts_kernel + tq_taxon_finish_kernel: the tile product on the plane records themselves: shared
//                 sites, differences, transitions and transversions of every pair of taxa per block of sites
//   nj.hpp        (host) neighbour joining on a distance matrix
// This file holds the context, the launch logic and the C ABI (include/tetrad_hip.h).
//
// The rules of the C boundary, each written once below:
//   api()          every entry point that can allocate host memory or that touches the device runs its body under this
//                  guard: the context's device is selected (no context: host back ends, context-free calls) and no
//                  exception leaves extern "C".  std::bad_alloc gives TQ_ERR_OOM "<name>: out of host memory";
//                  std::length_error (a size past max_size(): more memory was asked for than exists) gives TQ_ERR_OOM
//                  and any other std::exception TQ_ERR_INVALID_ARG, both with "<name>: <what()>".  Helpers below a
//                  guarded entry point neither select the device nor catch.  Accessors that copy scalars stay bare.
//   TQ_HIP / TQ_HIPF / TQ_LAUNCHED   early-return checks of a HIP call ("<call> failed: ..." / "<who>: ...") and of the
//                  launches before it ("<who>: launch failed: ..."); hipErrorOutOfMemory maps to TQ_ERR_OOM, anything
//                  else to TQ_ERR_HIP.  The accumulator creates hold their object in a std::unique_ptr and release it
//                  into *out on success; where a failure must release context state (free_data, free_source) an inner
//                  function returns early and its caller frees.
//   Options / OPTION_TABLE   the option fields with their defaults, and the one table tq_set_option looks names up in.
//
// Bounds: the scan is L2 / LDS-atomic / VALU work on a <= 40 MB resident matrix (HBM only on
// first touch), the singular-value stage is f64 VALU.  Algorithmic bytes per quartet: 4*S + 48
// (SURVEY.md 8d).  DESIGN.md section 4 has the per-kernel description and measurements.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <utility>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/tetrad_hip.h"

namespace {

#include "common.hpp"
#include "pinned_pool.hpp"
#include "device_mem.hpp"
#include "prepare.hpp"
#include "pack.hpp"
#include "scan.hpp"
#include "scan_pb.hpp"
#include "scan_dp.hpp"
#include "scan_f4.hpp"
#include "scan_plan.hpp"
#include "jacobi.hpp"
#include "hqr.hpp"
#include "bootstrap.hpp"
#include "format.hpp"
#include "qmc.hpp"
#include "concordance.hpp"
#include "species.hpp"
#include "supertree.hpp"
#include "consensus.hpp"
#include "bit_tile.hpp"
#include "tbe.hpp"
#include "treedist.hpp"
#include "fit.hpp"
#include "qdist.hpp"
#include "stability.hpp"
#include "nni.hpp"
#include "patterns.hpp"
#include "pattern_blocks.hpp"
#include "species_blocks.hpp"
#include "quintet_blocks.hpp"
#include "species_quintet_blocks.hpp"
#include "block_rows.hpp"
#include "scf.hpp"
#include "taxdist.hpp"
#include "nj.hpp"

}  // namespace

// ======================================================================================
// host side: context + C ABI
// ======================================================================================
enum { TAG_ORIGIN = -1, TAG_ORDER = 0, TAG_SCAN = 1, TAG_BIDIAG = 2, TAG_BDSQR = 3, TAG_SCORE = 4, TAG_COUNT = 5 };

// Every HIP resource below sits in an owner (device_mem.hpp), so `delete ctx` with the device selected releases all of
// it and the order of the members does not matter: a staging ring waits for its own copies before it gives its pieces
// back, and hipFree and hipStreamDestroy are safe with work queued.  Nothing is created before its first use.
struct tq_ctx {
    // What tq_set_option sets (OPTION_TABLE below names the fields and their legal values).  These initialisers are the only
    // place a default is written: "0 = default" reads it from a default-constructed Options.
    struct Options {
        int nrep = 1;
        int waves_per_cu = 0;           // 0 = from the occupancy query
        int phases = 3;                 // diagnostics only: 1 = scan kernel only, 2 = SVD kernel only
        int scan_method = -1;           // 0 = EXEC-masked slot per site, 1 = set-bit walk, 6 = bank-private counters (scan_pb.hpp,
                                        // A/B form; 0 / 1 where it does not apply); -1 = 1 if subsample else 0
        int64_t batch = 1 << 23;        // quartets per scan batch (8 GiB count slab)
        int order = 1;                  // 1 = process quartets in (a,b,c)-sorted order
        int scan_f4 = -1;               // the cooperative scan on 12-byte plane records only (SURVEY 8 row f4 as written; scan_f4.hpp):
                                        // -1 = in subsample mode (c3 scan 5.81 -> 5.58 ms), 1 = in both modes, 0 = never
        int scan_dp = 1;                // 1 = full-mode batches of >= dp_min_quartets go to tq_scan_dp_kernel (two quartets that share
                                        // (a,b,c) per wave, one LDS atomic per site and pair)
        int64_t dp_min_quartets = 32768;
        int64_t svd_chunk = 1 << 18;    // quartets per pass of the singular-value stage (and per result D2H piece)
        int svd_streams = 2;            // chunks alternate between this many streams (1 or 2) so that the tail of one
                                        // chunk's kernels is filled by the next chunk's (each stream has its own scratch)
        int svd_method = 1;             // 0 = one-sided Jacobi (tq_svd_kernel), 1 = Householder + bidiagonal QR
        int bidiag_layout = 1;          // 1 = matrix dealt 2 x 2 over the quad (tq_bidiag2_kernel), 0 = four column groups
        int bdsqr_maxit = 60;           // QR sweeps per singular value before a matrix is declared not converged
        int scan_wg = 4;                // waves per workgroup of the cooperative scan kernel (1 = one wave per quartet)
        int64_t wg_min_quartets = 4096; // smaller batches go to the one-wave-per-quartet kernel: a call of a few thousand quartets does not
                                        // fill the chip and is bound by the latency of one quartet's 25 dependent steps, which the
                                        // cooperative kernels' per-step barrier and image hand-over only lengthen (1 000 random
                                        // quartets 0.185 -> 0.164 ms per call, 3 000: 0.198 -> 0.191; the cooperative kernels win from
                                        // ~4 000 on: tools/experiments/wg_min_threshold.py)
        int xcd_remap = 1;              // 1: scan workgroups of one XCD take a contiguous part of the sorted order
        int count_invariant = 0;        // 1: invariant sites (all four bases equal, none missing) are counted as well -- what the reference's
                                        // count kernels do when their caller's mask leaves such a site open (resolve_quartets.py:59-64);
                                        // the worker itself always masks them (:218).  One-wave-per-quartet kernel only.
        int scan_pair = 0;              // 1: two quartets per wavefront (tq_scan_wg2_kernel)
        int park_t = 1;                 // 1 (default): transposed pattern park of the set-bit walk (conflict-free byte reads at the price of
                                        // 2 more VALU per counted site: c3 6.79 -> 6.42 ms); 0: lane-contiguous park (A/B)
        int share_c = 0;                // 1: scan kernel variant that also shares row c inside a workgroup (scan.hpp: SHC;
                                        // measured slower everywhere -- the kernel is LDS/VALU-bound, not byte-bound -- kept as an A/B option)
        int svd_wpc = 0;                // blocks per CU of the bidiag / bdsqr grids (0 = one pass per block)
        int cons_hash_bits = 64;        // consensus: the table key is the 64-bit mask hash cut to this many bits (results never depend on it;
                                        // read by tq_cons_create / tq_cons_reset)
        int64_t cons_scratch_bytes = int64_t(256) << 20;   // consensus: device + page-locked bytes of one chunk of trees (read at create)
        int64_t fit_scratch_bytes = int64_t(64) << 20;     // quartet fit: device bytes of the tables of one chunk of trees (no result depends on it)
        int64_t qdist_scratch_bytes = int64_t(256) << 20;  // quartet distances: device + page-locked bytes of one chunk of quartets (read at create)
        int qdist_kslices = 0;          // quartet distances: k slices of the product, 0 = chosen from the compute units (read at every score)
        int stree_lds = 1;              // supertree graph pass: 1 = private LDS counters where a level's cells fit, 0 = global atomics only
        int stree_search_dev = 1;       // supertree rule "exact" on device rows: 1 = the search kernel, 0 = the same rule on the host (A/B)
        int species_method = -1;        // -1: MFMA form when every species holds <= SPECIES_MFMA_MAX lineages, else VALU;
                                        // 0: VALU form (tq_species_pool_kernel); 1: MFMA form (tq_species_mfma_kernel)
        int species_alleles = 0;        // 1: every sample is two lineages, the alleles of its IUPAC genotype
        int site_pack = -1;             // -1: tq_set_data builds the packed set when the predicted scan cost falls (pack.hpp), 1: always
                                        // (while subsample mode is possible), 0: never, and a built set is not used
        int64_t taxdist_scratch_bytes = int64_t(256) << 20;    // taxon counts: device bytes of one chunk of whole blocks of the host-buffer
                                        // call (one block where a block alone exceeds it; no result depends on it)
        int taxdist_slice_words = TD_SLICE_WORDS;   // taxon counts: u64 words of a work item, a multiple of 8 (A/B: no result depends on it)
        int boot_pack = 0;              // 1: every replicate is packed, -1: when the rule said so for the source (boot_pack_auto),
                                        // 0: never (the replicate keeps the natural layout only); site_pack = 0 overrides
    };
    int device = 0;
    std::string err;
    hipDeviceProp_t prop{};
    // replicate data
    int64_t T = 0, S = 0;
    SiteSet nat;                    // the natural layout set (device_mem.hpp); its arrays are re-used by bootstrap replicates
    bool have_data = false;
    bool locus_runs_ok = false;
    // bootstrap source (tq_set_source): ASCII seqarr [T][S0], spans i64 [nloci][2]
    DevBuf<uint8_t> d_seqarr;
    DevBuf<int64_t> d_spans;
    int64_t src_T = 0, src_S0 = 0, nloci = 0, max_width = 0;
    DevBuf<int64_t> d_lidxs;        // [nloci]
    std::vector<int64_t> h_spans;   // host copy of the spans (replicate lengths are computed on the host)
    StagingRing<int64_t> lidx_ring; // a piece: the resampled locus indices i64 [nloci], behind them the packed starts u32 [nloci]
    DevBuf<uint32_t> d_boot;       // widths/offsets [nloci+1] | src_col [cap] | site_locus [cap]
    int64_t boot_cap = 0;
    DevBuf<char> d_boot_tmp;
    size_t boot_tmp_bytes = 0;
    // scratch for the host-buffer API (grow-only, in bytes)
    DevBuf<char> d_scratch;
    // count slab between the scan and the singular-value stage: u32 [batch][256]; ordering scratch
    DevBuf<uint32_t> d_cm;
    int64_t cm_quartets = 0;
    DevBuf<uint32_t> d_sort;        // 4 arrays of cm_quartets u32: keys/idx in, keys/idx out
    DevBuf<char> d_sort_tmp;
    size_t sort_tmp_bytes = 0;
    DevBuf<uint2> d_units;          // cm_quartets + 2 entries: unit list of the joint-histogram scan (scan_dp.hpp), then its count
    // singular-value stage scratch, sized for one chunk of `svd_chunk` quartets and re-used chunk after
    // chunk (so the bidiagonals / values of a chunk stay in the Infinity Cache between its three kernels):
    // de f64[3*chunk][32], sv f64[3*chunk][16], nsnps u32[chunk]
    DevBuf<double> d_de, d_sv;
    DevBuf<uint32_t> d_nsnps;
    int64_t svd_quartets = 0;
    Stream sX;                      // the second stream of the singular-value stage
    Event evFork, evJoin;
    DevBuf<uint64_t> d_bdsqr_stats;      // diagnostics (option "bdsqr_stats"): {matrices, rotation steps of all lanes,
                                         // lane-slots issued (64 x wave iterations), sweeps} summed over the launches
    // what tq_scan_dev left in the count slab (consumed by tq_svd_dev)
    const uint32_t *scanned_q = nullptr;
    int64_t scanned_Q = 0;
    int64_t scanned_T = 0;          // index bound of its rows (T; K for species rows): the score kernel flags ids >= it
    // species mode (tq_set_species, species.hpp): sample -> species map and the per-replicate species table, rebuilt
    // lazily on the stream of the first species call after the resident data changed (data_gen != sp_tab_gen)
    int64_t sp_T = 0, sp_K = 0;     // sp_K = 0: no map set
    std::vector<int32_t> sp_size;   // lineages per species
    uint64_t sp_bound = 0;          // product of the four largest species sizes (range rule: S * sp_bound < 2^32)
    uint64_t sp_bound5 = 0;         // product of the five largest (of all four where K = 4): the rule of five-species rows
    int32_t sp_max = 0;             // largest species size
    DevBuf<int32_t> d_sp_members;   // offsets [K+1], then the member samples grouped by species [T], then 2 x offsets [K+1]
    DevBuf<uint32_t> d_sp_tab;      // u32 [K][Sp]: {n_A, n_C, n_G, n_T} per species and site, then u8 [K][4][Sp] (MFMA form):
                                    // two u32 per (species, site) entry, grow-only
    uint64_t data_gen = 0;          // bumped by tq_set_data / tq_bootstrap(_async)
    uint64_t sp_tab_gen = ~0ull;    // data_gen the species table was built from (~0: none)
    // allele mode (option species_alleles): the table is built from the IUPAC source through the
    // resident replicate's site map (src_col in d_boot), every sample two lineages.  The map is the resident replicate's
    // exactly while boot_gen == data_gen (tq_bootstrap_async built what is resident) and boot_src_gen == src_gen (from
    // the source that is still the current one).
    uint64_t src_gen = 0;           // bumped by tq_set_source
    uint64_t boot_gen = ~0ull;      // data_gen of the last replicate tq_bootstrap_async built (~0: none)
    uint64_t boot_src_gen = ~0ull;  // src_gen it was built from
    // packed layout set `pk` (pack.hpp): a second copy of rows / nib / planes / planes3 + runbeg (no nib5) with whole loci per
    // lane word, read by the subsample-mode scans while it is current (pk_gen == data_gen).  tq_set_data builds it under site_pack,
    // tq_bootstrap_async under boot_pack (a replicate built without it leaves the set stale).  Everything else reads the
    // natural set.
    SiteSet pk;                     // its arrays grow only while T stays
    uint64_t pk_gen = ~0ull;        // data_gen the set was built from (~0: none)
    // the most recent scan launch (tq_debug_fetch which = 6): its kernel form (SCAN_FORM_*, 0 = none yet), T * pitch of
    // the layout set it read and whether that was the packed set
    int last_scan_form = 0;
    int64_t last_scan_tpitch = 0;
    int last_scan_packed = 0;
    // packed set of a device-built replicate (bootstrap.hpp: tq_boot_pack_*): planned on the host at locus level
    bool boot_pack_auto = false;    // pack_pays for the source matrix (tq_set_source): a replicate resamples its loci
    bool pk_from_boot = false;      // the packed set was built by tq_bootstrap_async (d_pk_src is its map)
    PackPlanner boot_plan;
    DevBuf<uint32_t> d_pstart;      // [nloci] packed start of every resampled locus (staged behind the indices in lidx_ring)
    DevBuf<uint32_t> d_pk_src;      // packed position -> natural site of the replicate, 0xFFFFFFFF = pad (grow-only)
    // host-buffer API: own compute and copy streams, events for the D2H pipeline
    Stream sK, sC;
    std::vector<Event> pipe_events;
    // the asynchronous device API (caller's stream) and the synchronous host API (stream sK) share the count
    // slab, the ordering scratch and the singular-value scratch: the last device-API enqueue records this event
    // and the host API makes sK wait for it before it touches any of them
    Event evDevApi;
    bool dev_api_pending = false;
    hipStream_t last_dev_stream = nullptr;   // stream of the last device-API enqueue (enter_dev_api orders across streams)
    // block boundaries of tq_patterns_blocks* (pattern_blocks.hpp): one device array, filled on the call's stream through
    // a staging ring
    DevBuf<int64_t> d_bstarts;      // [PBLK_MAX_BLOCKS + 1]
    StagingRing<int64_t> bstarts_ring;
    // work items of tq_taxon_counts* (taxdist.hpp): one device array of TD_LAUNCH_ITEMS items, filled launch by launch on
    // the call's stream through a staging ring
    DevBuf<TdItem> d_td_items;
    StagingRing<TdItem> td_ring;
    int64_t td_stats[5] = {0, 0, 0, 0, 0};      // of the last call: tile pairs, work items, slice words, blocks per chunk, chunks
    Options opt;                    // tq_set_option
    int pb_ok = 0;                  // tq_scan_pb_kernel's counters sit on a 64 KiB LDS boundary (probed once in tq_create)
    // timing: a sequence of tagged HIP events on the launch stream; the time between two consecutive
    // marks is attributed to the tag of the later one (TAG_ORIGIN starts a sequence)
    bool timing = false;
    struct Mark { int tag; int lane; Event ev; };           // lane: 0 = caller's stream, 1 = sX
    std::vector<Mark> marks;
    std::vector<Event> event_pool;
    int64_t timed_calls = 0;
};

namespace {

using Options = tq_ctx::Options;

std::string g_create_err;

int fail(tq_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    try {
        if (ctx) ctx->err = buf; else g_create_err = buf;
    } catch (...) {
    }
    return code;
}

#define TQ_HIP(ctx, call)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(ctx, e_ == hipErrorOutOfMemory ? TQ_ERR_OOM : TQ_ERR_HIP, "%s failed: %s", \
                        #call, hipGetErrorString(e_));                                        \
    } while (0)

// the same for a step of the function `who`, whose name opens the message
#define TQ_HIPF(ctx, who, call)                                                               \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(ctx, e_ == hipErrorOutOfMemory ? TQ_ERR_OOM : TQ_ERR_HIP, "%s: %s", who, hipGetErrorString(e_)); \
    } while (0)

// behind a kernel launch, or a group of launches, of the function `who`
#define TQ_LAUNCHED(ctx, who)                                                                 \
    do {                                                                                      \
        hipError_t e_ = hipGetLastError();                                                    \
        if (e_ != hipSuccess) return fail(ctx, TQ_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e_)); \
    } while (0)

// The guard of the C boundary: `body` runs with the context's device selected (`ctx` is NULL for the host back ends and
// the context-free calls) and no exception leaves it.  std::bad_alloc and std::length_error (a size past max_size(): the
// request was for more memory than there is) give TQ_ERR_OOM, any other std::exception TQ_ERR_INVALID_ARG; the message
// opens with `name`.  Every entry point that can allocate host memory or that touches the device goes through it, so
// neither it nor a helper below it selects the device or catches for itself.
template <class Body>
int api(tq_ctx *ctx, const char *name, Body &&body)
{
    try {
        if (ctx) TQ_HIP(ctx, hipSetDevice(ctx->device));
        return body();
    } catch (const std::bad_alloc &) {
        return fail(ctx, TQ_ERR_OOM, "%s: out of host memory", name);
    } catch (const std::length_error &e) {
        return fail(ctx, TQ_ERR_OOM, "%s: %s", name, e.what());
    } catch (const std::exception &e) {
        return fail(ctx, TQ_ERR_INVALID_ARG, "%s: %s", name, e.what());
    }
}

// the message for what StagingRing::ensure refused: `no_memory` where the pool had no piece, else the event's error
int ring_fail(tq_ctx *ctx, int rc, const char *no_memory)
{
    if (rc == TQ_ERR_OOM) return fail(ctx, rc, "%s", no_memory);
    return fail(ctx, rc, "hipEventCreateWithFlags failed: %s", hipGetErrorString(hipGetLastError()));
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// C(T, 4), the number of quartets of T taxa and the size of the rank space: exact for every T at which it is below 2^64,
// which rank_space_fits says (T <= 145 056; format.hpp's host_choose4 takes the last product in 128 bits).  Every call
// that takes or makes ranks asks rank_space_fits first and refuses with RANK_SPACE_MSG.
uint64_t choose4(uint64_t T) { return host_choose4(T); }
bool rank_space_fits(int64_t T) { return T >= 0 && (uint64_t)T <= CHOOSE4_MAX_T; }
#define RANK_SPACE_MSG "%s: C(%lld,4) does not fit 64 bits: quartet ranks are defined for at most 145056 taxa"

// whether the Q ranks from first_rank all lie below total, without forming first_rank + Q (which wraps near 2^64)
bool rank_range_fits(uint64_t first_rank, int64_t Q, uint64_t total)
{
    return Q <= 0 || (first_rank <= total && (uint64_t)Q <= total - first_rank);
}

// The cooperative kernels address a set with 32-bit offsets: a packed set past that range while the natural one is inside
// it would send the batch to the one-wave kernel, so such a set is not built automatically.
bool pack_fits_offsets(int64_t T, size_t packedSp, size_t naturalSp)
{
    return (uint64_t)T * (uint64_t)packedSp < SCAN_OFFSET_LIMIT || (uint64_t)T * (uint64_t)naturalSp >= SCAN_OFFSET_LIMIT;
}

// Contiguous copy of a strided locus column and the check subsample mode and the packed order rely on: no id 0xFFFFFFFF
// and every id in one contiguous run of sites (a sorted column needs no set).  `loc` is filled either way.
bool copy_locus_column(const uint32_t *locus, int64_t stride, int64_t S, std::vector<uint32_t> &loc)
{
    bool ok = true, sorted = true;
    loc.resize((size_t)S);
    for (int64_t i = 0; i < S; ++i) {
        loc[(size_t)i] = locus[i * stride];
        if (loc[(size_t)i] == 0xFFFFFFFFu) ok = false;
        if (i && loc[(size_t)i] < loc[(size_t)i - 1]) sorted = false;
    }
    if (ok && !sorted) {
        std::unordered_set<uint32_t> seen;
        seen.insert(loc[0]);
        for (int64_t i = 1; i < S && ok; ++i)
            if (loc[(size_t)i] != loc[(size_t)i - 1] && !seen.insert(loc[(size_t)i]).second) ok = false;
    }
    return ok;
}

void free_data(tq_ctx *ctx)
{
    ctx->nat.reset();
    ctx->pk.reset();
    ctx->pk_gen = ~0ull;
    ctx->pk_from_boot = false;
    ctx->have_data = false;
    ctx->scanned_Q = 0;
}

void free_source(tq_ctx *ctx)
{
    ctx->d_seqarr.reset();
    ctx->d_spans.reset();
    ctx->d_lidxs.reset();
    ctx->d_boot.reset();
    ctx->d_boot_tmp.reset();
    ctx->d_pstart.reset();
    ctx->d_pk_src.reset();
    ctx->pk_from_boot = false;
    ctx->boot_pack_auto = false;
    ctx->boot_cap = 0;
    ctx->nloci = 0;
    ctx->lidx_ring.reset();
}

// Before shared scratch is regrown: the host waits for the last *_dev call, whose kernels may still read the old block
// on any stream (device_mem.hpp: "a caller that regrows a buffer the device may still read waits for the device first").
// The host-buffer calls have drained their own streams when they return.  Only on the regrow path: no HIP call otherwise
// (tq_set_data frees its replicate on every call, so it waits on every call).
hipError_t regrow_wait(tq_ctx *ctx)
{
    return ctx->evDevApi ? hipEventSynchronize(ctx->evDevApi) : hipSuccess;
}

// the scratch of the host-buffer calls and of a range call without a quartet array, grow-only
hipError_t grow_scratch(tq_ctx *ctx, size_t bytes)
{
    if (bytes <= ctx->d_scratch.cap()) return hipSuccess;
    const hipError_t e = regrow_wait(ctx);
    return e != hipSuccess ? e : ctx->d_scratch.grow(bytes);
}

// count slab + ordering scratch for a scan batch of `quartets`
int ensure_cm(tq_ctx *ctx, int64_t quartets)
{
    if (quartets <= ctx->cm_quartets) return TQ_OK;
    TQ_HIP(ctx, regrow_wait(ctx));
    ctx->d_cm.reset();
    ctx->d_sort.reset();
    ctx->d_sort_tmp.reset();
    ctx->d_units.reset();
    ctx->cm_quartets = 0;
    ctx->scanned_Q = 0;
    TQ_HIP(ctx, ctx->d_cm.alloc((size_t)quartets * 256));
    TQ_HIP(ctx, ctx->d_sort.alloc((size_t)quartets * 4));
    size_t tmp = 0;
    uint32_t *k = ctx->d_sort;
    TQ_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, k, k, k, k, (int)quartets));
    size_t tmp2 = 0;
    TQ_HIP(ctx, hipcub::DeviceScan::InclusiveSum(nullptr, tmp2, k, k, (int)quartets));
    if (tmp2 > tmp) tmp = tmp2;
    TQ_HIP(ctx, ctx->d_sort_tmp.alloc(tmp ? tmp : 16));
    TQ_HIP(ctx, ctx->d_units.alloc((size_t)quartets + 2));
    ctx->sort_tmp_bytes = tmp;
    ctx->cm_quartets = quartets;
    return TQ_OK;
}

// scratch of the singular-value stage: two sets (one per stream) for chunks of `quartets`
int ensure_svd(tq_ctx *ctx, int64_t quartets)
{
    if (!ctx->sX) {
        TQ_HIP(ctx, ctx->sX.create());
        TQ_HIP(ctx, ctx->evFork.create());
        TQ_HIP(ctx, ctx->evJoin.create());
    }
    if (quartets <= ctx->svd_quartets) return TQ_OK;
    TQ_HIP(ctx, regrow_wait(ctx));
    ctx->d_de.reset();
    ctx->d_sv.reset();
    ctx->d_nsnps.reset();
    ctx->svd_quartets = 0;
    TQ_HIP(ctx, ctx->d_de.alloc(2 * (size_t)quartets * 3 * 32));
    TQ_HIP(ctx, ctx->d_sv.alloc(2 * (size_t)quartets * 3 * 16));
    TQ_HIP(ctx, ctx->d_nsnps.alloc(2 * (size_t)quartets));
    ctx->svd_quartets = quartets;
    return TQ_OK;
}

// ---- timing marks -------------------------------------------------------------------------------
int mark(tq_ctx *ctx, int tag, hipStream_t stream, int lane = 0)
{
    if (!ctx->timing) return TQ_OK;
    Event ev;                       // a push_back that throws (into the guard) destroys it
    if (!ctx->event_pool.empty()) {
        ev = std::move(ctx->event_pool.back());
        ctx->event_pool.pop_back();
    } else {
        TQ_HIP(ctx, ev.create(true));
    }
    ctx->marks.push_back({tag, lane, std::move(ev)});
    TQ_HIP(ctx, hipEventRecord(ctx->marks.back().ev, stream));
    return TQ_OK;
}

// order[] for one batch: indices sorted by (first, second[, third]) taxon; nullptr = natural order
int make_order(tq_ctx *ctx, const uint32_t *dq, int64_t n, bool input_sorted, hipStream_t stream,
               const uint32_t **order)
{
    *order = nullptr;
    // below ~32k quartets the sort's twenty small launches cost more than the shared rows save
    // (tools/small_call_order.py: 8 000 quartets 0.34 ms sorted, 0.31 ms in natural order; 62 500: 1.1 vs 2.4 ms)
    if (!ctx->opt.order || n < 32768 || ctx->T > 65535 || input_sorted) return TQ_OK;
    uint32_t *keys_in = ctx->d_sort, *idx_in = keys_in + ctx->cm_quartets;
    uint32_t *keys_out = idx_in + ctx->cm_quartets, *idx_out = keys_out + ctx->cm_quartets;
    const uint64_t T = (uint64_t)ctx->T;
    const int with_c = T * T * T <= 0xFFFFFFFFull;
    hipLaunchKernelGGL(tq_key_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dq, n,
                       (uint32_t)ctx->T, with_c, keys_in, idx_in);
    TQ_LAUNCHED(ctx, __func__);
    int bits = 1;
    while (bits < 32 && (1ull << bits) < (with_c ? T * T * T : T * T)) ++bits;
    size_t tmp = ctx->sort_tmp_bytes;
    TQ_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(ctx->d_sort_tmp, tmp, keys_in, keys_out, idx_in, idx_out, (int)n,
                                                   0, bits, stream));
    *order = idx_out;
    return TQ_OK;
}

// ordering + unit list of the joint-histogram scan: d_units[0..count) = (first quartet, second quartet or DP_NONE) in
// (a,b,c)-sorted order, count in d_units[cm_quartets] (read by the kernel: nothing comes back to the host)
int make_units(tq_ctx *ctx, const uint32_t *dq, int64_t n, bool input_sorted, hipStream_t stream)
{
    uint32_t *keys_in = ctx->d_sort, *idx_in = keys_in + ctx->cm_quartets;
    uint32_t *keys_out = idx_in + ctx->cm_quartets, *idx_out = keys_out + ctx->cm_quartets;
    const uint64_t T = (uint64_t)ctx->T;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(tq_key_kernel, dim3(blocks), dim3(256), 0, stream, dq, n, (uint32_t)ctx->T, 1, keys_in, idx_in);
    TQ_LAUNCHED(ctx, __func__);
    const uint32_t *keys = keys_in, *idx = idx_in;
    uint32_t *flags = keys_out;
    if (!input_sorted) {
        int bits = 1;
        while (bits < 32 && (1ull << bits) < T * T * T) ++bits;
        size_t tmp = ctx->sort_tmp_bytes;
        TQ_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(ctx->d_sort_tmp, tmp, keys_in, keys_out, idx_in, idx_out, (int)n,
                                                       0, bits, stream));
        keys = keys_out;
        idx = idx_out;
        flags = keys_in;
    }
    hipLaunchKernelGGL(tq_dp_flag_kernel, dim3(blocks), dim3(256), 0, stream, keys, idx, dq, n, (uint32_t)ctx->T, flags);
    TQ_LAUNCHED(ctx, __func__);
    size_t tmp = ctx->sort_tmp_bytes;
    TQ_HIP(ctx, hipcub::DeviceScan::InclusiveSum(ctx->d_sort_tmp, tmp, flags, flags, (int)n, stream));
    hipLaunchKernelGGL(tq_dp_units_kernel, dim3(blocks), dim3(256), 0, stream, keys, idx, (const uint32_t *)flags, n,
                       ctx->d_units, reinterpret_cast<uint32_t *>(ctx->d_units + ctx->cm_quartets));
    TQ_LAUNCHED(ctx, __func__);
    return TQ_OK;
}

DevData dev_data(const tq_ctx *ctx)
{
    DevData d;
    ctx->nat.fill(d, ctx->T);
    d.T = (int32_t)ctx->T;
    d.inv = ctx->opt.count_invariant ? 0xFFFFFFFFu : 0u;
    return d;
}

// the set a scan reads: in subsample mode the packed one while it is current (same counts, fewer walk trips per step);
// its nib5 is NULL: full-mode kernels only (scan_dp.hpp, species.hpp)
DevData scan_data(const tq_ctx *ctx, int subsample)
{
    DevData d = dev_data(ctx);
    if (subsample && ctx->opt.site_pack && ctx->pk.rows && ctx->pk_gen == ctx->data_gen) ctx->pk.fill(d, ctx->T);
    return d;
}

static_assert(SCAN_WAVE == WAVE && SCAN_TILE == TILE && SCAN_PB_NW == PB_NW && SCAN_PB_MAX_TILES == PB_MAX_TILES &&
              SCAN_DP_NW == DP_NW, "scan_plan.hpp and the kernel headers disagree");

// the options choose_scan reads
ScanKnobs scan_knobs(const tq_ctx *ctx)
{
    const Options &o = ctx->opt;
    return {o.scan_pair, o.scan_wg, o.scan_method, o.scan_f4, o.scan_dp, o.park_t, o.share_c, o.count_invariant, o.waves_per_cu,
            o.nrep, o.order, o.wg_min_quartets, o.dp_min_quartets, ctx->pb_ok, o.xcd_remap, ctx->prop.multiProcessorCount};
}

// remembers which kernel form takes the batch and the layout set it reads (a test hook; decides nothing)
void note_scan(tq_ctx *ctx, int form, const DevData &d)
{
    ctx->last_scan_form = form;
    ctx->last_scan_tpitch = ctx->T * d.pitch;
    ctx->last_scan_packed = ctx->pk.rows && d.rows == ctx->pk.rows ? 1 : 0;
}

template <typename K>
int grid_for(tq_ctx *ctx, K kern, int64_t items, int64_t *grid, int wpc_kernel = 0)
{
    int wpc = wpc_kernel > 0 ? wpc_kernel : ctx->opt.waves_per_cu;
    if (wpc <= 0) {
        int nb = 0;
        TQ_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, WAVE, 0));
        wpc = nb > 0 ? nb : 8;
    }
    int64_t g = (int64_t)ctx->prop.multiProcessorCount * wpc;
    if (g > items) g = items;
    if (g < 1) g = 1;
    *grid = g;
    return TQ_OK;
}

// ---- the scan launch: choose_scan (scan_plan.hpp) names an instantiation, this table holds every one that is built --------
using ScanWaveFn = void (*)(DevData, const uint32_t *, const uint32_t *, int64_t, uint32_t *);
using ScanWgFn = void (*)(DevData, const uint32_t *, const uint32_t *, int64_t, uint32_t *, int64_t);            // WG, WG2, F4
using ScanPbFn = void (*)(DevData, const uint32_t *, const uint32_t *, int64_t, uint32_t *, int64_t, uint32_t *);
using ScanDpFn = void (*)(DevData, const uint32_t *, const uint2 *, const uint32_t *, uint32_t *);

struct ScanKernel {
    int form, sub, method, nw, shc, park, nrep;    // as in ScanPlan
    ScanWaveFn wave;                               // exactly one of the four is set: the form's signature
    ScanWgFn wg;
    ScanPbFn pb;
    ScanDpFn dp;
};

template <int NREP>
void add_wave_rows(std::vector<ScanKernel> &t)
{
    t.push_back({SCAN_FORM_ONE_WAVE, 0, 0, 1, 0, 0, NREP, tq_scan_kernel<NREP, false, 0>});
    t.push_back({SCAN_FORM_ONE_WAVE, 0, 1, 1, 0, 0, NREP, tq_scan_kernel<NREP, false, 1>});
    t.push_back({SCAN_FORM_ONE_WAVE, 1, 0, 1, 0, 0, NREP, tq_scan_kernel<NREP, true, 0>});
    t.push_back({SCAN_FORM_ONE_WAVE, 1, 1, 1, 0, 0, NREP, tq_scan_kernel<NREP, true, 1>});
}

template <bool SUB, int METHOD, int NW, bool SHC = false, bool PARK_T = false>
ScanKernel wg_row()
{
    return {SCAN_FORM_WG, SUB, METHOD, NW, SHC, PARK_T, 0, nullptr, tq_scan_wg_kernel<SUB, METHOD, NW, SHC, PARK_T>};
}

template <int NW>
void add_wg_rows(std::vector<ScanKernel> &t)       // what every width has: methods 0 and 1 per mode, diagnostics 2 and 3
{
    t.push_back(wg_row<false, 0, NW>());
    t.push_back(wg_row<false, 1, NW>());
    t.push_back(wg_row<true, 0, NW>());
    t.push_back(wg_row<true, 1, NW>());
    t.push_back(wg_row<true, 2, NW>());
    t.push_back(wg_row<true, 3, NW>());
}

template <bool SUB, int NW>
ScanKernel f4_row() { return {SCAN_FORM_F4, SUB, 0, NW, 0, 0, 0, nullptr, tq_scan_f4_kernel<SUB, NW>}; }

template <bool SUB, int METHOD>
ScanKernel wg2_row() { return {SCAN_FORM_WG2, SUB, METHOD, 4, 0, 0, 0, nullptr, tq_scan_wg2_kernel<SUB, METHOD, 4>}; }

std::vector<ScanKernel> build_scan_table()
{
    std::vector<ScanKernel> t;
    add_wave_rows<1>(t), add_wave_rows<2>(t), add_wave_rows<4>(t), add_wave_rows<8>(t), add_wave_rows<16>(t), add_wave_rows<32>(t);
    add_wg_rows<2>(t), add_wg_rows<3>(t), add_wg_rows<4>(t), add_wg_rows<6>(t), add_wg_rows<8>(t), add_wg_rows<16>(t);
    t.push_back(wg_row<true, 4, 4>());
    t.push_back(wg_row<true, 5, 4>());
    t.push_back(wg_row<false, 1, 4, false, true>());                        // PARK_T
    t.push_back(wg_row<true, 1, 4, false, true>());
    t.push_back(wg_row<true, 1, 6, false, true>());
    t.push_back(wg_row<true, 1, 8, false, true>());
    t.push_back(wg_row<false, 0, 4, true>());                               // SHC
    t.push_back(wg_row<false, 1, 4, true>());
    t.push_back(wg_row<true, 0, 4, true>());
    t.push_back(wg_row<true, 1, 4, true>());
    t.push_back(wg2_row<false, 0>());
    t.push_back(wg2_row<false, 1>());
    t.push_back(wg2_row<true, 0>());
    t.push_back(wg2_row<true, 1>());
    t.push_back(f4_row<false, 2>());
    t.push_back(f4_row<true, 2>());
    t.push_back(f4_row<false, 4>());
    t.push_back(f4_row<true, 4>());
    t.push_back(f4_row<false, 8>());
    t.push_back(f4_row<true, 8>());
    t.push_back({SCAN_FORM_PB, 0, 0, PB_NW, 0, 0, 0, nullptr, nullptr, tq_scan_pb_kernel<false>});
    t.push_back({SCAN_FORM_PB, 1, 0, PB_NW, 0, 0, 0, nullptr, nullptr, tq_scan_pb_kernel<true>});
    t.push_back({SCAN_FORM_DP, 0, 0, DP_NW, 0, 0, 0, nullptr, nullptr, nullptr, tq_scan_dp_kernel<DP_NW>});
    return t;
}

const std::vector<ScanKernel> SCAN_TABLE = build_scan_table();

// the table row of a plan, or nullptr: the plan names an instantiation that is not built
const ScanKernel *find_scan_kernel(const ScanPlan &p)
{
    for (const ScanKernel &k : SCAN_TABLE)
        if (k.form == p.form && k.sub == p.sub && k.method == p.method && k.nw == p.nw && k.shc == p.shc && k.park == p.park &&
            k.nrep == p.nrep)
            return &k;
    return nullptr;
}

// launches the plan of any form but DP (launch_scan_dp: another argument list)
int launch_scan(tq_ctx *ctx, const ScanPlan &p, const DevData &d, const uint32_t *dq, const uint32_t *order, int64_t Q,
                hipStream_t stream)
{
    const ScanKernel *k = find_scan_kernel(p);
    if (!k || k->dp)
        return fail(ctx, TQ_ERR_INVALID_ARG, "no scan kernel is built for form %d sub %d method %d nw %d shc %d park %d nrep %d",
                    p.form, p.sub, p.method, p.nw, p.shc, p.park, p.nrep);
    if (k->wave) {
        int64_t grid;
        int rc = grid_for(ctx, k->wave, Q, &grid);
        if (rc) return rc;
        hipLaunchKernelGGL(k->wave, dim3((unsigned)grid), dim3(p.threads), 0, stream, d, dq, order, Q, ctx->d_cm);
    } else if (k->pb) {
        hipLaunchKernelGGL(k->pb, dim3((unsigned)p.grid), dim3(p.threads), 0, stream, d, dq, order, Q, ctx->d_cm, p.xcd_chunk,
                           (uint32_t *)nullptr);
    } else {
        hipLaunchKernelGGL(k->wg, dim3((unsigned)p.grid), dim3(p.threads), 0, stream, d, dq, order, Q, ctx->d_cm, p.xcd_chunk);
    }
    TQ_LAUNCHED(ctx, __func__);
    return TQ_OK;
}

// One-time check (tq_create) that the kernel's counters start on a 64 KiB LDS boundary, which its address arithmetic
// relies on: a launch with Q < 0 reports the offset and does nothing else.
int probe_scan_pb(tq_ctx *ctx)
{
    DevBuf<uint32_t> d;
    uint32_t h[2] = {0, 0};
    const char *who = "probe of tq_scan_pb_kernel";
    TQ_HIP(ctx, d.alloc(2));
    TQ_HIPF(ctx, who, hipMemset(d, 0, sizeof h));
    DevData none{};
    hipLaunchKernelGGL(tq_scan_pb_kernel<false>, dim3(1), dim3(PB_NW * WAVE), 0, 0, none, (const uint32_t *)nullptr,
                       (const uint32_t *)nullptr, (int64_t)-1, (uint32_t *)nullptr, (int64_t)0, d.get());
    hipLaunchKernelGGL(tq_scan_pb_kernel<true>, dim3(1), dim3(PB_NW * WAVE), 0, 0, none, (const uint32_t *)nullptr,
                       (const uint32_t *)nullptr, (int64_t)-1, (uint32_t *)nullptr, (int64_t)0, d + 1);
    TQ_LAUNCHED(ctx, who);
    TQ_HIPF(ctx, who, hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost));
    ctx->pb_ok = (h[0] == 0x80000000u && h[1] == 0x80000000u) ? 1 : -1;
    return TQ_OK;
}

// joint-histogram scan over the unit list make_units left (grid: scan_dp_grid)
int launch_scan_dp(tq_ctx *ctx, const uint32_t *dq, int64_t Q, hipStream_t stream)
{
    const DevData d = dev_data(ctx);
    hipLaunchKernelGGL(tq_scan_dp_kernel<DP_NW>, dim3((unsigned)scan_dp_grid(Q)), dim3(DP_NW * WAVE), 0, stream, d, dq,
                       (const uint2 *)ctx->d_units, reinterpret_cast<const uint32_t *>(ctx->d_units + ctx->cm_quartets),
                       ctx->d_cm);
    TQ_LAUNCHED(ctx, __func__);
    return TQ_OK;
}

// Jacobi path: count slab rows [cm, cm + n) -> outputs of the same rows
template <bool DEBUG>
int launch_svd(tq_ctx *ctx, const uint32_t *cm, const uint32_t *dq, int64_t n, const OutPtrs &out, hipStream_t stream,
               int lane)
{
    auto kern = tq_svd_kernel<DEBUG>;
    int64_t grid;
    int rc = grid_for(ctx, kern, (n + QPW - 1) / QPW, &grid);
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(WAVE), 0, stream, cm, dq, n, (int32_t)ctx->scanned_T, out);
    TQ_LAUNCHED(ctx, __func__);
    return mark(ctx, TAG_BIDIAG, stream, lane);
}

// Householder + QR path, one chunk (n <= svd scratch)
template <bool DEBUG>
int launch_hqr(tq_ctx *ctx, const uint32_t *cm, const uint32_t *dq, int64_t n, const OutPtrs &out, hipStream_t stream,
               int lane)
{
    // scratch set of this stream
    double *de = ctx->d_de + (size_t)lane * (size_t)ctx->svd_quartets * 96;
    double *sv = ctx->d_sv + (size_t)lane * (size_t)ctx->svd_quartets * 48;
    uint32_t *nsnps = ctx->d_nsnps + (size_t)lane * (size_t)ctx->svd_quartets;
    int64_t grid;
    auto k1 = ctx->opt.bidiag_layout ? tq_bidiag2_kernel<DEBUG> : tq_bidiag_kernel<DEBUG>;
    // one pass per block unless told otherwise: the work per pass varies (QR iterations), and the
    // hardware dispatcher balances it better than a static grid-stride loop (3.8 ms vs 5.1 ms per 1e6)
    const int svd_wpc = ctx->opt.svd_wpc > 0 ? ctx->opt.svd_wpc : (1 << 20);
    const int tsplit = n < 32768 ? 1 : 0;          // small batches: one block per (pass, flattening), tq_bidiag_kernel
    int rc = grid_for(ctx, k1, (tsplit ? 3 : 1) * ((n + 15) / 16), &grid, svd_wpc);
    if (rc) return rc;
    hipLaunchKernelGGL(k1, dim3((unsigned)grid), dim3(WAVE), 0, stream, cm, n, de, nsnps, out.cmats, tsplit);
    TQ_LAUNCHED(ctx, __func__);
    if ((rc = mark(ctx, TAG_BIDIAG, stream, lane))) return rc;
    const int64_t nmat = 3 * n;
    rc = grid_for(ctx, tq_bdsqr_kernel, (nmat + WAVE - 1) / WAVE, &grid, svd_wpc);
    if (rc) return rc;
    hipLaunchKernelGGL(tq_bdsqr_kernel, dim3((unsigned)grid), dim3(WAVE), 0, stream, (const double *)de, nmat, sv,
                       ctx->opt.bdsqr_maxit, (unsigned long long *)ctx->d_bdsqr_stats.get());
    TQ_LAUNCHED(ctx, __func__);
    if ((rc = mark(ctx, TAG_BDSQR, stream, lane))) return rc;
    hipLaunchKernelGGL(tq_score_kernel<DEBUG>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       (const double *)sv, (const uint32_t *)nsnps, dq, n, (int32_t)ctx->scanned_T, out);
    TQ_LAUNCHED(ctx, __func__);
    return mark(ctx, TAG_SCORE, stream, lane);
}

bool diagnostic_mode(const tq_ctx *ctx)
{
    return (ctx->opt.scan_method >= 2 && ctx->opt.scan_method <= 5) || ctx->opt.phases != 3;
}

// timing-diagnostic modes produce wrong rows: none leaves the library unmarked.  `flags` is the array the CALLER gave: a
// host-buffer call judges it at its entry, since the device array it hands `launch` is the library's own and never NULL.
int refuse_unflagged(tq_ctx *ctx, const uint8_t *flags)
{
    if (diagnostic_mode(ctx) && !flags)
        return fail(ctx, TQ_ERR_INVALID_ARG, "a timing-diagnostic mode is set (scan_method 2..5 or phases 1 / 2): its rows are "
                                             "not results and are only handed out with a flags array (TQ_FLAG_INVALID_DIAGNOSTIC)");
    return TQ_OK;
}

OutPtrs offset_out(const OutPtrs &o, int64_t q0)
{
    OutPtrs r = o;
    r.rstat = o.rstat + q0 * 2;
    r.rscor = o.rscor + q0 * 3;
    r.flags = o.flags ? o.flags + q0 : nullptr;
    r.cmats = o.cmats ? o.cmats + q0 * 768 : nullptr;
    r.svds = o.svds ? o.svds + q0 * 48 : nullptr;
    r.ranks = o.ranks ? o.ranks + q0 * 3 : nullptr;
    return r;
}

int check_ready(tq_ctx *ctx, int subsample)
{
    if (!ctx->have_data) return fail(ctx, TQ_ERR_NO_DATA, "tq_set_data has not been called");
    if (subsample && !ctx->locus_runs_ok)
        return fail(ctx, TQ_ERR_LOCUS_ORDER,
                    "subsample mode needs each locus id in one contiguous run of sites (and no id 0xFFFFFFFF)");
    return TQ_OK;
}

// Stage 1 of a pass: ordering + site scan of quartets dq[0..n) into the count slab (n <= ctx->opt.batch).
int stage_scan(tq_ctx *ctx, const uint32_t *dq, int64_t n, int subsample, bool input_sorted, hipStream_t stream)
{
    int rc = ensure_cm(ctx, n);
    if (rc) return rc;
    ctx->scanned_Q = 0;
    if ((rc = mark(ctx, TAG_ORIGIN, stream))) return rc;
    if (ctx->opt.phases & 1) {
        const DevData d = scan_data(ctx, subsample);
        const ScanPlan plan = choose_scan(scan_knobs(ctx), {ctx->T, d.pitch, ctx->nat.Sp, n, subsample, input_sorted});
        const uint32_t *order = nullptr;
        rc = plan.form == SCAN_FORM_DP ? make_units(ctx, dq, n, input_sorted, stream)
                                       : make_order(ctx, dq, n, input_sorted, stream, &order);
        if (rc) return rc;
        if ((rc = mark(ctx, TAG_ORDER, stream))) return rc;
        note_scan(ctx, plan.form, d);
        rc = plan.form == SCAN_FORM_DP ? launch_scan_dp(ctx, dq, n, stream) : launch_scan(ctx, plan, d, dq, order, n, stream);
        if (rc) return rc;
        if ((rc = mark(ctx, TAG_SCAN, stream))) return rc;
    }
    ctx->scanned_q = dq;
    ctx->scanned_Q = n;
    ctx->scanned_T = ctx->T;
    return TQ_OK;
}

// lineages per sample of the species map: 2 in allele mode (one per allele of a diploid genotype)
inline int species_lineages(const tq_ctx *ctx) { return ctx->opt.species_alleles ? 2 : 1; }

// Species mode: the map is set, matches the resident replicate and the pooled counts fit u32
// (allele mode: sizes in lineages = 2 x samples, and the resident data must be a device-built replicate of the current
// source -- the option can be set after the map, so everything is checked here, at call time)
int species_ready(tq_ctx *ctx, const char *who)
{
    if (ctx->opt.species_alleles) {
        if (!ctx->d_seqarr)
            return fail(ctx, TQ_ERR_NO_DATA, "%s: species_alleles needs the IUPAC source (call tq_set_source, then tq_bootstrap)", who);
        if (!ctx->have_data || ctx->boot_gen != ctx->data_gen || ctx->boot_src_gen != ctx->src_gen)
            return fail(ctx, TQ_ERR_NO_DATA, "%s: species_alleles needs the resident data to be a replicate built by "
                        "tq_bootstrap from the current source (tq_set_data and a new tq_set_source do not give one)", who);
    }
    if (!ctx->have_data) return fail(ctx, TQ_ERR_NO_DATA, "%s: tq_set_data has not been called", who);
    if (!ctx->sp_K) return fail(ctx, TQ_ERR_NO_DATA, "%s: no species map (call tq_set_species first)", who);
    if (ctx->sp_T != ctx->T)
        return fail(ctx, TQ_ERR_INVALID_ARG, "%s: the species map covers T=%lld samples, the resident replicate has T=%lld",
                    who, (long long)ctx->sp_T, (long long)ctx->T);
    const int lin = species_lineages(ctx);
    if (lin == 2 && ctx->sp_max > 127)
        return fail(ctx, TQ_ERR_INVALID_ARG, "%s: species_alleles takes species of at most 127 samples (254 lineages, one "
                    "byte per base), the map has one of %d", who, (int)ctx->sp_max);
    const uint64_t bound = ctx->sp_bound * (uint64_t)(lin * lin * lin * lin);      // <= 255^4 x 16 < 2^36
    if ((unsigned __int128)ctx->S * bound >= ((unsigned __int128)1 << 32))
        return fail(ctx, TQ_ERR_INVALID_ARG,
                    "%s: pooled counts may exceed u32: S=%lld x product of the four largest species sizes %llu >= 2^32%s",
                    who, (long long)ctx->S, (unsigned long long)bound, lin == 2 ? " (sizes in lineages: 2 per sample)" : "");
    if (ctx->opt.species_method == 1 && lin * ctx->sp_max > SPECIES_MFMA_MAX)
        return fail(ctx, TQ_ERR_INVALID_ARG, "%s: species_method 1 (MFMA, i8 operands) takes species of at most %d lineages, "
                    "the map has one of %d%s", who, SPECIES_MFMA_MAX, lin * (int)ctx->sp_max,
                    lin == 2 ? " (species_alleles: 2 per sample, i.e. at most 5 samples)" : "");
    return TQ_OK;
}

// The species table of the resident replicate, both layouts: rebuilt on `stream` when the resident data (or the lineage
// mode) changed since it was built, from the nibble rows or, in allele mode, from the IUPAC source.  The caller has
// passed species_ready.  Touches nothing but the table: no slab, no timing mark.
int ensure_species_table(tq_ctx *ctx, hipStream_t stream)
{
    if (ctx->sp_tab_gen != ctx->data_gen) {
        const int64_t Sp = ctx->nat.Sp, entries = ctx->sp_K * Sp;
        if ((size_t)entries * 2 > ctx->d_sp_tab.cap()) {
            if (ctx->d_sp_tab) TQ_HIP(ctx, hipDeviceSynchronize());      // a species call on another stream may still read it
            TQ_HIP(ctx, ctx->d_sp_tab.grow((size_t)entries * 2));
        }
        const int32_t *members = ctx->d_sp_members + ctx->sp_K + 1;
        if (ctx->opt.species_alleles)       // species_ready: d_boot holds the site map of the resident replicate
            hipLaunchKernelGGL(tq_species_allele_table_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, stream,
                               (const uint8_t *)ctx->d_seqarr, ctx->src_S0,
                               (const uint32_t *)(ctx->d_boot + 2 * (ctx->nloci + 1)), ctx->S, Sp, members,
                               (const int32_t *)ctx->d_sp_members, (int32_t)ctx->sp_K, ctx->d_sp_tab,
                               (uint8_t *)(ctx->d_sp_tab + entries));
        else
            hipLaunchKernelGGL(tq_species_table_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, stream,
                               (const uint8_t *)ctx->nat.nib5, Sp, ctx->S, members, (const int32_t *)ctx->d_sp_members,
                               (int32_t)ctx->sp_K, ctx->d_sp_tab, (uint8_t *)(ctx->d_sp_tab + entries));
        TQ_LAUNCHED(ctx, __func__);
        ctx->sp_tab_gen = ctx->data_gen;
    }
    return TQ_OK;
}

// the offsets the species kernels read for the per-row range rule: in allele mode the copy whose differences are 2n
inline const int32_t *species_lineage_offsets(const tq_ctx *ctx)
{
    return species_lineages(ctx) == 2 ? ctx->d_sp_members + ctx->sp_K + 1 + ctx->sp_T : ctx->d_sp_members;
}

// Stage 1 of a species pass: (re)build the species table if the resident data changed, then the pooled counts of
// species quartets dsq[0..n) into the count slab, where stage_svd finds them as it finds a scanned batch.
int stage_species(tq_ctx *ctx, const uint32_t *dsq, int64_t n, hipStream_t stream)
{
    int rc = ensure_cm(ctx, n);
    if (rc) return rc;
    ctx->scanned_Q = 0;
    if ((rc = mark(ctx, TAG_ORIGIN, stream))) return rc;
    if ((rc = ensure_species_table(ctx, stream))) return rc;
    if ((rc = mark(ctx, TAG_ORDER, stream))) return rc;
    const int lin = species_lineages(ctx);
    const bool mfma = ctx->opt.species_method == 1 || (ctx->opt.species_method < 0 && lin * ctx->sp_max <= SPECIES_MFMA_MAX);
    const int32_t *offsets = species_lineage_offsets(ctx);      // read for the per-row range rule only
    if (mfma)
        hipLaunchKernelGGL(tq_species_mfma_kernel, dim3((unsigned)n), dim3(WAVE * SPECIES_WAVES), 0, stream,
                           (const uint8_t *)(ctx->d_sp_tab + ctx->sp_K * ctx->nat.Sp), ctx->nat.Sp, ctx->S, dsq, n,
                           (int32_t)ctx->sp_K, offsets, ctx->d_cm);
    else
        hipLaunchKernelGGL(tq_species_pool_kernel, dim3((unsigned)n), dim3(WAVE * SPECIES_WAVES), 0, stream,
                           (const uint32_t *)ctx->d_sp_tab, ctx->nat.Sp, ctx->S, dsq, n, (int32_t)ctx->sp_K, offsets, ctx->d_cm);
    TQ_LAUNCHED(ctx, __func__);
    if ((rc = mark(ctx, TAG_SCAN, stream))) return rc;
    ctx->scanned_q = dsq;
    ctx->scanned_Q = n;
    ctx->scanned_T = ctx->sp_K;
    return TQ_OK;
}

// Rows per chunk of the singular-value stage for a range of n rows (the ONE place that decides it: stage_svd
// cuts by it and HostSink sizes its staging and picks its single-piece path by it).
int64_t svd_chunk_rows(const tq_ctx *ctx, int64_t n)
{
    int64_t chunk = ctx->opt.svd_chunk < n ? ctx->opt.svd_chunk : n;
    // a mid-size batch that would be one chunk is cut in two halves, one per stream: their tails fill each other
    // (125k quartets 1.58 -> 1.53 ms, 300k 3.45 -> 3.35 ms) and the host API gets a result piece to copy early
    if (ctx->opt.svd_streams > 1 && n >= 65536 && n < 2 * ctx->opt.svd_chunk && chunk > (n + 1) / 2) chunk = (n + 1) / 2;
    return chunk < 1 ? 1 : chunk;
}

// Stage 2 of a pass: singular values, ranks, scores and topology of rows [q0, q0+n) of the scanned
// batch, in chunks of svd_chunk quartets.  `out` points at the outputs of row q0.  Chunks alternate
// between the caller's stream and a second one (each with its own scratch set), so that the tail of one
// chunk's kernels -- a wave per 64 matrices with data-dependent iteration counts -- is filled by the next
// chunk's.  After each chunk `after_chunk(c0, cn, chunk_stream)` is called (c0 relative to q0) with the
// chunk's kernels enqueued on chunk_stream: the host-buffer API starts that chunk's result D2H there.
// On return the caller's stream has been made to wait for everything enqueued on the second stream.
template <typename F>
int stage_svd(tq_ctx *ctx, int64_t q0, int64_t n, bool debug, const OutPtrs &out, hipStream_t stream, F &&after_chunk)
{
    if (q0 < 0 || n < 0 || q0 + n > ctx->scanned_Q)
        return fail(ctx, TQ_ERR_INVALID_ARG, "rows [%lld,+%lld) are outside the scanned batch of %lld quartets",
                    (long long)q0, (long long)n, (long long)ctx->scanned_Q);
    const int64_t chunk = svd_chunk_rows(ctx, n);
    int rc = ensure_svd(ctx, chunk);
    if (rc) return rc;
    const bool diag = diagnostic_mode(ctx);
    if ((rc = refuse_unflagged(ctx, out.flags))) return rc;
    const bool two = ctx->opt.svd_streams > 1 && n > chunk;
    if (two) {
        TQ_HIP(ctx, hipEventRecord(ctx->evFork, stream));
        TQ_HIP(ctx, hipStreamWaitEvent(ctx->sX, ctx->evFork, 0));
    }
    int64_t ci = 0;
    for (int64_t c0 = 0; c0 < n; c0 += chunk, ++ci) {
        const int64_t cn = (n - c0) < chunk ? (n - c0) : chunk;
        const int lane = two ? (int)(ci & 1) : 0;
        hipStream_t st = lane ? ctx->sX : stream;
        if (!(ctx->opt.phases & 2)) {                   // no score kernel runs: flag the rows here
            if (hipMemsetAsync(out.flags + c0, TQ_FLAG_INVALID_DIAGNOSTIC, (size_t)cn, st) != hipSuccess) {
                rc = fail(ctx, TQ_ERR_HIP, "hipMemsetAsync(flags) failed");
                break;
            }
        }
        if (ctx->opt.phases & 2) {
            const uint32_t *cm = ctx->d_cm + (size_t)(q0 + c0) * 256;
            const uint32_t *dq = ctx->scanned_q + (q0 + c0) * 4;
            OutPtrs o = offset_out(out, c0);
            o.flag_or = diag ? (uint32_t)TQ_FLAG_INVALID_DIAGNOSTIC : 0u;
            if ((rc = mark(ctx, TAG_ORIGIN, st, lane))) break;
            if (ctx->opt.svd_method == 0)
                rc = debug ? launch_svd<true>(ctx, cm, dq, cn, o, st, lane) : launch_svd<false>(ctx, cm, dq, cn, o, st, lane);
            else
                rc = debug ? launch_hqr<true>(ctx, cm, dq, cn, o, st, lane) : launch_hqr<false>(ctx, cm, dq, cn, o, st, lane);
            if (rc) break;
        }
        if ((rc = after_chunk(c0, cn, st))) break;
    }
    if (two) {                                   // join, also on the error path: nothing may stay forked
        if (hipEventRecord(ctx->evJoin, ctx->sX) != hipSuccess || hipStreamWaitEvent(stream, ctx->evJoin, 0) != hipSuccess)
            if (!rc) rc = fail(ctx, TQ_ERR_HIP, "stream join failed");
    }
    return rc;
}

struct NoChunkHook {
    int operator()(int64_t, int64_t, hipStream_t) const { return TQ_OK; }
};

// One pass of the path over quartets dq[0..Q) with device outputs: scan batches of <= ctx->opt.batch quartets,
// each followed by its singular-value stage.
template <typename F>
int launch(tq_ctx *ctx, const uint32_t *dq, int64_t Q, int subsample, bool debug, bool input_sorted,
           const OutPtrs &out, hipStream_t stream, F &&after_chunk, bool species = false)
{
    int rc = species ? species_ready(ctx, "species resolve") : check_ready(ctx, subsample);
    if (rc) return rc;
    if (Q == 0) return TQ_OK;
    if (ctx->timing) ctx->timed_calls++;
    const int64_t batch = Q < ctx->opt.batch ? Q : ctx->opt.batch;
    for (int64_t q0 = 0; q0 < Q; q0 += batch) {
        const int64_t n = (Q - q0) < batch ? (Q - q0) : batch;
        rc = species ? stage_species(ctx, dq + q0 * 4, n, stream) : stage_scan(ctx, dq + q0 * 4, n, subsample, input_sorted, stream);
        if (rc) return rc;
        rc = stage_svd(ctx, 0, n, debug, offset_out(out, q0), stream,
                       [&](int64_t c0, int64_t cn, hipStream_t st) { return after_chunk(q0 + c0, cn, st); });
        if (rc) return rc;
    }
    ctx->scanned_Q = 0;          // the slab belongs to this call only
    return TQ_OK;
}

int ensure_streams(tq_ctx *ctx)
{
    if (!ctx->sK) {
        TQ_HIP(ctx, ctx->sK.create());
        TQ_HIP(ctx, ctx->sC.create());
    }
    if (ctx->dev_api_pending) {                  // work of the device API may still be using the shared scratch
        TQ_HIP(ctx, hipStreamWaitEvent(ctx->sK, ctx->evDevApi, 0));
        ctx->dev_api_pending = false;
    }
    return TQ_OK;
}

// called before a device-API entry point enqueues work that touches the shared scratch (count slab, ordering and
// singular-value scratch, replicate layout): if the previous device-API call went to ANOTHER stream, this stream is
// made to wait for it -- two device-API calls of one context are ordered in call order whatever their streams
int enter_dev_api(tq_ctx *ctx, hipStream_t stream)
{
    if (ctx->dev_api_pending && ctx->evDevApi && stream != ctx->last_dev_stream)
        TQ_HIP(ctx, hipStreamWaitEvent(stream, ctx->evDevApi, 0));
    return TQ_OK;
}

// called after a device-API entry point has enqueued work on the caller's stream
int note_dev_api(tq_ctx *ctx, hipStream_t stream, int rc)
{
    if (!ctx->evDevApi) TQ_HIP(ctx, ctx->evDevApi.create());
    TQ_HIP(ctx, hipEventRecord(ctx->evDevApi, stream));
    ctx->dev_api_pending = true;
    ctx->last_dev_stream = stream;
    return rc;
}

int pipe_event(tq_ctx *ctx, size_t i, hipEvent_t *ev)
{
    while (ctx->pipe_events.size() <= i) {
        Event e;
        TQ_HIP(ctx, e.create());
        ctx->pipe_events.push_back(std::move(e));
    }
    *ev = ctx->pipe_events[i];
    return TQ_OK;
}

// Results of the host-buffer API: kernels on stream sK, result copies on stream sC.  The copy of chunk i
// (8 + 24 + 1 bytes per quartet) runs under the kernels of chunk i+1.  Destinations in page-locked
// memory (tq_host_alloc, hipHostMalloc, hipHostRegister) are written by the copy engine directly;
// pageable destinations go through two pinned staging pieces and one host memcpy per chunk, which the
// host does while the GPU works on the next chunk.
struct HostSink {
    tq_ctx *ctx;
    uint32_t *rstat;
    double *rscor;
    uint8_t *flags;
    const OutPtrs *dev;            // device outputs of row 0
    bool direct = false;
    bool single = false;           // pageable destinations, one piece: ONE D2H of the contiguous device region
    size_t off_rscor = 0, off_flags = 0;           // byte offsets of rscor / flags inside a staging piece
    PoolBuf<char> stage[2];
    int64_t stage_rows = 0, total_rows = 0;
    int64_t single_q0 = 0, single_n = 0;
    hipStream_t single_stream = nullptr;
    struct Pending { int64_t q0, n; hipEvent_t done; int buf; };
    Pending pend[2];
    int npend = 0;
    size_t nchunk = 0;

    int begin(int64_t Q)
    {
        total_rows = Q;
        // (a call whose results fit one small piece is cheaper as ONE staged copy than as three direct ones)
        direct = (size_t)Q * 33 > ((size_t)1 << 20) && is_pinned(rstat, (size_t)Q * 8) &&
                 is_pinned(rscor, (size_t)Q * 24) && (!flags || is_pinned(flags, (size_t)Q));
        if (!direct) {
            // what stage_svd will cut this call into: one scan batch of min(Q, batch) rows at a time, each in
            // chunks of svd_chunk_rows(batch rows) -- the last batch may be shorter, never longer
            const int64_t first_batch = Q < ctx->opt.batch ? Q : ctx->opt.batch;
            stage_rows = svd_chunk_rows(ctx, first_batch);
            if (Q > first_batch) {
                const int64_t tail = svd_chunk_rows(ctx, Q % first_batch ? Q % first_batch : first_batch);
                if (tail > stage_rows) stage_rows = tail;
            }
            // small calls (the reference's distributor hands out chunks of a few thousand quartets,
            // run_inference.py:73-96) are dominated by the number of HIP calls: when the whole call is ONE
            // chunk, the device outputs [rstat | rscor | flags] are one contiguous region -> one copy
            single = Q <= ctx->opt.batch && stage_rows >= Q && dev->flags &&
                     (const char *)dev->rscor > (const char *)dev->rstat && (const char *)dev->flags > (const char *)dev->rscor;
            off_rscor = single ? (size_t)((const char *)dev->rscor - (const char *)dev->rstat) : (size_t)stage_rows * 8;
            off_flags = single ? (size_t)((const char *)dev->flags - (const char *)dev->rstat) : (size_t)stage_rows * 32;
            const size_t bytes = off_flags + (size_t)stage_rows;
            for (int i = 0; i < (single ? 1 : 2); ++i)
                if (stage[i].alloc(bytes) != TQ_OK)
                    return fail(ctx, TQ_ERR_OOM, "out of page-locked host memory for the result staging");
        }
        return TQ_OK;
    }
    int drain_one()
    {
        const Pending p = pend[0];
        pend[0] = pend[1];
        --npend;
        TQ_HIP(ctx, hipEventSynchronize(p.done));
        const char *s = stage[p.buf];
        memcpy(rstat + p.q0 * 2, s, (size_t)p.n * 8);
        memcpy(rscor + p.q0 * 3, s + off_rscor, (size_t)p.n * 24);
        if (flags) memcpy(flags + p.q0, s + off_flags, (size_t)p.n);
        return TQ_OK;
    }
    // the kernels of chunk [q0, q0+n) have been enqueued on `st`
    int chunk(int64_t q0, int64_t n, hipStream_t st)
    {
        if (!direct && n > stage_rows)
            return fail(ctx, TQ_ERR_HIP, "internal: result chunk of %lld rows exceeds the staging piece of %lld",
                        (long long)n, (long long)stage_rows);
        if (single) {
            // one piece, one copy, nothing to overlap with: the copy goes behind the kernels on their own stream
            // and finish() waits for that stream -- no events, no second stream (a 1 000-quartet call is a
            // dozen HIP calls; every one of them shows)
            if (q0 != 0 || n != total_rows || nchunk != 0)
                return fail(ctx, TQ_ERR_HIP, "internal: single-piece result path got chunk [%lld,+%lld) of %lld rows",
                            (long long)q0, (long long)n, (long long)total_rows);
            TQ_HIP(ctx, hipMemcpyAsync(stage[0], dev->rstat, off_flags + (size_t)n, hipMemcpyDeviceToHost, st));
            single_q0 = q0;
            single_n = n;
            single_stream = st;
            ++nchunk;
            return TQ_OK;
        }
        hipEvent_t ready, done;
        int rc = pipe_event(ctx, 2 * (nchunk % 4), &ready);
        if (!rc) rc = pipe_event(ctx, 2 * (nchunk % 4) + 1, &done);
        if (rc) return rc;
        TQ_HIP(ctx, hipEventRecord(ready, st));
        TQ_HIP(ctx, hipStreamWaitEvent(ctx->sC, ready, 0));
        if (direct) {
            TQ_HIP(ctx, hipMemcpyAsync(rstat + q0 * 2, dev->rstat + q0 * 2, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->sC));
            TQ_HIP(ctx, hipMemcpyAsync(rscor + q0 * 3, dev->rscor + q0 * 3, (size_t)n * 24, hipMemcpyDeviceToHost, ctx->sC));
            if (flags)
                TQ_HIP(ctx, hipMemcpyAsync(flags + q0, dev->flags + q0, (size_t)n, hipMemcpyDeviceToHost, ctx->sC));
        } else {
            if (npend == 2) {                       // the staging piece this chunk needs is still in flight
                rc = drain_one();
                if (rc) return rc;
            }
            const int b = (int)(nchunk & 1);
            char *s = stage[b];
            TQ_HIP(ctx, hipMemcpyAsync(s, dev->rstat + q0 * 2, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->sC));
            TQ_HIP(ctx, hipMemcpyAsync(s + off_rscor, dev->rscor + q0 * 3, (size_t)n * 24, hipMemcpyDeviceToHost, ctx->sC));
            if (flags)
                TQ_HIP(ctx, hipMemcpyAsync(s + off_flags, dev->flags + q0, (size_t)n, hipMemcpyDeviceToHost, ctx->sC));
            TQ_HIP(ctx, hipEventRecord(done, ctx->sC));
            pend[npend++] = Pending{q0, n, done, b};
            if (npend == 2) {                       // copy out the older piece while the GPU works on
                rc = drain_one();
                if (rc) return rc;
            }
        }
        ++nchunk;
        return TQ_OK;
    }
    int finish()
    {
        int rc = TQ_OK;
        if (single && nchunk) {
            TQ_HIP(ctx, hipStreamSynchronize(single_stream));
            const char *s = stage[0];
            memcpy(rstat + single_q0 * 2, s, (size_t)single_n * 8);
            memcpy(rscor + single_q0 * 3, s + off_rscor, (size_t)single_n * 24);
            if (flags) memcpy(flags + single_q0, s + off_flags, (size_t)single_n);
            return TQ_OK;
        }
        while (npend && !rc) rc = drain_one();
        if (!rc && hipStreamSynchronize(ctx->sC) != hipSuccess) rc = fail(ctx, TQ_ERR_HIP, "result copy failed");
        return rc;
    }
    ~HostSink()
    {
        // never leave copies in flight into memory the caller may free, nor into the staging pieces, which go back to
        // the pool behind this body
        (void)hipStreamSynchronize(ctx->sK);
        (void)hipStreamSynchronize(ctx->sC);
    }
};

struct NoHostWork {
    int operator()() const { return TQ_OK; }
};

// device quartets -> host results (synchronous).  `while_gpu_works()` runs on the host after everything has been
// enqueued and before the results are waited for (a non-zero return aborts the call after the streams have drained).
template <typename F = NoHostWork>
int resolve_to_host(tq_ctx *ctx, const uint32_t *dq, int64_t Q, int subsample, bool input_sorted, uint32_t *rstat,
                    double *rscor, uint8_t *flags, uint32_t *d_rstat, double *d_rscor, uint8_t *d_flags,
                    F &&while_gpu_works = F())
{
    OutPtrs out{d_rstat, d_rscor, d_flags, nullptr, nullptr, nullptr};
    HostSink sink{ctx, rstat, rscor, flags, &out};
    int rc = sink.begin(Q);
    if (rc) return rc;
    rc = launch(ctx, dq, Q, subsample, false, input_sorted, out, ctx->sK,
                [&](int64_t q0, int64_t n, hipStream_t st) { return sink.chunk(q0, n, st); });
    if (rc) return rc;
    if ((rc = while_gpu_works())) return rc;          // ~HostSink drains the streams
    return sink.finish();
}

// device species quartets -> host results (synchronous), the pipeline of resolve_to_host
int species_to_host(tq_ctx *ctx, const uint32_t *dsq, int64_t Q, uint32_t *rstat, double *rscor, uint8_t *flags,
                    uint32_t *d_rstat, double *d_rscor, uint8_t *d_flags)
{
    OutPtrs out{d_rstat, d_rscor, d_flags, nullptr, nullptr, nullptr};
    HostSink sink{ctx, rstat, rscor, flags, &out};
    int rc = sink.begin(Q);
    if (rc) return rc;
    rc = launch(ctx, dsq, Q, 0, false, false, out, ctx->sK,
                [&](int64_t q0, int64_t n, hipStream_t st) { return sink.chunk(q0, n, st); }, true);
    if (rc) return rc;
    return sink.finish();
}

// Device scratch of a host-buffer call (tq_resolve*, tq_resolve_species*): the quartets, copied in on stream sK, then
// the outputs and the debug outputs the caller asked for
struct HostScratch {
    char *base = nullptr;
    size_t o_rstat = 0, o_rscor = 0, o_flags = 0, o_cm = 0, o_sv = 0, o_rk = 0;
    const uint32_t *dq() const { return (const uint32_t *)base; }
    uint32_t *rstat() const { return (uint32_t *)(base + o_rstat); }
    double *rscor() const { return (double *)(base + o_rscor); }
    uint8_t *flags() const { return (uint8_t *)(base + o_flags); }
};

int host_scratch(tq_ctx *ctx, const uint32_t *quartets, int64_t Q, bool cmats, bool svds, bool ranks, HostScratch *h)
{
    h->o_rstat = align_up((size_t)Q * 16, 256);
    h->o_rscor = align_up(h->o_rstat + (size_t)Q * 8, 256);
    h->o_flags = align_up(h->o_rscor + (size_t)Q * 24, 256);
    h->o_cm = align_up(h->o_flags + (size_t)Q, 256);
    h->o_sv = align_up(h->o_cm + (cmats ? (size_t)Q * 3072 : 0), 256);
    h->o_rk = align_up(h->o_sv + (svds ? (size_t)Q * 384 : 0), 256);
    const size_t total = align_up(h->o_rk + (ranks ? (size_t)Q * 12 : 0), 256);
    TQ_HIP(ctx, grow_scratch(ctx, total));
    if (int rc = ensure_streams(ctx)) return rc;
    h->base = ctx->d_scratch;
    // quartets H2D on the compute stream (asynchronous when the caller's array is page-locked)
    TQ_HIP(ctx, hipMemcpyAsync(h->base, quartets, (size_t)Q * 16, hipMemcpyHostToDevice, ctx->sK));
    return TQ_OK;
}

// The debug path of a host-buffer call: one launch with the kernel-level outputs, then every array back (synchronous)
int debug_to_host(tq_ctx *ctx, const HostScratch &h, int64_t Q, int subsample, bool species, bool input_sorted,
                  uint32_t *rstat, double *rscor, uint8_t *flags, uint32_t *cmats, double *svds, int32_t *ranks)
{
    OutPtrs out{};
    out.rstat = h.rstat();
    out.rscor = h.rscor();
    out.flags = h.flags();
    out.cmats = cmats ? (uint32_t *)(h.base + h.o_cm) : nullptr;
    out.svds = svds ? (double *)(h.base + h.o_sv) : nullptr;
    out.ranks = ranks ? (int32_t *)(h.base + h.o_rk) : nullptr;
    int rc = launch(ctx, h.dq(), Q, subsample, true, input_sorted, out, ctx->sK, NoChunkHook(), species);
    if (rc) {
        (void)hipStreamSynchronize(ctx->sK);
        return rc;
    }
    TQ_HIP(ctx, hipStreamSynchronize(ctx->sK));
    TQ_HIP(ctx, hipMemcpy(rstat, out.rstat, (size_t)Q * 8, hipMemcpyDeviceToHost));
    TQ_HIP(ctx, hipMemcpy(rscor, out.rscor, (size_t)Q * 24, hipMemcpyDeviceToHost));
    if (flags) TQ_HIP(ctx, hipMemcpy(flags, out.flags, (size_t)Q, hipMemcpyDeviceToHost));
    if (cmats) TQ_HIP(ctx, hipMemcpy(cmats, out.cmats, (size_t)Q * 3072, hipMemcpyDeviceToHost));
    if (svds) TQ_HIP(ctx, hipMemcpy(svds, out.svds, (size_t)Q * 384, hipMemcpyDeviceToHost));
    if (ranks) TQ_HIP(ctx, hipMemcpy(ranks, out.ranks, (size_t)Q * 12, hipMemcpyDeviceToHost));
    return TQ_OK;
}

// Class rows of quartets dq[0..Q) (species quartets with `species`): scan batches of <= ctx->opt.batch quartets into the
// count slab, each followed on the same stream by the class kernel, which writes at the batch's offset of d_classes.
// The caller has checked that the data are ready and that no diagnostic mode is set.
int launch_patterns(tq_ctx *ctx, const uint32_t *dq, int64_t Q, int subsample, bool species, uint32_t *d_classes,
                    hipStream_t stream)
{
    if (ctx->timing) ctx->timed_calls++;
    const int64_t batch = Q < ctx->opt.batch ? Q : ctx->opt.batch;
    for (int64_t q0 = 0; q0 < Q; q0 += batch) {
        const int64_t n = (Q - q0) < batch ? (Q - q0) : batch;
        int rc = species ? stage_species(ctx, dq + q0 * 4, n, stream) : stage_scan(ctx, dq + q0 * 4, n, subsample, false, stream);
        if (rc) return rc;
        constexpr int per_block = PAT_THREADS / 16;
        hipLaunchKernelGGL(tq_pattern_class_kernel, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(PAT_THREADS), 0,
                           stream, (const uint32_t *)ctx->d_cm, n, d_classes + (size_t)q0 * PAT_ROW);
        TQ_LAUNCHED(ctx, __func__);
    }
    ctx->scanned_Q = 0;          // the slab belongs to this call only
    return TQ_OK;
}

// what every pattern call checks before anything is launched
int patterns_ready(tq_ctx *ctx, const char *who, int subsample, bool species)
{
    int rc = species ? species_ready(ctx, who) : check_ready(ctx, subsample);
    if (rc) return rc;
    if (diagnostic_mode(ctx))
        return fail(ctx, TQ_ERR_INVALID_ARG, "%s: a timing-diagnostic mode is set (scan_method 2..5 or phases 1 / 2): its rows "
                    "are not results and class rows have no flags array to mark them with", who);
    return TQ_OK;
}

// Rows of `width` (4 or 5) indices: every index below `bound` and the row strictly ascending.  Per row the bound is
// judged first.
int check_set_rows(tq_ctx *ctx, const char *who, const uint32_t *sets, int64_t Q, int width, uint32_t bound, const char *bound_name)
{
    for (int64_t i = 0; i < Q; ++i) {
        const uint32_t *q = sets + width * i;
        bool over = false, ascending = true;
        for (int k = 0; k < width; ++k) over |= q[k] >= bound;
        for (int k = 1; k < width; ++k) ascending &= q[k - 1] < q[k];
        if (over)
            return fail(ctx, TQ_ERR_INVALID_ARG, "%s: row %lld has an index >= %s=%u", who, (long long)i, bound_name, bound);
        if (!ascending && width == 4)
            return fail(ctx, TQ_ERR_INVALID_ARG, "%s: row %lld (%u, %u, %u, %u) is not strictly ascending", who, (long long)i,
                        q[0], q[1], q[2], q[3]);
        if (!ascending)
            return fail(ctx, TQ_ERR_INVALID_ARG, "%s: row %lld (%u, %u, %u, %u, %u) is not strictly ascending", who,
                        (long long)i, q[0], q[1], q[2], q[3], q[4]);
    }
    return TQ_OK;
}

int check_set_rows(tq_ctx *ctx, const char *who, const uint32_t *sets, int64_t Q, int width, bool species)
{
    return check_set_rows(ctx, who, sets, Q, width, (uint32_t)(species ? ctx->sp_K : ctx->T), species ? "K" : "T");
}

// What the device forms ask of their pointers: set rows of width 4 are read, and class rows written, as 16-byte words;
// 20-byte set rows are read as dwords.
int check_dev_alignment(tq_ctx *ctx, const char *who, const void *d_sets, int width, const void *d_classes)
{
    if (width == 4 && ((((uintptr_t)d_sets) | ((uintptr_t)d_classes)) & 15))
        return fail(ctx, TQ_ERR_INVALID_ARG, "%s: d_sets and d_classes must be 16-byte aligned", who);
    if (width != 4 && ((((uintptr_t)d_sets) & 3) | (((uintptr_t)d_classes) & 15)))
        return fail(ctx, TQ_ERR_INVALID_ARG, "%s: d_sets5 must be 4-byte and d_classes 16-byte aligned", who);
    return TQ_OK;
}

// host sets -> host class rows (synchronous): rows must be strictly ascending indices below T (species: K)
int patterns_to_host(tq_ctx *ctx, const char *who, const uint32_t *sets, int64_t Q, int subsample, bool species,
                     uint32_t *classes)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, who, [&]() -> int {
        if (Q < 0 || (Q > 0 && (!sets || !classes))) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: NULL pointer or negative Q", who);
        int rc = patterns_ready(ctx, who, subsample, species);
        if (rc) return rc;
        if (Q == 0) return TQ_OK;
        if ((rc = check_set_rows(ctx, who, sets, Q, 4, species))) return rc;
        const size_t o_cls = align_up((size_t)Q * 16, 256);
        TQ_HIP(ctx, grow_scratch(ctx, o_cls + (size_t)Q * PAT_ROW * sizeof(uint32_t)));
        if ((rc = ensure_streams(ctx))) return rc;
        char *base = ctx->d_scratch;
        uint32_t *d_classes = (uint32_t *)(base + o_cls);
        TQ_HIP(ctx, hipMemcpyAsync(base, sets, (size_t)Q * 16, hipMemcpyHostToDevice, ctx->sK));
        rc = launch_patterns(ctx, (const uint32_t *)base, Q, subsample, species, d_classes, ctx->sK);
        if (rc) {
            (void)hipStreamSynchronize(ctx->sK);
            return rc;
        }
        TQ_HIP(ctx, hipMemcpyAsync(classes, d_classes, (size_t)Q * PAT_ROW * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->sK));
        TQ_HIP(ctx, hipStreamSynchronize(ctx->sK));
        return TQ_OK;
    });
}

// device sets -> device class rows, enqueued on `stream`
int patterns_dev(tq_ctx *ctx, const char *who, const uint32_t *d_sets, int64_t Q, int subsample, bool species,
                 uint32_t *d_classes, hipStream_t stream)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, who, [&]() -> int {
        if (Q < 0 || (Q > 0 && (!d_sets || !d_classes))) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: NULL pointer or negative Q", who);
        if (int rc = patterns_ready(ctx, who, subsample, species)) return rc;
        if (Q == 0) return TQ_OK;
        if (int rc = check_dev_alignment(ctx, who, d_sets, 4, d_classes)) return rc;
        if (int rc = enter_dev_api(ctx, stream)) return rc;      // before any shared scratch is touched
        return note_dev_api(ctx, stream, launch_patterns(ctx, d_sets, Q, subsample, species, d_classes, stream));
    });
}

// the block count of every block-row and jackknife call
int check_block_count(tq_ctx *ctx, const char *who, int64_t B)
{
    if (B < 1 || B > PBLK_MAX_BLOCKS)
        return fail(ctx, TQ_ERR_INVALID_ARG, "%s: B=%lld blocks, must be 1..%lld", who, (long long)B, (long long)PBLK_MAX_BLOCKS);
    return TQ_OK;
}

// What the D-test entry points check: sizes and pointers (`rows_and_out`: the class rows and the output are there), the
// block count of the jackknife forms (`B`), and -- host forms only, `host_arrays` -- set_of and the validity of every test
// by its form (ClassPairTests, MaskPairTests).  The device forms cannot read their arrays and check sizes only.
template <class Tests>
int check_dstat_tests(tq_ctx *ctx, const char *who, bool rows_and_out, int64_t n_sets, const int64_t *B, const uint32_t *set_of,
                      const Tests tests, int64_t N, bool host_arrays)
{
    if (N < 0 || n_sets < 0 || (N > 0 && (!rows_and_out || !set_of || !tests.a || !tests.b)))
        return fail(ctx, TQ_ERR_INVALID_ARG, "%s: NULL pointer or negative size", who);
    if (B)
        if (int rc = check_block_count(ctx, who, *B)) return rc;
    for (int64_t t = 0; host_arrays && t < N; ++t) {
        if ((int64_t)set_of[t] >= n_sets)
            return fail(ctx, TQ_ERR_INVALID_ARG, "%s: test %lld has set_of=%u >= n_sets=%lld", who, (long long)t, set_of[t],
                        (long long)n_sets);
        if (!Tests::valid(tests[t]))
            return fail(ctx, TQ_ERR_INVALID_ARG, Tests::refusal, who, (long long)t, (unsigned)tests.a[t], (unsigned)tests.b[t]);
    }
    return TQ_OK;
}

// The device forms of the per-test kernels: one launch of one thread per test, `threads` to a workgroup, on `stream`.
template <class Kernel, class... Args>
int launch_per_test(tq_ctx *ctx, const char *who, Kernel kernel, int threads, int64_t N, void *stream, Args... args)
{
    if (N == 0) return TQ_OK;
    if (N > (int64_t)0x7FFFFFFF * threads) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: N=%lld tests exceed one launch", who, (long long)N);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((N + threads - 1) / threads)), dim3(threads), 0, (hipStream_t)stream, args...);
    TQ_LAUNCHED(ctx, who);
    return TQ_OK;
}

// The jackknife entry points, host and device form, for either form of the tests.
template <class Tests>
int jackknife_to_host(const char *who, const uint32_t *bclasses, int64_t n_sets, int64_t B, const uint32_t *set_of,
                      const Tests tests, int64_t N, double *out)
{
    return api(nullptr, who, [&]() -> int {
        if (int rc = check_dstat_tests(nullptr, who, bclasses && out, n_sets, &B, set_of, tests, N, true)) return rc;
        jackknife_host(bclasses, B, set_of, tests, N, out);
        return TQ_OK;
    });
}

template <class Tests>
int jackknife_dev(tq_ctx *ctx, const char *who, const uint32_t *d_bclasses, int64_t n_sets, int64_t B, const uint32_t *d_set_of,
                  const Tests tests, int64_t N, double *d_out, void *stream)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, who, [&]() -> int {
        if (int rc = check_dstat_tests(ctx, who, d_bclasses && d_out, n_sets, &B, d_set_of, tests, N, false)) return rc;
        return launch_per_test(ctx, who, tq_jackknife_kernel<Tests>, JK_THREADS, N, stream, d_bclasses, n_sets, B, d_set_of, tests, N,
                               d_out);
    });
}

// Block rows: of quartets (pattern_blocks.hpp), of species quartets (species_blocks.hpp), of five-taxon sets
// (quintet_blocks.hpp) or of five-species sets (species_quintet_blocks.hpp).
enum BlockKind { BLK_QUARTET, BLK_SPECIES, BLK_QUINTET, BLK_SPECIES_QUINTET };

constexpr int block_set_width(BlockKind kind) { return kind == BLK_QUINTET || kind == BLK_SPECIES_QUINTET ? QNT_TAXA : 4; }
constexpr bool block_set_species(BlockKind kind) { return kind == BLK_SPECIES || kind == BLK_SPECIES_QUINTET; }

// The range rule of five-species rows, behind species_ready (which holds the rule of four): every sum of a site is at most
// the product of the five totals, so S x product of the five largest species sizes < 2^32 keeps every slot in u32.
int species_quintet_ready(tq_ctx *ctx, const char *who)
{
    const int lin = species_lineages(ctx);
    const uint64_t bound = ctx->sp_bound5 * (uint64_t)(lin * lin * lin * lin * lin);        // <= 255^5 x 32 < 2^45
    if ((unsigned __int128)ctx->S * bound >= ((unsigned __int128)1 << 32))
        return fail(ctx, TQ_ERR_INVALID_ARG,
                    "%s: pooled counts may exceed u32: S=%lld x product of the five largest species sizes %llu >= 2^32%s",
                    who, (long long)ctx->S, (unsigned long long)bound, lin == 2 ? " (sizes in lineages: 2 per sample)" : "");
    return TQ_OK;
}

// The block rule: 1 <= B <= PBLK_MAX_BLOCKS blocks whose B + 1 boundaries increase strictly inside [0, S], the sites of
// `what` (ctx NULL: the context-free form of the taxon counts).
int check_block_rule(tq_ctx *ctx, const char *who, const int64_t *block_starts, int64_t B, int64_t S, const char *what)
{
    if (int rc = check_block_count(ctx, who, B)) return rc;
    if (block_starts[0] < 0)
        return fail(ctx, TQ_ERR_INVALID_ARG, "%s: block_starts[0]=%lld is negative", who, (long long)block_starts[0]);
    for (int64_t j = 0; j < B; ++j)
        if (block_starts[j + 1] <= block_starts[j])
            return fail(ctx, TQ_ERR_INVALID_ARG, "%s: block_starts[%lld]=%lld is not above block_starts[%lld]=%lld", who,
                        (long long)(j + 1), (long long)block_starts[j + 1], (long long)j, (long long)block_starts[j]);
    if (block_starts[B] > S)
        return fail(ctx, TQ_ERR_INVALID_ARG, "%s: block_starts[%lld]=%lld is past the S=%lld sites of the %s", who, (long long)B,
                    (long long)block_starts[B], (long long)S, what);
    return TQ_OK;
}

// What every form checks before anything is launched: the data (and the species map) and the block rule.
int blocks_ready(tq_ctx *ctx, const char *who, BlockKind kind, const int64_t *block_starts, int64_t B)
{
    if (int rc = block_set_species(kind) ? species_ready(ctx, who) : check_ready(ctx, 0)) return rc;
    if (kind == BLK_SPECIES_QUINTET)
        if (int rc = species_quintet_ready(ctx, who)) return rc;
    return check_block_rule(ctx, who, block_starts, B, ctx->S, "resident replicate");
}

// The boundaries reach the device behind the work already on `stream`, without waiting for it (StagingRing).  Calls of
// one context are ordered (enter_dev_api / ensure_streams), so one device array serves.
int stage_block_starts(tq_ctx *ctx, const int64_t *block_starts, int64_t B, hipStream_t stream)
{
    if (!ctx->d_bstarts) TQ_HIP(ctx, ctx->d_bstarts.alloc(PBLK_MAX_BLOCKS + 1));
    if (int rc = ctx->bstarts_ring.ensure(PBLK_MAX_BLOCKS + 1))
        return ring_fail(ctx, rc, "out of page-locked host memory for the block boundaries");
    int64_t *piece;
    TQ_HIP(ctx, ctx->bstarts_ring.next(piece));
    memcpy(piece, block_starts, (size_t)(B + 1) * sizeof(int64_t));
    TQ_HIP(ctx, hipMemcpyAsync(ctx->d_bstarts, piece, (size_t)(B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    TQ_HIP(ctx, ctx->bstarts_ring.sent(stream));
    return TQ_OK;
}

// Block rows of sets dq[0..Q) (u32[Q][4], five-taxon and five-species sets u32[Q][5]) into d_classes [Q][B][16]; the
// boundaries are in ctx->d_bstarts on this stream.  Always the natural layout; species sets read the species table
// (species_blocks.hpp, species_quintet_blocks.hpp),
// which is brought up to date on this stream first.  Neither the count slab nor the timing marks are touched.  A launch
// holds fewer than 2^31 items.
int launch_blocks(tq_ctx *ctx, BlockKind kind, const uint32_t *dq, int64_t Q, int64_t B, uint32_t *d_classes, hipStream_t stream)
{
    if (block_set_species(kind))
        if (int rc = ensure_species_table(ctx, stream)) return rc;
    const int64_t per = ((int64_t)1 << 30) / B;         // >= 2^18 sets
    const int64_t *starts = ctx->d_bstarts;
    for (int64_t q0 = 0; q0 < Q; q0 += per) {
        const int64_t n = (Q - q0) < per ? (Q - q0) : per;
        const dim3 grid((unsigned)((n * B + PBLK_ITEMS - 1) / PBLK_ITEMS)), block(PBLK_THREADS);
        const uint32_t *sets = dq + q0 * block_set_width(kind);
        uint32_t *rows = d_classes + (size_t)q0 * (size_t)B * PAT_ROW;
        const auto launch = [&](auto rule) {
            hipLaunchKernelGGL(tq_block_rows_kernel<decltype(rule)>, grid, block, 0, stream, rule, sets, n, starts, B, rows);
        };
        switch (kind) {
        case BLK_SPECIES:
            launch(SpeciesRule{{ctx->d_sp_tab, ctx->nat.Sp, ctx->S, (uint32_t)ctx->sp_K, species_lineage_offsets(ctx)}});
            break;
        case BLK_SPECIES_QUINTET:
            launch(SpeciesQuintetRule{{ctx->d_sp_tab, ctx->nat.Sp, ctx->S, (uint32_t)ctx->sp_K, species_lineage_offsets(ctx)}});
            break;
        case BLK_QUINTET:
            // (not a rule yet: as one its kernel measured slower, see quintet_blocks.hpp)
            hipLaunchKernelGGL(tq_quintet_blocks_kernel, grid, block, 0, stream, (const uint32_t *)ctx->nat.planes3, ctx->nat.W,
                               (uint32_t)ctx->T, sets, n, starts, B, rows);
            break;
        default:
            launch(QuartetRule{{ctx->nat.planes3, ctx->nat.W, (uint32_t)ctx->T}, ctx->opt.count_invariant ? 0xFFFFFFFFu : 0u});
        }
        TQ_LAUNCHED(ctx, __func__);
    }
    return TQ_OK;
}

// host sets -> host block rows (synchronous): tq_patterns_blocks, tq_patterns_blocks_species, tq_patterns_quintet_blocks
// and tq_patterns_quintet_blocks_species
int blocks_to_host(tq_ctx *ctx, const char *who, BlockKind kind, const uint32_t *sets, int64_t Q, const int64_t *block_starts,
                   int64_t B, uint32_t *classes)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, who, [&]() -> int {
        if (Q < 0 || !block_starts || (Q > 0 && (!sets || !classes)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "%s: NULL pointer or negative Q", who);
        int rc = blocks_ready(ctx, who, kind, block_starts, B);
        if (rc) return rc;
        const int width = block_set_width(kind);
        if ((rc = check_set_rows(ctx, who, sets, Q, width, block_set_species(kind)))) return rc;
        if (Q == 0) return TQ_OK;
        // chunks of whole sets, at most option "batch" items of Q * B each (one set where B alone exceeds it)
        int64_t chunk = ctx->opt.batch / B;
        if (chunk < 1) chunk = 1;
        if (chunk > Q) chunk = Q;
        const size_t row_bytes = (size_t)B * PAT_ROW * sizeof(uint32_t);
        const size_t set_bytes = (size_t)width * sizeof(uint32_t);
        const size_t o_cls = align_up((size_t)chunk * set_bytes, 256);
        TQ_HIP(ctx, grow_scratch(ctx, o_cls + (size_t)chunk * row_bytes));
        if ((rc = ensure_streams(ctx))) return rc;
        char *base = ctx->d_scratch;
        uint32_t *d_classes = (uint32_t *)(base + o_cls);
        rc = stage_block_starts(ctx, block_starts, B, ctx->sK);
        for (int64_t q0 = 0; q0 < Q && !rc; q0 += chunk) {
            const int64_t n = (Q - q0) < chunk ? (Q - q0) : chunk;
            if (hipMemcpyAsync(base, sets + q0 * width, (size_t)n * set_bytes, hipMemcpyHostToDevice, ctx->sK) != hipSuccess)
                rc = fail(ctx, TQ_ERR_HIP, "%s: copy of the sets failed", who);
            if (!rc) rc = launch_blocks(ctx, kind, (const uint32_t *)base, n, B, d_classes, ctx->sK);
            if (!rc && hipMemcpyAsync((char *)classes + (size_t)q0 * row_bytes, d_classes, (size_t)n * row_bytes, hipMemcpyDeviceToHost,
                                      ctx->sK) != hipSuccess)
                rc = fail(ctx, TQ_ERR_HIP, "%s: copy of the block rows failed", who);
        }
        if (hipStreamSynchronize(ctx->sK) != hipSuccess && !rc) rc = fail(ctx, TQ_ERR_HIP, "%s: hipStreamSynchronize failed", who);
        return rc;
    });
}

// device sets -> device block rows, enqueued on `stream`
int blocks_dev(tq_ctx *ctx, const char *who, BlockKind kind, const uint32_t *d_sets, int64_t Q, const int64_t *block_starts,
               int64_t B, uint32_t *d_classes, hipStream_t stream)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, who, [&]() -> int {
        if (Q < 0 || !block_starts || (Q > 0 && (!d_sets || !d_classes)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "%s: NULL pointer or negative Q", who);
        if (int rc = blocks_ready(ctx, who, kind, block_starts, B)) return rc;
        if (Q == 0) return TQ_OK;
        if (int rc = check_dev_alignment(ctx, who, d_sets, block_set_width(kind), d_classes)) return rc;
        if (int rc = enter_dev_api(ctx, stream)) return rc;          // behind a tq_bootstrap_async that rebuilds the layout
        int rc = stage_block_starts(ctx, block_starts, B, stream);
        if (!rc) rc = launch_blocks(ctx, kind, d_sets, Q, B, d_classes, stream);
        return note_dev_api(ctx, stream, rc);
    });
}

// ---------------------------------------------------------------------------------------------
// Taxon counts (taxdist.hpp): pair rows u32[B][T][T][4] of the resident replicate, natural layout always.
// ---------------------------------------------------------------------------------------------

// The items of one launch reach the device through a StagingRing too: a call of up to two launches never waits for the
// stream.
int stage_td_items(tq_ctx *ctx, const TdItem *items, int64_t n, hipStream_t stream)
{
    if (!ctx->d_td_items) TQ_HIP(ctx, ctx->d_td_items.alloc((size_t)TD_LAUNCH_ITEMS));
    if (int rc = ctx->td_ring.ensure((size_t)TD_LAUNCH_ITEMS))
        return ring_fail(ctx, rc, "out of page-locked host memory for the work items of the taxon counts");
    TdItem *piece;
    TQ_HIP(ctx, ctx->td_ring.next(piece));
    memcpy(piece, items, (size_t)n * sizeof(TdItem));
    TQ_HIP(ctx, hipMemcpyAsync(ctx->d_td_items, piece, (size_t)n * sizeof(TdItem), hipMemcpyHostToDevice, stream));
    TQ_HIP(ctx, ctx->td_ring.sent(stream));
    return TQ_OK;
}

// blocks per piece of the rows: a piece holds at most 2^30 pair rows (the finish grid) and, with `bytes`, fits them
int64_t td_piece_blocks(int64_t T, int64_t B, int64_t bytes)
{
    const int64_t TT = T * T;
    int64_t n = (int64_t(1) << 30) / TT;
    if (bytes > 0 && bytes / (TT * 16) < n) n = bytes / (TT * 16);
    return n < 1 ? 1 : (n > B ? B : n);
}

// Blocks [b0, b1) of `block_starts` into d_out = the rows of block b0, on `stream`: the region zeroed, the product in
// launches of at most TD_LAUNCH_ITEMS work items, then tv and the mirror.  Adds the items to *n_items.
int launch_taxon_counts(tq_ctx *ctx, const char *who, const int64_t *block_starts, int64_t b0, int64_t b1, uint32_t *d_out,
                        hipStream_t stream, int64_t *n_items)
{
    const int64_t T = ctx->T, nt = (T + TD_BT - 1) / TD_BT, pairs = nt * (nt + 1) / 2, rows = (b1 - b0) * T * T;
    std::vector<TdItem> items;
    td_make_items(block_starts, b0, b1, ctx->opt.taxdist_slice_words, items);
    TQ_HIPF(ctx, who, hipMemsetAsync(d_out, 0, (size_t)rows * 16, stream));
    for (int64_t i0 = 0; i0 < (int64_t)items.size(); i0 += TD_LAUNCH_ITEMS) {
        const int64_t n = std::min<int64_t>(TD_LAUNCH_ITEMS, (int64_t)items.size() - i0);
        if (int rc = stage_td_items(ctx, items.data() + i0, n, stream)) return rc;
        const TdArgs a{ctx->nat.planes3, ctx->d_td_items, d_out, ctx->nat.W, (int32_t)T, (int32_t)nt, (int32_t)b0};
        hipLaunchKernelGGL(tq_taxon_counts_kernel, dim3((unsigned)pairs, (unsigned)n), dim3(TD_THREADS), 0, stream, a);
        TQ_LAUNCHED(ctx, who);
    }
    hipLaunchKernelGGL(tq_taxon_finish_kernel, dim3((unsigned)((rows + TD_THREADS - 1) / TD_THREADS)), dim3(TD_THREADS), 0, stream,
                       (uint4 *)d_out, b1 - b0, (int32_t)T);
    TQ_LAUNCHED(ctx, who);
    *n_items += (int64_t)items.size();
    return TQ_OK;
}

void note_taxon_counts(tq_ctx *ctx, int64_t items, int64_t piece, int64_t pieces)
{
    const int64_t nt = (ctx->T + TD_BT - 1) / TD_BT;
    ctx->td_stats[0] = nt * (nt + 1) / 2;
    ctx->td_stats[1] = items;
    ctx->td_stats[2] = ctx->opt.taxdist_slice_words;
    ctx->td_stats[3] = piece;
    ctx->td_stats[4] = pieces;
}

// ---------------------------------------------------------------------------------------------
// Accumulators on a fixed tree: concordance (concordance.hpp; device totals u64 [7 E + 2 T + 1] = per edge {conc,
// disc1, disc2, nu, nsnps sum, weight sum (f64 bits), score sum (f64 bits)}, per taxon {QFc, QFd}, skipped rows) and
// site concordance (scf.hpp; u64 [8 E + 1] = per edge {nq, nq_zero, sum conc / d1 / d2, fx conc / d1 / d2}, skipped
// rows).  `TreeAcc` is what they share: tree, host totals of tq_*_add, device tables, slabs and totals, every
// operation but the row kernel and the layout of a read.
// ---------------------------------------------------------------------------------------------

// The event behind the last device work of an accumulator: an enqueue on another stream first waits for it, a read or
// reset synchronises on it.  The owner calls create() with its device selected and finish() in its destructor's body.
struct StreamOrder {
    Event ev;                       // recorded behind the last device work
    bool pending = false;
    hipStream_t last = nullptr;
    hipError_t create() { return ev.create(); }
    // The end of an owner on `ctx` (NULL: a host back end, nothing to do): device selected, the work waited for.  A
    // destructor's body runs before its members' destructors, so the event and the owner's buffers go behind this.
    void finish(const tq_ctx *ctx)
    {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)sync();
    }
    hipError_t join(hipStream_t st) { return pending && st != last ? hipStreamWaitEvent(st, ev, 0) : hipSuccess; }
    hipError_t mark(hipStream_t st)
    {
        const hipError_t e = hipEventRecord(ev, st);
        if (e == hipSuccess) { pending = true; last = st; }
        return e;
    }
    hipError_t sync()
    {
        const hipError_t e = pending ? hipEventSynchronize(ev) : hipSuccess;
        if (e == hipSuccess) pending = false;
        return e;
    }
};

struct TreeAcc {
    tq_ctx *ctx = nullptr;          // device adds need one; messages go to tq_last_error(ctx)
    ConcTree t;
    int64_t words = 0;
    std::vector<uint64_t> hi;       // host adds: integer words
    DevBuf<uint16_t> d_lca, d_dep;
    DevBuf<int32_t> d_eid;
    DevBuf<uint64_t> d_slab, d_tot;
    int gmax = 0;                   // workgroups the slab holds
    int num_cu = 0;
    StreamOrder order;              // of the device adds
    TreeAcc() = default;
    TreeAcc(const TreeAcc &) = delete;
    ~TreeAcc() { order.finish(ctx); }
};

}  // namespace

struct tq_conc : TreeAcc {
    uint32_t min_snps = 1;
    double min_ratio = 1.0;
    std::vector<double> hf;         // host adds: weight / score sums
};

struct tq_scf : TreeAcc {};

namespace {

// The tree, host totals of edge_words * E + tail_words words and, with a context, the device side.  `who` names the
// calling function in the messages.  After a failure the caller's owner frees the accumulator.
int tree_acc_init(TreeAcc *acc, const char *who, const int32_t *parent, int64_t n_nodes, int64_t T, int edge_words,
                  int64_t tail_words, tq_ctx *ctx)
{
    const std::string err = conc_build_tree(parent, n_nodes, T, acc->t);
    if (!err.empty()) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: %s", who, err.c_str());
    acc->words = (int64_t)acc->t.E * edge_words + tail_words;
    acc->hi.assign(acc->words, 0);
    if (!ctx) return TQ_OK;
    const ConcTree &t = acc->t;
    acc->ctx = ctx;
    acc->num_cu = std::max(1, ctx->prop.multiProcessorCount);
    acc->gmax = (int)std::max<int64_t>(1, std::min<int64_t>(acc->num_cu, (int64_t(64) << 20) / (acc->words * 8)));
    TQ_HIPF(ctx, who, acc->d_lca.alloc((size_t)T * T));
    TQ_HIPF(ctx, who, acc->d_dep.alloc((size_t)t.N));
    TQ_HIPF(ctx, who, acc->d_eid.alloc((size_t)t.N));
    TQ_HIPF(ctx, who, acc->d_slab.alloc((size_t)acc->gmax * acc->words));
    TQ_HIPF(ctx, who, acc->d_tot.alloc((size_t)acc->words));
    TQ_HIPF(ctx, who, hipMemcpy(acc->d_lca, t.lca.data(), (size_t)T * T * 2, hipMemcpyHostToDevice));
    TQ_HIPF(ctx, who, hipMemcpy(acc->d_dep, t.dep.data(), (size_t)t.N * 2, hipMemcpyHostToDevice));
    TQ_HIPF(ctx, who, hipMemcpy(acc->d_eid, t.eid.data(), (size_t)t.N * 4, hipMemcpyHostToDevice));
    TQ_HIPF(ctx, who, hipMemset(acc->d_tot, 0, (size_t)acc->words * 8));
    TQ_HIPF(ctx, who, acc->order.create());
    return TQ_OK;
}

int tree_acc_wait(TreeAcc *acc)
{
    if (!acc->order.pending) return TQ_OK;
    TQ_HIP(acc->ctx, acc->order.sync());
    return TQ_OK;
}

int tree_acc_reset(TreeAcc *acc)
{
    std::fill(acc->hi.begin(), acc->hi.end(), 0);
    if (acc->ctx) {
        if (int rc = tree_acc_wait(acc)) return rc;
        TQ_HIP(acc->ctx, hipMemset(acc->d_tot, 0, (size_t)acc->words * 8));
    }
    return TQ_OK;
}

int tree_acc_shape(const TreeAcc *acc, int64_t *T, int64_t *n_edges, int64_t *mask_words)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    if (T) *T = acc->t.T;
    if (n_edges) *n_edges = acc->t.E;
    if (mask_words) *mask_words = acc->t.W;
    return TQ_OK;
}

// waits for the device adds and copies their totals to `dv` (zeros without a context)
int tree_acc_read(TreeAcc *acc, const char *who, std::vector<uint64_t> &dv)
{
    dv.assign(acc->words, 0);
    if (acc->ctx) {
        if (int rc = tree_acc_wait(acc)) return rc;
        TQ_HIP(acc->ctx, hipMemcpy(dv.data(), acc->d_tot, (size_t)acc->words * 8, hipMemcpyDeviceToHost));
    }
    return TQ_OK;
}

// One device add of n > 0 rows on `st`, behind the adds made on other streams.  At most CONC_ROWS_PER_LAUNCH rows go
// into a launch; `launch(form, G, r0, m, e_lo, e_n, first)` enqueues the caller's row kernel on G workgroups for the m
// rows from r0 and the edges e_lo .. e_lo + e_n - 1 -- form 0 / 1: tables in LDS for T <= CONC_T_LDS_A / CONC_T_LDS_B
// and every edge; form 2: tables through L2, a pass per CONC_EDGE_TILE edges, `first` on the first one -- and the fold
// adds the G slabs to the totals, the first `f64_edges` concordance records with their f64 words.
template <class Launch>
int tree_acc_add_dev(TreeAcc *acc, const char *who, int64_t n, int32_t f64_edges, hipStream_t st, Launch launch)
{
    tq_ctx *ctx = acc->ctx;
    const ConcTree &t = acc->t;
    TQ_HIP(ctx, acc->order.join(st));            // slab / totals in call order
    for (int64_t r0 = 0; r0 < n; r0 += CONC_ROWS_PER_LAUNCH) {
        const int64_t m = std::min<int64_t>(CONC_ROWS_PER_LAUNCH, n - r0);
        const int G = (int)std::max<int64_t>(1, std::min<int64_t>({(m + 4095) / 4096, (int64_t)acc->num_cu, (int64_t)acc->gmax}));
        if (t.T <= CONC_T_LDS_A) {
            launch(0, G, r0, m, 0, t.E, 1);
        } else if (t.T <= CONC_T_LDS_B) {
            launch(1, G, r0, m, 0, t.E, 1);
        } else {
            for (int32_t e0 = 0; e0 < t.E || e0 == 0; e0 += CONC_EDGE_TILE)       // a pass per tile of edges
                launch(2, G, r0, m, e0, std::min<int32_t>(CONC_EDGE_TILE, t.E - e0), e0 == 0);
        }
        hipLaunchKernelGGL(tq_conc_fold_kernel, dim3((unsigned)((acc->words + CONC_THREADS - 1) / CONC_THREADS)),
                           dim3(CONC_THREADS), 0, st, (const uint64_t *)acc->d_slab, G, acc->words, f64_edges, acc->d_tot);
        TQ_LAUNCHED(ctx, who);
    }
    TQ_HIP(ctx, acc->order.mark(st));
    return TQ_OK;
}

#include "split_table.hpp"     // TreeChunk and SplitTable of the accumulators over sets of trees below

}  // namespace

// ---------------------------------------------------------------------------------------------
// Consensus accumulator (consensus.hpp).  Host back end: one exact map mask -> count.  Device back end: the hash table
// on the device plus the same map for the splits that lost a hash collision; `cons_table` merges both by mask.
// ---------------------------------------------------------------------------------------------
struct tq_cons {
    tq_ctx *ctx = nullptr;          // NULL: host back end; messages go to tq_last_error(ctx)
    TreeChunk chunk;                // T, W and the device back end's chunk of trees
    SplitTable table;               // host adds; with a context the device table and the unresolved splits of its adds
    int64_t ntrees = 0;
    bool table_ok = false;          // tmasks / tcounts hold the canonical table of everything added
    std::vector<uint64_t> tmasks;
    std::vector<int64_t> tcounts;
    StreamOrder order;              // behind the last chunk
    tq_cons() = default;
    tq_cons(const tq_cons &) = delete;
    ~tq_cons() { order.finish(ctx); }
};

namespace {

// Waits for the last chunk and counts its unresolved splits in the host map.
int cons_drain(tq_cons *a)
{
    int64_t nun;
    return a->table.drain(a->ctx, "tq_cons", a->order, a->chunk.d_masks, nun, [a](int64_t, const std::vector<uint64_t> &m) {
        ++a->table.host[m];
        return true;
    });
}

// One chunk of n prepared records through the three kernels on `st`.
int cons_launch(tq_cons *a, int64_t n, const int32_t *recs, hipStream_t st)
{
    tq_ctx *ctx = a->ctx;
    ConsArgs p{};
    a->chunk.fill(p, n);
    a->table.fill(p);
    TQ_HIP(ctx, a->chunk.stage(n, recs, st, p));
    TQ_HIP(ctx, a->table.begin_chunk(st));
    const unsigned blocks = (unsigned)((p.items * p.G + CONS_THREADS - 1) / CONS_THREADS);
    hipLaunchKernelGGL(tq_cons_insert_kernel, dim3(blocks), dim3(CONS_THREADS), 0, st, p);
    hipLaunchKernelGGL(tq_cons_count_kernel, dim3(blocks), dim3(CONS_THREADS), 0, st, p);
    TQ_LAUNCHED(ctx, "tq_cons_add");
    TQ_HIP(ctx, a->table.end_chunk(st));
    TQ_HIP(ctx, a->order.mark(st));
    ++a->chunk.chunks;
    return TQ_OK;
}

// The canonical table of everything added (cached until the next add / reset).
int cons_table(tq_cons *a, const char *who)
{
    SplitTable &t = a->table;
    const int32_t W = a->chunk.W;
    if (t.overflow) return t.overflowed(a->ctx, who);
    if (a->ctx)
        if (int rc = cons_drain(a)) return rc;
    if (a->table_ok) return TQ_OK;
    if (!a->ctx || t.dev_entries == 0) {
        cons_sorted_table(t.host, W, a->tmasks, a->tcounts);
    } else {
        const int64_t n = t.dev_entries;
        std::vector<uint64_t> rep((size_t)n * W), cnt((size_t)n);
        TQ_HIP(a->ctx, hipMemcpy(rep.data(), t.d_rep, rep.size() * 8, hipMemcpyDeviceToHost));
        TQ_HIP(a->ctx, hipMemcpy(cnt.data(), t.d_count, cnt.size() * 8, hipMemcpyDeviceToHost));
        ConsMap all = t.host;
        std::vector<uint64_t> m((size_t)W);
        for (int64_t e = 0; e < n; ++e) {
            m.assign(rep.begin() + e * W, rep.begin() + (e + 1) * W);
            all[m] += (int64_t)cnt[e];
        }
        cons_sorted_table(all, W, a->tmasks, a->tcounts);
    }
    a->table_ok = true;
    return TQ_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Transfer bootstrap accumulator (tbe.hpp).  The reference branches are fixed at create; host back end: phi_sum in a
// host vector; device back end: phi_sum on the device, one chunk of trees staged and scanned at a time.
// ---------------------------------------------------------------------------------------------
struct tq_tbe {
    tq_ctx *ctx = nullptr;          // NULL: host back end; messages go to tq_last_error(ctx)
    TreeChunk chunk;                // T, W and the device back end's chunk of trees
    int64_t E = 0, ntrees = 0;
    std::vector<uint64_t> masks;    // [E][W] ascending
    std::vector<int32_t> p;         // [E]
    std::vector<uint64_t> phi_sum;  // host back end
    // device back end
    PinnedBuf<uint16_t> p_phi;
    DevBuf<int32_t> d_p;
    DevBuf<uint64_t> d_ref;
    DevBuf<unsigned long long> d_phi_sum;
    DevBuf<uint16_t> d_phi;
    StreamOrder order;              // behind the last chunk
    tq_tbe() = default;
    tq_tbe(const tq_tbe &) = delete;
    ~tq_tbe() { order.finish(ctx); }
};

namespace {

// One chunk of n prepared records: the masks, then the distances, on `st`.  With `want_phi` the chunk's phi rows
// follow into the page-locked buffer.
int tbe_launch(tq_tbe *a, int64_t n, const int32_t *recs, hipStream_t st, bool want_phi)
{
    tq_ctx *ctx = a->ctx;
    const TreeChunk &c = a->chunk;
    ConsArgs p{};
    c.fill(p, n);
    TbeArgs t{};
    t.trees = c.d_trees; t.masks = c.d_masks; t.ref = a->d_ref; t.p = a->d_p; t.phi_sum = a->d_phi_sum;
    t.phi = want_phi ? a->d_phi.get() : nullptr;
    t.T = c.T; t.W = c.W; t.E = (int32_t)a->E;
    TQ_HIP(ctx, a->chunk.stage(n, recs, st, p));
    hipLaunchKernelGGL(tq_tbe_kernel, dim3((unsigned)n, (unsigned)((a->E + BT_ROWS - 1) / BT_ROWS)), dim3(BT_THREADS), 0, st, t);
    TQ_LAUNCHED(ctx, "tq_tbe_add");
    if (want_phi) TQ_HIP(ctx, hipMemcpyAsync(a->p_phi, a->d_phi, (size_t)n * a->E * 2, hipMemcpyDeviceToHost, st));
    TQ_HIP(ctx, a->order.mark(st));
    ++a->chunk.chunks;
    return TQ_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Tree distance accumulator (treedist.hpp).  Host back end: an exact map mask -> id and one ascending id list per tree.
// Device back end: a consensus table of its own gives the ids, the same map resolves the splits that lost a hash
// collision; a read builds the bit rows and multiplies them.
// ---------------------------------------------------------------------------------------------
struct tq_rf {
    tq_ctx *ctx = nullptr;          // NULL: host back end; messages go to tq_last_error(ctx)
    TreeChunk chunk;                // T, W and the device back end's chunk of trees
    SplitTable table;               // host: mask -> id (host back end) or -> k, the id being max_splits - 1 - k (device)
    int64_t max_trees = 0, ntrees = 0;
    std::vector<int64_t> host_count;        // [id or k] trees that hold it
    std::vector<std::vector<uint32_t>> lists;       // host back end: the ascending ids of every tree
    bool final_ok = false;          // the matrices below / on the device are those of everything added
    std::vector<int32_t> h_nsplits; // host back end results
    std::vector<uint32_t> h_shared, h_rf;
    int64_t columns = 0, col_chunks = 0;    // of the last read
    // device back end
    int64_t cw_chunk = 0;
    int64_t chunk_base = 0;         // first tree of the chunk in flight
    DevBuf<int32_t> d_nsplits;
    DevBuf<unsigned long long> d_bits;
    DevBuf<uint32_t> d_newid, d_ids, d_colmap, d_shared, d_rf;
    PinnedBuf<uint32_t> p_newid;
    StreamOrder order;              // behind the last chunk
    tq_rf() = default;
    tq_rf(const tq_rf &) = delete;
    ~tq_rf() { order.finish(ctx); }
};

namespace {

// the id of a split in the host map, which has room for `room` of them: a new split takes the next number; one more
// tree holds it.  NULL when the map is full.
const int64_t *rf_host_id(tq_rf *a, const std::vector<uint64_t> &m, int64_t room)
{
    auto it = a->table.host.find(m);
    if (it == a->table.host.end()) {
        if ((int64_t)a->table.host.size() >= room) return nullptr;
        it = a->table.host.emplace(m, (int64_t)a->table.host.size()).first;
        a->host_count.push_back(0);
    }
    ++a->host_count[(size_t)it->second];
    return &it->second;
}

// empty table and no trees (also the reset).  ids, bit rows and matrices need no clearing: a read uses the rows of the
// trees added since, all of which an add has written.
int rf_clear_dev(tq_rf *a)
{
    TQ_HIP(a->ctx, hipMemset(a->d_nsplits, 0, (size_t)a->max_trees * 4));
    return a->table.clear(a->ctx);
}

// Waits for the last chunk, gives its unresolved splits their ids from the host map and stores them.
int rf_drain(tq_rf *a)
{
    tq_ctx *ctx = a->ctx;
    SplitTable &t = a->table;
    int64_t nun;
    if (int rc = t.drain(ctx, "tq_rf", a->order, a->chunk.d_masks, nun, [a, &t](int64_t u, const std::vector<uint64_t> &m) {
            const int64_t *k = rf_host_id(a, m, t.max_splits - t.dev_entries);
            if (k) a->p_newid[u] = (uint32_t)(t.max_splits - 1 - *k);
            return k != nullptr;
        }))
        return rc;
    if (nun == 0) return TQ_OK;
    hipStream_t st = a->order.last;
    RfIdentArgs r{a->d_ids, a->d_nsplits, a->chunk_base};
    TQ_HIP(ctx, hipMemcpyAsync(a->d_newid, a->p_newid, (size_t)nun * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(tq_rf_patch_kernel, dim3((unsigned)((nun + CONS_THREADS - 1) / CONS_THREADS)), dim3(CONS_THREADS), 0, st,
                       (const uint32_t *)t.d_unres, (const uint32_t *)a->d_newid, nun, r, a->chunk.T - 2);
    TQ_LAUNCHED(ctx, __func__);
    TQ_HIP(ctx, hipStreamSynchronize(st));
    return TQ_OK;
}

// One chunk of n prepared records, trees first .. first + n - 1, on `st`.
int rf_launch(tq_rf *a, int64_t first, int64_t n, const int32_t *recs, hipStream_t st)
{
    tq_ctx *ctx = a->ctx;
    ConsArgs p{};
    a->chunk.fill(p, n);
    a->table.fill(p);
    const RfIdentArgs r{a->d_ids, a->d_nsplits, first};
    TQ_HIP(ctx, a->chunk.stage(n, recs, st, p));
    TQ_HIP(ctx, a->table.begin_chunk(st));
    const unsigned blocks = (unsigned)((p.items * p.G + CONS_THREADS - 1) / CONS_THREADS);
    hipLaunchKernelGGL(tq_cons_insert_kernel, dim3(blocks), dim3(CONS_THREADS), 0, st, p);
    hipLaunchKernelGGL(tq_rf_ident_kernel, dim3(blocks), dim3(CONS_THREADS), 0, st, p, r);
    TQ_LAUNCHED(ctx, "tq_rf_add");
    TQ_HIP(ctx, a->table.end_chunk(st));
    TQ_HIP(ctx, a->order.mark(st));
    a->chunk_base = first;
    ++a->chunk.chunks;
    return TQ_OK;
}

// Host back end: the three arrays of everything added.
void rf_host_final(tq_rf *a)
{
    const int64_t N = a->ntrees;
    a->h_nsplits.assign((size_t)N, 0);
    a->h_shared.assign((size_t)(N * N), 0);
    a->h_rf.assign((size_t)(N * N), 0);
    for (int64_t i = 0; i < N; ++i) a->h_nsplits[i] = (int32_t)a->lists[i].size();
    for (int64_t i = 0; i < N; ++i) {
        a->h_shared[i * N + i] = (uint32_t)a->h_nsplits[i];
        for (int64_t j = i + 1; j < N; ++j) {
            const uint32_t s = rf_host_shared(a->lists[i], a->lists[j]);
            const uint32_t d = rf_distance((uint32_t)a->h_nsplits[i], (uint32_t)a->h_nsplits[j], s);
            a->h_shared[i * N + j] = a->h_shared[j * N + i] = s;
            a->h_rf[i * N + j] = a->h_rf[j * N + i] = d;
        }
    }
    a->columns = 0;
    for (int64_t c : a->host_count) a->columns += c >= 2;
    a->col_chunks = 0;
}

// Device back end: columns, bit rows, the product and the epilogue; the matrices stay on the device.
int rf_dev_final(tq_rf *a)
{
    tq_ctx *ctx = a->ctx;
    const int64_t N = a->ntrees, nd = a->table.dev_entries, nh = (int64_t)a->host_count.size();
    const int64_t max_splits = a->table.max_splits, nodes = a->chunk.nodes();
    // columns in entry order: the device entries, then the host's
    std::vector<unsigned long long> cnt((size_t)nd);
    if (nd) TQ_HIP(ctx, hipMemcpy(cnt.data(), a->table.d_count, (size_t)nd * 8, hipMemcpyDeviceToHost));
    std::vector<uint32_t> dev_col((size_t)nd), host_col((size_t)nh);       // host_col[i] belongs to id max_splits - nh + i
    uint32_t C = 0;
    for (int64_t e = 0; e < nd; ++e) dev_col[e] = cnt[e] >= 2 ? C++ : RF_NONE;
    for (int64_t k = 0; k < nh; ++k) host_col[nh - 1 - k] = a->host_count[k] >= 2 ? C++ : RF_NONE;
    hipStream_t st = a->order.last;
    int64_t launched = 0;
    TQ_HIP(ctx, hipMemsetAsync(a->d_shared, 0, (size_t)(N * N) * 4, st));
    if (C) {
        if (nd) TQ_HIP(ctx, hipMemcpyAsync(a->d_colmap, dev_col.data(), (size_t)nd * 4, hipMemcpyHostToDevice, st));
        if (nh)
            TQ_HIP(ctx, hipMemcpyAsync(a->d_colmap + (max_splits - nh), host_col.data(), (size_t)nh * 4,
                                       hipMemcpyHostToDevice, st));
        const int64_t per = a->cw_chunk * 64, nt = (N + RF_BT - 1) / RF_BT;
        RfBitArgs b{};
        b.ids = a->d_ids; b.colmap = a->d_colmap; b.bits = a->d_bits;
        b.items = N * nodes; b.nodes = (int32_t)nodes;
        RfGemmArgs g{};
        g.bits = (const uint64_t *)a->d_bits.get(); g.shared = a->d_shared;
        g.N = (int32_t)N; g.nt = (int32_t)nt;
        for (int64_t c0 = 0; c0 < (int64_t)C; c0 += per) {
            b.col0 = (uint32_t)c0;
            b.ncol = (uint32_t)std::min<int64_t>(per, (int64_t)C - c0);
            g.Cw = (int32_t)((b.ncol + 63) / 64);
            b.pitch = g.pitch = g.Cw;           // rows packed to the chunk's words (at most cw_chunk)
            TQ_HIP(ctx, hipMemsetAsync(a->d_bits, 0, (size_t)(N * g.Cw) * 8, st));
            hipLaunchKernelGGL(tq_rf_scatter_kernel, dim3((unsigned)((b.items + RF_THREADS - 1) / RF_THREADS)), dim3(RF_THREADS),
                               0, st, b);
            hipLaunchKernelGGL(tq_rf_gemm_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(RF_THREADS), 0, st, g);
            ++launched;
        }
    }
    hipLaunchKernelGGL(tq_rf_final_kernel, dim3((unsigned)((N * N + RF_THREADS - 1) / RF_THREADS)), dim3(RF_THREADS), 0, st,
                       a->d_shared.get(), a->d_rf.get(), (const int32_t *)a->d_nsplits.get(), (int32_t)N);
    TQ_LAUNCHED(ctx, "tq_rf_read");
    TQ_HIP(ctx, hipStreamSynchronize(st));      // dev_col / host_col live until here
    a->columns = C;
    a->col_chunks = launched;
    return TQ_OK;
}

// The matrices of everything added (kept until the next add / reset).
int rf_final(tq_rf *a, const char *who)
{
    if (a->table.overflow) return a->table.overflowed(a->ctx, who);
    if (a->ctx)
        if (int rc = rf_drain(a)) return rc;
    if (a->final_ok) return TQ_OK;
    if (a->ntrees == 0) {
        a->columns = a->col_chunks = 0;
    } else if (!a->ctx) {
        rf_host_final(a);
    } else if (int rc = rf_dev_final(a)) {
        return rc;
    }
    a->final_ok = true;
    return TQ_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Accumulators over the quartet planes of a tree set: quartet distances (qdist.hpp) and leaf stability (stability.hpp).
// Both back ends keep the depth table of every tree added; a score call walks its quartets a chunk at a time: the planes
// of every tree, then their product (two u64 matrices) or their sums along the trees (counts rows and per-taxon sums).
// ---------------------------------------------------------------------------------------------
namespace {

// What QuartetPlanes::add and tq_stree_fit share (fit.hpp).  pars[r] = the prepared parent array of tree r: every tree is
// validated before anything is written.
int prepare_fit_trees(tq_ctx *ctx, const char *who, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride,
                      int64_t T, std::vector<std::vector<int32_t>> &pars)
{
    pars.assign((size_t)R, {});
    std::vector<std::vector<int32_t>> nch;
    for (int64_t r = 0; r < R; ++r) {
        if (n_nodes[r] > stride)
            return fail(ctx, TQ_ERR_INVALID_ARG, "%s: tree %lld: n_nodes exceeds the stride", who, (long long)r);
        const std::string err = conc_prepare_tree(parents + r * stride, n_nodes[r], T, pars[(size_t)r], nch);
        if (!err.empty()) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: tree %lld: %s", who, (long long)r, err.c_str());
        if ((int64_t)pars[(size_t)r].size() > 2 * T - 2)
            return fail(ctx, TQ_ERR_INVALID_ARG, "%s: tree %lld: internal error: a prepared tree of T taxa has "
                        "at most 2 T - 2 nodes", who, (long long)r);
    }
    return TQ_OK;
}

// the records tq_fit_table_kernel reads, S = 2 T words a tree: the prepared parents, zeros, the node count in the last word
void fit_stage_records(int32_t *rec0, const std::vector<std::vector<int32_t>> &pars, int64_t S)
{
    memset(rec0, 0, pars.size() * (size_t)S * 4);
    for (size_t r = 0; r < pars.size(); ++r) {
        memcpy(rec0 + r * S, pars[r].data(), pars[r].size() * 4);
        rec0[r * S + S - 1] = (int32_t)pars[r].size();
    }
}

// the grid of tq_fit_table_kernel in x (its y: the trees)
unsigned fit_table_blocks(int64_t T)
{
    const int64_t span = (int64_t)fit_pairs_span((uint32_t)T);
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((span + 4 * FIT_THREADS - 1) / (4 * FIT_THREADS), FIT_TABLE_BLOCKS));
}

// What the accumulators over the quartet planes of a tree set share (quartet distances, qdist.hpp; leaf stability,
// stability.hpp): the depth table of every tree added with the add path, one chunk of quartets with its page-locked
// staging, and the walk of a score call, chunk by chunk: unrank where ranks come in, the planes of every tree, then
// whatever the owner does with the planes.
struct QuartetPlanes {
    tq_ctx *ctx = nullptr;          // NULL: host back end; messages go to tq_last_error(ctx)
    int32_t T = 0;
    int64_t max_trees = 0, ntrees = 0;
    uint64_t q_total = 0;           // quartets scored since create / clear / reset
    bool scored = false;            // adds are refused until a clear or reset
    int64_t chunk_words = 0;        // plane words (of 64 quartets) of one chunk
    int64_t chunks = 0, tables = 0;
    // host back end
    std::vector<uint16_t> h_tab;    // [ntrees][T][T]
    // device back end
    int num_cu = 1;
    DevBuf<uint16_t> d_tab;         // [max_trees][T][T]
    DevBuf<int32_t> d_rec;          // [max_trees][2 T]: the prepared parents, as tq_fit_table_kernel reads them
    PinnedBuf<int32_t> p_rec;
    DevBuf<uint32_t> d_quart;       // [64 chunk_words][4]
    DevBuf<uint64_t> d_ranks, d_planes;     // [64 chunk_words], [max_trees][3][chunk_words]
    PinnedBuf<uint64_t> p_stage;    // 16 bytes per quartet of a chunk: its taxa or its rank on the way to the device
    StreamOrder copy;               // behind the last copy out of p_stage
    StreamOrder order;              // behind the last add / score
    QuartetPlanes() = default;
    QuartetPlanes(const QuartetPlanes &) = delete;
    ~QuartetPlanes() { finish(); }
    // the owner calls this in its destructor's body, ahead of its own buffers
    void finish()
    {
        order.finish(ctx);
        copy.finish(ctx);
    }
    int table_form() const { return !ctx ? 0 : T <= FIT_T_LDS ? 1 : 2; }

    // The limits, and with a context every allocation but the owner's.  `own_per_word`: the bytes per plane word of a
    // chunk the owner allocates on top.
    int create(const char *who, int64_t T_, int64_t max_trees_, tq_ctx *ctx_, int64_t own_per_word)
    {
        if (T_ < 4 || T_ > STREE_T_MAX) return fail(ctx_, TQ_ERR_INVALID_ARG, "%s: T must be 4..%d", who, STREE_T_MAX);
        if (max_trees_ < 1 || max_trees_ > QD_MAX_TREES)
            return fail(ctx_, TQ_ERR_INVALID_ARG, "%s: max_trees must be 1..%lld", who, (long long)QD_MAX_TREES);
        ctx = ctx_;
        T = (int32_t)T_;
        max_trees = max_trees_;
        chunk_words = QD_HOST_CHUNK_WORDS;
        if (!ctx) return TQ_OK;
        // per plane word of a chunk: 64 quartets as taxa and as ranks on the device, 16 page-locked bytes each, and
        // three plane words of every tree
        const int64_t per_word = 64 * (16 + 8 + 16) + max_trees * 3 * 8 + own_per_word;
        chunk_words = std::max<int64_t>(1, std::min<int64_t>(ctx->opt.qdist_scratch_bytes / per_word, QD_MAX_CHUNK_WORDS));
        num_cu = std::max(1, ctx->prop.multiProcessorCount);
        const size_t cq = (size_t)chunk_words * 64;
        TQ_HIPF(ctx, who, d_tab.alloc((size_t)max_trees * T * T));
        TQ_HIPF(ctx, who, d_rec.alloc((size_t)max_trees * 2 * T));
        TQ_HIPF(ctx, who, p_rec.alloc((size_t)max_trees * 2 * T));
        TQ_HIPF(ctx, who, d_quart.alloc(cq * 4));
        TQ_HIPF(ctx, who, d_ranks.alloc(cq));
        TQ_HIPF(ctx, who, d_planes.alloc((size_t)max_trees * 3 * chunk_words));
        TQ_HIPF(ctx, who, p_stage.alloc(cq * 2));
        TQ_HIPF(ctx, who, order.create());
        TQ_HIPF(ctx, who, copy.create());
        return TQ_OK;
    }

    // Every tree is validated first; the tables of the new trees are built and kept.
    int add(const char *who, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride, hipStream_t st)
    {
        if (int rc = tree_set_args(ctx, who, parents, n_nodes, R, stride)) return rc;
        if (R == 0) return TQ_OK;
        if (scored) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: quartets have been scored; clear or reset the accumulator first", who);
        if (ntrees + R > max_trees)
            return fail(ctx, TQ_ERR_INVALID_ARG, "%s: %lld trees held and %lld offered exceed max_trees = %lld", who,
                        (long long)ntrees, (long long)R, (long long)max_trees);
        const int64_t T64 = T;
        std::vector<std::vector<int32_t>> pars;
        if (int rc = prepare_fit_trees(ctx, who, parents, n_nodes, R, stride, T64, pars)) return rc;
        if (!ctx) {
            h_tab.resize((size_t)((ntrees + R) * T64 * T64));
            std::vector<uint32_t> dep;
            for (int64_t r = 0; r < R; ++r)
                fit_host_table(pars[(size_t)r], (uint32_t)T64, dep, &h_tab[(size_t)((ntrees + r) * T64 * T64)]);
            ntrees += R;
            tables += R;
            return TQ_OK;
        }
        TQ_HIP(ctx, order.join(st));
        const int64_t S = 2 * T64, first = ntrees;
        int32_t *rec0 = p_rec + first * S;                          // every tree has a record of its own: none is reused
        fit_stage_records(rec0, pars, S);
        TQ_HIP(ctx, hipMemcpyAsync(d_rec + first * S, rec0, (size_t)(R * S) * 4, hipMemcpyHostToDevice, st));
        FitTableArgs ta{d_rec + first * S, d_tab + first * T64 * T64, (uint32_t)T64};
        hipLaunchKernelGGL(tq_fit_table_kernel, dim3(fit_table_blocks(T64), (unsigned)R), dim3(FIT_THREADS), 0, st, ta);
        TQ_LAUNCHED(ctx, who);
        TQ_HIP(ctx, order.mark(st));
        ntrees += R;
        tables += R;
        return TQ_OK;
    }

    // quartets i32 [Q][4]: every one is validated before anything is scored
    int check_quartets(const char *who, const int32_t *quartets, int64_t Q) const
    {
        if (Q < 0 || (Q > 0 && !quartets)) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: NULL pointer or negative Q", who);
        for (int64_t i = 0; i < Q; ++i) {
            const int32_t *q = quartets + 4 * i;
            if (q[0] < 0 || q[0] >= T || q[1] < 0 || q[1] >= T || q[2] < 0 || q[2] >= T || q[3] < 0 || q[3] >= T)
                return fail(ctx, TQ_ERR_INVALID_ARG, "%s: quartet %lld: taxon out of range 0..%d", who, (long long)i, T - 1);
            if (q[0] == q[1] || q[0] == q[2] || q[0] == q[3] || q[1] == q[2] || q[1] == q[3] || q[2] == q[3])
                return fail(ctx, TQ_ERR_INVALID_ARG, "%s: quartet %lld: repeated taxon", who, (long long)i);
        }
        return TQ_OK;
    }

    // ranks u64 [Q], or NULL for the Q consecutive ranks from first_rank
    int check_ranks(const char *who, const uint64_t *ranks, uint64_t first_rank, int64_t Q) const
    {
        if (Q < 0) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: negative Q", who);
        if (!rank_space_fits(T)) return fail(ctx, TQ_ERR_INVALID_ARG, RANK_SPACE_MSG, who, (long long)T);
        const uint64_t total = choose4((uint64_t)T);
        if (ranks) {
            for (int64_t i = 0; i < Q; ++i)
                if (ranks[i] >= total)
                    return fail(ctx, TQ_ERR_INVALID_ARG, "%s: rank %lld: %llu is not below C(%d,4) = %llu", who, (long long)i,
                                (unsigned long long)ranks[i], T, (unsigned long long)total);
        } else if (!rank_range_fits(first_rank, Q, total)) {
            return fail(ctx, TQ_ERR_INVALID_ARG, "%s: rank range [%llu,+%lld) exceeds C(%d,4) = %llu", who,
                        (unsigned long long)first_rank, (long long)Q, T, (unsigned long long)total);
        }
        return TQ_OK;
    }

    // One score call: explicit quartets (`quartets`), explicit ranks (`ranks`) or the range from first_rank (both NULL).
    // Everything has been validated.  Per chunk of n quartets that begins at quartet q0 of the call, behind the planes:
    //   host back end   host(planes u64 [N][3][cw], cw, taxa u32 [n][4], n, q0)
    //   device          dev(n, q0) -> a return code: what it enqueues on `st` finds the taxa in d_quart and the planes in
    //                   d_planes ([N][3][(n + 63) / 64])
    template <class Host, class Dev>
    int score(const int32_t *quartets, const uint64_t *ranks, uint64_t first_rank, int64_t Q, hipStream_t st, const char *who,
              Host &&host, Dev &&dev)
    {
        if (Q == 0 || ntrees == 0) return TQ_OK;
        const int64_t N = ntrees;
        if (!ctx) {
            const int64_t per = QD_HOST_CHUNK_WORDS * 64, piece = per * 16;     // unranked a piece at a time
            std::vector<uint32_t> q;
            std::vector<uint64_t> planes;
            for (int64_t p0 = 0; p0 < Q; p0 += piece) {
                const int64_t np = std::min(piece, Q - p0);
                const uint32_t *src = quartets ? (const uint32_t *)quartets + 4 * p0 : nullptr;
                if (!quartets) {
                    q.resize((size_t)np * 4);
                    unrank_host(ranks ? ranks + p0 : nullptr, first_rank + (uint64_t)p0, np, T, q.data());
                    src = q.data();
                }
                for (int64_t q0 = 0; q0 < np; q0 += per) {
                    const int64_t nq = std::min(per, np - q0), cw = (nq + 63) / 64;
                    planes.resize((size_t)(N * 3 * cw));
                    for (int64_t t = 0; t < N; ++t)
                        qd_host_encode(&h_tab[(size_t)(t * T * T)], (uint32_t)T, src + 4 * q0, nq, cw, &planes[(size_t)(t * 3 * cw)]);
                    host(planes.data(), cw, src + 4 * q0, nq, p0 + q0);
                    ++chunks;
                }
                scored = true;
            }
            q_total += (uint64_t)Q;
            return TQ_OK;
        }
        TQ_HIP(ctx, order.join(st));
        const int64_t per = chunk_words * 64;
        for (int64_t q0 = 0; q0 < Q; q0 += per) {
            const int64_t n = std::min(per, Q - q0);
            if (quartets || ranks) {
                TQ_HIP(ctx, copy.sync());                               // the staging buffer is free again
                if (quartets) {
                    memcpy(p_stage, quartets + 4 * q0, (size_t)n * 16);
                    TQ_HIP(ctx, hipMemcpyAsync(d_quart, p_stage, (size_t)n * 16, hipMemcpyHostToDevice, st));
                } else {
                    memcpy(p_stage, ranks + q0, (size_t)n * 8);
                    TQ_HIP(ctx, hipMemcpyAsync(d_ranks, p_stage, (size_t)n * 8, hipMemcpyHostToDevice, st));
                }
                TQ_HIP(ctx, copy.mark(st));
            }
            if (!quartets) {
                hipLaunchKernelGGL(tq_unrank_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                                   ranks ? (const uint64_t *)d_ranks.get() : (const uint64_t *)nullptr,
                                   first_rank + (uint64_t)q0, n, T, d_quart.get());
                TQ_LAUNCHED(ctx, who);
            }
            scored = true;                                              // from here on the results hold part of the call
            const int64_t cw = (n + 63) / 64;
            QdEncodeArgs e{(const uint4 *)d_quart.get(), d_tab, d_planes, n, (int32_t)cw, (uint32_t)T};
            const unsigned slices = (unsigned)std::max<int64_t>(
                1, std::min<int64_t>((cw + QD_ENC_WORDS_PER_BLOCK - 1) / QD_ENC_WORDS_PER_BLOCK, 4096));
            if (T <= FIT_T_LDS)
                hipLaunchKernelGGL(tq_qd_encode_kernel<true>, dim3(slices, (unsigned)N), dim3(QD_THREADS), 0, st, e);
            else
                hipLaunchKernelGGL(tq_qd_encode_kernel<false>, dim3(slices, (unsigned)N), dim3(QD_THREADS), 0, st, e);
            TQ_LAUNCHED(ctx, who);
            if (int rc = dev(n, q0)) return rc;
            ++chunks;
            TQ_HIP(ctx, order.mark(st));
        }
        q_total += (uint64_t)Q;
        return TQ_OK;
    }

    // before the owner zeroes its results: the device is idle
    int quiesce()
    {
        if (!ctx) return TQ_OK;
        TQ_HIP(ctx, order.sync());
        TQ_HIP(ctx, copy.sync());
        return TQ_OK;
    }
    void forget_scores() { q_total = 0; scored = false; }
    void forget_trees()
    {
        h_tab.clear();
        ntrees = 0;
        chunks = tables = 0;
    }
};

}  // namespace

struct tq_qd {
    QuartetPlanes set;
    int64_t kslices = 0;
    std::vector<uint64_t> h_same, h_both;   // host back end: [ntrees][ntrees] once something has been scored
    DevBuf<unsigned long long> d_same, d_both;      // device back end: [max_trees^2], row pitch = ntrees
    tq_qd() = default;
    tq_qd(const tq_qd &) = delete;
    ~tq_qd() { set.finish(); }
};

// ---------------------------------------------------------------------------------------------
// Leaf stability accumulator (stability.hpp).  The trees, the chunk and the walk are a QuartetPlanes; behind the planes of
// a chunk the counts of every quartet along the trees, and the u64 sums per taxon.
// ---------------------------------------------------------------------------------------------
struct tq_ls {
    QuartetPlanes set;
    int64_t groups = 0;             // workgroups of the last count launch (0 on the host)
    std::vector<uint64_t> h_acc;    // host back end: [T][4]
    DevBuf<unsigned long long> d_acc;       // [T][4]
    DevBuf<uint2> d_counts;         // [64 chunk_words] rows of u16 x 4
    PinnedBuf<uint2> p_counts;
    tq_ls() = default;
    tq_ls(const tq_ls &) = delete;
    ~tq_ls() { set.finish(); }
};

namespace {

// the k slices of one product launch: `want` 0 = about QD_GRID_PER_CU workgroups per compute unit; never more than the
// staged word chunks, and no slice is empty.  Returns the words per slice.
int64_t qd_kslices(int64_t cw, int64_t nt, int num_cu, int want, int64_t *slices)
{
    const int64_t nchunks = (cw + BT_KW - 1) / BT_KW, pairs = nt * (nt + 1) / 2;
    int64_t ks = want > 0 ? want : ((int64_t)QD_GRID_PER_CU * num_cu + pairs - 1) / pairs;
    ks = std::max<int64_t>(1, std::min<int64_t>({ks, nchunks, 65535}));
    const int64_t per = (nchunks + ks - 1) / ks;
    *slices = (nchunks + per - 1) / per;
    return per * BT_KW;
}

// the product of the planes of the nq quartets of a chunk, on `st`
int qd_product(tq_qd *a, int64_t nq, hipStream_t st, const char *who)
{
    tq_ctx *ctx = a->set.ctx;
    const int64_t N = a->set.ntrees, cw = (nq + 63) / 64, nt = (N + QD_BT - 1) / QD_BT;
    QdGemmArgs g{};
    g.planes = a->set.d_planes; g.same = a->d_same; g.both = a->d_both;
    g.N = (int32_t)N; g.cw = (int32_t)cw; g.nt = (int32_t)nt;
    int64_t ks = 1;
    g.slice_words = (int32_t)qd_kslices(cw, nt, a->set.num_cu, ctx->opt.qdist_kslices, &ks);
    g.atomic = ks > 1;
    hipLaunchKernelGGL(tq_qd_gemm_kernel, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)ks), dim3(QD_THREADS), 0, st, g);
    TQ_LAUNCHED(ctx, who);
    a->kslices = ks;
    return TQ_OK;
}

// One score call of the quartet distances; everything has been validated
int qd_score(tq_qd *a, const int32_t *quartets, const uint64_t *ranks, uint64_t first_rank, int64_t Q, hipStream_t st,
             const char *who)
{
    const int64_t N = a->set.ntrees;
    return a->set.score(
        quartets, ranks, first_rank, Q, st, who,
        [&](const uint64_t *planes, int64_t cw, const uint32_t *, int64_t, int64_t) {
            if (a->h_same.empty()) {
                a->h_same.assign((size_t)(N * N), 0);
                a->h_both.assign((size_t)(N * N), 0);
            }
            qd_host_product(planes, N, cw, a->h_same.data(), a->h_both.data());
        },
        [&](int64_t n, int64_t) { return qd_product(a, n, st, who); });
}

// zero counts (device: the part of the matrices that N trees use; the rest has not been written since create)
int qd_zero(tq_qd *a)
{
    tq_ctx *ctx = a->set.ctx;
    if (int rc = a->set.quiesce()) return rc;
    if (ctx) {
        const size_t n = (size_t)(a->set.ntrees * a->set.ntrees) * 8;
        if (n && a->set.scored) {
            TQ_HIP(ctx, hipMemset(a->d_same, 0, n));
            TQ_HIP(ctx, hipMemset(a->d_both, 0, n));
            TQ_HIP(ctx, hipDeviceSynchronize());
        }
    }
    a->h_same.clear();
    a->h_both.clear();
    a->set.forget_scores();
    return TQ_OK;
}

// One score call of the leaf stability; everything has been validated.  With a counts array (u16 [Q][4]) the rows of a
// chunk come back through the page-locked staging before the next chunk is enqueued.
int ls_score(tq_ls *a, const int32_t *quartets, const uint64_t *ranks, uint64_t first_rank, int64_t Q, uint16_t *counts,
             hipStream_t st, const char *who)
{
    QuartetPlanes &s = a->set;
    tq_ctx *ctx = s.ctx;
    const int64_t N = s.ntrees;
    return s.score(
        quartets, ranks, first_rank, Q, st, who,
        [&](const uint64_t *planes, int64_t cw, const uint32_t *q, int64_t nq, int64_t q0) {
            ls_host_count(planes, N, cw, q, nq, counts ? counts + 4 * q0 : nullptr, a->h_acc.data());
        },
        [&](int64_t n, int64_t q0) -> int {
            LsCountArgs c{(const uint4 *)s.d_quart.get(), s.d_planes, counts ? a->d_counts.get() : nullptr, a->d_acc,
                          n, (int32_t)((n + 63) / 64), (int32_t)N, (uint32_t)s.T};
            const int64_t groups = (c.cw + LS_GROUP_WORDS - 1) / LS_GROUP_WORDS;
            const size_t lds = (size_t)(LS_TILE_WORDS + 4 * s.T) * 8;
            hipLaunchKernelGGL(tq_ls_count_kernel, dim3((unsigned)groups), dim3(LS_THREADS), lds, st, c);
            TQ_LAUNCHED(ctx, who);
            a->groups = groups;
            if (counts) {
                TQ_HIP(ctx, hipMemcpyAsync(a->p_counts, a->d_counts, (size_t)n * 8, hipMemcpyDeviceToHost, st));
                TQ_HIP(ctx, hipStreamSynchronize(st));
                memcpy(counts + 4 * q0, a->p_counts, (size_t)n * 8);
            }
            return TQ_OK;
        });
}

// zero sums; the trees stay
int ls_zero(tq_ls *a)
{
    tq_ctx *ctx = a->set.ctx;
    if (int rc = a->set.quiesce()) return rc;
    if (ctx && a->set.scored) {
        TQ_HIP(ctx, hipMemset(a->d_acc, 0, (size_t)a->set.T * 4 * 8));
        TQ_HIP(ctx, hipDeviceSynchronize());
    }
    std::fill(a->h_acc.begin(), a->h_acc.end(), 0);
    a->set.forget_scores();
    return TQ_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Exact supertree accumulator (supertree.hpp).  Host adds keep the weighted splits in host vectors; device adds append
// them to the root store on the device.  A build never modifies either, so it may be repeated with any seed.
// ---------------------------------------------------------------------------------------------
struct tq_stree {
    tq_ctx *ctx = nullptr;          // device adds and device builds need one; messages go to tq_last_error(ctx)
    int64_t ntaxa = 0, capacity = 0;
    int weights = 0;
    uint32_t min_snps = 1;
    double min_ratio = 1.0;
    int mode = 0;                   // 0: nothing added yet, 1: host rows, 2: device rows (they do not mix)
    int search = 0;                 // cut search rule: 0 = qmc_search on doubles, 1 = stree_search_exact (tq_stree_set_search)
    int64_t rows_in = 0;            // rows offered since create / reset (capacity counts these)
    // host rows
    std::vector<uint64_t> h_t, h_k;
    int64_t h_skipped = 0;
    unsigned __int128 h_sum = 0;
    // device rows and the working state of a build
    DevBuf<uint64_t> d_root_t, d_root_k;
    DevBuf<uint64_t> d_wt[2], d_wk[2];
    DevBuf<uint32_t> d_wn[2];
    DevBuf<unsigned long long> d_cnt, d_mat;
    DevBuf<StreeNode> d_nodes;
    DevBuf<uint32_t> d_map;
    DevBuf<uint8_t> d_side, d_cut;  // the search kernel's answer: side bytes as the map is laid out, a cut byte per node
    PinnedBuf<uint8_t> p_side, p_cut;
    PinnedBuf<uint64_t> p_mat;      // page-locked: a level's matrices, its nodes and side map, the counters
    PinnedBuf<StreeNode> p_nodes;
    PinnedBuf<uint32_t> p_map;
    PinnedBuf<unsigned long long> p_cnt;
    int64_t max_cells = 0, max_nodes = 0;
    int num_cu = 1;
    StreamOrder order;              // behind the last device add
    Stream own;                     // stream of tq_stree_graph / tq_stree_rows, which take none
    std::vector<StreeLevelStat> stats;   // of the last build
    // quartet fit (fit.hpp): allocated at the first fit, grow-only, freed with the accumulator
    int64_t fit_bytes = 0;          // bound of the table region, the option "fit_scratch_bytes" as the first fit read it
    DevBuf<uint16_t> d_fit_tab;     // [chunk trees][T][T]
    DevBuf<int32_t> d_fit_rec;      // [trees][2 T] prepared parent arrays
    PinnedBuf<int32_t> p_fit_rec;
    DevBuf<unsigned long long> d_fit_out;           // [trees][6], then the accumulator's counters
    PinnedBuf<unsigned long long> p_fit_out;
    int64_t fit_trees = 0;          // trees the record and result buffers hold
    // NNI scan (nni.hpp): allocated at the first scan on device rows (sizes depend on ntaxa alone), freed with the accumulator
    DevBuf<uint16_t> d_nni_tab;     // [T][T] LCA nodes, then [2 T] node depths
    DevBuf<uint64_t> d_nni_rec;     // [T] words = the 2 T i32 of the parent record, then [T] edge records
    PinnedBuf<uint64_t> p_nni_rec;
    DevBuf<unsigned long long> d_nni_w;             // [T][3] sums, then the accumulator's counters
    PinnedBuf<unsigned long long> p_nni_w;
    tq_stree() = default;
    tq_stree(const tq_stree &) = delete;
    ~tq_stree() { order.finish(ctx); }
};

namespace {

#define STREE_HIP(call)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            err = std::string(#call) + " failed: " + hipGetErrorString(e_);                   \
            return e_ == hipErrorOutOfMemory ? TQ_ERR_OOM : TQ_ERR_HIP;                       \
        }                                                                                     \
    } while (0)

// the two operations on the device, everything on the stream of the build call; each ends with one synchronisation
struct StreeDevBackend : StreeBackend {
    tq_stree *a = nullptr;
    hipStream_t st = nullptr;
    int cur = -1;                   // work buffer that holds the live quartets, -1: the root store
    int64_t n_live = 0;

    void fill(StreePassArgs &p) const
    {
        p.t4 = cur < 0 ? a->d_root_t : a->d_wt[cur];
        p.k = cur < 0 ? a->d_root_k : a->d_wk[cur];
        p.node = cur < 0 ? nullptr : a->d_wn[cur];
        p.n_live = &a->d_cnt[cur < 0 ? SC_KEPT : SC_LIVE0 + cur];
        p.nodes = a->d_nodes;
        p.mat = a->d_mat;
    }
    int begin(int64_t &live, std::string &err) override
    {
        STREE_HIP(hipMemcpyAsync(a->p_cnt, a->d_cnt, SC_WORDS * 8, hipMemcpyDeviceToHost, st));
        STREE_HIP(hipStreamSynchronize(st));
        cur = -1;
        live = n_live = (int64_t)a->p_cnt[SC_KEPT];
        return TQ_OK;
    }
    int graphs(const std::vector<StreeNode> &nodes, int64_t cells, int, const uint64_t *&mat, std::string &err) override
    {
        if (cells > a->max_cells || (int64_t)nodes.size() > a->max_nodes) {
            err = "a level exceeds the cells or nodes the accumulator was created for";
            return TQ_ERR_INVALID_ARG;
        }
        memcpy(a->p_nodes, nodes.data(), nodes.size() * sizeof(StreeNode));
        STREE_HIP(hipMemcpyAsync(a->d_nodes, a->p_nodes, nodes.size() * sizeof(StreeNode), hipMemcpyHostToDevice, st));
        STREE_HIP(hipMemsetAsync(a->d_mat, 0, (size_t)(2 * cells) * 8, st));
        StreePassArgs p{};
        fill(p);
        p.n_nodes = (int32_t)nodes.size();
        p.cells = cells;
        if (a->ctx->opt.stree_lds && cells <= STREE_LDS_CELLS && n_live >= 4096) {
            const int pairs = (int)std::max<int64_t>(1, std::min<int64_t>((n_live + 16383) / 16384, 64));
            hipLaunchKernelGGL(tq_stree_graph_lds_kernel, dim3(2 * pairs), dim3(STREE_LDS_THREADS), 0, st, p);
        } else {
            const int G = (int)std::max<int64_t>(1, std::min<int64_t>((n_live + STREE_THREADS - 1) / STREE_THREADS,
                                                                     8 * (int64_t)a->num_cu));
            hipLaunchKernelGGL(tq_stree_graph_kernel, dim3(G), dim3(STREE_THREADS), 0, st, p);
        }
        STREE_HIP(hipGetLastError());
        if (exact && a->ctx->opt.stree_search_dev) {                   // the search kernel reads d_mat behind this on `st`
            mat = nullptr;
            return TQ_OK;
        }
        STREE_HIP(hipMemcpyAsync(a->p_mat, a->d_mat, (size_t)(2 * cells) * 8, hipMemcpyDeviceToHost, st));
        STREE_HIP(hipStreamSynchronize(st));
        mat = a->p_mat;
        return TQ_OK;
    }
    int search(const std::vector<StreeNode> &nodes, int64_t cells, int level, uint64_t seed, std::vector<uint8_t> &sides,
               std::vector<uint8_t> &cuts, std::string &err) override
    {
        if (!a->ctx->opt.stree_search_dev) {                            // the matrices are in p_mat
            stree_search_level_host(nodes, a->p_mat, cells, level, seed, sides, cuts);
            return TQ_OK;
        }
        if ((int64_t)nodes.size() > a->max_nodes || (int64_t)sides.size() > 3 * a->max_nodes) {
            err = "a level exceeds the nodes the accumulator was created for";
            return TQ_ERR_INVALID_ARG;
        }
        StreeSearchArgs p{};
        p.nodes = a->d_nodes;                                       // uploaded by `graphs`
        p.n_nodes = (int32_t)nodes.size();
        p.cells = cells;
        p.mat = a->d_mat;
        p.seed = seed;
        p.level = (uint32_t)level;
        p.side = a->d_side;
        p.cut = a->d_cut;
        hipLaunchKernelGGL(tq_stree_search_kernel, dim3((unsigned)nodes.size()), dim3(STREE_SEARCH_THREADS), 0, st, p);
        STREE_HIP(hipGetLastError());
        STREE_HIP(hipMemcpyAsync(a->p_side, a->d_side, sides.size(), hipMemcpyDeviceToHost, st));
        STREE_HIP(hipMemcpyAsync(a->p_cut, a->d_cut, nodes.size(), hipMemcpyDeviceToHost, st));
        STREE_HIP(hipStreamSynchronize(st));
        memcpy(sides.data(), a->p_side, sides.size());
        memcpy(cuts.data(), a->p_cut, nodes.size());
        return TQ_OK;
    }
    int partition(const std::vector<StreeNode> &nodes, const std::vector<uint32_t> &map, int, int64_t &live,
                  std::string &err) override
    {
        if ((int64_t)nodes.size() > a->max_nodes || (int64_t)map.size() > 3 * a->max_nodes) {
            err = "a level exceeds the nodes the accumulator was created for";
            return TQ_ERR_INVALID_ARG;
        }
        const int dst = cur < 0 ? 0 : cur ^ 1;
        memcpy(a->p_nodes, nodes.data(), nodes.size() * sizeof(StreeNode));
        memcpy(a->p_map, map.data(), map.size() * 4);
        STREE_HIP(hipMemcpyAsync(a->d_nodes, a->p_nodes, nodes.size() * sizeof(StreeNode), hipMemcpyHostToDevice, st));
        STREE_HIP(hipMemcpyAsync(a->d_map, a->p_map, map.size() * 4, hipMemcpyHostToDevice, st));
        STREE_HIP(hipMemsetAsync(&a->d_cnt[SC_LIVE0 + dst], 0, 8, st));
        StreePassArgs p{};
        fill(p);
        p.n_nodes = (int32_t)nodes.size();
        p.map = a->d_map;
        p.out_t4 = a->d_wt[dst];
        p.out_k = a->d_wk[dst];
        p.out_node = a->d_wn[dst];
        p.out_live = &a->d_cnt[SC_LIVE0 + dst];
        const int G = (int)std::max<int64_t>(1, std::min<int64_t>((n_live + STREE_THREADS - 1) / STREE_THREADS,
                                                                 8 * (int64_t)a->num_cu));
        hipLaunchKernelGGL(tq_stree_partition_kernel, dim3(G), dim3(STREE_THREADS), 0, st, p);
        STREE_HIP(hipGetLastError());
        STREE_HIP(hipMemcpyAsync(&a->p_cnt[SC_LIVE0 + dst], &a->d_cnt[SC_LIVE0 + dst], 8, hipMemcpyDeviceToHost, st));
        STREE_HIP(hipStreamSynchronize(st));
        cur = dst;
        live = n_live = (int64_t)a->p_cnt[SC_LIVE0 + dst];
        return TQ_OK;
    }
};

// orders `st` behind the device adds made on another stream
int stree_join(tq_stree *acc, hipStream_t st)
{
    TQ_HIP(acc->ctx, acc->order.join(st));
    return TQ_OK;
}

// kept / skipped rows and the sum of k of everything added so far, read on `st` behind the device adds
int stree_counts(tq_stree *acc, hipStream_t st, int64_t &kept, int64_t &skipped, unsigned __int128 &sum)
{
    if (acc->mode == 2) {
        if (int rc = stree_join(acc, st)) return rc;
        TQ_HIP(acc->ctx, hipMemcpyAsync(acc->p_cnt, acc->d_cnt, SC_WORDS * 8, hipMemcpyDeviceToHost, st));
        TQ_HIP(acc->ctx, hipStreamSynchronize(st));
        kept = (int64_t)acc->p_cnt[SC_KEPT];
        skipped = (int64_t)acc->p_cnt[SC_SKIPPED];
        sum = (unsigned __int128)acc->p_cnt[SC_SUM_LO] + ((unsigned __int128)acc->p_cnt[SC_SUM_HI] << 32);
    } else {
        kept = (int64_t)acc->h_t.size();
        skipped = acc->h_skipped;
        sum = acc->h_sum;
    }
    return TQ_OK;
}

// One scan of the canonical tree `t` against the kept rows (nni.hpp): w[E][3].  Host rows, or none: the host execution.
// Device rows: the parent record and the edge records go up, tq_nni_table_kernel and tq_nni_kernel run on `st` behind
// the adds, the sums and the counters come back; one synchronisation.  `who` names the caller in messages.
int nni_scan_once(tq_stree *acc, const NniTree &t, hipStream_t st, const char *who, std::vector<uint64_t> &w)
{
    tq_ctx *ctx = acc->ctx;
    const int64_t T = acc->ntaxa, E = t.E;
    if (acc->mode != 2) {
        if (acc->h_sum >> 64) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: the sum of k does not fit in 64 bits", who);
        nni_host_rows(t, acc->h_t.data(), acc->h_k.data(), (int64_t)acc->h_t.size(), w);
        return TQ_OK;
    }
    if (int rc = stree_join(acc, st)) return rc;                    // behind the adds made on other streams
    const size_t wn = (size_t)T * 3;
    if (!acc->d_nni_tab.get()) {                                    // no scan is in flight: each one ends with a synchronisation
        TQ_HIP(ctx, acc->d_nni_rec.grow((size_t)2 * T));
        TQ_HIP(ctx, acc->p_nni_rec.grow((size_t)2 * T));
        TQ_HIP(ctx, acc->d_nni_w.grow(wn + SC_WORDS));
        TQ_HIP(ctx, acc->p_nni_w.grow(wn + SC_WORDS));
        TQ_HIP(ctx, acc->d_nni_tab.grow((size_t)T * T + 2 * T));
    }
    memset(acc->p_nni_rec, 0, (size_t)2 * T * 8);
    int32_t *prec = (int32_t *)acc->p_nni_rec.get();
    memcpy(prec, t.par.data(), (size_t)t.N * 4);
    prec[2 * T - 1] = t.N;
    if (E) memcpy(acc->p_nni_rec + T, t.rec.data(), (size_t)E * 8);
    TQ_HIP(ctx, hipMemcpyAsync(acc->d_nni_rec, acc->p_nni_rec, (size_t)2 * T * 8, hipMemcpyHostToDevice, st));
    TQ_HIP(ctx, hipMemsetAsync(acc->d_nni_w, 0, wn * 8, st));
    if (E > 0 && acc->rows_in > 0) {
        const int64_t span = (int64_t)fit_pairs_span((uint32_t)T);
        const unsigned table_blocks = (unsigned)std::max<int64_t>(
            1, std::min<int64_t>((span + 4 * NNI_THREADS - 1) / (4 * NNI_THREADS), NNI_TABLE_BLOCKS));
        const unsigned slices = (unsigned)std::max<int64_t>(
            1, std::min<int64_t>((acc->rows_in + NNI_ROWS_PER_BLOCK - 1) / NNI_ROWS_PER_BLOCK, NNI_MAX_SLICES));
        NniTableArgs ta{(const int32_t *)acc->d_nni_rec.get(), acc->d_nni_tab, (uint32_t)T};
        hipLaunchKernelGGL(tq_nni_table_kernel, dim3(table_blocks), dim3(NNI_THREADS), 0, st, ta);
        TQ_LAUNCHED(ctx, who);
        NniArgs na{acc->d_root_t, acc->d_root_k, &acc->d_cnt[SC_KEPT], acc->d_nni_tab, acc->d_nni_rec + T, acc->d_nni_w,
                   (uint32_t)T, (uint32_t)t.N, (uint32_t)E};
        if (T <= NNI_T_LDS) hipLaunchKernelGGL(tq_nni_kernel<true>, dim3(slices), dim3(NNI_THREADS), 0, st, na);
        else hipLaunchKernelGGL(tq_nni_kernel<false>, dim3(slices), dim3(NNI_THREADS), 0, st, na);
        TQ_LAUNCHED(ctx, who);
    }
    unsigned long long *cnt = acc->p_nni_w + wn;
    TQ_HIP(ctx, hipMemcpyAsync(acc->p_nni_w, acc->d_nni_w, wn * 8, hipMemcpyDeviceToHost, st));
    TQ_HIP(ctx, hipMemcpyAsync(cnt, acc->d_cnt, SC_WORDS * 8, hipMemcpyDeviceToHost, st));
    TQ_HIP(ctx, hipStreamSynchronize(st));
    const unsigned __int128 sum = (unsigned __int128)cnt[SC_SUM_LO] + ((unsigned __int128)cnt[SC_SUM_HI] << 32);
    if (sum >> 64) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: the sum of k does not fit in 64 bits", who);
    w.assign(acc->p_nni_w.get(), acc->p_nni_w.get() + (size_t)E * 3);
    return TQ_OK;
}

// One row per option of tq_set_option (bdsqr_stats, which holds no value, aside): the field of Options, its legal values
// -- lo..hi or, where `listed` is set, exactly the values whose bits it holds --, the value that asks for the default
// (NO_KEY: none), which is then read from a default-constructed Options, and the message of a refused value.  A flag
// stores value != 0 and refuses nothing.
struct OptionRow {
    const char *name;
    int Options::*i;                // the field is an int ...
    int64_t Options::*l;            // ... or an int64_t
    int64_t lo, hi;
    uint64_t listed;
    int64_t default_key;
    const char *refusal;
    bool flag;
};
constexpr int64_t NO_KEY = INT64_MIN, ANY = INT64_MAX;
constexpr OptionRow opt(const char *name, int Options::*f, int64_t lo, int64_t hi, int64_t key, const char *refusal)
{
    return {name, f, nullptr, lo, hi, 0, key, refusal, false};
}
constexpr OptionRow opt(const char *name, int64_t Options::*f, int64_t lo, int64_t hi, int64_t key, const char *refusal)
{
    return {name, nullptr, f, lo, hi, 0, key, refusal, false};
}
template <class... V>
constexpr OptionRow opt_listed(const char *name, int Options::*f, const char *refusal, V... values)
{
    return {name, f, nullptr, 0, 0, ((uint64_t(1) << values) | ...), 0, refusal, false};
}
constexpr OptionRow opt_flag(const char *name, int Options::*f) { return {name, f, nullptr, 0, 0, 0, NO_KEY, "", true}; }

constexpr OptionRow OPTION_TABLE[] = {
    opt_listed("nrep", &Options::nrep, "nrep must be 1,2,4,8,16 or 32", 1, 2, 4, 8, 16, 32),
    opt("waves_per_cu", &Options::waves_per_cu, 0, 1 << 20, NO_KEY, "waves_per_cu must be 0..2^20"),
    opt_flag("xcd_remap", &Options::xcd_remap),
    opt_flag("count_invariant", &Options::count_invariant),
    opt_flag("scan_pair", &Options::scan_pair),
    opt("scan_f4", &Options::scan_f4, -1, 1, NO_KEY, "scan_f4 must be -1 (subsample mode only), 0 or 1"),
    opt("site_pack", &Options::site_pack, -1, 1, NO_KEY, "site_pack must be -1 (automatic), 0 or 1"),
    opt("boot_pack", &Options::boot_pack, -1, 1, NO_KEY, "boot_pack must be -1 (automatic), 0 or 1"),
    opt("scan_dp", &Options::scan_dp, 0, 1, NO_KEY, "scan_dp must be 0 or 1"),
    opt("dp_min_quartets", &Options::dp_min_quartets, 0, ANY, 0, "dp_min_quartets must be >= 0"),
    opt("wg_min_quartets", &Options::wg_min_quartets, 0, ANY, 0, "wg_min_quartets must be >= 0"),
    opt("bidiag_layout", &Options::bidiag_layout, 0, 1, -1, "bidiag_layout must be -1 (default), 0 or 1"),
    opt_flag("park_t", &Options::park_t),
    opt_flag("share_c", &Options::share_c),
    opt("cons_hash_bits", &Options::cons_hash_bits, 1, 64, 0, "cons_hash_bits must be 1..64 (0 = default 64)"),
    opt("cons_scratch_bytes", &Options::cons_scratch_bytes, 1, ANY, 0, "cons_scratch_bytes must be >= 0 (0 = default 256 MiB)"),
    opt("stree_search_dev", &Options::stree_search_dev, 0, 1, NO_KEY, "stree_search_dev must be 0 or 1"),
    opt("fit_scratch_bytes", &Options::fit_scratch_bytes, 1, ANY, NO_KEY, "fit_scratch_bytes must be at least 1"),
    opt("qdist_scratch_bytes", &Options::qdist_scratch_bytes, 1, ANY, 0, "qdist_scratch_bytes must be >= 0 (0 = default 256 MiB)"),
    opt("taxdist_scratch_bytes", &Options::taxdist_scratch_bytes, 1, ANY, 0, "taxdist_scratch_bytes must be >= 0 (0 = default 256 MiB)"),
    opt("taxdist_slice_words", &Options::taxdist_slice_words, 8, TD_MAX_SLICE_WORDS, 0,
        "taxdist_slice_words must be a multiple of 8 in 8..65536 (0 = default)"),
    opt("qdist_kslices", &Options::qdist_kslices, 0, 65535, NO_KEY, "qdist_kslices must be 0 (auto) .. 65535"),
    opt("stree_lds", &Options::stree_lds, 0, 1, NO_KEY, "stree_lds must be 0 or 1"),
    opt("svd_wpc", &Options::svd_wpc, 0, 1 << 20, NO_KEY, "svd_wpc must be 0..2^20"),
    opt("svd_chunk", &Options::svd_chunk, 1, ANY, 0, "svd_chunk must be >= 0"),
    opt("svd_streams", &Options::svd_streams, 1, 2, 0, "svd_streams must be 0 (default), 1 or 2"),
    opt("bdsqr_maxit", &Options::bdsqr_maxit, 1, 1000, 0, "bdsqr_maxit must be 0..1000"),
    opt_listed("scan_wg", &Options::scan_wg, "scan_wg must be 0 (default), 1, 2, 3, 4, 6, 8 or 16", 1, 2, 3, 4, 6, 8, 16),
    opt("svd_method", &Options::svd_method, 0, 1, NO_KEY, "svd_method must be 0 (Jacobi) or 1 (HQR)"),
    opt("order", &Options::order, 0, 1, NO_KEY, "order must be 0 or 1"),
    opt("scan_method", &Options::scan_method, -1, 6, NO_KEY, "scan_method must be -1 (auto), 0, 1, 6 (or 2..5: timing diagnostics)"),
    opt("batch", &Options::batch, 1, ANY, 0, "batch must be >= 0"),
    opt("species_method", &Options::species_method, -1, 1, NO_KEY, "species_method must be -1 (auto), 0 (VALU form) or 1 (MFMA form)"),
    opt("species_alleles", &Options::species_alleles, 0, 1, NO_KEY,
        "species_alleles must be 0 (one lineage per sample) or 1 (two: both alleles)"),
    opt("phases", &Options::phases, 1, 3, 0, "phases must be 1, 2 or 3"),
};

}  // namespace

extern "C" {

int tq_create(tq_ctx **out, int device_id)
{
    if (!out) return fail(nullptr, TQ_ERR_INVALID_ARG, "tq_create: out is NULL");
    *out = nullptr;
    return api(nullptr, "tq_create", [&]() -> int {     // no context yet: messages go to tq_last_error(NULL)
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n <= 0)
            return fail(nullptr, TQ_ERR_NO_DEVICE, "no HIP device available (%s)", hipGetErrorString(e));
        if (device_id < 0 || device_id >= n)
            return fail(nullptr, TQ_ERR_INVALID_ARG, "device_id %d out of range (0..%d)", device_id, n - 1);
        std::unique_ptr<tq_ctx> ctx(new tq_ctx());      // nothing but its buffers to release until it is handed out
        ctx->device = device_id;
        e = hipSetDevice(device_id);
        if (e == hipSuccess) e = hipGetDeviceProperties(&ctx->prop, device_id);
        if (e != hipSuccess) return fail(nullptr, TQ_ERR_HIP, "device %d not usable: %s", device_id, hipGetErrorString(e));
        if (int rc = probe_scan_pb(ctx.get())) {
            g_create_err = ctx->err;
            return rc;
        }
        *out = ctx.release();
        return TQ_OK;
    });
}

void tq_destroy(tq_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);     // every member that holds a HIP resource releases it in its destructor
    delete ctx;
}

const char *tq_last_error(const tq_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int tq_host_alloc(int64_t bytes, void **out)
{
    if (!out || bytes < 0) return TQ_ERR_INVALID_ARG;
    *out = nullptr;
    return pool().alloc((size_t)bytes, out);
}

int tq_host_free(void *p)
{
    if (!p) return TQ_OK;
    return pool().release(p);
}

// the uploads and the layout kernels of tq_set_data, after free_data; the caller frees again on a failure.  The resident
// sets leave no head-room (the packed one is built at exactly pSp); the three upload temporaries go with their scope
static int upload_data(tq_ctx *ctx, const uint8_t *tmparr, int64_t T, int64_t S, int64_t Sp, const std::vector<uint32_t> &loc,
                       const std::vector<uint32_t> &pack_src)
{
    const char *who = "tq_set_data";
    const int64_t pSp = (int64_t)pack_src.size();
    DevBuf<uint8_t> d_raw;
    DevBuf<uint32_t> d_loc, d_src;
    TQ_HIPF(ctx, who, ctx->nat.alloc(T, Sp, true));
    TQ_HIPF(ctx, who, d_raw.alloc((size_t)(T * S)));
    TQ_HIPF(ctx, who, d_loc.alloc((size_t)S));
    if (pSp) TQ_HIPF(ctx, who, ctx->pk.alloc(T, pSp, false));
    if (pSp) TQ_HIPF(ctx, who, d_src.alloc((size_t)pSp));
    ctx->nat.set_sites(Sp);
    ctx->pk.set_sites(pSp);
    auto prepare = [&](const SiteSet &s, const uint32_t *src) {
        const int64_t n = T * s.W;
        hipLaunchKernelGGL(tq_prepare_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_raw.get(), d_loc.get(), src, S,
                           s.Sp, s.W, (int32_t)T, s.rows.get(), s.nib.get(), s.nib5.get(), s.planes.get(), s.planes3.get(),
                           s.runbeg(T));
    };
    TQ_HIPF(ctx, who, hipMemcpy(d_raw, tmparr, (size_t)(T * S), hipMemcpyHostToDevice));
    TQ_HIPF(ctx, who, hipMemcpy(d_loc, loc.data(), (size_t)S * sizeof(uint32_t), hipMemcpyHostToDevice));
    prepare(ctx->nat, nullptr);
    TQ_LAUNCHED(ctx, who);
    if (pSp) {
        TQ_HIPF(ctx, who, hipMemcpy(d_src, pack_src.data(), (size_t)pSp * sizeof(uint32_t), hipMemcpyHostToDevice));
        prepare(ctx->pk, d_src);
        TQ_LAUNCHED(ctx, who);
    }
    TQ_HIPF(ctx, who, hipDeviceSynchronize());
    return TQ_OK;
}

int tq_set_data(tq_ctx *ctx, const uint8_t *tmparr, int64_t T, int64_t S, const uint32_t *locus,
                int64_t locus_stride)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_set_data", [&]() -> int {
        if (!tmparr || !locus) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_set_data: NULL pointer");
        if (T < 1 || S < 1 || locus_stride < 1 || T > 0x7FFFFFFF)
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_set_data: bad shape T=%lld S=%lld stride=%lld", (long long)T,
                        (long long)S, (long long)locus_stride);
        // a *_dev call still queued reads the replicate that goes now.  tq_set_data always frees, so for it every call is
        // the regrow path: one hipEventSynchronize per call once a *_dev call has been made, queued work or not
        TQ_HIP(ctx, regrow_wait(ctx));
        free_data(ctx);
        ctx->data_gen++;

        // contiguous copy of the locus column + the run-contiguity check: not ok means no subsample mode
        std::vector<uint32_t> loc;
        const bool ok = copy_locus_column(locus, locus_stride, S, loc);
        ctx->locus_runs_ok = ok;

        const int64_t Sp = (int64_t)align_up((size_t)S, TILE);
        // packed layout for the subsample-mode scans (pack.hpp): planned on the host, taken when forced or when it pays
        std::vector<uint32_t> pack_src;
        if (ok && ctx->opt.site_pack != 0 && S < 0xFFFFFFFFll) {        // the map holds site indices as u32
            std::vector<LocusRun> runs;
            locus_runs(loc.data(), S, runs);
            pack_sites(runs, pack_src);
            if (ctx->opt.site_pack < 0) {
                double cost[2], trips[2];
                const double gain_low = pack_estimate(tmparr, T, S, runs, pack_src, cost, trips);
                if (!pack_pays(gain_low) || !pack_fits_offsets(T, pack_src.size(), (size_t)Sp)) pack_src.clear();
            }
        }

        ctx->T = T; ctx->S = S;
        if (int rc = upload_data(ctx, tmparr, T, S, Sp, loc, pack_src)) {
            free_data(ctx);             // the context holds no half-built replicate
            return rc;
        }
        ctx->have_data = true;
        if (!pack_src.empty()) ctx->pk_gen = ctx->data_gen;
        return TQ_OK;
    });
}

int tq_pack_sites(const uint8_t *tmparr, int64_t T, int64_t S, const uint32_t *locus, int64_t locus_stride, uint32_t *src,
                  int64_t cap, int64_t *packed_sites, int32_t *pays, double *estimate)
{
    return api(nullptr, "tq_pack_sites", [&]() -> int {
        if (!locus || S < 1 || S >= 0xFFFFFFFFll || locus_stride < 1 || cap < 0 || (cap > 0 && !src) || (tmparr && T < 1))
            return TQ_ERR_INVALID_ARG;
        std::vector<uint32_t> loc;
        if (!copy_locus_column(locus, locus_stride, S, loc)) return TQ_ERR_LOCUS_ORDER;
        std::vector<LocusRun> runs;
        std::vector<uint32_t> map;
        locus_runs(loc.data(), S, runs);
        pack_sites(runs, map);
        if (packed_sites) *packed_sites = (int64_t)map.size();
        if (tmparr) {
            double cost[2], trips[2];
            const double gain_low = pack_estimate(tmparr, T, S, runs, map, cost, trips);
            if (pays) *pays = pack_pays(gain_low) ? 1 : 0;
            if (estimate) {
                estimate[0] = cost[0];
                estimate[1] = cost[1];
                estimate[2] = trips[0];
                estimate[3] = trips[1];
                estimate[4] = gain_low;
            }
        }
        if ((int64_t)map.size() <= cap) memcpy(src, map.data(), map.size() * sizeof(uint32_t));
        return TQ_OK;
    });
}

int tq_resolve_dev(tq_ctx *ctx, const uint32_t *d_quartets, int64_t Q, int subsample, uint32_t *d_rstat,
                   double *d_rscor, uint8_t *d_flags, void *stream)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_resolve_dev", [&]() -> int {
        if (Q < 0 || (Q > 0 && (!d_quartets || !d_rstat || !d_rscor)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_resolve_dev: NULL pointer or negative Q");
        OutPtrs out{d_rstat, d_rscor, d_flags, nullptr, nullptr, nullptr};
        if (int rc = enter_dev_api(ctx, (hipStream_t)stream)) return rc;
        return note_dev_api(ctx, (hipStream_t)stream,
                            launch(ctx, d_quartets, Q, subsample, false, false, out, (hipStream_t)stream, NoChunkHook()));
    });
}

int tq_scan_dev(tq_ctx *ctx, const uint32_t *d_quartets, int64_t Q, int subsample, void *stream)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_scan_dev", [&]() -> int {
        if (Q < 1 || !d_quartets) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_scan_dev: NULL pointer or Q < 1");
        if (Q > ctx->opt.batch)
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_scan_dev: Q=%lld exceeds the scan batch of %lld quartets (option 'batch')",
                        (long long)Q, (long long)ctx->opt.batch);
        int rc = check_ready(ctx, subsample);
        if (rc) return rc;
        if (ctx->timing) ctx->timed_calls++;
        if ((rc = enter_dev_api(ctx, (hipStream_t)stream))) return rc;
        return note_dev_api(ctx, (hipStream_t)stream, stage_scan(ctx, d_quartets, Q, subsample, false, (hipStream_t)stream));
    });
}

int tq_svd_dev(tq_ctx *ctx, int64_t q0, int64_t n, uint32_t *d_rstat, double *d_rscor, uint8_t *d_flags, void *stream)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_svd_dev", [&]() -> int {
        if (n < 0 || (n > 0 && (!d_rstat || !d_rscor)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_svd_dev: NULL pointer or negative n");
        if (ctx->scanned_Q == 0) return fail(ctx, TQ_ERR_NO_DATA, "tq_svd_dev: no scanned batch (call tq_scan_dev first)");
        if (n == 0) return TQ_OK;
        OutPtrs out{d_rstat, d_rscor, d_flags, nullptr, nullptr, nullptr};
        if (int rc = enter_dev_api(ctx, (hipStream_t)stream)) return rc;
        return note_dev_api(ctx, (hipStream_t)stream, stage_svd(ctx, q0, n, false, out, (hipStream_t)stream, NoChunkHook()));
    });
}

int tq_unrank_dev(tq_ctx *ctx, const uint64_t *d_ranks, int64_t Q, uint32_t *d_quartets, void *stream)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_unrank_dev", [&]() -> int {
        if (!ctx->have_data) return fail(ctx, TQ_ERR_NO_DATA, "tq_set_data has not been called");
        if (Q < 0 || (Q > 0 && (!d_ranks || !d_quartets)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_unrank_dev: NULL pointer or negative Q");
        if (!rank_space_fits(ctx->T)) return fail(ctx, TQ_ERR_INVALID_ARG, RANK_SPACE_MSG, "tq_unrank_dev", (long long)ctx->T);
        if (Q == 0) return TQ_OK;
        hipLaunchKernelGGL(tq_unrank_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           d_ranks, (uint64_t)0, Q, (int32_t)ctx->T, d_quartets);
        TQ_LAUNCHED(ctx, "tq_unrank_dev");
        return TQ_OK;
    });
}

int tq_resolve_range_dev(tq_ctx *ctx, uint64_t first_rank, int64_t Q, int subsample, uint32_t *d_quartets,
                         uint32_t *d_rstat, double *d_rscor, uint8_t *d_flags, void *stream)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_resolve_range_dev", [&]() -> int {
        if (!ctx->have_data) return fail(ctx, TQ_ERR_NO_DATA, "tq_set_data has not been called");
        if (Q < 0 || (Q > 0 && (!d_rstat || !d_rscor)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_resolve_range_dev: NULL pointer or negative Q");
        if (!rank_space_fits(ctx->T))
            return fail(ctx, TQ_ERR_INVALID_ARG, RANK_SPACE_MSG, "tq_resolve_range_dev", (long long)ctx->T);
        if (Q == 0) return TQ_OK;
        const uint64_t total = choose4((uint64_t)ctx->T);
        if (!rank_range_fits(first_rank, Q, total))
            return fail(ctx, TQ_ERR_INVALID_ARG, "rank range [%llu,+%lld) exceeds C(%lld,4)=%llu",
                        (unsigned long long)first_rank, (long long)Q, (long long)ctx->T, (unsigned long long)total);
        // before any shared scratch is touched: without d_quartets the unrank writes into d_scratch, which the scan of a
        // range call still queued on another stream reads its quartets from
        if (int rc2 = enter_dev_api(ctx, (hipStream_t)stream)) return rc2;
        uint32_t *dq = d_quartets;
        if (!dq) {
            TQ_HIP(ctx, grow_scratch(ctx, (size_t)Q * 16));
            dq = (uint32_t *)ctx->d_scratch.get();
        }
        hipLaunchKernelGGL(tq_unrank_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const uint64_t *)nullptr, first_rank, Q, (int32_t)ctx->T, dq);
        TQ_LAUNCHED(ctx, "tq_resolve_range_dev");
        OutPtrs out{d_rstat, d_rscor, d_flags, nullptr, nullptr, nullptr};
        // consecutive lexicographic ranks are in (a,b,c) order already
        return note_dev_api(ctx, (hipStream_t)stream,
                            launch(ctx, dq, Q, subsample, false, true, out, (hipStream_t)stream, NoChunkHook()));
    });
}

int tq_resolve_to_host(tq_ctx *ctx, const uint32_t *d_quartets, int64_t Q, int subsample, uint32_t *rstat,
                       double *rscor, uint8_t *flags)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_resolve_to_host", [&]() -> int {
        if (Q < 0 || (Q > 0 && (!d_quartets || !rstat || !rscor)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_resolve_to_host: NULL pointer or negative Q");
        int rc = check_ready(ctx, subsample);
        if (rc) return rc;
        if ((rc = refuse_unflagged(ctx, flags))) return rc;
        if (Q == 0) return TQ_OK;
        if ((rc = ensure_streams(ctx))) return rc;
        const size_t o_rstat = 0;
        const size_t o_rscor = align_up(o_rstat + (size_t)Q * 8, 256);
        const size_t o_flags = align_up(o_rscor + (size_t)Q * 24, 256);
        TQ_HIP(ctx, grow_scratch(ctx, align_up(o_flags + (size_t)Q, 256)));
        char *base = ctx->d_scratch;
        return resolve_to_host(ctx, d_quartets, Q, subsample, false, rstat, rscor, flags, (uint32_t *)(base + o_rstat),
                               (double *)(base + o_rscor), (uint8_t *)(base + o_flags));
    });
}

int tq_resolve_debug(tq_ctx *ctx, const uint32_t *quartets, int64_t Q, int subsample, uint32_t *rstat,
                     double *rscor, uint8_t *flags, uint32_t *cmats, double *svds, int32_t *ranks)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_resolve_debug", [&]() -> int {
        if (Q < 0 || (Q > 0 && (!quartets || !rstat || !rscor)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_resolve: NULL pointer or negative Q");
        int rc = check_ready(ctx, subsample);
        if (rc) return rc;
        if ((rc = refuse_unflagged(ctx, flags))) return rc;
        if (Q == 0) return TQ_OK;
        // Taxon indices are checked on the host (the kernels re-check and flag them, and never dereference a bad
        // one).  For chunks of the size the reference's distributor hands out the same pass notices input that
        // already is in (a,b,c) order -- its default mode's lexicographic chunks are (combinations.py:40-55) -- so
        // that the device sort (about twenty small kernels, most of the time of a chunk of a few thousand
        // quartets) is skipped.  A large batch is checked WHILE THE GPU WORKS on it (the pass over 16 B per quartet
        // costs ~1 ms per 1e6 on the host, the sort it could save 0.2 ms).
        constexpr int64_t CHECK_FIRST = 1 << 16;
        auto check_indices = [ctx, quartets, Q]() -> int {
            const uint32_t T = (uint32_t)ctx->T;
            uint32_t worst = 0;
            for (int64_t i = 0; i < 4 * Q; ++i) worst = quartets[i] > worst ? quartets[i] : worst;      // vectorises
            if (worst < T) return TQ_OK;
            for (int64_t i = 0; i < 4 * Q; ++i)
                if (quartets[i] >= T)
                    return fail(ctx, TQ_ERR_INVALID_ARG, "quartet %lld has taxon index %u >= T=%lld", (long long)(i / 4),
                                quartets[i], (long long)ctx->T);
            return TQ_OK;
        };
        bool input_sorted = false;
        if (Q <= CHECK_FIRST) {
            if ((rc = check_indices())) return rc;
            bool sorted = true;
            uint64_t prev_key = 0;
            for (int64_t i = 0; i < Q; ++i) {
                const uint32_t *q = quartets + i * 4;
                const uint64_t key = ((uint64_t)q[0] << 42) | ((uint64_t)q[1] << 21) | (uint64_t)q[2];
                sorted &= key >= prev_key;
                prev_key = key;
            }
            input_sorted = sorted && ctx->T < (1 << 21);
        }
        HostScratch h;
        if ((rc = host_scratch(ctx, quartets, Q, cmats, svds, ranks, &h))) return rc;
        if (!(cmats || svds || ranks)) {
            if (Q <= CHECK_FIRST)
                return resolve_to_host(ctx, h.dq(), Q, subsample, input_sorted, rstat, rscor, flags, h.rstat(), h.rscor(),
                                       h.flags());
            return resolve_to_host(ctx, h.dq(), Q, subsample, false, rstat, rscor, flags, h.rstat(), h.rscor(), h.flags(),
                                   check_indices);
        }
        if (Q > CHECK_FIRST && (rc = check_indices())) {
            (void)hipStreamSynchronize(ctx->sK);
            return rc;
        }
        return debug_to_host(ctx, h, Q, subsample, false, input_sorted, rstat, rscor, flags, cmats, svds, ranks);
    });
}

int tq_resolve(tq_ctx *ctx, const uint32_t *quartets, int64_t Q, int subsample, uint32_t *rstat, double *rscor,
               uint8_t *flags)
{
    return tq_resolve_debug(ctx, quartets, Q, subsample, rstat, rscor, flags, nullptr, nullptr, nullptr);
}

int tq_set_species(tq_ctx *ctx, const int32_t *species_of, int64_t T, int64_t K)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_set_species", [&]() -> int {
        if (!species_of) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_set_species: NULL pointer");
        if (K < 4 || K > 0x7FFFFFFF)
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_set_species: K=%lld species (a species quartet needs K >= 4)", (long long)K);
        const int64_t known = ctx->have_data ? ctx->T : ctx->d_seqarr ? ctx->src_T : 0;
        if (T < 1 || (known && T != known))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_set_species: T=%lld, the resident / source data have T=%lld", (long long)T,
                        (long long)known);
        std::vector<int32_t> size((size_t)K, 0), members;
        for (int64_t i = 0; i < T; ++i) {
            const int32_t k = species_of[i];
            if (k < -1 || k >= K)
                return fail(ctx, TQ_ERR_INVALID_ARG, "tq_set_species: sample %lld has species id %d outside [-1, %lld)",
                            (long long)i, k, (long long)K);
            if (k >= 0 && ++size[(size_t)k] > 255)
                return fail(ctx, TQ_ERR_INVALID_ARG, "tq_set_species: species %d has more than 255 lineages", k);
        }
        // offsets [K+1], then the members grouped by species (ascending sample index inside a species), then the
        // offsets in lineages of allele mode [K+1] (differences 2n: the per-row range rule of the pooled kernels)
        members.assign((size_t)(K + 1 + T + K + 1), 0);
        for (int64_t k = 0; k < K; ++k) {
            members[(size_t)k + 1] = members[(size_t)k] + size[(size_t)k];
            members[(size_t)(K + 1 + T + k + 1)] = 2 * members[(size_t)k + 1];
        }
        std::vector<int32_t> fill(members.begin(), members.begin() + K);
        for (int64_t i = 0; i < T; ++i)
            if (species_of[i] >= 0) members[(size_t)(K + 1 + fill[(size_t)species_of[i]]++)] = (int32_t)i;
        std::vector<int32_t> top(size);
        std::sort(top.begin(), top.end(), [](int32_t a, int32_t b) { return a > b; });
        uint64_t bound = 1;
        for (int i = 0; i < 4; ++i) bound *= (uint64_t)top[(size_t)i];
        const uint64_t bound5 = bound * (uint64_t)(K > 4 ? top[4] : 1);     // <= 255^5 < 2^40
        TQ_HIP(ctx, hipDeviceSynchronize());         // a species call may still read the old map / table
        ctx->sp_K = 0;
        TQ_HIP(ctx, ctx->d_sp_members.alloc(members.size()));
        TQ_HIP(ctx, hipMemcpy(ctx->d_sp_members, members.data(), members.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        ctx->sp_size.swap(size);
        ctx->sp_T = T;
        ctx->sp_K = K;
        ctx->sp_bound = bound;
        ctx->sp_bound5 = bound5;
        ctx->sp_max = top[0];
        ctx->sp_tab_gen = ~0ull;
        return TQ_OK;
    });
}

int tq_resolve_species_dev(tq_ctx *ctx, const uint32_t *d_squartets, int64_t Q, uint32_t *d_rstat, double *d_rscor,
                           uint8_t *d_flags, void *stream)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_resolve_species_dev", [&]() -> int {
        if (Q < 0 || (Q > 0 && (!d_squartets || !d_rstat || !d_rscor)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_resolve_species_dev: NULL pointer or negative Q");
        if (int rc = species_ready(ctx, "tq_resolve_species_dev")) return rc;
        if (Q == 0) return TQ_OK;
        if (int rc = enter_dev_api(ctx, (hipStream_t)stream)) return rc;      // before any shared scratch is touched
        OutPtrs out{d_rstat, d_rscor, d_flags, nullptr, nullptr, nullptr};
        return note_dev_api(ctx, (hipStream_t)stream,
                            launch(ctx, d_squartets, Q, 0, false, false, out, (hipStream_t)stream, NoChunkHook(), true));
    });
}

int tq_resolve_species_debug(tq_ctx *ctx, const uint32_t *squartets, int64_t Q, uint32_t *rstat, double *rscor,
                             uint8_t *flags, uint32_t *cmats, double *svds, int32_t *ranks)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_resolve_species_debug", [&]() -> int {
        if (Q < 0 || (Q > 0 && (!squartets || !rstat || !rscor)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_resolve_species: NULL pointer or negative Q");
        int rc = species_ready(ctx, "tq_resolve_species");
        if (rc) return rc;
        if ((rc = refuse_unflagged(ctx, flags))) return rc;
        if (Q == 0) return TQ_OK;
        // ids on the host (the kernels re-check them and flag the row); a row that repeats a species can exceed the
        // call's range bound, so its own product is checked when the bound leaves room for that
        const uint32_t K = (uint32_t)ctx->sp_K;
        const uint64_t lin4 = ctx->opt.species_alleles ? 16 : 1;      // lineages per sample, to the fourth
        const bool per_row = (unsigned __int128)ctx->S * ((uint64_t)ctx->sp_max * ctx->sp_max * ctx->sp_max * ctx->sp_max * lin4) >=
                             ((unsigned __int128)1 << 32);
        for (int64_t i = 0; i < Q; ++i) {
            const uint32_t *q = squartets + 4 * i;
            if ((q[0] >= K) | (q[1] >= K) | (q[2] >= K) | (q[3] >= K))
                return fail(ctx, TQ_ERR_INVALID_ARG, "species quartet %lld has a species id >= K=%u", (long long)i, K);
            if (per_row) {
                const uint64_t p = (uint64_t)ctx->sp_size[q[0]] * ctx->sp_size[q[1]] * ctx->sp_size[q[2]] * ctx->sp_size[q[3]] * lin4;
                if ((unsigned __int128)ctx->S * p >= ((unsigned __int128)1 << 32))
                    return fail(ctx, TQ_ERR_INVALID_ARG, "species quartet %lld: S=%lld x its lineage product %llu >= 2^32",
                                (long long)i, (long long)ctx->S, (unsigned long long)p);
            }
        }
        HostScratch h;
        if ((rc = host_scratch(ctx, squartets, Q, cmats, svds, ranks, &h))) return rc;
        if (!(cmats || svds || ranks)) return species_to_host(ctx, h.dq(), Q, rstat, rscor, flags, h.rstat(), h.rscor(), h.flags());
        return debug_to_host(ctx, h, Q, 0, true, false, rstat, rscor, flags, cmats, svds, ranks);
    });
}

int tq_resolve_species(tq_ctx *ctx, const uint32_t *squartets, int64_t Q, uint32_t *rstat, double *rscor, uint8_t *flags)
{
    return tq_resolve_species_debug(ctx, squartets, Q, rstat, rscor, flags, nullptr, nullptr, nullptr);
}

int tq_pattern_class_table(uint8_t *out)
{
    if (!out) return TQ_ERR_INVALID_ARG;
    for (int p = 0; p < 256; ++p) out[p] = (uint8_t)pattern_class(p >> 6, (p >> 4) & 3, (p >> 2) & 3, p & 3);
    return TQ_OK;
}

int tq_scan_plan(const int64_t *rows, int64_t n, int64_t *plans, int64_t *n_kernels)
{
    return api(nullptr, "tq_scan_plan", [&]() -> int {
        if (n < 0 || (n && (!rows || !plans))) return TQ_ERR_INVALID_ARG;
        if (n_kernels) *n_kernels = (int64_t)SCAN_TABLE.size();
        for (int64_t i = 0; i < n; ++i) {
            const int64_t *r = rows + i * 22;
            const ScanKnobs k = {(int)r[0], (int)r[1], (int)r[2], (int)r[3], (int)r[4], (int)r[5], (int)r[6], (int)r[7], (int)r[8],
                                 (int)r[9], (int)r[10], r[11], r[12], (int)r[13], (int)r[14], (int)r[15]};
            const ScanShape s = {r[16], r[17], r[18], r[19], (int)r[20], (int)r[21]};
            const ScanPlan p = choose_scan(k, s);
            const ScanKernel *kern = find_scan_kernel(p);
            const int64_t out[12] = {p.form, p.sub, p.method, p.nw, p.shc, p.park, p.nrep, p.qpw, p.threads, p.grid, p.xcd_chunk,
                                     kern ? (int64_t)(kern - SCAN_TABLE.data()) : -1};
            memcpy(plans + i * 12, out, sizeof out);
        }
        return TQ_OK;
    });
}

int tq_patterns(tq_ctx *ctx, const uint32_t *sets, int64_t Q, int subsample, uint32_t *classes)
{
    return patterns_to_host(ctx, "tq_patterns", sets, Q, subsample, false, classes);
}

int tq_patterns_dev(tq_ctx *ctx, const uint32_t *d_sets, int64_t Q, int subsample, uint32_t *d_classes, void *stream)
{
    return patterns_dev(ctx, "tq_patterns_dev", d_sets, Q, subsample, false, d_classes, (hipStream_t)stream);
}

int tq_patterns_species(tq_ctx *ctx, const uint32_t *ssets, int64_t Q, uint32_t *classes)
{
    return patterns_to_host(ctx, "tq_patterns_species", ssets, Q, 0, true, classes);
}

int tq_patterns_species_dev(tq_ctx *ctx, const uint32_t *d_ssets, int64_t Q, uint32_t *d_classes, void *stream)
{
    return patterns_dev(ctx, "tq_patterns_species_dev", d_ssets, Q, 0, true, d_classes, (hipStream_t)stream);
}

int tq_dstat_accumulate(const uint32_t *classes, int64_t n_sets, const uint32_t *set_of, const uint8_t *ia, const uint8_t *ib,
                        int64_t N, double *acc)
{
    if (int rc = check_dstat_tests(nullptr, "tq_dstat_accumulate", classes && acc, n_sets, nullptr, set_of,
                                   ClassPairTests{ia, ib}, N, true))
        return rc;
    dstat_add_host(classes, set_of, ia, ib, N, acc);
    return TQ_OK;
}

int tq_dstat_accumulate_dev(tq_ctx *ctx, const uint32_t *d_classes, int64_t n_sets, const uint32_t *d_set_of,
                            const uint8_t *d_ia, const uint8_t *d_ib, int64_t N, double *d_acc, void *stream)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_dstat_accumulate_dev", [&]() -> int {
        const char *who = "tq_dstat_accumulate_dev";
        if (int rc = check_dstat_tests(ctx, who, d_classes && d_acc, n_sets, nullptr, d_set_of, ClassPairTests{d_ia, d_ib}, N, false))
            return rc;
        return launch_per_test(ctx, who, tq_dstat_kernel, DSTAT_THREADS, N, stream, d_classes, n_sets, d_set_of, d_ia, d_ib, N, d_acc);
    });
}

int tq_patterns_blocks(tq_ctx *ctx, const uint32_t *sets, int64_t Q, const int64_t *block_starts, int64_t B, uint32_t *classes)
{
    return blocks_to_host(ctx, "tq_patterns_blocks", BLK_QUARTET, sets, Q, block_starts, B, classes);
}

int tq_patterns_blocks_dev(tq_ctx *ctx, const uint32_t *d_sets, int64_t Q, const int64_t *block_starts, int64_t B,
                           uint32_t *d_classes, void *stream)
{
    return blocks_dev(ctx, "tq_patterns_blocks_dev", BLK_QUARTET, d_sets, Q, block_starts, B, d_classes, (hipStream_t)stream);
}

int tq_patterns_blocks_species(tq_ctx *ctx, const uint32_t *ssets, int64_t Q, const int64_t *block_starts, int64_t B,
                               uint32_t *classes)
{
    return blocks_to_host(ctx, "tq_patterns_blocks_species", BLK_SPECIES, ssets, Q, block_starts, B, classes);
}

int tq_patterns_blocks_species_dev(tq_ctx *ctx, const uint32_t *d_ssets, int64_t Q, const int64_t *block_starts, int64_t B,
                                   uint32_t *d_classes, void *stream)
{
    return blocks_dev(ctx, "tq_patterns_blocks_species_dev", BLK_SPECIES, d_ssets, Q, block_starts, B, d_classes, (hipStream_t)stream);
}

int tq_pooled_site_classes(const uint32_t *packed, uint32_t *out)
{
    if (!packed || !out) return fail(nullptr, TQ_ERR_INVALID_ARG, "tq_pooled_site_classes: NULL pointer");
    uint32_t f[PAT_CLASSES] = {}, row[PAT_ROW];
    pooled_site_f(packed[0], packed[1], packed[2], packed[3], f);
    pooled_invert(f, row);
    memcpy(out, row, sizeof(row));
    return TQ_OK;
}

int tq_dstat_jackknife(const uint32_t *bclasses, int64_t n_sets, int64_t B, const uint32_t *set_of, const uint8_t *ia,
                       const uint8_t *ib, int64_t N, double *out)
{
    return jackknife_to_host("tq_dstat_jackknife", bclasses, n_sets, B, set_of, ClassPairTests{ia, ib}, N, out);
}

int tq_dstat_jackknife_dev(tq_ctx *ctx, const uint32_t *d_bclasses, int64_t n_sets, int64_t B, const uint32_t *d_set_of,
                           const uint8_t *d_ia, const uint8_t *d_ib, int64_t N, double *d_out, void *stream)
{
    return jackknife_dev(ctx, "tq_dstat_jackknife_dev", d_bclasses, n_sets, B, d_set_of, ClassPairTests{d_ia, d_ib}, N, d_out,
                         stream);
}

int tq_quintet_class_table(uint8_t *out)
{
    if (!out) return TQ_ERR_INVALID_ARG;
    for (int p = 0; p < 1024; ++p) {
        const int k = quintet_class(p >> 8, (p >> 6) & 3, (p >> 4) & 3, (p >> 2) & 3, p & 3);
        out[p] = (uint8_t)(k < 0 ? 0 : k);
    }
    return TQ_OK;
}

int tq_patterns_quintet_blocks(tq_ctx *ctx, const uint32_t *sets5, int64_t Q, const int64_t *block_starts, int64_t B,
                               uint32_t *classes)
{
    return blocks_to_host(ctx, "tq_patterns_quintet_blocks", BLK_QUINTET, sets5, Q, block_starts, B, classes);
}

int tq_patterns_quintet_blocks_dev(tq_ctx *ctx, const uint32_t *d_sets5, int64_t Q, const int64_t *block_starts, int64_t B,
                                   uint32_t *d_classes, void *stream)
{
    return blocks_dev(ctx, "tq_patterns_quintet_blocks_dev", BLK_QUINTET, d_sets5, Q, block_starts, B, d_classes,
                      (hipStream_t)stream);
}

int tq_patterns_quintet_blocks_species(tq_ctx *ctx, const uint32_t *ssets5, int64_t Q, const int64_t *block_starts, int64_t B,
                                       uint32_t *classes)
{
    return blocks_to_host(ctx, "tq_patterns_quintet_blocks_species", BLK_SPECIES_QUINTET, ssets5, Q, block_starts, B, classes);
}

int tq_patterns_quintet_blocks_species_dev(tq_ctx *ctx, const uint32_t *d_ssets5, int64_t Q, const int64_t *block_starts,
                                           int64_t B, uint32_t *d_classes, void *stream)
{
    return blocks_dev(ctx, "tq_patterns_quintet_blocks_species_dev", BLK_SPECIES_QUINTET, d_ssets5, Q, block_starts, B, d_classes,
                      (hipStream_t)stream);
}

int tq_pooled_quintet_site_classes(const uint32_t *packed, uint32_t *out)
{
    if (!packed || !out) return fail(nullptr, TQ_ERR_INVALID_ARG, "tq_pooled_quintet_site_classes: NULL pointer");
    uint32_t f[PAT_ROW] = {}, row[PAT_ROW];
    pooled5_site_f(packed[0], packed[1], packed[2], packed[3], packed[4], f);
    pooled5_finish(f, row);
    memcpy(out, row, sizeof(row));
    return TQ_OK;
}

int tq_dstat_jackknife_masks(const uint32_t *bclasses, int64_t n_sets, int64_t B, const uint32_t *set_of, const uint16_t *lmask,
                             const uint16_t *rmask, int64_t N, double *out)
{
    return jackknife_to_host("tq_dstat_jackknife_masks", bclasses, n_sets, B, set_of, MaskPairTests{lmask, rmask}, N, out);
}

int tq_dstat_jackknife_masks_dev(tq_ctx *ctx, const uint32_t *d_bclasses, int64_t n_sets, int64_t B, const uint32_t *d_set_of,
                                 const uint16_t *d_lmask, const uint16_t *d_rmask, int64_t N, double *d_out, void *stream)
{
    return jackknife_dev(ctx, "tq_dstat_jackknife_masks_dev", d_bclasses, n_sets, B, d_set_of, MaskPairTests{d_lmask, d_rmask},
                         N, d_out, stream);
}

int tq_taxon_counts(tq_ctx *ctx, const int64_t *block_starts, int64_t B, uint32_t *out)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    const char *who = "tq_taxon_counts";
    return api(ctx, who, [&]() -> int {
        if (!block_starts) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: NULL pointer", who);
        int rc = blocks_ready(ctx, who, BLK_QUARTET, block_starts, B);
        if (rc) return rc;
        if (!out) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: NULL pointer", who);
        const int64_t T = ctx->T, chunk = td_piece_blocks(T, B, ctx->opt.taxdist_scratch_bytes);
        const size_t block_bytes = (size_t)(T * T) * 16;
        TQ_HIP(ctx, grow_scratch(ctx, (size_t)chunk * block_bytes));
        if ((rc = ensure_streams(ctx))) return rc;
        uint32_t *d_rows = (uint32_t *)ctx->d_scratch.get();
        int64_t items = 0, chunks = 0;
        for (int64_t b0 = 0; b0 < B && !rc; b0 += chunk, ++chunks) {
            const int64_t b1 = std::min(B, b0 + chunk);
            rc = launch_taxon_counts(ctx, who, block_starts, b0, b1, d_rows, ctx->sK, &items);
            if (!rc && hipMemcpyAsync((char *)out + (size_t)b0 * block_bytes, d_rows, (size_t)(b1 - b0) * block_bytes,
                                      hipMemcpyDeviceToHost, ctx->sK) != hipSuccess)
                rc = fail(ctx, TQ_ERR_HIP, "%s: copy of the pair rows failed", who);
        }
        if (hipStreamSynchronize(ctx->sK) != hipSuccess && !rc) rc = fail(ctx, TQ_ERR_HIP, "%s: hipStreamSynchronize failed", who);
        if (!rc) note_taxon_counts(ctx, items, chunk, chunks);
        return rc;
    });
}

int tq_taxon_counts_dev(tq_ctx *ctx, const int64_t *block_starts, int64_t B, uint32_t *d_out, void *stream)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    const char *who = "tq_taxon_counts_dev";
    return api(ctx, who, [&]() -> int {
        if (!block_starts) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: NULL pointer", who);
        if (int rc = blocks_ready(ctx, who, BLK_QUARTET, block_starts, B)) return rc;
        if (!d_out) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: NULL pointer", who);
        if ((uintptr_t)d_out & 15) return fail(ctx, TQ_ERR_INVALID_ARG, "%s: d_out must be 16-byte aligned", who);
        if (int rc = enter_dev_api(ctx, (hipStream_t)stream)) return rc;     // behind a tq_bootstrap_async that rebuilds the layout
        const int64_t T = ctx->T, piece = td_piece_blocks(T, B, 0);
        int64_t items = 0, pieces = 0;
        int rc = TQ_OK;
        for (int64_t b0 = 0; b0 < B && !rc; b0 += piece, ++pieces)
            rc = launch_taxon_counts(ctx, who, block_starts, b0, std::min(B, b0 + piece), d_out + (size_t)b0 * (size_t)(T * T) * 4,
                                     (hipStream_t)stream, &items);
        if (!rc) note_taxon_counts(ctx, items, piece, pieces);
        return note_dev_api(ctx, (hipStream_t)stream, rc);
    });
}

int tq_taxon_counts_host(const uint8_t *tmparr, int64_t T, int64_t S, const int64_t *block_starts, int64_t B, uint32_t *out)
{
    const char *who = "tq_taxon_counts_host";
    return api(nullptr, who, [&]() -> int {
        if (!tmparr || !block_starts || !out) return fail(nullptr, TQ_ERR_INVALID_ARG, "%s: NULL pointer", who);
        if (T < 2 || S < 1) return fail(nullptr, TQ_ERR_INVALID_ARG, "%s: T=%lld, S=%lld: need T >= 2 and S >= 1", who, (long long)T, (long long)S);
        if (int rc = check_block_rule(nullptr, who, block_starts, B, S, "matrix")) return rc;
        td_host_counts(tmparr, T, S, block_starts, B, out);
        return TQ_OK;
    });
}

int tq_taxon_counts_stats(tq_ctx *ctx, int64_t *out)
{
    if (!ctx || !out) return TQ_ERR_INVALID_ARG;
    for (int i = 0; i < 5; ++i) out[i] = ctx->td_stats[i];
    return TQ_OK;
}

int tq_nj_tree(const double *dist, int64_t T, int32_t *parent, double *length)
{
    const char *who = "tq_nj_tree";
    return api(nullptr, who, [&]() -> int {
        if (!dist || !parent || !length) return fail(nullptr, TQ_ERR_INVALID_ARG, "%s: NULL pointer", who);
        if (T < 3 || T > 0x3FFFFFFF) return fail(nullptr, TQ_ERR_INVALID_ARG, "%s: T=%lld taxa, need at least 3", who, (long long)T);
        for (int64_t i = 0; i < T; ++i)
            for (int64_t j = i + 1; j < T; ++j) {
                const double a = dist[i * T + j], b = dist[j * T + i];
                if (!std::isfinite(a) || !std::isfinite(b))
                    return fail(nullptr, TQ_ERR_INVALID_ARG, "%s: the distance of the pair (%lld, %lld) is not finite", who, (long long)i,
                                (long long)j);
                if (a != b)
                    return fail(nullptr, TQ_ERR_INVALID_ARG, "%s: dist is not symmetric at the pair (%lld, %lld): %.17g against %.17g", who,
                                (long long)i, (long long)j, a, b);
            }
        nj_host_tree(dist, T, parent, length);
        return TQ_OK;
    });
}

int tq_timing_enable(tq_ctx *ctx, int on)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    ctx->timing = on != 0;
    return TQ_OK;
}

int tq_timing_read_kernels(tq_ctx *ctx, double *ms, int n_ms, int64_t *calls)
{
    if (!ctx || (n_ms > 0 && !ms)) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_timing_read_kernels", [&]() -> int {
        double t[TAG_COUNT] = {0, 0, 0, 0, 0};
        hipEvent_t prev[2] = {nullptr, nullptr};
        int rc = TQ_OK;
        ctx->event_pool.reserve(ctx->event_pool.size() + ctx->marks.size());      // all or nothing: no push_back below throws
        for (auto &m : ctx->marks) {
            if (!rc && hipEventSynchronize(m.ev) != hipSuccess) rc = fail(ctx, TQ_ERR_HIP, "timing event failed");
            if (!rc && m.tag >= 0 && m.tag < TAG_COUNT && prev[m.lane]) {
                float a = 0.f;
                if (hipEventElapsedTime(&a, prev[m.lane], m.ev) == hipSuccess) t[m.tag] += a;
            }
            prev[m.lane] = m.ev;
            ctx->event_pool.push_back(std::move(m.ev));
        }
        ctx->marks.clear();
        for (int i = 0; i < n_ms; ++i) ms[i] = i < TAG_COUNT ? t[i] : 0.0;
        if (calls) *calls = ctx->timed_calls;
        ctx->timed_calls = 0;
        return rc;
    });
}

int tq_timing_read_split(tq_ctx *ctx, double *total_ms, double *scan_ms, double *svd_ms, int64_t *calls)
{
    double t[TAG_COUNT];
    const int rc = tq_timing_read_kernels(ctx, t, TAG_COUNT, calls);
    if (rc) return rc;
    const double a = t[TAG_ORDER] + t[TAG_SCAN], b = t[TAG_BIDIAG] + t[TAG_BDSQR] + t[TAG_SCORE];
    if (total_ms) *total_ms = a + b;
    if (scan_ms) *scan_ms = a;
    if (svd_ms) *svd_ms = b;
    return TQ_OK;
}

int tq_timing_read(tq_ctx *ctx, double *kernel_ms, int64_t *launches)
{
    return tq_timing_read_split(ctx, kernel_ms, nullptr, nullptr, launches);
}

int tq_set_option(tq_ctx *ctx, const char *name, int64_t value)
{
    if (!ctx || !name) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_set_option", [&]() -> int {
        if (!strcmp(name, "bdsqr_stats")) {                  // 1: allocate + zero the counters, 0: free them
            ctx->d_bdsqr_stats.reset();
            if (value) {
                TQ_HIP(ctx, ctx->d_bdsqr_stats.alloc(8));
                TQ_HIP(ctx, hipMemset(ctx->d_bdsqr_stats, 0, 8 * sizeof(uint64_t)));
            }
            return TQ_OK;
        }
        const OptionRow *row = std::find_if(std::begin(OPTION_TABLE), std::end(OPTION_TABLE),
                                            [name](const OptionRow &r) { return !strcmp(r.name, name); });
        if (row == std::end(OPTION_TABLE)) return fail(ctx, TQ_ERR_INVALID_ARG, "unknown option '%s'", name);
        const Options defaults;
        int64_t v = value;
        if (row->flag)
            v = value != 0;
        else if (value == row->default_key && row->default_key != NO_KEY)
            v = row->i ? defaults.*row->i : defaults.*row->l;
        else if (row->listed ? value < 0 || value > 63 || !(row->listed >> value & 1) : value < row->lo || value > row->hi)
            return fail(ctx, TQ_ERR_INVALID_ARG, "%s", row->refusal);
        if (row->i == &Options::taxdist_slice_words && v % BT_KW) return fail(ctx, TQ_ERR_INVALID_ARG, "%s", row->refusal);
        if (row->l == &Options::batch && v > 0x7FFFFFFFll) v = 0x7FFFFFFFll;     // item counts reach hipCUB as int
        if (row->i == &Options::species_alleles && ctx->opt.species_alleles != (int)v)
            ctx->sp_tab_gen = ~0ull;                        // the next species call rebuilds the table
        if (row->i) ctx->opt.*row->i = (int)v;
        else ctx->opt.*row->l = v;
        return TQ_OK;
    });
}

// the uploads, staging pieces and the packing rule of tq_set_source, after free_source; the caller frees again on a failure,
// a returned code or an exception (the host copies below allocate: the recoded matrix is the largest host block of the library)
static int build_source(tq_ctx *ctx, const uint8_t *seqarr, int64_t T, int64_t S0, const int64_t *spans, int64_t nloci, int64_t maxw)
{
    TQ_HIP(ctx, ctx->d_seqarr.alloc((size_t)(T * S0)));
    TQ_HIP(ctx, ctx->d_spans.alloc((size_t)nloci * 2));
    TQ_HIP(ctx, ctx->d_lidxs.alloc((size_t)nloci));
    TQ_HIP(ctx, hipMemcpy(ctx->d_seqarr, seqarr, (size_t)(T * S0), hipMemcpyHostToDevice));
    TQ_HIP(ctx, hipMemcpy(ctx->d_spans, spans, (size_t)nloci * 16, hipMemcpyHostToDevice));
    ctx->h_spans.assign(spans, spans + 2 * nloci);
    if (int rc = ctx->lidx_ring.ensure((size_t)nloci + (size_t)(nloci + 1) / 2))       // i64 [nloci], then u32 [nloci]
        return ring_fail(ctx, rc, "tq_set_source: out of page-locked host memory");
    TQ_HIP(ctx, ctx->d_pstart.alloc((size_t)nloci));
    // the automatic rule of boot_pack = -1, once, on the source: its loci (the spans, in their order) with the bases recoded
    // as tq_set_data takes them -- a two-base IUPAC code counts as present (its first base) -- under the rule and the
    // 32-bit-offset condition of tq_set_data.  A replicate resamples these loci, so their statistics are the replicate's.
    std::vector<LocusRun> runs((size_t)nloci);
    int64_t Ssrc = 0;
    for (int64_t i = 0; i < nloci; ++i) {
        runs[(size_t)i] = {Ssrc, spans[2 * i + 1] - spans[2 * i]};
        Ssrc += runs[(size_t)i].len;
    }
    if (Ssrc < 0xFFFFFFFFll) {
        uint8_t code[256];
        memset(code, 78, sizeof code);
        for (int v = 0; v < 4; ++v) code[v] = (uint8_t)v;
        code[65] = 0; code[67] = 1; code[71] = 2; code[84] = 3;
        code[82] = 0; code[75] = 3; code[83] = 1; code[89] = 1; code[87] = 0; code[77] = 0;     // R K S Y W M
        std::vector<uint8_t> arr((size_t)(T * Ssrc));
        for (int64_t t = 0; t < T; ++t)
            for (int64_t i = 0; i < nloci; ++i)
                for (int64_t s = 0; s < runs[(size_t)i].len; ++s)
                    arr[(size_t)(t * Ssrc + runs[(size_t)i].start + s)] = code[seqarr[t * S0 + spans[2 * i] + s]];
        std::vector<uint32_t> src;
        pack_sites(runs, src);
        double cost[2], trips[2];
        const double gain_low = pack_estimate(arr.data(), T, Ssrc, runs, src, cost, trips);
        ctx->boot_pack_auto = pack_pays(gain_low) && pack_fits_offsets(T, src.size(), align_up((size_t)Ssrc, TILE));
    }
    ctx->src_T = T;
    ctx->src_S0 = S0;
    ctx->nloci = nloci;
    ctx->max_width = maxw;
    return TQ_OK;
}

int tq_set_source(tq_ctx *ctx, const uint8_t *seqarr, int64_t T, int64_t S0, const int64_t *spans, int64_t nloci)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_set_source", [&]() -> int {
        if (!seqarr || !spans) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_set_source: NULL pointer");
        if (T < 1 || S0 < 1 || nloci < 1 || T > 0x7FFFFFFF)
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_set_source: bad shape T=%lld S0=%lld nloci=%lld", (long long)T,
                        (long long)S0, (long long)nloci);
        int64_t maxw = 0;
        for (int64_t i = 0; i < nloci; ++i) {
            const int64_t a = spans[2 * i], b = spans[2 * i + 1];
            if (a < 0 || b <= a || b > S0)
                return fail(ctx, TQ_ERR_INVALID_ARG, "tq_set_source: span %lld = [%lld,%lld) outside [0,%lld)",
                            (long long)i, (long long)a, (long long)b, (long long)S0);
            if (b - a > maxw) maxw = b - a;
        }
        free_source(ctx);
        ctx->src_gen++;                     // a replicate of the earlier source is no replicate of this one
        // the context holds no half-built source, whether the build returns a code or throws into the guard
        struct Undo {
            tq_ctx *ctx;
            bool keep;
            ~Undo() { if (!keep) free_source(ctx); }
        } undo{ctx, false};
        const int rc = build_source(ctx, seqarr, T, S0, spans, nloci, maxw);
        undo.keep = rc == TQ_OK;
        return rc;
    });
}

int tq_bootstrap_async(tq_ctx *ctx, const int64_t *lidxs, int64_t n, uint64_t seed_shuffle, uint64_t seed_ambig,
                       int64_t *out_S, void *stream_)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_bootstrap_async", [&]() -> int {
        if (!ctx->d_seqarr) return fail(ctx, TQ_ERR_NO_DATA, "tq_set_source has not been called");
        if (!lidxs || n != ctx->nloci)
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_bootstrap: lidxs must hold nloci=%lld locus indices", (long long)ctx->nloci);
        hipStream_t stream = (hipStream_t)stream_;
        // replicate length on the host (jit/resample.py:7-17): no device round trip, the call stays asynchronous
        int64_t S = 0;
        for (int64_t i = 0; i < n; ++i) {
            if (lidxs[i] < 0 || lidxs[i] >= ctx->nloci)
                return fail(ctx, TQ_ERR_INVALID_ARG, "tq_bootstrap: locus index %lld out of range", (long long)lidxs[i]);
            S += ctx->h_spans[2 * lidxs[i] + 1] - ctx->h_spans[2 * lidxs[i]];
        }
        // the packed layout of the replicate, planned here at locus level (pack.hpp): the packed length is a launch argument,
        // so it has to be known at enqueue time; only the packed start of every draw goes to the device
        const bool pack = ctx->opt.site_pack != 0 && (ctx->opt.boot_pack > 0 || (ctx->opt.boot_pack < 0 && ctx->boot_pack_auto));
        int64_t pSp = 0;
        if (pack) {
            const int64_t *sp = ctx->h_spans.data();
            pSp = (int64_t)ctx->boot_plan.plan((size_t)n, [sp, lidxs](size_t i) { return sp[2 * lidxs[i] + 1] - sp[2 * lidxs[i]]; });
            if (pSp >= 0xFFFFFFFFll) pSp = 0;              // the map holds positions as u32: such a replicate keeps the natural layout
        }
        const int64_t pW = pSp / 32;
        if (int rc0 = enter_dev_api(ctx, stream)) return rc0;      // a resolve still scanning the previous replicate on another stream
        const int64_t T = ctx->src_T;
        // worst-case replicate length; buffers grow only
        const int64_t cap = n * ctx->max_width;
        if (cap > ctx->boot_cap) {
            TQ_HIP(ctx, hipDeviceSynchronize());
            ctx->d_boot.reset();
            ctx->d_boot_tmp.reset();
            ctx->boot_cap = 0;
            TQ_HIP(ctx, ctx->d_boot.alloc((size_t)(2 * (n + 1) + 2 * cap)));
            size_t tmp = 0;
            uint32_t *u = ctx->d_boot;
            TQ_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, u, u, (int)(n + 1)));
            size_t tmp2 = 0;
            TQ_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2, u, u, (int)(cap / 32 + 2)));
            if (tmp2 > tmp) tmp = tmp2;
            TQ_HIP(ctx, ctx->d_boot_tmp.alloc(tmp ? tmp : 16));
            ctx->boot_tmp_bytes = tmp;
            ctx->boot_cap = cap;
        }
        if (S < 1 || S > ctx->boot_cap) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_bootstrap: replicate length %lld", (long long)S);
        const int64_t Sp = (int64_t)align_up((size_t)S, TILE);
        const int64_t W = Sp / 32;
        SiteSet &nat = ctx->nat, &pk = ctx->pk;
        if (Sp > nat.capSp || T != ctx->T) {
            TQ_HIP(ctx, hipDeviceSynchronize());           // kernels of the previous replicate may still read the old buffers
            free_data(ctx);
            TQ_HIP(ctx, nat.alloc(T, (int64_t)align_up((size_t)(Sp + Sp / 8), TILE), true));   // head-room: replicate lengths vary
        }
        // the packed set grows only, with the same head-room; a set tq_set_data allocated serves while it is large enough
        if (pSp > pk.capSp || (size_t)pSp > ctx->d_pk_src.cap()) {
            TQ_HIP(ctx, hipDeviceSynchronize());
            const int64_t capSp = (int64_t)align_up((size_t)(pSp + pSp / 8), TILE);
            if (pSp > pk.capSp) {
                ctx->pk_gen = ~0ull;
                ctx->pk_from_boot = false;
                TQ_HIP(ctx, pk.alloc(T, capSp, false));
            }
            TQ_HIP(ctx, ctx->d_pk_src.grow((size_t)capSp));
        }
        uint32_t *widths = ctx->d_boot, *offsets = widths + (n + 1);
        uint32_t *src_col = offsets + (n + 1), *site_locus = src_col + ctx->boot_cap;
        // locus indices, and behind them the packed starts, through one piece of the staging ring: the draws of the next
        // replicate can be handed over while these copies are still queued
        int64_t *piece;
        TQ_HIP(ctx, ctx->lidx_ring.next(piece));
        memcpy(piece, lidxs, (size_t)n * 8);
        TQ_HIP(ctx, hipMemcpyAsync(ctx->d_lidxs, piece, (size_t)n * 8, hipMemcpyHostToDevice, stream));
        if (pSp) {
            uint32_t *stage = (uint32_t *)(piece + n);
            for (int64_t i = 0; i < n; ++i) stage[i] = (uint32_t)ctx->boot_plan.start[(size_t)i];
            TQ_HIP(ctx, hipMemcpyAsync(ctx->d_pstart, stage, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        }
        TQ_HIP(ctx, ctx->lidx_ring.sent(stream));
        TQ_HIP(ctx, hipMemsetAsync(widths + n, 0, sizeof(uint32_t), stream));
        hipLaunchKernelGGL(tq_boot_width_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ctx->d_spans,
                           ctx->d_lidxs, n, ctx->nloci, widths);
        size_t tmp = ctx->boot_tmp_bytes;
        TQ_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(ctx->d_boot_tmp, tmp, widths, offsets, (int)(n + 1), stream));
        hipLaunchKernelGGL(tq_boot_perm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ctx->d_spans,
                           ctx->d_lidxs, offsets, n, ctx->nloci, seed_shuffle, src_col, site_locus);
        const int64_t nw = T * W;
        hipLaunchKernelGGL(tq_boot_build_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, stream, ctx->d_seqarr,
                           ctx->src_S0, src_col, site_locus, S, Sp, W, (int32_t)T, seed_ambig, nat.rows, nat.nib, nat.nib5,
                           nat.planes, nat.planes3, nat.runbeg(T));
        TQ_LAUNCHED(ctx, "tq_bootstrap_async");
        if (pSp) {
            TQ_HIP(ctx, hipMemsetAsync(ctx->d_pk_src, 0xFF, (size_t)pSp * sizeof(uint32_t), stream));
            hipLaunchKernelGGL(tq_boot_pack_map_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, stream,
                               (const uint32_t *)offsets, (const uint32_t *)site_locus, (const uint32_t *)ctx->d_pstart, S, n, pSp,
                               ctx->d_pk_src);
            const int64_t np = T * pW;
            hipLaunchKernelGGL(tq_boot_pack_build_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, stream,
                               (const uint32_t *)ctx->d_pk_src, (const uint8_t *)nat.nib5, (const uint32_t *)nat.runbeg(T), S, Sp,
                               pSp, pW, (int32_t)T, pk.rows, pk.nib, pk.planes, pk.planes3, pk.runbeg(T));
            TQ_LAUNCHED(ctx, "tq_bootstrap_async");
        }
        ctx->T = T;
        ctx->S = S;
        nat.set_sites(Sp);
        ctx->have_data = true;
        ctx->locus_runs_ok = true;          // locus ids are the ordinals 0..n-1, one run each
        ctx->scanned_Q = 0;
        ctx->data_gen++;                    // the species table is rebuilt by the next species call
        ctx->boot_gen = ctx->data_gen;
        ctx->boot_src_gen = ctx->src_gen;
        if (pSp) {
            pk.set_sites(pSp);
            ctx->pk_gen = ctx->data_gen;
            ctx->pk_from_boot = true;
        }
        if (out_S) *out_S = S;
        return note_dev_api(ctx, stream, TQ_OK);       // the host API must not scan a half-built replicate
    });
}

int tq_bootstrap(tq_ctx *ctx, const int64_t *lidxs, int64_t n, uint64_t seed_shuffle, uint64_t seed_ambig,
                 int64_t *out_S)
{
    const int rc = tq_bootstrap_async(ctx, lidxs, n, seed_shuffle, seed_ambig, out_S, nullptr);
    if (rc) return rc;
    TQ_HIP(ctx, hipStreamSynchronize(nullptr));
    return TQ_OK;
}

int tq_sample_quartets_dev(tq_ctx *ctx, uint64_t seed, int64_t Q, uint64_t *d_ranks, uint32_t *d_quartets, void *stream)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_sample_quartets_dev", [&]() -> int {
        if (!ctx->have_data && !ctx->d_seqarr) return fail(ctx, TQ_ERR_NO_DATA, "no data on the device (T unknown)");
        if (Q < 0 || (Q > 0 && !d_quartets)) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_sample_quartets_dev: NULL pointer or negative Q");
        const uint64_t T = (uint64_t)(ctx->have_data ? ctx->T : ctx->src_T);
        if (!rank_space_fits((int64_t)T)) return fail(ctx, TQ_ERR_INVALID_ARG, RANK_SPACE_MSG, "tq_sample_quartets_dev", (long long)T);
        const uint64_t total = choose4(T);
        if ((uint64_t)Q > total)
            return fail(ctx, TQ_ERR_INVALID_ARG, "cannot draw %lld distinct quartets from C(%llu,4)=%llu", (long long)Q,
                        (unsigned long long)T, (unsigned long long)total);
        if (Q == 0) return TQ_OK;
        int half = 1;
        while (half < 32 && (1ull << (2 * half)) < total) ++half;
        hipLaunchKernelGGL(tq_sample_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, total,
                           half, Q, (int32_t)T, d_ranks, d_quartets);
        TQ_LAUNCHED(ctx, "tq_sample_quartets_dev");
        return TQ_OK;
    });
}

int tq_get_data(tq_ctx *ctx, uint8_t *tmparr, uint32_t *tmpmap)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_get_data", [&]() -> int {
        if (!ctx->have_data) return fail(ctx, TQ_ERR_NO_DATA, "no replicate on the device");
        if (!tmparr || !tmpmap) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_get_data: NULL pointer");
        TQ_HIP(ctx, hipDeviceSynchronize());     // a replicate may still be queued (tq_bootstrap_async) on any stream
        const SiteSet &nat = ctx->nat;
        const int64_t T = ctx->T, S = ctx->S, W = nat.W;
        const size_t bytes = align_up((size_t)(T * S), 256) + align_up((size_t)S * 8, 256) + align_up((size_t)(W + 1) * 8, 256);
        TQ_HIP(ctx, grow_scratch(ctx, bytes));
        uint8_t *d_arr = (uint8_t *)ctx->d_scratch.get();
        uint32_t *d_map = (uint32_t *)(ctx->d_scratch + align_up((size_t)(T * S), 256));
        uint32_t *d_cnt = (uint32_t *)((char *)d_map + align_up((size_t)S * 8, 256));
        uint32_t *d_base = d_cnt + (W + 1);
        hipLaunchKernelGGL(tq_export_kernel, dim3((unsigned)((T * S + 255) / 256)), dim3(256), 0, 0, nat.rows, nat.planes, S,
                           nat.Sp, W, (int32_t)T, d_arr, d_map);
        hipLaunchKernelGGL(tq_export_runcount_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, 0, nat.planes, W, d_cnt);
        size_t tmp = 0;
        TQ_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, d_cnt, d_base, (int)W));
        DevBuf<char> d_tmp;
        TQ_HIP(ctx, d_tmp.alloc(tmp ? tmp : 16));
        TQ_HIPF(ctx, "tq_get_data", hipcub::DeviceScan::ExclusiveSum(d_tmp.get(), tmp, d_cnt, d_base, (int)W));
        hipLaunchKernelGGL(tq_export_locus_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, 0, nat.planes,
                           (const uint32_t *)d_base, S, W, d_map);
        TQ_LAUNCHED(ctx, "tq_get_data");
        TQ_HIPF(ctx, "tq_get_data", hipMemcpy(tmparr, d_arr, (size_t)(T * S), hipMemcpyDeviceToHost));
        TQ_HIPF(ctx, "tq_get_data", hipMemcpy(tmpmap, d_map, (size_t)S * 8, hipMemcpyDeviceToHost));
        return TQ_OK;
    });
}

int tq_data_shape(tq_ctx *ctx, int64_t *T, int64_t *S)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    if (T) *T = ctx->have_data ? ctx->T : 0;
    if (S) *S = ctx->have_data ? ctx->S : 0;
    return TQ_OK;
}

int tq_debug_fetch(tq_ctx *ctx, int which, void *dst, int64_t bytes)
{
    if (!ctx || !dst || bytes < 0) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_debug_fetch", [&]() -> int {
        if (which == 4) {                       // the packed layout set: {its sites (0: none), 1 if the subsample scans read it now}
            const int64_t st[2] = {ctx->pk.Sp, ctx->pk.rows && scan_data(ctx, 1).rows == ctx->pk.rows ? 1 : 0};
            if (bytes != (int64_t)sizeof st) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_debug_fetch: which=4 takes 16 bytes");
            memcpy(dst, st, sizeof st);
            return TQ_OK;
        }
        if (which == 6) {                       // the most recent scan launch: {kernel form, T * pitch of the set it read, packed}
            const int64_t st[3] = {ctx->last_scan_form, ctx->last_scan_tpitch, ctx->last_scan_packed};
            if (bytes != (int64_t)sizeof st) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_debug_fetch: which=6 takes 24 bytes");
            memcpy(dst, st, sizeof st);
            return TQ_OK;
        }
        if (which == 5) {                       // the map of the current replicate's packed set (option boot_pack)
            if (!ctx->pk_from_boot || !ctx->pk.rows || ctx->pk_gen != ctx->data_gen)
                return fail(ctx, TQ_ERR_INVALID_ARG, "tq_debug_fetch: which=5 needs a current packed set built by tq_bootstrap");
            if (bytes != ctx->pk.Sp * (int64_t)sizeof(uint32_t))
                return fail(ctx, TQ_ERR_INVALID_ARG, "tq_debug_fetch: which=5 takes %lld bytes", (long long)(ctx->pk.Sp * 4));
            TQ_HIP(ctx, hipDeviceSynchronize());
            TQ_HIP(ctx, hipMemcpy(dst, ctx->d_pk_src, (size_t)bytes, hipMemcpyDeviceToHost));
            return TQ_OK;
        }
        const void *src = which == 0 ? (const void *)ctx->d_cm.get() : which == 1 ? (const void *)ctx->d_de.get()
                          : which == 2 ? (const void *)ctx->d_sv.get() : which == 3 ? (const void *)ctx->d_bdsqr_stats.get() : nullptr;
        if (!src) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_debug_fetch: nothing to fetch (which=%d)", which);
        TQ_HIP(ctx, hipDeviceSynchronize());
        TQ_HIP(ctx, hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
        return TQ_OK;
    });
}

int tq_debug_bdsqr(tq_ctx *ctx, const double *de, int64_t nmat, double *sv, uint32_t *work, int reps, double *ms)
{
    if (!ctx || !de || nmat < 1 || reps < 1) return TQ_ERR_INVALID_ARG;
    return api(ctx, "tq_debug_bdsqr", [&]() -> int {
        DevBuf<double> d_de, d_sv;      // locals: every exit frees them
        DevBuf<uint32_t> d_work;
        Event e0, e1;
        int rc = TQ_OK;
        auto step = [&](hipError_t e, const char *what) {
            if (!rc && e != hipSuccess) rc = fail(ctx, e == hipErrorOutOfMemory ? TQ_ERR_OOM : TQ_ERR_HIP, "tq_debug_bdsqr: %s: %s", what, hipGetErrorString(e));
        };
        step(d_de.alloc((size_t)nmat * 32), "hipMalloc");
        if (!rc) step(d_sv.alloc((size_t)nmat * 16), "hipMalloc");
        if (!rc) step(d_work.alloc((size_t)nmat), "hipMalloc");
        if (!rc) step(hipMemcpy(d_de, de, (size_t)nmat * 256, hipMemcpyHostToDevice), "H2D");
        if (!rc) step(e0.create(true), "event");
        if (!rc) step(e1.create(true), "event");
        const unsigned grid = (unsigned)((nmat + WAVE - 1) / WAVE);
        if (!rc) {
            // The launch is judged by the thread's last error, and that is sticky: an error that another user of the HIP
            // runtime in this thread left unread (a finaliser run by the host language, say) is not this launch's.  Every
            // call above was judged by its own return value, so whatever is pending here is foreign: read it away.
            (void)hipGetLastError();
            // once with the per-matrix counters (slower), then `reps` timed launches of the product form
            hipLaunchKernelGGL(tq_bdsqr_kernel, dim3(grid), dim3(WAVE), 0, 0, (const double *)d_de, nmat, d_sv.get(), ctx->opt.bdsqr_maxit,
                               (unsigned long long *)nullptr, d_work.get());
            step(hipGetLastError(), "launch");
            if (!rc) step(hipEventRecord(e0, 0), "record");
            for (int i = 0; i < reps && !rc; ++i)
                hipLaunchKernelGGL(tq_bdsqr_kernel, dim3(grid), dim3(WAVE), 0, 0, (const double *)d_de, nmat, d_sv.get(), ctx->opt.bdsqr_maxit,
                                   (unsigned long long *)nullptr, (uint32_t *)nullptr);
            if (!rc) step(hipEventRecord(e1, 0), "record");
            if (!rc) step(hipEventSynchronize(e1), "sync");
            float t = 0.f;
            if (!rc) step(hipEventElapsedTime(&t, e0, e1), "elapsed");
            if (ms) *ms = (double)t / reps;
        }
        if (!rc && sv) step(hipMemcpy(sv, d_sv, (size_t)nmat * 128, hipMemcpyDeviceToHost), "D2H");
        if (!rc && work) step(hipMemcpy(work, d_work, (size_t)nmat * 4, hipMemcpyDeviceToHost), "D2H");
        return rc;
    });
}

int tq_format_tsv(const uint32_t *quartets, const uint32_t *rstat, const double *rscor, int64_t Q, char *out,
                  int64_t cap, int64_t *written)
{
    if (Q < 0 || cap < 0 || !written || (Q > 0 && (!quartets || !rstat || !rscor || !out))) return TQ_ERR_INVALID_ARG;
    const int64_t n = format_tsv(quartets, rstat, rscor, Q, out, cap);
    *written = n < 0 ? -n : n;
    return n < 0 ? TQ_ERR_OOM : TQ_OK;
}

int tq_format_qmc(const uint32_t *quartets, const uint32_t *rstat, const double *rscor, int64_t Q, int weights,
                  int64_t min_snps, double min_ratio, char *out, int64_t cap, int64_t *written, int64_t *n_lines)
{
    if (Q < 0 || cap < 0 || !written || weights < 0 || weights > 3 ||
        (Q > 0 && (!quartets || !rstat || !rscor || !out)))
        return TQ_ERR_INVALID_ARG;
    const int64_t n = format_qmc(quartets, rstat, rscor, Q, weights, min_snps, min_ratio, out, cap, n_lines);
    *written = n < 0 ? -n : n;
    return n < 0 ? TQ_ERR_OOM : TQ_OK;
}

int tq_qmc_splits(const uint32_t *quartets, const uint32_t *rstat, const double *rscor, int64_t Q, int weights,
                  int64_t min_snps, double min_ratio, uint32_t *splits, double *wout, int64_t *n_rows)
{
    if (Q < 0 || !n_rows || weights < 0 || weights > 3 || (Q > 0 && (!quartets || !rstat || !rscor || !splits || !wout)))
        return TQ_ERR_INVALID_ARG;
    *n_rows = qmc_splits(quartets, rstat, rscor, Q, weights, min_snps, min_ratio, splits, wout);
    return TQ_OK;
}

int tq_numpy_choice_tail(void *np_bitgen, uint64_t pop, int64_t size, int64_t *out)
{
    if (!np_bitgen || !out || size < 1 || (uint64_t)size > pop || pop < 2 || pop > 0xFFFFFFFEull) return TQ_ERR_INVALID_ARG;
    return numpy_choice_tail((NpBitgen *)np_bitgen, pop, size, out);
}

int tq_unrank(const uint64_t *ranks, uint64_t first_rank, int64_t Q, int64_t T, uint32_t *quartets)
{
    if (Q < 0 || T < 4 || (Q > 0 && !quartets))
        return fail(nullptr, TQ_ERR_INVALID_ARG, "tq_unrank: NULL pointer, negative Q or fewer than 4 taxa");
    if (!rank_space_fits(T)) return fail(nullptr, TQ_ERR_INVALID_ARG, RANK_SPACE_MSG, "tq_unrank", (long long)T);
    const uint64_t total = choose4((uint64_t)T);
    if (ranks) {
        for (int64_t i = 0; i < Q; ++i)
            if (ranks[i] >= total)
                return fail(nullptr, TQ_ERR_INVALID_ARG, "tq_unrank: rank %lld: %llu is not below C(%lld,4) = %llu", (long long)i,
                            (unsigned long long)ranks[i], (long long)T, (unsigned long long)total);
    } else if (!rank_range_fits(first_rank, Q, total)) {
        return fail(nullptr, TQ_ERR_INVALID_ARG, "tq_unrank: rank range [%llu,+%lld) exceeds C(%lld,4) = %llu",
                    (unsigned long long)first_rank, (long long)Q, (long long)T, (unsigned long long)total);
    }
    unrank_host(ranks, first_rank, Q, (int32_t)T, quartets);
    return TQ_OK;
}

int tq_qmc_tree(const uint32_t *splits, const double *weights, int64_t n, int64_t ntaxa, uint64_t seed, char *out,
                int64_t cap, int64_t *written)
{
    return api(nullptr, "tq_qmc_tree", [&]() -> int {
        if (n < 0 || cap < 0 || !written || ntaxa < 1 || ntaxa > (1 << 24) || (n > 0 && !splits) || (cap > 0 && !out))
            return TQ_ERR_INVALID_ARG;
        *written = 0;                   // what a failure leaves
        std::string nwk;
        const int rc = qmc_tree(splits, weights, n, ntaxa, seed, nwk);
        if (rc) return rc;
        *written = (int64_t)nwk.size();
        if ((int64_t)nwk.size() > cap) return TQ_ERR_OOM;
        memcpy(out, nwk.data(), nwk.size());
        return TQ_OK;
    });
}

int tq_conc_create(tq_conc **out, const int32_t *parent, int64_t n_nodes, int64_t T, int64_t min_snps, double min_ratio,
                   tq_ctx *ctx)
{
    if (!out) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_conc_create: out is NULL");
    *out = nullptr;
    return api(ctx, "tq_conc_create", [&]() -> int {
        if (!parent) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_conc_create: parent is NULL");
        if (std::isnan(min_ratio)) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_conc_create: min_ratio is NaN");
        std::unique_ptr<tq_conc> acc(new tq_conc());
        acc->min_snps = (uint32_t)std::min<int64_t>(std::max<int64_t>(1, min_snps), 0xFFFFFFFFll);   // deviation 2
        acc->min_ratio = min_ratio;
        if (int rc = tree_acc_init(acc.get(), "tq_conc_create", parent, n_nodes, T, CONC_EDGE_WORDS, 2 * T + 1, ctx)) return rc;
        acc->hf.assign(acc->words, 0.0);
        *out = acc.release();
        return TQ_OK;
    });
}

void tq_conc_destroy(tq_conc *acc) { delete acc; }

int tq_conc_reset(tq_conc *acc)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_conc_reset", [&]() -> int {
        std::fill(acc->hf.begin(), acc->hf.end(), 0.0);
        return tree_acc_reset(acc);
    });
}

int tq_conc_add(tq_conc *acc, const uint32_t *quartets, const uint32_t *rstat, const double *rscor, const uint8_t *flags,
                int64_t n)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_conc_add", [&]() -> int {
        if (n < 0 || (n > 0 && (!quartets || !rstat || !rscor)))
            return fail(acc->ctx, TQ_ERR_INVALID_ARG, "tq_conc_add: NULL pointer or negative n");
        conc_add_host(acc->t, acc->min_snps, acc->min_ratio, quartets, rstat, rscor, flags, n, acc->hi, acc->hf);
        return TQ_OK;
    });
}

int tq_conc_add_dev(tq_conc *acc, const uint32_t *d_quartets, const uint32_t *d_rstat, const double *d_rscor,
                    const uint8_t *d_flags, int64_t n, void *stream)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    tq_ctx *ctx = acc->ctx;
    return api(ctx, "tq_conc_add_dev", [&]() -> int {
        if (!ctx) return fail(nullptr, TQ_ERR_INVALID_ARG, "tq_conc_add_dev: the accumulator was created without a context");
        if (n < 0 || (n > 0 && (!d_quartets || !d_rstat || !d_rscor)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_conc_add_dev: NULL pointer or negative n");
        if (n == 0) return TQ_OK;
        hipStream_t st = (hipStream_t)stream;
        return tree_acc_add_dev(acc, "tq_conc_add_dev", n, acc->t.E, st,
                                [=](int form, int G, int64_t r0, int64_t m, int32_t e_lo, int32_t e_n, int first) {
            const ConcTree &t = acc->t;
            const ConcArgs a{d_quartets + 4 * r0, d_rstat + 2 * r0, d_rscor + 3 * r0, d_flags ? d_flags + r0 : nullptr, m,
                             acc->d_lca, acc->d_dep, acc->d_eid, t.T, t.N, t.E, acc->min_snps, acc->min_ratio, e_lo, e_n, first,
                             acc->d_slab, acc->words};
            if (form == 0)
                hipLaunchKernelGGL((tq_conc_kernel<true, CONC_T_LDS_A, CONC_T_LDS_A>), dim3(G), dim3(CONC_THREADS), 0, st, a);
            else if (form == 1)
                hipLaunchKernelGGL((tq_conc_kernel<true, CONC_T_LDS_B, CONC_T_LDS_B>), dim3(G), dim3(CONC_THREADS), 0, st, a);
            else
                hipLaunchKernelGGL((tq_conc_kernel<false, CONC_T_MAX, CONC_EDGE_TILE>), dim3(G), dim3(CONC_THREADS), 0, st, a);
        });
    });
}

int tq_conc_shape(const tq_conc *acc, int64_t *T, int64_t *n_edges, int64_t *mask_words)
{
    return tree_acc_shape(acc, T, n_edges, mask_words);
}

int tq_conc_read(tq_conc *acc, int64_t *edge_counts, double *edge_sums, uint64_t *masks, int64_t *tip_counts,
                 int64_t *skipped)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_conc_read", [&]() -> int {
        const ConcTree &t = acc->t;
        std::vector<uint64_t> dv;
        if (int rc = tree_acc_read(acc, "tq_conc_read", dv)) return rc;
        for (int32_t e = 0; e < t.E; ++e) {
            const uint64_t *d = &dv[(size_t)e * CONC_EDGE_WORDS];
            const uint64_t *h = &acc->hi[(size_t)e * CONC_EDGE_WORDS];
            if (edge_counts) {
                int64_t *o = edge_counts + 6 * (int64_t)e;
                o[0] = (int64_t)t.nqrts[e];
                for (int k = 0; k < 5; ++k) o[1 + k] = (int64_t)(d[k] + h[k]);
            }
            if (edge_sums)
                for (int k = 0; k < 2; ++k) {
                    double dvf;
                    memcpy(&dvf, &d[CW_WEIGHT + k], 8);
                    edge_sums[2 * (int64_t)e + k] = dvf + acc->hf[(size_t)e * CONC_EDGE_WORDS + CW_WEIGHT + k];
                }
        }
        if (masks) memcpy(masks, t.masks.data(), t.masks.size() * 8);
        const int64_t tb = (int64_t)t.E * CONC_EDGE_WORDS;
        if (tip_counts)
            for (int64_t i = 0; i < 2 * (int64_t)t.T; ++i) tip_counts[i] = (int64_t)(dv[tb + i] + acc->hi[tb + i]);
        if (skipped) *skipped = (int64_t)(dv[tb + 2 * t.T] + acc->hi[tb + 2 * t.T]);
        return TQ_OK;
    });
}

int tq_scf_create(tq_scf **out, const int32_t *parent, int64_t n_nodes, int64_t T, tq_ctx *ctx)
{
    if (!out) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_scf_create: out is NULL");
    *out = nullptr;
    return api(ctx, "tq_scf_create", [&]() -> int {
        if (!parent) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_scf_create: parent is NULL");
        std::unique_ptr<tq_scf> acc(new tq_scf());
        if (int rc = tree_acc_init(acc.get(), "tq_scf_create", parent, n_nodes, T, SCF_EDGE_WORDS, 1, ctx)) return rc;
        *out = acc.release();
        return TQ_OK;
    });
}

void tq_scf_destroy(tq_scf *acc) { delete acc; }

int tq_scf_reset(tq_scf *acc)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_scf_reset", [&]() -> int { return tree_acc_reset(acc); });
}

int tq_scf_add(tq_scf *acc, const uint32_t *sets, const uint32_t *classes, int64_t n)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_scf_add", [&]() -> int {
        if (n < 0 || (n > 0 && (!sets || !classes)))
            return fail(acc->ctx, TQ_ERR_INVALID_ARG, "tq_scf_add: NULL pointer or negative n");
        scf_add_host(acc->t, sets, classes, n, acc->hi);
        return TQ_OK;
    });
}

int tq_scf_add_dev(tq_scf *acc, const uint32_t *d_sets, const uint32_t *d_classes, int64_t n, void *stream)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    tq_ctx *ctx = acc->ctx;
    return api(ctx, "tq_scf_add_dev", [&]() -> int {
        if (!ctx) return fail(nullptr, TQ_ERR_INVALID_ARG, "tq_scf_add_dev: the accumulator was created without a context");
        if (n < 0 || (n > 0 && (!d_sets || !d_classes)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_scf_add_dev: NULL pointer or negative n");
        if (n == 0) return TQ_OK;
        if ((((uintptr_t)d_sets) | ((uintptr_t)d_classes)) & 15)     // sets are read as 16-byte words
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_scf_add_dev: d_sets and d_classes must be 16-byte aligned");
        hipStream_t st = (hipStream_t)stream;
        return tree_acc_add_dev(acc, "tq_scf_add_dev", n, 0, st,
                                [=](int form, int G, int64_t r0, int64_t m, int32_t e_lo, int32_t e_n, int first) {
            const ConcTree &t = acc->t;
            const ScfArgs a{d_sets + 4 * r0, d_classes + 16 * r0, m, acc->d_lca, acc->d_dep, acc->d_eid, t.T, t.N, t.E, e_lo, e_n,
                            first, acc->d_slab, acc->words};
            if (form == 0)
                hipLaunchKernelGGL((tq_scf_kernel<true, SCF_T_LDS_A, SCF_T_LDS_A>), dim3(G), dim3(CONC_THREADS), 0, st, a);
            else if (form == 1)
                hipLaunchKernelGGL((tq_scf_kernel<true, SCF_T_LDS_B, SCF_T_LDS_B>), dim3(G), dim3(CONC_THREADS), 0, st, a);
            else
                hipLaunchKernelGGL((tq_scf_kernel<false, CONC_T_MAX, SCF_EDGE_TILE>), dim3(G), dim3(CONC_THREADS), 0, st, a);
        });
    });
}

int tq_scf_shape(const tq_scf *acc, int64_t *T, int64_t *n_edges, int64_t *mask_words)
{
    return tree_acc_shape(acc, T, n_edges, mask_words);
}

int tq_scf_read(tq_scf *acc, int64_t *edge_counts, uint64_t *masks, int64_t *skipped)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_scf_read", [&]() -> int {
        const ConcTree &t = acc->t;
        std::vector<uint64_t> dv;
        if (int rc = tree_acc_read(acc, "tq_scf_read", dv)) return rc;
        const int64_t eb = (int64_t)t.E * SCF_EDGE_WORDS;
        if (edge_counts)
            for (int64_t i = 0; i < eb; ++i) edge_counts[i] = (int64_t)(dv[i] + acc->hi[i]);
        if (masks) memcpy(masks, t.masks.data(), t.masks.size() * 8);
        if (skipped) *skipped = (int64_t)(dv[eb] + acc->hi[eb]);
        return TQ_OK;
    });
}

int tq_stree_create(tq_stree **out, int64_t ntaxa, int64_t capacity_rows, int weights, int64_t min_snps, double min_ratio,
                    tq_ctx *ctx)
{
    const char *who = "tq_stree_create";
    if (!out) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_create: out is NULL");
    *out = nullptr;
    return api(ctx, who, [&]() -> int {
        if (ntaxa < 1 || ntaxa > 65535) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_create: ntaxa must be 1..65535");
        if (ctx && (ntaxa < 4 || ntaxa > STREE_T_MAX))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_create: the device path takes 4 <= ntaxa <= %d", STREE_T_MAX);
        if (capacity_rows < 0 || capacity_rows >= (int64_t(1) << 31))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_create: capacity_rows must be 0..2^31-1");
        if (weights < 0 || weights > 3) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_create: no weight strategy %d", weights);
        if (std::isnan(min_ratio)) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_create: min_ratio is NaN");
        std::unique_ptr<tq_stree> acc(new tq_stree());
        acc->ctx = ctx;
        acc->ntaxa = ntaxa;
        acc->capacity = capacity_rows;
        acc->weights = weights;
        acc->min_snps = (uint32_t)std::min<int64_t>(std::max<int64_t>(1, min_snps), 0xFFFFFFFFll);
        acc->min_ratio = min_ratio;
        if (ctx) {
            acc->num_cu = std::max(1, ctx->prop.multiProcessorCount);
            acc->max_nodes = 3 * ntaxa;                                  // the taxa of a level number fewer than 3 ntaxa
            acc->max_cells = 3 * ntaxa * ntaxa / 2 + 16;                 // sum of n (n - 1) / 2 with n <= ntaxa, sum of n < 3 ntaxa
            const size_t rows = (size_t)std::max<int64_t>(1, capacity_rows);
            const size_t cells = (size_t)acc->max_cells, nodes = (size_t)acc->max_nodes;
            TQ_HIPF(ctx, who, acc->d_root_t.alloc(rows));
            TQ_HIPF(ctx, who, acc->d_root_k.alloc(rows));
            for (int b = 0; b < 2; ++b) {
                TQ_HIPF(ctx, who, acc->d_wt[b].alloc(rows));
                TQ_HIPF(ctx, who, acc->d_wk[b].alloc(rows));
                TQ_HIPF(ctx, who, acc->d_wn[b].alloc(rows));
            }
            TQ_HIPF(ctx, who, acc->d_cnt.alloc(SC_WORDS));
            TQ_HIPF(ctx, who, acc->d_mat.alloc(cells * 2));
            TQ_HIPF(ctx, who, acc->d_nodes.alloc(nodes));
            TQ_HIPF(ctx, who, acc->d_map.alloc(nodes * 3));
            TQ_HIPF(ctx, who, acc->p_mat.alloc(cells * 2));
            TQ_HIPF(ctx, who, acc->p_nodes.alloc(nodes));
            TQ_HIPF(ctx, who, acc->p_map.alloc(nodes * 3));
            TQ_HIPF(ctx, who, acc->p_cnt.alloc(SC_WORDS));
            TQ_HIPF(ctx, who, acc->d_side.alloc(nodes * 3));
            TQ_HIPF(ctx, who, acc->d_cut.alloc(nodes));
            TQ_HIPF(ctx, who, acc->p_side.alloc(nodes * 3));
            TQ_HIPF(ctx, who, acc->p_cut.alloc(nodes));
            TQ_HIPF(ctx, who, hipMemset(acc->d_cnt, 0, SC_WORDS * 8));
            TQ_HIPF(ctx, who, acc->order.create());
            TQ_HIPF(ctx, who, acc->own.create());
        }
        *out = acc.release();
        return TQ_OK;
    });
}

void tq_stree_destroy(tq_stree *acc) { delete acc; }

int tq_stree_reset(tq_stree *acc)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_stree_reset", [&]() -> int {
        acc->h_t.clear();
        acc->h_k.clear();
        acc->h_skipped = 0;
        acc->h_sum = 0;
        acc->rows_in = 0;
        acc->mode = 0;
        if (acc->ctx) {
            TQ_HIP(acc->ctx, acc->order.sync());
            TQ_HIP(acc->ctx, hipMemsetAsync(acc->d_cnt, 0, SC_WORDS * 8, acc->own));   // not the null stream: it would wait
            TQ_HIP(acc->ctx, hipStreamSynchronize(acc->own));                           // for every other stream's work
        }
        return TQ_OK;
    });
}

int tq_stree_add(tq_stree *acc, const uint32_t *quartets, const uint32_t *rstat, const double *rscor, const uint8_t *flags,
                 int64_t n)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_stree_add", [&]() -> int {
        if (n < 0 || (n > 0 && (!quartets || !rstat || !rscor)))
            return fail(acc->ctx, TQ_ERR_INVALID_ARG, "tq_stree_add: NULL pointer or negative n");
        if (acc->mode == 2) return fail(acc->ctx, TQ_ERR_INVALID_ARG, "tq_stree_add: device rows were added; host rows do not mix");
        if (acc->rows_in + n > acc->capacity)
            return fail(acc->ctx, TQ_ERR_INVALID_ARG, "tq_stree_add: %lld rows added, %lld more exceed the capacity of %lld",
                        (long long)acc->rows_in, (long long)n, (long long)acc->capacity);
        if (n == 0) return TQ_OK;
        acc->h_t.reserve(acc->h_t.size() + (size_t)n);
        acc->h_k.reserve(acc->h_k.size() + (size_t)n);
        acc->mode = 1;
        acc->rows_in += n;
        for (int64_t i = 0; i < n; ++i) {
            const uint32_t *q = quartets + 4 * i;
            uint32_t sp[4];
            uint64_t k;
            if (!stree_row((uint32_t)acc->ntaxa, acc->weights, acc->min_snps, acc->min_ratio, q[0], q[1], q[2], q[3], rstat[2 * i],
                           rstat[2 * i + 1], rscor[3 * i], rscor[3 * i + 1], rscor[3 * i + 2], flags ? flags[i] : 0u, sp, k)) {
                ++acc->h_skipped;
                continue;
            }
            acc->h_t.push_back((uint64_t)sp[0] | (uint64_t)sp[1] << 16 | (uint64_t)sp[2] << 32 | (uint64_t)sp[3] << 48);
            acc->h_k.push_back(k);
            acc->h_sum += k;
        }
        return TQ_OK;
    });
}

int tq_stree_add_dev(tq_stree *acc, const uint32_t *d_quartets, const uint32_t *d_rstat, const double *d_rscor,
                     const uint8_t *d_flags, int64_t n, void *stream)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    tq_ctx *ctx = acc->ctx;
    return api(ctx, "tq_stree_add_dev", [&]() -> int {
        if (!ctx) return fail(nullptr, TQ_ERR_INVALID_ARG, "tq_stree_add_dev: the accumulator was created without a context");
        if (n < 0 || (n > 0 && (!d_quartets || !d_rstat || !d_rscor)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_add_dev: NULL pointer or negative n");
        if (acc->mode == 1) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_add_dev: host rows were added; device rows do not mix");
        if (acc->rows_in + n > acc->capacity)
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_add_dev: %lld rows added, %lld more exceed the capacity of %lld",
                        (long long)acc->rows_in, (long long)n, (long long)acc->capacity);
        if (n == 0) return TQ_OK;
        hipStream_t st = (hipStream_t)stream;
        if (int rc = stree_join(acc, st)) return rc;                    // appends in call order
        StreeAddArgs a{d_quartets, d_rstat, d_rscor, d_flags, n, (uint32_t)acc->ntaxa, acc->min_snps, acc->weights,
                       acc->min_ratio, acc->d_root_t, acc->d_root_k, acc->capacity, acc->d_cnt};
        hipLaunchKernelGGL(tq_stree_rows_kernel, dim3((unsigned)((n + STREE_THREADS - 1) / STREE_THREADS)), dim3(STREE_THREADS), 0,
                           st, a);
        TQ_LAUNCHED(ctx, "tq_stree_add_dev");
        TQ_HIP(ctx, acc->order.mark(st));
        acc->mode = 2;
        acc->rows_in += n;
        return TQ_OK;
    });
}

int tq_stree_graph(tq_stree *acc, uint64_t *G, uint64_t *B, int64_t *kept, int64_t *skipped, uint64_t *sum_k)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_stree_graph", [&]() -> int {
        int64_t nk = 0, ns = 0;
        unsigned __int128 sum = 0;
        if (int rc = stree_counts(acc, acc->own, nk, ns, sum)) return rc;
        if (kept) *kept = nk;
        if (skipped) *skipped = ns;
        if (sum_k) *sum_k = (sum >> 64) ? ~0ull : (uint64_t)sum;
        if (!G && !B) return TQ_OK;
        if (sum >> 63) return fail(acc->ctx, TQ_ERR_INVALID_ARG, "tq_stree_graph: the sum of k exceeds 2^63, a cell could wrap");
        const int64_t T = acc->ntaxa;
        if (G) memset(G, 0, (size_t)T * T * 8);
        if (B) memset(B, 0, (size_t)T * T * 8);
        if (T < 4 || nk == 0) return TQ_OK;
        std::vector<StreeNode> nodes(1);
        nodes[0].n = (int32_t)T;
        nodes[0].childA = nodes[0].childB = -1;
        const int64_t cells = T * (T - 1) / 2;
        const uint64_t *mat = nullptr;
        std::string err;
        StreeHostBackend hb;
        StreeDevBackend db;
        int64_t live = 0;
        int rc;
        if (acc->mode == 2) {
            db.a = acc;
            db.st = acc->own;
            rc = db.begin(live, err);
            if (!rc) rc = db.graphs(nodes, cells, 0, mat, err);
        } else {
            hb.root_t = &acc->h_t;
            hb.root_k = &acc->h_k;
            rc = hb.begin(live, err);
            if (!rc) rc = hb.graphs(nodes, cells, 0, mat, err);
        }
        if (rc) return fail(acc->ctx, rc, "tq_stree_graph: %s", err.c_str());
        int64_t c = 0;
        for (int64_t u = 0; u < T; ++u)
            for (int64_t v = u + 1; v < T; ++v, ++c) {
                if (G) G[u * T + v] = G[v * T + u] = mat[c];
                if (B) B[u * T + v] = B[v * T + u] = mat[cells + c];
            }
        return TQ_OK;
    });
}

int tq_stree_rows(tq_stree *acc, uint32_t *splits, uint64_t *k, int64_t *n)
{
    if (!acc || !n) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_stree_rows", [&]() -> int {
        int64_t nk = 0, ns = 0;
        unsigned __int128 sum = 0;
        if (int rc = stree_counts(acc, acc->own, nk, ns, sum)) return rc;
        *n = nk;
        if (nk == 0 || (!splits && !k)) return TQ_OK;
        const uint64_t *t4 = acc->h_t.data(), *kk = acc->h_k.data();
        std::vector<uint64_t> tmp;
        if (acc->mode == 2) {
            tmp.resize((size_t)nk * 2);
            TQ_HIP(acc->ctx, hipMemcpyAsync(tmp.data(), acc->d_root_t, (size_t)nk * 8, hipMemcpyDeviceToHost, acc->own));
            TQ_HIP(acc->ctx, hipMemcpyAsync(tmp.data() + nk, acc->d_root_k, (size_t)nk * 8, hipMemcpyDeviceToHost, acc->own));
            TQ_HIP(acc->ctx, hipStreamSynchronize(acc->own));
            t4 = tmp.data();
            kk = tmp.data() + nk;
        }
        for (int64_t i = 0; i < nk; ++i) {
            if (splits)
                for (int j = 0; j < 4; ++j) splits[4 * i + j] = (uint32_t)((t4[i] >> (16 * j)) & 0xFFFF);
            if (k) k[i] = kk[i];
        }
        return TQ_OK;
    });
}

int tq_stree_build(tq_stree *acc, uint64_t seed, void *stream, char *out, int64_t cap, int64_t *written, int64_t *levels)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_stree_build", [&]() -> int {
        if (cap < 0 || !written || (cap > 0 && !out))
            return fail(acc->ctx, TQ_ERR_INVALID_ARG, "tq_stree_build: NULL pointer or negative cap");
        *written = 0;
        int64_t nk = 0, ns = 0;
        unsigned __int128 sum = 0;
        if (int rc = stree_counts(acc, (hipStream_t)stream, nk, ns, sum)) return rc;
        if (sum >= STREE_SUM_LIMIT)
            return fail(acc->ctx, TQ_ERR_INVALID_ARG,
                        "tq_stree_build: 6 x the sum of the integer weights reaches 2^53 (sum of k >= %llu): the graph would "
                        "not be exact in doubles", (unsigned long long)STREE_SUM_LIMIT);
        std::string nwk, err;
        int64_t lv = 0;
        int rc;
        if (acc->mode == 2) {
            StreeDevBackend db;
            db.a = acc;
            db.st = (hipStream_t)stream;
            db.exact = acc->search == 1;
            rc = stree_build(db, acc->ntaxa, seed, nwk, lv, acc->stats, err);
        } else {
            StreeHostBackend hb;
            hb.root_t = &acc->h_t;
            hb.root_k = &acc->h_k;
            hb.exact = acc->search == 1;
            rc = stree_build(hb, acc->ntaxa, seed, nwk, lv, acc->stats, err);
        }
        if (rc) return fail(acc->ctx, rc, "tq_stree_build: %s", err.c_str());
        if (levels) *levels = lv;
        *written = (int64_t)nwk.size();
        if ((int64_t)nwk.size() > cap) return TQ_ERR_OOM;
        memcpy(out, nwk.data(), nwk.size());
        return TQ_OK;
    });
}

int tq_stree_set_search(tq_stree *acc, int search)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    if (search != 0 && search != 1)
        return fail(acc->ctx, TQ_ERR_INVALID_ARG, "tq_stree_set_search: no search rule %d (0 = f64, 1 = exact)", search);
    acc->search = search;
    return TQ_OK;
}

int tq_stree_fit(tq_stree *acc, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride, void *stream,
                 uint64_t *out)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    tq_ctx *ctx = acc->ctx;
    return api(ctx, "tq_stree_fit", [&]() -> int {
        if (R < 0 || stride < 0 || (R > 0 && (!parents || !n_nodes || !out)))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_fit: NULL pointer or negative size");
        if (R == 0) return TQ_OK;
        const int64_t T = acc->ntaxa;
        std::vector<std::vector<int32_t>> pars;
        if (int rc = prepare_fit_trees(ctx, "tq_stree_fit", parents, n_nodes, R, stride, T, pars)) return rc;
        const char *wide = "tq_stree_fit: the sum of k does not fit in 64 bits";
        if (acc->mode != 2) {                                       // host rows, or none yet
            if (acc->h_sum >> 64) return fail(ctx, TQ_ERR_INVALID_ARG, "%s", wide);
            std::vector<uint16_t> D((size_t)T * T);
            std::vector<uint32_t> dep;
            std::vector<uint64_t> res((size_t)R * FIT_WORDS);
            for (int64_t r = 0; r < R; ++r) {
                fit_host_table(pars[(size_t)r], (uint32_t)T, dep, D.data());
                fit_host_rows(D.data(), (uint32_t)T, acc->h_t.data(), acc->h_k.data(), (int64_t)acc->h_t.size(),
                              &res[(size_t)r * FIT_WORDS]);
            }
            memcpy(out, res.data(), res.size() * 8);
            return TQ_OK;
        }
        hipStream_t st = (hipStream_t)stream;
        if (int rc = stree_join(acc, st)) return rc;                // behind the adds made on other streams
        const int64_t S = 2 * T;
        if (!acc->fit_bytes) acc->fit_bytes = ctx->opt.fit_scratch_bytes;
        const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(acc->fit_bytes / (2 * T * T), FIT_MAX_CHUNK_TREES));
        const int64_t tab_trees = std::min(R, chunk);
        if (R > acc->fit_trees) {                                   // no fit is in flight: each one ends with a synchronisation
            acc->fit_trees = 0;
            const size_t rec = (size_t)R * S, res = (size_t)R * FIT_WORDS + SC_WORDS;
            TQ_HIP(ctx, acc->d_fit_rec.alloc(rec));
            TQ_HIP(ctx, acc->d_fit_out.alloc(res));
            TQ_HIP(ctx, acc->p_fit_rec.alloc(rec));
            TQ_HIP(ctx, acc->p_fit_out.alloc(res));
            acc->fit_trees = R;
        }
        TQ_HIP(ctx, acc->d_fit_tab.grow((size_t)tab_trees * T * T));
        fit_stage_records(acc->p_fit_rec, pars, S);
        TQ_HIP(ctx, hipMemcpyAsync(acc->d_fit_rec, acc->p_fit_rec, (size_t)R * S * 4, hipMemcpyHostToDevice, st));
        TQ_HIP(ctx, hipMemsetAsync(acc->d_fit_out, 0, (size_t)R * FIT_WORDS * 8, st));
        const unsigned table_blocks = fit_table_blocks(T);
        const unsigned slices = (unsigned)std::max<int64_t>(
            1, std::min<int64_t>((acc->rows_in + FIT_ROWS_PER_BLOCK - 1) / FIT_ROWS_PER_BLOCK, FIT_MAX_SLICES));
        for (int64_t r0 = 0; r0 < R; r0 += chunk) {                 // the next chunk's tables follow this chunk's fit on `st`
            const unsigned n = (unsigned)std::min<int64_t>(chunk, R - r0);
            FitTableArgs ta{acc->d_fit_rec + r0 * S, acc->d_fit_tab, (uint32_t)T};
            hipLaunchKernelGGL(tq_fit_table_kernel, dim3(table_blocks, n), dim3(FIT_THREADS), 0, st, ta);
            TQ_LAUNCHED(ctx, "tq_stree_fit");
            if (acc->rows_in == 0) continue;
            FitArgs fa{acc->d_root_t, acc->d_root_k, &acc->d_cnt[SC_KEPT], acc->d_fit_tab, acc->d_fit_out + r0 * FIT_WORDS,
                       (uint32_t)T};
            if (T <= FIT_T_LDS) hipLaunchKernelGGL(tq_fit_kernel<true>, dim3(slices, n), dim3(FIT_THREADS), 0, st, fa);
            else hipLaunchKernelGGL(tq_fit_kernel<false>, dim3(slices, n), dim3(FIT_THREADS), 0, st, fa);
            TQ_LAUNCHED(ctx, "tq_stree_fit");
        }
        unsigned long long *cnt = acc->p_fit_out + R * FIT_WORDS;
        TQ_HIP(ctx, hipMemcpyAsync(acc->p_fit_out, acc->d_fit_out, (size_t)R * FIT_WORDS * 8, hipMemcpyDeviceToHost, st));
        TQ_HIP(ctx, hipMemcpyAsync(cnt, acc->d_cnt, SC_WORDS * 8, hipMemcpyDeviceToHost, st));
        TQ_HIP(ctx, hipStreamSynchronize(st));
        const unsigned __int128 sum = (unsigned __int128)cnt[SC_SUM_LO] + ((unsigned __int128)cnt[SC_SUM_HI] << 32);
        if (sum >> 64) return fail(ctx, TQ_ERR_INVALID_ARG, "%s", wide);
        memcpy(out, acc->p_fit_out, (size_t)R * FIT_WORDS * 8);
        return TQ_OK;
    });
}

int tq_stree_nni_scan(tq_stree *acc, const int32_t *parent, int64_t n_nodes, void *stream, int64_t *n_edges,
                      uint8_t *eligible, uint64_t *corners, uint64_t *w)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    tq_ctx *ctx = acc->ctx;
    return api(ctx, "tq_stree_nni_scan", [&]() -> int {
        if (!parent || n_nodes < 0) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_nni_scan: NULL pointer or negative size");
        NniTree t;
        const std::string err = nni_prepare(parent, n_nodes, acc->ntaxa, t);    // validated before anything is written
        if (!err.empty()) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_nni_scan: tree 0: %s", err.c_str());
        std::vector<uint64_t> sums;
        if (int rc = nni_scan_once(acc, t, (hipStream_t)stream, "tq_stree_nni_scan", sums)) return rc;
        if (n_edges) *n_edges = t.E;
        if (eligible && t.E) memcpy(eligible, t.elig.data(), (size_t)t.E);
        if (corners) nni_corner_masks(t, corners);
        if (w && t.E) memcpy(w, sums.data(), (size_t)t.E * 3 * 8);
        return TQ_OK;
    });
}

int tq_stree_polish(tq_stree *acc, const int32_t *parent, int64_t n_nodes, int64_t max_rounds, void *stream, char *out,
                    int64_t cap, int64_t *written, uint64_t *trace, int64_t *rounds, int *converged)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    tq_ctx *ctx = acc->ctx;
    return api(ctx, "tq_stree_polish", [&]() -> int {
        if (!parent || n_nodes < 0 || cap < 0 || !written || (cap > 0 && !out))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_polish: NULL pointer or negative size");
        if (max_rounds < 0 || max_rounds > NNI_MAX_ROUNDS)
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_polish: max_rounds must be 0..%lld", (long long)NNI_MAX_ROUNDS);
        NniTree t;
        const std::string err = nni_prepare(parent, n_nodes, acc->ntaxa, t);    // validated before anything is written
        if (!err.empty()) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_polish: tree 0: %s", err.c_str());
        std::vector<uint64_t> sums, tr;
        int conv = 0;
        for (int64_t r = 0; r < max_rounds; ++r) {
            if (int rc = nni_scan_once(acc, t, (hipStream_t)stream, "tq_stree_polish", sums)) return rc;
            uint64_t gain = 0;
            const int64_t moves = nni_round(t, sums, gain);
            if (!moves) {
                conv = 1;
                break;
            }
            tr.push_back((uint64_t)moves);
            tr.push_back(gain);
        }
        const std::string nwk = nni_newick(t);
        *written = (int64_t)nwk.size();
        if ((int64_t)nwk.size() > cap) return TQ_ERR_OOM;
        memcpy(out, nwk.data(), nwk.size());
        if (trace && !tr.empty()) memcpy(trace, tr.data(), tr.size() * 8);
        if (rounds) *rounds = (int64_t)(tr.size() / 2);
        if (converged) *converged = conv;
        return TQ_OK;
    });
}

int tq_stree_search(tq_ctx *ctx, int64_t n_nodes, const int32_t *sizes, const uint64_t *G, const uint64_t *B,
                    const uint64_t *node_seeds, uint8_t *side, uint8_t *cut, int32_t *rounds)
{
    return api(ctx, "tq_stree_search", [&]() -> int {
        if (n_nodes < 1 || n_nodes > (int64_t(1) << 20) || !sizes || !G || !B || !node_seeds || !side || !cut)
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_search: NULL pointer or n_nodes not in 1..2^20");
        std::vector<StreeNode> nodes((size_t)n_nodes);
        uint64_t cells = 0, moff = 0;
        for (int64_t i = 0; i < n_nodes; ++i) {
            const int64_t n = sizes[i];
            if (n < 4 || n > (ctx ? STREE_T_MAX : 65535))
                return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_search: node %lld has %lld taxa, outside 4..%d", (long long)i,
                            (long long)n, ctx ? STREE_T_MAX : 65535);
            nodes[(size_t)i].toff = (uint32_t)cells;
            nodes[(size_t)i].moff = (uint32_t)moff;
            nodes[(size_t)i].n = (int32_t)n;
            nodes[(size_t)i].childA = nodes[(size_t)i].childB = -1;
            cells += (uint64_t)n * (uint64_t)(n - 1) / 2;
            moff += (uint64_t)n;
            if (cells > 0xFFFFFFFFull) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_stree_search: more than 2^32 cells");
        }
        if (!ctx) {
            for (int64_t i = 0; i < n_nodes; ++i) {
                const StreeNode &nd = nodes[(size_t)i];
                int r = 0;
                cut[i] = stree_search_exact(G + nd.toff, B + nd.toff, nd.n, node_seeds[i], side + nd.moff, r) ? 1 : 0;
                if (!cut[i]) memset(side + nd.moff, 0, (size_t)nd.n);
                if (rounds) rounds[i] = r;
            }
            return TQ_OK;
        }
        DevBuf<unsigned long long> d_mat;                           // locals: every exit frees them
        DevBuf<StreeNode> d_nodes;
        DevBuf<uint64_t> d_seeds;
        DevBuf<uint8_t> d_out;                                      // side bytes, cut bytes, round bytes
        std::vector<uint8_t> out((size_t)moff + 2 * (size_t)n_nodes);
        const char *who = "tq_stree_search";
        TQ_HIPF(ctx, who, d_mat.alloc((size_t)cells * 2));
        TQ_HIPF(ctx, who, d_nodes.alloc((size_t)n_nodes));
        TQ_HIPF(ctx, who, d_seeds.alloc((size_t)n_nodes));
        TQ_HIPF(ctx, who, d_out.alloc(out.size()));
        TQ_HIPF(ctx, who, hipMemcpy(d_mat, G, (size_t)cells * 8, hipMemcpyHostToDevice));
        TQ_HIPF(ctx, who, hipMemcpy(d_mat + cells, B, (size_t)cells * 8, hipMemcpyHostToDevice));
        TQ_HIPF(ctx, who, hipMemcpy(d_nodes, nodes.data(), (size_t)n_nodes * sizeof(StreeNode), hipMemcpyHostToDevice));
        TQ_HIPF(ctx, who, hipMemcpy(d_seeds, node_seeds, (size_t)n_nodes * 8, hipMemcpyHostToDevice));
        TQ_HIPF(ctx, who, hipMemset(d_out, 0, out.size()));
        StreeSearchArgs p{};
        p.nodes = d_nodes;
        p.n_nodes = (int32_t)n_nodes;
        p.cells = (int64_t)cells;
        p.mat = d_mat;
        p.seeds = d_seeds;
        p.side = d_out;
        p.cut = d_out + moff;
        p.rounds = d_out + moff + n_nodes;
        hipLaunchKernelGGL(tq_stree_search_kernel, dim3((unsigned)n_nodes), dim3(STREE_SEARCH_THREADS), 0, 0, p);
        TQ_LAUNCHED(ctx, who);
        TQ_HIPF(ctx, who, hipDeviceSynchronize());
        TQ_HIPF(ctx, who, hipMemcpy(out.data(), d_out, out.size(), hipMemcpyDeviceToHost));
        memcpy(side, out.data(), (size_t)moff);
        memcpy(cut, out.data() + moff, (size_t)n_nodes);
        if (rounds)
            for (int64_t i = 0; i < n_nodes; ++i) rounds[i] = out[(size_t)moff + (size_t)n_nodes + (size_t)i];
        return TQ_OK;
    });
}

int tq_stree_level_stats(const tq_stree *acc, int64_t *n_levels, double *out)
{
    if (!acc || !n_levels) return TQ_ERR_INVALID_ARG;
    *n_levels = (int64_t)acc->stats.size();
    if (out)
        for (size_t i = 0; i < acc->stats.size(); ++i) {
            const StreeLevelStat &s = acc->stats[i];
            double *o = out + 6 * i;
            o[0] = (double)s.nodes; o[1] = (double)s.live; o[2] = (double)s.cells;
            o[3] = s.graph_ms; o[4] = s.search_ms; o[5] = s.part_ms;
        }
    return TQ_OK;
}

int tq_cons_create(tq_cons **out, int64_t T, int64_t max_splits, tq_ctx *ctx)
{
    const char *who = "tq_cons_create";
    if (!out) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_cons_create: out is NULL");
    *out = nullptr;
    return api(ctx, who, [&]() -> int {
        if (T < 4 || T > CONS_T_MAX) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_cons_create: T must be 4..%d", CONS_T_MAX);
        if (max_splits < 1 || max_splits > (int64_t(1) << 26))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_cons_create: max_splits must be 1..2^26");
        std::unique_ptr<tq_cons> a(new tq_cons());
        a->ctx = ctx;
        a->chunk.shape(T);
        a->table.max_splits = max_splits;
        if (ctx) {
            const int64_t nodes = a->chunk.nodes();
            TQ_HIPF(ctx, who, a->chunk.alloc(ctx->opt.cons_scratch_bytes, nodes * 4));        // the unresolved items
            TQ_HIPF(ctx, who, a->table.alloc(ctx, a->chunk.W, a->chunk.chunk_trees * nodes));
            TQ_HIPF(ctx, who, a->chunk.alloc_host());
            TQ_HIPF(ctx, who, a->table.alloc_host());
            TQ_HIPF(ctx, who, a->order.create());
            if (int rc = a->table.clear(ctx)) return rc;
        }
        *out = a.release();
        return TQ_OK;
    });
}

void tq_cons_destroy(tq_cons *acc) { delete acc; }

int tq_cons_reset(tq_cons *acc)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_cons_reset", [&]() -> int {
        if (acc->ctx) {
            TQ_HIP(acc->ctx, acc->order.sync());
            if (int rc = acc->table.clear(acc->ctx)) return rc;
        }
        acc->table.forget(acc->ctx);
        acc->ntrees = 0;
        acc->chunk.chunks = 0;
        acc->table_ok = false;
        return TQ_OK;
    });
}

int tq_cons_add(tq_cons *acc, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride, void *stream)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    tq_ctx *ctx = acc->ctx;
    return api(ctx, "tq_cons_add", [&]() -> int {
        SplitTable &t = acc->table;
        const int32_t T = acc->chunk.T, W = acc->chunk.W;
        if (int rc = tree_set_args(ctx, "tq_cons_add", parents, n_nodes, R, stride)) return rc;
        if (t.overflow) return t.overflowed(ctx, "tq_cons_add");
        if (R == 0) return TQ_OK;
        const int64_t S = cons_stride(T);
        std::vector<int32_t> recs;
        if (int rc = prepare_trees(ctx, "tq_cons_add", parents, n_nodes, R, stride, T, recs)) return rc;
        acc->table_ok = false;
        acc->ntrees += R;
        if (!ctx) {
            std::vector<uint64_t> tmp, sides, m((size_t)W);
            for (int64_t r = 0; r < R; ++r) {
                sides.clear();
                cons_host_splits(&recs[(size_t)r * S], T, W, tmp, sides);
                for (size_t e = 0; e < sides.size(); e += W) {
                    m.assign(sides.begin() + e, sides.begin() + e + W);
                    auto it = t.host.find(m);
                    if (it != t.host.end()) { ++it->second; continue; }
                    if ((int64_t)t.host.size() >= t.max_splits) return t.overflowed(ctx, "tq_cons_add");
                    t.host.emplace(m, 1);
                }
            }
            return TQ_OK;
        }
        for (int64_t r0 = 0; r0 < R; r0 += acc->chunk.chunk_trees) {
            const int64_t n = std::min<int64_t>(acc->chunk.chunk_trees, R - r0);
            if (int rc = cons_drain(acc)) return rc;        // the staging buffer and the mask scratch are free again
            if (int rc = cons_launch(acc, n, &recs[(size_t)r0 * S], (hipStream_t)stream)) return rc;
        }
        return TQ_OK;
    });
}

int tq_cons_shape(tq_cons *acc, int64_t *T, int64_t *W, int64_t *ntrees, int64_t *nsplits)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    if (T) *T = acc->chunk.T;
    if (W) *W = acc->chunk.W;
    if (ntrees) *ntrees = acc->ntrees;
    if (!nsplits) return TQ_OK;                 // scalars only: nothing to guard
    return api(acc->ctx, "tq_cons_shape", [&]() -> int {
        if (int rc = cons_table(acc, "tq_cons_shape")) return rc;
        *nsplits = (int64_t)acc->tcounts.size();
        return TQ_OK;
    });
}

int tq_cons_read(tq_cons *acc, uint64_t *masks, int64_t *counts)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_cons_read", [&]() -> int {
        if (int rc = cons_table(acc, "tq_cons_read")) return rc;
        if (masks && !acc->tmasks.empty()) memcpy(masks, acc->tmasks.data(), acc->tmasks.size() * 8);
        if (counts && !acc->tcounts.empty()) memcpy(counts, acc->tcounts.data(), acc->tcounts.size() * 8);
        return TQ_OK;
    });
}

int tq_cons_tree(tq_cons *acc, int64_t min_count, char *out, int64_t cap, int64_t *written)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_cons_tree", [&]() -> int {
        if (cap < 0 || !written || (cap > 0 && !out))
            return fail(acc->ctx, TQ_ERR_INVALID_ARG, "tq_cons_tree: NULL pointer or negative cap");
        *written = 0;
        if (min_count < 1) return fail(acc->ctx, TQ_ERR_INVALID_ARG, "tq_cons_tree: min_count must be at least 1");
        if (int rc = cons_table(acc, "tq_cons_tree")) return rc;
        const std::string nwk = cons_newick(acc->tmasks, acc->tcounts, acc->chunk.T, acc->chunk.W, acc->ntrees, min_count);
        *written = (int64_t)nwk.size();
        if ((int64_t)nwk.size() > cap) return TQ_ERR_OOM;
        memcpy(out, nwk.data(), nwk.size());
        return TQ_OK;
    });
}

int tq_cons_support(tq_cons *acc, const int32_t *parent, int64_t n_nodes, int64_t *counts_out, uint64_t *masks_out,
                    int64_t *n_edges)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_cons_support", [&]() -> int {
        if (!parent || !n_edges) return fail(acc->ctx, TQ_ERR_INVALID_ARG, "tq_cons_support: NULL pointer");
        *n_edges = 0;
        const int32_t T = acc->chunk.T, W = acc->chunk.W;
        std::vector<int32_t> rec((size_t)cons_stride(T));
        const std::string err = cons_prepare(parent, n_nodes, T, rec.data());
        if (!err.empty()) return fail(acc->ctx, TQ_ERR_INVALID_ARG, "tq_cons_support: %s", err.c_str());
        if (int rc = cons_table(acc, "tq_cons_support")) return rc;
        std::vector<uint64_t> tmp, sides;
        cons_host_splits(rec.data(), T, W, tmp, sides);
        const int64_t E = (int64_t)(sides.size() / W);
        std::vector<int64_t> order(E);
        for (int64_t e = 0; e < E; ++e) order[e] = e;
        std::sort(order.begin(), order.end(),
                  [&](int64_t x, int64_t y) { return cons_mask_less(&sides[x * W], &sides[y * W], W); });
        ConsMap seen;                               // the table by mask
        std::vector<uint64_t> m((size_t)W);
        for (size_t i = 0; i < acc->tcounts.size(); ++i) {
            m.assign(acc->tmasks.begin() + i * W, acc->tmasks.begin() + (i + 1) * W);
            seen.emplace(m, acc->tcounts[i]);
        }
        for (int64_t e = 0; e < E; ++e) {
            const uint64_t *src = &sides[order[e] * W];
            m.assign(src, src + W);
            const auto it = seen.find(m);
            if (counts_out) counts_out[e] = it == seen.end() ? 0 : it->second;
            if (masks_out) memcpy(masks_out + e * W, src, (size_t)W * 8);
        }
        *n_edges = E;
        return TQ_OK;
    });
}

int tq_cons_stats(tq_cons *acc, int64_t *out)
{
    if (!acc || !out) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_cons_stats", [&]() -> int {
        if (acc->ctx && !acc->table.overflow)
            if (int rc = cons_drain(acc)) return rc;
        out[0] = acc->chunk.chunk_trees;
        out[1] = acc->chunk.chunks;
        out[2] = acc->table.dev_entries;
        out[3] = (int64_t)acc->table.host.size();
        out[4] = acc->table.unresolved;
        out[5] = acc->table.hash_bits;
        return TQ_OK;
    });
}

int tq_tbe_create(tq_tbe **out, int64_t T, const int32_t *ref_parent, int64_t n_nodes, tq_ctx *ctx)
{
    const char *who = "tq_tbe_create";
    if (!out) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_tbe_create: out is NULL");
    *out = nullptr;
    return api(ctx, who, [&]() -> int {
        if (T < 4 || T > CONS_T_MAX) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_tbe_create: T must be 4..%d", CONS_T_MAX);
        if (!ref_parent) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_tbe_create: ref_parent is NULL");
        std::vector<int32_t> rec((size_t)cons_stride(T));
        const std::string err = cons_prepare(ref_parent, n_nodes, T, rec.data());
        if (!err.empty()) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_tbe_create: %s", err.c_str());
        std::unique_ptr<tq_tbe> a(new tq_tbe());
        a->ctx = ctx;
        a->chunk.shape(T);
        tbe_reference(rec.data(), a->chunk.T, a->chunk.W, a->masks, a->p);
        a->E = (int64_t)a->p.size();
        a->phi_sum.assign((size_t)a->E, 0);
        if (ctx) {
            const int64_t W = a->chunk.W, E1 = std::max<int64_t>(1, a->E);
            TQ_HIPF(ctx, who, a->chunk.alloc(ctx->opt.cons_scratch_bytes, E1 * 2));       // the phi row
            const int64_t C = a->chunk.chunk_trees;
            TQ_HIPF(ctx, who, a->d_phi.alloc((size_t)C * E1));
            TQ_HIPF(ctx, who, a->d_ref.alloc((size_t)E1 * W));
            TQ_HIPF(ctx, who, a->d_p.alloc((size_t)E1));
            TQ_HIPF(ctx, who, a->d_phi_sum.alloc((size_t)E1));
            TQ_HIPF(ctx, who, a->chunk.alloc_host());
            TQ_HIPF(ctx, who, a->p_phi.alloc((size_t)C * E1));
            TQ_HIPF(ctx, who, a->order.create());
            if (a->E) TQ_HIPF(ctx, who, hipMemcpy(a->d_ref, a->masks.data(), (size_t)a->E * W * 8, hipMemcpyHostToDevice));
            if (a->E) TQ_HIPF(ctx, who, hipMemcpy(a->d_p, a->p.data(), (size_t)a->E * 4, hipMemcpyHostToDevice));
            TQ_HIPF(ctx, who, hipMemset(a->d_phi_sum, 0, (size_t)E1 * 8));
            TQ_HIPF(ctx, who, hipDeviceSynchronize());
        }
        *out = a.release();
        return TQ_OK;
    });
}

void tq_tbe_destroy(tq_tbe *acc) { delete acc; }

int tq_tbe_reset(tq_tbe *acc)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_tbe_reset", [&]() -> int {
        if (acc->ctx) {
            TQ_HIP(acc->ctx, acc->order.sync());
            TQ_HIP(acc->ctx, hipMemset(acc->d_phi_sum, 0, (size_t)std::max<int64_t>(1, acc->E) * 8));
            TQ_HIP(acc->ctx, hipDeviceSynchronize());
        }
        std::fill(acc->phi_sum.begin(), acc->phi_sum.end(), uint64_t(0));
        acc->ntrees = 0;
        acc->chunk.chunks = 0;
        return TQ_OK;
    });
}

int tq_tbe_add(tq_tbe *acc, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride, void *stream,
               uint16_t *phi_out)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    tq_ctx *ctx = acc->ctx;
    return api(ctx, "tq_tbe_add", [&]() -> int {
        const int32_t T = acc->chunk.T, W = acc->chunk.W;
        if (int rc = tree_set_args(ctx, "tq_tbe_add", parents, n_nodes, R, stride)) return rc;
        if (R == 0) return TQ_OK;
        const int64_t S = cons_stride(T), E = acc->E;
        std::vector<int32_t> recs;
        if (int rc = prepare_trees(ctx, "tq_tbe_add", parents, n_nodes, R, stride, T, recs)) return rc;
        acc->ntrees += R;
        if (E == 0) return TQ_OK;                       // a star reference: nothing to measure
        if (!ctx) {
            std::vector<uint64_t> tmp, sides;
            std::vector<uint32_t> phi((size_t)E);
            for (int64_t r = 0; r < R; ++r) {
                tbe_host_tree(&recs[(size_t)r * S], T, W, acc->masks, acc->p, tmp, sides, phi.data());
                for (int64_t e = 0; e < E; ++e) {
                    acc->phi_sum[e] += phi[e];
                    if (phi_out) phi_out[r * E + e] = (uint16_t)phi[e];
                }
            }
            return TQ_OK;
        }
        for (int64_t r0 = 0; r0 < R; r0 += acc->chunk.chunk_trees) {
            const int64_t n = std::min<int64_t>(acc->chunk.chunk_trees, R - r0);
            TQ_HIP(ctx, acc->order.sync());             // the staging buffer and the mask scratch are free again
            if (int rc = tbe_launch(acc, n, &recs[(size_t)r0 * S], (hipStream_t)stream, phi_out != nullptr)) return rc;
            if (phi_out) {
                TQ_HIP(ctx, acc->order.sync());
                memcpy(phi_out + r0 * E, acc->p_phi, (size_t)n * E * 2);
            }
        }
        return TQ_OK;
    });
}

int tq_tbe_shape(tq_tbe *acc, int64_t *T, int64_t *W, int64_t *E, int64_t *ntrees)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    if (T) *T = acc->chunk.T;
    if (W) *W = acc->chunk.W;
    if (E) *E = acc->E;
    if (ntrees) *ntrees = acc->ntrees;
    return TQ_OK;
}

int tq_tbe_read(tq_tbe *acc, uint64_t *masks, int64_t *p, uint64_t *phi_sum)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_tbe_read", [&]() -> int {
        const int64_t E = acc->E;
        if (acc->ctx) {
            TQ_HIP(acc->ctx, acc->order.sync());
            if (phi_sum && E) TQ_HIP(acc->ctx, hipMemcpy(phi_sum, acc->d_phi_sum, (size_t)E * 8, hipMemcpyDeviceToHost));
        } else if (phi_sum && E) {
            memcpy(phi_sum, acc->phi_sum.data(), (size_t)E * 8);
        }
        if (masks && E) memcpy(masks, acc->masks.data(), (size_t)E * acc->chunk.W * 8);
        if (p)
            for (int64_t e = 0; e < E; ++e) p[e] = acc->p[e];
        return TQ_OK;
    });
}

int tq_tbe_stats(tq_tbe *acc, int64_t *out)
{
    if (!acc || !out) return TQ_ERR_INVALID_ARG;
    out[0] = acc->chunk.chunk_trees;
    out[1] = acc->chunk.chunks;
    return TQ_OK;
}

int tq_rf_create(tq_rf **out, int64_t T, int64_t max_trees, int64_t max_splits, tq_ctx *ctx)
{
    const char *who = "tq_rf_create";
    if (!out) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_rf_create: out is NULL");
    *out = nullptr;
    return api(ctx, who, [&]() -> int {
        if (T < 4 || T > CONS_T_MAX) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_rf_create: T must be 4..%d", CONS_T_MAX);
        if (max_trees < 1 || max_trees > RF_MAX_TREES)
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_rf_create: max_trees must be 1..%lld", (long long)RF_MAX_TREES);
        if (max_splits < 1 || max_splits > (int64_t(1) << 26))
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_rf_create: max_splits must be 1..2^26");
        std::unique_ptr<tq_rf> a(new tq_rf());
        a->ctx = ctx;
        a->chunk.shape(T);
        a->max_trees = max_trees;
        a->table.max_splits = max_splits;
        if (ctx) {
            const int64_t nodes = a->chunk.nodes();
            // a column is a split of at least two trees
            const int64_t max_cols = std::max<int64_t>(1, std::min<int64_t>(max_splits, max_trees * (T - 3) / 2));
            a->cw_chunk = std::max<int64_t>(1, std::min<int64_t>((max_cols + 63) / 64, ctx->opt.cons_scratch_bytes / (max_trees * 8)));
            // beside a tree's masks: its unresolved items and their ids, device and page-locked
            TQ_HIPF(ctx, who, a->chunk.alloc(ctx->opt.cons_scratch_bytes, nodes * 4 * 3, max_trees));
            const int64_t items = a->chunk.chunk_trees * nodes;
            TQ_HIPF(ctx, who, a->table.alloc(ctx, a->chunk.W, items));
            TQ_HIPF(ctx, who, a->d_newid.alloc((size_t)items));
            TQ_HIPF(ctx, who, a->d_colmap.alloc((size_t)max_splits));
            TQ_HIPF(ctx, who, a->d_ids.alloc((size_t)max_trees * nodes));
            TQ_HIPF(ctx, who, a->d_nsplits.alloc((size_t)max_trees));
            TQ_HIPF(ctx, who, a->d_bits.alloc((size_t)max_trees * a->cw_chunk));
            TQ_HIPF(ctx, who, a->d_shared.alloc((size_t)max_trees * max_trees));
            TQ_HIPF(ctx, who, a->d_rf.alloc((size_t)max_trees * max_trees));
            TQ_HIPF(ctx, who, a->chunk.alloc_host());
            TQ_HIPF(ctx, who, a->table.alloc_host());
            TQ_HIPF(ctx, who, a->p_newid.alloc((size_t)items));
            TQ_HIPF(ctx, who, a->order.create());
            if (int rc = rf_clear_dev(a.get())) return rc;
        }
        *out = a.release();
        return TQ_OK;
    });
}

void tq_rf_destroy(tq_rf *acc) { delete acc; }

int tq_rf_reset(tq_rf *acc)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_rf_reset", [&]() -> int {
        if (acc->ctx) {
            TQ_HIP(acc->ctx, acc->order.sync());
            if (int rc = rf_clear_dev(acc)) return rc;
        }
        acc->table.forget(acc->ctx);
        acc->host_count.clear();
        acc->lists.clear();
        acc->ntrees = 0;
        acc->chunk.chunks = 0;
        acc->columns = acc->col_chunks = 0;
        acc->final_ok = false;
        return TQ_OK;
    });
}

int tq_rf_add(tq_rf *acc, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride, void *stream)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    tq_ctx *ctx = acc->ctx;
    return api(ctx, "tq_rf_add", [&]() -> int {
        SplitTable &t = acc->table;
        const int32_t T = acc->chunk.T, W = acc->chunk.W;
        if (int rc = tree_set_args(ctx, "tq_rf_add", parents, n_nodes, R, stride)) return rc;
        if (t.overflow) return t.overflowed(ctx, "tq_rf_add");
        if (R == 0) return TQ_OK;
        if (acc->ntrees + R > acc->max_trees)
            return fail(ctx, TQ_ERR_INVALID_ARG, "tq_rf_add: %lld trees held and %lld offered exceed max_trees = %lld",
                        (long long)acc->ntrees, (long long)R, (long long)acc->max_trees);
        const int64_t S = cons_stride(T);
        std::vector<int32_t> recs;
        if (int rc = prepare_trees(ctx, "tq_rf_add", parents, n_nodes, R, stride, T, recs)) return rc;
        if (!ctx) {
            std::vector<uint64_t> tmp, sides, m((size_t)W);
            acc->lists.reserve((size_t)(acc->ntrees + R));
            for (int64_t r = 0; r < R; ++r) {
                sides.clear();
                cons_host_splits(&recs[(size_t)r * S], T, W, tmp, sides);
                std::vector<uint32_t> ids;
                ids.reserve(sides.size() / W);
                for (size_t e = 0; e < sides.size(); e += W) {
                    m.assign(sides.begin() + e, sides.begin() + e + W);
                    const int64_t *id = rf_host_id(acc, m, t.max_splits);
                    if (!id) return t.overflowed(ctx, "tq_rf_add");
                    ids.push_back((uint32_t)*id);
                }
                std::sort(ids.begin(), ids.end());
                acc->lists.push_back(std::move(ids));
                acc->final_ok = false;
                ++acc->ntrees;
            }
            return TQ_OK;
        }
        for (int64_t r0 = 0; r0 < R; r0 += acc->chunk.chunk_trees) {
            const int64_t n = std::min<int64_t>(acc->chunk.chunk_trees, R - r0);
            if (int rc = rf_drain(acc)) return rc;          // the staging buffer and the mask scratch are free again
            acc->final_ok = false;
            if (int rc = rf_launch(acc, acc->ntrees, n, &recs[(size_t)r0 * S], (hipStream_t)stream)) return rc;
            acc->ntrees += n;
        }
        return TQ_OK;
    });
}

int tq_rf_shape(tq_rf *acc, int64_t *T, int64_t *W, int64_t *ntrees, int64_t *nsplits, int64_t *columns)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_rf_shape", [&]() -> int {
        if (T) *T = acc->chunk.T;
        if (W) *W = acc->chunk.W;
        if (ntrees) *ntrees = acc->ntrees;
        if (nsplits) {
            if (acc->ctx && !acc->table.overflow)
                if (int rc = rf_drain(acc)) return rc;
            *nsplits = (acc->ctx ? acc->table.dev_entries : 0) + (int64_t)acc->table.host.size();
        }
        if (columns) *columns = acc->columns;
        return TQ_OK;
    });
}

int tq_rf_read(tq_rf *acc, int32_t *nsplits, uint32_t *shared, uint32_t *rf)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_rf_read", [&]() -> int {
        if (int rc = rf_final(acc, "tq_rf_read")) return rc;
        const size_t N = (size_t)acc->ntrees;
        if (N == 0) return TQ_OK;
        if (acc->ctx) {
            if (nsplits) TQ_HIP(acc->ctx, hipMemcpy(nsplits, acc->d_nsplits, N * 4, hipMemcpyDeviceToHost));
            if (shared) TQ_HIP(acc->ctx, hipMemcpy(shared, acc->d_shared, N * N * 4, hipMemcpyDeviceToHost));
            if (rf) TQ_HIP(acc->ctx, hipMemcpy(rf, acc->d_rf, N * N * 4, hipMemcpyDeviceToHost));
        } else {
            if (nsplits) memcpy(nsplits, acc->h_nsplits.data(), N * 4);
            if (shared) memcpy(shared, acc->h_shared.data(), N * N * 4);
            if (rf) memcpy(rf, acc->h_rf.data(), N * N * 4);
        }
        return TQ_OK;
    });
}

int tq_rf_stats(tq_rf *acc, int64_t *out)
{
    if (!acc || !out) return TQ_ERR_INVALID_ARG;
    return api(acc->ctx, "tq_rf_stats", [&]() -> int {
        if (acc->ctx && !acc->table.overflow)
            if (int rc = rf_drain(acc)) return rc;
        out[0] = acc->chunk.chunk_trees;
        out[1] = acc->chunk.chunks;
        out[2] = acc->columns;
        out[3] = acc->cw_chunk;
        out[4] = acc->col_chunks;
        out[5] = acc->table.unresolved;
        out[6] = acc->table.hash_bits;
        out[7] = acc->table.dev_entries;
        return TQ_OK;
    });
}

uint32_t tq_rf_word_shared(uint64_t x, uint64_t y) { return rf_word_shared(x, y); }

int tq_qd_create(tq_qd **out, int64_t T, int64_t max_trees, tq_ctx *ctx)
{
    const char *who = "tq_qd_create";
    if (!out) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_qd_create: out is NULL");
    *out = nullptr;
    return api(ctx, who, [&]() -> int {
        std::unique_ptr<tq_qd> a(new tq_qd());
        if (int rc = a->set.create(who, T, max_trees, ctx, 0)) return rc;
        if (ctx) {
            const size_t mm = (size_t)(max_trees * max_trees);
            TQ_HIPF(ctx, who, a->d_same.alloc(mm));
            TQ_HIPF(ctx, who, a->d_both.alloc(mm));
            TQ_HIPF(ctx, who, hipMemset(a->d_same, 0, mm * 8));
            TQ_HIPF(ctx, who, hipMemset(a->d_both, 0, mm * 8));
            TQ_HIPF(ctx, who, hipDeviceSynchronize());
        }
        *out = a.release();
        return TQ_OK;
    });
}

void tq_qd_destroy(tq_qd *acc) { delete acc; }

int tq_qd_clear(tq_qd *acc)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->set.ctx, "tq_qd_clear", [&]() -> int { return qd_zero(acc); });
}

int tq_qd_reset(tq_qd *acc)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->set.ctx, "tq_qd_reset", [&]() -> int {
        if (int rc = qd_zero(acc)) return rc;
        acc->set.forget_trees();
        acc->kslices = 0;
        return TQ_OK;
    });
}

int tq_qd_add(tq_qd *acc, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride, void *stream)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->set.ctx, "tq_qd_add",
               [&]() -> int { return acc->set.add("tq_qd_add", parents, n_nodes, R, stride, (hipStream_t)stream); });
}

int tq_qd_score(tq_qd *acc, const int32_t *quartets, int64_t Q, void *stream)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->set.ctx, "tq_qd_score", [&]() -> int {
        if (int rc = acc->set.check_quartets("tq_qd_score", quartets, Q)) return rc;
        return qd_score(acc, quartets, nullptr, 0, Q, (hipStream_t)stream, "tq_qd_score");
    });
}

int tq_qd_score_ranks(tq_qd *acc, const uint64_t *ranks, uint64_t first_rank, int64_t Q, void *stream)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->set.ctx, "tq_qd_score_ranks", [&]() -> int {
        if (int rc = acc->set.check_ranks("tq_qd_score_ranks", ranks, first_rank, Q)) return rc;
        return qd_score(acc, nullptr, ranks, ranks ? 0 : first_rank, Q, (hipStream_t)stream, "tq_qd_score_ranks");
    });
}

int tq_qd_shape(tq_qd *acc, int64_t *T, int64_t *ntrees, uint64_t *q_total)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    if (T) *T = acc->set.T;
    if (ntrees) *ntrees = acc->set.ntrees;
    if (q_total) *q_total = acc->set.q_total;
    return TQ_OK;
}

int tq_qd_read(tq_qd *acc, uint64_t *same, uint64_t *both)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    tq_ctx *ctx = acc->set.ctx;
    return api(ctx, "tq_qd_read", [&]() -> int {
        QuartetPlanes &set = acc->set;
        const int64_t N = set.ntrees;
        const size_t bytes = (size_t)(N * N) * 8;
        if (N == 0) return TQ_OK;
        if (!ctx) {
            if (!set.scored) {
                if (same) memset(same, 0, bytes);
                if (both) memset(both, 0, bytes);
                return TQ_OK;
            }
            if (same) memcpy(same, acc->h_same.data(), bytes);
            if (both) memcpy(both, acc->h_both.data(), bytes);
            return TQ_OK;
        }
        hipStream_t st = set.order.last;
        if (set.scored && N > QD_BT) {                                  // the tiles below the diagonal, behind the last score
            hipLaunchKernelGGL(tq_qd_final_kernel, dim3((unsigned)((N * N + QD_THREADS - 1) / QD_THREADS)), dim3(QD_THREADS), 0, st,
                               acc->d_same.get(), acc->d_both.get(), (int32_t)N);
            TQ_LAUNCHED(ctx, "tq_qd_read");
            TQ_HIP(ctx, set.order.mark(st));
        }
        TQ_HIP(ctx, set.order.sync());
        if (same) TQ_HIP(ctx, hipMemcpy(same, acc->d_same, bytes, hipMemcpyDeviceToHost));
        if (both) TQ_HIP(ctx, hipMemcpy(both, acc->d_both, bytes, hipMemcpyDeviceToHost));
        return TQ_OK;
    });
}

int tq_qd_stats(tq_qd *acc, int64_t *out)
{
    if (!acc || !out) return TQ_ERR_INVALID_ARG;
    out[0] = acc->set.chunk_words * 64;
    out[1] = acc->set.chunks;
    out[2] = acc->kslices;
    out[3] = acc->set.tables;
    out[4] = acc->set.table_form();
    out[5] = acc->set.chunk_words;
    return TQ_OK;
}

void tq_qd_word_counts(uint64_t x0, uint64_t x1, uint64_t x2, uint64_t y0, uint64_t y1, uint64_t y2, uint32_t *same,
                       uint32_t *both)
{
    const QdCounts c = qd_word(x0, x1, x2, y0, y1, y2);
    if (same) *same = c.same;
    if (both) *both = c.both;
}

int tq_ls_create(tq_ls **out, int64_t T, int64_t max_trees, tq_ctx *ctx)
{
    const char *who = "tq_ls_create";
    if (!out) return fail(ctx, TQ_ERR_INVALID_ARG, "tq_ls_create: out is NULL");
    *out = nullptr;
    return api(ctx, who, [&]() -> int {
        std::unique_ptr<tq_ls> a(new tq_ls());
        // on top of the planes' chunk: a counts row of 8 bytes per quartet on the device and as many page-locked
        if (int rc = a->set.create(who, T, max_trees, ctx, 64 * (8 + 8))) return rc;
        if (!ctx) {
            a->h_acc.assign((size_t)T * 4, 0);
        } else {
            const size_t cq = (size_t)a->set.chunk_words * 64;
            TQ_HIPF(ctx, who, a->d_acc.alloc((size_t)T * 4));
            TQ_HIPF(ctx, who, a->d_counts.alloc(cq));
            TQ_HIPF(ctx, who, a->p_counts.alloc(cq));
            TQ_HIPF(ctx, who, hipMemset(a->d_acc, 0, (size_t)T * 4 * 8));
            TQ_HIPF(ctx, who, hipDeviceSynchronize());
        }
        *out = a.release();
        return TQ_OK;
    });
}

void tq_ls_destroy(tq_ls *acc) { delete acc; }

int tq_ls_clear(tq_ls *acc)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->set.ctx, "tq_ls_clear", [&]() -> int { return ls_zero(acc); });
}

int tq_ls_reset(tq_ls *acc)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->set.ctx, "tq_ls_reset", [&]() -> int {
        if (int rc = ls_zero(acc)) return rc;
        acc->set.forget_trees();
        acc->groups = 0;
        return TQ_OK;
    });
}

int tq_ls_add(tq_ls *acc, const int32_t *parents, const int64_t *n_nodes, int64_t R, int64_t stride, void *stream)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->set.ctx, "tq_ls_add",
               [&]() -> int { return acc->set.add("tq_ls_add", parents, n_nodes, R, stride, (hipStream_t)stream); });
}

int tq_ls_score(tq_ls *acc, const int32_t *quartets, int64_t Q, uint16_t *counts, void *stream)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->set.ctx, "tq_ls_score", [&]() -> int {
        if (int rc = acc->set.check_quartets("tq_ls_score", quartets, Q)) return rc;
        return ls_score(acc, quartets, nullptr, 0, Q, counts, (hipStream_t)stream, "tq_ls_score");
    });
}

int tq_ls_score_ranks(tq_ls *acc, const uint64_t *ranks, uint64_t first_rank, int64_t Q, uint16_t *counts, void *stream)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    return api(acc->set.ctx, "tq_ls_score_ranks", [&]() -> int {
        if (int rc = acc->set.check_ranks("tq_ls_score_ranks", ranks, first_rank, Q)) return rc;
        return ls_score(acc, nullptr, ranks, ranks ? 0 : first_rank, Q, counts, (hipStream_t)stream, "tq_ls_score_ranks");
    });
}

int tq_ls_shape(tq_ls *acc, int64_t *T, int64_t *ntrees, uint64_t *q_total)
{
    if (!acc) return TQ_ERR_INVALID_ARG;
    if (T) *T = acc->set.T;
    if (ntrees) *ntrees = acc->set.ntrees;
    if (q_total) *q_total = acc->set.q_total;
    return TQ_OK;
}

int tq_ls_read(tq_ls *acc, uint64_t *out)
{
    if (!acc || !out) return TQ_ERR_INVALID_ARG;
    tq_ctx *ctx = acc->set.ctx;
    return api(ctx, "tq_ls_read", [&]() -> int {
        const size_t bytes = (size_t)acc->set.T * 4 * 8;
        if (!ctx) {
            memcpy(out, acc->h_acc.data(), bytes);
            return TQ_OK;
        }
        TQ_HIP(ctx, acc->set.order.sync());
        TQ_HIP(ctx, hipMemcpy(out, acc->d_acc, bytes, hipMemcpyDeviceToHost));
        return TQ_OK;
    });
}

int tq_ls_stats(tq_ls *acc, int64_t *out)
{
    if (!acc || !out) return TQ_ERR_INVALID_ARG;
    out[0] = acc->set.chunk_words * 64;
    out[1] = acc->set.chunks;
    out[2] = acc->set.tables;
    out[3] = acc->set.table_form();
    out[4] = acc->set.chunk_words;
    out[5] = acc->groups;
    out[6] = LS_TILE;
    return TQ_OK;
}

int tq_device_info(tq_ctx *ctx, int32_t *num_cu, int32_t *waves_per_cu, int64_t *row_pitch)
{
    if (!ctx) return TQ_ERR_INVALID_ARG;
    if (num_cu) *num_cu = ctx->prop.multiProcessorCount;
    if (waves_per_cu) *waves_per_cu = ctx->opt.waves_per_cu;
    if (row_pitch) *row_pitch = ctx->nat.Sp;
    return TQ_OK;
}

}  // extern "C"

