// scan_plan.hpp -- which site-scan kernel takes a batch, and with what grid.
//
// choose_scan() is the whole rule: a pure function of the options (ScanKnobs) and the batch (ScanShape) that names one
// kernel instantiation (ScanPlan).  tetrad_hip.hip looks the plan up in its table of instantiations and launches it;
// tq_scan_plan() hands the same plan to tests.  Plain host C++17: no HIP types, so the rule also compiles on its own.
// DESIGN.md section 4.1 has the decision table.
#include <cstdint>

// kernel forms, as tq_debug_fetch(which = 6) reports them
enum { SCAN_FORM_NONE = 0, SCAN_FORM_ONE_WAVE = 1, SCAN_FORM_WG = 2, SCAN_FORM_WG2 = 3, SCAN_FORM_F4 = 4, SCAN_FORM_PB = 5,
       SCAN_FORM_DP = 6 };

// what the rule has to know about the kernels (tetrad_hip.hip asserts that they agree with the kernel headers)
constexpr int SCAN_WAVE = 64;                 // lanes per wave
constexpr int SCAN_TILE = 2048;               // sites per wave step
constexpr int SCAN_PB_NW = 4;                 // waves per workgroup of the PB form
constexpr int SCAN_PB_MAX_TILES = 1023;       // its 16-bit counters hold this many steps
constexpr int SCAN_DP_NW = 4;                 // waves (= pairs) per workgroup of the DP form
// The cooperative forms address a layout set with 32-bit byte offsets: T * pitch must stay below this.
constexpr uint64_t SCAN_OFFSET_LIMIT = 0xFFFF0000ull;

struct ScanKnobs {                            // options of the context, under their tq_set_option names
    int scan_pair, scan_wg, scan_method, scan_f4, scan_dp, park_t, share_c, count_invariant, waves_per_cu, nrep, order;
    int64_t wg_min_quartets, dp_min_quartets;
    int pb_ok;                                // 1: the PB kernel's LDS probe passed (tq_create)
    int xcd_remap;
    int num_cu;
};

struct ScanShape {
    int64_t T;
    int64_t pitch;                            // sites per row of the set the scan reads (packed or natural)
    int64_t Sp;                               // sites per row of the natural set (the DP form reads that one)
    int64_t Q;
    int subsample, input_sorted;
};

struct ScanPlan {
    int form;                                 // SCAN_FORM_*
    // template arguments of the kernel; 0 where the form's kernel has no such argument
    int sub, method, nw, shc, park, nrep;
    int qpw, threads;                         // quartets and threads per workgroup
    int64_t grid, xcd_chunk;                  // grid 0: the one-wave form sizes its grid by the occupancy query at launch
};

// Grid of the joint-histogram scan: its unit list has at least ceil(Q / 2) units and at most Q -- the grid covers the
// least (rounded to the 8 XCDs) and a workgroup whose id + grid is still a block takes that one as well.
inline int64_t scan_dp_grid(int64_t Q)
{
    const int64_t least = ((Q + 1) / 2 + SCAN_DP_NW - 1) / SCAN_DP_NW;
    return (least + 7) / 8 * 8;
}

// Grid of the workgroup forms (WG, WG2, F4, PB).  Default: one block of qpw quartets per workgroup, dispatched in sorted
// order.  Workgroups that run at the same time are then neighbours of the (a,b) order (their shared rows are L2 hits)
// and the dispatcher balances the load; a persistent grid-stride loop was 13 % slower.  Option waves_per_cu caps the
// grid (WG form only: the other forms are chosen with waves_per_cu == 0).
inline void scan_wg_grid(const ScanKnobs &k, int64_t Q, ScanPlan &p)
{
    const int wgs = k.waves_per_cu > 0 ? (k.waves_per_cu + p.nw - 1) / p.nw : 0;
    const int64_t nblk = (Q + p.qpw - 1) / p.qpw;
    p.grid = wgs > 0 ? (int64_t)k.num_cu * wgs : nblk;
    p.xcd_chunk = 0;
    if (p.grid >= nblk) {
        p.grid = nblk;
        if (k.xcd_remap && nblk >= 64) {                     // one block per workgroup, XCD-contiguous
            p.xcd_chunk = (nblk + 7) / 8;
            p.grid = p.xcd_chunk * 8;
        }
    }
    if (p.grid < 1) p.grid = 1;
}

inline ScanPlan choose_scan(const ScanKnobs &k, const ScanShape &s)
{
    const int sub = s.subsample != 0;
    const int wg = k.scan_wg;
    const int64_t Q = s.Q;
    const uint64_t T = (uint64_t)s.T;
    const int mode_method = sub ? 1 : 0;                     // what scan_method -1 stands for
    const bool auto_method = k.scan_method < 0;
    const bool offsets_fit_32 = T * (uint64_t)s.pitch < SCAN_OFFSET_LIMIT;
    const bool natural_offsets_fit_32 = T * (uint64_t)s.Sp < SCAN_OFFSET_LIMIT;
    const bool plain_options = !k.count_invariant && !k.share_c && k.waves_per_cu == 0;
    const bool one_per_wave = !k.scan_pair;
    // WG and F4 leave small batches to the one-wave form (option wg_min_quartets: latency-bound calls); WG2 and PB ask
    // for one XCD round of blocks only, the literal 64
    const bool fills_chip = Q >= k.wg_min_quartets;
    const bool some_blocks = Q >= 64;
    // scan_f4 -1: row f4 as written takes subsample mode when nothing else was asked for
    const bool f4_wanted = k.scan_f4 < 0 ? (sub && auto_method && k.park_t) : k.scan_f4 != 0;

    ScanPlan p{};
    auto workgroup = [&](int form, int nw, int qpw) {
        p.form = form;
        p.sub = sub;
        p.nw = nw;
        p.qpw = qpw;
        p.threads = nw * SCAN_WAVE;
        scan_wg_grid(k, Q, p);
    };

    // DP: two quartets that share (a,b,c) per wave, one joint histogram.  Full mode, automatic kernel choice, the
    // default workgroup shape, keys that hold (a,b,c), and an order the pairing can rely on (sorted here, or on arrival).
    if (!sub && k.scan_dp && k.scan_f4 <= 0 && auto_method && wg == 4 && plain_options && one_per_wave &&
        (k.order || s.input_sorted) && Q >= k.dp_min_quartets && Q >= 2 && Q <= 0x7FFFFFFF && T * T * T <= 0xFFFFFFFFull &&
        natural_offsets_fit_32) {
        p.form = SCAN_FORM_DP;
        p.nw = SCAN_DP_NW;
        p.qpw = 2 * SCAN_DP_NW;
        p.threads = SCAN_DP_NW * SCAN_WAVE;
        p.grid = scan_dp_grid(Q);
        return p;
    }
    // WG2: two quartets per wave (option scan_pair), methods 0 and 1 at four waves
    if (k.scan_pair && wg == 4 && some_blocks && plain_options && k.scan_method < 2 && offsets_fit_32) {
        workgroup(SCAN_FORM_WG2, 4, 8);
        p.method = auto_method ? mode_method : k.scan_method;
        return p;
    }
    // F4: own rows as 12-byte plane records only, pattern bits pulled out in the walk (method 1 by construction)
    if (f4_wanted && (wg == 4 || wg == 8 || wg == 2) && fills_chip && plain_options && one_per_wave &&
        (auto_method || k.scan_method == 1) && offsets_fit_32) {
        workgroup(SCAN_FORM_F4, wg, wg);
        return p;
    }
    // PB: bank-private 16-bit counters (scan_method 6, an A/B form), so only while a quartet has at most
    // SCAN_PB_MAX_TILES steps and the LDS probe passed.  Where it does not apply, method 6 is the mode's default below.
    if (k.scan_method == 6 && k.pb_ok == 1 && wg == 4 && some_blocks && plain_options && one_per_wave &&
        s.pitch / SCAN_TILE <= SCAN_PB_MAX_TILES && offsets_fit_32) {
        workgroup(SCAN_FORM_PB, SCAN_PB_NW, SCAN_PB_NW);
        return p;
    }
    const int method = auto_method || k.scan_method == 6 ? mode_method : k.scan_method;
    // WG: one quartet per wave, wg waves share rows a and b.  scan_wg 1 asks for the one-wave form.
    if ((wg == 2 || wg == 3 || wg == 4 || wg == 6 || wg == 8 || wg == 16) && fills_chip && !k.count_invariant &&
        offsets_fit_32) {
        workgroup(SCAN_FORM_WG, wg, wg);
        if (method == 2 || method == 3) {
            // the timing diagnostics are built on the subsample kernel only: SUB whatever the mode
            p.sub = 1;
            p.method = method;
        } else if (wg == 4 && (method == 4 || method == 5)) {
            // further diagnostics, built at four waves only (also SUB); at other widths they are method 1
            p.sub = 1;
            p.method = method;
        } else {
            p.method = method ? 1 : 0;
            // PARK_T (transposed pattern park of the walk, method 1) is built at four waves in both modes and at six
            // and eight in subsample mode, never together with share_c; two waves never have it
            const bool park_built = wg == 4 || ((wg == 6 || wg == 8) && sub);
            if (k.park_t && method == 1 && !k.share_c && park_built) p.park = 1;
            // SHC (row c shared as well) is built at four waves, methods 0 and 1; other widths ignore share_c
            else if (k.share_c && wg == 4 && method <= 1) p.shc = 1;
        }
        return p;
    }
    // one wave per quartet: methods 0 and 1 only (anything else is 1), and the only form option nrep reaches
    p.form = SCAN_FORM_ONE_WAVE;
    p.sub = sub;
    p.method = method ? 1 : 0;
    p.nw = 1;
    p.nrep = k.nrep == 2 || k.nrep == 4 || k.nrep == 8 || k.nrep == 16 || k.nrep == 32 ? k.nrep : 1;
    p.qpw = 1;
    p.threads = SCAN_WAVE;
    return p;
}
