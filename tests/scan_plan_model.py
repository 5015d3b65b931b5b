"""Which scan kernel takes a batch: the rule as the library had it before scan_plan.hpp existed, transcribed statement
by statement from `use_dp`, `launch_scan_n` and the five launchers of tetrad_hip.hip at commit c9022ff -- same nesting,
same order, the dispatch macros (TQ_F4_CASE, TQ_WG_CASE, TQ_SCAN_CASE) as loops.  It is the independent statement of
the behaviour that tests/test_scan_plan_cpu.py holds `choose_scan` to; it is not derived from scan_plan.hpp and must
not be "tidied" to look like it.

A launch is written down as the tuple PLAN_FIELDS: the kernel form, the template arguments of the kernel (0 where
the form's kernel has no such argument), quartets and threads per workgroup, grid and xcd_chunk (grid 0: the one-wave
form, whose grid comes from the occupancy query at launch).
"""
from collections import namedtuple

KNOB_FIELDS = ("scan_pair", "scan_wg", "scan_method", "scan_f4", "scan_dp", "park_t", "share_c", "count_invariant",
               "waves_per_cu", "nrep", "order", "wg_min_quartets", "dp_min_quartets", "pb_ok", "xcd_remap", "num_cu")
SHAPE_FIELDS = ("T", "pitch", "Sp", "Q", "subsample", "input_sorted")
PLAN_FIELDS = ("form", "sub", "method", "nw", "shc", "park", "nrep", "qpw", "threads", "grid", "xcd_chunk")
Plan = namedtuple("Plan", PLAN_FIELDS)

#: a context's defaults (struct tq_ctx) on a 256-CU device whose PB probe passed
DEFAULT_KNOBS = dict(scan_pair=0, scan_wg=4, scan_method=-1, scan_f4=-1, scan_dp=1, park_t=1, share_c=0, count_invariant=0,
                     waves_per_cu=0, nrep=1, order=1, wg_min_quartets=4096, dp_min_quartets=32768, pb_ok=1, xcd_remap=1,
                     num_cu=256)

ONE_WAVE, WG, WG2, F4, PB, DP = 1, 2, 3, 4, 5, 6
FORM_NAMES = {ONE_WAVE: "one_wave", WG: "wg", WG2: "wg2", F4: "f4", PB: "pb", DP: "dp"}
WAVE = 64
TILE = 2048
PB_NW = 4
PB_MAX_TILES = 1023
DP_NW = 4
U64 = (1 << 64) - 1


def use_dp(k, T, Sp, n, subsample, input_sorted):
    T3 = (T * T * T) & U64
    return bool(not subsample and k["scan_dp"] and k["scan_f4"] <= 0 and k["scan_method"] < 0 and k["scan_wg"] == 4
                and not k["count_invariant"] and not k["share_c"] and not k["scan_pair"] and k["waves_per_cu"] == 0
                and (k["order"] or input_sorted) and n >= k["dp_min_quartets"] and n >= 2 and n <= 0x7FFFFFFF
                and T3 <= 0xFFFFFFFF and ((T * Sp) & U64) < 0xFFFF0000)


def launch_scan(k, Q, NREP, SUB, METHOD):
    return Plan(ONE_WAVE, int(SUB), METHOD, 1, 0, 0, NREP, 1, WAVE, 0, 0)


def launch_scan_wg(k, Q, SUB, METHOD, NW, SHC=False, PARK_T=False):
    wgs = (k["waves_per_cu"] + NW - 1) // NW if k["waves_per_cu"] > 0 else 0
    nblk = (Q + NW - 1) // NW
    grid = k["num_cu"] * wgs if wgs > 0 else nblk
    xcd_chunk = 0
    if grid >= nblk:
        grid = nblk
        if k["xcd_remap"] and nblk >= 64:
            xcd_chunk = (nblk + 7) // 8
            grid = xcd_chunk * 8
    if grid < 1:
        grid = 1
    return Plan(WG, int(SUB), METHOD, NW, int(SHC), int(PARK_T), 0, NW, NW * WAVE, grid, xcd_chunk)


def launch_scan_pb(k, Q, SUB):
    nblk = (Q + PB_NW - 1) // PB_NW
    grid, xcd_chunk = nblk, 0
    if k["xcd_remap"] and nblk >= 64:
        xcd_chunk = (nblk + 7) // 8
        grid = xcd_chunk * 8
    if grid < 1:
        grid = 1
    return Plan(PB, int(SUB), 0, PB_NW, 0, 0, 0, PB_NW, PB_NW * WAVE, grid, xcd_chunk)


def launch_scan_wg2(k, Q, SUB, METHOD, NW):
    nblk = (Q + 2 * NW - 1) // (2 * NW)
    grid, xcd_chunk = nblk, 0
    if k["xcd_remap"] and nblk >= 64:
        xcd_chunk = (nblk + 7) // 8
        grid = xcd_chunk * 8
    if grid < 1:
        grid = 1
    return Plan(WG2, int(SUB), METHOD, NW, 0, 0, 0, 2 * NW, NW * WAVE, grid, xcd_chunk)


def launch_scan_dp(k, Q):
    least = ((Q + 1) // 2 + DP_NW - 1) // DP_NW
    grid = (least + 7) // 8 * 8
    return Plan(DP, 0, 0, DP_NW, 0, 0, 0, 2 * DP_NW, DP_NW * WAVE, grid, 0)


def launch_scan_n(k, T, pitch, Q, subsample):
    fits = ((T * pitch) & U64) < 0xFFFF0000
    if (k["scan_pair"] and k["scan_wg"] == 4 and Q >= 64 and not k["count_invariant"] and not k["share_c"]
            and k["waves_per_cu"] == 0 and k["scan_method"] < 2 and fits):
        m = (1 if subsample else 0) if k["scan_method"] < 0 else k["scan_method"]
        if subsample:
            return launch_scan_wg2(k, Q, True, 1, 4) if m else launch_scan_wg2(k, Q, True, 0, 4)
        return launch_scan_wg2(k, Q, False, 1, 4) if m else launch_scan_wg2(k, Q, False, 0, 4)
    f4 = (subsample != 0 and k["scan_method"] < 0 and bool(k["park_t"])) if k["scan_f4"] < 0 else k["scan_f4"] != 0
    if (f4 and (k["scan_wg"] == 4 or k["scan_wg"] == 8 or k["scan_wg"] == 2) and Q >= k["wg_min_quartets"]
            and not k["count_invariant"] and not k["share_c"] and not k["scan_pair"] and k["waves_per_cu"] == 0
            and (k["scan_method"] < 0 or k["scan_method"] == 1) and fits):
        nw = k["scan_wg"]
        nblk = (Q + nw - 1) // nw
        grid, xcd_chunk = nblk, 0
        if k["xcd_remap"] and nblk >= 64:
            xcd_chunk = (nblk + 7) // 8
            grid = xcd_chunk * 8
        for SUBF, NWF in ((True, 4), (False, 4), (True, 8), (False, 8), (True, 2), (False, 2)):      # TQ_F4_CASE
            if (subsample != 0) == SUBF and nw == NWF:
                return Plan(F4, int(SUBF), 0, NWF, 0, 0, 0, NWF, NWF * WAVE, grid, xcd_chunk)
        raise AssertionError("the f4 block launched nothing")
    pb_fits = (k["pb_ok"] == 1 and k["scan_wg"] == 4 and Q >= 64 and not k["count_invariant"] and not k["share_c"]
               and not k["scan_pair"] and k["waves_per_cu"] == 0 and pitch // TILE <= PB_MAX_TILES and fits)
    if pb_fits and k["scan_method"] == 6:
        return launch_scan_pb(k, Q, True) if subsample else launch_scan_pb(k, Q, False)
    if k["scan_wg"] >= 2 and Q >= k["wg_min_quartets"] and not k["count_invariant"] and fits:
        m = (1 if subsample else 0) if k["scan_method"] < 0 else k["scan_method"]
        if m == 6:
            m = 1 if subsample else 0

        def wg_case(NW):                                                                             # TQ_WG_CASE
            if k["scan_wg"] == NW:
                if m == 2:
                    return launch_scan_wg(k, Q, True, 2, NW)
                if m == 3:
                    return launch_scan_wg(k, Q, True, 3, NW)
                if NW == 4 and m == 4:
                    return launch_scan_wg(k, Q, True, 4, 4)
                if NW == 4 and m == 5:
                    return launch_scan_wg(k, Q, True, 5, 4)
                if subsample:
                    return launch_scan_wg(k, Q, True, 1, NW) if m else launch_scan_wg(k, Q, True, 0, NW)
                return launch_scan_wg(k, Q, False, 1, NW) if m else launch_scan_wg(k, Q, False, 0, NW)
            return None

        r = wg_case(2)
        if r:
            return r
        if k["scan_wg"] == 4 and k["park_t"] and m == 1 and not k["share_c"]:
            return (launch_scan_wg(k, Q, True, 1, 4, False, True) if subsample
                    else launch_scan_wg(k, Q, False, 1, 4, False, True))
        if (k["scan_wg"] == 8 or k["scan_wg"] == 6) and k["park_t"] and m == 1 and subsample and not k["share_c"]:
            return (launch_scan_wg(k, Q, True, 1, 8, False, True) if k["scan_wg"] == 8
                    else launch_scan_wg(k, Q, True, 1, 6, False, True))
        if k["scan_wg"] == 4 and k["share_c"] and m <= 1:
            if subsample:
                return launch_scan_wg(k, Q, True, 1, 4, True) if m else launch_scan_wg(k, Q, True, 0, 4, True)
            return launch_scan_wg(k, Q, False, 1, 4, True) if m else launch_scan_wg(k, Q, False, 0, 4, True)
        for NW in (4, 3, 6, 16, 8):
            r = wg_case(NW)
            if r:
                return r
    method = (1 if subsample else 0) if (k["scan_method"] < 0 or k["scan_method"] == 6) else k["scan_method"]

    def scan_case(N):                                                                                # TQ_SCAN_CASE
        if method == 0:
            return launch_scan(k, Q, N, True, 0) if subsample else launch_scan(k, Q, N, False, 0)
        return launch_scan(k, Q, N, True, 1) if subsample else launch_scan(k, Q, N, False, 1)

    for N in (2, 4, 8, 16, 32):
        if k["nrep"] == N:
            return scan_case(N)
    return scan_case(1)


def plan(knobs, shape):
    """stage_scan's choice for a context with options `knobs` (dict over KNOB_FIELDS) and a batch `shape` (dict over
    SHAPE_FIELDS): a Plan."""
    k, s = knobs, shape
    if use_dp(k, s["T"], s["Sp"], s["Q"], s["subsample"], s["input_sorted"]):
        return launch_scan_dp(k, s["Q"])
    return launch_scan_n(k, s["T"], s["pitch"], s["Q"], s["subsample"])


def built_kernels():
    """Every scan instantiation the parent's launch code names, as (form, sub, method, nw, shc, park, nrep): the template
    arguments each dispatch macro and each explicit launch line spells out."""
    out = set()
    for N in (2, 4, 8, 16, 32, 1):                                                                  # TQ_SCAN_CASE
        for SUB in (1, 0):
            for M in (0, 1):
                out.add((ONE_WAVE, SUB, M, 1, 0, 0, N))
    for NW in (2, 4, 3, 6, 16, 8):                                                                  # TQ_WG_CASE
        out |= {(WG, 1, 2, NW, 0, 0, 0), (WG, 1, 3, NW, 0, 0, 0), (WG, 1, 4, 4, 0, 0, 0), (WG, 1, 5, 4, 0, 0, 0),
                (WG, 1, 1, NW, 0, 0, 0), (WG, 1, 0, NW, 0, 0, 0), (WG, 0, 1, NW, 0, 0, 0), (WG, 0, 0, NW, 0, 0, 0)}
    out |= {(WG, 1, 1, 4, 0, 1, 0), (WG, 0, 1, 4, 0, 1, 0), (WG, 1, 1, 8, 0, 1, 0), (WG, 1, 1, 6, 0, 1, 0)}       # PARK_T
    out |= {(WG, 1, 1, 4, 1, 0, 0), (WG, 1, 0, 4, 1, 0, 0), (WG, 0, 1, 4, 1, 0, 0), (WG, 0, 0, 4, 1, 0, 0)}       # SHC
    out |= {(WG2, 1, 1, 4, 0, 0, 0), (WG2, 1, 0, 4, 0, 0, 0), (WG2, 0, 1, 4, 0, 0, 0), (WG2, 0, 0, 4, 0, 0, 0)}
    for SUBF, NWF in ((1, 4), (0, 4), (1, 8), (0, 8), (1, 2), (0, 2)):                              # TQ_F4_CASE
        out.add((F4, SUBF, 0, NWF, 0, 0, 0))
    out |= {(PB, 1, 0, PB_NW, 0, 0, 0), (PB, 0, 0, PB_NW, 0, 0, 0)}
    out.add((DP, 0, 0, DP_NW, 0, 0, 0))
    return out
