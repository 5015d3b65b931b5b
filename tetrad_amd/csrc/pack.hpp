// pack.hpp -- site packing for subsample mode: whole loci per 32-site lane word, words grouped by their locus count
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace).  Host code only.
//
// In subsample mode one site per locus run is counted (scan.hpp: count_from_candidates), so the number of trips a lane's
// set-bit walk makes in a step is the number of loci with a counted site in its 32-site word, and a wave walks for its
// longest lane.  In the natural layout a word holds whatever loci start in its window (4 to 9 at c3 shape) and the wave
// pays for the fullest.  The count matrix is a histogram over loci -- the order of the loci, their position on the padded
// site axis and sites missing in every taxon do not change it; only the order of the sites INSIDE a locus does -- so the
// device may hold a second copy of the matrix in an order of its own:
//   1. the sites of a locus stay adjacent and in their order;
//   2. a locus of <= 32 sites lies inside one word;
//   3. a longer locus starts a word and runs through consecutive words (the lane / step carry of the scan handles it);
//      the rest of its last word takes further loci;
//   4. words are laid out by falling locus count, so the 64 words of a step hold (nearly) the same number;
//   5. a pad is missing in every taxon and carries no run-begin bit: it belongs to the run before it and is never counted.
// Words are filled best-fit in order of falling locus length (33 stacks of open words by free sites: linear time), which
// keeps the number of steps at ceil(S / 2048) or one more; a step then costs max-count trips instead of the natural
// layout's max over 64 random windows.  DESIGN.md section 4.1, profiles/site_pack/README.md.
#pragma once

constexpr uint32_t PACK_PAD = 0xFFFFFFFFu;

// predicted vector instructions of the plane-record scan per quartet: PACK_STEP_COST per 2048-site step outside the walk,
// PACK_TRIP_COST per walk trip (profiles/r04_scan/README.md section 9: 141 per step at 8.2 trips of 15).  The estimate comes
// from PACK_SAMPLE quartets, both layouts on the same ones.  Packing is taken when the gain is at least PACK_MIN_GAIN of the
// natural cost (the second layout set costs memory and build time) AND that holds two standard errors of the sample's paired
// differences below its mean: on sparse matrices the trips of a quartet scatter widely (taxa 85-98 % missing), a sample
// mean alone says "3 %" where 200 quartets say 0.7 %, and nothing is gained there.
constexpr double PACK_STEP_COST = 18.0, PACK_TRIP_COST = 15.0, PACK_MIN_GAIN = 0.03;
constexpr int PACK_SAMPLE = 24;

inline size_t pack_round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct LocusRun {
    int64_t start, len;
};

// runs of equal locus id (the caller has checked that every id forms one run)
inline void locus_runs(const uint32_t *loc, int64_t S, std::vector<LocusRun> &runs)
{
    runs.clear();
    for (int64_t s = 0; s < S;) {
        int64_t e = s + 1;
        while (e < S && loc[e] == loc[s]) ++e;
        runs.push_back({s, e - s});
        s = e;
    }
}

// The packing plan at locus level: packed start of every run from the run lengths alone (no work per site).  The scratch
// vectors live in the planner and keep their capacity, so a planner that is kept (one per bootstrap source) allocates
// nothing once it has seen its number of loci.
struct PackPlanner {
    std::vector<uint64_t> start;                     // start[i] = packed position of the first site of run i
    std::vector<uint32_t> by_len, bin_of, bin_count, first, fill, member, order;
    std::vector<uint32_t> open[33];                  // open[r]: bins with r free sites
    std::vector<uint32_t> bucket[33];

    // len_of(i) = sites of run i (>= 1), runs in the order of the matrix; returns the padded length, a multiple of TILE
    template <typename LenOf>
    size_t plan(size_t n, LenOf len_of)
    {
        // loci by falling length: the long ones (> 32 sites) first, then buckets 32 .. 1, each in the original order
        by_len.clear();
        for (auto &v : bucket) v.clear();
        for (size_t i = 0; i < n; ++i) {
            const int64_t len = (int64_t)len_of(i);
            if (len > 32) by_len.push_back((uint32_t)i);
            else bucket[len].push_back((uint32_t)i);
        }
        for (int l = 32; l >= 1; --l) by_len.insert(by_len.end(), bucket[l].begin(), bucket[l].end());
        // a bin = one word, preceded by the full words of a long first locus; its count = loci that may be counted in its word
        bin_count.clear();
        bin_of.resize(n);
        for (auto &v : open) v.clear();
        for (uint32_t i : by_len) {
            const int64_t len = (int64_t)len_of(i);
            const int need = (int)(len > 32 ? (len - 1) % 32 + 1 : len);       // sites in the bin's own word
            int r = 33;
            if (len <= 32)
                for (r = need; r <= 32 && open[r].empty(); ++r) {}
            uint32_t b;
            if (r <= 32) {
                b = open[r].back();
                open[r].pop_back();
            } else {
                b = (uint32_t)bin_count.size();
                bin_count.push_back(0);
                r = 32;
            }
            bin_of[i] = b;
            bin_count[b]++;
            if (r - need > 0) open[r - need].push_back(b);
        }
        // the loci of each bin, in placement order (a long locus is the first of its bin)
        const size_t nb = bin_count.size();
        first.assign(nb + 1, 0);
        member.resize(n);
        for (size_t i = 0; i < n; ++i) first[bin_of[i] + 1]++;
        for (size_t b = 0; b < nb; ++b) first[b + 1] += first[b];
        fill.assign(first.begin(), first.end() - 1);
        for (uint32_t i : by_len) member[fill[bin_of[i]]++] = i;
        // bins by falling count (stable)
        order.clear();
        for (auto &v : bucket) v.clear();
        for (size_t b = 0; b < nb; ++b) bucket[bin_count[b]].push_back((uint32_t)b);
        for (int c = 32; c >= 1; --c) order.insert(order.end(), bucket[c].begin(), bucket[c].end());
        start.resize(n);
        size_t pos = 0;
        for (uint32_t b : order) {
            for (uint32_t k = first[b]; k < first[b + 1]; ++k) {
                start[member[k]] = pos;
                pos += (size_t)len_of(member[k]);
            }
            pos = pack_round_up(pos, 32);
        }
        return pack_round_up(pos ? pos : 1, TILE);
    }
};

// src[p] = original site of packed position p, or PACK_PAD; src.size() is a multiple of TILE: the plan, site by site
inline void pack_sites(const std::vector<LocusRun> &runs, std::vector<uint32_t> &src)
{
    PackPlanner pl;
    const size_t total = pl.plan(runs.size(), [&runs](size_t i) { return runs[i].len; });
    src.assign(total, PACK_PAD);
    for (size_t i = 0; i < runs.size(); ++i)
        for (int64_t s = 0; s < runs[i].len; ++s) src[pl.start[i] + (size_t)s] = (uint32_t)(runs[i].start + s);
}

// Walk trips and predicted cost per quartet of the natural and of the packed layout, from PACK_SAMPLE pseudo-random
// quartets evaluated on the host: the counted site of a locus is its first site that no taxon of the quartet misses and
// where the four bases differ (resolve_quartets.py:58-64, 216-218); a step costs the largest number of counted sites in
// one of its 64 words.  cost[0] = natural, cost[1] = packed; trips likewise.  Returns the relative gain
// (cost[0] - cost[1]) / cost[0], lowered by two standard errors of the paired per-quartet differences.
inline double pack_estimate(const uint8_t *tmparr, int64_t T, int64_t S, const std::vector<LocusRun> &runs,
                          const std::vector<uint32_t> &src, double cost[2], double trips[2])
{
    const int64_t Wn = (int64_t)pack_round_up((size_t)S, TILE) / 32, Wp = (int64_t)src.size() / 32;
    cost[0] = PACK_STEP_COST * (double)(Wn / WAVE);
    cost[1] = PACK_STEP_COST * (double)(Wp / WAVE);
    trips[0] = trips[1] = 0.0;
    if (T < 4) return 0.0;
    std::vector<uint32_t> pos((size_t)S);
    for (size_t p = 0; p < src.size(); ++p)
        if (src[p] != PACK_PAD) pos[src[p]] = (uint32_t)p;
    std::vector<uint8_t> cn((size_t)Wn), cp((size_t)Wp);
    uint64_t x = 0x9E3779B97F4A7C15ull ^ (uint64_t)S;
    auto next = [&x]() {
        x += 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    uint64_t sum[2] = {0, 0};
    double dsum = 0.0, dsq = 0.0;                    // paired differences natural - packed, in trips
    for (int q = 0; q < PACK_SAMPLE; ++q) {
        int64_t t[4];
        for (int k = 0; k < 4; ++k) {
            bool again;
            do {
                t[k] = (int64_t)(next() % (uint64_t)T);
                again = false;
                for (int j = 0; j < k; ++j) again |= t[j] == t[k];
            } while (again);
        }
        const uint8_t *a = tmparr + t[0] * S, *b = tmparr + t[1] * S, *c = tmparr + t[2] * S, *d = tmparr + t[3] * S;
        std::fill(cn.begin(), cn.end(), (uint8_t)0);
        std::fill(cp.begin(), cp.end(), (uint8_t)0);
        for (const LocusRun &run : runs) {
            for (int64_t s = run.start; s < run.start + run.len; ++s) {
                const uint8_t va = a[s], vb = b[s], vc = c[s], vd = d[s];
                if ((va | vb | vc | vd) > 3 || (va == vb && va == vc && va == vd)) continue;
                cn[(size_t)(s >> 5)]++;
                cp[pos[(size_t)s] >> 5]++;
                break;
            }
        }
        uint64_t tq[2] = {0, 0};
        for (int64_t w = 0; w < Wn; w += WAVE) tq[0] += *std::max_element(cn.begin() + w, cn.begin() + w + WAVE);
        for (int64_t w = 0; w < Wp; w += WAVE) tq[1] += *std::max_element(cp.begin() + w, cp.begin() + w + WAVE);
        sum[0] += tq[0];
        sum[1] += tq[1];
        const double dq = (double)tq[0] - (double)tq[1];
        dsum += dq;
        dsq += dq * dq;
    }
    for (int k = 0; k < 2; ++k) {
        trips[k] = (double)sum[k] / PACK_SAMPLE;
        cost[k] += PACK_TRIP_COST * trips[k];
    }
    const double n = PACK_SAMPLE, mean = dsum / n, var = std::max(0.0, (dsq - n * mean * mean) / (n - 1));
    const double se = std::sqrt(var / n) * PACK_TRIP_COST;
    return cost[0] > 0.0 ? (cost[0] - cost[1] - 2.0 * se) / cost[0] : 0.0;
}

inline bool pack_pays(double gain_low) { return gain_low >= PACK_MIN_GAIN; }
