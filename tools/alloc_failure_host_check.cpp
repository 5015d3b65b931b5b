/* alloc_failure_host_check.cpp -- every host allocation of the context-free entry points, failed in turn.
 *
 * The global operator new (throwing and nothrow) and operator delete (plain and sized) are replaced here by versions over
 * malloc / free that fail the k-th allocation from now on demand.  Each scenario below is a short sequence of calls
 * without a context (every accumulator is created with ctx = NULL; no device is needed or touched); it runs once with
 * nothing armed, then with k = 1, 2, ... until a pass ends in which no failure was injected.  A pass stops at its first
 * call that fails; the destroy runs with the injection switched off.  Required: every pass returns TQ_OK or TQ_ERR_OOM
 * and nothing else; a pass that returned TQ_OK although an allocation failed (something absorbed the failure) and the
 * last pass give the outputs of the unarmed run; and, from the sanitizers this is built with, no report and no leak.
 * The check itself allocates nothing through operator new while a failure is armed.
 *
 * Built and run by tools/host_checks.sh.  ALLOC_FAILURE_TRACE=1 prints the stack of every injected failure that was
 * absorbed (with the address sanitizer's symbolizer).  Prints one line per scenario -- passes, failures that returned
 * TQ_ERR_OOM, failures absorbed -- then "alloc_failure_host_check: ok", and returns 0 when every requirement held. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "tetrad_hip.h"

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/common_interface_defs.h>
#define HAVE_STACK_TRACE 1
#endif
#endif

namespace {

long g_fail_at = 0;         // 0: nothing armed; k: the k-th allocation from the arming fails
long g_seen = 0;
bool g_injected = false, g_trace = false;

void *take(size_t n)
{
    if (g_fail_at && ++g_seen == g_fail_at) {
        g_injected = true;
#ifdef HAVE_STACK_TRACE
        if (g_trace) __sanitizer_print_stack_trace();
#endif
        return nullptr;
    }
    return malloc(n ? n : 1);
}

}  // namespace

void *operator new(size_t n)
{
    if (void *p = take(n)) return p;
    throw std::bad_alloc();
}
void *operator new(size_t n, const std::nothrow_t &) noexcept { return take(n); }
void operator delete(void *p) noexcept { free(p); }
void operator delete(void *p, size_t) noexcept { free(p); }

namespace {

#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            fprintf(stderr, "alloc_failure_host_check: line %d: %s\n", __LINE__, #cond);  \
            exit(1);                                                                      \
        }                                                                                 \
    } while (0)

/* first failure ends the pass */
#define TRY(call)                 \
    do {                          \
        const int rc_ = (call);   \
        if (rc_) return rc_;      \
    } while (0)

/* the outputs of a pass, as bytes in a fixed buffer */
struct Blob {
    unsigned char bytes[1 << 15];
    size_t n = 0;
    void put(const void *p, size_t size)
    {
        CHECK(n + size <= sizeof bytes);
        memcpy(bytes + n, p, size);
        n += size;
    }
    bool equals(const Blob &o) const { return n == o.n && !memcmp(bytes, o.bytes, n); }
};

/* ---- the inputs: T = 9, two caterpillar trees, six quartet rows ---------------------------------------------------- */
constexpr int32_t T = 9;
constexpr int64_t STRIDE = 2 * T, R = 2, Q = 6;
int32_t g_parents[R * STRIDE];
int64_t g_nodes[R];
const uint32_t g_quartets[Q * 4] = {0, 1, 2, 3, 0, 2, 5, 7, 1, 3, 4, 8, 2, 4, 6, 8, 0, 3, 6, 7, 1, 5, 7, 8};
const int32_t g_iquartets[Q * 4] = {0, 1, 2, 3, 0, 2, 5, 7, 1, 3, 4, 8, 2, 4, 6, 8, 0, 3, 6, 7, 1, 5, 7, 8};
const uint32_t g_rstat[Q * 2] = {0, 40, 1, 25, 2, 31, 0, 12, 1, 90, 0, 7};
const double g_rscor[Q * 3] = {0.1, 0.5, 0.7, 0.6, 0.2, 0.9, 0.8, 0.4, 0.05, 0.3, 0.31, 0.9, 0.5, 0.1, 0.6, 0.2, 0.7, 0.8};
uint32_t g_classes[Q * 16];

void caterpillar(const int32_t *order, int32_t *parent, int64_t *n_nodes)
{
    int32_t n = T, cur = order[0];
    for (int32_t i = 1; i < T; ++i) {
        parent[cur] = n;
        parent[order[i]] = n;
        cur = n++;
    }
    parent[cur] = -1;
    *n_nodes = n;
}

void make_inputs()
{
    const int32_t a[T] = {0, 1, 2, 3, 4, 5, 6, 7, 8}, b[T] = {4, 7, 0, 2, 8, 1, 6, 3, 5};
    caterpillar(a, g_parents, &g_nodes[0]);
    caterpillar(b, g_parents + STRIDE, &g_nodes[1]);
    for (int i = 0; i < Q * 16; ++i) g_classes[i] = (uint32_t)((i * 7 + 3) % 23);
}

/* ---- the scenarios: each ends with its accumulator destroyed, whatever it returns ---------------------------------- */
template <class Acc, void (*Destroy)(Acc *)>
struct Owner {
    Acc *p = nullptr;
    ~Owner()
    {
        const long armed = g_fail_at;
        g_fail_at = 0;                  /* destroy with the injection switched off */
        Destroy(p);
        g_fail_at = armed;
    }
};

int cons(Blob &out)
{
    Owner<tq_cons, tq_cons_destroy> a;
    char nwk[512];
    int64_t written = 0;
    TRY(tq_cons_create(&a.p, T, 64, nullptr));
    TRY(tq_cons_add(a.p, g_parents, g_nodes, R, STRIDE, nullptr));
    TRY(tq_cons_tree(a.p, 1, nwk, sizeof nwk, &written));
    out.put(&written, sizeof written);
    out.put(nwk, (size_t)written);
    return TQ_OK;
}

int tbe(Blob &out)
{
    Owner<tq_tbe, tq_tbe_destroy> a;
    uint16_t phi[R * T] = {};
    int64_t E = 0;
    TRY(tq_tbe_create(&a.p, T, g_parents, g_nodes[0], nullptr));
    TRY(tq_tbe_add(a.p, g_parents, g_nodes, R, STRIDE, nullptr, phi));
    TRY(tq_tbe_shape(a.p, nullptr, nullptr, &E, nullptr));
    CHECK(E > 0 && E <= T);
    out.put(phi, (size_t)(R * E) * sizeof phi[0]);
    return TQ_OK;
}

int rf(Blob &out)
{
    Owner<tq_rf, tq_rf_destroy> a;
    int32_t nsplits[R];
    uint32_t shared[R * R], dist[R * R];
    TRY(tq_rf_create(&a.p, T, R, 64, nullptr));
    TRY(tq_rf_add(a.p, g_parents, g_nodes, R, STRIDE, nullptr));
    TRY(tq_rf_read(a.p, nsplits, shared, dist));
    out.put(nsplits, sizeof nsplits);
    out.put(shared, sizeof shared);
    out.put(dist, sizeof dist);
    return TQ_OK;
}

int qd(Blob &out)
{
    Owner<tq_qd, tq_qd_destroy> a;
    uint64_t same[R * R], both[R * R];
    TRY(tq_qd_create(&a.p, T, R, nullptr));
    TRY(tq_qd_add(a.p, g_parents, g_nodes, R, STRIDE, nullptr));
    TRY(tq_qd_score(a.p, g_iquartets, Q, nullptr));
    TRY(tq_qd_read(a.p, same, both));
    out.put(same, sizeof same);
    out.put(both, sizeof both);
    return TQ_OK;
}

int ls(Blob &out)
{
    Owner<tq_ls, tq_ls_destroy> a;
    uint16_t counts[Q * 4];
    uint64_t sums[T * 4];
    TRY(tq_ls_create(&a.p, T, R, nullptr));
    TRY(tq_ls_add(a.p, g_parents, g_nodes, R, STRIDE, nullptr));
    TRY(tq_ls_score(a.p, g_iquartets, Q, counts, nullptr));
    TRY(tq_ls_read(a.p, sums));
    out.put(counts, sizeof counts);
    out.put(sums, sizeof sums);
    return TQ_OK;
}

int conc(Blob &out)
{
    Owner<tq_conc, tq_conc_destroy> a;
    int64_t counts[T * 6], tips[T * 2], skipped = 0, E = 0;
    double sums[T * 2];
    uint64_t masks[T];
    TRY(tq_conc_create(&a.p, g_parents, g_nodes[0], T, 1, 0.0, nullptr));
    TRY(tq_conc_add(a.p, g_quartets, g_rstat, g_rscor, nullptr, Q));
    TRY(tq_conc_shape(a.p, nullptr, &E, nullptr));
    CHECK(E > 0 && E <= T);
    TRY(tq_conc_read(a.p, counts, sums, masks, tips, &skipped));
    out.put(counts, (size_t)E * 6 * 8);
    out.put(sums, (size_t)E * 2 * 8);
    out.put(masks, (size_t)E * 8);
    out.put(tips, sizeof tips);
    out.put(&skipped, sizeof skipped);
    return TQ_OK;
}

int scf(Blob &out)
{
    Owner<tq_scf, tq_scf_destroy> a;
    int64_t counts[T * 8], skipped = 0, E = 0;
    uint64_t masks[T];
    TRY(tq_scf_create(&a.p, g_parents, g_nodes[0], T, nullptr));
    TRY(tq_scf_add(a.p, g_quartets, g_classes, Q));
    TRY(tq_scf_shape(a.p, nullptr, &E, nullptr));
    CHECK(E > 0 && E <= T);
    TRY(tq_scf_read(a.p, counts, masks, &skipped));
    out.put(counts, (size_t)E * 8 * 8);
    out.put(masks, (size_t)E * 8);
    out.put(&skipped, sizeof skipped);
    return TQ_OK;
}

int stree(Blob &out)
{
    Owner<tq_stree, tq_stree_destroy> a;
    char nwk[512];
    int64_t written = 0, levels = 0;
    uint64_t fit[R * 6];
    TRY(tq_stree_create(&a.p, T, 64, 0, 1, 0.0, nullptr));
    TRY(tq_stree_add(a.p, g_quartets, g_rstat, g_rscor, nullptr, Q));
    TRY(tq_stree_build(a.p, 1, nullptr, nwk, sizeof nwk, &written, &levels));
    TRY(tq_stree_fit(a.p, g_parents, g_nodes, R, STRIDE, nullptr, fit));
    out.put(&written, sizeof written);
    out.put(nwk, (size_t)written);
    out.put(&levels, sizeof levels);
    out.put(fit, sizeof fit);
    return TQ_OK;
}

int pack_sites(Blob &out)
{
    constexpr int64_t S = 96;
    uint8_t arr[T * S];
    uint32_t locus[S], src[4096];
    int64_t packed = 0;
    int32_t pays = 0;
    double estimate[5] = {};
    for (int64_t i = 0; i < T * S; ++i) arr[i] = (uint8_t)((i * 5 + i / 7) & 3);
    for (int64_t s = 0; s < S; ++s) locus[s] = (uint32_t)(s / 8);
    TRY(tq_pack_sites(arr, T, S, locus, 1, src, 4096, &packed, &pays, estimate));
    CHECK(packed > 0 && packed <= 4096);
    out.put(&packed, sizeof packed);
    out.put(src, (size_t)packed * 4);
    out.put(&pays, sizeof pays);
    out.put(estimate, sizeof estimate);
    return TQ_OK;
}

int jackknife(Blob &out)
{
    constexpr int64_t SETS = 2, B = 3, N = 2;
    uint32_t rows[SETS * B * 16];
    const uint32_t set_of[N] = {0, 1};
    const uint8_t ia[N] = {1, 2}, ib[N] = {2, 4};
    double res[N * 4] = {};
    for (int i = 0; i < SETS * B * 16; ++i) rows[i] = (uint32_t)((i * 11 + 5) % 37);
    TRY(tq_dstat_jackknife(rows, SETS, B, set_of, ia, ib, N, res));
    out.put(res, sizeof res);
    return TQ_OK;
}

int taxdist(Blob &out)
{
    constexpr int64_t S = 150, B = 2;
    const int64_t starts[B + 1] = {3, 70, 150};
    uint8_t arr[T * S];
    uint32_t counts[B * T * T * 4];
    double dist[T * T];
    int32_t parent[2 * T - 2];
    double length[2 * T - 2];
    for (int64_t i = 0; i < T * S; ++i) arr[i] = (uint8_t)((i * 5 + i / 7) % 5 == 4 ? 78 : (i * 5 + i / 7) % 5);
    TRY(tq_taxon_counts_host(arr, T, S, starts, B, counts));
    for (int64_t i = 0; i < T * T; ++i)        /* p-distances of the two blocks together */
        dist[i] = (double)(counts[4 * i + 1] + counts[4 * (T * T + i) + 1]) / (double)(counts[4 * i] + counts[4 * (T * T + i)]);
    TRY(tq_nj_tree(dist, T, parent, length));
    out.put(counts, sizeof counts);
    out.put(parent, sizeof parent);
    out.put(length, sizeof length);
    return TQ_OK;
}

void sweep(const char *name, int (*scenario)(Blob &))
{
    static Blob want, got;
    want.n = 0;
    g_fail_at = 0;
    CHECK(scenario(want) == TQ_OK);
    long oom = 0, absorbed = 0, k = 0;
    for (;;) {
        got.n = 0;
        g_injected = false;
        g_seen = 0;
        g_fail_at = ++k;
        const int rc = scenario(got);
        g_fail_at = 0;
        if (rc != TQ_OK && rc != TQ_ERR_OOM)
            fprintf(stderr, "alloc_failure_host_check: %s: allocation %ld failed and the pass returned %d: %s\n", name, k, rc,
                    tq_last_error(nullptr));
        CHECK(rc == TQ_OK || rc == TQ_ERR_OOM);
        CHECK(g_injected || rc == TQ_OK);
        if (rc == TQ_OK) {
            if (!got.equals(want))
                fprintf(stderr, "alloc_failure_host_check: %s: the pass of allocation %ld returned TQ_OK with other outputs\n",
                        name, k);
            CHECK(got.equals(want));
        }
        if (!g_injected) break;
        if (rc == TQ_OK) {
            ++absorbed;
            printf("alloc_failure_host_check: %s: allocation %ld failed, the pass returned TQ_OK with the right outputs\n", name, k);
            fflush(stdout);
            if (getenv("ALLOC_FAILURE_TRACE")) {        /* the same pass again, this time showing where */
                got.n = 0;
                g_seen = 0;
                g_fail_at = k;
                g_trace = true;
                (void)scenario(got);
                g_trace = false;
                g_fail_at = 0;
            }
        } else {
            ++oom;
        }
        CHECK(k < 100000);
    }
    printf("alloc_failure_host_check: %-10s %4ld passes, %4ld injected failures returned TQ_ERR_OOM, %ld absorbed\n", name, k,
           oom, absorbed);
}

}  // namespace

int main()
{
    make_inputs();
    sweep("cons", cons);
    sweep("tbe", tbe);
    sweep("rf", rf);
    sweep("qd", qd);
    sweep("ls", ls);
    sweep("conc", conc);
    sweep("scf", scf);
    sweep("stree", stree);
    sweep("pack_sites", pack_sites);
    sweep("jackknife", jackknife);
    sweep("taxdist", taxdist);
    printf("alloc_failure_host_check: ok\n");
    return 0;
}
