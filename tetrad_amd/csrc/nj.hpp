// nj.hpp -- (host) neighbour joining on a distance matrix.  No reference counterpart.
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace).
//
// One rule (Saitou & Nei 1987 with the Q criterion of Studier & Keppler 1988), f64 throughout; every floating operation
// is one correctly rounded operation in the order written (contraction is off for the function, as for
// dstat_jackknife_row), so a model in plain Python floats agrees bit for bit.
//   nodes   0 .. T - 1 are the taxa, new nodes get T, T + 1, ...; the active list is kept in ascending node id
//   round   (n > 3 active nodes)  r_i = the sum of d(i, k) over the active k != i in ascending id, recomputed every round;
//           Q(i, j) = ((n - 2) d(i, j) - r_i) - r_j; the pair with the smallest Q is joined, ties to the lexicographically
//           lowest (i, j), i < j.  New node u: l_i = 0.5 d(i, j) + (r_i - r_j) / (2 (n - 2)), l_j = d(i, j) - l_i,
//           d(u, k) = 0.5 ((d(i, k) + d(j, k)) - d(i, j)) for every other active k; u is appended to the list.
//   end     (n = 3) the active i < j < k become children of the last node, 2 T - 3, with l_i = 0.5 ((d_ij + d_ik) - d_jk),
//           l_j = 0.5 ((d_ij + d_jk) - d_ik), l_k = 0.5 ((d_ik + d_jk) - d_ij).
// parent i32[2 T - 2] (parent[root] = -1), length f64[2 T - 2] (the root's 0); negative lengths are returned as computed.
// O(T^3) time, (2 T - 3)^2 doubles of memory.
#pragma once

// dist f64[T][T], T >= 3, checked by the caller (finite and symmetric off the diagonal, which is ignored)
inline void nj_host_tree(const double *dist, int64_t T, int32_t *parent, double *length)
{
#pragma clang fp contract(off)
    const int64_t M = 2 * T - 3;                // every node but the root has distances
    std::vector<double> D((size_t)(M * M), 0.0), r((size_t)M, 0.0);
    for (int64_t i = 0; i < T; ++i)
        for (int64_t j = 0; j < T; ++j) D[(size_t)(i * M + j)] = i == j ? 0.0 : dist[i * T + j];
    std::vector<int64_t> act((size_t)T);
    for (int64_t i = 0; i < T; ++i) act[(size_t)i] = i;
    for (int64_t v = 0; v < 2 * T - 2; ++v) {
        parent[v] = -1;
        length[v] = 0.0;
    }
    int64_t next = T;
    while (act.size() > 3) {
        const int64_t n = (int64_t)act.size();
        for (int64_t i : act) {
            double s = 0.0;
            for (int64_t k : act)
                if (k != i) s = s + D[(size_t)(i * M + k)];
            r[(size_t)i] = s;
        }
        const double n2 = (double)(n - 2);
        size_t ba = 0, bb = 1;
        double bq = 0.0;
        bool have = false;
        for (size_t a = 0; a < act.size(); ++a)
            for (size_t b = a + 1; b < act.size(); ++b) {
                const int64_t i = act[a], j = act[b];
                const double p = n2 * D[(size_t)(i * M + j)];
                const double q = (p - r[(size_t)i]) - r[(size_t)j];
                if (!have || q < bq) {
                    have = true;
                    bq = q;
                    ba = a;
                    bb = b;
                }
            }
        const int64_t i = act[ba], j = act[bb], u = next++;
        const double dij = D[(size_t)(i * M + j)];
        const double half = 0.5 * dij;
        const double rd = r[(size_t)i] - r[(size_t)j];
        const double den = 2.0 * n2;
        const double corr = rd / den;
        const double li = half + corr;
        const double lj = dij - li;
        parent[i] = (int32_t)u;
        parent[j] = (int32_t)u;
        length[i] = li;
        length[j] = lj;
        for (int64_t k : act) {
            if (k == i || k == j) continue;
            const double s = D[(size_t)(i * M + k)] + D[(size_t)(j * M + k)];
            const double e = s - dij;
            const double duk = 0.5 * e;
            D[(size_t)(u * M + k)] = duk;
            D[(size_t)(k * M + u)] = duk;
        }
        act.erase(act.begin() + (ptrdiff_t)bb);     // bb > ba: the earlier index stays valid
        act.erase(act.begin() + (ptrdiff_t)ba);
        act.push_back(u);
    }
    const int64_t i = act[0], j = act[1], k = act[2], root = 2 * T - 3;
    const double dij = D[(size_t)(i * M + j)], dik = D[(size_t)(i * M + k)], djk = D[(size_t)(j * M + k)];
    const double si = dij + dik, sj = dij + djk, sk = dik + djk;
    const double ei = si - djk, ej = sj - dik, ek = sk - dij;
    parent[i] = parent[j] = parent[k] = (int32_t)root;
    length[i] = 0.5 * ei;
    length[j] = 0.5 * ej;
    length[k] = 0.5 * ek;
}
