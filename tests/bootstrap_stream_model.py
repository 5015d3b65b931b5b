"""TEST INFRASTRUCTURE: the random stream of the device bootstrap (csrc/bootstrap.hpp), restated in NumPy uint64 arithmetic.

THIS FILE IS THE DEFINITION OF THE DEVICE STREAM.  tests/test_gpu_bootstrap_layout.py requires tq_bootstrap to produce,
bit for bit, the replicate `replicate` returns here, so a change to a constant, to the order of the hash inputs or to
the shuffle -- here or in the kernels -- changes every seeded replicate a user has produced, and fails that test.  The
statistics of the stream (tests/test_bootstrap_stream_cpu.py) are checked on this model and hold for the device through
that equality.

The stream: `mix64` is the splitmix64 step (add the golden-ratio constant, then the finaliser).  The columns of the
locus drawn at ordinal i are shuffled by Fisher-Yates, j = w .. 2, with state_0 = mix64(seed_shuffle ^ i * SHUFFLE_MUL),
state <- mix64(state) per step and r = ((state >> 32) * j) >> 32; p[j-1] and p[r] are swapped.  Cell (t, s) of the
replicate resolves an IUPAC two-base code by the top bit of mix64(seed_ambig ^ t * TAXON_MUL ^ s * SITE_MUL): set = the
first base of GETCONS, clear = the second.  A, C, G, T (or bytes 0..3) become 0..3; every other byte is missing, 78."""
import numpy as np

U = np.uint64
GOLDEN, M1, M2 = U(0x9E3779B97F4A7C15), U(0xBF58476D1CE4E5B9), U(0x94D049BB133111EB)
SHUFFLE_MUL, TAXON_MUL, SITE_MUL = U(0xD1342543DE82EF95), GOLDEN, U(0xC2B2AE3D27D4EB4F)
# ambiguity code, base on coin 1, base on coin 0 (R K S Y W M)
GETCONS = ((82, 71, 65), (75, 71, 84), (83, 71, 67), (89, 84, 67), (87, 84, 65), (77, 67, 65))


def mix64(x):
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=U) + GOLDEN
        x = (x ^ (x >> U(30))) * M1
        x = (x ^ (x >> U(27))) * M2
    return x ^ (x >> U(31))


def shuffles(widths, seed_shuffle):
    """perm[i] = the order in which the columns 0..w-1 of the locus drawn at ordinal i appear (i64[w] each)."""
    widths = np.asarray(widths, dtype=np.int64)
    out = [None] * len(widths)
    with np.errstate(over="ignore"):
        state0 = mix64(U(seed_shuffle) ^ (np.arange(len(widths), dtype=U) * SHUFFLE_MUL))
    for w in np.unique(widths):                       # every ordinal of one width at once
        who = np.flatnonzero(widths == w)
        p = np.tile(np.arange(w, dtype=np.int64), (len(who), 1))
        state, rows = state0[who], np.arange(len(who))
        for j in range(int(w), 1, -1):
            state = mix64(state)
            r = (((state >> U(32)) * U(j)) >> U(32)).astype(np.int64)
            last, other = p[:, j - 1].copy(), p[rows, r].copy()
            p[:, j - 1], p[rows, r] = other, last
        for k, i in enumerate(who):
            out[i] = p[k]
    return out


def coins(T, S, seed_ambig):
    """u8[T,S]: the coin of every cell."""
    with np.errstate(over="ignore"):
        h = U(seed_ambig) ^ (np.arange(T, dtype=U) * TAXON_MUL)[:, None] ^ (np.arange(S, dtype=U) * SITE_MUL)[None, :]
    return (mix64(h) >> U(63)).astype(np.uint8)


def replicate(seqarr, spans, lidxs, seed_shuffle, seed_ambig):
    """(tmparr u8[T,S] of 0..3 / 78, tmpmap u32[S,2]) as tq_bootstrap + tq_get_data return them."""
    seqarr, spans, lidxs = np.asarray(seqarr, np.uint8), np.asarray(spans, np.int64).reshape(-1, 2), np.asarray(lidxs)
    widths = spans[lidxs, 1] - spans[lidxs, 0]
    perm = shuffles(widths, seed_shuffle)
    src_col = np.concatenate([spans[l, 0] + p for l, p in zip(lidxs, perm)])
    S = int(widths.sum())
    v = seqarr[:, src_col]
    coin = coins(seqarr.shape[0], S, seed_ambig) != 0
    for amb, one, zero in GETCONS:
        v = np.where(v == amb, np.where(coin, one, zero), v).astype(np.uint8)
    tmparr = np.full(v.shape, 78, np.uint8)
    for byte, code in ((65, 0), (67, 1), (71, 2), (84, 3), (0, 0), (1, 1), (2, 2), (3, 3)):
        tmparr[v == byte] = code
    tmpmap = np.stack([np.repeat(np.arange(len(lidxs)), widths), np.arange(S)], axis=1).astype(np.uint32)
    return tmparr, tmpmap
