"""TEST INFRASTRUCTURE: inputs on which every float64 sum the small kernels form is EXACT, so that neither the order of a parallel
reduction nor CPython's left-to-right sum rounds anything and a kernel must agree with oracle/rag_oracle.py bit for bit
(tests/test_small_kernels_gpu.py); tests/test_oracle_golden.py checks the recipe itself on the CPU.

Why the sums are exact
  * MMR: embeddings with integer entries in [-3, 3]. Every product is an integer of magnitude <= 9, every partial sum an integer
    below 9 * dim < 2**53: dot products and squared norms are exact in ANY order. sqrt and the one division are correctly rounded
    on both sides, the score expression has the same association on both sides.
  * chunk chain: the running embedding is halved at each join, so it gains one fractional bit per join. All sentence lengths are
    10, max_chunk 90 and min_chunk 25: a chunk holds at most 9 sentences (8 joins), entries are multiples of 2**-8 of magnitude
    <= 3, squares multiples of 2**-16 <= 9, and a sum of 8192 of them needs at most 17 + 16 = 33 bits. Without the cap (24 joins
    in a row) dim 8192 does become order-dependent.
Each GPU test still asserts its precondition (identical similarities under a permuted summation order) on the very input it uses.
"""
import math

import numpy as np

CHAIN_DIMS = [1, 3, 64, 255, 256, 257, 1536, 4096, 8192]
CHAIN_LEN, CHAIN_MAX, CHAIN_MIN, CHAIN_N = 10, 90, 25, 40


def int_vectors(rng, n, dim, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, (n, dim)).astype(np.float32)


def exact_chain(seed, dim, n=CHAIN_N):
    """n sentence embeddings with integer entries in [-3, 3]: three cluster centres with entries in [-2, 2] plus noise in
    {-1, 0, 1} on a quarter of the coordinates, the cluster changing every 1..6 sentences - similar neighbours join, a change of
    cluster splits. Returns (embs float32 [n, dim], sent_len int32 [n])."""
    rng = np.random.default_rng([seed, dim])
    centres = rng.integers(-2, 3, (3, dim))
    which, c = [], 0
    while len(which) < n:
        which += [c] * int(rng.integers(1, 7))
        c = (c + int(rng.integers(1, 3))) % 3
    noise = rng.integers(-1, 2, (n, dim)) * (rng.random((n, dim)) < 0.25)
    embs = (centres[which[:n]] + noise).astype(np.float32)
    assert np.abs(embs).max() <= 3
    return embs, np.full(n, CHAIN_LEN, dtype=np.int32)


def chain_hinges(groups, sent_len, max_chunk, min_chunk):
    """hinge[i - 1] = True when the similarity alone decided sentence i: the chunk before it had reached min_chunk and had room."""
    out, size = [], int(sent_len[0])
    for i in range(1, len(groups)):
        out.append(size >= min_chunk and size + int(sent_len[i]) <= max_chunk)
        size = size + int(sent_len[i]) if groups[i] == groups[i - 1] else int(sent_len[i])
    return out


def deciding_threshold(groups, sims, sent_len, max_chunk, min_chunk):
    """The smallest similarity that joined a sentence at a hinge in a run of the chain (None if there is none). Run again with
    THIS value as the threshold, every hinge that joined still joins (its similarity is >= it) and every hinge that split had a
    similarity below the first run's threshold, hence below this one: the chain repeats exactly, one sentence now sits exactly
    on the threshold, and `>` in place of `>=` (or the next float above as threshold) splits there."""
    h = chain_hinges(groups, sent_len, max_chunk, min_chunk)
    joined = [sims[i - 1] for i in range(1, len(groups)) if h[i - 1] and groups[i] == groups[i - 1]]
    return min(joined) if joined else None


def next_up(x):
    return math.nextafter(x, math.inf)


def ulps(got, exp):
    """|got - exp| in units of the last place of exp (float64 arrays)."""
    got = np.asarray(got, dtype=np.float64)
    exp = np.asarray(exp, dtype=np.float64)
    return np.abs(got - exp) / np.spacing(np.abs(exp))


def clustered_sentences(rng, n, dim, n_centres=3, noise=0.6):
    """Gaussian sentence embeddings around a few centres (plain Gaussian vectors are nearly orthogonal at dim 1536 and would never
    join): float32 [n, dim]."""
    centres = rng.standard_normal((n_centres, dim))
    which, c = [], 0
    while len(which) < n:
        which += [c] * int(rng.integers(1, 5))
        c = (c + int(rng.integers(1, n_centres))) % n_centres
    return (centres[which[:n]] + noise * rng.standard_normal((n, dim))).astype(np.float32)
