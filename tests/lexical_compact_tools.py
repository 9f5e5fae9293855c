"""Reference and cases for rag_lexical_compact_* (a text's per-position lexical weights -> its sorted sparse vector), shared by
tests/test_lexical_compact_cpu.py (the reference against the Python path: m3_tools.lexical_map + LexicalPostings.encode_queries)
and tests/test_lexical_compact_gpu.py (the kernel against the reference, bit for bit).

The reference is written without the kernel's device: no sort of (id, weight) keys, but numpy's unique + maximum.at per text."""
import numpy as np

INT32_MAX = 2**31 - 1
SUBNORMAL = np.float32(1e-41)                     # a float32 subnormal: kept (it is > 0)
SEQ_LENS = (1, 2, 5, 33, 64, 65, 257, 300, 1025, 8192)
N_TEXTS = (1, 64, 65, 1024, 1025)                 # at seq_len 8: the scan crosses a wave, a workgroup, its own per-thread loop
SKIP8 = (0, 1, 2, 3, 7, 11, 13, 17)
# every class of the issue's list; test_lexical_compact_cpu.py checks that cases() reaches each of them
CLASSES = {f"seq_len_{L}" for L in SEQ_LENS} | {f"n_texts_{n}" for n in N_TEXTS} | {
    "len_0", "len_over_seq_len", "all_special_middle", "all_special_last", "one_id_max_first", "one_id_max_middle", "one_id_max_last",
    "equal_maxima", "weight_classes", "ids_0_and_int32_max", "id_negative", "n_skip_0", "n_skip_8"}


def compact(ids, weights, lens, skip=()):
    """(term_ptr int32 [n + 1], terms int32, qweights float32): for text i the positions t < clamp(lens[i], 0, L) whose id is >= 0 and
    not in `skip` and whose weight is > 0; each distinct id once, ascending, with the largest weight it carries."""
    ids, weights = np.asarray(ids, dtype=np.int32), np.asarray(weights, dtype=np.float32)
    n, L = ids.shape
    ptr = np.zeros(n + 1, dtype=np.int64)
    terms, qw = [], []
    skip = np.asarray(sorted(set(int(s) for s in skip)), dtype=np.int32)
    for i in range(n):
        m = int(np.clip(int(lens[i]), 0, L))
        a, w = ids[i, :m], weights[i, :m]
        with np.errstate(invalid="ignore"):
            keep = (a >= 0) & (w > 0) & ~np.isin(a, skip)
        a, w = a[keep], w[keep]
        u, inv = np.unique(a, return_inverse=True)
        best = np.full(u.shape[0], -np.inf, dtype=np.float32)
        np.maximum.at(best, inv, w)
        terms.append(u.astype(np.int32))
        qw.append(best)
        ptr[i + 1] = ptr[i] + u.shape[0]
    return (ptr.astype(np.int32), np.concatenate(terms).astype(np.int32) if terms else np.zeros(0, np.int32),
            np.concatenate(qw).astype(np.float32) if qw else np.zeros(0, np.float32))


def random_texts(rng, n, L, vocab, lens=None, zero_share=0.3):
    """ids from a vocabulary small enough to repeat, float32 weights of which a share is 0; positions past a length hold junk that
    must not be read as content (a large id with a large weight)"""
    ids = rng.integers(0, vocab, (n, L)).astype(np.int32)
    w = rng.random((n, L)).astype(np.float32)
    w[rng.random((n, L)) < zero_share] = 0.0
    lens = rng.integers(0, L + 1, n).astype(np.int32) if lens is None else np.asarray(lens, dtype=np.int32)
    past = np.arange(L)[None, :] >= np.clip(lens, 0, L)[:, None]
    ids[past] = vocab + 5
    w[past] = 9.0
    return ids, w, lens


def _case(name, ids, w, lens, skip, classes):
    return dict(name=name, ids=np.ascontiguousarray(ids, dtype=np.int32), weights=np.ascontiguousarray(w, dtype=np.float32),
                lens=np.ascontiguousarray(lens, dtype=np.int32), skip=tuple(skip), classes=set(classes))


def cases():
    """The list of cases: dict(name, ids [n, L], weights [n, L], lens [n], skip, classes)."""
    rng = np.random.default_rng(20260)
    out = []
    for j, L in enumerate(SEQ_LENS):
        n = 2 if L == 8192 else 4
        lens = rng.integers(0, L + 1, n)
        lens[0] = L                                                     # one text fills the row
        ids, w, lens = random_texts(rng, n, L, vocab=max(4, L // 3), lens=lens)
        ids += 4                                                        # half of SKIP8 lies below every id: not everything is skipped
        skip = SKIP8 if j % 2 else ()
        out.append(_case(f"seq_len_{L}", ids, w, lens, skip, {f"seq_len_{L}", "n_skip_8" if skip else "n_skip_0"}))
    # text shapes, at a length that is no power of two
    L = 33
    ids, w, lens = random_texts(rng, 9, L, vocab=40, lens=[0, 40, 20, 0, L, L, L, 12, 9])
    special = np.asarray(SKIP8, dtype=np.int32)
    ids[2, :20] = special[rng.integers(0, 8, 20)]                       # all special tokens, in the middle (count 0)
    w[2, :20] = 1.0
    lens[3] = 17                                                        # one id repeated with equal maxima
    ids[3, :17], w[3, :17] = 21, 0.25
    w[3, [2, 9, 16]] = 0.75
    for row, at in ((4, 0), (5, L // 2), (6, L - 1)):                   # one id L times, the maximum first / in the middle / last
        ids[row], w[row] = 30, rng.random(L).astype(np.float32) * 0.5
        w[row, at] = 0.875
    ids[8, :9] = special[rng.integers(0, 8, 9)]                         # ... and as the last text
    w[8, :9] = 2.0
    out.append(_case("text_shapes", ids, w, lens, SKIP8,
                     {"len_0", "len_over_seq_len", "all_special_middle", "all_special_last", "one_id_max_first", "one_id_max_middle",
                      "one_id_max_last", "equal_maxima", "n_skip_8"}))
    # weight classes and the ends of the id range in one text; a negative id
    L = 16
    ids = np.zeros((2, L), dtype=np.int32)
    w = np.zeros((2, L), dtype=np.float32)
    ids[0] = [50, 51, 52, 53, 54, 55, 56, 0, INT32_MAX, INT32_MAX, 0, -1, -7, 54, 53, 50]
    w[0] = [0.0, -0.0, -1.0, np.nan, np.inf, SUBNORMAL, 3e38, 0.5, 0.125, 0.25, 0.75, 4.0, 1.0, 3e38, 2.0, SUBNORMAL]
    ids[1] = ids[0][::-1]
    w[1] = w[0][::-1]
    out.append(_case("values_and_id_range", ids, w, [L, L - 1], (),
                     {"weight_classes", "ids_0_and_int32_max", "id_negative", "n_skip_0"}))
    for n in N_TEXTS:
        ids, w, lens = random_texts(rng, n, 8, vocab=6)
        out.append(_case(f"n_texts_{n}", ids, w, lens, (1,), {f"n_texts_{n}"}))
    return out
