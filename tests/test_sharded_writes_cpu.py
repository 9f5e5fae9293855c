"""CPU-only, numpy: why writes on row shards are exact. The owner policy is a function of the layout alone; merging the shards'
top-k lists by (score desc, id asc) reproduces the whole corpus when ids ascend with the rows on every shard - and does NOT for a
shard whose ids do not ascend and which holds an exact tie at the k-th place, which is why the shard entries ask the id map for
ids_ascending; the statistics of rag_bm25_refresh are sums of integers, so the shards' sums give the whole corpus's table."""
import numpy as np
import pytest

from optimized_rag_amd.bm25 import Bm25Postings
from optimized_rag_amd.sharded import ShardedDenseIndex


def local_topk(scores, ids, k):
    """what a handle returns: score desc, ties by lower ROW -> (ids, scores)"""
    rows = np.arange(len(scores))
    top = rows[np.lexsort((rows, -scores))[:k]]
    return ids[top], scores[top]


def merged_topk(parts, k):
    """what the merge over shards returns: score desc, ties by lower ID"""
    ids = np.concatenate([p[0] for p in parts])
    sc = np.concatenate([p[1] for p in parts])
    top = np.lexsort((ids, -sc))[:k]
    return ids[top], sc[top]


def test_owner_policy_is_a_function_of_the_layout_alone():
    assert ShardedDenseIndex.owner_of([2100, 2494, 6]) == 2
    assert ShardedDenseIndex.owner_of([5, 5, 5]) == 0                  # ties: the lowest rank
    assert ShardedDenseIndex.owner_of([7, 5, 5]) == 1
    assert ShardedDenseIndex.owner_of([0]) == 0
    # every rank replays the same blocks on its own copy of the layout: the same owners, the same rows, no collective
    rng = np.random.default_rng(0)
    blocks = [int(b) for b in rng.integers(1, 900, 40)]
    copies = [[2100, 2494, 6, 300] for _ in range(4)]
    owners = [[] for _ in copies]
    for n in blocks:
        for rank, rows in enumerate(copies):
            o = ShardedDenseIndex.owner_of(rows)
            rows[o] += n
            owners[rank].append(o)
    assert all(o == owners[0] for o in owners) and all(c == copies[0] for c in copies)
    assert set(owners[0]) == {0, 1, 2, 3} and max(copies[0]) - min(copies[0]) <= max(blocks)


def world(rng, ascending):
    """three shards of a corpus in id order, scores with many exact ties; after deletes and an insert on the shortest shard"""
    n, k = 600, 10
    scores = rng.integers(0, 12, n).astype(np.float64) / 4.0          # few distinct values: ties everywhere
    ids = 7 + 3 * np.arange(n, dtype=np.int64)
    bounds = [(0, 250), (250, 590), (590, 600)]
    shards = [[ids[lo:hi].copy(), scores[lo:hi].copy()] for lo, hi in bounds]
    gone = rng.choice(n, 80, replace=False)
    new_ids = ids[-1] + 3 * np.arange(1, 41)
    new_sc = rng.integers(0, 12, 40).astype(np.float64) / 4.0
    owner = ShardedDenseIndex.owner_of([len(s[0]) for s in shards])
    shards[owner] = [np.concatenate([shards[owner][0], new_ids]), np.concatenate([shards[owner][1], new_sc])]
    whole = [np.concatenate([ids, new_ids]), np.concatenate([scores, new_sc])]
    keep = ~np.isin(whole[0], ids[gone])
    whole = [whole[0][keep], whole[1][keep]]
    shards = [[s[0][~np.isin(s[0], ids[gone])], s[1][~np.isin(s[0], ids[gone])]] for s in shards]
    if not ascending:                                                  # one shard stores its rows in another order than its ids
        p = rng.permutation(len(shards[0][0]))
        shards[0] = [shards[0][0][p], shards[0][1][p]]
    return shards, whole, k


@pytest.mark.parametrize("seed", range(5))
def test_merge_after_writes_equals_the_whole_corpus_when_ids_ascend(seed):
    shards, whole, k = world(np.random.default_rng(seed), ascending=True)
    assert all((np.diff(s[0]) > 0).all() for s in shards) and (np.diff(whole[0]) > 0).all()
    got = merged_topk([local_topk(s[1], s[0], k) for s in shards], k)
    exp = local_topk(whole[1], whole[0], k)
    np.testing.assert_array_equal(got[0], exp[0])
    np.testing.assert_array_equal(got[1], exp[1])
    assert len(np.unique(exp[1])) < k, "the top-k holds exact ties"


def test_merge_differs_when_a_shard_does_not_ascend_and_ties_at_the_kth_place():
    """the counter-example behind the gate: shard 0 holds ids (10, 20, 30) in rows (0, 1, 2) = (30, 10, 20); 30 and 10 tie, k = 1.
    Locally the lower ROW wins (id 30); the whole corpus, in id order, and the merge prefer the lower ID (10), which shard 0 never
    sent."""
    k = 1
    shard0 = (np.array([30, 10, 20], dtype=np.int64), np.array([0.5, 0.5, 0.25]))
    shard1 = (np.array([40, 50], dtype=np.int64), np.array([0.125, 0.0]))
    got = merged_topk([local_topk(shard0[1], shard0[0], k), local_topk(shard1[1], shard1[0], k)], k)
    order = np.argsort(np.concatenate([shard0[0], shard1[0]]))
    whole_ids = np.concatenate([shard0[0], shard1[0]])[order]
    whole_sc = np.concatenate([shard0[1], shard1[1]])[order]
    exp = local_topk(whole_sc, whole_ids, k)
    assert exp[0].tolist() == [10] and got[0].tolist() == [30]
    # the same shard with ids ascending: equal again
    s = np.argsort(shard0[0])
    got = merged_topk([local_topk(shard0[1][s], shard0[0][s], k), local_topk(shard1[1], shard1[0], k)], k)
    assert got[0].tolist() == exp[0].tolist()


def test_sharded_statistics_sums_give_the_table_of_the_whole_corpus():
    rng = np.random.default_rng(3)
    texts = [" ".join(f"t{int(t)}" for t in rng.zipf(1.4, int(rng.integers(1, 30))) if t < 400) or "t1" for _ in range(900)]
    whole = Bm25Postings.from_corpus(texts)
    live = rng.uniform(size=900) > 0.2
    V = whole.indptr.shape[0] - 1
    term_of = np.repeat(np.arange(V), np.diff(whole.indptr))
    total = np.zeros(V + 2, dtype=np.int64)
    for lo, hi in ((0, 400), (400, 893), (893, 900)):
        # a rank's counts: df of every term over its live documents (a rank that never saw the last terms pads with zeros)
        sel = (whole.doc >= lo) & (whole.doc < hi) & live[whole.doc]
        df = np.bincount(term_of[sel], minlength=V)
        known = int(np.nonzero(df)[0].max()) + 1 if df.any() else 0
        mine = np.zeros(V + 2, dtype=np.int64)
        mine[:known] = df[:known]
        mine[-2:] = (live[lo:hi].sum(), whole.doc_len[lo:hi][live[lo:hi]].sum())
        total += mine
    idf, mean = Bm25Postings.idf_of_counts(total[:-2], int(total[-2]))
    avgdl = int(total[-1]) / int(total[-2])
    exp = Bm25Postings.from_corpus(texts).refresh(live)
    np.testing.assert_array_equal(idf.view(np.int64), exp.idf.view(np.int64))
    assert avgdl == exp.avgdl and mean == exp._frozen_mean
    # ... which, with every document live, is the table a rebuild computes
    idf_all, _ = Bm25Postings.idf_of_counts(np.diff(whole.indptr), 900)
    np.testing.assert_array_equal(idf_all.view(np.int64), whole.idf.view(np.int64))
