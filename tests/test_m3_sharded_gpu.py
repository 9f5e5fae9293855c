"""GPU: the row-sharded bge-m3 search (rag_m3_candidates_gathered_dev, rag_m3_score_ids_dev, rag_m3_combine_gathered_dev and
sharded.ShardedM3Index) against the one-call entries on the unsharded index. One process, three RagEngine handles holding the
unequal shards [0, 4096) / [4096, 10260) / [10260, 10300) of corpus A (the last one has fewer rows than the pool), a fourth
holding the whole corpus; every index is loaded with id_base. The sends of the three handles are stacked as the all-gather stacks
them. Everything is compared EXACTLY: ids, float64 score bits, component bits, candidate lists, on every one of the three ranks."""
import numpy as np
import pytest

import m3_fused_tools as F
import sparse_tools as S

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = r"\(-1\)", r"\(-3\)"
N, POOL, K = F.N_A, F.POOL, 10
BOUNDS = ((0, 4096), (4096, 10260), (10260, N))
DUP_A, DUP_B = 100, 5000                                                 # one embedding in two shards: an exact dense tie
LAST = 10270                                                             # a row of the short shard, queried exactly
T7 = (4200, 4700)                                                        # tenant 7 owns these rows only: all in shard 1
NO_MATCH, NO_VECS = 2, 3                                                 # queries: terms that match nothing / no token vectors
_D = {}


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def data():
    """corpus A's world with the cases the sharded path must get right written into it (see the module constants)"""
    if not _D:
        from optimized_rag_amd.sparse import LexicalPostings
        w, a = F.world(), F.corpus_a()
        emb = np.array(w["emb"])
        emb[DUP_B] = emb[DUP_A]
        q_emb = np.array(w["q_emb"])
        q_emb[0] = emb[DUP_A]
        q_emb[4] = emb[LAST]
        # one document's postings copied into a row of another shard: an exact sparse tie for every query
        sp_a = int(np.argmax(a["all"][1]))
        sp_b = 6000 if sp_a < 4096 else 200
        term_of = np.repeat(np.arange(F.V_A, dtype=np.int64), np.diff(a["indptr"]))
        doc = a["doc"].astype(np.int64)
        keep, src = doc != sp_b, doc == sp_a
        t2 = np.concatenate([term_of[keep], term_of[src]])
        d2 = np.concatenate([doc[keep], np.full(int(src.sum()), sp_b)])
        w2 = np.concatenate([a["w"][keep], a["w"][src]])
        order = np.argsort(t2 * N + d2, kind="stable")
        indptr = np.zeros(F.V_A + 1, dtype=np.int64)
        np.cumsum(np.bincount(t2, minlength=F.V_A), out=indptr[1:])
        post = LexicalPostings(indptr, d2[order].astype(np.int32), np.ascontiguousarray(w2[order]), N)
        queries = list(a["queries"])
        queries[NO_MATCH] = (np.array([F.V_A + 5]), np.array([1.0], np.float32))
        tenants = (np.arange(N) % 3).astype(np.int32)
        tenants[T7[0]:T7[1]] = 7
        _D.update(emb=emb, q_emb=q_emb, post=post, packed=S.pack_queries(queries), tenants=tenants, sp=(sp_a, sp_b), d_vecs=w["d_vecs"],
                  d_off=w["d_off"], qv=w["qv"], qo=w["qo"], per_query=np.array([-1, 0, 1, 2, 7] * 7, np.int32)[:32])
    return _D


def _load(e, lo, hi, form="fp16", sparse=True, tokvec=True, deleted=()):
    """rows [lo, hi) under id_base = lo, with their tenants, postings and token vectors; `deleted` global ids are deleted"""
    from optimized_rag_amd.sharded import ShardedM3Index
    d = data()
    ix = ShardedM3Index(e, rank=0, world=1)
    v = np.array(d["d_vecs"][d["d_off"][lo]:d["d_off"][hi]])
    ix.load_shard(np.array(d["emb"][lo:hi]), lo, d["post"].shard(lo, hi) if sparse else None, v if tokvec else None,
                  (d["d_off"][lo:hi + 1] - d["d_off"][lo]).astype(np.int64) if tokvec else None, form=form)
    e.set_tenants(np.array(d["tenants"][lo:hi]))
    mine = [int(i) for i in deleted if lo <= i < hi]
    if mine:
        assert e.index_delete(np.array(mine, np.int64)) == len(mine)


def _dev():
    import torch
    d = data()
    ptr, terms, wts = d["packed"]
    return dict(q_emb=_t(d["q_emb"]), ptr=_t(ptr), terms=_t(terms), w=_t(wts), qv=_t(d["qv"]), qo=_t(d["qo"]))


@pytest.fixture(scope="module", params=("fp16", "mxfp8"))
def rig(request):
    """dict(whole, shards = three ShardedM3Index of world 3, dev inputs, deleted ids): rows of shard 1 that head query 5's dense
    list and query 6's sparse list are deleted there, and the same global rows on the whole index"""
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.sharded import ShardedM3Index
    d = data()
    engines = [RagEngine(dim=F.DIM, device=0) for _ in range(4)]
    whole = engines[3]
    _load(whole, 0, N, request.param)
    lo, hi = BOUNDS[1]
    d_ids, _, _ = whole.dense_topk(d["q_emb"][5:6], POOL)
    s_ids, _, _ = whole.sparse_topk(*S.pack_queries([F.corpus_a()["queries"][6]]), POOL)
    deleted = [int(i) for i in d_ids[0] if lo <= i < hi and not T7[0] <= i < T7[1]][:2] + [int(i) for i in s_ids[0] if lo <= i < hi][:1]
    assert len(deleted) == 3 and len(set(deleted)) == 3 and not set(deleted) & {DUP_A, DUP_B, *d["sp"]}
    assert whole.index_delete(np.array(deleted, np.int64)) == 3
    shards = []
    for e, (b, t) in zip(engines, BOUNDS):
        _load(e, b, t, request.param, deleted=deleted)
        shards.append(ShardedM3Index(e, rank=len(shards), world=3))
    assert [s.engine.index_deleted_rows() for s in shards] == [0, 3, 0] and whole.index_deleted_rows() == 3
    yield dict(whole=whole, shards=shards, dev=_dev(), deleted=deleted, form=request.param)
    for e in engines:
        e.close()


def _sub(dev, Q):
    """the first Q queries of the device inputs"""
    if Q is None:
        return dev
    return dict(q_emb=dev["q_emb"][:Q].contiguous(), ptr=dev["ptr"][:Q + 1].contiguous(), terms=dev["terms"], w=dev["w"], qv=dev["qv"],
                qo=dev["qo"][:Q + 1].contiguous())


def _sharded(shards, d, mode, weights, tenant=-1, pool=POOL, k=K, lexical=True):
    """the protocol with the two gathers replaced by stacking -> per rank (ids, scores, components, candidates), and rank 0's
    merged lists (ids [2, Q, pool], scores [2, Q, pool])"""
    import torch
    lex = dict(term_ptr=d["ptr"], terms=d["terms"], weights=d["w"]) if lexical else dict(term_ptr=None, terms=None, weights=None)
    recv = torch.stack([s.local_lists(d["q_emb"], lex["term_ptr"], lex["terms"], lex["weights"], pool, k, mode=mode, tenant=tenant).clone()
                        for s in shards])
    cands = [s.candidates_gathered(recv, k, mode=mode).clone() for s in shards]
    slots = cands[0].shape[1]
    b0 = shards[0]._m3_buffers(d["q_emb"].shape[0], pool, slots, k, recv.device)
    lists = (b0["lists"].clone(), b0["scores"].clone())
    recv2 = torch.stack([s.score_local(c, d["q_emb"], lex["term_ptr"], lex["terms"], lex["weights"], d["qv"], d["qo"], pool, k, w=weights).clone()
                         for s, c in zip(shards, cands)])
    out = []
    for s, c in zip(shards, cands):
        r = s.combine_gathered(c, recv2, pool, k, w=weights)
        out.append([r[n].clone() for n in ("ids", "scores", "components", "candidates")])
    torch.cuda.synchronize()
    return out, lists, recv2


def _whole(e, d, mode, weights, tenant=-1, pool=POOL, k=K):
    import torch
    kw = {}
    if mode != 0 or weights[1] > 0:
        kw.update(term_ptr=d["ptr"], terms=d["terms"], weights=d["w"])
    if weights[2] > 0:
        kw.update(q_vecs=d["qv"], q_off=d["qo"])
    out = e.retrieve_m3_dev(d["q_emb"], pool, k, mode=mode, w=weights, tenant=tenant, **kw)
    torch.cuda.synchronize()
    return [x.clone() for x in out]


def _same(got, exp, what):
    g, x = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in exp]
    np.testing.assert_array_equal(g[0], x[0], err_msg=what + ": ids")
    np.testing.assert_array_equal(S.bits(g[1]), S.bits(x[1]), err_msg=what + ": score bits")
    np.testing.assert_array_equal(S.bits(g[2]), S.bits(x[2]), err_msg=what + ": component bits")
    np.testing.assert_array_equal(g[3], x[3], err_msg=what + ": candidates")


def _lists_of(e, d, tenant=-1, pool=POOL):
    """the whole index's own dense and sparse lists at k = pool"""
    import torch
    Q = d["q_emb"].shape[0]
    ids = torch.empty((2, Q, pool), dtype=torch.int64, device="cuda")
    sc = torch.empty((2, Q, pool), dtype=torch.float64, device="cuda")
    e.dense_topk_dev(d["q_emb"], pool, ids[0], None, sc[0], tenant=tenant)
    e.sparse_topk_dev(d["ptr"], d["terms"], d["w"], pool, ids[1], None, sc[1], tenant=tenant)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def test_the_inputs_hold_every_case_the_sharded_path_must_get_right(rig):
    """the preconditions, on the reference lists of the whole index"""
    d = data()
    ids, sc = _lists_of(rig["whole"], rig["dev"])
    shard_of = lambda i: next(r for r, (lo, hi) in enumerate(BOUNDS) if lo <= i < hi)
    assert list(ids[0, 0, :2]) == [DUP_A, DUP_B] and S.bits(sc[0, 0, 0]) == S.bits(sc[0, 0, 1]) and shard_of(DUP_A) != shard_of(DUP_B)
    a, b = sorted(d["sp"])
    pos = list(ids[1, 1]).index(a)
    assert ids[1, 1, pos + 1] == b and S.bits(sc[1, 1, pos]) == S.bits(sc[1, 1, pos + 1]) and sc[1, 1, pos] > 0 and shard_of(a) != shard_of(b)
    assert (ids[1, NO_MATCH] == -1).all() and (sc[1, NO_MATCH] == 0).all(), "a query whose terms match nothing: an all-padding sparse list"
    assert ids[0, 4, 0] == LAST, "the short shard contributes"
    cand = _whole(rig["whole"], rig["dev"], 2, F.WEIGHT_SETS[0])[3].cpu().numpy()
    assert any(not ((cand[q] >= BOUNDS[2][0]) & (cand[q] < N)).any() for q in range(32)), "a query for which one shard contributes no candidate"
    assert d["qo"][NO_VECS] == d["qo"][NO_VECS + 1], "a query without token vectors"
    rows = cand[cand >= 0]
    assert (np.diff(d["d_off"])[rows] == 0).any(), "candidate documents with 0 token rows"
    assert not np.isin(rig["deleted"], ids).any() and not np.isin(rig["deleted"], cand).any(), "deleted rows are hidden"
    ten = d["per_query"]
    assert (ten == 7).sum() >= 6 and (ten == -1).any()
    tc = _whole(rig["whole"], rig["dev"], 2, F.WEIGHT_SETS[0], tenant=ten)[3].cpu().numpy()
    seven = tc[ten == 7]
    assert (seven >= 0).any() and ((seven < 0) | ((seven >= T7[0]) & (seven < T7[1]))).all(), "one tenant's rows lie in a single shard"


@pytest.mark.parametrize("weights", F.WEIGHT_SETS)
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_three_shards_equal_the_one_call_entry(rig, mode, weights):
    exp = _whole(rig["whole"], rig["dev"], mode, weights)
    got, (l_ids, l_sc), recv2 = _sharded(rig["shards"], rig["dev"], mode, weights)
    for r in range(3):
        _same(got[r], exp, f"{rig['form']} mode {mode} weights {weights} rank {r}")
    assert (exp[0].cpu().numpy()[:, 0] >= 0).all()
    # the merged lists are the whole index's own lists
    ids, sc = _lists_of(rig["whole"], rig["dev"])
    n = 1 if mode == 0 else 2
    np.testing.assert_array_equal(l_ids.cpu().numpy()[:n], ids[:n])
    np.testing.assert_array_equal(S.bits(l_sc.cpu().numpy()[:n]), S.bits(sc[:n]))
    if mode == 0:
        assert (l_ids.cpu().numpy()[1] == -1).all() and (l_sc.cpu().numpy()[1] == 0).all()
    # every candidate has exactly one owner, and an unowned slot carries zeros
    part = recv2.cpu().numpy()
    cand = exp[3].cpu().numpy()
    np.testing.assert_array_equal(part[:, 0].sum(axis=0), (cand >= 0).astype(np.int64))
    assert (part[:, 1:][np.broadcast_to(part[:, :1] == 0, part[:, 1:].shape)] == 0).all()


@pytest.mark.parametrize("tenant", ("scalar", "per_query"))
def test_tenants_are_forwarded_to_the_local_searches(rig, tenant):
    ten = 1 if tenant == "scalar" else data()["per_query"]
    for mode in (1, 2):
        exp = _whole(rig["whole"], rig["dev"], mode, F.WEIGHT_SETS[0], tenant=ten)
        got, (l_ids, l_sc), _ = _sharded(rig["shards"], rig["dev"], mode, F.WEIGHT_SETS[0], tenant=ten)
        for r in range(3):
            _same(got[r], exp, f"{rig['form']} tenant {tenant} mode {mode} rank {r}")
        ids, sc = _lists_of(rig["whole"], rig["dev"], tenant=ten)
        np.testing.assert_array_equal(l_ids.cpu().numpy(), ids)
        np.testing.assert_array_equal(S.bits(l_sc.cpu().numpy()), S.bits(sc))


@pytest.mark.parametrize("mode", (0, 1))
def test_late_interaction_equals_retrieve_maxsim(rig, mode):
    import torch
    d = rig["dev"]
    lex = dict(term_ptr=d["ptr"], terms=d["terms"], weights=d["w"]) if mode else {}
    ids, sc, cand = [x.clone() for x in rig["whole"].retrieve_maxsim_dev(d["q_emb"], d["qv"], d["qo"], POOL, K, **lex)]
    torch.cuda.synchronize()
    got, _, _ = _sharded(rig["shards"], d, mode, (0.0, 0.0, 1.0), lexical=bool(mode))
    e_ids = ids.cpu().numpy()
    assert (e_ids[NO_VECS] == -1).all() and ((e_ids >= 0).sum(axis=1) < K).sum() >= 1, "slots without token vectors are left out"
    for r in range(3):
        np.testing.assert_array_equal(got[r][0].cpu().numpy(), e_ids, err_msg=f"rank {r}: ids")
        np.testing.assert_array_equal(S.bits(got[r][1].cpu().numpy()), S.bits(sc.cpu().numpy()), err_msg=f"rank {r}: score bits")
        np.testing.assert_array_equal(got[r][3].cpu().numpy(), cand.cpu().numpy(), err_msg=f"rank {r}: candidates")


def test_a_small_call_after_a_larger_one_reuses_the_workspaces(rig):
    big = _sharded(rig["shards"], rig["dev"], 2, F.WEIGHT_SETS[0])[0]
    small_in = _sub(rig["dev"], 3)
    exp = _whole(rig["whole"], small_in, 1, F.WEIGHT_SETS[0], pool=7, k=3)
    got = _sharded(rig["shards"], small_in, 1, F.WEIGHT_SETS[0], pool=7, k=3)[0]
    for r in range(3):
        _same(got[r], exp, f"small after large, rank {r}")
    again = _sharded(rig["shards"], rig["dev"], 2, F.WEIGHT_SETS[0])[0]
    _same(again[0], big[0], "the larger call again")


def test_world_one_search_equals_the_one_call_entries(rig):
    import torch
    from optimized_rag_amd.sharded import ShardedM3Index
    d, whole = rig["dev"], rig["whole"]
    one = ShardedM3Index(whole, rank=0, world=1)
    for mode in (0, 1, 2):
        exp = _whole(whole, d, mode, F.WEIGHT_SETS[0])
        r = one.search_m3(d["q_emb"], d["ptr"], d["terms"], d["w"], d["qv"], d["qo"], POOL, K, mode=mode)
        torch.cuda.synchronize()
        _same([r[n] for n in ("ids", "scores", "components", "candidates")], exp, f"world 1 mode {mode}")
    ids, sc = _lists_of(whole, d, pool=K)
    l_ids, l_sc = one.search_lexical(d["ptr"], d["terms"], d["w"], K)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(l_ids.cpu().numpy(), ids[1])
    np.testing.assert_array_equal(S.bits(l_sc.cpu().numpy()), S.bits(sc[1]))
    # the sparse list alone over the three shards: one merge of the stacked local lists
    send = torch.stack([torch.stack([s.search_lexical(d["ptr"], d["terms"], d["w"], K)[0].clone(),
                                     s.search_lexical(d["ptr"], d["terms"], d["w"], K)[1].clone().view(torch.int64)])
                        for s in [ShardedM3Index(s.engine, rank=0, world=1) for s in rig["shards"]]])
    out_i = torch.empty((32, K), dtype=torch.int64, device="cuda")
    out_s = torch.empty((32, K), dtype=torch.float64, device="cuda")
    whole.merge_topk_dev(send, send.view(torch.float64)[:, 1], out_i, out_s, n_lists=3, list_stride=2 * 32 * K)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out_i.cpu().numpy(), ids[1])
    np.testing.assert_array_equal(S.bits(out_s.cpu().numpy()), S.bits(sc[1]))


def test_overlapping_owners_resolve_to_the_lowest_rank(rig):
    """two ranks claim slot 0 (a caller error): rank 0's components are taken; a slot nobody owns is empty"""
    import torch
    e = rig["whole"]
    cand = _t(np.array([[11, 12, 13]], np.int64))
    part = np.zeros((2, 4, 1, 3), np.int64)
    f = lambda x: int(np.float64(x).view(np.int64))
    part[0, 0, 0, 0], part[0, 1, 0, 0] = 1, f(0.25)
    part[1, 0, 0, 0], part[1, 1, 0, 0] = 1, f(0.75)
    part[1, 0, 0, 1], part[1, 1, 0, 1] = 1, f(0.5)
    ids = torch.empty((1, 3), dtype=torch.int64, device="cuda")
    sc = torch.empty((1, 3), dtype=torch.float64, device="cuda")
    comp = torch.empty((1, 3, 3), dtype=torch.float64, device="cuda")
    e.m3_combine_gathered_dev(cand, _t(part), ids, sc, comp, w=(1.0, 0.0, 0.0))
    torch.cuda.synchronize()
    assert ids.cpu().tolist() == [[12, 11, -1]] and sc.cpu().tolist() == [[0.5, 0.25, 0.0]]
    assert comp.cpu().tolist() == [[[0.5, 0, 0], [0.25, 0, 0], [0, 0, 0]]]


def test_error_paths_return_their_code_and_leave_the_handle_usable(rig):
    import torch
    from optimized_rag_amd import RagEngine, RagError
    from optimized_rag_amd.sharded import ShardedM3Index
    d, dv = data(), rig["dev"]
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64, device="cuda")
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    whole = rig["whole"]
    with pytest.raises(RagError, match=ERR_ARG):                         # mode 2: pool <= 128
        whole.m3_candidates_gathered_dev(i64(1, 4, 1, 129), i64(2, 1, 129), f64(2, 1, 129), i64(1, 258), mode=2)
    with pytest.raises(RagError, match=ERR_ARG):                         # world * pool > 4092
        whole.m3_candidates_gathered_dev(i64(17, 4, 1, 256), i64(2, 1, 256), f64(2, 1, 256), i64(1, 256), mode=1)
    with pytest.raises(RagError, match=ERR_ARG):                         # the weights' rule
        whole.m3_combine_gathered_dev(i64(1, 4), i64(1, 4, 1, 4), i64(1, 2), f64(1, 2), w=(0.0, 0.0, 0.0))
    exp = _whole(whole, dv, 2, F.WEIGHT_SETS[0])
    _same(_whole(whole, dv, 2, F.WEIGHT_SETS[0]), exp, "the handle after three refusals")
    e = RagEngine(dim=F.DIM, device=0)
    try:
        e.index_load(np.array(d["emb"][:300]), ids=(7 + 2 * np.arange(300)).astype(np.int64))
        with pytest.raises(RagError, match=ERR_STATE):                   # explicit ids: ownership is defined through id_base only
            e.m3_score_ids_dev(i64(32, POOL), i64(4, 32, POOL), q_emb=dv["q_emb"], w=(1.0, 0.0, 0.0))
        assert e.dense_topk(d["q_emb"][:2], 3)[0][0, 0] >= 7
        # no token-vector store: a colbert weight is refused, a weight of 0 needs none - and gives the whole index's bits
        _load(e, 0, N, tokvec=False, deleted=rig["deleted"])
        one = ShardedM3Index(e, rank=0, world=1)
        with pytest.raises(RagError, match=ERR_STATE):
            one.search_m3(dv["q_emb"], dv["ptr"], dv["terms"], dv["w"], dv["qv"], dv["qo"], POOL, K, mode=2)
        r = one.search_m3(dv["q_emb"], dv["ptr"], dv["terms"], dv["w"], None, None, POOL, K, mode=2, w=F.WEIGHT_SETS[1])
        torch.cuda.synchronize()
        _same([r[n] for n in ("ids", "scores", "components", "candidates")], _whole(whole, dv, 2, F.WEIGHT_SETS[1]), "no store, w_colbert = 0")
    finally:
        e.close()
    e = RagEngine(dim=F.DIM, device=0)
    try:
        # no postings: mode 0 with w_sparse = 0 runs no sparse search and needs none
        _load(e, 0, N, form=rig["form"], sparse=False, deleted=rig["deleted"])
        one = ShardedM3Index(e, rank=0, world=1)
        r = one.search_m3(dv["q_emb"], None, None, None, dv["qv"], dv["qo"], POOL, K, mode=0, w=F.WEIGHT_SETS[2])
        torch.cuda.synchronize()
        _same([r[n] for n in ("ids", "scores", "components", "candidates")], _whole(whole, dv, 0, F.WEIGHT_SETS[2]), "no postings, w_sparse = 0")
        with pytest.raises(RagError, match=ERR_STATE):
            one.search_m3(dv["q_emb"], dv["ptr"], dv["terms"], dv["w"], dv["qv"], dv["qo"], POOL, K, mode=0, w=F.WEIGHT_SETS[0])
    finally:
        e.close()
