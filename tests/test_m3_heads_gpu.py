"""GPU: the embedder's token-vector and lexical heads (rag_embed_heads_load_host, rag_embed_multi_*) and their pair scores
(rag_maxsim_*, rag_lexical_match_*) against the float64 reference of tests/m3_tools.py, itself held to an independent torch
restatement by tests/test_m3_heads_cpu.py. Bars: token vectors |d| < 1e-3 per component and 1 - cos < 1e-6 per row, row norms
within 1e-5 of 1 (the project's bars for unit vectors, tests/test_embeddings_gpu.py); lexical weights |d| < 2e-3 * |lex_w|_1 (its
bar for a raw hidden component times the head's l1 norm, seeded to 1); MaxSim |d| < 1e-4 on float32 unit vectors (3 * 2^-22 operand
error + 1024 * 2^-24 accumulation = 6.2e-5); lexical match relative 1e-6; every contract clause bit-exact."""
import numpy as np
import pytest

import m3_tools as M
import stream_tools as T
import xlmr_tools as X
from oracle import bert_oracle as B

pytestmark = pytest.mark.gpu

LENS = [1, 2, 15, 16, 17, 33, 64]
L = 64
MODELS = {
    # the split forward with 64-wide attention (and the streamed length class 768 for the long text)
    "h128x64": dict(vocab_size=500, hidden=128, layers=2, heads=2, ffn=256, max_pos=768, type_vocab=2, eps=1e-12),
    "h256x32": dict(vocab_size=500, hidden=256, layers=2, heads=8, ffn=512, max_pos=128, type_vocab=2, eps=1e-12),
    "h384mx": dict(vocab_size=500, hidden=384, layers=2, heads=12, ffn=768, max_pos=128, type_vocab=2, eps=1e-12),      # the MX forward
}
CASES = [("h128x64", 128), ("h128x64", 32), ("h256x32", 256), ("h256x32", 96), ("h384mx", 384), ("h384mx", 96)]
_CACHE = {}


def _texts(cfg, seed=3):
    rng = np.random.default_rng(seed)
    lens = np.array(LENS, dtype=np.int32)
    ids = rng.integers(5, cfg["vocab_size"], (len(lens), L)).astype(np.int32)
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    return ids, np.zeros_like(ids), lens


def _model(name):
    """(cfg, weights, engine with the encoder loaded ([CLS] pooling, normalised), texts, float64 last hidden state): once per model"""
    if name not in _CACHE:
        from optimized_rag_amd import RagEngine
        from optimized_rag_amd.cross_encoder import flatten_state_dict
        cfg = MODELS[name]
        w = B.seeded_weights(cfg, 40 + len(name))
        eng = RagEngine(dim=cfg["hidden"], device=0)
        eng.embed_load(cfg, flatten_state_dict(w, cfg["layers"], head=False), normalize=True, pooling="cls")
        _CACHE[name] = (cfg, w, eng, _texts(cfg))
    return _CACHE[name]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for _, _, eng, _ in _CACHE.values():
        eng.close()
    _CACHE.clear()


def _multi_dev(eng, ids, tt, lens, tok_dim, cap=None, dense=True, lex=True, tok=True, stream=None):
    """rag_embed_multi_dev on numpy inputs with every output poisoned first -> numpy (dense, lex, tok [cap], row_off)"""
    import torch
    n, Ls = ids.shape
    total = int((np.clip(lens, 1, Ls) - 1).sum())
    cap = total if cap is None else cap
    d = torch.full((n, eng.embed_hidden), float("nan"), device="cuda") if dense else None
    lx = torch.full((n, Ls), float("nan"), device="cuda") if lex else None
    tk = torch.full((max(cap, 1), tok_dim), float("nan"), device="cuda")[:cap] if tok else None
    off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    eng.embed_multi_dev(torch.from_numpy(ids).cuda(), torch.from_numpy(tt).cuda(), torch.from_numpy(lens).cuda(), dense=d, lex=lx, tok=tk,
                        row_off=off, stream=stream)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (d, lx, tk, off))


def _check_heads(got_tok, got_lex, ref, lens, what, tok_bar=(1e-3, 1e-6), lex_bar=2e-3):
    exp = np.concatenate(ref["vecs"])
    assert got_tok.shape == exp.shape and np.isfinite(got_tok).all()
    d_tok = float(np.abs(got_tok - exp).max())
    cos = float((1.0 - (got_tok.astype(np.float64) * exp).sum(1)).max())
    nrm = float(np.abs(np.linalg.norm(got_tok.astype(np.float64), axis=1) - 1.0).max())
    d_lex = float(np.abs(got_lex - ref["lex"]).max())
    print(f"{what}: token vectors max |d| = {d_tok:.3e}, max 1 - cos = {cos:.3e}, max |norm - 1| = {nrm:.3e}; lexical max |d| = {d_lex:.3e}")
    assert d_tok < tok_bar[0] and cos < tok_bar[1] and nrm < 1e-5
    assert d_lex < lex_bar
    return d_tok, cos, d_lex


@pytest.mark.parametrize("name,tok_dim", CASES)
def test_heads_against_the_float64_reference(name, tok_dim):
    import torch
    cfg, w, eng, (ids, tt, lens) = _model(name)
    heads = M.seeded_heads(cfg["hidden"], tok_dim, 7 + tok_dim, bias=tok_dim != 96)            # the 96-wide head has no bias
    assert abs(float(np.abs(heads["lex_w"].astype(np.float64)).sum()) - 1.0) < 1e-6
    eng.embed_heads_load(**heads)
    ref = M.heads_reference(w, cfg, ids, tt, lens, heads)
    dense, lex, tok, off = _multi_dev(eng, ids, tt, lens, tok_dim)
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(lens - 1)]))             # a text of length 1 has no rows
    assert off[1] == 0 and tok.shape == (int((lens - 1).sum()), tok_dim)
    assert (lex[np.arange(L)[None, :] >= lens[:, None]] == 0).all() and (lex[np.arange(L)[None, :] < lens[:, None]] >= 0).all()
    assert (ref["lex"] > 0).any()
    _check_heads(tok, lex, ref, lens, f"{name} tok_dim {tok_dim}")
    # dense_out: the bits of rag_embed_dev; the host form: the bits of the device form
    out = torch.full((len(lens), cfg["hidden"]), float("nan"), device="cuda")
    eng.embed_dev(torch.from_numpy(ids).cuda(), torch.from_numpy(tt).cuda(), torch.from_numpy(lens).cuda(), out)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dense, out.cpu().numpy())
    assert np.abs(dense - ref["dense"]).max() < 1e-3
    hd, hl, ht, ho = eng.embed_multi(ids, tt, lens)
    for a, b in ((hd, dense), (hl, lex), (ht, tok), (ho, off)):
        np.testing.assert_array_equal(a, b)


def test_a_600_token_text_in_the_streamed_length_class():
    cfg, w, eng, _ = _model("h128x64")
    heads = M.seeded_heads(128, 128, 11)
    eng.embed_heads_load(**heads)
    rng = np.random.default_rng(8)
    ids = rng.integers(5, cfg["vocab_size"], (1, 600)).astype(np.int32)
    tt, lens = np.zeros_like(ids), np.array([600], dtype=np.int32)
    assert eng.ce_length_class(64, 600) == 768
    ref = M.heads_reference(w, cfg, ids, tt, lens, heads)
    dense, lex, tok, off = _multi_dev(eng, ids, tt, lens, 128)
    assert off.tolist() == [0, 599]
    _check_heads(tok, lex, ref, lens, "h128x64 600 tokens")
    assert np.abs(dense - ref["dense"]).max() < 1e-3


@pytest.mark.parametrize("name,tok_dim", [("h128x64", 32), ("h256x32", 96), ("h384mx", 384)])
def test_outputs_of_a_text_do_not_depend_on_the_call(name, tok_dim):
    """bit-identical across seq_len 64 and 128, alone or among others, and a forced chunk split (one text per chunk)"""
    cfg, w, eng, (ids, tt, lens) = _model(name)
    eng.embed_heads_load(**M.seeded_heads(cfg["hidden"], tok_dim, 5, bias=tok_dim != 96))
    base = _multi_dev(eng, ids, tt, lens, tok_dim)
    wide = np.zeros((len(lens), 128), dtype=np.int32)
    wide[:, :L] = ids
    eng.set_option("ce_chunk_tokens", 64)
    try:
        split = _multi_dev(eng, ids, tt, lens, tok_dim)
    finally:
        eng.set_option("ce_chunk_tokens", 0)
    w128 = _multi_dev(eng, wide, np.zeros_like(wide), lens, tok_dim)
    for other, what in ((split, "chunk split"), (w128, "seq_len 128")):
        np.testing.assert_array_equal(other[0], base[0], err_msg=what)
        np.testing.assert_array_equal(other[1][:, :L], base[1], err_msg=what)
        assert (other[1][:, L:] == 0).all()
        np.testing.assert_array_equal(other[2], base[2], err_msg=what)
        np.testing.assert_array_equal(other[3], base[3], err_msg=what)
    for i in (0, 2, 4, 6):                                                                       # alone
        one = _multi_dev(eng, ids[i:i + 1], tt[i:i + 1], lens[i:i + 1], tok_dim)
        np.testing.assert_array_equal(one[0][0], base[0][i])
        np.testing.assert_array_equal(one[1][0], base[1][i])
        np.testing.assert_array_equal(one[2], base[2][base[3][i]:base[3][i + 1]])


def test_capacity_and_missing_heads():
    import torch
    from optimized_rag_amd import RagError
    cfg, w, eng, (ids, tt, lens) = _model("h256x32")
    eng.embed_heads_load(**M.seeded_heads(256, 96, 5, bias=False))
    full = _multi_dev(eng, ids, tt, lens, 96)
    total = int((lens - 1).sum())
    # device form: rows past the cap are dropped, the poison behind the cap survives, row_off[n] is still the true total
    cap = 40
    buf = torch.full((cap + 8, 96), float("nan"), device="cuda")
    off = torch.full((len(lens) + 1,), -7, dtype=torch.int64, device="cuda")
    eng.embed_multi_dev(torch.from_numpy(ids).cuda(), torch.from_numpy(tt).cuda(), torch.from_numpy(lens).cuda(), tok=buf[:cap], row_off=off)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got[:cap], full[2][:cap])
    assert np.isnan(got[cap:]).all() and int(off[-1]) == total > cap
    # host form: an error before any launch, and the handle stays usable after it
    with pytest.raises(RagError, match=r"\(-1\)"):
        eng.embed_multi(ids, tt, lens, tok_rows_cap=total - 1)
    np.testing.assert_array_equal(eng.embed_multi(ids, tt, lens, tok_rows_cap=total + 3)[2], full[2])
    # a head that is not loaded: RAG_ERR_STATE; a reload of the encoder drops the heads
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    eng.embed_load(cfg, flatten_state_dict(w, cfg["layers"], head=False), normalize=True, pooling="cls")
    with pytest.raises(RagError, match=r"\(-3\)"):
        eng.embed_multi(ids, tt, lens, dense=False, tokens=False)
    eng.embed_heads_load(lex_w=M.seeded_heads(256, 96, 5)["lex_w"], lex_b=0.01)
    eng.embed_tok_dim = 96
    with pytest.raises(RagError, match=r"\(-3\)"):
        eng.embed_multi(ids, tt, lens, dense=False, lexical=False)
    d, lx, tk, off2 = eng.embed_multi(ids, tt, lens, tokens=False)
    np.testing.assert_array_equal(d, full[0])
    assert tk is None and lx.shape == (len(lens), L) and off2[-1] == total
    with pytest.raises(RagError, match=r"\(-1\)"):
        eng.embed_heads_load(tok_w=np.zeros((40, 256), dtype=np.float32))                        # 40 is no multiple of 32
    from optimized_rag_amd import RagEngine
    bare = RagEngine(dim=128, device=0)
    try:
        with pytest.raises(RagError, match=r"\(-3\)"):
            bare.embed_heads_load(lex_w=np.zeros(128, dtype=np.float32))
    finally:
        bare.close()
    _CACHE.pop("h256x32")[2].close()                                                             # the next test reloads this model


# ---- MaxSim -------------------------------------------------------------------------------------------------------------------
COUNTS = [0, 1, 15, 16, 17, 31, 32, 33, 100, 513]


@pytest.fixture(scope="module")
def eng():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=128, device=0)
    yield e
    e.close()


def _unit_rows(rng, counts, dim):
    return [M.normalize(rng.standard_normal((n, dim))).astype(np.float32) for n in counts]


def _maxsim_dev(eng, q, qo, d, do, pq, pd):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = torch.full((len(pq),), float("nan"), device="cuda")
    eng.maxsim_dev(t(q), t(qo), t(d), t(do), t(np.asarray(pq, dtype=np.int32)), t(np.asarray(pd, dtype=np.int32)), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("dim", [32, 96, 1024])
def test_maxsim_against_float64(eng, dim):
    rng = np.random.default_rng(dim)
    qs, ds = _unit_rows(rng, COUNTS, dim), _unit_rows(rng, COUNTS, dim)
    q, qo = M.pack(qs, dim)
    d, do = M.pack(ds, dim)
    pq, pd = np.meshgrid(np.arange(len(COUNTS)), np.arange(len(COUNTS)), indexing="ij")
    pq, pd = pq.reshape(-1).astype(np.int32), pd.reshape(-1).astype(np.int32)
    exp = np.array([M.maxsim(qs[a], ds[b]) for a, b in zip(pq, pd)])
    got = _maxsim_dev(eng, q, qo, d, do, pq, pd)
    err = float(np.abs(got - exp).max())
    print(f"maxsim dim {dim}: max |d| = {err:.3e}")
    assert err < 1e-4 and got.dtype == np.float32
    assert (got[(np.array(COUNTS)[pq] == 0) | (np.array(COUNTS)[pd] == 0)] == 0).all()          # an empty side gives 0
    # two runs give identical bits; the host form too; independent of pair order; duplicates, out-of-range and -1 indices
    np.testing.assert_array_equal(_maxsim_dev(eng, q, qo, d, do, pq, pd), got)
    np.testing.assert_array_equal(eng.maxsim(q, qo, d, do, pq, pd), got)
    perm = rng.permutation(len(pq))
    np.testing.assert_array_equal(_maxsim_dev(eng, q, qo, d, do, pq[perm], pd[perm]), got[perm])
    odd_q = np.array([3, 3, -1, 4, len(COUNTS), 5, 2**30], dtype=np.int32)
    odd_d = np.array([4, 4, 4, -1, 4, len(COUNTS), 4], dtype=np.int32)
    odd = _maxsim_dev(eng, q, qo, d, do, odd_q, odd_d)
    assert odd[0] == odd[1] == got[3 * len(COUNTS) + 4] != 0 and (odd[2:] == 0).all()


def test_maxsim_all_negative_and_exact_powers_of_two(eng):
    rng = np.random.default_rng(1)
    # every similarity negative: document rows are the negated query direction plus noise; zero-filled padding would return >= 0
    dim = 96
    u = M.normalize(rng.standard_normal((1, dim)))
    qs = [M.normalize(u + 0.05 * rng.standard_normal((n, dim))).astype(np.float32) for n in (17, 5)]
    ds = [M.normalize(-u + 0.05 * rng.standard_normal((n, dim))).astype(np.float32) for n in (17, 33, 1)]
    q, qo = M.pack(qs, dim)
    d, do = M.pack(ds, dim)
    pq, pd = [0, 0, 0, 1, 1, 1], [0, 1, 2, 0, 1, 2]
    exp = np.array([M.maxsim(qs[a], ds[b]) for a, b in zip(pq, pd)])
    got = _maxsim_dev(eng, q, qo, d, do, pq, pd)
    assert (exp < -0.5).all() and (got < 0).all() and np.abs(got - exp).max() < 1e-4
    # entries in {0, +-2^-k}: every product and sum is exact in float32 and float64 alike, so the result is the float32 rounding of the
    # exact value - an indexing error (a wrong row, a wrong k slice, a pad row in a maximum) changes it
    dim = 64

    def sparse_rows(n):
        a = np.zeros((n, dim), dtype=np.float32)
        for r in range(n):
            cols = rng.choice(dim, 4, replace=False)
            a[r, cols] = rng.choice([-1.0, 1.0], 4) * 2.0 ** -rng.integers(1, 6, 4)
        return a

    counts_q, counts_d = [1, 16, 17, 33, 40], [1, 15, 17, 32, 70]
    qs, ds = [sparse_rows(n) for n in counts_q], [sparse_rows(n) for n in counts_d]
    q, qo = M.pack(qs, dim)
    d, do = M.pack(ds, dim)
    pq, pd = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
    pq, pd = pq.reshape(-1), pd.reshape(-1)
    exp = np.array([M.maxsim(qs[a], ds[b]) for a, b in zip(pq, pd)]).astype(np.float32)
    np.testing.assert_array_equal(_maxsim_dev(eng, q, qo, d, do, pq, pd), exp)
    assert len(set(exp.tolist())) > 8


# ---- lexical match ------------------------------------------------------------------------------------------------------------
def _lex_ref(ids, w, lens, skip):
    return [M.lexical_map(ids[i], w[i], max(0, min(int(lens[i]), ids.shape[1])), set(skip)) for i in range(len(lens))]


def test_lexical_match_against_a_dict_loop(eng):
    import torch
    rng = np.random.default_rng(2)
    skip = [0, 1, 2, 3, 250001, 7, 9, 11]                                                         # eight skip ids, every one present below
    Lq, Ld = 24, 300
    pool = np.array([0, 1, 2, 3, 7, 9, 11, 250001, 250000, 249999, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30], dtype=np.int32)
    q_ids = rng.choice(pool, (6, Lq)).astype(np.int32)                                           # duplicates inside a text, ids up to 250001
    d_ids = rng.choice(pool, (5, Ld)).astype(np.int32)
    q_w = rng.standard_normal((6, Lq)).astype(np.float32)                                        # about half negative
    d_w = rng.standard_normal((5, Ld)).astype(np.float32)
    q_w[0, :4] = 0.0
    q_lens = np.array([Lq, 1, 5, Lq, 0, Lq + 9], dtype=np.int32)
    d_lens = np.array([Ld, 1, 17, Ld, 200], dtype=np.int32)
    q_ids[3] = rng.integers(1000, 2000, Lq)                                                      # no overlap with any document: 0
    pq, pd = np.meshgrid(np.arange(6), np.arange(5), indexing="ij")
    pq = np.concatenate([pq.reshape(-1), [-1, 6, 0]]).astype(np.int32)
    pd = np.concatenate([pd.reshape(-1), [0, 0, 5]]).astype(np.int32)
    mq, md = _lex_ref(q_ids, q_w, q_lens, skip), _lex_ref(d_ids, d_w, d_lens, skip)
    exp = np.array([M.lexical_score(mq[a], md[b]) if 0 <= a < 6 and 0 <= b < 5 else 0.0 for a, b in zip(pq, pd)])
    t = lambda a: torch.from_numpy(a).cuda()
    out = torch.full((len(pq),), float("nan"), device="cuda")
    eng.lexical_match_dev(t(q_ids), t(q_w), t(q_lens), t(d_ids), t(d_w), t(d_lens), t(pq), t(pd), out, skip_ids=skip)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (exp > 0).sum() > 5 and any(250000 in m for m in mq)
    np.testing.assert_allclose(got, exp, rtol=1e-6, atol=0)
    assert (got[pq == 3] == 0).all() and (got[pq == 4] == 0).all() and (got[-3:] == 0).all()
    np.testing.assert_array_equal(eng.lexical_match(q_ids, q_w, q_lens, d_ids, d_w, d_lens, pq, pd, skip_ids=skip), got)
    # without the skip list the skipped ids count: the list is what removed them
    more = eng.lexical_match(q_ids, q_w, q_lens, d_ids, d_w, d_lens, pq, pd)
    mq0, md0 = _lex_ref(q_ids, q_w, q_lens, []), _lex_ref(d_ids, d_w, d_lens, [])
    exp0 = np.array([M.lexical_score(mq0[a], md0[b]) if 0 <= a < 6 and 0 <= b < 5 else 0.0 for a, b in zip(pq, pd)])
    np.testing.assert_allclose(more, exp0, rtol=1e-6, atol=0)
    assert (exp0 > exp).any()
    from optimized_rag_amd import RagError
    with pytest.raises(RagError, match=r"\(-1\)"):
        eng.lexical_match(q_ids, q_w, q_lens, d_ids, d_w, d_lens, pq, pd, skip_ids=list(range(9)))


# ---- stream order: each _dev call on a side stream between a producer and a consumer ---------------------------------------------
def test_dev_calls_are_ordered_on_the_caller_s_stream():
    import torch
    cfg, w, eng, (ids, tt, lens) = _model("h256x32")
    eng.embed_heads_load(**M.seeded_heads(256, 96, 5, bias=False))
    total = int((lens - 1).sum())
    rng = np.random.default_rng(6)

    def multi(dev, s):
        d = torch.full((len(lens), 256), float("nan"), device="cuda")
        lx = torch.full((len(lens), L), float("nan"), device="cuda")
        tk = torch.full((total, 96), float("nan"), device="cuda")
        off = torch.full((len(lens) + 1,), -7, dtype=torch.int64, device="cuda")
        eng.embed_multi_dev(dev["ids"], dev["tt"], dev["lens"], dense=d, lex=lx, tok=tk, row_off=off, stream=s)
        return [d, lx, tk, off]

    wrong_ids = np.where(ids > 0, (ids + 17) % cfg["vocab_size"], 0).astype(np.int32)
    real, wrong = dict(ids=ids, tt=tt, lens=lens), dict(ids=wrong_ids, tt=tt, lens=np.full_like(lens, 3))
    ref = T.serial(multi, wrong, real)
    got, _ = T.late_producer(multi, wrong, real, torch.cuda.Stream())
    T.assert_same(got, ref, "embed_multi_dev")

    qs, ds = _unit_rows(rng, [5, 33], 96), _unit_rows(rng, [17, 100, 1], 96)
    q, qo = M.pack(qs, 96)
    d, do = M.pack(ds, 96)
    pq, pd = np.array([0, 0, 1, 1, 1], dtype=np.int32), np.array([0, 1, 2, 0, 1], dtype=np.int32)

    def maxsim(dev, s):
        out = torch.full((len(pq),), float("nan"), device="cuda")
        eng.maxsim_dev(dev["q"], dev["qo"], dev["d"], dev["do"], dev["pq"], dev["pd"], out, stream=s)
        return [out]

    real = dict(q=q, qo=qo, d=d, do=do, pq=pq, pd=pd)
    wrong = dict(q=q[::-1].copy(), qo=np.array([0, 1, 2], dtype=np.int64), d=d[::-1].copy(), do=np.array([0, 1, 2, 3], dtype=np.int64),
                 pq=np.zeros_like(pq), pd=np.zeros_like(pd))
    ref = T.serial(maxsim, wrong, real)
    got, _ = T.late_producer(maxsim, wrong, real, torch.cuda.Stream())
    T.assert_same(got, ref, "maxsim_dev")
    assert np.abs(ref[0] - [M.maxsim(qs[a], ds[b]) for a, b in zip(pq, pd)]).max() < 1e-4

    li = rng.integers(4, 30, (4, 20)).astype(np.int32)
    lw = rng.random((4, 20)).astype(np.float32)
    ll = np.array([20, 7, 1, 13], dtype=np.int32)

    def lexical(dev, s):
        out = torch.full((4,), float("nan"), device="cuda")
        eng.lexical_match_dev(dev["i"], dev["w"], dev["l"], dev["i"], dev["w"], dev["l"], dev["pq"], dev["pd"], out, skip_ids=[4], stream=s)
        return [out]

    real = dict(i=li, w=lw, l=ll, pq=np.array([0, 1, 2, 3], dtype=np.int32), pd=np.array([1, 2, 3, 0], dtype=np.int32))
    wrong = dict(i=li[::-1].copy(), w=lw * 0, l=np.ones_like(ll), pq=np.zeros(4, dtype=np.int32), pd=np.zeros(4, dtype=np.int32))
    ref = T.serial(lexical, wrong, real)
    got, _ = T.late_producer(lexical, wrong, real, torch.cuda.Stream())
    T.assert_same(got, ref, "lexical_match_dev")
    assert (ref[0] > 0).any()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
def test_service_and_reranker_from_a_checkpoint_directory(tmp_path):
    import json
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    from optimized_rag_amd.reranker import LateInteractionReranker
    from optimized_rag_amd.selective_reranker import SelectiveReranker
    words = [f"w{i}" for i in range(60)]
    hf = X.xlmr_hf_config(vocab_size=64, hidden=128, layers=2, heads=4, ffn=256)
    sd = X.seeded_xlmr(hf, 9, head=False)
    heads = M.seeded_heads(128, 96, 4)
    plain, full = tmp_path / "plain", tmp_path / "m3"
    for d in (plain, full):
        X.write_checkpoint(d, hf, sd, words=words)
        (d / "1_Pooling").mkdir()
        (d / "1_Pooling" / "config.json").write_text(json.dumps(dict(pooling_mode_cls_token=True, pooling_mode_mean_tokens=False)))
    M.write_head_files(full, heads)
    cfg = dict(vocab_size=64, hidden=128, layers=2, heads=4, ffn=256, max_pos=64, type_vocab=1, eps=1e-5)
    w = X.xlmr_to_bert_names(sd, head=False)
    rng = np.random.default_rng(3)
    query = " ".join(rng.choice(words[:20], 6))
    # 11 candidates + an empty one, picked from a pool by the REFERENCE's scores so that they lie at least 4e-3 apart: every score is
    # held to 1e-3, so the reference's order is then the only order within the bars (a seeded encoder scores random texts within 0.1
    # of each other, and twelve of them at random lie closer than the bars)
    pool = [" ".join(rng.choice(words[:30], int(rng.integers(2, 40)))) for _ in range(60)]
    tk = X.roberta_tokenizer(words)
    enc = tk.encode_batch([query] + pool)
    pl = np.array([len(x.ids) for x in enc], dtype=np.int32)
    pi = np.zeros((len(enc), int(pl.max())), dtype=np.int32)
    for i, x in enumerate(enc):
        pi[i, :pl[i]] = x.ids
    ps = M.score_pairs(M.heads_reference(w, cfg, pi, np.zeros_like(pi), pl, heads), pi, pl, [0] * 60, list(range(1, 61)), {0, 1, 2, 3})
    picked = []
    for i in np.argsort(ps["colbert+sparse+dense"]):
        if not picked or ps["colbert+sparse+dense"][i] - ps["colbert+sparse+dense"][picked[-1]] >= 4e-3:
            picked.append(int(i))
    assert len(picked) >= 11
    cands = [pool[i] for i in rng.permutation(picked[-11:])] + [""]
    e = RagEngine(dim=128, device=0)
    try:
        svc = LocalEmbeddingService.from_dir(str(full), engine=e, max_length=64)
        assert svc.has_token_head and svc.has_lexical_head and svc.special_ids() == [0, 1, 2, 3]
        texts = [query] + cands
        enc = svc.encode_multi(texts)
        ids, tt, lens = svc.tokenize(texts)
        assert lens[-1] == 2 and sorted(enc) == ["colbert_vecs", "dense_vecs", "lexical_weights"]
        ref = M.heads_reference(w, cfg, ids, tt, lens, heads)
        assert enc["dense_vecs"].shape == (13, 128) and np.abs(enc["dense_vecs"] - ref["dense"]).max() < 1e-3
        assert [v.shape for v in enc["colbert_vecs"]] == [(int(n) - 1, 96) for n in lens]
        assert np.abs(np.concatenate(enc["colbert_vecs"]) - np.concatenate(ref["vecs"])).max() < 1e-3
        for i, m in enumerate(enc["lexical_weights"]):
            want = M.lexical_map(ids[i], ref["lex"][i], lens[i], {0, 1, 2, 3})
            assert all(isinstance(k, int) and v > 0 for k, v in m.items()) and not set(m) & {0, 1, 2, 3}
            assert all(abs(m.get(k, 0.0) - want.get(k, 0.0)) < 2e-3 for k in set(m) | set(want))
        only = svc.encode_multi(texts[:2], return_sparse=False, return_colbert_vecs=False)
        assert only["lexical_weights"] is None and only["colbert_vecs"] is None
        np.testing.assert_array_equal(only["dense_vecs"], enc["dense_vecs"][:2])
        pairs = [[query, c] for c in cands]
        got = svc.compute_score(pairs)
        exp = M.score_pairs(ref, ids, lens, [0] * 12, list(range(1, 13)), {0, 1, 2, 3})
        assert sorted(got) == sorted(M.SCORE_KEYS)
        for k in M.SCORE_KEYS:
            err = float(np.abs(np.asarray(got[k]) - exp[k]).max())
            print("compute_score", k, "max |d| =", err)
            assert len(got[k]) == 12 and err < 1e-3, k
        assert max(got["sparse"]) > 0 and got["sparse"][-1] == 0.0
        # the reranker: the reference's order and keys; never raises; SelectiveReranker drives it as it drives a cross-encoder
        rr = LateInteractionReranker(svc)
        assert rr.is_available()
        results = [dict(content=c, score=0.1 * i) for i, c in enumerate(cands)]
        ranked = rr.rerank(query, results, 5)
        order = np.argsort(-exp["colbert+sparse+dense"], kind="stable")[:5]
        gaps = np.diff(np.sort(exp["colbert+sparse+dense"]))
        assert gaps.min() > 2e-3, "the reference's order must not hang on the kernels' error"
        assert [r["content"] for r in ranked] == [cands[i] for i in order]
        for r in ranked:
            i = cands.index(r["content"])
            assert r["embedding_score"] == 0.1 * i and abs(r["score"] - exp["colbert+sparse+dense"][i]) < 1e-3
            assert abs(r["m3_dense_score"] - exp["dense"][i]) < 1e-3 and abs(r["m3_sparse_score"] - exp["sparse"][i]) < 1e-3
            assert abs(r["m3_colbert_score"] - exp["colbert"][i]) < 1e-3
        assert rr.rerank(query, [], 5) == []
        by_colbert = LateInteractionReranker(svc, mode="colbert").rerank(query, [dict(content=c) for c in cands], 3)
        assert len(by_colbert) == 3 and all(r["score"] == r["m3_colbert_score"] and "embedding_score" not in r for r in by_colbert)
        assert by_colbert[0]["score"] >= by_colbert[1]["score"] >= by_colbert[2]["score"] > np.sort(exp["colbert"])[-4] - 1e-3
        sel = SelectiveReranker(cross_encoder_reranker=rr)
        assert [r["content"] for r in sel.rerank(query, [dict(content=c, score=0.0) for c in cands], "qa", 5)] == [cands[i] for i in order]
        # a directory without the head files: the service of before (no heads, the same dense vectors, the new calls refuse)
        old = LocalEmbeddingService.from_dir(str(plain), engine=e, max_length=64)
        assert not old.has_token_head and not old.has_lexical_head and not LateInteractionReranker(old).is_available()
        np.testing.assert_array_equal(np.asarray(old.generate_embeddings_batch(texts[:4]), dtype=np.float32), enc["dense_vecs"][:4])
        with pytest.raises(ValueError):
            old.encode_multi(texts[:2])
        fallback = LateInteractionReranker(old).rerank(query, [dict(content=c) for c in cands], 4)
        assert [r["content"] for r in fallback] == cands[:4]
    finally:
        e.close()
