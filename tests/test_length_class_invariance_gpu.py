"""GPU: a sequence's output is the same bits whatever padded length it arrives with and whatever its batch neighbours are.

rag_ce_score_* / rag_embed_* round the padded length L_in of a call up to an attention length class (32, 64, 96, 128, 192, 256, 384,
512). The class picks the attention instance (split fp16: one 16-query block per wave at 32, two above; MX: one up to 256, two
above), the LDS layout and the launch shape, and the neighbours decide where a sequence's rows sit in the packed GEMM tiles. The mirror
classes pad to the longest item of a batch and their caches hand a vector computed in one batch back for the same text alone, so
none of that may change a bit of the result. Sequences of 1, 16, 17, 31 and 32 tokens are scored alone at L_in = their own length,
then first, in the middle and last in batches padded to 33, 64, 97, 129, 200, 300 and 512 (every class boundary crossed, both
attention instances of each forward), on hidden 384 with option ce_mx = 1 and -1 and on a split-only shape (hidden 128), both heads;
every result is also within the project's bars of the float64 oracle (logits 4e-3; unit vectors 1e-3 per component, 1 - cos < 1e-6)."""
import json

import numpy as np
import pytest

from oracle import bert_oracle as B

pytestmark = pytest.mark.gpu

LOGIT_TOL = 4e-3
EMB_TOL = 1e-3
COS_TOL = 1e-6
SEQ_LENS = [1, 16, 17, 31, 32]
L_INS = [33, 64, 97, 129, 200, 300, 512]
MODELS = {
    "h384-mx": (dict(vocab_size=2000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=512, type_vocab=2, eps=1e-12), 1),
    "h384-split16": (dict(vocab_size=2000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=512, type_vocab=2, eps=1e-12), -1),
    "h128-split-only": (dict(vocab_size=2000, hidden=128, layers=2, heads=4, ffn=512, max_pos=512, type_vocab=2, eps=1e-12), 0),
}


@pytest.fixture(scope="module")
def eng():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=384, device=0)
    e.loaded = None
    yield e
    e.close()


def _rows(rng, cfg, lens, L):
    lens = np.asarray(lens, dtype=np.int32)
    ids = rng.integers(5, cfg["vocab_size"], (len(lens), L)).astype(np.int32)
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    tt = ((np.arange(L)[None, :] >= 9) & (np.arange(L)[None, :] < lens[:, None])).astype(np.int32)
    return ids, tt, lens


def _pad(a, L):
    out = np.zeros((a.shape[0], L), dtype=np.int32)
    out[:, :a.shape[1]] = a
    return out


def _run(eng, model, head, ids, tt, lens):
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    cfg, mode = MODELS[model]
    w = B.seeded_weights(cfg, 77)
    if eng.loaded != (cfg["hidden"], head):
        if head == "classifier":
            eng.ce_load(cfg, flatten_state_dict(w, cfg["layers"]))
        else:
            eng.embed_load(cfg, flatten_state_dict(w, cfg["layers"], head=False), normalize=True)
        eng.loaded = (cfg["hidden"], head)
    eng.set_option("ce_mx", mode)
    try:
        return eng.ce_score(ids, tt, lens) if head == "classifier" else eng.embed(ids, tt, lens)
    finally:
        eng.set_option("ce_mx", 0)


_ALONE = {}


def _alone(eng, model, head):
    """The five sequences, each scored alone at L_in = its own length, and checked against the oracle."""
    if (model, head) not in _ALONE:
        cfg, _ = MODELS[model]
        ids, tt, lens = _rows(np.random.default_rng(515), cfg, SEQ_LENS, 32)
        got = np.stack([_run(eng, model, head, ids[i:i + 1, :n], tt[i:i + 1, :n], lens[i:i + 1])[0] for i, n in enumerate(SEQ_LENS)])
        w = B.seeded_weights(cfg, 77)
        if head == "classifier":
            exp = B.forward_logits(w, cfg, ids.astype(np.int64), tt.astype(np.int64), lens, fast_erf=True)
        else:
            exp = B.sentence_embeddings(w, cfg, ids.astype(np.int64), tt.astype(np.int64), lens, fast_erf=True)
        _ALONE[(model, head)] = (ids, tt, lens, got, exp)
    return _ALONE[(model, head)]


def _within_the_bar(got, exp, head):
    assert np.isfinite(got).all()
    if head == "classifier":
        assert np.abs(got - exp).max() < LOGIT_TOL
    else:
        g = got.astype(np.float64)
        assert np.abs(g - exp).max() < EMB_TOL
        assert (1.0 - (g * exp).sum(1) / np.linalg.norm(g, axis=1)).max() < COS_TOL


@pytest.mark.parametrize("L_in", L_INS)
@pytest.mark.parametrize("head", ["classifier", "embedding"])
@pytest.mark.parametrize("model", list(MODELS))
def test_bits_do_not_depend_on_padded_length_or_neighbours(eng, model, head, L_in):
    cfg, _ = MODELS[model]
    ids, tt, lens, alone, exp = _alone(eng, model, head)
    _within_the_bar(alone, exp, head)
    # neighbours: one full-length row (it sets L_in), one with an odd count of 16-row tiles
    n_ids, n_tt, n_lens = _rows(np.random.default_rng(L_in), cfg, [L_in, max(1, (L_in // 2) | 1)], L_in)
    s_ids, s_tt = _pad(ids, L_in), _pad(tt, L_in)
    k = len(SEQ_LENS)
    for where, order in (("first", list(range(k)) + [k, k + 1]), ("middle", [k] + list(range(k)) + [k + 1]),
                         ("last", [k, k + 1] + list(range(k)))):
        b_ids, b_tt, b_lens = (np.concatenate([a, b])[order] for a, b in ((s_ids, n_ids), (s_tt, n_tt), (lens, n_lens)))
        got = _run(eng, model, head, np.ascontiguousarray(b_ids), np.ascontiguousarray(b_tt), np.ascontiguousarray(b_lens))
        mine = got[[order.index(i) for i in range(k)]]
        _within_the_bar(mine, exp, head)
        np.testing.assert_array_equal(mine, alone, err_msg=f"{model} {head} L_in={L_in}, sequences {where} in the batch")


# ---- through the mirror classes ----------------------------------------------------------------------------------------------
WORDS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(195)]
MIRROR_CFG = dict(vocab_size=200, hidden=384, layers=2, heads=12, ffn=1536, max_pos=512, type_vocab=2, eps=1e-12)


def _checkpoint(tmp_path, w, keep):
    from safetensors.numpy import save_file
    d = tmp_path / "model"
    d.mkdir()
    (d / "vocab.txt").write_text("\n".join(WORDS) + "\n")
    c = MIRROR_CFG
    (d / "config.json").write_text(json.dumps(dict(vocab_size=c["vocab_size"], hidden_size=c["hidden"], num_hidden_layers=c["layers"],
                                                   num_attention_heads=c["heads"], intermediate_size=c["ffn"],
                                                   max_position_embeddings=c["max_pos"], type_vocab_size=2, hidden_act="gelu",
                                                   layer_norm_eps=1e-12)))
    save_file(keep(w), str(d / "model.safetensors"))
    return str(d)


def _text(rng, n):
    return " ".join(rng.choice(WORDS[5:], n))


@pytest.mark.parametrize("mode", [0, 1, -1], ids=["default", "mx", "split16"])
def test_embedding_service_vector_does_not_depend_on_a_long_neighbour(tmp_path, mode):
    """generate_embedding(t, use_cache=False) is the slot of t in a batch that also holds a 400-token text (padded length class
    512 instead of 32 ... 64): what the service's cache relies on."""
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    w = B.seeded_weights(MIRROR_CFG, 5)
    path = _checkpoint(tmp_path, w, lambda w: {k[len("bert."):]: v for k, v in w.items() if k.startswith("bert.") and "pooler" not in k})
    e = RagEngine(dim=384, device=0)
    try:
        svc = LocalEmbeddingService.from_dir(path, engine=e, max_length=512)
        rng = np.random.default_rng(3)
        texts = [_text(rng, n) for n in (1, 3, 14, 15, 29, 30, 45, 60)]
        batch = texts[:4] + [_text(rng, 398)] + texts[4:]
        e.set_option("ce_mx", mode)
        vecs = np.asarray(svc.generate_embeddings_batch(batch, use_cache=False), dtype=np.float32)
        ids, tt, lens = svc.tokenize(batch)
        assert lens.max() == 400 and ids.shape[1] == 400
        exp = B.sentence_embeddings(w, MIRROR_CFG, ids.astype(np.int64), tt.astype(np.int64), lens, fast_erf=True)
        assert np.abs(vecs - exp).max() < EMB_TOL
        for t in texts:
            one = np.asarray(svc.generate_embedding(t, use_cache=False), dtype=np.float32)
            np.testing.assert_array_equal(one, vecs[batch.index(t)])
    finally:
        e.close()


@pytest.mark.parametrize("mode", [0, 1, -1], ids=["default", "mx", "split16"])
def test_cross_encoder_logits_do_not_depend_on_where_predict_splits(tmp_path, mode):
    """LocalCrossEncoder.predict with batch_pairs = 4096 (one call, padded to the longest pair) and with batch_pairs = 4, which puts
    the short pairs and the long pairs into calls of their own: the same logits, bit for bit."""
    from optimized_rag_amd import RagEngine
    from optimized_rag_amd.cross_encoder import LocalCrossEncoder
    w = B.seeded_weights(MIRROR_CFG, 6)
    path = _checkpoint(tmp_path, w, lambda w: dict(w))
    e = RagEngine(dim=384, device=0)
    try:
        ce = LocalCrossEncoder.from_dir(path, engine=e)
        rng = np.random.default_rng(4)
        short = [(_text(rng, a), _text(rng, b)) for a, b in ((1, 1), (3, 9), (5, 24), (2, 27), (6, 40), (4, 11), (7, 50), (3, 3))]
        long_ = [(_text(rng, 8), _text(rng, n)) for n in (280, 340, 400, 300)]
        pairs = short[:4] + long_ + short[4:]
        e.set_option("ce_mx", mode)
        ce.batch_pairs = 4096
        whole = ce.predict(pairs)
        ce.batch_pairs = 4
        split = ce.predict(pairs)
        ids, tt, lens = ce.tokenize_pairs(pairs)
        assert lens[:4].max() <= 32 and lens[4:8].min() > 256
        exp = B.forward_logits(w, MIRROR_CFG, ids.astype(np.int64), tt.astype(np.int64), lens, fast_erf=True)
        assert np.abs(whole - exp).max() < LOGIT_TOL and np.abs(split - exp).max() < LOGIT_TOL
        np.testing.assert_array_equal(whole, split)
    finally:
        e.close()
