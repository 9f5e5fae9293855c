"""GPU parity of the cross-encoder forward (K7) against the float64 numpy oracle (pinned to the transformers
implementation by tests/test_oracle_bert.py) and the committed golden logits. Tolerance: the north star asks for
rerank scores within 1e-3; logits are checked at 4e-3 absolute (sigmoid' <= 1/4) and sigmoid scores at 1e-3."""
import json
import os

import numpy as np
import pytest

from oracle import bert_oracle as B
from oracle import rag_oracle as O

pytestmark = pytest.mark.gpu

LOGIT_TOL = 4e-3
SCORE_TOL = 1e-3


@pytest.fixture(scope="module", params=["mx", "split16"])
def eng(request):
    """Every test of this file runs on both forwards: the MX kernels (hi16 + lo8 operands, csrc/ce_mx.h; option ce_mx = 1 forces
    them; they are also the default for this shape at every batch size) and the split-fp16 kernels of rounds 1-3 (ce_mx = -1), which
    remain the path of other hidden sizes."""
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=1536, device=0)
    e.ce_mode = 1 if request.param == "mx" else -1
    e.set_option("ce_mx", e.ce_mode)
    yield e
    e.close()


def load_model(eng, cfg, w):
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    eng.ce_load(cfg, flatten_state_dict(w, cfg["layers"]))


def test_minilm_golden_logits(eng, golden_dir):
    g = np.load(os.path.join(golden_dir, "bert_minilm.npz"))
    cfg = B.minilm_config()
    w = B.seeded_weights(cfg, int(g["seed"]))
    load_model(eng, cfg, w)
    got = eng.ce_score(g["input_ids"], g["token_type_ids"], g["lens"])
    exp = g["logits"]
    assert np.abs(got - exp).max() < LOGIT_TOL, (got, exp)
    sg = np.array([O.sigmoid(float(x)) for x in got])
    se = np.array([O.sigmoid(float(x)) for x in exp])
    assert np.abs(sg - se).max() < SCORE_TOL


@pytest.mark.parametrize("P,L", [(3, 32), (5, 64), (2, 200), (1, 512), (7, 100), (2, 300)])
def test_minilm_shapes_vs_oracle(eng, P, L):
    cfg = B.minilm_config()
    w = B.seeded_weights(cfg, 99)
    load_model(eng, cfg, w)
    rng = np.random.default_rng(P * 1000 + L)
    lens = rng.integers(2, L + 1, P)
    lens[0] = L
    ids = np.zeros((P, L), dtype=np.int64)
    tt = np.zeros((P, L), dtype=np.int64)
    for p in range(P):
        n = int(lens[p])
        ids[p, :n] = rng.integers(1000, cfg["vocab_size"], n)
        tt[p, n // 3:n] = 1
    got = eng.ce_score(ids, tt, lens)
    sel = slice(0, min(P, 3))                      # the float64 oracle is slow at long L: check a few pairs
    exp = B.forward_logits(w, cfg, ids[sel], tt[sel], lens[sel])
    assert np.abs(got[sel] - exp).max() < LOGIT_TOL, (got[sel], exp)


def _random_pairs(rng, cfg, P, L, lens):
    ids = rng.integers(1000, cfg["vocab_size"], (P, L)).astype(np.int32)
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    tt = ((np.arange(L)[None, :] >= 18) & (np.arange(L)[None, :] < lens[:, None])).astype(np.int32)
    return ids, tt


def test_bench_path_persistent_handover_and_two_chunks(eng):
    """The path the rerank throughput is measured on: 6-layer MiniLM shape, L = 256, 8192 pairs of mixed
    length = ~1.5M packed rows, so every persistent GEMM workgroup walks several tiles (the cross-tile DMA hand-over in
    all three epilogue variants) and the 2M-token chunk loop runs twice (7812 + 380 pairs). Pairs are independent, so the
    float64 oracle is evaluated on a sample: first / last pair, both sides of the chunk boundary, short and full-length
    pairs, pairs deep inside the first chunk."""
    import torch
    cfg = B.minilm_config()
    w = B.seeded_weights(cfg, 99)
    load_model(eng, cfg, w)
    P, L = 8192, 256
    rng = np.random.default_rng(8192)
    lens = (18 + rng.integers(96, 225, P)).clip(max=L).astype(np.int32)             # the bench's length mix
    lens[rng.integers(0, P, 400)] = rng.integers(2, 60, 400)                         # plus short pairs ...
    lens[rng.integers(0, P, 200)] = L                                                # ... and full-length ones
    sample = [0, 1, 40, 977, 3000, 5000, 7810, 7811, 7812, 7813, 8000, P - 1]
    lens[[1, 7811]] = [5, L]
    lens[[7812, 8000]] = [L, 33]
    ids, tt = _random_pairs(rng, cfg, P, L, lens)
    out = torch.empty((P,), dtype=torch.float32, device="cuda")
    eng.ce_score_dev(torch.from_numpy(ids).cuda(), torch.from_numpy(tt).cuda(), torch.from_numpy(lens).cuda(), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    exp = B.forward_logits(w, cfg, ids[sample].astype(np.int64), tt[sample].astype(np.int64), lens[sample], fast_erf=True)
    assert np.abs(got[sample] - exp).max() < LOGIT_TOL, (got[sample], exp)
    sg = np.array([O.sigmoid(float(x)) for x in got[sample]])
    se = np.array([O.sigmoid(float(x)) for x in exp])
    assert np.abs(sg - se).max() < SCORE_TOL
    # the host-pointer entry walks the same chunk loop with H2D staging per chunk: same bits
    np.testing.assert_array_equal(eng.ce_score(ids[7700:7900], tt[7700:7900], lens[7700:7900]), got[7700:7900])


def test_mx_and_split16_forwards_agree_and_default_threshold(eng):
    """The two forwards on the same pairs: both within the bar of the float64 oracle, hence within twice the bar of each other; with
    the option at its default (0) the MiniLM shape takes the MX kernels at EVERY batch size (bit-identical to the forced MX run for
    64 pairs and for 3: a pair's logit does not depend on how a batch is split over ranks or chunks)."""
    cfg = B.minilm_config()
    w = B.seeded_weights(cfg, 2024)
    load_model(eng, cfg, w)
    rng = np.random.default_rng(77)
    P, L = 64, 128
    lens = rng.integers(2, L + 1, P).astype(np.int32)
    ids, tt = _random_pairs(rng, cfg, P, L, lens)
    res = {}
    try:
        for mode in (1, -1, 0):
            eng.set_option("ce_mx", mode)
            res[mode] = (eng.ce_score(ids, tt, lens), eng.ce_score(ids[:3], tt[:3], lens[:3]))
    finally:
        eng.set_option("ce_mx", eng.ce_mode)
    exp = B.forward_logits(w, cfg, ids[:12].astype(np.int64), tt[:12].astype(np.int64), lens[:12], fast_erf=True)
    assert np.abs(res[1][0][:12] - exp).max() < LOGIT_TOL
    assert np.abs(res[-1][0][:12] - exp).max() < LOGIT_TOL
    assert np.abs(res[1][0] - res[-1][0]).max() < 2 * LOGIT_TOL
    assert np.abs(res[1][0] - res[-1][0]).max() > 0            # they ARE different arithmetic
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(res[1][1], res[1][0][:3])    # the same pairs alone or inside a larger batch: the same bits


def test_small_multi_chunk_loop(eng, monkeypatch):
    """Option ce_chunk_tokens shrinks the activation chunk: 300 pairs at L = 64 in chunks of 64 pairs (5 chunks, the last one
    short) must give the same logits, bit for bit, as one chunk (pairs are independent; every output element sums its K
    range in the same order whatever tile it lands in), and match the float64 oracle."""
    cfg = dict(vocab_size=5000, hidden=384, layers=2, heads=12, ffn=1536, max_pos=64, type_vocab=2, eps=1e-12)
    w = B.seeded_weights(cfg, 3)
    load_model(eng, cfg, w)
    rng = np.random.default_rng(64)
    P, L = 300, 64
    lens = rng.integers(2, L + 1, P).astype(np.int32)
    ids, tt = _random_pairs(rng, cfg, P, L, lens)
    one = eng.ce_score(ids, tt, lens)
    eng.set_option("ce_chunk_tokens", 4096)
    try:
        many = eng.ce_score(ids, tt, lens)
    finally:
        eng.set_option("ce_chunk_tokens", 0)
    np.testing.assert_array_equal(one, many)
    sel = [0, 63, 64, 65, 255, 256, 299]
    exp = B.forward_logits(w, cfg, ids[sel].astype(np.int64), tt[sel].astype(np.int64), lens[sel])
    assert np.abs(many[sel] - exp).max() < LOGIT_TOL


def test_reranker_from_local_dir(eng, tmp_path):
    """End to end through the mirror class: local checkpoint dir -> tokeniser -> HIP forward -> sigmoid -> sort."""
    from safetensors.numpy import save_file
    from optimized_rag_amd.reranker import CrossEncoderReranker
    words = ("memory vector index query document retrieval ranking fusion agent graph node embedding cosine score "
             "keyword search context token model latency cache batch shard kernel").split()
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words + ["##s", "##ing", ".", ","]
    cfg = dict(vocab_size=len(vocab), hidden=384, layers=2, heads=12, ffn=1536, max_pos=64, type_vocab=2, eps=1e-12)
    w = B.seeded_weights(cfg, 5)
    d = tmp_path / "ce"
    d.mkdir()
    (d / "vocab.txt").write_text("\n".join(vocab) + "\n")
    (d / "config.json").write_text(json.dumps(dict(
        vocab_size=len(vocab), hidden_size=384, num_hidden_layers=2, num_attention_heads=12, intermediate_size=1536,
        max_position_embeddings=64, type_vocab_size=2, hidden_act="gelu", layer_norm_eps=1e-12)))
    save_file({k: v for k, v in w.items()}, str(d / "model.safetensors"))
    ce = CrossEncoderReranker(model_name=str(d), max_length=64, engine=eng)
    assert ce.is_available()
    rng = np.random.default_rng(3)
    docs = [{"content": " ".join(rng.choice(words, size=int(rng.integers(3, 80)))) + ".", "pos": i, "score": 0.1 * i}
            for i in range(9)]
    query = "vector index latency"
    out = ce.rerank(query, [dict(x) for x in docs], top_k=5)
    ids, tt, lens = ce.model.tokenize_pairs([[query, x["content"]] for x in docs])
    assert ids.shape[1] <= 64 and ids[0, 0] == 2 and (lens >= 6).all()
    exp = B.forward_logits(w, cfg, ids.astype(np.int64), tt.astype(np.int64), lens)
    sig = [O.sigmoid(float(np.float32(x))) for x in exp]
    order = [int(i) for i in O.stable_topk_desc(sig, 5)]
    assert [x["pos"] for x in out] == order
    for x in out:
        assert abs(x["cross_encoder_score"] - sig[x["pos"]]) < SCORE_TOL
        assert abs(x["cross_encoder_raw_score"] - exp[x["pos"]]) < LOGIT_TOL
        assert x["embedding_score"] == 0.1 * x["pos"] and x["score"] == x["cross_encoder_score"]


def test_sixteen_row_packing_edges_and_position_independence(eng):
    """Pairs are packed to 16-row multiples, so a pair may start at an odd multiple of 16 (its 32-key attention blocks then
    straddle two 32-row stretches of the packed space) and may own an odd number of 16-row tiles (the second half of its last
    key block belongs to the NEXT pair, or lies past the packed end for the last pair). Lengths around every tile edge, in an
    order that produces all four (start parity, tile-count parity) combinations, against the float64 oracle; then the same
    pairs in reverse order and one at a time: a pair's logit must not depend on its neighbours (bit for bit)."""
    cfg = B.minilm_config()
    w = B.seeded_weights(cfg, 99)
    load_model(eng, cfg, w)
    L = 64
    lens = np.array([1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 2, 40, 16, 16, 20, 64, 5], dtype=np.int32)
    P = len(lens)
    rng = np.random.default_rng(1616)
    ids, tt = _random_pairs(rng, cfg, P, L, lens)
    got = eng.ce_score(ids, tt, lens)
    exp = B.forward_logits(w, cfg, ids.astype(np.int64), tt.astype(np.int64), lens, fast_erf=True)
    assert np.isfinite(got).all()
    assert np.abs(got - exp).max() < LOGIT_TOL, (got, exp)
    rev = eng.ce_score(ids[::-1].copy(), tt[::-1].copy(), lens[::-1].copy())
    np.testing.assert_array_equal(rev[::-1], got)
    for p in (0, 3, 6, 11, P - 1):
        np.testing.assert_array_equal(eng.ce_score(ids[p:p + 1], tt[p:p + 1], lens[p:p + 1]), got[p:p + 1])


def test_large_batch_vs_oracle_and_same_bits_as_a_small_batch(eng):
    """3000 pairs of mixed length at L = 256 = ~600k packed rows: every persistent GEMM workgroup walks several tiles (the
    cross-tile DMA hand-over), lengths hit every 16-row packing edge. Every logit is finite, a sample is held against the float64
    oracle, and the first 70 pairs scored alone (fewer tiles than CUs, the last tile partial) give the same bits as inside the
    large batch: each forward picks its kernels by shape, never by batch size."""
    import torch
    cfg = B.minilm_config()
    w = B.seeded_weights(cfg, 99)
    load_model(eng, cfg, w)
    P, L = 3000, 256
    rng = np.random.default_rng(1536)
    lens = (18 + rng.integers(96, 225, P)).clip(max=L).astype(np.int32)
    lens[:40] = np.arange(1, 41)
    lens[40:60] = L
    ids, tt = _random_pairs(rng, cfg, P, L, lens)
    d_ids, d_tt, d_lens = torch.from_numpy(ids).cuda(), torch.from_numpy(tt).cuda(), torch.from_numpy(lens).cuda()
    out = torch.empty((P,), dtype=torch.float32, device="cuda")
    small = torch.empty((70,), dtype=torch.float32, device="cuda")
    eng.ce_score_dev(d_ids, d_tt, d_lens, out)
    eng.ce_score_dev(d_ids[:70].contiguous(), d_tt[:70].contiguous(), d_lens[:70].contiguous(), small)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    sample = [0, 1, 15, 16, 39, 40, 59, 60, 1500, P - 1]
    exp = B.forward_logits(w, cfg, ids[sample].astype(np.int64), tt[sample].astype(np.int64), lens[sample], fast_erf=True)
    assert np.abs(got[sample] - exp).max() < LOGIT_TOL, (got[sample], exp)
    np.testing.assert_array_equal(small.cpu().numpy(), got[:70])
