"""CPU: what loading an XLM-RoBERTa reranker or embedder rests on, without a GPU.
1. cross_encoder.map_checkpoint on a seeded transformers.XLMRobertaForSequenceClassification / XLMRobertaModel written to disk in
   float64: the float64 BERT oracle on the mapped tensors equals transformers to 1e-12 (measured 2.8e-16 for the logits) - the
   encoder needs no new arithmetic, only other names, a position table without its reserved rows, and one token type. The three
   refusals raise.
2. The RoBERTa pair layout the device builder writes (tests/xlmr_tools.build_pairs, which the GPU tests compare the kernel with)
   is the `tokenizers` package's own: template <s> $A </s> </s> $B </s>, longest_first truncation - over the case grid of
   tests/test_pair_truncation.py.
3. The five new entry points are declared, bound and exported.
4. A shard whose token ids reach 250001 records token_id_max and returns the ids unchanged from its memory map."""
import json
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G
import xlmr_tools as X
from oracle import bert_oracle as B
from oracle import rag_oracle as O

NEW_EXPORTS = ["rag_tokens_load_wide_host", "rag_tokens_reserve_wide", "rag_tokens_info", "rag_ce_set_pair_format"]
ROW_LENS = [1, 5, 17, 33, 40, 48]
L = 48


def _hf_config(cls, **more):
    return cls(vocab_size=70000, hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
               max_position_embeddings=66, type_vocab_size=1, layer_norm_eps=1e-5, hidden_dropout_prob=0.0,
               attention_probs_dropout_prob=0.0, pad_token_id=1, bos_token_id=0, eos_token_id=2, **more)


def _rows(seed):
    """right-padded rows of lengths 1 .. 48 at L = 48: real ids from 5 up, <pad> = 1 behind them, the attention mask"""
    rng = np.random.default_rng(seed)
    lens = np.array(ROW_LENS, dtype=np.int64)
    ids = rng.integers(5, 70000, (len(lens), L)).astype(np.int64)
    mask = np.arange(L)[None, :] < lens[:, None]
    ids[~mask] = 1
    return ids, lens, mask


def _save(model, d):
    """config.json + model.safetensors as save_pretrained lays them out (float64 tensors)"""
    from safetensors.torch import save_file
    d.mkdir()
    (d / "config.json").write_text(model.config.to_json_string())
    save_file({k: v.contiguous() for k, v in model.state_dict().items()}, str(d / "model.safetensors"))
    return d


def _load(d):
    from safetensors.numpy import load_file
    return json.loads((d / "config.json").read_text()), load_file(str(d / "model.safetensors"))


def test_mapped_classifier_equals_transformers_in_float64(tmp_path):
    import torch
    from transformers import XLMRobertaConfig, XLMRobertaForSequenceClassification
    from optimized_rag_amd.cross_encoder import flatten_state_dict, map_checkpoint
    torch.manual_seed(11)
    model = XLMRobertaForSequenceClassification(_hf_config(XLMRobertaConfig, num_labels=1)).double().eval()
    hf_cfg, sd = _load(_save(model, tmp_path / "ce"))
    cfg, w = map_checkpoint(hf_cfg, sd)
    assert cfg["max_pos"] == 64 and cfg["type_vocab"] == 1 and cfg["eps"] == 1e-5 and cfg["vocab_size"] == 70000
    assert (cfg["pair_format"], cfg["cls_id"], cfg["sep_id"]) == (1, 0, 2)
    assert w["bert.embeddings.position_embeddings.weight"].shape == (64, 128) and w["classifier.weight"].dtype == np.float64
    ids, lens, mask = _rows(3)
    with torch.no_grad():
        want = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask.astype(np.int64))).logits[:, 0].numpy()
    got = B.forward_logits(w, cfg, ids, np.zeros_like(ids), lens)
    err = float(np.abs(got - want).max())
    print("max |oracle(mapped) - transformers| logits:", err)
    assert err <= 1e-12
    # the hand-written relabelling of xlmr_tools (what the GPU tests load as a BERT) names the same tensors
    hand = X.xlmr_to_bert_names(sd)
    assert sorted(hand) == sorted(w)
    for k in w:
        np.testing.assert_array_equal(hand[k], w[k])
    # and the engine's tensor order takes them: 5 + 16 per layer + 4, float32
    flat = flatten_state_dict(w, cfg["layers"])
    assert len(flat) == 5 + 16 * 2 + 4 and all(t.dtype == np.float32 for t in flat)
    # the prefix-less spelling of the same file maps to the same tensors
    cfg2, w2 = map_checkpoint(hf_cfg, {(k[len("roberta."):] if k.startswith("roberta.") else k): v for k, v in sd.items()})
    assert cfg2 == cfg and all(np.array_equal(w2[k], w[k]) for k in w)


def test_mapped_encoder_equals_transformers_in_float64_mean_and_cls(tmp_path):
    import torch
    from transformers import XLMRobertaConfig, XLMRobertaModel
    from optimized_rag_amd.cross_encoder import flatten_state_dict, map_checkpoint
    torch.manual_seed(12)
    model = XLMRobertaModel(_hf_config(XLMRobertaConfig)).double().eval()
    hf_cfg, sd = _load(_save(model, tmp_path / "enc"))
    cfg, w = map_checkpoint(hf_cfg, sd, head=False)
    assert not any("pooler" in k or k.startswith("classifier") for k in w)
    assert len(flatten_state_dict(w, cfg["layers"], head=False)) == 5 + 16 * 2
    ids, lens, mask = _rows(4)
    with torch.no_grad():
        hid = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask.astype(np.int64))).last_hidden_state.numpy()
    m = mask[:, :, None].astype(np.float64)
    mean = (hid * m).sum(1) / m.sum(1)
    want_mean = mean / np.linalg.norm(mean, axis=1, keepdims=True)
    got_mean = B.sentence_embeddings(w, cfg, ids, np.zeros_like(ids), lens)
    _, got_hid = B.forward_hidden(w, cfg, ids, np.zeros_like(ids), lens)
    e_mean, e_cls = float(np.abs(got_mean - want_mean).max()), float(np.abs(got_hid[:, 0] - hid[:, 0]).max())
    print("max |oracle(mapped) - transformers| mean-pooled unit vector:", e_mean, " [CLS] row:", e_cls)
    assert e_mean <= 1e-12 and e_cls <= 1e-12


def test_the_three_refusals():
    from optimized_rag_amd.cross_encoder import map_checkpoint
    hf = X.xlmr_hf_config(vocab_size=50, max_position_embeddings=20)
    sd = X.seeded_xlmr(hf, 1)
    cfg, _ = map_checkpoint(hf, sd)                                             # the base case loads
    assert cfg["max_pos"] == 18
    with pytest.raises(ValueError, match="position_embedding_type"):
        map_checkpoint(dict(hf, position_embedding_type="relative_key"), sd)
    with pytest.raises(ValueError, match="GELU"):
        map_checkpoint(dict(hf, hidden_act="gelu_new"), sd)
    two = dict(sd)
    two["classifier.out_proj.weight"] = np.repeat(sd["classifier.out_proj.weight"], 2, axis=0)
    two["classifier.out_proj.bias"] = np.repeat(sd["classifier.out_proj.bias"], 2)
    with pytest.raises(ValueError, match="single-logit"):
        map_checkpoint(hf, two)
    with pytest.raises(ValueError, match="single-logit"):
        map_checkpoint(dict(hf, num_labels=3), sd)
    map_checkpoint(hf, two, head=False)                                         # the embedder never looks at the head
    with pytest.raises(ValueError, match="model_type"):
        map_checkpoint(dict(hf, model_type="deberta-v2"), sd)


def test_roberta_pair_layout_is_the_tokenizers_package_s():
    """ids, type ids and lengths of xlmr_tools.build_pairs(fmt = RoBERTa) against `tokenizers` itself, on the grid of
    tests/test_pair_truncation.py (600 cases up to L = 32, 40 random ones at L = 512). Token a = id 4 is the query's, b = 5 the
    passage's; the kept lengths are also O.longest_first_lengths over L - 4."""
    tok = X.roberta_tokenizer(["a", "b"])
    rng = np.random.default_rng(0)
    cases = [(n1, n2, Lp) for Lp in (8, 9, 16, 31, 32) for n1 in (0, 1, 2, 3, 5, 8, 13, 14, 15, 16, 29, 40) for n2 in (0, 1, 4, 6, 7, 13, 14, 15, 30, 64)]
    cases += [(int(rng.integers(0, 600)), int(rng.integers(0, 600)), 512) for _ in range(40)]
    assert len(cases) == 640
    for n1, n2, Lp in cases:
        tok.enable_truncation(max_length=Lp, strategy="longest_first")
        enc = tok.encode(" ".join(["a"] * n1), " ".join(["b"] * n2))
        q_tok, d_tok = np.full((1, max(n1, 1)), 4, dtype=np.int32), np.full((1, max(n2, 1)), 5, dtype=np.int32)
        ids, tt, lens = X.build_pairs(q_tok, np.array([n1]), np.zeros((1, 1), dtype=np.int64), d_tok, np.array([n2]), Lp, X.XLMR_CLS,
                                      X.XLMR_SEP, fmt=X.PAIR_ROBERTA)
        n = len(enc.ids)
        assert int(lens[0]) == n, (n1, n2, Lp)
        assert ids[0, :n].tolist() == enc.ids and (ids[0, n:] == 0).all(), (n1, n2, Lp)
        assert tt[0, :n].tolist() == enc.type_ids and not tt.any(), (n1, n2, Lp)
        assert (enc.ids.count(4), enc.ids.count(5)) == O.longest_first_lengths(n1, n2, Lp - 4), (n1, n2, Lp)


def test_new_entry_points_are_declared_bound_and_exported():
    from optimized_rag_amd import _lib
    G.build()
    hdr = open(os.path.join(G.ROOT, "include", "rag_hip.h")).read()
    declared = set(re.findall(r"\b(rag_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load_library()
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+RAG_PAIR_BERT\s+0\b", hdr) and re.search(r"#define\s+RAG_PAIR_ROBERTA\s+1\b", hdr)
    assert (_lib.PAIR_BERT, _lib.PAIR_ROBERTA) == (0, 1)
    # no handle: an error code, never a crash (nothing here touches a GPU)
    assert lib.rag_tokens_info(None, None, None, None) != 0 and lib.rag_ce_set_pair_format(None, 0) != 0
    assert lib.rag_tokens_reserve_wide(None, 4, 4, 24) != 0 and lib.rag_tokens_load_wide_host(None, None, None, 4, 4, 24) != 0


def test_shard_records_token_id_max_and_returns_wide_ids_unchanged(tmp_path):
    from optimized_rag_amd import shard_format as SF
    rng = np.random.default_rng(2)
    n, dim, Lt = 9, 8, 5
    tokens = rng.integers(0, 250002, (n, Lt)).astype(np.int32)
    tokens[0, 0], tokens[n - 1, Lt - 1], tokens[3, 2] = 250001, 65536, 65535
    lens = rng.integers(0, Lt + 1, n).astype(np.int32)
    w = SF.ShardWriter(str(tmp_path / "wide"), dim)
    for i in range(n):
        w.add(100 + i, "agent", f"text {i}", rng.standard_normal(dim).astype(np.float32))
    w.close(build_bm25=False, tokens=tokens, token_lens=lens)
    meta = json.loads((tmp_path / "wide" / "meta.json").read_text())
    assert meta["token_id_max"] == 250001 and meta["token_len"] == Lt and meta["version"] == SF.FORMAT_VERSION
    sh = SF.open_shard(str(tmp_path / "wide"))
    try:
        assert sh.token_id_bits() == 24
        assert sh.tokens.dtype == np.int32
        np.testing.assert_array_equal(np.asarray(sh.tokens), tokens)
        np.testing.assert_array_equal(np.asarray(sh.token_lens), lens)
    finally:
        sh.close()
    # ids that fit 16 bits keep the 16-bit store, as does a shard written before the key existed
    w = SF.ShardWriter(str(tmp_path / "narrow"), dim)
    w.add(1, "agent", "text", np.ones(dim, dtype=np.float32))
    w.close(build_bm25=False, tokens=np.full((1, Lt), 65535, dtype=np.int32), token_lens=np.array([Lt], dtype=np.int32))
    sh = SF.open_shard(str(tmp_path / "narrow"))
    assert sh.meta["token_id_max"] == 65535 and sh.token_id_bits() == 16
    del sh.meta["token_id_max"]
    assert sh.token_id_bits() == 16
    sh.close()
    w = SF.ShardWriter(str(tmp_path / "none"), dim)
    w.add(1, "agent", "text", np.ones(dim, dtype=np.float32))
    w.close(build_bm25=False)
    assert "token_id_max" not in json.loads((tmp_path / "none" / "meta.json").read_text())
