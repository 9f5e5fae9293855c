"""CPU: the token-vector and lexical heads of the embedder (bge-m3's three heads, ColBERT checkpoints) without a GPU.
1. tests/m3_tools.py, the float64 reference the GPU tests compare with, against an independent torch float64 restatement of
   FlagEmbedding's BGEM3FlagModel on transformers.XLMRobertaModel: heads, MaxSim (torch.einsum) and the lexical match (a dict loop)
   agree within 1e-10, the bar of the float64-against-float64 tests of tests/test_xlmr_cpu.py.
2. cross_encoder.load_m3_heads on directories with both, one and none of colbert_linear.pt / sparse_linear.pt, a weight of the wrong
   width, a 96-wide head without a bias.
3. The MaxSim reference on hand-made cases: an empty side, one row, all similarities negative.
4. The new entry points are declared, bound and exported."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G
import m3_tools as M
import xlmr_tools as X

NEW_EXPORTS = ["rag_embed_heads_load_host", "rag_embed_multi_host", "rag_embed_multi_dev", "rag_maxsim_host", "rag_maxsim_dev",
               "rag_lexical_match_host", "rag_lexical_match_dev"]
ROW_LENS = [1, 2, 5, 17, 33, 48]
L = 48
SKIP = (0, 1, 2, 3)


def test_m3_tools_equal_an_independent_torch_restatement(tmp_path):
    import torch
    import torch.nn.functional as F
    from safetensors.numpy import load_file
    from safetensors.torch import save_file
    from transformers import XLMRobertaConfig, XLMRobertaModel
    from optimized_rag_amd.cross_encoder import map_checkpoint
    torch.manual_seed(21)
    hf = XLMRobertaConfig(vocab_size=300, hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=256,
                          max_position_embeddings=66, type_vocab_size=1, layer_norm_eps=1e-5, hidden_dropout_prob=0.0,
                          attention_probs_dropout_prob=0.0, pad_token_id=1, bos_token_id=0, eos_token_id=2)
    model = XLMRobertaModel(hf).double().eval()
    d = tmp_path / "enc"
    d.mkdir()
    save_file({k: v.contiguous() for k, v in model.state_dict().items()}, str(d / "model.safetensors"))
    cfg, w = map_checkpoint(json.loads(hf.to_json_string()), load_file(str(d / "model.safetensors")), head=False)
    rng = np.random.default_rng(5)
    lens = np.array(ROW_LENS, dtype=np.int64)
    ids = rng.integers(4, 40, (len(lens), L)).astype(np.int64)           # a small id range: texts share ids, ids repeat inside a text
    ids[:, 0] = 0
    ids[np.arange(len(lens)), lens - 1] = 2
    ids[0, 0] = 0
    mask = np.arange(L)[None, :] < lens[:, None]
    ids[~mask] = 1
    heads = M.seeded_heads(128, 96, 3)
    ref = M.heads_reference(w, cfg, ids, np.zeros_like(ids), lens, heads)
    pq = [0, 1, 2, 3, 4, 5, 5, 3]
    pd = [5, 4, 3, 2, 1, 0, 5, 0]
    got = M.score_pairs(ref, ids, lens, pq, pd, SKIP)

    # ---- the restatement: transformers for the encoder, torch for the heads and scores, nothing shared with m3_tools
    with torch.no_grad():
        hid = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask.astype(np.int64))).last_hidden_state
        tw, tb = torch.from_numpy(heads["tok_w"]).double(), torch.from_numpy(heads["tok_b"]).double()
        lw = torch.from_numpy(heads["lex_w"]).double()
        dense = F.normalize(hid[:, 0], dim=-1)
        lex = torch.relu(hid @ lw + heads["lex_b"])
        col = F.normalize(F.linear(hid[:, 1:], tw, tb), dim=-1)
    want = {k: [] for k in M.SCORE_KEYS}
    for p in range(len(lens)):
        n = int(lens[p])
        assert float((dense[p] - torch.from_numpy(ref["dense"][p])).abs().max()) <= 1e-10
        assert float((lex[p, :n] - torch.from_numpy(ref["lex"][p, :n])).abs().max()) <= 1e-10 and (ref["lex"][p, n:] == 0).all()
        assert ref["vecs"][p].shape == (n - 1, 96)
        if n > 1:
            assert float((col[p, :n - 1] - torch.from_numpy(ref["vecs"][p])).abs().max()) <= 1e-10
    assert (ref["lex"] > 0).any() and (ref["lex"][mask] == 0).any()       # the relu cuts some and keeps some

    def lexmap(p):
        m = {}
        for t in range(int(lens[p])):
            k, v = int(ids[p, t]), float(lex[p, t])
            if k in SKIP or v <= 0:
                continue
            m[k] = max(m.get(k, 0.0), v)
        return m

    for q, dd in zip(pq, pd):
        nq, nd = int(lens[q]) - 1, int(lens[dd]) - 1
        if nq == 0 or nd == 0:
            c = 0.0
        else:
            c = float(torch.einsum("in,jn->ij", col[q, :nq], col[dd, :nd]).max(-1).values.sum() / nq)
        mq, md = lexmap(q), lexmap(dd)
        s = 0.0
        for k, v in mq.items():
            if k in md:
                s += v * md[k]
        dn = float(dense[q] @ dense[dd])
        want["colbert"].append(c)
        want["sparse"].append(s)
        want["dense"].append(dn)
        want["sparse+dense"].append((0.2 * s + 0.4 * dn) / 0.6)
        want["colbert+sparse+dense"].append((0.4 * c + 0.2 * s + 0.4 * dn) / 1.0)
    for k in M.SCORE_KEYS:
        err = float(np.abs(np.asarray(want[k]) - got[k]).max())
        print(k, "max |m3_tools - torch restatement|:", err)
        assert err <= 1e-10, k
    assert max(want["sparse"]) > 0 and got["colbert"][0] == 0.0           # shared ids exist; a one-token text has no rows


def test_load_m3_heads_both_one_none_wrong_width_and_no_bias(tmp_path):
    import torch
    from optimized_rag_amd.cross_encoder import load_m3_heads
    heads = M.seeded_heads(128, 128, 1)
    both, one, none, bad, nobias = (tmp_path / n for n in ("both", "one", "none", "bad", "nobias"))
    for d in (both, one, none, bad, nobias):
        d.mkdir()
        (d / "config.json").write_text(json.dumps(dict(hidden_size=128)))
    M.write_head_files(both, heads)
    got = load_m3_heads(str(both))
    np.testing.assert_array_equal(got["tok_w"], heads["tok_w"])
    np.testing.assert_array_equal(got["tok_b"], heads["tok_b"])
    np.testing.assert_array_equal(got["lex_w"], heads["lex_w"])
    assert got["lex_w"].shape == (128,) and got["lex_b"] == heads["lex_b"] and got["tok_w"].dtype == np.float32
    M.write_head_files(one, dict(lex_w=heads["lex_w"], lex_b=heads["lex_b"]))
    got = load_m3_heads(str(one), hidden=128)
    assert got["tok_w"] is None and got["tok_b"] is None and got["lex_w"].shape == (128,)
    got = load_m3_heads(str(none))
    assert got == dict(tok_w=None, tok_b=None, lex_w=None, lex_b=0.0)
    M.write_head_files(bad, heads)
    with pytest.raises(ValueError, match="colbert_linear.pt"):
        load_m3_heads(str(bad), hidden=256)
    torch.save({"weight": torch.zeros(2, 128)}, str(bad / "sparse_linear.pt"))
    os.remove(str(bad / "colbert_linear.pt"))
    with pytest.raises(ValueError, match="sparse_linear.pt"):
        load_m3_heads(str(bad))
    h96 = M.seeded_heads(128, 96, 2, bias=False)
    M.write_head_files(nobias, dict(tok_w=h96["tok_w"], tok_b=None))
    got = load_m3_heads(str(nobias))
    assert got["tok_w"].shape == (96, 128) and got["tok_b"] is None and got["lex_w"] is None
    torch.save({"weight": torch.zeros(40, 128)}, str(nobias / "colbert_linear.pt"))       # 40 is no multiple of 32
    with pytest.raises(ValueError, match="colbert_linear.pt"):
        load_m3_heads(str(nobias))


def test_maxsim_reference_on_hand_made_cases():
    e = np.eye(4)
    assert M.maxsim(np.zeros((0, 4)), e) == 0.0 and M.maxsim(e, np.zeros((0, 4))) == 0.0
    assert M.maxsim(e[:1], e[:1]) == 1.0 and M.maxsim(e[:1], e[1:2]) == 0.0
    # one query row against two rows: the larger dot; two query rows: the mean of their maxima
    assert M.maxsim(np.array([[1.0, 0, 0, 0]]), np.array([[0.5, 0, 0, 0], [0.25, 0, 0, 0]])) == 0.5
    assert M.maxsim(np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0]]), np.array([[0.5, 0.125, 0, 0]])) == (0.5 + 0.125) / 2
    # every similarity negative: the maximum is the least negative one, never 0
    assert M.maxsim(np.array([[1.0, 0, 0, 0]]), np.array([[-0.5, 0, 0, 0], [-0.25, 0, 0, 0]])) == -0.25
    assert M.lexical_score({5: 0.5, 7: 2.0}, {7: 0.25, 9: 1.0}) == 0.5
    assert M.lexical_map([5, 5, 7, 0, 9], [0.5, 0.75, -1.0, 3.0, 0.0], 5, {0}) == {5: 0.75}


def test_new_entry_points_are_declared_bound_and_exported():
    G.build()
    import optimized_rag_amd
    from optimized_rag_amd import _lib
    lib = optimized_rag_amd.load_library()
    hdr = open(os.path.join(G.ROOT, "include", "rag_hip.h")).read()
    declared = set(re.findall(r"\b(rag_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert lib.rag_maxsim_host.argtypes[-1] is ctypes.c_void_p
    for m in ("embed_heads_load", "embed_multi", "embed_multi_dev", "maxsim", "maxsim_dev", "lexical_match", "lexical_match_dev"):
        assert callable(getattr(_lib.RagEngine, m)), m
    from optimized_rag_amd.reranker import LateInteractionReranker
    assert LateInteractionReranker(None).is_available() is False and LateInteractionReranker(None).rerank("q", [{"content": "a"}], 3) == [{"content": "a"}]
    with pytest.raises(ValueError):
        LateInteractionReranker(None, mode="cross")
