"""CPU: what the 64-wide-head GPU tests (tests/test_head64_gpu.py) rest on.

1. oracle/bert_oracle.py at head dim 64 (128 / 2 and 768 / 12, 2 layers) against transformers.BertModel in float64, within 1e-12
   on the real tokens: the oracle is generic in the head dimension, and this pins it there.
2. LocalEmbeddingService.from_dir's reading of sentence-transformers' 1_Pooling/config.json, over a stub engine: mean, [CLS], the
   missing file (mean) and an unsupported mode (a ValueError that names it)."""
import json

import numpy as np
import pytest

from oracle import bert_oracle as B


@pytest.mark.parametrize("hidden,heads", [(128, 2), (768, 12)])
def test_oracle_at_head_dim_64_matches_transformers_bert_model(hidden, heads):
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    cfg = dict(vocab_size=300, hidden=hidden, layers=2, heads=heads, ffn=4 * hidden, max_pos=40, type_vocab=2, eps=1e-12)
    assert cfg["hidden"] // cfg["heads"] == 64
    w = B.seeded_weights(cfg, 64 + hidden)
    hf = tr.BertModel(tr.BertConfig(
        vocab_size=300, hidden_size=hidden, num_hidden_layers=2, num_attention_heads=heads, intermediate_size=4 * hidden,
        max_position_embeddings=40, type_vocab_size=2, hidden_act="gelu", layer_norm_eps=1e-12), add_pooling_layer=False).eval().double()
    sd = hf.state_dict()
    for k in sd:
        sd[k].copy_(torch.from_numpy(w["bert." + k]).double())
    rng = np.random.default_rng(hidden)
    P, L = 5, 33
    lens = np.array([33, 1, 17, 16, 32])
    ids = rng.integers(1, 300, (P, L))
    tt = (np.arange(L)[None, :] >= 9).astype(np.int64) * np.ones((P, 1), dtype=np.int64)
    mask = (np.arange(L)[None] < lens[:, None]).astype(np.int64)
    with torch.no_grad():
        ref = hf(input_ids=torch.from_numpy(ids), token_type_ids=torch.from_numpy(tt),
                 attention_mask=torch.from_numpy(mask)).last_hidden_state.numpy()
    _, mine = B.forward_hidden(w, cfg, ids, tt, lens)
    real = mask.astype(bool)
    err = np.abs(mine - ref)[real].max()
    assert err < 1e-12, err
    # the two heads the GPU tests compare: the [CLS] row and the masked mean of the same hidden state
    assert np.abs(mine[:, 0] - ref[:, 0]).max() < 1e-12
    m = mask[:, :, None].astype(np.float64)
    mean_ref = (ref * m).sum(1) / m.sum(1)
    assert np.abs(B.sentence_embeddings(w, cfg, ids, tt, lens, normalize=False) - mean_ref).max() < 1e-12


# ---- from_dir and 1_Pooling/config.json -------------------------------------------------------------------------------------
CFG = dict(vocab_size=40, hidden=128, layers=1, heads=2, ffn=128, max_pos=32, type_vocab=2, eps=1e-12)
WORDS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(35)]


class StubEngine:
    """Records embed_load's arguments; no library, no GPU."""

    def __init__(self):
        self.loads = []

    def embed_load(self, cfg, tensors, normalize=True, pooling="mean"):
        self.loads.append(dict(cfg=cfg, n=len(tensors), normalize=normalize, pooling=pooling))


def _checkpoint(tmp_path, pooling_cfg):
    from safetensors.numpy import save_file
    d = tmp_path / "encoder"
    d.mkdir()
    (d / "vocab.txt").write_text("\n".join(WORDS) + "\n")
    c = CFG
    (d / "config.json").write_text(json.dumps(dict(vocab_size=c["vocab_size"], hidden_size=c["hidden"], num_hidden_layers=c["layers"],
                                                   num_attention_heads=c["heads"], intermediate_size=c["ffn"],
                                                   max_position_embeddings=c["max_pos"], type_vocab_size=2, hidden_act="gelu",
                                                   layer_norm_eps=1e-12)))
    w = B.seeded_weights(CFG, 1)
    save_file({k[len("bert."):]: v for k, v in w.items() if k.startswith("bert.") and "pooler" not in k}, str(d / "model.safetensors"))
    if pooling_cfg is not None:
        (d / "1_Pooling").mkdir()
        (d / "1_Pooling" / "config.json").write_text(json.dumps(pooling_cfg))
    return str(d)


def _st_pooling(**on):
    """1_Pooling/config.json as sentence-transformers writes it: every mode present, the chosen ones true."""
    cfg = dict(word_embedding_dimension=CFG["hidden"], pooling_mode_cls_token=False, pooling_mode_mean_tokens=False,
               pooling_mode_max_tokens=False, pooling_mode_mean_sqrt_len_tokens=False, pooling_mode_weightedmean_tokens=False,
               pooling_mode_lasttoken=False, include_prompt=True)
    cfg.update(on)
    return cfg


@pytest.mark.parametrize("pooling_cfg,expect", [
    (None, "mean"),
    (_st_pooling(pooling_mode_mean_tokens=True), "mean"),
    (_st_pooling(pooling_mode_cls_token=True), "cls"),
    (dict(word_embedding_dimension=128, pooling_mode_cls_token=True, pooling_mode_mean_tokens=False), "cls"),   # the older, shorter file
], ids=["no-file", "mean", "cls", "cls-short-file"])
def test_from_dir_takes_the_pooling_mode_of_the_checkpoint(tmp_path, pooling_cfg, expect):
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    eng = StubEngine()
    svc = LocalEmbeddingService.from_dir(_checkpoint(tmp_path, pooling_cfg), engine=eng, normalize=False)
    assert svc.pooling == expect
    assert eng.loads == [dict(cfg=svc.cfg, n=5 + 16 * CFG["layers"], normalize=False, pooling=expect)]     # normalize: the caller's
    assert svc.get_embedding_dimension() == CFG["hidden"] and svc.cfg["heads"] == 2


@pytest.mark.parametrize("on,named", [
    (dict(pooling_mode_max_tokens=True), "max"),
    (dict(pooling_mode_weightedmean_tokens=True), "weightedmean"),
    (dict(pooling_mode_lasttoken=True), "lasttoken"),
    (dict(pooling_mode_mean_sqrt_len_tokens=True), "mean_sqrt_len"),
    (dict(pooling_mode_cls_token=True, pooling_mode_mean_tokens=True), "cls+mean"),
])
def test_from_dir_refuses_a_pooling_mode_the_engine_has_no_head_for(tmp_path, on, named):
    from optimized_rag_amd.embeddings import LocalEmbeddingService
    eng = StubEngine()
    with pytest.raises(ValueError, match=named.replace("+", r"\+")):
        LocalEmbeddingService.from_dir(_checkpoint(tmp_path, _st_pooling(**on)), engine=eng)
    assert eng.loads == []


def test_the_engine_binding_refuses_an_unknown_pooling_name():
    from optimized_rag_amd._lib import RagEngine
    with pytest.raises(ValueError, match="median"):
        RagEngine.embed_load(object(), CFG, [], pooling="median")
