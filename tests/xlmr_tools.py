"""Shared by tests/test_xlmr_cpu.py, tests/test_xlmr_gpu.py and tests/test_wide_tokens_gpu.py: the numpy pair builder for both pair
layouts (rag_ce_set_pair_format), the relabelling of an XLM-RoBERTa state dict into the names oracle/bert_oracle.py reads - written
out by hand here, independently of optimized_rag_amd.cross_encoder.map_checkpoint, which the tests compare with it - and small
seeded XLM-R-shaped checkpoints that need neither transformers nor a download."""
import json

import numpy as np

from oracle import bert_oracle as B
from oracle import rag_oracle as O

PAIR_BERT, PAIR_ROBERTA = 0, 1
XLMR_CLS, XLMR_PAD, XLMR_SEP = 0, 1, 2           # <s>, <pad>, </s> of XLM-R's vocabulary


def build_pairs(q_tok, q_len, cand, tok, tok_len, L, cls_id, sep_id, fmt=PAIR_BERT, id_base=0):
    """cand [Q, pool] doc ids (id_base + row, -1 or a row outside the store = empty passage) -> ids, token types [Q * pool, L] and
    lens [Q * pool] as rag_ce_build_pairs_dev writes them: 'longest_first' over L - 3 (BERT) or L - 4 (RoBERTa) content tokens."""
    Q, pool = cand.shape
    extra = 1 if fmt == PAIR_ROBERTA else 0
    ids = np.zeros((Q * pool, L), dtype=np.int32)
    tt = np.zeros((Q * pool, L), dtype=np.int32)
    lens = np.zeros(Q * pool, dtype=np.int32)
    for q in range(Q):
        for j in range(pool):
            r = int(cand[q, j]) - id_base if cand[q, j] >= 0 else -1
            have = 0 <= r < tok.shape[0]
            n1 = max(0, int(min(q_len[q], q_tok.shape[1])))
            n2 = max(0, int(min(tok_len[r], tok.shape[1]))) if have else 0
            ql, dl = O.longest_first_lengths(n1, n2, L - 3 - extra)
            row = [cls_id] + [int(t) for t in q_tok[q, :ql]] + [sep_id] * (1 + extra) + ([int(t) for t in tok[r, :dl]] if have else []) + [sep_id]
            p = q * pool + j
            ids[p, :len(row)] = row
            if fmt == PAIR_BERT:
                tt[p, ql + 2:len(row)] = 1
            lens[p] = len(row)
    return ids, tt, lens


def device_pairs(eng, q_tok, q_len, cand, L, cls_id, sep_id, id_base=0):
    """rag_ce_build_pairs_dev on numpy inputs -> numpy (ids, tt, lens); the outputs start poisoned, so an unwritten slot shows."""
    import torch
    Q, pool = cand.shape
    ids = torch.full((Q * pool, L), -7, dtype=torch.int32, device="cuda")
    tt = torch.full((Q * pool, L), -7, dtype=torch.int32, device="cuda")
    lens = torch.full((Q * pool,), -7, dtype=torch.int32, device="cuda")
    eng.ce_build_pairs_dev(torch.from_numpy(np.ascontiguousarray(q_tok, dtype=np.int32)).cuda(),
                           torch.from_numpy(np.ascontiguousarray(q_len, dtype=np.int32)).cuda(),
                           torch.from_numpy(np.ascontiguousarray(cand, dtype=np.int64)).cuda(), ids, tt, lens, token_id_base=id_base,
                           cls_id=cls_id, sep_id=sep_id)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), tt.cpu().numpy(), lens.cpu().numpy()


def xlmr_to_bert_names(sd, pad_token_id=XLMR_PAD, type_rows=1, head=True):
    """An XLM-R state dict (prefix `roberta.` or none) under BERT's names: the position table without its first pad_token_id + 1
    rows, classifier.dense as the pooler, classifier.out_proj as the classifier, the one token-type row `type_rows` times."""
    src = "roberta." if any(k.startswith("roberta.") for k in sd) else ""
    out = {}
    for k, v in sd.items():
        if not k.startswith(src) or k.startswith("classifier.") or "pooler" in k or k.endswith("position_ids"):
            continue
        out["bert." + k[len(src):]] = np.asarray(v)
    pos = "bert.embeddings.position_embeddings.weight"
    out[pos] = out[pos][pad_token_id + 1:]
    typ = "bert.embeddings.token_type_embeddings.weight"
    out[typ] = np.repeat(out[typ][:1], type_rows, axis=0)
    if head:
        out["bert.pooler.dense.weight"], out["bert.pooler.dense.bias"] = np.asarray(sd["classifier.dense.weight"]), np.asarray(sd["classifier.dense.bias"])
        out["classifier.weight"], out["classifier.bias"] = np.asarray(sd["classifier.out_proj.weight"]), np.asarray(sd["classifier.out_proj.bias"])
    return out


def xlmr_hf_config(vocab_size=70000, hidden=128, layers=2, heads=4, ffn=512, max_position_embeddings=66, eps=1e-5, **more):
    """config.json of an XLM-R checkpoint of this shape, as transformers writes the keys the loader reads."""
    cfg = dict(model_type="xlm-roberta", vocab_size=vocab_size, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads,
               intermediate_size=ffn, max_position_embeddings=max_position_embeddings, type_vocab_size=1, layer_norm_eps=eps,
               hidden_act="gelu", position_embedding_type="absolute", pad_token_id=XLMR_PAD, bos_token_id=XLMR_CLS, eos_token_id=XLMR_SEP)
    cfg.update(more)
    return cfg


def seeded_xlmr(hf_cfg, seed, head=True, prefix="roberta."):
    """A seeded float32 state dict under XLM-R's names for hf_cfg (oracle.bert_oracle.seeded_weights renamed; the pad_token_id + 1
    reserved position rows are filled with large values, so reading one would show)."""
    pad = hf_cfg["pad_token_id"]
    cfg = dict(vocab_size=hf_cfg["vocab_size"], hidden=hf_cfg["hidden_size"], layers=hf_cfg["num_hidden_layers"],
               heads=hf_cfg["num_attention_heads"], ffn=hf_cfg["intermediate_size"], max_pos=hf_cfg["max_position_embeddings"] - pad - 1,
               type_vocab=1, eps=hf_cfg["layer_norm_eps"])
    w = B.seeded_weights(cfg, seed)
    sd = {}
    for k, v in w.items():
        if k.startswith("bert.pooler.dense."):
            if head:
                sd["classifier.dense." + k.rsplit(".", 1)[1]] = v
        elif k.startswith("classifier."):
            if head:
                sd["classifier.out_proj." + k.rsplit(".", 1)[1]] = v
        else:
            sd[prefix + k[len("bert."):]] = v
    pos = prefix + "embeddings.position_embeddings.weight"
    sd[pos] = np.concatenate([np.full((pad + 1, cfg["hidden"]), 50.0, dtype=np.float32), sd[pos]])
    return sd


def write_checkpoint(d, hf_cfg, sd, words=None, word_ids=None):
    """config.json + model.safetensors (+ a WordLevel tokenizer.json with XLM-R's pair template over `words`) in directory d."""
    from safetensors.numpy import save_file
    d.mkdir(parents=True, exist_ok=True)
    (d / "config.json").write_text(json.dumps(hf_cfg))
    save_file({k: np.ascontiguousarray(v) for k, v in sd.items()}, str(d / "model.safetensors"))
    if words is not None:
        roberta_tokenizer(words, word_ids).save(str(d / "tokenizer.json"))
    return str(d)


def roberta_tokenizer(words, word_ids=None):
    """`tokenizers` WordLevel model over <s> <pad> </s> <unk> + words with the RoBERTa / XLM-R template <s> $A </s> </s> $B </s>.
    word_ids: the id of each word (default 4, 5, ...): lets a small word list reach ids anywhere in a 250k-entry vocabulary; the ids
    between them get filler entries, as a vocabulary with holes makes `tokenizers` print every missing id when it is saved."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    by_id = {XLMR_CLS: "<s>", XLMR_PAD: "<pad>", XLMR_SEP: "</s>", 3: "<unk>"}
    by_id.update({int(i): w for w, i in zip(words, word_ids if word_ids is not None else range(4, 4 + len(words)))})
    vocab = {by_id.get(i, f"<filler{i}>"): i for i in range(max(by_id) + 1)}
    tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tok.post_processor = processors.TemplateProcessing(single="<s> $A </s>", pair="<s> $A </s> </s> $B </s>",
                                                       special_tokens=[("<s>", XLMR_CLS), ("</s>", XLMR_SEP)])
    return tok
