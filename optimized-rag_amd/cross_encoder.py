"""Host side of the cross-encoder (K7): local checkpoint loading (BERT, and RoBERTa / XLM-RoBERTa relabelled as BERT:
map_checkpoint), tokenisation of (query, doc) pairs (WordPiece from vocab.txt, or whatever tokenizer.json describes) and
batching into rag_ce_score_host. Stands where `sentence_transformers.CrossEncoder` stands in the reference
(/root/reference/rag/reranker.py:312-313,355): `predict(pairs)` returns RAW logits (the ms-marco checkpoints use an
identity activation, which is why the reference applies its own sigmoid at :359).

Weights are read with `safetensors` (numpy) and handed to the HIP engine as float32 arrays; PyTorch is not needed.
"""
import json
import os

import numpy as np

from .engine import get_engine

LAYER_KEYS = ["attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight",
              "attention.self.key.bias", "attention.self.value.weight", "attention.self.value.bias",
              "attention.output.dense.weight", "attention.output.dense.bias", "attention.output.LayerNorm.weight",
              "attention.output.LayerNorm.bias", "intermediate.dense.weight", "intermediate.dense.bias",
              "output.dense.weight", "output.dense.bias", "output.LayerNorm.weight", "output.LayerNorm.bias"]


def flatten_state_dict(sd, n_layers, head=True, prefix="bert."):
    """HF BertForSequenceClassification state dict -> the tensor order rag_ce_load_host expects. head=False: a plain BertModel
    encoder for rag_embed_load_host (no pooler / classifier; sentence-transformers checkpoints store it without the `bert.`
    prefix: prefix="")."""
    names = [prefix + "embeddings.word_embeddings.weight", prefix + "embeddings.position_embeddings.weight",
             prefix + "embeddings.token_type_embeddings.weight", prefix + "embeddings.LayerNorm.weight",
             prefix + "embeddings.LayerNorm.bias"]
    for l in range(n_layers):
        names += [f"{prefix}encoder.layer.{l}.{k}" for k in LAYER_KEYS]
    if head:
        names += [prefix + "pooler.dense.weight", prefix + "pooler.dense.bias", "classifier.weight", "classifier.bias"]
    missing = [n for n in names if n not in sd]
    if missing:
        raise KeyError(f"checkpoint lacks {missing[:3]}{'...' if len(missing) > 3 else ''}")
    return [np.ascontiguousarray(np.asarray(sd[n], dtype=np.float32)) for n in names]


def config_from_hf(cfg):
    """config.json of the checkpoint -> engine config (shape comes from the checkpoint, nothing is hard-coded)."""
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise ValueError("only exact-erf GELU checkpoints are supported")
    return dict(vocab_size=cfg["vocab_size"], hidden=cfg["hidden_size"], layers=cfg["num_hidden_layers"],
                heads=cfg["num_attention_heads"], ffn=cfg["intermediate_size"], max_pos=cfg["max_position_embeddings"],
                type_vocab=cfg.get("type_vocab_size", 2), eps=cfg.get("layer_norm_eps", 1e-12))


ROBERTA_TYPES = ("xlm-roberta", "roberta")


def map_checkpoint(hf_cfg, sd, head=True):
    """config.json (a dict) and a state dict -> (engine config, state dict under the names flatten_state_dict(prefix="bert.")
    reads). Pure: no engine, no file, no cast - the tensors keep their dtype, so a float64 checkpoint stays float64.

    model_type `bert` (or none): the names are taken with the prefix `bert.` or none. head=True wants the pooler and a one-logit
    classifier; head=False a bare encoder (a pooler, when the file has one, is left out).
    model_type `xlm-roberta` / `roberta` (prefix `roberta.` or none): the same encoder under other names, with two differences.
    RoBERTa numbers the real tokens of a right-padded row pad_token_id + 1, pad_token_id + 2, ...: the position table loses its
    first pad_token_id + 1 rows and max_pos = max_position_embeddings - pad_token_id - 1, after which position = token index as
    in BERT. RobertaClassificationHead is dense + tanh + out_proj on row 0, which is BERT's pooler + classifier:
    classifier.dense -> bert.pooler.dense, classifier.out_proj -> classifier. Such a model has ONE token type (the engine then
    gives every token row 0 of the type table) and its pairs are laid out [cls] q [sep] [sep] d [sep]: the config carries
    pair_format = 1 and cls_id / sep_id = bos_token_id / eos_token_id for rag_ce_set_pair_format and the pair builder.
    (The engine takes a row's real tokens to be its first `len` ones; a pad id INSIDE a text would shift transformers' position
    numbers, which no tokenizer produces.)
    ValueError: position_embedding_type other than absolute, a GELU that is not the exact erf one, more than one label."""
    mt = hf_cfg.get("model_type", "bert")
    if mt != "bert" and mt not in ROBERTA_TYPES:
        raise ValueError(f"unsupported model_type {mt!r}: bert, roberta and xlm-roberta checkpoints are supported")
    if hf_cfg.get("position_embedding_type", "absolute") != "absolute":
        raise ValueError(f"unsupported position_embedding_type {hf_cfg['position_embedding_type']!r}: only absolute positions")
    cfg = config_from_hf(hf_cfg)                                  # raises on a non-erf GELU
    roberta = mt in ROBERTA_TYPES
    src = "roberta." if roberta else "bert."
    if not any(k.startswith(src) for k in sd):
        src = ""
    names = ["embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight",
             "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
    names += [f"encoder.layer.{l}.{k}" for l in range(cfg["layers"]) for k in LAYER_KEYS]
    pairs = [(src + n, "bert." + n) for n in names]
    if head:
        hd = ("classifier.dense.", "classifier.out_proj.") if roberta else (src + "pooler.dense.", "classifier.")
        pairs += [(hd[0] + t, "bert.pooler.dense." + t) for t in ("weight", "bias")] + [(hd[1] + t, "classifier." + t) for t in ("weight", "bias")]
    missing = [a for a, _ in pairs if a not in sd]
    if missing:
        raise KeyError(f"checkpoint lacks {missing[:3]}{'...' if len(missing) > 3 else ''}")
    out = {b: sd[a] for a, b in pairs}
    if head and (int(hf_cfg.get("num_labels", 1)) != 1 or len(hf_cfg.get("id2label", {0: 0})) != 1 or out["classifier.weight"].shape[0] != 1):
        raise ValueError("only single-logit classifiers are supported (num_labels = 1)")
    if roberta:
        pad = int(hf_cfg.get("pad_token_id", 1))
        cfg["max_pos"] = cfg["max_pos"] - pad - 1
        out["bert.embeddings.position_embeddings.weight"] = out["bert.embeddings.position_embeddings.weight"][pad + 1:]
        if cfg["max_pos"] < 1:
            raise ValueError("max_position_embeddings leaves no position after the pad_token_id + 1 reserved rows")
        cfg.update(pair_format=1, cls_id=int(hf_cfg.get("bos_token_id", 0)), sep_id=int(hf_cfg.get("eos_token_id", 2)))
    return cfg, out


def load_tokenizer(path):
    """The tokenizer of a checkpoint directory: tokenizer.json (any model of the `tokenizers` package, with its own special-token
    template: XLM-R's SentencePiece one writes <s> a </s> </s> b </s>) when it is there, else WordPiece from vocab.txt."""
    tj = os.path.join(path, "tokenizer.json")
    if os.path.exists(tj):
        from tokenizers import Tokenizer
        return Tokenizer.from_file(tj)
    from tokenizers import BertWordPieceTokenizer
    lower = True
    tk_cfg = os.path.join(path, "tokenizer_config.json")
    if os.path.exists(tk_cfg):
        with open(tk_cfg) as f:
            lower = bool(json.load(f).get("do_lower_case", True))
    return BertWordPieceTokenizer(os.path.join(path, "vocab.txt"), lowercase=lower)


M3_HEAD_FILES = {"tok": "colbert_linear.pt", "lex": "sparse_linear.pt"}


def load_m3_heads(path, hidden=None):
    """The optional heads beside model.safetensors in a bge-m3-style directory: colbert_linear.pt (token vectors, nn.Linear hidden ->
    tok_dim) and sparse_linear.pt (lexical weights, nn.Linear hidden -> 1), each a torch state dict holding `weight` and maybe
    `bias`. Pure: no engine. Returns dict(tok_w [tok_dim, hidden] | None, tok_b [tok_dim] | None, lex_w [hidden] | None, lex_b float)
    as float32 numpy; a file that is not there leaves its entries None. hidden defaults to config.json's hidden_size.
    ValueError naming the file: a weight whose shape does not fit hidden, a tok_dim that is no multiple of 32 in [32, 1024]."""
    if hidden is None:
        with open(os.path.join(path, "config.json")) as f:
            hidden = json.load(f)["hidden_size"]
    hidden = int(hidden)
    out = dict(tok_w=None, tok_b=None, lex_w=None, lex_b=0.0)
    for kind, name in M3_HEAD_FILES.items():
        fp = os.path.join(path, name)
        if not os.path.exists(fp):
            continue
        import torch
        sd = torch.load(fp, map_location="cpu", weights_only=True)
        if "weight" not in sd:
            raise ValueError(f"{fp}: no `weight` in the state dict")
        w = np.ascontiguousarray(sd["weight"].detach().to(torch.float32).numpy())
        b = sd.get("bias")
        b = None if b is None else np.ascontiguousarray(b.detach().to(torch.float32).numpy()).reshape(-1)
        if w.ndim != 2 or w.shape[1] != hidden:
            raise ValueError(f"{fp}: weight of shape {tuple(w.shape)} does not fit hidden {hidden}")
        if b is not None and b.shape[0] != w.shape[0]:
            raise ValueError(f"{fp}: bias of {b.shape[0]} entries does not fit weight of shape {tuple(w.shape)}")
        if kind == "tok":
            if w.shape[0] % 32 or not 32 <= w.shape[0] <= 1024:
                raise ValueError(f"{fp}: token dimension {w.shape[0]} is not a multiple of 32 in [32, 1024]")
            out["tok_w"], out["tok_b"] = w, b
        else:
            if w.shape[0] != 1:
                raise ValueError(f"{fp}: weight of shape {tuple(w.shape)} is not one row of {hidden}")
            out["lex_w"], out["lex_b"] = w[0].copy(), 0.0 if b is None else float(b[0])
    return out


MINILM_L6_CONFIG = dict(vocab_size=30522, hidden=384, layers=6, heads=12, ffn=1536, max_pos=512, type_vocab=2, eps=1e-12)
"""Shape of cross-encoder/ms-marco-MiniLM-L-6-v2 (the checkpoint the reference names at config.py:49), for benchmarks
that run without the downloaded weights; a real deployment takes the shape from the checkpoint's config.json."""


def random_init_tensors(cfg, seed=0):
    """Random-init weights of the architecture in rag_ce_load_host's tensor order (benchmarks have no checkpoint: there
    is no network). Scales are those of a trained BERT (0.02-0.1), LayerNorm gains around 1."""
    rng = np.random.default_rng(seed)
    H, F = cfg["hidden"], cfg["ffn"]

    def mat(*shape, s=0.05):
        return (rng.standard_normal(shape) * s).astype(np.float32)

    def gain():
        return (1.0 + mat(H, s=0.1)).astype(np.float32)

    out = [mat(cfg["vocab_size"], H, s=0.1), mat(cfg["max_pos"], H, s=0.1), mat(cfg.get("type_vocab", 2), H, s=0.1), gain(), mat(H, s=0.1)]
    for _ in range(cfg["layers"]):
        out += [mat(H, H, s=0.08), mat(H), mat(H, H, s=0.08), mat(H), mat(H, H, s=0.08), mat(H),      # q, k, v
                mat(H, H), mat(H), gain(), mat(H, s=0.1),                                              # attention output + LN
                mat(F, H), mat(F), mat(H, F), mat(H), gain(), mat(H, s=0.1)]                           # FFN + LN
    out += [mat(H, H), mat(H), mat(1, H, s=0.5), mat(1, s=0.5)]                                        # pooler, classifier
    return out


def seq_limit(cfg):
    """The longest sequence, in tokens, a call on a model of this config may carry (rag_model_seq_limit): its position table, capped
    at 8192 for 64-wide heads (the streamed attention kernel) and at 512 for 32-wide heads."""
    return min(cfg["max_pos"], 8192 if cfg["hidden"] // cfg["heads"] == 64 else 512)


class LocalCrossEncoder:
    def __init__(self, cfg, tensors, tokenizer, max_length=512, engine=None, batch_pairs=4096):
        self.cfg = cfg
        self.engine = engine or get_engine()
        self.tokenizer = tokenizer
        self.max_length = min(int(max_length), seq_limit(cfg))
        self.batch_pairs = batch_pairs
        # what the device-side pair builder needs to assemble the pairs this model was trained on (rag_ce_set_pair_format,
        # the cls_id / sep_id arguments of retrieve_rerank_dev and ce_build_pairs_dev), and the width a token store must have
        self.pair_format = int(cfg.get("pair_format", 0))
        self.vocab_size = int(cfg["vocab_size"])
        tid = getattr(tokenizer, "token_to_id", lambda t: None)
        self.cls_id = int(cfg["cls_id"]) if "cls_id" in cfg else (101 if tid("[CLS]") is None else tid("[CLS]"))
        self.sep_id = int(cfg["sep_id"]) if "sep_id" in cfg else (102 if tid("[SEP]") is None else tid("[SEP]"))
        self.engine.ce_load(cfg, tensors)
        self.engine.ce_set_pair_format(self.pair_format)

    @classmethod
    def from_dir(cls, path, max_length=512, engine=None):
        from safetensors.numpy import load_file
        with open(os.path.join(path, "config.json")) as f:
            cfg, sd = map_checkpoint(json.load(f), load_file(os.path.join(path, "model.safetensors")))
        return cls(cfg, flatten_state_dict(sd, cfg["layers"]), load_tokenizer(path), max_length=max_length, engine=engine)

    def tokenize_pairs(self, pairs):
        """[CLS] q [SEP] d [SEP], token_type 0/1 (or the tokenizer.json's own template: <s> q </s> </s> d </s>, all 0), truncation
        'longest_first' to max_length, padded to the longest."""
        self.tokenizer.enable_truncation(max_length=self.max_length, strategy="longest_first")
        self.tokenizer.no_padding()
        enc = self.tokenizer.encode_batch([(str(q), str(d)) for q, d in pairs])
        L = max(len(e.ids) for e in enc)
        ids = np.zeros((len(enc), L), dtype=np.int32)
        tt = np.zeros((len(enc), L), dtype=np.int32)
        lens = np.zeros((len(enc),), dtype=np.int32)
        for i, e in enumerate(enc):
            n = len(e.ids)
            ids[i, :n] = e.ids
            tt[i, :n] = e.type_ids
            lens[i] = n
        return ids, tt, lens

    def predict(self, pairs):
        out = np.empty((len(pairs),), dtype=np.float32)
        for b in range(0, len(pairs), self.batch_pairs):
            ids, tt, lens = self.tokenize_pairs(pairs[b:b + self.batch_pairs])
            out[b:b + len(lens)] = self.engine.ce_score(ids, tt, lens)
        return out
