"""Local embedding service on the GPU: the class surface of the reference's `EmbeddingService`
(/root/reference/memory/embeddings.py: generate_embedding :64-98, generate_embeddings_batch :154-224, get_embedding_dimension
:312-332, cache statistics :248-310) with the OpenAI HTTP calls (:100-115, :226-246) replaced by a BERT sentence encoder run by
the HIP engine (rag_embed_load_host / rag_embed_host: the cross-encoder's kernels behind a mean- or [CLS]-pooling + L2-normalise
head, i.e. a sentence-transformers `Transformer -> Pooling(mean | cls) -> Normalize` checkpoint such as all-MiniLM-L6-v2 or a
BERT-base-shaped encoder).

NOT a parity replacement: a local encoder returns different vectors (and a different dimension: the encoder's hidden size, 384
for the MiniLM shape, 768 for BERT-base, 1024 for BERT-large) than text-embedding-3-small. An index has to be built and queried with the same service; what the tests pin is this forward against
`transformers.BertModel`. There is no CPU fallback.
"""
import json
import os
import threading
from collections import OrderedDict

import numpy as np

from .cross_encoder import flatten_state_dict, load_m3_heads, load_tokenizer, map_checkpoint, seq_limit
from .engine import get_engine


# pooling_mode_* keys of sentence-transformers' 1_Pooling/config.json -> what they are called in an error message
_POOLING_KEYS = {"pooling_mode_cls_token": "cls", "pooling_mode_mean_tokens": "mean", "pooling_mode_max_tokens": "max",
                 "pooling_mode_mean_sqrt_len_tokens": "mean_sqrt_len", "pooling_mode_weightedmean_tokens": "weightedmean",
                 "pooling_mode_lasttoken": "lasttoken"}


def pooling_mode_of_dir(path):
    """"mean" or "cls" for a checkpoint directory: what its 1_Pooling/config.json switches on ("mean" when the file is missing).
    Any other mode, or several at once (their vectors are concatenated), is a ValueError that names it: the engine has no such
    head, and pooling such a checkpoint by the mean would silently return other vectors than the model was trained to give."""
    cfg_path = os.path.join(path, "1_Pooling", "config.json")
    if not os.path.exists(cfg_path):
        return "mean"
    with open(cfg_path) as f:
        pc = json.load(f)
    on = [name for key, name in _POOLING_KEYS.items() if pc.get(key)]
    on += [k for k, v in pc.items() if k.startswith("pooling_mode_") and k not in _POOLING_KEYS and v is True]
    if on == ["mean"] or on == ["cls"]:
        return on[0]
    raise ValueError(f"unsupported pooling mode {'+'.join(on) or 'none'} in {cfg_path}: only mean and cls are supported")


class LocalEmbeddingService:
    def __init__(self, cfg, tensors, tokenizer, max_length=256, engine=None, batch_size=2048, normalize=True, model="local-bert-mean-pool",
                 cache_size=1000, pooling="mean"):
        self.cfg = cfg
        self.model = model
        self.dimensions = int(cfg["hidden"])
        self.engine = engine or get_engine(dim=self.dimensions)
        self.tokenizer = tokenizer
        self.max_length = min(int(max_length), seq_limit(cfg))
        self.batch_size = int(batch_size)
        self.pooling = pooling
        self.engine.embed_load(cfg, tensors, normalize=normalize, pooling=pooling)
        # LRU cache of `cache_size` texts (the reference: cachetools.LRUCache(maxsize=EMBEDDING_CACHE_SIZE), default 1000 -
        # memory/embeddings.py:50, config.py:77): ingesting a large corpus must not keep every text in host memory
        self._cache, self._cache_lock = OrderedDict(), threading.Lock()
        self._cache_max = max(1, int(cache_size))
        self._cache_hits = self._cache_misses = 0

    def _cache_get(self, text):                      # caller holds the lock
        hit = self._cache.get(text)
        if hit is not None:
            self._cache.move_to_end(text)
        return hit

    def _cache_put(self, text, emb):                 # caller holds the lock
        self._cache[text] = emb
        self._cache.move_to_end(text)
        while len(self._cache) > self._cache_max:
            self._cache.popitem(last=False)

    @classmethod
    def from_dir(cls, path, max_length=256, engine=None, **kw):
        """A local sentence-transformers / HF BertModel, RobertaModel or XLMRobertaModel directory: config.json, model.safetensors,
        tokenizer.json or vocab.txt (cross_encoder.map_checkpoint / load_tokenizer). The pooling mode is
        the one sentence-transformers recorded in 1_Pooling/config.json (mean or [CLS]; mean without the file); `normalize` stays
        the caller's argument."""
        from safetensors.numpy import load_file
        with open(os.path.join(path, "config.json")) as f:
            cfg, sd = map_checkpoint(json.load(f), load_file(os.path.join(path, "model.safetensors")), head=False)
        svc = cls(cfg, flatten_state_dict(sd, cfg["layers"], head=False), load_tokenizer(path), max_length=max_length, engine=engine,
                  model=os.path.basename(os.path.normpath(path)), pooling=pooling_mode_of_dir(path), **kw)
        # bge-m3's other two heads (and a ColBERT checkpoint's projection), when their files lie beside the encoder
        heads = load_m3_heads(path, hidden=cfg["hidden"])
        if heads["tok_w"] is not None or heads["lex_w"] is not None:
            svc.load_heads(heads)
        return svc

    # ---- token-vector and lexical heads: the surface of FlagEmbedding's BGEM3FlagModel (encode / compute_score), restated ----
    has_token_head = has_lexical_head = False

    def load_heads(self, heads):
        """heads: what cross_encoder.load_m3_heads returns (tok_w / tok_b / lex_w / lex_b, None where a head is absent)."""
        self.engine.embed_heads_load(tok_w=heads.get("tok_w"), tok_b=heads.get("tok_b"), lex_w=heads.get("lex_w"), lex_b=heads.get("lex_b", 0.0))
        self.has_token_head = self.has_token_head or heads.get("tok_w") is not None
        self.has_lexical_head = self.has_lexical_head or heads.get("lex_w") is not None

    def special_ids(self):
        """The token ids a lexical-weight map leaves out: the tokenizer's cls / eos / pad / unk, whichever it has (at most 8)."""
        tid = getattr(self.tokenizer, "token_to_id", lambda t: None)
        ids = {int(self.cfg[k]) for k in ("cls_id", "sep_id") if k in self.cfg}
        ids |= {tid(t) for t in ("<s>", "</s>", "<pad>", "<unk>", "[CLS]", "[SEP]", "[PAD]", "[UNK]")} - {None}
        return sorted(ids)[:8]

    def _need_heads(self, lexical, tokens):
        if (lexical and not self.has_lexical_head) or (tokens and not self.has_token_head):
            raise ValueError(f"{self.model}: the {'lexical' if lexical and not self.has_lexical_head else 'token-vector'} head is not loaded "
                             "(sparse_linear.pt / colbert_linear.pt beside the checkpoint)")

    def encode_multi(self, texts, return_dense=True, return_sparse=True, return_colbert_vecs=True):
        """One forward per text, upstream's keys: dense_vecs [n, hidden], lexical_weights (a list of {token_id: weight}: the largest
        weight > 0 of each id, special tokens left out) and colbert_vecs (a list of [len - 1, tok_dim] arrays); a key that was not
        asked for is None."""
        self._need_heads(return_sparse, return_colbert_vecs)
        texts = [str(t) for t in texts]
        dense, lexw, vecs = [], [], []
        skip = set(self.special_ids())
        for b in range(0, len(texts), self.batch_size):
            ids, tt, lens = self.tokenize(texts[b:b + self.batch_size])
            d, lx, tk, off = self.engine.embed_multi(ids, tt, lens, dense=return_dense, lexical=return_sparse, tokens=return_colbert_vecs)
            if return_dense:
                dense.append(d)
            for i in range(len(lens)):
                if return_sparse:
                    m = {}
                    for t in range(int(lens[i])):
                        k, w = int(ids[i, t]), float(lx[i, t])
                        if k not in skip and w > 0 and w > m.get(k, 0.0):
                            m[k] = w
                    lexw.append(m)
                if return_colbert_vecs:
                    vecs.append(tk[int(off[i]):int(off[i + 1])].copy())
        return {"dense_vecs": np.concatenate(dense) if return_dense and dense else None,
                "lexical_weights": lexw if return_sparse else None, "colbert_vecs": vecs if return_colbert_vecs else None}

    def compute_score(self, pairs, weights=(0.4, 0.2, 0.4)):
        """[(query, passage), ...] -> upstream's five lists: dense, sparse, colbert, sparse+dense and colbert+sparse+dense, the last
        two weighted means by weights = (dense, sparse, colbert) over the weights in use. Every distinct text goes through ONE
        embed_multi call; MaxSim and the lexical match run on the device (rag_maxsim_*, rag_lexical_match_*), the dense score is the
        existing pairwise cosine."""
        self._need_heads(True, True)
        pairs = [(str(q), str(d)) for q, d in pairs]
        if not pairs:
            return {k: [] for k in ("colbert", "sparse", "dense", "sparse+dense", "colbert+sparse+dense")}
        index = {}
        for q, d in pairs:
            index.setdefault(q, len(index))
            index.setdefault(d, len(index))
        pq = np.asarray([index[q] for q, _ in pairs], dtype=np.int32)
        pd = np.asarray([index[d] for _, d in pairs], dtype=np.int32)
        ids, tt, lens = self.tokenize(list(index))
        dense, lx, tk, off = self.engine.embed_multi(ids, tt, lens)
        colbert = self.engine.maxsim(tk, off, tk, off, pq, pd).astype(np.float64)
        sparse = self.engine.lexical_match(ids, lx, lens, ids, lx, lens, pq, pd, skip_ids=self.special_ids()).astype(np.float64)
        dn = np.empty(len(pairs), dtype=np.float64)
        for b in range(0, len(pairs), 256):                   # the cosine call gives a matrix: its diagonal, block by block
            e = min(len(pairs), b + 256)
            dn[b:e] = np.diagonal(self.engine.pairwise_cosine(dense[pq[b:e]], dense[pd[b:e]]))
        w0, w1, w2 = (float(w) for w in weights)
        return {"colbert": colbert.tolist(), "sparse": sparse.tolist(), "dense": dn.tolist(),
                "sparse+dense": ((w1 * sparse + w0 * dn) / (w0 + w1)).tolist(),
                "colbert+sparse+dense": ((w2 * colbert + w1 * sparse + w0 * dn) / (w0 + w1 + w2)).tolist()}

    # ---- tokenisation: [CLS] text [SEP], truncated to max_length, padded to the longest of the batch -----------------
    def tokenize(self, texts):
        self.tokenizer.enable_truncation(max_length=self.max_length)
        self.tokenizer.no_padding()
        enc = self.tokenizer.encode_batch([str(t) for t in texts])
        L = max(len(e.ids) for e in enc)
        ids = np.zeros((len(enc), L), dtype=np.int32)
        lens = np.zeros((len(enc),), dtype=np.int32)
        for i, e in enumerate(enc):
            ids[i, :len(e.ids)] = e.ids
            lens[i] = len(e.ids)
        return ids, np.zeros_like(ids), lens

    def _embed_uncached(self, texts):
        out = np.empty((len(texts), self.dimensions), dtype=np.float32)
        for b in range(0, len(texts), self.batch_size):
            ids, tt, lens = self.tokenize(texts[b:b + self.batch_size])
            out[b:b + len(lens)] = self.engine.embed(ids, tt, lens)
        return out

    # ---- the reference's surface ------------------------------------------------------------------------------------
    def generate_embedding(self, text, use_cache=True):
        if not text or not text.strip():
            raise ValueError("Text cannot be empty")                              # memory/embeddings.py:75-76
        if use_cache:
            with self._cache_lock:
                hit = self._cache_get(text)
                if hit is not None:
                    self._cache_hits += 1
                    return list(hit)
                self._cache_misses += 1
        emb = [float(x) for x in self._embed_uncached([text])[0]]
        if use_cache:
            with self._cache_lock:
                self._cache_put(text, tuple(emb))
        return emb

    def generate_embeddings_batch(self, texts, use_cache=True):
        """List[str] -> List[List[float]] in input order; cached texts are not recomputed; an empty or whitespace-only text gets [] in
        its slot and touches neither the cache nor its counters (memory/embeddings.py:154-224, :164-168)."""
        if not texts:
            return []
        out, todo = [[] for _ in texts], []
        for i, t in enumerate(texts):
            if not t or not t.strip():
                continue
            hit = None
            if use_cache:
                with self._cache_lock:
                    hit = self._cache_get(t)
                    if hit is not None:
                        self._cache_hits += 1
                    else:
                        self._cache_misses += 1
            if hit is not None:
                out[i] = list(hit)
            else:
                todo.append(i)
        if todo:
            vecs = self._embed_uncached([texts[i] for i in todo])
            for i, v in zip(todo, vecs):
                out[i] = [float(x) for x in v]
                if use_cache:
                    with self._cache_lock:
                        self._cache_put(texts[i], tuple(out[i]))
        return out

    def get_embedding_dimension(self):
        return self.dimensions

    def get_cache_stats(self):
        with self._cache_lock:
            total = self._cache_hits + self._cache_misses
            rate = self._cache_hits / total if total else 0.0
            return {"hits": self._cache_hits, "misses": self._cache_misses, "hit_rate": rate, "hit_rate_percent": f"{rate * 100:.1f}%",
                    "current_size": len(self._cache), "max_size": self._cache_max, "cache_full": len(self._cache) >= self._cache_max}

    def clear_cache(self):
        with self._cache_lock:
            self._cache.clear()
            self._cache_hits = self._cache_misses = 0
