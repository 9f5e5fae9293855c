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

from .cross_encoder import flatten_state_dict, load_tokenizer, map_checkpoint, seq_limit
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
        return cls(cfg, flatten_state_dict(sd, cfg["layers"], head=False), load_tokenizer(path), max_length=max_length, engine=engine,
                   model=os.path.basename(os.path.normpath(path)), pooling=pooling_mode_of_dir(path), **kw)

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
