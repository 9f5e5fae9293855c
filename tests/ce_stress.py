"""Stress weights for the cross-encoder tests (a helper module, not a conftest): deterministic transforms of
oracle/bert_oracle.seeded_weights towards what trained BERT-family checkpoints look like.

Seeded weights are i.i.d. Gaussian at one mild scale: layer-0 attention logits have a standard deviation of about 2.5 per row and
no feature is an outlier. MiniLM is distilled from BERT's attention distributions, so many of its heads are sharp, and its
LayerNorms have a few outlier dimensions. Every transform returns a new state dict and checks its own target on a fixed batch in
numpy (`stats`), so that a later edit cannot quietly make the stress mild again; tests/test_ce_stress_targets.py pins the targets
of the levels tests/test_cross_encoder_stress_gpu.py runs."""
import math

import numpy as np

from oracle import bert_oracle as B

OUTLIER_DIMS = (7, 100, 222, 333)


def probe_batch(cfg, pairs=4, L=64, seed=0):
    """A fixed batch of full-length pairs: token ids above the special / unused ids when the vocabulary has them, type 1 from
    position 18."""
    rng = np.random.default_rng(seed)
    lo = 1000 if cfg["vocab_size"] > 2000 else 5
    L = min(L, cfg["max_pos"])
    ids = rng.integers(lo, cfg["vocab_size"], (pairs, L)).astype(np.int64)
    tt = np.zeros((pairs, L), dtype=np.int64)
    tt[:, 18:] = 1
    return ids, tt, np.full(pairs, L, dtype=np.int64)


def stats(w, cfg, dims=OUTLIER_DIMS):
    """On probe_batch, float64:
    attn_std  layer-0 attention logits (q.k / sqrt(d_head)): standard deviation over the keys of a row, mean over rows
    outlier   mean |embedding-LayerNorm output| on `dims` / the same on the other dims
    gelu_tail fraction of layer-0 FFN-up pre-activations (the GELU inputs) with |x| > 5"""
    ids, tt, _ = probe_batch(cfg)
    W = {k: v.astype(np.float64) for k, v in w.items()}
    P, L = ids.shape
    H, nh = cfg["hidden"], cfg["heads"]
    dh = H // nh
    x = (W["bert.embeddings.word_embeddings.weight"][ids] + W["bert.embeddings.token_type_embeddings.weight"][tt]
         + W["bert.embeddings.position_embeddings.weight"][np.arange(L)][None])
    x = B._ln(x, W["bert.embeddings.LayerNorm.weight"], W["bert.embeddings.LayerNorm.bias"], cfg["eps"])
    mask = np.zeros(H, dtype=bool)
    mask[list(dims)] = True
    outlier = np.abs(x[..., mask]).mean() / np.abs(x[..., ~mask]).mean()
    p = "bert.encoder.layer.0."
    sp = lambda t: t.reshape(P, L, nh, dh).transpose(0, 2, 1, 3)
    q = sp(x @ W[p + "attention.self.query.weight"].T + W[p + "attention.self.query.bias"])
    k = sp(x @ W[p + "attention.self.key.weight"].T + W[p + "attention.self.key.bias"])
    s = q @ k.transpose(0, 1, 3, 2) / math.sqrt(dh)
    attn_std = float(s.std(-1).mean())
    # the GELU inputs of layer 0, after the attention block (the oracle's own layer, without its FFN)
    a = np.exp(s - s.max(-1, keepdims=True))
    a /= a.sum(-1, keepdims=True)
    v = sp(x @ W[p + "attention.self.value.weight"].T + W[p + "attention.self.value.bias"])
    ctx = (a @ v).transpose(0, 2, 1, 3).reshape(P, L, H)
    o = ctx @ W[p + "attention.output.dense.weight"].T + W[p + "attention.output.dense.bias"]
    x = B._ln(o + x, W[p + "attention.output.LayerNorm.weight"], W[p + "attention.output.LayerNorm.bias"], cfg["eps"])
    hpre = x @ W[p + "intermediate.dense.weight"].T + W[p + "intermediate.dense.bias"]
    return dict(attn_std=attn_std, outlier=float(outlier), gelu_tail=float((np.abs(hpre) > 5).mean()))


def _layers(cfg):
    return [f"bert.encoder.layer.{l}." for l in range(cfg["layers"])]


def sharp(w, cfg, f):
    """Query and key weights of every layer times f: attention logits times ~f^2 (sharp heads)."""
    out = dict(w)
    for p in _layers(cfg):
        for nm in ("query", "key"):
            out[p + f"attention.self.{nm}.weight"] = (w[p + f"attention.self.{nm}.weight"] * np.float32(f)).astype(np.float32)
    before, after = stats(w, cfg)["attn_std"], stats(out, cfg)["attn_std"]
    assert after >= 0.9 * f * f * before, (before, after)
    return out


def outliers(w, cfg, g, b=0.0, dims=OUTLIER_DIMS):
    """LayerNorm gamma times g and beta + b on `dims`, in every LayerNorm including the embedding one: a few hidden features
    ~g times larger than the rest through the whole residual stream."""
    out = dict(w)
    names = ["bert.embeddings.LayerNorm."] + [p + s for p in _layers(cfg) for s in ("attention.output.LayerNorm.", "output.LayerNorm.")]
    idx = list(dims)
    for n in names:
        gam, bet = w[n + "weight"].copy(), w[n + "bias"].copy()
        gam[idx] *= np.float32(g)
        bet[idx] += np.float32(b)
        out[n + "weight"], out[n + "bias"] = gam, bet
    r = stats(out, cfg, dims)["outlier"]
    assert r >= 0.7 * g, r
    return out


def ffn_tails(w, cfg, f):
    """FFN-up (intermediate) weights of every layer times f: the GELU sees inputs well past |x| = 5."""
    out = dict(w)
    for p in _layers(cfg):
        out[p + "intermediate.dense.weight"] = (w[p + "intermediate.dense.weight"] * np.float32(f)).astype(np.float32)
    tail = stats(out, cfg)["gelu_tail"]
    assert tail >= 0.01, tail
    return out


def centre_logits(w, cfg):
    """Classifier bias set so that the oracle's logits on probe_batch (at two lengths) have mean 0: the sigmoid is steepest there,
    so the 1e-3 score bar is tightest."""
    ids, tt, lens = probe_batch(cfg, pairs=8)
    lens = lens.copy()
    lens[::2] = lens[::2] // 2
    out = dict(w)
    out["classifier.bias"] = np.zeros(1, dtype=np.float32)
    z = B.forward_logits(out, cfg, ids, tt, lens, fast_erf=True)
    out["classifier.bias"] = np.array([-z.mean()], dtype=np.float32)
    assert abs(B.forward_logits(out, cfg, ids, tt, lens, fast_erf=True).mean()) < 1e-3
    return out


# ---- the stress levels of the MiniLM shape and their batch, shared by tests/test_cross_encoder_stress_gpu.py (classifier),
# tests/test_embeddings_stress_gpu.py (embedding head) and tests/test_ce_stress_targets.py (CPU preconditions)
CFG = B.minilm_config()
LEVELS = {
    "seeded": lambda w: w,
    "moderate": lambda w: outliers(sharp(w, CFG, 1.5), CFG, 8),
    "sharp": lambda w: sharp(w, CFG, 2),
    "outlier": lambda w: outliers(w, CFG, 12, 3),
    "combined": lambda w: ffn_tails(outliers(sharp(w, CFG, 1.5), CFG, 8), CFG, 3),
}
L = 128
LENS = np.array([128, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 95, 96, 97, 111, 112, 113, 127, 128], dtype=np.int32)


def batch(lens=LENS, L=L, seed=2468, pair_types=True):
    """Token ids above the special / unused ids, pad id 0 past each length; type 1 from position 18 (a pair) or type 0 throughout
    (a single text, what an embedding model sees)."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int32)
    ids = rng.integers(1000, CFG["vocab_size"], (len(lens), L)).astype(np.int32)
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    tt = ((np.arange(L)[None, :] >= 18) & (np.arange(L)[None, :] < lens[:, None])).astype(np.int32)
    return ids, tt if pair_types else np.zeros_like(tt)


# ---- the error-budget tests (tests/test_ce_error_budget.py on the CPU simulator, tests/test_cross_encoder_budget_gpu.py on the GPU):
# the seeded model with centred logits, pair token types on BOTH heads so that one encoder pass of the oracle serves both
# what the CPU test asserts of a forward that lost a correction product (rms error / shipped rms error), and the margins the GPU
# test gives each forward over its measured error: a margin must stay under its ratio
SPLIT16_MUTANT_RATIO, MX_MUTANT_RATIO = 20.0, 2.0
SPLIT16_MARGIN, MX_MARGIN = 2.0, 1.5
# the non-384 shape of the budget tests: split fp16 only, the unfused LayerNorm and the GEMM instantiations MiniLM does not take
H128 = dict(vocab_size=2000, hidden=128, layers=2, heads=4, ffn=512, max_pos=128, type_vocab=2, eps=1e-12)


def budget_weights(cfg=CFG, seed=99):
    return centre_logits(B.seeded_weights(cfg, seed), cfg)


def budget_batch(reps=1, cfg=None):
    """(ids, tt, lens) of reps x 24 pairs at L = 128: batch(seed=2468 + i) for i < reps, LENS tiled. 24 pairs pack into 1760 rows of
    16-row-aligned pairs, so reps = 4 gives 7040 rows: exactly 55 token tiles of 128 rows and 27.5 of 256. cfg: a smaller model's
    shape - the token ids are folded into its vocabulary."""
    parts = [batch(seed=2468 + i) for i in range(reps)]
    ids, tt = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    if cfg is not None and cfg["vocab_size"] < CFG["vocab_size"]:
        ids = np.where(ids > 0, 5 + ids % (cfg["vocab_size"] - 5), 0).astype(np.int32)
    return ids, tt, np.tile(LENS, reps)


def heads(W, x, lens):
    """(classifier logits [P], raw mean-pooled vectors [P, H]) of one last hidden state, float64: the two small heads of
    oracle/bert_oracle.py (forward_logits, sentence_embeddings with normalize=False) behind one encoder pass"""
    pooled = np.tanh(x[:, 0] @ W["bert.pooler.dense.weight"].T + W["bert.pooler.dense.bias"])
    logits = (pooled @ W["classifier.weight"].T + W["classifier.bias"])[:, 0]
    ok = (np.arange(x.shape[1])[None, :] < np.asarray(lens)[:, None]).astype(np.float64)[:, :, None]
    return logits, (x * ok).sum(1) / np.maximum(ok.sum(1), 1e-9)


def oracle_heads(w, cfg, ids, tt, lens):
    W, x = B.forward_hidden(w, cfg, ids.astype(np.int64), tt.astype(np.int64), lens, fast_erf=True)
    return heads(W, x, lens)


def budget_errors(logits, raw, exp_logits, exp_raw):
    """The four figures a budget holds: max and rms over all pairs of |logit - oracle|, max and rms over all components of
    |raw pooled - oracle| / ||oracle||."""
    dl = np.abs(np.asarray(logits, dtype=np.float64) - exp_logits)
    dr = np.abs(np.asarray(raw, dtype=np.float64) - exp_raw) / np.linalg.norm(exp_raw, axis=1, keepdims=True)
    return dict(logit_max=float(dl.max()), logit_rms=float(np.sqrt((dl ** 2).mean())),
                raw_max=float(dr.max()), raw_rms=float(np.sqrt((dr ** 2).mean())))
