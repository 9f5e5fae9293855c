"""Float64 reference for the embedder's token-vector and lexical heads and their pair scores, shared by tests/test_m3_heads_cpu.py
and tests/test_m3_heads_gpu.py. Built on oracle.bert_oracle.forward_hidden; the semantics are restated from FlagEmbedding's
BGEM3FlagModel (dense / sparse / colbert heads, colbert_score, compute_lexical_matching_score, compute_score), which is not
installed here: parity with upstream is not pinned, only this restatement against an independent torch one (the CPU test)."""
import numpy as np

from oracle import bert_oracle as B

WEIGHTS = (0.4, 0.2, 0.4)                        # upstream's default (dense, sparse, colbert)
SCORE_KEYS = ("colbert", "sparse", "dense", "sparse+dense", "colbert+sparse+dense")


def seeded_heads(hidden, tok_dim, seed, bias=True):
    """Seeded float32 heads: tok_w [tok_dim, hidden] at the scale of the encoder's matrices, lex_w [hidden] with an l1 norm of 1 (so
    lexical weights stay O(1) and the bar 2e-3 * |lex_w|_1 is 2e-3), biases that leave about half of the lexical weights at zero."""
    rng = np.random.default_rng(seed)
    tok_w = (rng.standard_normal((tok_dim, hidden)) * 0.05).astype(np.float32)
    tok_b = (rng.standard_normal(tok_dim) * 0.05).astype(np.float32) if bias else None
    lex_w = rng.standard_normal(hidden)
    lex_w = (lex_w / np.abs(lex_w).sum()).astype(np.float32)
    lex_b = float(np.float32(0.01)) if bias else 0.0
    return dict(tok_w=tok_w, tok_b=tok_b, lex_w=lex_w, lex_b=lex_b)


def normalize(x):
    """torch.nn.functional.normalize over the last axis: x / max(|x|, 1e-12)"""
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-12)


def heads_reference(w, cfg, ids, tt, lens, heads):
    """dict(dense [P, H] = normalize(x[:, 0]); lex [P, L] = relu(lex_w . x[t] + lex_b) for t < len, 0 behind; vecs = a list of
    [len - 1, tok_dim] arrays normalize(tok_w . x[t] + tok_b), t = 1 ... len - 1), all float64. lens are clamped to [1, L]."""
    ids = np.asarray(ids, dtype=np.int64)
    P, L = ids.shape
    lens = np.clip(np.asarray(lens, dtype=np.int64), 1, L)
    _, x = B.forward_hidden(w, cfg, ids, np.asarray(tt, dtype=np.int64), lens, fast_erf=True)
    out = dict(dense=normalize(x[:, 0]), hidden=x)
    if heads.get("lex_w") is not None:
        lw = np.maximum(x @ heads["lex_w"].astype(np.float64) + float(heads["lex_b"]), 0.0)
        lw[np.arange(L)[None, :] >= lens[:, None]] = 0.0
        out["lex"] = lw
    if heads.get("tok_w") is not None:
        tw = heads["tok_w"].astype(np.float64)
        tb = 0.0 if heads.get("tok_b") is None else heads["tok_b"].astype(np.float64)
        out["vecs"] = [normalize(x[p, 1:lens[p]] @ tw.T + tb) for p in range(P)]
    return out


def lexical_map(ids_row, w_row, n, skip):
    """{token id: largest weight > 0 over the positions < n holding it}, the ids in `skip` left out"""
    m = {}
    for t in range(int(n)):
        k, v = int(ids_row[t]), float(w_row[t])
        if k in skip or not v > 0:
            continue
        if v > m.get(k, 0.0):
            m[k] = v
    return m


def lexical_score(mq, md):
    return float(sum(v * md[k] for k, v in mq.items() if k in md))


def maxsim(vq, vd):
    """(1 / nq) * sum_i max_j <vq[i], vd[j]> over the texts' own rows; 0 when either side has none"""
    vq, vd = np.asarray(vq, dtype=np.float64), np.asarray(vd, dtype=np.float64)
    if vq.shape[0] == 0 or vd.shape[0] == 0:
        return 0.0
    return float((vq @ vd.T).max(axis=1).sum() / vq.shape[0])


def combine(dense, sparse, colbert, weights=WEIGHTS):
    w0, w1, w2 = (float(x) for x in weights)
    dense, sparse, colbert = (np.asarray(a, dtype=np.float64) for a in (dense, sparse, colbert))
    return {"colbert": colbert, "sparse": sparse, "dense": dense, "sparse+dense": (w1 * sparse + w0 * dense) / (w0 + w1),
            "colbert+sparse+dense": (w2 * colbert + w1 * sparse + w0 * dense) / (w0 + w1 + w2)}


def score_pairs(ref, ids, lens, pair_q, pair_d, skip, weights=WEIGHTS):
    """compute_score over a heads_reference result: the five score arrays for the pairs (pair_q[i], pair_d[i]) of its texts"""
    skip = set(int(s) for s in skip)
    lens = np.clip(np.asarray(lens, dtype=np.int64), 1, np.asarray(ids).shape[1])
    maps = [lexical_map(ids[p], ref["lex"][p], lens[p], skip) for p in range(len(lens))]
    dense = [float(ref["dense"][q] @ ref["dense"][d]) for q, d in zip(pair_q, pair_d)]
    sparse = [lexical_score(maps[q], maps[d]) for q, d in zip(pair_q, pair_d)]
    colbert = [maxsim(ref["vecs"][q], ref["vecs"][d]) for q, d in zip(pair_q, pair_d)]
    return combine(dense, sparse, colbert, weights)


def pack(vecs, dim, dtype=np.float32):
    """a list of [n_i, dim] arrays -> (packed [sum n_i, dim], int64 offsets [len + 1])"""
    off = np.zeros(len(vecs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([v.shape[0] for v in vecs])
    out = np.zeros((int(off[-1]), dim), dtype=dtype)
    for i, v in enumerate(vecs):
        out[off[i]:off[i + 1]] = v
    return out, off


def write_head_files(d, heads):
    """colbert_linear.pt / sparse_linear.pt as bge-m3 ships them: torch state dicts holding `weight` and maybe `bias`"""
    import torch
    if heads.get("tok_w") is not None:
        sd = {"weight": torch.from_numpy(heads["tok_w"].copy())}
        if heads.get("tok_b") is not None:
            sd["bias"] = torch.from_numpy(heads["tok_b"].copy())
        torch.save(sd, str(d / "colbert_linear.pt"))
    if heads.get("lex_w") is not None:
        torch.save({"weight": torch.from_numpy(heads["lex_w"].reshape(1, -1).copy()),
                    "bias": torch.tensor([heads["lex_b"]], dtype=torch.float32)}, str(d / "sparse_linear.pt"))
