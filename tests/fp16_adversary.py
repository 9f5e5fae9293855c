"""Worst-case inputs for the dense search's fp16 pass, and a numpy emulation of that pass (no GPU needed).

The exactness proof above select_kernel (csrc/dense.hip) rests on |S~ - S| <= eps for the fp16 MFMA score S~ of a row whose
float64 cosine is S. On Gaussian data the fp16 rounding errors of the products cancel and |S~ - S| is ~1e-5, a hundredth of
eps, so a wrong eps or a wrong threshold goes unnoticed. The rows built here make every product's error point the same way.

fp16 rounding has relative error up to 2^-11, reached just above a power of two: 2^e * (1 + 2^-11 + d) rounds UP to
2^e * (1 + 2^-10), 2^e * (1 + 2^-11 - d) rounds DOWN to 2^e. The query's components, at the kernel's norm of 128, sit at such
midpoints: set A rounds up, set B rounds down; fillers bring the norm to exactly 128 so that the normalisation leaves the
others where they are. Corpus rows carry the same magnitudes (hence the same norm and the same roundings) with chosen signs:
  plus row   + on A, - on B: every midpoint product errs upwards   (S~ - S ~ +2^-10 * (1 - S))
  minus row  - on A, + on B: every midpoint product errs downwards (S~ - S ~ -2^-10 * (1 - S))
The big fillers are positive in both kinds, so both have the same cosine `cosine`; one small component (negative in plus rows,
positive in minus rows) lifts the minus rows' exact cosine a hair above every plus row's. A minus row therefore BELONGS in the
exact top-k while its fp16 score sits ~2^-9 * (1 - S) below the plus rows'.
"""
import numpy as np

SCALE = 128.0                      # 2^RAG_SCALE_LOG2: rows are scaled to this norm before the cast to fp16
U16 = 2.0 ** -11                   # fp16 unit roundoff
OFF = 2.0 ** -16                   # distance of a midpoint component from the fp16 rounding boundary (relative)
TINY = (0.11, 0.07)                # low-mass fillers whose sign differs between plus rows: distinct near-ties (~1e-6 apart)
LIFT = 2e-5                        # exact cosine of a minus row minus the best plus row's


def pad_dim(dim):
    return (dim + 127) // 128 * 128


def analytic_bound(dim):
    """|S~ - S| of unit vectors from the number formats alone: two fp16 roundings per product (2^-10 + 2^-22 in all, times
    sum |q_i c_i| <= 1) plus the float32 accumulation of dim_pad terms and the float32 normalisation (2 * dim_pad * 2^-24)."""
    return 2.0 ** -10 + 2.0 * pad_dim(dim) * 2.0 ** -24


def emulate_rows(x):
    """normalize_rows_kernel in numpy: float64 sum of squares of the float32 row, scale = 128 / sqrt(sum) (formed and applied
    the way the kernel does: see _scaled), cast to fp16 (round to nearest even); a zero or non-finite norm gives a zero row."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    acc = np.sum(x.astype(np.float64) ** 2, axis=1)
    ok = (acc > 0.0) & (acc < 1e300)
    with np.errstate(all="ignore"):
        y = _scaled(x, np.where(ok, acc, 1.0))
    y[~ok] = 0.0
    return y.astype(np.float16)


def _scaled(x, acc):
    # the product is formed in float64 and rounded to float32 once (a float32 scale would overflow for rows of denormals)
    return (x.astype(np.float64) * (SCALE / np.sqrt(acc))[:, None]).astype(np.float32)


def emulate_scores(q16, c16):
    """[Q, D] x [N, D] fp16 rows -> [Q, N] scores: the fp16 products summed in float64, divided by 2^14. The MFMA sums the same
    products in float32 in an order of its own: at most 2 * dim_pad * 2^-24 away."""
    return np.asarray(q16, dtype=np.float64) @ np.asarray(c16, dtype=np.float64).T / (SCALE * SCALE)


def exact_scores(q, c):
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    c = np.atleast_2d(np.asarray(c, dtype=np.float64))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)) @ (c / np.linalg.norm(c, axis=1, keepdims=True)).T


def _magnitudes(dim, cosine):
    """Component magnitudes of a family at norm 128: midpoint components (in one or two neighbouring binades, so that any dim
    reaches the wanted mass), big fillers, the small lifting component and the tiny per-row fillers. Returns (mag, kind) with
    kind 0 = set A, 1 = set B, 2 = big filler, 3 = small, 4 + j = tiny filler j."""
    total = SCALE * SCALE
    n_big = max(2, dim // 16)
    n_mid = (dim - n_big - 1 - len(TINY)) // 4 * 4          # a multiple of 4: each binade splits evenly into A and B
    want = (1.0 - cosine) * total
    e = int(np.floor(np.log2(want / n_mid) / 2.0))          # n_mid * 4^e <= want < n_mid * 4^(e+1)
    n_hi = int((want - n_mid * 4.0 ** e) // (3.0 * 4.0 ** e)) // 2 * 2
    base = np.concatenate([np.full(n_hi, 2.0 ** (e + 1)), np.full(n_mid - n_hi, 2.0 ** e)])
    kind = np.concatenate([np.arange(n_hi) % 2, np.arange(n_mid - n_hi) % 2])
    mid = base * (1.0 + U16 + np.where(kind == 0, OFF, -OFF))
    m_a, m_b = np.sum(mid[kind == 0] ** 2), np.sum(mid[kind == 1] ** 2)
    # plus: (+A - B + big - small - tiny...) / total; minus: (-A + B + big + small + tiny...) / total. The small component
    # cancels the A/B imbalance and adds LIFT on top.
    small = np.sqrt((LIFT * total + 2.0 * (m_a - m_b)) / 2.0)
    tiny = np.asarray(TINY)
    rest = total - m_a - m_b - small ** 2 - np.sum(tiny ** 2)
    assert rest > 0, (dim, cosine)
    big = np.full(n_big, np.sqrt(rest / n_big))
    n_zero = dim - n_mid - n_big - 1 - len(TINY)
    mag = np.concatenate([mid, big, [small], tiny, np.zeros(n_zero)])
    kinds = np.concatenate([kind, np.full(n_big, 2), [3], 4 + np.arange(len(TINY)), np.full(n_zero, 2)])
    return mag, kinds.astype(np.int64)


def build(dim, k, n_minus, cosine, scale=1.0, rng=None, n_plus=None):
    """One adversarial family. Returns a dict:
      q [dim], plus [n_plus, dim], minus [n_minus, dim]   float32 (n_plus defaults to k)
      S_plus, St_plus, S_minus, St_minus                  float64 cosine S and emulated fp16-pass score S~ of every row
    `scale` (a power of two) multiplies every vector; `rng` places the components and picks the query's signs, so that families
    built from different draws are (nearly) orthogonal: one query's rows are background for another's. Plus row r flips the
    tiny fillers by the bits of r % 4: rows 0, 4, 8, ... are identical (exact ties), rows 0..3 differ by ~1e-6 (near-ties)."""
    assert dim % 4 == 0 and dim >= 32 and 0 < n_minus
    n_plus = k if n_plus is None else n_plus
    mag, kind = _magnitudes(dim, cosine)
    sign_q = np.ones(dim)
    if rng is not None:
        perm = rng.permutation(dim)
        mag, kind = mag[perm], kind[perm]
        sign_q = rng.choice([-1.0, 1.0], dim)
    sp = np.select([kind == 0, kind == 1, kind == 3], [1.0, -1.0, -1.0], 1.0)
    sm = np.select([kind == 0, kind == 1], [-1.0, 1.0], 1.0)
    plus = np.tile(mag * sp * sign_q, (n_plus, 1))
    for j in range(len(TINY)):
        flip = (np.arange(n_plus) >> j) & 1
        plus[:, kind == 4 + j] *= np.where(flip, -1.0, 1.0)[:, None]
    minus = np.tile(mag * sm * sign_q, (n_minus, 1))
    out = dict(q=(mag * sign_q * scale).astype(np.float32), plus=(plus * scale).astype(np.float32),
               minus=(minus * scale).astype(np.float32))
    q16 = emulate_rows(out["q"])
    for name in ("plus", "minus"):
        out["S_" + name] = exact_scores(out["q"], out[name])[0]
        out["St_" + name] = emulate_scores(q16, emulate_rows(out[name]))[0]
    return out


def background(rng, n, queries, offset=0.05):
    """Gaussian rows kept out of the families' way: the component along every query direction is removed and replaced by
    -offset (as a cosine; a scalar or one value per row), so that no background row competes with cosines of ~0.2. Needs
    fewer queries than dimensions."""
    q = np.atleast_2d(np.asarray(queries, dtype=np.float64))
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    assert q.shape[0] < q.shape[1]
    g = rng.standard_normal((n, q.shape[1]))
    gram_inv = np.linalg.inv(q @ q.T)
    g -= (g @ q.T) @ gram_inv @ q                                     # orthogonal to every query
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    push = np.ones(q.shape[0]) @ gram_inv @ q                          # push . q_j = 1 for every unit query q_j
    off = np.broadcast_to(np.asarray(offset, dtype=np.float64), (n,))
    return (g - off[:, None] * push[None, :]).astype(np.float32)


class Case:
    """Adversarial families inside a background corpus. corpus [N, dim], queries [Q, dim] float32; plus_rows[q] / minus_rows[q]
    are the corpus rows of query q's own family."""

    def __init__(self, corpus, queries, plus_rows, minus_rows, k):
        self.corpus, self.queries, self.plus_rows, self.minus_rows, self.k = corpus, queries, plus_rows, minus_rows, k


def make_case(seed, dim, k, Q, cosine, N, plus_at=0, minus_at=None, n_minus=1, n_plus=None, scale=1.0, offset=None):
    """Q families (each built from its own draw of positions and signs) in N rows: all plus rows in one contiguous block
    starting at row plus_at (family after family), all minus rows in one block starting at minus_at (default: the end of the
    table), background rows everywhere else: cosines spread over -0.3 ... -0.05 against every query (a background of equal
    cosines would overflow the candidate buffer whenever a stage sets its threshold from background rows alone); `offset`
    (a value, or a function of (rng, N)) overrides that."""
    rng = np.random.default_rng(seed)
    # k + 4 plus rows by default: the (k+1)-th best fp16 score is then a plus row's too. select_wave's pivot may stop anywhere
    # between the k-th and the (k+1)-th key, so only then is its threshold known to sit AT s~(k) - 2 eps and not lower.
    n_plus = k + 4 if n_plus is None else n_plus
    fams = [build(dim, k, n_minus, cosine, scale=scale, rng=rng, n_plus=n_plus) for _ in range(Q)]
    queries = np.stack([f["q"] for f in fams])
    n_p = fams[0]["plus"].shape[0]
    minus_at = N - Q * n_minus if minus_at is None else minus_at
    assert plus_at + Q * n_p <= minus_at or minus_at + Q * n_minus <= plus_at
    assert max(plus_at + Q * n_p, minus_at + Q * n_minus) <= N
    off = rng.uniform(0.05, 0.3, N) if offset is None else offset(rng, N) if callable(offset) else offset
    corpus = background(rng, N, queries, off) * np.float32(scale)
    plus_rows, minus_rows = [], []
    for qi, f in enumerate(fams):
        plus_rows.append(np.arange(n_p) + plus_at + qi * n_p)
        minus_rows.append(np.arange(n_minus) + minus_at + qi * n_minus)
        corpus[plus_rows[-1]] = f["plus"]
        corpus[minus_rows[-1]] = f["minus"]
    return Case(corpus, queries, plus_rows, minus_rows, k)


def conditions(queries, corpus, k, minus_rows_of, bound):
    """The CPU preconditions of a case, over the WHOLE corpus (background and the other families included). For every query:
    the largest |S~ - S| over its own family's rows, the fp16 gap between the k-th best S~ and each of its minus rows, whether
    its minus rows are all inside the exact top-k, and whether the exact top-k differs from the top-k by S~. Returns a dict of
    arrays over queries; `bound` is the analytic E the gap is measured in."""
    S = exact_scores(queries, corpus)
    St = emulate_scores(emulate_rows(queries), emulate_rows(corpus))
    Q = S.shape[0]
    gap = np.empty(Q)
    minus_in, differs = np.empty(Q, dtype=bool), np.empty(Q, dtype=bool)
    for qi in range(Q):
        order = np.lexsort((np.arange(S.shape[1]), -S[qi]))[:k]
        order_t = np.lexsort((np.arange(S.shape[1]), -St[qi]))[:k]
        mr = np.asarray(minus_rows_of[qi])
        gap[qi] = St[qi, order_t[-1]] - St[qi, mr].max()
        minus_in[qi] = np.isin(mr, order).all()
        differs[qi] = set(order.tolist()) != set(order_t.tolist())
    return dict(gap=gap, gap_ratio=gap / bound, minus_in=minus_in, differs=differs, err=np.abs(St - S), S=S, St=St)


SLACK = 2.0 ** -20                 # the float32 roundings of the normalisation, relative to the fp16 error bound
GAP_TARGET = 1.25


def emit_bound(dim):
    """E: the analytic fp16-pass bound plus 1e-6 of absolute slack; independent of the project's own eps."""
    return 2.0 ** -10 + 2.0 * pad_dim(dim) * 2.0 ** -24 + 1e-6


def check_case(case, corpus=None, k=None):
    """Asserts the CPU preconditions of a case over its whole corpus (see conditions) and returns the measured figures."""
    corpus = case.corpus if corpus is None else corpus
    k = case.k if k is None else k
    dim = corpus.shape[1]
    E = emit_bound(dim)
    c = conditions(case.queries, corpus, k, case.minus_rows, E)
    own = np.zeros(c["err"].shape, dtype=bool)
    for qi in range(len(case.queries)):
        own[qi, case.plus_rows[qi]] = own[qi, case.minus_rows[qi]] = True
    err = float(c["err"][own].max())
    assert err <= (2.0 ** -10 + 2.0 ** -22) * (1.0 + SLACK), err            # the rows are legal inputs to the proof
    assert c["gap_ratio"].min() >= GAP_TARGET, c["gap_ratio"].min()          # a threshold one bound below s~(k) loses a row ...
    assert c["minus_in"].all()                                               # ... that the exact top-k contains
    assert c["differs"].all()                                                # not vacuous: the fp16 order alone is wrong
    return dict(err=err, err_ratio=err / analytic_bound(dim), gap=float(c["gap"].max()), gap_ratio=float(c["gap_ratio"].min()), E=E)


# (dim, k, Q, cosine, N) of the shape sweep in tests/test_dense_exactness_gpu.py. 300 queries need a dim whose random
# cross-family cosines (sd 1 / sqrt(dim)) stay far below the families' own cosine: dim 384 at cosine 0.25.
SHAPES = [
    (64, 1, 1, 0.19, 2305), (64, 5, 1, 0.19, 2600), (64, 20, 1, 0.19, 6000), (64, 100, 1, 0.19, 2600), (64, 256, 1, 0.19, 6000),
    (100, 5, 1, 0.19, 2600), (100, 100, 1, 0.19, 4000), (100, 256, 1, 0.19, 2600),
    (384, 1, 300, 0.25, 3000), (384, 5, 300, 0.25, 5000), (384, 20, 130, 0.25, 6000), (384, 256, 1, 0.19, 3000),
    (1536, 1, 130, 0.19, 2600), (1536, 20, 130, 0.19, 5000), (1536, 100, 1, 0.19, 3000), (1536, 256, 1, 0.19, 2600),
]
