"""CPU: the batch of tests/test_cross_encoder_budget_gpu.py separates the shipped cross-encoder arithmetic from arithmetic that lost
one correction product, on the CPU simulator (tools/ce_numerics_sim.py). The GPU test holds each forward to a small multiple of
its own measured error; that only bites if a forward without a correction product lands well outside the multiple, and this
module pins that it does, so that an edit of the batch or the weights cannot quietly make the budget toothless.

Model: seeded MiniLM (seed 99) with centred logits; batch: the 24 pairs of ce_stress.batch() (one quarter of the GPU test's 96),
pair token types on both heads. Every figure is an rms over the batch of |logit - oracle|, or of |raw pooled - oracle| / ||oracle||
over all components, and every assertion is a ratio mutant / shipped.

    split16 (hi.hi + lo.hi + hi.lo at all eight products): every one of the six linear sites run as plain hi.hi (scheme f16, all six
    layers), Q.K^T without K_lo.Q_hi and P.V without V_hi.P_lo must each be >= 20 x the shipped error on both heads. The GPU
    budget is 2 x measured.
    MX (shiprn: hi16 + lo8 operands in the GEMMs, attention in split fp16): every linear site as plain hi.hi must be >= 2 x the
    shipped error on both heads. The GPU budget is 1.5 x measured.

NOT covered, on purpose: the MX forward's hi8 rounding mode and its missing P_lo term. The budget does not separate them from
what ships: on 96 pairs the logit rms is 3.40e-4 as shipped, 4.25e-4 with hi8 truncated and 4.53e-4 without P_lo (1.25 x and
1.33 x, inside the 1.5 x margin); on 24 pairs the head rms is 2.64e-6 as shipped and 2.48e-6 with truncation. Nobody should read
the MX budget as guarding either.

The hidden-128 shape of the GPU test (ce_stress.H128, split fp16 only) gets one shipped run and one mutant, the Q projection as
plain hi.hi, on all 96 pairs of its batch: that pins the simulated figures beside that shape's GPU budget and that the budget
bites there too.

Ratios seen (logits / head; this module prints them, run with -s): Q 117 / 82, K 123 / 114, V 483 / 331, attention-out 455 / 322,
FFN-up 492 / 300, FFN-down 323 / 309, k_lo 120 / 95, p_lo 58 / 22 (the thinnest: 10 % over the bar on the head); MX 2.9 / 2.6,
4.6 / 3.4, 13.3 / 9.0, 10.3 / 8.7, 15.9 / 8.3, 7.4 / 8.5; hidden 128: Q 73 / 52."""
import numpy as np
import pytest

import ce_stress as S
from tools import ce_numerics_sim as sim

CFG = S.CFG
SPLIT16_RATIO, MX_RATIO = S.SPLIT16_MUTANT_RATIO, S.MX_MUTANT_RATIO
SPLIT16_MUTANTS = [("site", s) for s in sim.SITES] + [("attn", d) for d in sim.ATTN_DROPS]
MX_MUTANTS = [("site", s) for s in sim.SITES]


@pytest.fixture(scope="module")
def world():
    """weights, the batch, the oracle's two heads (computed once) and a cache of simulated error figures"""
    w = S.budget_weights()
    ids, tt, lens = S.budget_batch()
    exp = S.oracle_heads(w, CFG, ids, tt, lens)
    cache = {}

    def errors(scheme, kind=None, what=None):
        key = (scheme, kind, what)
        if key not in cache:
            kw = {} if kind is None else {"site_scheme": {what: sim.Scheme("f16")}} if kind == "site" else {"attn_drop": (what,)}
            W, x = sim.hidden(w, CFG, ids.astype(np.int64), tt.astype(np.int64), lens, sim.Scheme(scheme), **kw)
            cache[key] = S.budget_errors(*S.heads(W, x, lens), *exp)
            print(f"\nSIMULATED {scheme} {kind or 'shipped'} {what or ''}: " + " ".join(f"{k} {v:.2e}" for k, v in cache[key].items()))
        return cache[key]
    return errors


def test_shipped_schemes_are_where_the_issue_measured_them(world):
    """split16 1.5e-5 max / 7.4e-6 rms on the logits and 7.3e-8 rms on the head; MX 5.1e-4 / 2.7e-4 and 2.6e-6: within 15 %,
    the room a change of BLAS summation order could ever take at these magnitudes is far smaller."""
    s, m = world("split16"), world("shiprn")
    assert s["logit_max"] == pytest.approx(1.5e-5, rel=0.15) and s["logit_rms"] == pytest.approx(7.4e-6, rel=0.15)
    assert s["raw_rms"] == pytest.approx(7.3e-8, rel=0.15)
    assert m["logit_max"] == pytest.approx(5.1e-4, rel=0.15) and m["logit_rms"] == pytest.approx(2.7e-4, rel=0.15)
    assert m["raw_rms"] == pytest.approx(2.6e-6, rel=0.15)


@pytest.mark.parametrize("kind,what", SPLIT16_MUTANTS, ids=[w for _, w in SPLIT16_MUTANTS])
def test_split16_without_one_correction_product_is_20x_worse(world, kind, what):
    base, mut = world("split16"), world("split16", kind, what)
    rl, rr = mut["logit_rms"] / base["logit_rms"], mut["raw_rms"] / base["raw_rms"]
    print(f"\nRATIO split16 {what}: logits {rl:.1f} head {rr:.1f}")
    assert rl >= SPLIT16_RATIO and rr >= SPLIT16_RATIO, f"{what}: logit rms x{rl:.1f}, head rms x{rr:.1f}"


@pytest.mark.parametrize("kind,what", MX_MUTANTS, ids=[w for _, w in MX_MUTANTS])
def test_mx_site_without_corrections_is_2x_worse(world, kind, what):
    base, mut = world("shiprn"), world("shiprn", kind, what)
    rl, rr = mut["logit_rms"] / base["logit_rms"], mut["raw_rms"] / base["raw_rms"]
    print(f"\nRATIO mx {what}: logits {rl:.1f} head {rr:.1f}")
    assert rl >= MX_RATIO and rr >= MX_RATIO, f"{what}: logit rms x{rl:.1f}, head rms x{rr:.1f}"


def test_h128_row_of_the_gpu_table_and_its_q_mutant():
    """hidden 128, FFN 512, 2 layers, the 96 pairs of the GPU test: split16 as shipped is where the GPU module's table has it
    (1.7e-6 / 9.5e-7 on the logits, 1.2e-7 / 3.2e-8 on the head, within 15 %), and the Q projection as plain hi.hi is >= 20 x worse."""
    cfg = S.H128
    w = S.budget_weights(cfg, 99)
    ids, tt, lens = S.budget_batch(4, cfg)
    exp = S.oracle_heads(w, cfg, ids, tt, lens)

    def errors(**kw):
        W, x = sim.hidden(w, cfg, ids.astype(np.int64), tt.astype(np.int64), lens, sim.Scheme("split16"), **kw)
        return S.budget_errors(*S.heads(W, x, lens), *exp)
    base, mut = errors(), errors(site_scheme={"attention.self.query": sim.Scheme("f16")})
    print("\nSIMULATED h128 split16: " + " ".join(f"{k} {v:.2e}" for k, v in base.items()))
    for k, v in dict(logit_max=1.7e-6, logit_rms=9.5e-7, raw_max=1.2e-7, raw_rms=3.2e-8).items():
        assert base[k] == pytest.approx(v, rel=0.15), k
    rl, rr = mut["logit_rms"] / base["logit_rms"], mut["raw_rms"] / base["raw_rms"]
    print(f"RATIO h128 split16 attention.self.query: logits {rl:.1f} head {rr:.1f}")
    assert rl >= SPLIT16_RATIO and rr >= SPLIT16_RATIO


def test_margins_sit_under_the_mutant_ratios_and_the_batch_ends_where_the_gpu_test_says():
    """The GPU budgets (margin x measured) stay under what a mutant costs, and the 96-pair batch packs into 7040 rows = 55 MX token
    tiles of 128 = 27.5 split-fp16 tiles of 256; 95 pairs end on a tile edge of both kernels, 92 pairs inside a tile of both."""
    assert S.SPLIT16_MARGIN < SPLIT16_RATIO and S.MX_MARGIN < MX_RATIO
    rows = np.cumsum((S.budget_batch(4)[2] + 15) // 16 * 16)
    assert rows[95] == 7040 == 55 * 128 and rows[95] % 256 == 128
    assert rows[94] == 6912 == 54 * 128 == 27 * 256
    assert rows[91] == 6544 and rows[91] % 128 != 0 and rows[91] % 256 != 0


def test_site_lookup_is_exact():
    """`output.dense` is the FFN-down projection alone: the simulator refuses a site it does not know, and a scheme at
    `output.dense` leaves `attention.output.dense` as shipped (the two give different hidden states)."""
    with pytest.raises(AssertionError):
        sim.hidden({}, CFG, None, None, None, sim.Scheme("split16"), site_scheme={"dense": sim.Scheme("f16")})
    cfg = dict(vocab_size=200, hidden=64, layers=1, heads=2, ffn=128, max_pos=16, type_vocab=2, eps=1e-12)
    from oracle import bert_oracle as B
    w = B.seeded_weights(cfg, 3)
    ids = np.random.default_rng(0).integers(5, 200, (2, 16))
    tt, lens = np.zeros_like(ids), np.array([16, 9])
    run = lambda **kw: sim.hidden(w, cfg, ids, tt, lens, sim.Scheme("split16"), **kw)[1]
    plain, down, attn_out = run(), run(site_scheme={"output.dense": sim.Scheme("f16")}), run(site_scheme={"attention.output.dense": sim.Scheme("f16")})
    both = run(site_scheme={"output.dense": sim.Scheme("f16"), "attention.output.dense": sim.Scheme("f16")})
    assert np.array_equal(plain, run(site_scheme={}, attn_drop=()))
    d = lambda a, b: float(np.abs(a - b).max())
    assert d(plain, down) > 0 and d(plain, attn_out) > 0 and d(down, attn_out) > 0 and d(both, down) > 0 and d(both, attn_out) > 0


def test_simulator_fp16_rounding_is_numpy_fp16_rounding():
    """sim.f16 rounds the fp16-subnormal range arithmetically (speed): the same bits as astype(np.float16) on every finite fp16
    value, every midpoint between two neighbours (the ties), the float64 values next to each midpoint, and random values over
    13 decades, in both signs; overflow to infinity included."""
    rng = np.random.default_rng(0)
    ref = lambda x: x.astype(np.float16).astype(np.float64)
    h = np.arange(0x7C00, dtype=np.uint16)
    a, b = h.view(np.float16).astype(np.float64), (h + 1).astype(np.uint16).view(np.float16).astype(np.float64)
    b[-1] = 65536.0                                                   # the value past the largest finite one
    mid = (a + b) / 2
    rnd = rng.standard_normal(200000) * 10.0 ** rng.uniform(-9, 4, 200000)
    cases = np.concatenate([a, mid, np.nextafter(mid, np.inf), np.nextafter(mid, -np.inf), rnd, [0.0, 1e-50, 2.0 ** -25, 65519.9, 65520.0]])
    for x in (cases, -cases):
        with np.errstate(over="ignore"):
            want, got = ref(x), sim.f16(x)
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
