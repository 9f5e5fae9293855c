"""GPU: each cross-encoder forward held to its OWN measured error, not to the product bars.

The product bars (4e-3 on a logit, 1e-3 per component of a unit vector) are 10 to 100 times wider than what the split-fp16 forward
delivers, so a kernel that lost one correction product of one GEMM would still pass every other test. Here the classifier logits
of ALL pairs and every component of the raw mean-pooled vectors are compared with the float64 oracle, and the four figures

    logit max / rms    max and rms over all pairs of |logit - oracle|
    head  max / rms    max and rms over all components of |raw pooled - oracle| / ||oracle||

must stay within BUDGET: 2 x the figure measured on the MI355X for split fp16 (option ce_mx = -1) and 1.5 x for MX (ce_mx = 1).
The forward is deterministic and independent of the batch composition (pinned below and in tests/test_length_class_invariance_gpu.py),
so the margin is only room for a legitimate re-association of fp32 sums. tests/test_ce_error_budget.py pins on the CPU simulator
that a forward without one correction product is >= 20 x (split fp16) or >= 2 x (MX, one linear site as plain hi.hi) worse on this
batch: the margins sit under those ratios. The MX budget does NOT separate the hi8 rounding mode or the missing P_lo term
(1.25 x and 1.33 x on the simulator, see that module).

Model: seeded MiniLM (seed 99, logits centred), loaded as cross-encoder and as embedding model (normalize = 0); both heads get the
pair token types, so one oracle encoder pass serves both. Batch: 96 pairs at L = 128, ce_stress.batch(seed = 2468 + i) for i < 4 with
LENS tiled: 7040 packed rows = exactly 55 MX token tiles (128 rows) and 27.5 split-fp16 tiles (256 rows). The first 95 pairs alone
(6912 rows: pair 96 is a full 128 rows, so this is 54 and 27 whole tiles) and the first 92 (6544 rows: a part-filled last tile for
both kernels) must give the first 95 / 92 results bit for bit. The same checks run at hidden 128, FFN 512, 2 layers (split fp16
only: the unfused LayerNorm and the GEMM instantiations of a non-384 shape).

Measured on the MI355X (96 pairs), beside the CPU simulator (tools/ce_numerics_sim.py; split16 / shiprn; 24 pairs for MiniLM):

    forward             logit max   logit rms   head max   head rms  | simulated: logit max   logit rms   head max   head rms
    MiniLM split fp16   1.05e-4     2.03e-5     2.84e-6    1.52e-7   |            1.5e-5      7.4e-6      3.0e-7     7.3e-8
    MiniLM MX           1.14e-3     3.52e-4     1.91e-5    2.67e-6   |            5.1e-4      2.7e-4      2.2e-5     2.6e-6
    h128   split fp16   4.44e-6     1.23e-6     3.55e-7    4.30e-8   |            1.7e-6      9.5e-7      1.2e-7     3.2e-8

(The first 24 of the 96 pairs, the simulator's batch, measure 4.6e-5 / 1.8e-5 / 7.3e-7 / 1.2e-7 on split fp16 and 6.8e-4 / 3.2e-4 /
1.5e-5 / 2.6e-6 on MX.)

The budgets are multiples of what the MI355X MEASURES, not of a derived floor. The GPU's split-fp16 figures are about 2 x the
simulator's from the first layer on, at every depth (the simulator rounds only the MFMA operands); the kernels' fp32 stages account
for that at one layer and for 1.4 x of the 2.5 x at six, the rest has no stage assigned. The budgets hold a
later change to today's error; they do not say that today's error is the least these kernels could have.

Run against four scratch builds of the library without one correction MFMA each (QKV GEMM without W_lo * x_hi; attention without
K_lo * Q_hi; without V_hi * P_lo; MX QKV GEMM without the bf8 MFMA), test_forward_stays_within_its_own_measured_error failed in every
forward that runs the changed kernel, at 3 x to 500 x the measured figure, and passed with unchanged bits in the others."""
import numpy as np
import pytest

import ce_stress as S
from oracle import bert_oracle as B

pytestmark = pytest.mark.gpu

MINILM = S.CFG
H128 = S.H128
SPLIT16_MARGIN, MX_MARGIN = S.SPLIT16_MARGIN, S.MX_MARGIN
# measured on the MI355X: (logit max, logit rms, head max, head rms); the budget is margin x measured
MEASURED = {
    ("minilm", -1): (1.052e-4, 2.034e-5, 2.836e-6, 1.516e-7),
    ("minilm", 1): (1.144e-3, 3.516e-4, 1.912e-5, 2.672e-6),
    ("h128", -1): (4.436e-6, 1.233e-6, 3.546e-7, 4.296e-8),
}
KEYS = ("logit_max", "logit_rms", "raw_max", "raw_rms")


def budget(model, mode):
    margin = MX_MARGIN if mode == 1 else SPLIT16_MARGIN
    return {k: margin * v for k, v in zip(KEYS, MEASURED[(model, mode)])}


_WORLD = {}


def world(model):
    """(cfg, weights, the 96-pair batch, the oracle's logits and raw pooled vectors): computed once per module"""
    if model not in _WORLD:
        cfg = MINILM if model == "minilm" else H128
        w = S.budget_weights(cfg, 99)
        ids, tt, lens = S.budget_batch(4, cfg)
        _WORLD[model] = (cfg, w, (ids, tt, lens), S.oracle_heads(w, cfg, ids, tt, lens))
    return _WORLD[model]


@pytest.fixture(scope="module")
def eng():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=384, device=0)
    e.loaded = None
    yield e
    e.close()


def run(eng, model, mode, n=None):
    """(logits, raw pooled vectors) of the first n pairs of the model's batch on one forward"""
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    cfg, w, (ids, tt, lens), _ = world(model)
    if eng.loaded != model:
        eng.ce_load(cfg, flatten_state_dict(w, cfg["layers"]))
        eng.embed_load(cfg, flatten_state_dict(w, cfg["layers"], head=False), normalize=False)
        eng.loaded = model
    eng.set_option("ce_mx", mode)
    try:
        return eng.ce_score(ids[:n], tt[:n], lens[:n]), eng.embed(ids[:n], tt[:n], lens[:n])
    finally:
        eng.set_option("ce_mx", 0)


CASES = [pytest.param("minilm", -1, id="minilm-split16"), pytest.param("minilm", 1, id="minilm-mx"),
         pytest.param("h128", -1, id="h128-split16")]


@pytest.mark.parametrize("model,mode", CASES)
def test_forward_stays_within_its_own_measured_error(eng, model, mode):
    _, _, (ids, _, _), (exp_logits, exp_raw) = world(model)
    logits, raw = run(eng, model, mode)
    assert logits.shape == exp_logits.shape and raw.shape == exp_raw.shape
    assert np.isfinite(logits).all() and np.isfinite(raw).all()
    got = S.budget_errors(logits, raw, exp_logits, exp_raw)
    print(f"\nMEASURED {model} ce_mx={mode}: " + " ".join(f"{k} {got[k]:.3e}" for k in KEYS))
    lim = budget(model, mode)
    over = {k: (got[k], lim[k]) for k in KEYS if not got[k] <= lim[k]}
    assert not over, f"{model} ce_mx={mode}: over budget (figure, budget): {over}"


@pytest.mark.parametrize("n", [95, 92])
@pytest.mark.parametrize("model,mode", CASES)
def test_fewer_pairs_give_the_same_bits(eng, model, mode, n):
    """The first n pairs sit in the same packed rows whatever follows them. 96 pairs end half way through a 256-row split-fp16 tile
    and on an MX tile edge; 95 pairs end on a tile edge of both; 92 pairs (6544 rows = 51.1 x 128 = 25.6 x 256) leave both kernels
    a part-filled last tile. None of that may change a bit of the first n results."""
    logits, raw = run(eng, model, mode)
    logits_n, raw_n = run(eng, model, mode, n)
    np.testing.assert_array_equal(logits_n, logits[:n])
    np.testing.assert_array_equal(raw_n, raw[:n])


def test_forced_mx_runs_the_mx_forward(eng):
    """The budgets are one-sided: split-fp16 results would pass every MX budget with 10 x to spare, so option ce_mx = 1 quietly
    ignored would go unseen. The two forwards round differently at every GEMM: their results differ in bits on both heads, and the
    MX logit rms lies above the whole split-fp16 BUDGET (3.5e-4 measured against 4.1e-5)."""
    _, _, _, (exp_logits, exp_raw) = world("minilm")
    (l_mx, r_mx), (l_s, r_s) = run(eng, "minilm", 1), run(eng, "minilm", -1)
    assert (l_mx != l_s).mean() > 0.9 and (r_mx != r_s).mean() > 0.9
    assert S.budget_errors(l_mx, r_mx, exp_logits, exp_raw)["logit_rms"] > budget("minilm", -1)["logit_rms"]
