"""GPU: the cross-encoder forward on stress weights (tests/ce_stress.py: sharp attention heads, LayerNorm outlier dimensions, GELU
tails, logits centred where the sigmoid is steepest) against the float64 oracle, on each forward: option ce_mx = 1 (MX kernels,
hi16 + lo8 operands), -1 (split fp16) and 0 (the default: MX where the shape allows it and the load-time probe saw it hold).
Bars as in tests/test_cross_encoder_gpu.py: logits within 4e-3, sigmoid scores within 1e-3.

MiniLM shape (6 layers, hidden 384), seed 99; 24 pairs at L = 128 with lengths on the 16-row edges, 6 of them checked against the
oracle. Max |logit - oracle| over those 6 pairs, measured on the MI355X, next to the CPU simulator's prediction for MX
(tools/ce_numerics_sim.py, scheme shiprn); |MX - split16| is the largest difference over all 24 pairs (split16 is within 7e-4 of
the oracle on the checked pairs), and the last column the forward the load-time probe picked for option ce_mx = 0:

    level      MX measured   MX simulated   split16 measured   |MX - split16|, 24 pairs   default
    seeded     6.0e-4        5.1e-4         4.6e-5             6.8e-4                     MX
    moderate   9.8e-3        7.3e-3         6.2e-5             2.0e-2                     split16
    sharp      2.2e-2        1.7e-2         6.6e-4             3.1e-2                     split16
    outlier    2.5e-3        1.1e-3         9.2e-5             4.6e-3                     split16
    combined   2.6e-3        2.9e-3         5.5e-5             3.8e-3                     split16

MX holds the bar on the seeded model only. At the outlier and combined levels the 6 checked pairs pass on MX, but other pairs of the
same batch miss (4.6e-3, 3.8e-3): the probe is right to take split16 there. The forced-MX cases of the levels where the checked pairs
miss are strict xfails carrying the measured error: a precision fix of the MX forward has to turn them back on."""
import numpy as np
import pytest

import ce_stress as S
from oracle import bert_oracle as B

pytestmark = pytest.mark.gpu

LOGIT_TOL = 4e-3
SCORE_TOL = 1e-3
CFG, L, LENS, LEVELS = S.CFG, S.L, S.LENS, S.LEVELS          # shared with the embedding-head stress test
SEL = [0, 2, 7, 12, 18, 23]

# forced MX at the levels where the checked pairs miss the bar: max |logit - oracle| measured on the MI355X
MX_MISSES = {"moderate": "MX forward: max |logit - oracle| 9.8e-3, |score - oracle| 1.0e-3 on the MI355X (bar 4e-3 / 1e-3)",
             "sharp": "MX forward: max |logit - oracle| 2.2e-2, |score - oracle| 2.3e-3 on the MI355X (bar 4e-3 / 1e-3)"}
# the forward the load-time probe picks for option ce_mx = 0 (MX where it stays within 2.5e-3 of split16 on the probe's own batch)
DEFAULT_IS_MX = {"seeded": True, "moderate": False, "sharp": False, "outlier": False, "combined": False}


batch = S.batch


_LEVEL_CACHE = {}


def level(name):
    """(weights, oracle logits of the SEL pairs) of a stress level, logits centred"""
    if name not in _LEVEL_CACHE:
        w = S.centre_logits(LEVELS[name](B.seeded_weights(CFG, 99)), CFG)
        ids, tt = batch()
        exp = B.forward_logits(w, CFG, ids[SEL].astype(np.int64), tt[SEL].astype(np.int64), LENS[SEL], fast_erf=True)
        _LEVEL_CACHE[name] = (w, exp)
    return _LEVEL_CACHE[name]


@pytest.fixture(scope="module")
def eng():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=384, device=0)
    e.loaded_level = None
    yield e
    e.close()


def score(eng, name, mode):
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    w, exp = level(name)
    if eng.loaded_level != name:
        eng.ce_load(CFG, flatten_state_dict(w, CFG["layers"]))
        eng.loaded_level = name
    ids, tt = batch()
    eng.set_option("ce_mx", mode)
    try:
        return eng.ce_score(ids, tt, LENS), exp
    finally:
        eng.set_option("ce_mx", 0)


def _cases():
    for name in LEVELS:
        for mode, tag in ((1, "mx"), (-1, "split16"), (0, "default")):
            marks = [pytest.mark.xfail(strict=True, reason=MX_MISSES[name])] if mode == 1 and name in MX_MISSES else []
            yield pytest.param(name, mode, marks=marks, id=f"{name}-{tag}")


@pytest.mark.parametrize("name,mode", list(_cases()))
def test_stress_level_within_the_bar(eng, name, mode):
    got, exp = score(eng, name, mode)
    assert np.isfinite(got).all()
    err = float(np.abs(got[SEL] - exp).max())
    sig = lambda z: 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=np.float64)))
    serr = float(np.abs(sig(got[SEL]) - sig(exp)).max())
    assert err < LOGIT_TOL and serr < SCORE_TOL, f"{name} ce_mx={mode}: max |logit - oracle| {err:.2e}, max |score - oracle| {serr:.2e}"


@pytest.mark.parametrize("name", list(LEVELS))
def test_default_forward_follows_the_load_time_probe(eng, name):
    """The probe's choice, pinned: option ce_mx = 0 gives the forced-MX bits on the seeded model and the split-fp16 bits on every
    stress level; whichever it takes is within the bar of split16 (hence of the oracle) on all 24 pairs, not only the checked 6."""
    default, _ = score(eng, name, 0)
    mx, _ = score(eng, name, 1)
    split16, _ = score(eng, name, -1)
    np.testing.assert_array_equal(default, mx if DEFAULT_IS_MX[name] else split16)
    assert np.abs(default - split16).max() < LOGIT_TOL
