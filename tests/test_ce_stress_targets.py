"""CPU: the stress transforms of tests/ce_stress.py reach their targets on the MiniLM shape (seed 99, the model of
tests/test_cross_encoder_stress_gpu.py), so that an edit of a transform cannot quietly make the GPU stress levels mild; and the
preconditions of tests/test_embeddings_stress_gpu.py: the oracle's pooled vectors are long enough for the unit-vector bars to mean
something, and the split-fp16 operand scheme stays far inside them on the CPU simulator."""
import numpy as np
import pytest

import ce_stress as S
from oracle import bert_oracle as B

CFG = B.minilm_config()
W = B.seeded_weights(CFG, 99)


def test_seeded_weights_are_the_mild_baseline():
    st = S.stats(W, CFG)
    assert 1.8 < st["attn_std"] < 3.0                    # ~2.5 per row: no sharp head
    assert st["outlier"] < 1.5                           # no outlier feature
    assert st["gelu_tail"] < 1e-3                        # the GELU never sees |x| > 5


def test_sharp_scales_the_attention_logits():
    base = S.stats(W, CFG)["attn_std"]
    assert S.stats(S.sharp(W, CFG, 1.5), CFG)["attn_std"] > max(4.5, 2.0 * base)
    st = S.stats(S.sharp(W, CFG, 2), CFG)
    assert st["attn_std"] > max(8.0, 3.6 * base)
    assert st["outlier"] < 1.5                           # only the attention changed
    np.testing.assert_array_equal(S.sharp(W, CFG, 2)["bert.encoder.layer.0.attention.self.value.weight"],
                                  W["bert.encoder.layer.0.attention.self.value.weight"])


def test_outliers_make_a_few_dims_dominant_in_every_layernorm():
    assert S.stats(S.outliers(W, CFG, 8), CFG)["outlier"] > 7.0
    w = S.outliers(W, CFG, 12, 3)
    assert S.stats(w, CFG)["outlier"] > 11.0
    for name in ("bert.embeddings.LayerNorm.", "bert.encoder.layer.0.attention.output.LayerNorm.", "bert.encoder.layer.5.output.LayerNorm."):
        g, b = w[name + "weight"], W[name + "weight"]
        np.testing.assert_allclose(g[list(S.OUTLIER_DIMS)], 12 * b[list(S.OUTLIER_DIMS)], rtol=1e-6)
        assert (w[name + "bias"][list(S.OUTLIER_DIMS)] - W[name + "bias"][list(S.OUTLIER_DIMS)] > 2.99).all()
        others = np.setdiff1d(np.arange(CFG["hidden"]), S.OUTLIER_DIMS)
        np.testing.assert_array_equal(g[others], b[others])


def test_ffn_tails_push_the_gelu_inputs_past_5():
    assert S.stats(S.ffn_tails(W, CFG, 3), CFG)["gelu_tail"] > 0.05


def test_centre_logits_puts_the_oracle_logits_around_0():
    w = S.centre_logits(S.sharp(W, CFG, 2), CFG)
    ids, tt, lens = S.probe_batch(CFG, pairs=8)
    z = B.forward_logits(w, CFG, ids, tt, lens, fast_erf=True)
    assert abs(float(np.median(z))) < 3.0 and w["classifier.bias"][0] != W["classifier.bias"][0]


# ---- preconditions of the embedding-head stress test (tests/test_embeddings_stress_gpu.py): its batch, token types 0 ------------
_POOLED = {}


def _pooled(name):
    """(stress weights, the oracle's un-normalised pooled vectors of the 24 texts)"""
    if name not in _POOLED:
        w = S.LEVELS[name](W)
        ids, tt = S.batch(pair_types=False)
        _POOLED[name] = (w, B.sentence_embeddings(w, CFG, ids.astype(np.int64), tt.astype(np.int64), S.LENS, normalize=False, fast_erf=True))
    return _POOLED[name]


@pytest.mark.parametrize("name", list(S.LEVELS))
def test_pooled_vectors_are_long_enough_to_normalise(name):
    """||pooled|| >= 10 at every level (15 to 116 seen): dividing by it is well conditioned, so an error of the unit vector is an
    error of the encoder and not of a near-zero mean."""
    _, raw = _pooled(name)
    assert np.isfinite(raw).all()
    assert np.linalg.norm(raw, axis=1).min() >= 10.0


@pytest.mark.parametrize("name", list(S.LEVELS))
def test_split_fp16_operands_stay_far_inside_the_embedding_bar_on_the_simulator(name):
    """tools/ce_numerics_sim.py, scheme split16 (what the split-fp16 kernels store): under 1e-5 per component of the unit vector at
    every level, a hundredth of the 1e-3 bar. A GPU miss of the MX forward at a level is then MX operand precision, not the test."""
    from tools import ce_numerics_sim as sim
    w, raw = _pooled(name)
    ids, tt = S.batch(pair_types=False)
    got = sim.sentence_embeddings(w, CFG, ids.astype(np.int64), tt.astype(np.int64), S.LENS, sim.Scheme("split16"))
    exp = raw / np.linalg.norm(raw, axis=1, keepdims=True)
    assert np.abs(got - exp).max() < 1e-5
