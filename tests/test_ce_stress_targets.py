"""CPU: the stress transforms of tests/ce_stress.py reach their targets on the MiniLM shape (seed 99, the model of
tests/test_cross_encoder_stress_gpu.py), so that an edit of a transform cannot quietly make the GPU stress levels mild."""
import numpy as np

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
