"""GPU: the sentence-embedding forward (the cross-encoder's kernels behind the mean-pooling head) on the stress weights of
tests/ce_stress.py, against the float64 oracle, on each forward: option ce_mx = 1 (MX kernels, hi16 + lo8 operands), -1 (split fp16)
and 0 (the default). MiniLM shape, seed 99, the 24 texts of tests/test_cross_encoder_stress_gpu.py at L = 128 with token types 0,
all 24 checked; on the `sharp` level also a handful of texts at L_in = 300 (attention class 384) and 512, the classes whose MX
attention runs two query blocks per wave.

Bars. Normalised head: 1e-3 per component of the unit vector and 1 - cos < 1e-6, the project's bars for this head
(tests/test_embeddings_gpu.py). Raw head (normalize=0): max |got - exp| <= 1e-3 * ||exp|| per text, the unit-vector bar scaled by
the vector's length; an absolute bar cannot hold once ||pooled|| reaches 100.

Measured on the MI355X, maxima over the texts of a batch, next to the CPU simulator's prediction for MX (tools/ce_numerics_sim.py,
scheme shiprn, sentence_embeddings); `comp` is the largest per-component error of the unit vector, `raw` the raw head's
max |got - exp| / ||exp||. Option ce_mx = 0 takes MX at every level (an embedding model has no load-time probe), bit for bit:

    level (L_in)     ||pooled||   MX comp   MX 1-cos   MX raw    sim. MX comp   sim. MX 1-cos   split16 comp   split16 1-cos   default
    seeded (128)     20.0-20.3    1.5e-5    4.5e-9     1.5e-5    2.2e-5         5.1e-9          4.2e-7         3.1e-12         MX
    moderate (128)   18-85        1.4e-4    1.2e-8     1.3e-4    9.9e-5         9.5e-9          6.0e-6         2.6e-11         MX
    sharp (128)      19.6-20.3    1.9e-4    6.5e-7     1.9e-4    2.0e-4         7.3e-7          2.5e-5         9.1e-9          MX
    outlier (128)    73-116       5.4e-5    2.9e-9     5.7e-5    4.8e-5         2.0e-9          1.9e-6         2.4e-12         MX
    combined (128)   15-44        4.6e-5    2.9e-9     5.2e-5    4.7e-5         2.0e-9          4.6e-6         2.3e-11         MX
    sharp (300)      19.8-20.4    1.9e-4    5.1e-7     1.9e-4    -              -               7.8e-6         1.6e-9          MX
    sharp (512)      19.8-20.0    2.3e-4    5.9e-7     2.4e-4    -              -               9.6e-6         1.5e-9          MX

MX holds every bar at every level: the component bar with a margin of 4x or more, the raw bar likewise (in absolute terms the raw
error reaches 4.7e-3, which is why that bar is relative), and the cosine bar with 80x or more everywhere except `sharp`, where
1 - cos is 5.1e-7 to 6.5e-7: a margin of 1.5x, as the simulator predicted (7.3e-7). Sharp attention heads are where the MX operands
cost most; a model much sharper than `sharp(2)` would need the split-fp16 forward (option ce_mx = -1), which keeps 100x there.
"""
import numpy as np
import pytest

import ce_stress as S
from oracle import bert_oracle as B

pytestmark = pytest.mark.gpu

COMP_TOL = 1e-3                    # per component of the unit vector
COS_TOL = 1e-6                     # 1 - cos to the oracle
RAW_REL_TOL = 1e-3                 # raw head: max |got - exp| / ||exp||
CFG, LEVELS = S.CFG, S.LEVELS
MODES = ((1, "mx"), (-1, "split16"), (0, "default"))
# (lengths, L_in) of the batches: the 24 texts at 128, and the two long classes on the sharp level
BATCHES = {
    "L128": (S.LENS, S.L),
    "L300": (np.array([300, 257, 1, 289, 273, 300], dtype=np.int32), 300),
    "L512": (np.array([512, 385, 17, 500, 512], dtype=np.int32), 512),
}
# an embedding model takes MX by shape; the measurements above are what backs that
DEFAULT_IS_MX = {"seeded": True, "moderate": True, "sharp": True, "outlier": True, "combined": True}


def texts(bname):
    lens, L_in = BATCHES[bname]
    ids, tt = S.batch(lens, L_in, seed=2468 + L_in, pair_types=False) if bname != "L128" else S.batch(pair_types=False)
    return ids, tt, lens


_CACHE = {}


def level(name, bname="L128"):
    """(weights, the oracle's un-normalised pooled vectors of the batch, float64)"""
    if name not in _CACHE:
        _CACHE[name] = (LEVELS[name](B.seeded_weights(CFG, 99)), {})
    w, exp = _CACHE[name]
    if bname not in exp:
        ids, tt, lens = texts(bname)
        exp[bname] = B.sentence_embeddings(w, CFG, ids.astype(np.int64), tt.astype(np.int64), lens, normalize=False, fast_erf=True)
    return w, exp[bname]


@pytest.fixture(scope="module")
def eng():
    from optimized_rag_amd import RagEngine
    e = RagEngine(dim=384, device=0)
    e.loaded = None
    yield e
    e.close()


def embed(eng, name, mode, normalize, bname="L128"):
    from optimized_rag_amd.cross_encoder import flatten_state_dict
    w, raw = level(name, bname)
    if eng.loaded != (name, normalize):
        eng.embed_load(CFG, flatten_state_dict(w, CFG["layers"], head=False), normalize=normalize)
        eng.loaded = (name, normalize)
    ids, tt, lens = texts(bname)
    eng.set_option("ce_mx", mode)
    try:
        return eng.embed(ids, tt, lens), raw
    finally:
        eng.set_option("ce_mx", 0)


def unit_errors(got, raw):
    """(largest per-component error, largest 1 - cos) of unit vectors against the oracle's, float64"""
    got = got.astype(np.float64)
    exp = raw / np.linalg.norm(raw, axis=1, keepdims=True)
    cos = (got * exp).sum(1) / np.linalg.norm(got, axis=1)
    return float(np.abs(got - exp).max()), float((1.0 - cos).max())


def raw_error(got, raw):
    """largest over the texts of max |got - exp| / ||exp||"""
    return float((np.abs(got.astype(np.float64) - raw).max(1) / np.linalg.norm(raw, axis=1)).max())


def _cases(names):
    return [pytest.param(name, mode, id=f"{name}-{tag}") for name in names for mode, tag in MODES]


def _check(eng, name, mode, bname):
    got, raw = embed(eng, name, mode, True, bname)
    assert got.shape == raw.shape and np.isfinite(got).all()
    np.testing.assert_allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, atol=1e-5)
    comp, cos = unit_errors(got, raw)
    got0, _ = embed(eng, name, mode, False, bname)
    assert np.isfinite(got0).all()
    rel = raw_error(got0, raw)
    nrm = np.linalg.norm(raw, axis=1)
    print(f"\nMEASURED {bname} {name} ce_mx={mode}: comp {comp:.2e} 1-cos {cos:.2e} raw/||exp|| {rel:.2e} "
          f"raw abs {np.abs(got0 - raw).max():.2e} ||pooled|| {nrm.min():.1f}-{nrm.max():.1f}")
    assert comp < COMP_TOL and cos < COS_TOL and rel <= RAW_REL_TOL, \
        f"{bname} {name} ce_mx={mode}: component error {comp:.2e}, 1 - cos {cos:.2e}, raw error / ||exp|| {rel:.2e}"


@pytest.mark.parametrize("name,mode", _cases(LEVELS))
def test_stress_level_within_the_bars(eng, name, mode):
    _check(eng, name, mode, "L128")


@pytest.mark.parametrize("bname", ["L300", "L512"])
@pytest.mark.parametrize("name,mode", _cases(["sharp"]))
def test_sharp_level_in_the_long_attention_classes(eng, name, mode, bname):
    """L_in = 300 and 512 run in the attention classes 384 and 512: on MX two 16-query blocks per wave instead of one."""
    _check(eng, name, mode, bname)


@pytest.mark.parametrize("name", list(LEVELS))
def test_default_forward_is_the_pinned_one(eng, name):
    """Option ce_mx = 0 gives the bits of the forward DEFAULT_IS_MX names, on both heads."""
    for normalize in (True, False):
        default, _ = embed(eng, name, 0, normalize)
        forced, _ = embed(eng, name, 1 if DEFAULT_IS_MX[name] else -1, normalize)
        np.testing.assert_array_equal(default, forced)
