"""CPU: the adversarial fp16 rows of tests/fp16_adversary.py do what the GPU tests rely on, judged on the numpy emulation of
the fp16 pass alone (no GPU, none of the project's own error bounds)."""
import numpy as np
import pytest

import fp16_adversary as A


def test_emulated_rounding_directions():
    """Set A rounds up, set B rounds down, whatever power of two scales the row."""
    for scale in (1.0, 2.0 ** -100, 2.0 ** 90):
        f = A.build(64, 3, 1, 0.19, scale=scale)
        mag, kind = A._magnitudes(64, 0.19)
        r = A.emulate_rows(f["q"])[0].astype(np.float64)
        assert (r[kind == 0] > mag[kind == 0]).all() and (r[kind == 1] < mag[kind == 1]).all()
        rel = np.abs(r[kind < 2] / mag[kind < 2] - 1.0)
        assert rel.min() > 0.96 * A.U16 and rel.max() < 1.04 * A.U16
        assert abs(np.linalg.norm(f["q"].astype(np.float64)) / scale - A.SCALE) < 1e-4


def test_plus_rows_tie_exactly_and_nearly():
    f = A.build(64, 8, 2, 0.19, rng=np.random.default_rng(3))
    assert np.array_equal(f["plus"][0], f["plus"][4]) and np.array_equal(f["plus"][3], f["plus"][7])
    s = f["S_plus"]
    assert s[0] == s[4] and len(set(s[:4].tolist())) == 4 and 1e-8 < s[:4].max() - s[:4].min() < 1e-5
    assert f["S_minus"].min() > s.max()                       # every minus row outranks every plus row exactly ...
    assert f["St_minus"].max() < f["St_plus"].min()           # ... and trails every one of them in fp16


def test_pad_columns_stay_zero_for_a_dim_off_the_tile():
    f = A.build(100, 5, 1, 0.19, rng=np.random.default_rng(4))
    assert f["q"].shape == (100,) and f["plus"].shape == (5, 100) and A.pad_dim(100) == 128


@pytest.mark.parametrize("dim,k,Q,cosine,N", A.SHAPES)
def test_preconditions_of_every_gpu_shape(dim, k, Q, cosine, N):
    """For every (dim, k, Q) the GPU sweep runs, over the whole corpus (background and foreign families included):
      max |S~ - S| over the built rows <= (2^-10 + 2^-22) * (1 + 2^-20): the rows are legal inputs to the proof;
      S~(k-th best) - S~(minus row) >= 1.25 * E with E = 2^-10 + 2 * dim_pad * 2^-24 + 1e-6, and every minus row's exact
        cosine is inside the exact top-k: a threshold ONE bound below s~(k) must lose a true top-k row;
      the exact top-k differs from the top-k by S~: the case is not vacuous.
    Reached in the emulation (max |S~ - S| / (2^-10 + 2 * dim_pad * 2^-24), gap / E):
      dim   64 cosine 0.19   0.85   1.51          dim  384 cosine 0.19   0.77   1.47
      dim  100 cosine 0.19   0.77   1.48          dim  384 cosine 0.25   0.79   1.36
      dim 1536 cosine 0.19   0.69   1.30
    (the error scales with 1 - cosine: 2^-10 * (1 - S) per row, twice that between a plus and a minus row)."""
    E = 2.0 ** -10 + 2.0 * ((dim + 127) // 128 * 128) * 2.0 ** -24 + 1e-6
    case = A.make_case(1000 + dim + k + Q, dim, k, Q, cosine, N)
    m = A.check_case(case)
    assert m["E"] == E
    print(f"dim {dim} k {k} Q {Q}: max|S~-S| = {m['err']:.3e} ({m['err_ratio']:.3f} of the analytic bound), gap = {m['gap_ratio']:.3f} E")


def test_a_threshold_of_one_bound_loses_the_minus_row():
    """The emulated search itself: with tau = s~(k) - 2 E the minus row survives, with tau = s~(k) - E it is lost."""
    case = A.make_case(7, 64, 20, 1, 0.19, 3000)
    c = A.conditions(case.queries, case.corpus, 20, case.minus_rows, A.emit_bound(64))
    st = c["St"][0]
    kth = np.sort(st)[-20]
    m = case.minus_rows[0][0]
    assert st[m] >= kth - 2 * A.emit_bound(64) and st[m] < kth - A.emit_bound(64)
