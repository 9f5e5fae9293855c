"""CPU: the numpy reference quantiser of the token-vector store's 8-bit form (tests/tokvec_q8_tools.py, the contract of
include/rag_hip.h), which the GPU tests hold rag_tokvec_fetch_host to bit for bit.

Checked here: every stored value is an fp16 value; the rounding agrees with torch.float8_e4m3fn's cast of the scaled, clipped
blocks (an independent implementation); the scale exponent is the smallest one that fits; quantising stored values returns them;
the edge blocks (zero, -0.0, amax at and one ulp above 448 * 2^e, below the lower clamp, 65504 / 65519 saturating to 57344, ties to
even on the E4M3 grid); bound (b): float64 MaxSim over the stored rows against float64 MaxSim over the original unit rows moves by
at most 2^-4 + 2^-13 (derived in the header: a component at or above the block's smallest normal moves by <= 2^-4 |x|, a smaller
one by <= 2^-18 amax; a mean of maxima is 1-Lipschitz).
Measured (seeded unit rows with a planted query component, 11 documents of 1 ... 257 rows, 33 query rows, 20 seeds per dim): the
float64 MaxSim moves by at most 2.7e-3 at dim 32, 2.1e-3 at dim 96, 1.6e-3 at dim 128, 6.6e-4 at dim 1024; the top 5 of the 11
documents is the same set in 18, 20, 19 and 20 of the 20 trials (neighbouring documents' planted strengths differ by 0.07: some
scores lie closer than the error). On an MI355X the kernel's scores over the tile-edge rows move by 9.3e-3, 5.8e-3, 4.3e-3 and
1.8e-3 (tests/test_tokvec_q8_gpu.py). Ranking quality on a real checkpoint's vectors is unmeasured: none exists offline."""
import numpy as np
import pytest

import m3_tools as M
import tokvec_q8_tools as Q8
import tokvec_tools as V

DIMS = [32, 96, 128, 1024]


def _seeded(dim, n=67):
    rng = np.random.default_rng(dim)
    unit = V.unit_rows(rng, n, dim)
    wide = (rng.standard_normal((n, dim)) * np.exp(rng.uniform(-12, 9, (n, 1)))).astype(np.float32)     # every exponent and both clamps
    return np.concatenate([unit, wide, Q8.edge_rows(dim)])


@pytest.mark.parametrize("dim", DIMS)
def test_stored_values_are_fp16_values_and_the_bytes_decode_to_them(dim):
    x = _seeded(dim)
    code, sb, vals = Q8.quantise(x)
    assert code.shape == x.shape and sb.shape == (x.shape[0], dim // 32) and vals.dtype == np.float32
    np.testing.assert_array_equal(vals.astype(np.float16).astype(np.float32).view(np.uint32), vals.view(np.uint32))
    np.testing.assert_array_equal(Q8.decode(code, sb).view(np.uint32), vals.view(np.uint32))
    assert ((code & 0x7f) != 0x7f).all()                             # the NaN codes are never stored
    assert sb.min() >= 127 - 15 and sb.max() <= 127 + 7
    assert np.abs(vals).max() <= 57344.0


@pytest.mark.parametrize("dim", DIMS)
def test_scale_exponent_is_the_smallest_that_fits(dim):
    x = _seeded(dim)
    e = Q8.block_exponents(x)
    amax = np.abs(x.reshape(x.shape[0], -1, 32)).max(axis=2).astype(np.float64)
    fits = amax <= 448.0 * np.ldexp(1.0, e)
    assert (fits | (e == 7)).all()
    assert ((amax > 448.0 * np.ldexp(1.0, e - 1)) | (e == -15)).all()
    assert (e == 7).any() and (e == -15).any() and len(np.unique(e)) >= 10


@pytest.mark.parametrize("dim", DIMS)
def test_rounding_agrees_with_torchs_e4m3fn_cast(dim):
    import torch
    x = _seeded(dim)
    code, sb, _ = Q8.quantise(x)
    scale = np.repeat(np.ldexp(1.0, sb.astype(np.int64) - 127), 32, axis=1)
    y = np.clip(x.astype(np.float64) / scale, -448.0, 448.0).astype(np.float32)      # a power-of-two scaling: exact or far below the grid
    got = torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    np.testing.assert_array_equal(got, code)


@pytest.mark.parametrize("dim", DIMS)
def test_quantising_stored_values_returns_them(dim):
    x = _seeded(dim)
    code, sb, vals = Q8.quantise(x)
    code2, sb2, vals2 = Q8.quantise(vals)
    np.testing.assert_array_equal(vals2.view(np.uint32), vals.view(np.uint32))
    # the bytes may differ only where a block's amax fell to a lower exponent: the values do not
    same_scale = np.repeat(sb2 == sb, 32, axis=1)
    np.testing.assert_array_equal(code2[same_scale], code[same_scale])


def test_edge_blocks():
    x = Q8.edge_rows(32)
    code, sb, vals = Q8.quantise(x)
    e = sb.astype(np.int64)[:, 0] - 127
    assert e[0] == -15 and (code[0] == 0).all() and (vals[0] == 0).all()
    # signed zeros: the sign bit is kept, the value is a zero of that sign
    np.testing.assert_array_equal(code[1, [0, 1, 5, 6]], [0x00, 0x80, 0x80, 0x00])
    np.testing.assert_array_equal(np.signbit(vals[1, :8]), np.signbit(x[1, :8]))
    # amax exactly 448 * 2^-3: e = -3, code 0x7e; one ulp above: e = -2, and the value rounds to 224 * 2^-2 = the same 56
    assert e[2] == -3 and code[2, 0] == 0x7e and vals[2, 0] == 56.0
    assert e[3] == -2 and code[3, 0] == 0x76 and vals[3, 0] == 56.0
    # the lower clamp: the step is fp16's 2^-24; 2^-25 ties to even (zero), 3 * 2^-25 ties to 2^-23
    assert e[4] == -15 and code[4, 0] == 0x7e
    np.testing.assert_array_equal(vals[4, 1:5], np.array([2.0 ** -24, 0.0, 2.0 ** -23, -0.0], dtype=np.float32))
    assert np.signbit(vals[4, 4])
    assert e[5] == -15 and vals[5, 0] == np.float32(448.0 * 2.0 ** -16) and vals[5, 3] == np.float32(2.0 ** -24)
    # 1e-6 * 2^15 = 0.0328 lies in [2^-5, 2^-4): step 2^-8, 8.39 steps -> 8: 2^-20
    assert e[6] == -15 and vals[6, 0] == np.float32(2.0 ** -20) and vals[6, 1] == np.float32(-(2.0 ** -20))
    # the upper clamp: 65504, 65519 and 60000 saturate to 57344
    assert e[7] == 7 and e[8] == 7
    np.testing.assert_array_equal(vals[7, :7], np.array([57344, -57344, 57344, 57344, -57344, 1, 192], dtype=np.float32))
    np.testing.assert_array_equal(vals[8, :4], np.array([57344, -57344, 49152, 0], dtype=np.float32))
    # ties to even at e = -8 (grid step 2^-3 of the value 1.x; subnormal step 2^-17)
    assert e[9] == -8
    exp = [1.75, 1.0, 1.25, 1.25, -1.5, 2.0 ** -14, 0.0, 2.0 ** -16, -(2.0 ** -16), 2.0 ** -14]
    np.testing.assert_array_equal(vals[9, :10], np.array(exp, dtype=np.float32))


@pytest.mark.parametrize("dim", DIMS)
def test_bound_b_on_seeded_unit_rows(dim):
    worst, top5_same, trials = 0.0, 0, 20
    for seed in range(trials):
        q, qo, d, do = Q8.planted_case(1000 * dim + seed, dim)
        st = Q8.stored(d)
        # per component: <= 2^-4 |x| at or above the block's smallest normal, <= 2^(e - 10) below
        e = np.repeat(Q8.block_exponents(d), 32, axis=1)
        err = np.abs(st.astype(np.float64) - d.astype(np.float64))
        assert (err <= np.maximum(2.0 ** -4 * np.abs(d.astype(np.float64)), np.ldexp(1.0, e - 10))).all()
        a = np.array([M.maxsim(q, d[do[i]:do[i + 1]]) for i in range(len(do) - 1)])
        b = np.array([M.maxsim(q, st[do[i]:do[i + 1]]) for i in range(len(do) - 1)])
        worst = max(worst, float(np.abs(a - b).max()))
        top5_same += set(np.argsort(-a, kind="stable")[:5]) == set(np.argsort(-b, kind="stable")[:5])
    print(f"8-bit form, dim {dim}: float64 MaxSim moves by at most {worst:.3e} over {trials} seeds; top 5 of 11 unchanged in {top5_same}")
    assert worst <= 2.0 ** -4 + 2.0 ** -13
