"""Numpy reference of the token-vector store's 8-bit form (RAG_TOKVEC_MXFP8, include/rag_hip.h; tests/test_tokvec_q8_*.py).

The reference IS the contract: a row of `dim` components is dim / 32 blocks of 32 consecutive components; for a block with
amax = max |x| the scale exponent e is the smallest integer with amax <= 448 * 2^e, clamped to [-15, 7] (e = -15 for an all-zero
block) and stored as the E8M0 byte e + 127; a component is stored as E4M3 "FN" (max 448, no infinities) of x * 2^-e, rounded to
nearest even with subnormals kept, magnitudes above 448 saturating to 448, the sign - of zero too - kept; the stored value is
code * 2^e. Everything is float64 arithmetic on exactly representable numbers (power-of-two scalings, np.rint on a multiple of
the grid step): no rounding happens but the one the contract names. Nothing here touches the GPU or the package under test."""
import numpy as np

import tokvec_tools as V

E_MIN, E_MAX, BLOCK = -15, 7, 32
BAR_B = 2.0 ** -4 + 2.0 ** -13 + 1e-4        # a dot of unit rows moves by <= 2^-4 + sqrt(dim) 2^-18 <= 2^-4 + 2^-13; + the kernel's 1e-4


def block_exponents(x):
    """int [rows, dim / 32]: the smallest e with amax <= 448 * 2^e = 0.875 * 2^(e + 9), clamped"""
    x = np.asarray(x, dtype=np.float32)
    amax = np.abs(x.reshape(x.shape[0], -1, BLOCK)).max(axis=2).astype(np.float64)
    m, ex = np.frexp(amax)                                           # amax = m * 2^ex, m in [0.5, 1)
    e = ex - 9 + (m > 0.875)
    return np.clip(np.where(amax == 0, E_MIN, e), E_MIN, E_MAX).astype(np.int64)


def quantise(x):
    """float32 [rows, dim] -> (codes uint8 [rows, dim], scale bytes uint8 [rows, dim / 32], stored values float32 [rows, dim])"""
    x = np.asarray(x, dtype=np.float32)
    rows, dim = x.shape
    assert dim % BLOCK == 0
    e = block_exponents(x)
    scale = np.repeat(np.ldexp(1.0, e), BLOCK, axis=1)               # 2^e per component, float64
    a = np.minimum(np.abs(x.astype(np.float64)) / scale, 448.0)
    _, ex = np.frexp(a)                                              # floor(log2 a) = ex - 1
    step = np.ldexp(1.0, np.maximum(ex - 1, -6) - 3)                 # 3 mantissa bits; below 2^-6 the subnormal step 2^-9
    q = np.rint(a / step) * step                                     # ties to even
    neg = np.signbit(x)
    m, ex = np.frexp(q)
    normal = q >= 2.0 ** -6
    code = np.where(normal, ((ex - 1 + 7) << 3) + np.rint((2 * m - 1) * 8).astype(np.int64), np.rint(q * 512).astype(np.int64))
    code = (code | np.where(neg, 0x80, 0)).astype(np.uint8)
    vals = np.where(neg, -q, q) * scale
    return code, (e + 127).astype(np.uint8), vals.astype(np.float32)


def stored(x):
    """what rag_tokvec_fetch_host returns for rows appended as x"""
    return quantise(x)[2]


def decode(code, scale_bytes):
    """code * 2^e from the stored bytes alone, as float32 (an independent reading of the encoding)"""
    c = code.astype(np.int64)
    ex, man = (c >> 3) & 15, c & 7
    mag = np.where(ex > 0, np.ldexp(8.0 + man, ex - 10), np.ldexp(man.astype(np.float64), -9))
    e = np.repeat(scale_bytes.astype(np.int64) - 127, BLOCK, axis=1)
    return (np.where(c & 0x80, -mag, mag) * np.ldexp(1.0, e)).astype(np.float32)


def edge_rows(dim):
    """float32 [n, dim] of the contract's edge blocks, the rest of every row filled with small seeded values"""
    rng = np.random.default_rng(77)
    f32 = np.float32
    heads = [
        [0.0] * 8,                                                   # an all-zero block (the whole first block is zeroed below)
        [0.0, -0.0, 1.0, -1.0, 0.5, -0.0, 0.0, 0.25],               # signed zeros beside values
        [448.0 * 2.0 ** -3, 1e-3, -1e-3],                            # amax exactly 448 * 2^e ...
        [np.nextafter(f32(448.0 * 2.0 ** -3), f32(np.inf)), 1e-3],   # ... and one float32 ulp above it: the next exponent
        [448.0 * 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -25],     # the lower clamp: fp16's subnormal step
        [448.0 * 2.0 ** -16, 1e-6, -1e-6, 2.0 ** -24],               # amax below 448 * 2^-15
        [1e-6, -1e-6, 1e-7],                                         # a block of 1e-6
        [65504.0, -65504.0, 57344.0, 60000.0, -60000.0, 1.0, 200.0], # the upper clamp: saturate to 448 * 2^7 = 57344
        [65519.0, -65519.0, 50000.0, 128.0 * 2.0 ** -9 * 0.5],       # the largest accepted magnitude; a tie at the clamp's subnormal step
        # halfway cases on the E4M3 grid at e = -8 (amax 1.75 = 448 * 2^-8): ties to even, normal and subnormal
        [1.75, 1.0 + 1 / 16, 1.0 + 3 / 16, 1.0 + 5 / 16, -(1.0 + 7 / 16), 2.0 ** -8 * 2.0 ** -6 * (1 + 1 / 16),
         2.0 ** -8 * 2.0 ** -10, 2.0 ** -8 * 3 * 2.0 ** -10, -(2.0 ** -8) * 5 * 2.0 ** -10, 2.0 ** -8 * 15 * 2.0 ** -10],
    ]
    out = np.zeros((len(heads), dim), dtype=np.float32)
    for r, h in enumerate(heads):
        amax = max(abs(float(v)) for v in h)
        out[r] = (rng.uniform(-0.5, 0.5, dim) * amax).astype(np.float32)     # every block's amax is the head's
        out[r, :len(h)] = np.array(h, dtype=np.float32)
    out[0, :BLOCK] = 0.0
    return out


def planted_case(seed, dim, d_rows=(1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257), q_rows=33):
    """seeded unit rows with a planted query component: every document holds noisy copies of some query rows, of a strength that
    falls from document to document, so that the documents' MaxSim scores are spread out -> (q, q_off, d, d_off)"""
    import m3_tools as M
    rng = np.random.default_rng(seed)
    q = V.unit_rows(rng, q_rows, dim)
    docs = []
    for i, n in enumerate(d_rows):
        noise = rng.standard_normal((n, dim)) / np.sqrt(dim)
        plant = q[rng.integers(0, q_rows, n)] * (0.9 - 0.07 * i)
        v = plant + noise
        docs.append((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))
    d, d_off = M.pack(docs, dim)
    return q, np.array([0, q_rows], dtype=np.int64), d, d_off
