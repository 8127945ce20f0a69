"""Plain Python / numpy restatement of Shamir sharing over GF(2^8) with the reference field
(reduction polynomial 0x11D, generator 2: src/crypto/Shamir.cpp:10-35), through exp / log tables.
Test infrastructure only: the tests use it where the compiled reference cannot reach (255 shares,
random bulk batches); tests/golden/shamir.json, made from the compiled reference, pins it
(tests/test_shamir_api.py::test_gf256_ref_matches_golden)."""
import numpy as np

POLY = 0x11D

EXP = np.zeros(512, dtype=np.uint8)
LOG = np.zeros(256, dtype=np.int32)
_x = 1
for _i in range(255):
    EXP[_i] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= POLY
EXP[255:510] = EXP[0:255]
EXP[510:] = EXP[0:2]


def mul(a, b):
    """Elementwise product of uint8 arrays (or ints), broadcasting."""
    a = np.asarray(a, dtype=np.uint8)
    b = np.asarray(b, dtype=np.uint8)
    r = EXP[LOG[a] + LOG[b]]
    return np.where((a == 0) | (b == 0), np.uint8(0), r).astype(np.uint8)


def inv(a):
    a = np.asarray(a, dtype=np.uint8)
    assert np.all(a != 0)
    return EXP[(255 - LOG[a]) % 255].astype(np.uint8)


def split(secrets, coeffs, share_count):
    """secrets uint8 [n,32], coeffs uint8 [n,t-1,32] -> shares uint8 [n,share_count,32]: share j is
    the polynomial secret + sum_d coeffs[d-1] x^d at x = j + 1 (evaluate_polynomial, :68-80)."""
    secrets = np.asarray(secrets, dtype=np.uint8)
    coeffs = np.asarray(coeffs, dtype=np.uint8).reshape(secrets.shape[0], -1, 32)
    n = secrets.shape[0]
    x = np.arange(1, share_count + 1, dtype=np.uint8)[None, :, None]
    power = np.ones((1, share_count, 1), dtype=np.uint8)
    out = np.repeat(secrets[:, None, :], share_count, axis=1)
    for d in range(coeffs.shape[1]):
        power = mul(power, x)
        out ^= mul(coeffs[:, d, None, :], power)
    return out


def combine(indices, values):
    """indices uint8 [n,t], values uint8 [n,t,32] -> (secrets uint8 [n,32], ok uint8 [n]): Lagrange
    interpolation at 0 (interpolate, :82-110); a record with two equal indices gives ok 0, zeros."""
    indices = np.asarray(indices, dtype=np.uint8)
    values = np.asarray(values, dtype=np.uint8)
    n, t = indices.shape
    out = np.zeros((n, 32), dtype=np.uint8)
    ok = np.ones(n, dtype=np.uint8)
    for r in range(n):
        xs = indices[r]
        if len(set(xs.tolist())) != t:
            ok[r] = 0
            continue
        for i in range(t):
            num, den = np.uint8(1), np.uint8(1)
            for j in range(t):
                if j != i:
                    num = mul(num, xs[j])
                    den = mul(den, xs[j] ^ xs[i])
            factor = mul(num, inv(den))
            out[r] ^= mul(values[r, i], factor)
    return out, ok


def solve_coefficients(xs, ys):
    """The polynomial through t points: xs uint8 [t] (distinct), ys uint8 [t,32] -> c uint8 [t,32]
    with ys[k] = sum_d c[d] xs[k]^d, by Gauss-Jordan elimination on the Vandermonde system."""
    t = len(xs)
    a = np.zeros((t, t), dtype=np.uint8)
    for k in range(t):
        p = np.uint8(1)
        for d in range(t):
            a[k, d] = p
            p = mul(p, np.uint8(xs[k]))
    y = np.array(ys, dtype=np.uint8).reshape(t, 32).copy()
    for col in range(t):
        piv = next(r for r in range(col, t) if a[r, col] != 0)
        if piv != col:
            a[[col, piv]] = a[[piv, col]]
            y[[col, piv]] = y[[piv, col]]
        f = inv(a[col, col])
        a[col] = mul(a[col], f)
        y[col] = mul(y[col], f)
        for r in range(t):
            if r != col and a[r, col] != 0:
                g = a[r, col]
                a[r] ^= mul(a[col], g)
                y[r] ^= mul(y[col], g)
    return y
