"""Exact-integer reference for the K9 tests (tests/test_marlin_rounds_host.py, tests/test_gpu_marlin_rounds.py): r(alpha, .) on H, the
column re-indexing of `reindex_by_subdomain`, t on H as a transposed sparse mat-vec, and the rational sumcheck's a, b and f -- every
value by its formula in include/pcdhip.h, over the moduli of tests/kzg_reference.py.  Domain elements are an ARGUMENT everywhere (a list
of the powers of the domain's generator): the tests take them from the oracle's transform of the unit vector, never from the library."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kzg_reference import LIMBS, MODULI, horner, ints_of_limbs, limbs_of_ints, to_ints, to_mont  # noqa: E402,F401
from poly_algebra_reference import batch_inverse  # noqa: E402


def domain_elements(co, field, n, m=1):
    """[w^i for i < n] of the domain of n = m * 2^a elements: the oracle's forward transform of the unit vector e_1"""
    if n == 1:
        return [1]
    e1 = to_mont(co, field, [0, 1] + [0] * (n - 2))
    out = co.fft(field, e1) if m == 1 else co.fft_general(field, e1, m)
    return to_ints(co, field, out)


def bivariate_lagrange(x, dom, p):
    """(x^n - 1) / (x - w^i) for the w^i of `dom`; all zero when x is one of them (batch_inversion leaves the zero, the scale is zero)"""
    vh = (pow(x, len(dom), p) - 1) % p
    return batch_inverse([(x - w) % p for w in dom], p, vh)


def reindex(c, h_n, x_n):
    """ark-marlin reindex_by_subdomain: the place in H (|H| = h_n) of variable c, the first x_n variables on the subdomain X"""
    period = h_n // x_n
    if c < x_n:
        return c * period
    i = c - x_n
    return i + i // (period - 1) + 1


def t_evals(mats, eta, r_alpha, h_n, x_n, p):
    """t[j] = sum_M eta_M sum_{(r, c, v) in M, pi(c) = j} v r_alpha[r]; mats: three lists of (r, c, v) entries, duplicates accumulate"""
    t = [0] * h_n
    for e, entries in zip(eta, mats):
        for r, c, v in entries:
            j = reindex(c, h_n, x_n)
            t[j] = (t[j] + e * v * r_alpha[r]) % p
    return t


def sumcheck_d(alpha, beta, row, col, row_col, p):
    """d per element: the four-term form with row_col as given, or (beta - row)(alpha - col) when row_col is None"""
    if row_col is None:
        return [(beta - r) * (alpha - c) % p for r, c in zip(row, col)]
    return [(alpha * beta - alpha * r - beta * c + rc) % p for r, c, rc in zip(row, col, row_col)]


def sumcheck_ab(alpha, beta, coeff, row, col, row_col, val, p):
    """row, col, val: three vectors each; row_col: three vectors or None -> (a, b)"""
    d = [sumcheck_d(alpha, beta, row[m], col[m], None if row_col is None else row_col[m], p) for m in range(3)]
    n = len(row[0])
    b = [d[0][i] * d[1][i] * d[2][i] % p for i in range(n)]
    a = [(coeff[0] * val[0][i] * d[1][i] * d[2][i] + coeff[1] * val[1][i] * d[0][i] * d[2][i] + coeff[2] * val[2][i] * d[0][i] * d[1][i]) % p
         for i in range(n)]
    return a, b


def sumcheck_f(alpha, beta, coeff, row, col, row_col, val, p):
    """f_i = a_i / b_i, 0 where b_i = 0"""
    a, b = sumcheck_ab(alpha, beta, coeff, row, col, row_col, val, p)
    return [x * y % p for x, y in zip(a, batch_inverse(b, p))]


def arithmetize(entries, dom_h, h_n, x_n, k_n, p):
    """the index's evaluations on K of one matrix: row = w^pi(c), col = w^r, val = v w^pi(c) / |H| for entry (r, c, v), K padded
    with val = 0 (and row = col = 1)"""
    assert len(entries) <= k_n
    hinv = pow(h_n, -1, p)
    row, col, val = [1] * k_n, [1] * k_n, [0] * k_n
    for k, (r, c, v) in enumerate(entries):
        w = dom_h[reindex(c, h_n, x_n)]
        row[k], col[k], val[k] = w, dom_h[r], v * w % p * hinv % p
    return row, col, val


def interpolate(evals, dom, p):
    """coefficients of the polynomial of degree < n with these values on `dom` (n <= a few hundred: the quadratic inverse transform)"""
    n = len(dom)
    ninv = pow(n, -1, p)
    return [sum(evals[i] * dom[(-i * j) % n] for i in range(n)) % p * ninv % p for j in range(n)]
