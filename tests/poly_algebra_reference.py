"""Exact-integer reference for the K8 tests (tests/test_poly_algebra_host.py, tests/test_gpu_poly_algebra.py): batch inversion,
division by the vanishing polynomial X^n - 1 and the schoolbook polynomial product, over the moduli of tests/kzg_reference.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kzg_reference import LIMBS, MODULI, horner, ints_of_limbs, limbs_of_ints, to_ints, to_mont  # noqa: E402,F401


def batch_inverse(xs, p, scale=1):
    """ark-ff batch_inversion_and_mul: scale / x for x != 0, zeros left zero -- Montgomery's trick with one pow(x, -1, p)"""
    pre, run = [], 1
    for x in xs:
        pre.append(run)
        if x % p:
            run = run * x % p
    inv = pow(run, -1, p) * scale % p
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        if xs[i] % p:
            out[i] = inv * pre[i] % p
            inv = inv * xs[i] % p
    return out


def div_vanishing(coeffs, n, p):
    """the unique (q, r) with coeffs = q (X^n - 1) + r, deg r < n: q_j = c_(j+n) + q_(j+n), r_j = c_j + q_j"""
    ln = len(coeffs)
    q = [0] * max(ln - n, 0)
    for j in range(len(q) - 1, -1, -1):
        q[j] = (coeffs[j + n] + (q[j + n] if j + n < len(q) else 0)) % p
    r = [(coeffs[j] + (q[j] if j < len(q) else 0)) % p for j in range(min(ln, n))]
    return q, r


def mul_schoolbook(a, b, p):
    """len(a) + len(b) - 1 coefficients, not trimmed; empty when an operand is"""
    if not a or not b:
        return []
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] += x * y
    return [c % p for c in out]
