"""Exact-integer reference for the K12 tests (tests/test_marlin_sumcheck2_host.py, tests/test_gpu_marlin_sumcheck2.py): the pointwise
core q = a - b f of the second sumcheck and the driver's chain -- f on K, its interpolation and split, a and b on B from the
B-evaluations of the interpolated row / col / row_col / val, their interpolation, b f_poly as a polynomial product, the division by
X^|K| - 1 -- every value by its formula in include/pcdhip.h, on top of tests/marlin_reference.py and tests/marlin_round1_reference.py.
Domain elements are an ARGUMENT everywhere.  `interp` (evaluations, domain -> coefficients) and `extend` (coefficients, domain ->
evaluations) are the transforms a caller wants used: the quadratic ones by default, the oracle's where sizes ask for it."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kzg_reference import horner  # noqa: E402
from marlin_reference import interpolate, sumcheck_ab, sumcheck_f  # noqa: E402
from marlin_round1_reference import poly_add, poly_mul  # noqa: E402
from poly_algebra_reference import div_vanishing  # noqa: E402


def sumcheck2_q(alpha, beta, coeff, row, col, row_col, val, f, p):
    """q_i = a_i - b_i f_i, a and b those of marlin_reference.sumcheck_ab (row_col: three vectors or None)"""
    a, b = sumcheck_ab(alpha, beta, coeff, row, col, row_col, val, p)
    return [(x - y * z) % p for x, y, z in zip(a, b, f)]


def evaluate(coeffs, dom, p):
    """the polynomial's values on `dom` by Horner (quadratic: small sizes)"""
    return [horner(coeffs, x, p) for x in dom]


def sumcheck2(alpha, beta, coeff, on_k, dom_k, dom_b, p, interp=interpolate, extend=evaluate):
    """on_k = (row, col, row_col, val), each the three matrices' vectors on K as the index holds them -> dict of
    f_evals (f on K), f_poly (|K| coefficients), sigma, g2 (|K| - 1), polys (the twelve coefficient vectors, [poly][matrix]),
    a_poly, b_poly (3 |K| - 2 coefficients each), q (4 |K| - 3), h2 (3 |K| - 3, not trimmed), rem (|K|)"""
    k_n, b_n = len(dom_k), len(dom_b)
    assert b_n >= 3 * k_n - 2
    f_evals = sumcheck_f(alpha, beta, coeff, *on_k, p)
    f_poly = interp(f_evals, dom_k, p)
    polys = [[interp(v, dom_k, p) for v in vecs] for vecs in on_k]
    on_b = [[extend(c, dom_b, p) for c in vecs] for vecs in polys]
    a_evals, b_evals = sumcheck_ab(alpha, beta, coeff, *on_b, p)
    a_poly, b_poly = interp(a_evals, dom_b, p), interp(b_evals, dom_b, p)
    ab_len = 3 * k_n - 2
    assert not any(a_poly[ab_len:]) and not any(b_poly[ab_len:])  # both are of degree <= 3 |K| - 3
    a_poly, b_poly = a_poly[:ab_len], b_poly[:ab_len]
    q = poly_add(a_poly, poly_mul(b_poly, f_poly, p), p, scale=p - 1)
    assert len(q) == 4 * k_n - 3
    h2, rem = div_vanishing(q, k_n, p)
    return {"f_evals": f_evals, "f_poly": f_poly, "sigma": f_poly[0], "g2": f_poly[1:], "polys": polys, "a_poly": a_poly, "b_poly": b_poly,
            "q": q, "h2": h2, "rem": rem}


def ab_at(alpha, beta, coeff, polys, z, p):
    """a(z) and b(z) from the definition over the twelve coefficient vectors ([poly][matrix]): the formulas of sumcheck_ab at the one
    point z, every polynomial by Horner"""
    at = [[[horner(c, z, p)] for c in vecs] for vecs in polys]
    a, b = sumcheck_ab(alpha, beta, coeff, *at, p)
    return a[0], b[0]
