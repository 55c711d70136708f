"""Exact-integer reference for the K11 tests (tests/test_marlin_round1_host.py, tests/test_gpu_marlin_round1.py): the assignment on H at
`reindex_by_subdomain`'s places, z_M = M z, the hiding multiples of the vanishing polynomial, w with its remainder, the pointwise
core q of the first sumcheck and h_1 / g_1 by schoolbook division -- every value by its formula in include/pcdhip.h, over the moduli
of tests/kzg_reference.py.  Domain elements are an ARGUMENT everywhere, as in tests/marlin_reference.py: the tests take them from the
oracle's transform of the unit vector, never from the library.  `interp` is the interpolation a caller wants used (evaluations on a
domain -> coefficients): the quadratic one of marlin_reference by default, the oracle's inverse transform where sizes ask for it."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kzg_reference import LIMBS, MODULI, horner, to_ints, to_mont  # noqa: E402,F401
from marlin_reference import bivariate_lagrange, domain_elements, interpolate, reindex, t_evals  # noqa: E402,F401
from poly_algebra_reference import div_vanishing, mul_schoolbook  # noqa: E402,F401


def place(z, h_n, x_n, num_cols=None):
    """z on H at pi's places by the header's formula for k (NOT through reindex: the host test checks the two against each other)"""
    num_cols = len(z) if num_cols is None else num_cols
    period = h_n // x_n
    out = []
    for k in range(h_n):
        c = k // period if k % period == 0 else x_n + (k - k // period - 1)
        out.append(z[c] if c < num_cols else 0)
    return out


def zm_evals(entries, z, h_n, p):
    """out[r] = sum_{(r, c, v)} v z[c], zeros up to h_n; duplicates accumulate"""
    out = [0] * h_n
    for r, c, v in entries:
        out[r] = (out[r] + v * z[c]) % p
    return out


def add_vanishing_multiple(coeffs, blind, n, p):
    """coeffs + blind(X) (X^n - 1), max(len, n + k) coefficients; k == 0 leaves coeffs as they are"""
    if not blind:
        return list(coeffs)
    out = list(coeffs) + [0] * max(n + len(blind) - len(coeffs), 0)
    for i, b in enumerate(blind):
        out[i] = (out[i] - b) % p
        out[n + i] = (out[n + i] + b) % p
    return out


def poly_mul(a, b, p):
    """the schoolbook product's coefficients through ONE product of Python integers (Kronecker substitution: every coefficient in a
    slot wide enough for min(len) products below p^2), exact; tests/test_marlin_round1_host.py checks it against mul_schoolbook"""
    if not a or not b:
        return []
    slot = 2 * p.bit_length() + min(len(a), len(b)).bit_length() + 1
    pack = lambda v: int.from_bytes(b"".join(x.to_bytes(slot // 8 + 1, "little") for x in v), "little")
    width = (slot // 8 + 1) * 8
    prod = pack(a) * pack(b)
    raw = prod.to_bytes((len(a) + len(b)) * (width // 8), "little")
    return [int.from_bytes(raw[i * (width // 8):(i + 1) * (width // 8)], "little") % p for i in range(len(a) + len(b) - 1)]


def poly_add(a, b, p, scale=1):
    out = list(a) + [0] * max(len(b) - len(a), 0)
    for i, x in enumerate(b):
        out[i] = (out[i] + scale * x) % p
    return out


def round1(mats, z, h_n, x_n, dom_h, dom_x, blinds, p, interp=interpolate):
    """mats: A, B (, C) as lists of (r, c, v); z: the assignment; blinds: (b_w, b_a, b_b) lists of coefficients -> dict of x_hat, z_poly,
    w, w_rem, za_poly, zb_poly (coefficients) and za_evals, zb_evals (on H)"""
    b_w, b_a, b_b = blinds
    x_hat = interp((list(z[:x_n]) + [0] * x_n)[:x_n], dom_x, p)
    z_poly = add_vanishing_multiple(interp(place(z, h_n, x_n), dom_h, p), b_w, h_n, p)
    w, w_rem = div_vanishing(poly_add(z_poly, x_hat, p, scale=p - 1), x_n, p)
    za_evals, zb_evals = zm_evals(mats[0], z, h_n, p), zm_evals(mats[1], z, h_n, p)
    return {"x_hat": x_hat, "z_poly": z_poly, "w": w, "w_rem": w_rem, "za_evals": za_evals, "zb_evals": zb_evals,
            "za_poly": add_vanishing_multiple(interp(za_evals, dom_h, p), b_a, h_n, p),
            "zb_poly": add_vanishing_multiple(interp(zb_evals, dom_h, p), b_b, h_n, p)}


def sumcheck1_q(eta, za, zb, r, t, z, p):
    """q_i = r_i (eta_A za_i + eta_B zb_i + eta_C za_i zb_i) - t_i z_i"""
    return [(r[i] * (eta[0] * za[i] + eta[1] * zb[i] + eta[2] * za[i] * zb[i]) - t[i] * z[i]) % p for i in range(len(za))]


def q1_length(h_n, len_za, len_zb, len_z, len_mask=0):
    """the length pcdhip_marlin_sumcheck1 gives q_1: the bound of its three terms, not the trimmed degree"""
    return max(h_n + len_za + len_zb - 2, h_n + len_z - 1, len_mask)


def sumcheck1(mats, eta, alpha, za_poly, zb_poly, z_poly, mask, h_n, x_n, dom_h, p, interp=interpolate):
    """q_1 = s + r (eta_A z_A + eta_B z_B + eta_C z_A z_B) - t z over the coefficients, divided by X^h_n - 1 by the schoolbook
    recurrence -> dict of t_poly, h1 (q_1's length less h_n coefficients), g1, sigma (the remainder's constant term), q1"""
    r_evals = bivariate_lagrange(alpha, dom_h, p)
    r_poly = interp(r_evals, dom_h, p)
    t_poly = interp(t_evals(mats, eta, r_evals, h_n, x_n, p), dom_h, p)
    inner = poly_add([eta[0] * x % p for x in za_poly], zb_poly, p, scale=eta[1])
    inner = poly_add(inner, poly_mul(za_poly, zb_poly, p), p, scale=eta[2])
    q1 = poly_add(poly_mul(r_poly, inner, p), poly_mul(t_poly, z_poly, p), p, scale=p - 1)
    q1 = poly_add(q1, mask or [], p)
    n = q1_length(h_n, len(za_poly), len(zb_poly), len(z_poly), len(mask or []))
    assert len(q1) <= n
    q1 += [0] * (n - len(q1))
    h1, rem = div_vanishing(q1, h_n, p)
    return {"t_poly": t_poly, "h1": h1, "g1": rem[1:], "sigma": rem[0], "q1": q1, "r_poly": r_poly}


def r_alpha_at(alpha, beta, n, p):
    """r(alpha, beta) = (alpha^n - beta^n) / (alpha - beta), alpha != beta"""
    return (pow(alpha, n, p) - pow(beta, n, p)) * pow(alpha - beta, -1, p) % p


def verifier_equation_holds(eta, alpha, beta, polys, sc, mask, h_n, p):
    """s(beta) + r(alpha, beta) (eta_A z_A(beta) + eta_B z_B(beta) + eta_C z_A(beta) z_B(beta)) - t(beta) z(beta)
       = h_1(beta) v_H(beta) + beta g_1(beta) + sigma      (sigma = 0 for a satisfied system and a mask that sums to zero on H)
    polys: dict with za_poly, zb_poly, z_poly; sc: dict with t_poly, h1, g1, sigma"""
    at = lambda c: horner(c, beta, p)
    za, zb = at(polys["za_poly"]), at(polys["zb_poly"])
    lhs = (at(mask or []) + r_alpha_at(alpha, beta, h_n, p) * (eta[0] * za + eta[1] * zb + eta[2] * za * zb) - at(sc["t_poly"]) * at(polys["z_poly"])) % p
    rhs = (at(sc["h1"]) * (pow(beta, h_n, p) - 1) + beta * at(sc["g1"]) + sc["sigma"]) % p
    return lhs == rhs


def satisfied_system(rnd, p, rows, cols, x_n, entries_per_row=3):
    """random A, B and z with every z[c] != 0, and C with ONE entry per row, (r, c, (A z)_r (B z)_r / z[c]): A z o B z = C z"""
    z = [rnd.randrange(1, p) for _ in range(cols)]
    a = [(r, rnd.randrange(cols), rnd.choice([1, p - 1, 2, rnd.randrange(p)])) for r in range(rows) for _ in range(rnd.randrange(1, entries_per_row + 1))]
    b = [(r, rnd.randrange(cols), rnd.choice([1, p - 1, 3, rnd.randrange(p)])) for r in range(rows) for _ in range(rnd.randrange(1, entries_per_row + 1))]
    az, bz = zm_evals(a, z, rows, p), zm_evals(b, z, rows, p)
    c = []
    for r in range(rows):
        col = rnd.randrange(cols)
        c.append((r, col, az[r] * bz[r] % p * pow(z[col], -1, p) % p))
    return [a, b, c], z


def zero_sum_mask(rnd, p, h_n, length, dom_h=None):
    """a random polynomial of `length` coefficients whose sum over H is zero: sum_H X^j = |H| for j a multiple of |H| and 0 otherwise, so
    the coefficients at 0, |H|, 2 |H|, ... must cancel"""
    s = [rnd.randrange(p) for _ in range(length)]
    s[0] = (-sum(s[j] for j in range(h_n, length, h_n))) % p
    return s
