"""Integer reference for the K14 tests (tests/test_kzg_check_host.py, tests/test_gpu_kzg_check.py), independent of the library: the
column scalars of the MarlinKZG10 check for both modes, and its verdict on a setup that keeps its trapdoor
(kzg_commit_reference.Srs) -- every point is then a known multiple of g, and an equation e(L, h) == e(R, beta_h) is L = beta R (mod r)
in integers (the technique of tests/verify_reference.py and tests/dlog_reference.py).

The check's vector, N = 2 + n_shift + 2 m + P points:
    [0] g   [1] gamma_g   [2 + k] S_k   [2 + n_shift + i] comm_i   [2 + n_shift + m + i] shifted_i   [2 + n_shift + 2 m + o] W_o
Tables are lists of Python integers: a, s, item_values P x m (s and item_values may be None), points, values, random_v (may be None) of
P entries, shift_index of m entries (-1: no degree bound), randomizers P entries or None for per-opening mode."""


def randomizer_rows(P, randomizers):
    """the E x P matrix of a mode: the caller's row, or the identity"""
    if randomizers is not None:
        return [list(randomizers)]
    return [[1 if o == e else 0 for o in range(P)] for e in range(P)]


def collapse(p, n_shift, shift_index, points, a, s, values, random_v, item_values, randomizers):
    """-> (left: E rows of N column scalars, right: E rows of P), every entry in [0, p)"""
    P = len(points)
    m = len(a[0]) if P else 0
    left, right = [], []
    for rho in randomizer_rows(P, randomizers):
        g = -sum(rho[o] * values[o] for o in range(P))
        gg = -sum(rho[o] * random_v[o] for o in range(P)) if random_v is not None else 0
        sk = [0] * n_shift
        if s is not None:
            for o in range(P):
                for i in range(m):
                    if s[o][i] % p:
                        assert 0 <= shift_index[i] < n_shift, "s != 0 on an item without a shift power"
                        sk[shift_index[i]] -= rho[o] * s[o][i] * item_values[o][i]
        comm = [sum(rho[o] * a[o][i] for o in range(P)) for i in range(m)]
        shifted = [sum(rho[o] * s[o][i] for o in range(P)) if s is not None else 0 for i in range(m)]
        w = [rho[o] * points[o] for o in range(P)]
        left.append([x % p for x in [g, gg] + sk + comm + shifted + w])
        right.append([x % p for x in rho])
    return left, right


def vector_exponents(srs, shift_exps, comm_exps, shifted_exps, w_exps):
    """the discrete logarithms of the check's vector to the base g (the identity is 0); shifted_exps may be None"""
    m = len(comm_exps)
    return [1, srs.gamma] + list(shift_exps) + list(comm_exps) + list(shifted_exps if shifted_exps is not None else [0] * m) + list(w_exps)


def verdict(srs, shift_exps, comm_exps, shifted_exps, w_exps, shift_index, points, a, s, values, random_v, item_values, randomizers):
    """-> one bool per equation: sum_c left_c x_c == beta sum_o right_o w_o (mod r)"""
    p = srs.p
    left, right = collapse(p, len(shift_exps), shift_index, points, a, s, values, random_v, item_values, randomizers)
    x = vector_exponents(srs, shift_exps, comm_exps, shifted_exps, w_exps)
    out = []
    for lrow, rrow in zip(left, right):
        assert len(lrow) == len(x)
        lhs = sum(c * e for c, e in zip(lrow, x)) % p
        rhs = srs.beta * sum(c * e for c, e in zip(rrow, w_exps)) % p
        out.append(lhs == rhs)
    return out


def combined_exponent(srs, shift_exps, comm_exps, shifted_exps, shift_index, a_row, s_row, item_values_row):
    """the exponent of C_o = sum_i a_i comm_i + sum_i s_i (shifted_i - v_i S_k(i))"""
    p = srs.p
    c = sum(ai * ci for ai, ci in zip(a_row, comm_exps))
    if s_row is not None:
        for i, si in enumerate(s_row):
            if si % p:
                c += si * (shifted_exps[i] - item_values_row[i] * shift_exps[shift_index[i]])
    return c % p


def solve_witness(srs, c, value, random_v, z):
    """The exponent w of the witness that opens ANY commitment exponent c at z to ANY value: c - v - gamma rv + z w = beta w.
    z == beta has no solution unless the numerator is zero (then every w serves; 0 is returned)."""
    p = srs.p
    num = (c - value - srs.gamma * random_v) % p
    den = (srs.beta - z) % p
    if den == 0:
        assert num == 0
        return 0
    return num * pow(den, -1, p) % p
