"""Exact-integer reference for Groth16 key generation (tests/test_setup_reference_host.py, tests/test_gpu_setup_edges.py): the scalars
of every query of `pcdhip_groth16_setup` by their formulas in Python integers mod r, over the moduli of tests/kzg_reference.py, and the
case lists both test files run.  With Z(tau) = tau^n - 1 and w the generator of the domain of n elements:

  u_j = Z(tau) w^j / (n (tau - w^j))                           (one batch inversion)
  a_i = sum_j A[j][i] u_j  (+ u_(nc+i) for i < ni)      b_i, c_i likewise from B, C, without the extra term
  gamma_abc_i = (beta a_i + alpha b_i + c_i) / gamma  (i < ni)           l_i = (beta a_i + alpha b_i + c_i) / delta  (i >= ni)
  h_i = tau^i Z(tau) / delta  (i < n - 1)                      and the six single scalars alpha, beta, delta | beta, gamma, delta

A matrix is a list of (row, column, value) entries in which duplicates accumulate.  Domain elements are an ARGUMENT (marlin_reference.
domain_elements: the oracle's forward transform of e_1, mixed radix included), so the reference uses the w of the transforms.  The
expected points are fixed-base multiples of the group generators (co.fixed_base_mul, pinned against double-and-add elsewhere); a scalar
0 is a flagged identity with zero coordinates.  Nothing here goes through a setup routine of either oracle."""
import collections
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kzg_reference import LIMBS, MODULI, limbs_of_ints, to_mont  # noqa: E402
from marlin_reference import domain_elements  # noqa: E402
from poly_algebra_reference import batch_inverse  # noqa: E402

CURVE_FR = [1, 0, 3, 2]   # scalar field of curve cid
LONG_ROW = 16             # a transposed row of more entries than this is a wave's (common.h SPMV_LONG_ROW)
FLUSH = 48                # small coefficients a lane sums before it reduces (inst_field.hip SPMV_FLUSH)
SMALL = 32                # |c| <= 32 is a small-integer coefficient (capi_witness.hip SmallCoeffTable)

POINTS = (("alpha_g1", 1), ("beta_g1", 1), ("delta_g1", 1), ("beta_g2", 2), ("gamma_g2", 2), ("delta_g2", 2))
QUERIES = (("a_query", 1, "a_inf"), ("b_g1_query", 1, "b_g1_inf"), ("b_g2_query", 2, "b_g2_inf"), ("h_query", 1, "h_inf"),
           ("l_query", 1, "l_inf"), ("gamma_abc_g1", 1, "gamma_abc_inf"))


# ------------------------------------------------------------------------------------------------------------------ the scalars
def lagrange_at(tau, dom, p):
    """[u_j for j < n]; ValueError when tau is a domain element (the library's PCDHIP_E_ARG)"""
    n = len(dom)
    den = [(tau - w) % p for w in dom]
    if 0 in den:
        raise ValueError("tau lies in the evaluation domain")
    scale = (pow(tau, n, p) - 1) * pow(n, -1, p) % p
    return [w * d % p for w, d in zip(dom, batch_inverse(den, p, scale))]


def transposed(entries, u, m, p):
    """[sum_j M[j][i] u_j for i < m]"""
    out = [0] * m
    for r, c, v in entries:
        out[c] = (out[c] + v * u[r]) % p
    return out


def key_scalars(mats, nc, m, ni, toxic, dom, p):
    """{field of the key: scalar or list of scalars}, every value reduced mod p"""
    alpha, beta, gamma, delta, tau = toxic
    n = len(dom)
    assert 1 <= ni <= m and nc + ni <= n and all(0 <= t < p for t in toxic) and alpha and beta and gamma and delta
    assert all(0 <= r < nc and 0 <= c < m and 0 <= v < p for e in mats for r, c, v in e)
    u = lagrange_at(tau, dom, p)
    a, b, c = (transposed(e, u, m, p) for e in mats)
    for i in range(ni):
        a[i] = (a[i] + u[nc + i]) % p
    dinv, ginv = pow(delta, -1, p), pow(gamma, -1, p)
    mix = [(beta * a[i] + alpha * b[i] + c[i]) % p for i in range(m)]
    h, cur = [], (pow(tau, n, p) - 1) * dinv % p
    for _ in range(n - 1):
        h.append(cur)
        cur = cur * tau % p
    return dict(alpha_g1=alpha, beta_g1=beta, delta_g1=delta, beta_g2=beta, gamma_g2=gamma, delta_g2=delta, a_query=a, b_g1_query=b,
                b_g2_query=list(b), h_query=h, l_query=[mix[i] * dinv % p for i in range(ni, m)],
                gamma_abc_g1=[mix[i] * ginv % p for i in range(ni)])


# ------------------------------------------------------------------------------------------------------------------- the points
def multiples(co, cid, group, ks, nthreads=8):
    """k G for the group's generator -> (affine points, flags); flag = (k == 0), a flagged point has zero coordinates"""
    if not len(ks):
        return np.zeros((0, co.point_words(cid, group)), dtype=np.uint64), np.zeros(0, dtype=np.uint8)
    words = limbs_of_ints(ks, LIMBS[CURVE_FR[cid]])
    xy, inf = co.fixed_base_mul(cid, group, co.generator(cid, group), words, nthreads=nthreads)
    assert np.array_equal(inf != 0, np.array([k == 0 for k in ks]))
    xy[inf != 0] = 0
    return xy, inf


def expected_key(co, cid, scalars, h_sample=None):
    """{name: array} of every point and flag array of the key.  h_sample: indices of h_query whose points are wanted (all when None);
    then h_query holds those rows only, h_inf is complete all the same (a flag is scalar == 0)"""
    K = {}
    for group in (1, 2):   # one fixed-base batch per group: the batch's table is made once
        parts = [(name, [scalars[name]]) for name, grp in POINTS if grp == group]
        for name, grp, _ in QUERIES:
            if grp == group:
                ks = scalars[name]
                parts.append((name, [ks[i] for i in h_sample] if name == "h_query" and h_sample is not None else ks))
        xy, inf = multiples(co, cid, group, [k for _, ks in parts for k in ks])
        at = 0
        for name, ks in parts:
            K[name], K[name + "/inf"] = np.ascontiguousarray(xy[at:at + len(ks)]), np.ascontiguousarray(inf[at:at + len(ks)])
            at += len(ks)
    for name, _ in POINTS:
        assert not K.pop(name + "/inf")[0]
        K[name] = K[name][0]
    for name, _, flags in QUERIES:
        K[flags] = K.pop(name + "/inf")
    if h_sample is not None:
        K["h_inf"] = np.array([k == 0 for k in scalars["h_query"]], dtype=np.uint8)
    return K


def assert_matches_oracle(arrays, keys, tag):
    """every point, query and flag of a co.Keys (the oracle's setup) against a {name: array} key with zero coordinates under its flags
    (the oracle leaves a flagged entry's coordinates as they come)"""
    for name, _ in POINTS:
        assert np.array_equal(getattr(keys, name), arrays[name]), (tag, name)
    for name, _, flags in QUERIES:
        got, inf = getattr(keys, name), getattr(keys, flags)
        assert got.shape == arrays[name].shape and np.array_equal(inf != 0, arrays[flags] != 0), (tag, flags)
        fin = arrays[flags] == 0
        assert np.array_equal(got[fin], arrays[name][fin]), (tag, name)


# ------------------------------------------------------------------------------------------------------------- the case lists
Case =collections.namedtuple("Case", "name cid nc ni m n dom_m mats toxic")   # n = dom_m * 2^a; mats: three entry lists; toxic: 5 ints


def csr_of(co, field, entries, rows):
    """entry list -> (row_ptr, col, coeff) in the C-ABI layout; the entries of a row keep their order, duplicates stay separate"""
    order = sorted(range(len(entries)), key=lambda k: entries[k][0])   # (stable)
    rp = np.zeros(rows + 1, dtype=np.uint64)
    if entries:
        rp[1:] = np.cumsum(np.bincount(np.array([e[0] for e in entries], dtype=np.int64), minlength=rows))
    col = np.array([entries[k][1] for k in order], dtype=np.uint32)
    return rp, col, to_mont(co, field, [entries[k][2] for k in order]).reshape(len(order), LIMBS[field])


def r1cs_of(co, case):
    """the case's constraint system as co.R1CS (what co.groth16_setup and the library's Python wrapper take); no assignment is needed"""
    field = CURVE_FR[case.cid]
    a, b, c = (csr_of(co, field, e, case.nc) for e in case.mats)
    r = co.R1CS(field, case.ni, *a, *b, *c, np.zeros((case.m, LIMBS[field]), dtype=np.uint64))
    assert r.num_constraints == case.nc and r.num_vars == case.m
    return r


def random_toxic(rnd, p):
    return tuple(rnd.randrange(1, p) for _ in range(5))


def toxic_mont(co, cid, toxic):
    return to_mont(co, CURVE_FR[cid], list(toxic))


TINY_SHAPES = [(0, 1, 1, 1), (1, 1, 2, 2), (2, 2, 4, 4), (5, 3, 6, 8), (6, 3, 7, 16), (13, 3, 9, 16)]   # nc, ni, m, n


def tiny_case(cid, shape):
    """random coefficients, one to three entries per row and matrix, random toxic waste"""
    nc, ni, m, n = shape
    p = MODULI[CURVE_FR[cid]]
    rnd = random.Random(f"setup/tiny/{cid}/{shape}")
    mats = [[(r, rnd.randrange(m), rnd.randrange(p)) for r in range(nc) for _ in range(rnd.randrange(1, 4))] for _ in range(3)]
    return Case(f"tiny{cid}_{nc}_{ni}_{m}", cid, nc, ni, m, n, 1, mats, random_toxic(rnd, p))


def is_small(v, p):
    return v <= SMALL or p - v <= SMALL


Planted = collections.namedtuple("Planted", "empty_vars v16 v17 v_long n_light v_special empty_row dup")


def planted_matrix(rnd, p, nc, m, n_light, v_long):
    """one matrix with everything the transposed mat-vec can meet, and where it is -> (entries, Planted).  Variable 1 and m - 2 have no
    entry; v16 / v17 exactly 16 / 17; v_long n_light small-integer entries (+-1, +-2, +-32) and then seven random ones; v_special the
    coefficients 0, 1, p - 1, 32, p - 32, 33, p - 33; one (row, column) twice; constraint row nc - 2 empty; the other variables a
    handful of random entries"""
    empty_vars, empty_row = (1, m - 2), nc - 2
    free = [v for v in range(m) if v not in empty_vars and v != v_long]
    v16, v17, v_special = free[0], free[1], free[2]
    rows = [r for r in range(nc) if r != empty_row]
    assert n_light + 7 <= len(rows) and len(free) >= 5
    entries = []
    for v, cnt in ((v16, LONG_ROW), (v17, LONG_ROW + 1)):
        entries += [(r, v, rnd.randrange(p)) for r in rnd.sample(rows, cnt)]
    where = rnd.sample(rows, n_light + 7)
    entries += [(r, v_long, rnd.choice([1, p - 1, 2, p - 2, 32, p - 32])) for r in where[:n_light]]
    entries += [(r, v_long, rnd.randrange(SMALL + 1, p - SMALL)) for r in where[n_light:]]
    entries += [(r, v_special, v) for r, v in zip(rnd.sample(rows, 7), [0, 1, p - 1, 32, p - 32, 33, p - 33])]
    for v in free[3:]:
        entries += [(r, v, rnd.randrange(p)) for r in rnd.sample(rows, rnd.randrange(1, 6))]
    r_dup = rnd.choice(rows)
    entries += [(r_dup, free[3], rnd.randrange(p)), (r_dup, free[3], rnd.randrange(p))]
    rnd.shuffle(entries)
    return entries, Planted(empty_vars, v16, v17, v_long, n_light, v_special, empty_row, (r_dup, free[3]))


def check_planted(entries, pl, nc, m, p):
    """the conditions of planted_matrix, recounted from the entry list alone"""
    per_var = collections.Counter(c for _, c, _ in entries)
    assert all(per_var[v] == 0 for v in pl.empty_vars)
    assert per_var[pl.v16] == LONG_ROW and per_var[pl.v17] == LONG_ROW + 1
    mine = [v for _, c, v in entries if c == pl.v_long]
    light = [v for v in mine if is_small(v, p)]
    assert len(light) == pl.n_light > FLUSH and len(mine) == pl.n_light + 7
    assert {min(v, p - v) for v in light} == {1, 2, 32} and {v > p // 2 for v in light} == {False, True}
    assert {v for _, c, v in entries if c == pl.v_special} == {0, 1, p - 1, 32, p - 32, 33, p - 33}
    assert all(r != pl.empty_row for r, _, _ in entries)
    assert sum(1 for r, c, _ in entries if (r, c) == pl.dup) >= 2
    assert all(0 <= r < nc and 0 <= c < m for r, c, _ in entries)


# name, nc, ni, m, n, small entries of the long variable
PLANTED_SHAPES = [("planted", 3200, 3, 40, 4096, 64 * FLUSH + 28), ("planted_all_inputs", 100, 12, 12, 128, FLUSH + 12),
                  ("planted_one_input", 100, 1, 12, 128, FLUSH + 12)]


def planted_case(cid, which):
    """-> (Case, [Planted of A, B, C]).  The long variable is 0 in A (the constant one), 2 in B, 5 in C"""
    name, nc, ni, m, n, n_light = next(s for s in PLANTED_SHAPES if s[0] == which)
    p = MODULI[CURVE_FR[cid]]
    rnd = random.Random(f"setup/{name}/{cid}")
    made = [planted_matrix(rnd, p, nc, m, n_light, v_long) for v_long in (0, 2, 5)]
    for entries, pl in made:
        check_planted(entries, pl, nc, m, p)
    if which == "planted":
        # every lane of the long-row wave takes at least FLUSH small entries (they are dealt out 64 apart), and heavy ones follow;
        # one variable without entries below ni, one above
        lo, hi = made[0][1].empty_vars
        assert n_light // 64 >= FLUSH and n_light > 64 * FLUSH and lo < ni <= hi and m <= 40
    return Case(f"{name}{cid}", cid, nc, ni, m, n, 1, [e for e, _ in made], random_toxic(rnd, p)), [pl for _, pl in made]


# Mixed-radix domains, n = dom_m 2^a with dom_m = q or q^2: name -> (curve, dom_m, a, nc + ni).  GeneralEvaluationDomain::new takes the
# SMALLEST q^b 2^a' (b <= 2) that holds nc + ni.  One past the scalar field's radix-2 limit that is 49 * 2^12 = 200 704 for MNT6-298
# (below 7 * 2^15 = 229 376) and 5 * 2^13 = 40 960 for MNT6-753 (below 25 * 2^11); 7 * 2^15 is the domain of 200 705 .. 229 376.
MIXED = {"mixed1": (1, 49, 12, (1 << 17) + 1), "mixed3": (3, 5, 13, (1 << 15) + 1), "mixed1_q7": (1, 7, 15, 49 * (1 << 12) + 1)}
MIXED_VARS = 24


def few_variable_mats(cid, nc, m, seed):
    """one to three entries per constraint row on m variables, coefficients from a table of 16 values (small integers and random
    elements): every variable's transposed row is a long row whose lanes reduce many times"""
    p = MODULI[CURVE_FR[cid]]
    rnd = random.Random(f"setup/few/{cid}/{seed}")
    table = [1, p - 1, 2, p - 2, 32, p - 32, 33, p - 33, 0, 1, 1, p - 1] + [rnd.randrange(p) for _ in range(4)]
    g = np.random.Generator(np.random.PCG64([21, cid, nc, m]))
    mats = []
    for _ in range(3):
        rows = np.repeat(np.arange(nc, dtype=np.int64), g.integers(1, 4, size=nc))
        cols = g.integers(0, m, size=len(rows))
        vals = g.integers(0, len(table), size=len(rows))
        mats.append([(r, c, table[v]) for r, c, v in zip(rows.tolist(), cols.tolist(), vals.tolist())])
        assert min(np.bincount(cols, minlength=m)) > LONG_ROW
    return mats


_MIXED = {}


def mixed_case(name, ni=2):
    """a case of MIXED over few_variable_mats (made once, shared, read-only)"""
    if name not in _MIXED:
        cid, dom_m, a, need = MIXED[name]
        rnd = random.Random(f"setup/{name}")
        _MIXED[name] = Case(name, cid, need - ni, ni, MIXED_VARS, dom_m << a, dom_m, few_variable_mats(cid, need - ni, MIXED_VARS, name),
                            random_toxic(rnd, MODULI[CURVE_FR[cid]]))
    return _MIXED[name]


def h_sample(n):
    """0, 1, n - 2 and a stride of about 1000 over h_query's n - 1 entries"""
    return sorted(set([0, 1, n - 2] + list(range(0, n - 1, 997))))


_DOM, _SCALARS = {}, {}


def domain(co, field, n, dom_m=1):
    if (field, n) not in _DOM:
        _DOM[(field, n)] = domain_elements(co, field, n, dom_m)
        assert len(_DOM[(field, n)]) == n and _DOM[(field, n)][0] == 1
    return _DOM[(field, n)]


def case_scalars(co, case, toxic=None):
    """key_scalars of a case (with other toxic waste if given); the case's own are made once and shared, callers leave them unchanged"""
    field = CURVE_FR[case.cid]
    if toxic is not None:
        return key_scalars(case.mats, case.nc, case.m, case.ni, toxic, domain(co, field, case.n, case.dom_m), MODULI[field])
    if case.name not in _SCALARS or _SCALARS[case.name][0] is not case:
        _SCALARS[case.name] = (case, case_scalars(co, case, case.toxic))
    return _SCALARS[case.name][1]
