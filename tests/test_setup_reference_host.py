"""Host checks of tests/setup_reference.py (no GPU, no library): on the tiny domains and the planted matrices that
tests/test_gpu_setup_edges.py runs on the device, the integer reference IS the key the C++ oracle's setup makes -- every array and every
flag -- and, at one 298-bit shape, the key of the pure-Python oracle.  The case lists assert their own row-length conditions when they
are built, so a malformed case fails here before it meets a kernel.

Mixed-radix domains: the C++ oracle's setup (oracle/groth16.hpp G16::setup) builds a Radix2Domain of 2^ceil(log2(nc + ni)) elements
whatever the field's 2-adicity, and oracle/pyoracle.py groth16_setup does the same, so neither accepts such a domain; the GPU tests use
the integer reference alone there.  What can be checked on the CPU is checked below: the oracle's mixed-radix transform gives a cyclic
group of the right order, and the Lagrange coefficients over it sum to 1 and interpolate X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import setup_reference as sr  # noqa: E402


def check_against_oracle(co, case):
    field = sr.CURVE_FR[case.cid]
    assert co.domain_size(field, case.nc + case.ni) == case.n
    want = sr.expected_key(co, case.cid, sr.case_scalars(co, case))
    keys = co.groth16_setup(case.cid, sr.r1cs_of(co, case), sr.toxic_mont(co, case.cid, case.toxic), nthreads=8)
    assert keys.domain_size == case.n
    sr.assert_matches_oracle(want, keys, case.name)
    return want


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_tiny_domains_are_the_oracles_keys(co, cid):
    for shape in sr.TINY_SHAPES:
        case = sr.tiny_case(cid, shape)
        want = check_against_oracle(co, case)
        assert want["h_query"].shape[0] == case.n - 1 and want["l_query"].shape[0] == case.m - case.ni
    # nc = 0: the one Lagrange coefficient of the one-element domain is 1, whatever tau
    sc = sr.case_scalars(co, sr.tiny_case(cid, sr.TINY_SHAPES[0]))
    assert sc["a_query"] == [1] and sc["b_g1_query"] == [0] and sc["h_query"] == [] and sc["l_query"] == []


@pytest.mark.parametrize("which", [s[0] for s in sr.PLANTED_SHAPES])
@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_planted_matrices_are_the_oracles_keys(co, cid, which):
    case, planted = sr.planted_case(cid, which)
    want = check_against_oracle(co, case)
    # the variables without entries are identities in b (and in a above ni: the input rows put every instance variable into a)
    for v in planted[0].empty_vars:
        assert want["b_g1_inf"][v] and want["b_g2_inf"][v] and bool(want["a_inf"][v]) == (v >= case.ni)


def test_pure_python_oracle_agrees_at_one_shape(co):
    from oracle import pyoracle as O
    cid = 0
    case = sr.tiny_case(cid, (5, 3, 6, 8))
    curve = O.CURVES[cid]
    rows = [[[(v, c) for r, c, v in e if r == j] for j in range(case.nc)] for e in case.mats]
    pk = O.groth16_setup(curve, O.R1CS(curve.fr, case.ni, *rows, [0] * case.m), case.toxic)
    want = sr.expected_key(co, cid, sr.case_scalars(co, case))
    for name, grp in sr.POINTS:
        xy, inf = O.pack_points(curve, grp, [pk[name]])
        assert not inf[0] and np.array_equal(xy[0], want[name]), name
    for name, grp, flags in sr.QUERIES:
        xy, inf = O.pack_points(curve, grp, pk[name])
        assert np.array_equal(inf, want[flags]) and np.array_equal(xy, want[name]), name


def test_tau_zero_scalars(co):
    """Z(0) = -1: every Lagrange coefficient is 1 / n, h_0 = -1 / delta and the rest of h is zero"""
    case = sr.tiny_case(1, (5, 3, 6, 8))
    p = sr.MODULI[sr.CURVE_FR[1]]
    dom = sr.domain(co, sr.CURVE_FR[1], case.n)
    assert sr.lagrange_at(0, dom, p) == [pow(case.n, -1, p)] * case.n
    sc = sr.case_scalars(co, case, case.toxic[:4] + (0,))
    assert sc["h_query"] == [-pow(case.toxic[3], -1, p) % p] + [0] * (case.n - 2)
    with pytest.raises(ValueError):
        sr.lagrange_at(dom[3], dom, p)
    assert dom[case.n // 2] == p - 1


@pytest.mark.parametrize("name", list(sr.MIXED))
def test_mixed_radix_case_is_well_formed(co, name):
    case = sr.mixed_case(name)
    cid, dom_m, a, need = sr.MIXED[name]
    field = sr.CURVE_FR[cid]
    p = sr.MODULI[field]
    n = dom_m << a
    q = {49: 7, 7: 7, 5: 5}[dom_m]
    # GeneralEvaluationDomain::new picks dom_m 2^a here (the smallest q^b 2^a' that holds nc + ni), which the setup of neither oracle
    # can run on: theirs would be the radix-2 domain of 2^log elements, more than the field's 2-adicity allows
    log = (need - 1).bit_length()
    assert need == case.nc + case.ni and co.domain_size(field, need) == n == case.n and co.domain_size(field, need - 1) == need - 1
    assert case.m <= 24 and sr.r1cs_of(co, case).domain_log == log and n < (1 << log)
    assert name == "mixed1_q7" or need == (1 << (log - 1)) + 1   # one past the last radix-2 domain
    dom = sr.domain(co, field, n, dom_m)
    w = dom[1]
    assert pow(w, n, p) == 1 and pow(w, n // 2, p) == p - 1 and pow(w, n // q, p) != 1
    assert all(dom[k] == pow(w, k, p) for k in (2, 7, 8, n // 2, n - 1))
    u = sr.lagrange_at(case.toxic[4], dom, p)
    assert sum(u) % p == 1 and sum(x * y for x, y in zip(u, dom)) % p == case.toxic[4]
    hs = sr.h_sample(n)
    assert hs[:2] == [0, 1] and hs[-1] == n - 2 and n // 997 <= len(hs) <= n // 997 + 4
    for k in (0, 1, 7, 8, n - 1):
        with pytest.raises(ValueError):
            sr.lagrange_at(dom[k], dom, p)
