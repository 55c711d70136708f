"""GPU: Groth16 key generation (`pcdhip_groth16_setup`) at its edges -- one-element to 16-element domains, partial batches of the
Lagrange kernel, transposed matrices with planted long rows, flush and lane / wave boundaries, mixed-radix domains, tau inside the
domain, tau = 0, zero and unreduced toxic waste -- every point and every flag bit-exact against the integer reference of
tests/setup_reference.py, and against the oracle's setup wherever that runs (radix-2 domains).  tests/test_setup_reference_host.py
checks the same case lists on the CPU."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import setup_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu

_R1CS = {}


def r1cs(co, case):
    if case.name not in _R1CS or _R1CS[case.name][0] is not case:
        _R1CS[case.name] = (case, sr.r1cs_of(co, case))
    return _R1CS[case.name][1]


def gpu_setup(ctx, co, case, toxic_mont=None):
    cid = case.cid
    tm = sr.toxic_mont(co, cid, case.toxic) if toxic_mont is None else toxic_mont
    K = ctx.groth16_setup(cid, r1cs(co, case), co.generator(cid, 1), co.generator(cid, 2), tm)
    assert K["domain_size"] == case.n
    return K


def assert_key(K, want, tag, h_sample=None):
    """every point, query and flag; a flagged entry has all-zero coordinates (the expected arrays have them too).  With h_sample the
    expected h_query holds those rows only; the flags of h are always complete"""
    for name, _ in sr.POINTS:
        assert np.array_equal(K[name], want[name]), (tag, name)
    for name, _, flags in sr.QUERIES:
        assert K[flags].shape == want[flags].shape and np.array_equal(K[flags], want[flags]), (tag, flags)
        assert not K[name][K[flags] != 0].any(), (tag, name, "coordinates under a flag")
        got = K[name][h_sample] if name == "h_query" and h_sample is not None else K[name]
        assert got.shape == want[name].shape and np.array_equal(got, want[name]), (tag, name)


def check_case(ctx, co, case, oracle=True):
    want = sr.expected_key(co, case.cid, sr.case_scalars(co, case))
    K = gpu_setup(ctx, co, case)
    assert_key(K, want, case.name)
    if oracle:
        keys = co.groth16_setup(case.cid, r1cs(co, case), sr.toxic_mont(co, case.cid, case.toxic), nthreads=8)
        sr.assert_matches_oracle({k: v for k, v in K.items() if k != "domain_size"}, keys, case.name)
    return K


def refused(fn):
    """the call returns PCDHIP_E_ARG (-1)"""
    from pcd_amd import capi
    with pytest.raises(capi.PcdHipError) as e:
        fn()
    assert "(rc=-1)" in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------------- tiny domains
@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_tiny_domains(co, gpu_ctx, cid):
    """n = 1 (no constraints, no h, no l: a_0 = L_0(tau) = 1), 2, 4 (a partial batch of the Lagrange kernel), 8 (exactly one batch) and 16
    with the input rows in the middle and at the end of the domain"""
    for shape in sr.TINY_SHAPES:
        case = sr.tiny_case(cid, shape)
        K = check_case(gpu_ctx, co, case)
        assert K["h_query"].shape[0] == case.n - 1 and K["l_query"].shape[0] == case.m - case.ni
    K = gpu_setup(gpu_ctx, co, sr.tiny_case(cid, sr.TINY_SHAPES[0]))
    assert np.array_equal(K["a_query"][0], co.generator(cid, 1)) and not K["a_inf"][0] and K["b_g1_inf"][0] and K["b_g2_inf"][0]


# ------------------------------------------------------------------------------------------------------------ planted matrices
@pytest.mark.parametrize("which", [s[0] for s in sr.PLANTED_SHAPES])
@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_planted_matrices(co, gpu_ctx, cid, which):
    """the transposed mat-vec over variables with no entry, exactly 16 and 17 entries, more than 48 * 64 small-integer entries and
    then heavy ones, the coefficients 0, +-1, +-32, +-33, a duplicated (row, column), an empty constraint row (planted_case asserts all
    of it from the entry lists); at nc = 100 also with every variable an input (l_query = NULL) and with one input"""
    case, planted = sr.planted_case(cid, which)
    K = check_case(gpu_ctx, co, case)
    for v in planted[0].empty_vars:
        assert K["b_g1_inf"][v] and K["b_g2_inf"][v] and bool(K["a_inf"][v]) == (v >= case.ni)
    assert K["l_query"].shape[0] == case.m - case.ni and (which != "planted_all_inputs" or K["l_query"].size == 0)


# ---------------------------------------------------------------------------------------------------------- mixed-radix domains
def check_mixed(ctx, co, name):
    case = sr.mixed_case(name)
    assert co.domain_size(sr.CURVE_FR[case.cid], case.nc + case.ni) == case.n
    hs = sr.h_sample(case.n)
    want = sr.expected_key(co, case.cid, sr.case_scalars(co, case), h_sample=hs)
    K = gpu_setup(ctx, co, case)
    assert_key(K, want, name, h_sample=hs)
    assert K["h_query"].shape[0] == case.n - 1 and not K["h_inf"].any()
    return case


def test_mixed_radix_domain_mnt6_298(co, gpu_ctx):
    """nc + ni = 2^17 + 1 on MNT6-298: GeneralEvaluationDomain::new takes 49 * 2^12 = 200 704 elements (the smallest q^b 2^a; 7 * 2^15
    is larger and is the domain of test_tau_inside_a_mixed_radix_domain).  24 variables, every transposed row a long row.  All of a /
    b_g1 / b_g2 / gamma_abc / l, every flag of h and 200-odd sampled points of h against the integer reference (the oracle's setup is
    radix-2 only).  Measured wall time of this test on an MI355X host, reference and case building included: 1.5 s (printed below)"""
    t0 = time.perf_counter()
    check_mixed(gpu_ctx, co, "mixed1")
    print(f"mixed1: {time.perf_counter() - t0:.1f} s")


def test_mixed_radix_domain_mnt6_753(co, gpu_ctx):
    """nc + ni = 2^15 + 1 on MNT6-753: 5 * 2^13 = 40 960 elements; as above.  Measured wall time of this test on an MI355X host: 1.2 s"""
    t0 = time.perf_counter()
    check_mixed(gpu_ctx, co, "mixed3")
    print(f"mixed3: {time.perf_counter() - t0:.1f} s")


# ------------------------------------------------------------------------------------------------------------ tau in the domain
@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_tau_inside_the_domain_is_refused(co, gpu_ctx, cid):
    """tau = w^k: n = 4 (one partial batch), k = 3; n = 64, k = 3 (mid-batch), 7 (end of a batch), 8 (first slot of the second lane), 63
    (last slot); tau = r - 1 = w^(n/2) on every even n.  The context gives the reference's key afterwards"""
    field = sr.CURVE_FR[cid]
    p = sr.MODULI[field]
    for shape, ks in (((2, 2, 4, 4), (3,)), ((40, 3, 9, 64), (3, 7, 8, 63)), ((1, 1, 2, 2), ())):
        case = sr.tiny_case(cid, shape)
        dom = sr.domain(co, field, case.n)
        assert dom[case.n // 2] == p - 1
        for tau in [dom[k] for k in ks] + [p - 1]:
            with pytest.raises(ValueError):
                sr.case_scalars(co, case, case.toxic[:4] + (tau,))
            refused(lambda: gpu_setup(gpu_ctx, co, case, sr.toxic_mont(co, cid, case.toxic[:4] + (tau,))))
        check_case(gpu_ctx, co, case)


def test_tau_inside_a_mixed_radix_domain(co, gpu_ctx):
    """n = 7 * 2^15 (MNT6-298, nc + ni = 200 705), tau = w^k for k = 0, 1, 7, 8, n - 1 over the few-variable matrices; then the key of
    that domain with the case's own tau, compared as in the mixed-radix tests.  Measured wall time on an MI355X host: 1.7 s"""
    case = sr.mixed_case("mixed1_q7")
    assert case.n == 7 << 15
    dom = sr.domain(co, sr.CURVE_FR[case.cid], case.n, case.dom_m)
    for k in (0, 1, 7, 8, case.n - 1):
        refused(lambda: gpu_setup(gpu_ctx, co, case, sr.toxic_mont(co, case.cid, case.toxic[:4] + (dom[k],))))
    t0 = time.perf_counter()
    check_mixed(gpu_ctx, co, "mixed1_q7")
    print(f"mixed1_q7: {time.perf_counter() - t0:.1f} s")


# ------------------------------------------------------------------------------------------------------------------ toxic edges
@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_tau_zero_is_legal(co, gpu_ctx, cid):
    """Z(0) = -1, every L_j = 1 / n; h_0 = -1 / delta and every later h is the identity with its flag set"""
    p = sr.MODULI[sr.CURVE_FR[cid]]
    for shape in ((5, 3, 6, 8), (13, 3, 9, 16)):
        case = sr.tiny_case(cid, shape)
        toxic = case.toxic[:4] + (0,)
        sc = sr.case_scalars(co, case, toxic)
        assert sc["h_query"] == [-pow(toxic[3], -1, p) % p] + [0] * (case.n - 2)
        tm = sr.toxic_mont(co, cid, toxic)
        K = gpu_setup(gpu_ctx, co, case, tm)
        assert_key(K, sr.expected_key(co, cid, sc), case.name)
        assert not K["h_inf"][0] and K["h_inf"][1:].all() and not K["h_query"][1:].any()
        keys = co.groth16_setup(cid, r1cs(co, case), tm, nthreads=8)
        sr.assert_matches_oracle({k: v for k, v in K.items() if k != "domain_size"}, keys, case.name)


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_zero_and_unreduced_toxic_waste_is_refused(co, gpu_ctx, cid):
    """alpha, beta, gamma or delta = 0, and an ABI image >= the modulus in any of the five slots (the modulus itself, all bits set):
    PCDHIP_E_ARG, and after each refusal the same context makes the reference's key"""
    field = sr.CURVE_FR[cid]
    p, L = sr.MODULI[field], sr.LIMBS[field]
    case = sr.tiny_case(cid, (5, 3, 6, 8))
    want = sr.expected_key(co, cid, sr.case_scalars(co, case))
    good = sr.toxic_mont(co, cid, case.toxic)
    bad = []
    for slot in range(4):
        t = good.copy()
        t[slot] = 0
        bad.append(t)
    for slot in range(5):
        for image in (p, (1 << (64 * L)) - 1):
            t = good.copy()
            t[slot] = sr.limbs_of_ints([image], L)[0]
            bad.append(t)
    assert len(bad) == 14 and all(not np.array_equal(t, good) for t in bad)
    for t in bad:
        refused(lambda: gpu_setup(gpu_ctx, co, case, t))
        assert_key(gpu_setup(gpu_ctx, co, case), want, case.name)
