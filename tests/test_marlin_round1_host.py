"""CPU: the K11 entry points (round 1 and the first sumcheck) as the header declares them, their argument checks without a device, and
the exact-integer reference the GPU tests compare against (tests/marlin_round1_reference.py) checked against itself: the placement
against reindex_by_subdomain, w against z_poly, the interpolation against the oracle's inverse transform, a satisfied system's
zero sum, and the AHP verifier's equation at a random point."""
import ctypes as C
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_rust_boundary as crb  # noqa: E402
import marlin_reference as mr  # noqa: E402
import marlin_round1_reference as m1  # noqa: E402
import poly_algebra_reference as par  # noqa: E402

K11 = {
    "pcdhip_marlin_mats_upload_ex": ("i32", ["ptr", "i32", "ptr", "ptr", "ptr", "usize", "usize", "usize", "u32", "ptr"]),
    "pcdhip_marlin_zm_evals": ("i32", ["ptr"] * 6),
    "pcdhip_marlin_place_assignment": ("i32", ["ptr", "i32", "usize", "usize", "ptr", "usize", "ptr"]),
    "pcdhip_poly_add_vanishing_multiple": ("i32", ["ptr", "ptr", "usize", "ptr", "usize", "usize", "ptr"]),
    "pcdhip_marlin_sumcheck1_q": ("i32", ["ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "usize", "ptr"]),
    "pcdhip_marlin_round1": ("i32", ["ptr", "ptr", "ptr", "ptr", "usize", "ptr", "usize", "ptr", "usize"] + ["ptr"] * 9),
    "pcdhip_marlin_sumcheck1": ("i32", ["ptr"] * 4 + ["ptr", "usize"] * 4 + ["usize"] + ["ptr"] * 5),
}


def test_prototypes_exports_and_rust_declarations():
    from pcd_amd import capi
    protos, _ = crb.c_prototypes()
    rust, _ = crb.rust_externs()
    lib = capi.lib()
    for name, sig in K11.items():
        assert protos.get(name) == sig, name
        assert rust.get(name) == sig, name
        assert name in capi.EXPORTS
        assert hasattr(lib, name), name


def test_null_arguments_are_argument_errors():
    from pcd_amd import capi
    lib = capi.lib()
    E_ARG = -1
    h = C.c_void_p()
    n = C.c_size_t(7)
    assert lib.pcdhip_marlin_mats_upload_ex(None, 1, None, None, None, 0, 4, 4, 3, C.byref(h)) == E_ARG and not h.value
    assert lib.pcdhip_marlin_zm_evals(None, None, None, None, None, None) == E_ARG
    assert lib.pcdhip_marlin_place_assignment(None, 1, 4, 4, None, 0, None) == E_ARG
    assert lib.pcdhip_poly_add_vanishing_multiple(None, None, 0, None, 0, 4, C.byref(n)) == E_ARG and n.value == 7
    assert lib.pcdhip_marlin_sumcheck1_q(None, None, None, None, None, None, None, 0, None) == E_ARG
    assert lib.pcdhip_marlin_round1(None, None, None, None, 0, None, 0, None, 0, None, None, None, None, None, None, None, None, None) == E_ARG
    assert lib.pcdhip_marlin_sumcheck1(None, None, None, None, None, 0, None, 0, None, 0, None, 0, 0, None, None, None, None, None) == E_ARG


def test_place_is_the_inverse_of_reindex():
    for h_n, x_n in ((1, 1), (8, 8), (8, 2), (64, 4), (512, 16)):
        for cols in sorted({1, max(h_n - 3, 1), h_n}):
            z = [100 + c for c in range(cols)]
            placed = m1.place(z, h_n, x_n)
            assert len(placed) == h_n
            for c in range(cols):
                assert placed[mr.reindex(c, h_n, x_n)] == z[c], (h_n, x_n, c)
            assert sorted(placed) == [0] * (h_n - cols) + z  # every other place reads as zero
    assert m1.place([5, 6, 7], 4, 4, num_cols=2) == [5, 6, 0, 0]


def test_poly_mul_and_vanishing_multiple_against_schoolbook():
    rnd = random.Random(1101)
    for field in (1, 3):
        p = mr.MODULI[field]
        for la, lb in ((1, 1), (3, 9), (17, 17), (40, 2)):
            a, b = [rnd.randrange(p) for _ in range(la)], [rnd.randrange(p) for _ in range(lb)]
            a[0], b[-1] = p - 1, p - 1
            assert m1.poly_mul(a, b, p) == par.mul_schoolbook(a, b, p)
        assert m1.poly_mul([], [1], p) == []
        for ln, k, n in ((5, 1, 8), (9, 1, 8), (12, 2, 8), (3, 3, 2), (8, 0, 8)):
            c, blind = [rnd.randrange(p) for _ in range(ln)], [rnd.randrange(p) for _ in range(k)]
            got = m1.add_vanishing_multiple(c, blind, n, p)
            want = m1.poly_add(c, par.mul_schoolbook(blind, [p - 1] + [0] * (n - 1) + [1], p), p)
            assert got == want and len(got) == (max(ln, n + k) if k else ln)


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_reference_round1_and_first_sumcheck(field):
    from oracle import coracle as co
    rnd = random.Random(1110 + field)
    p = mr.MODULI[field]
    rows, cols, h_n, x_n = 5, 7, 8, 2
    dom_h, dom_x = mr.domain_elements(co, field, h_n), mr.domain_elements(co, field, x_n)
    mats, z = m1.satisfied_system(rnd, p, rows, cols, x_n)
    assert all(a * b % p == c for a, b, c in zip(*(m1.zm_evals(m, z, h_n, p) for m in mats)))
    for ks in ((0, 0, 0), (1, 1, 1), (2, 1, 0)):
        blinds = [[rnd.randrange(p) for _ in range(k)] for k in ks]
        r1 = m1.round1(mats, z, h_n, x_n, dom_h, dom_x, blinds, p)
        assert [len(r1[k]) for k in ("x_hat", "z_poly", "w", "w_rem", "za_poly", "zb_poly")] == [x_n, h_n + ks[0], h_n + ks[0] - x_n, x_n,
                                                                                               h_n + ks[1], h_n + ks[2]]
        # interp(place(z)) at w^pi(c) gives z[c], blinded or not; x_hat at the points of X gives the public input
        for c in range(cols):
            assert mr.horner(r1["z_poly"], dom_h[mr.reindex(c, h_n, x_n)], p) == z[c]
        assert [mr.horner(r1["x_hat"], x, p) for x in dom_x] == z[:x_n]
        # w v_X + x_hat = z_poly coefficient by coefficient, with a zero remainder
        assert r1["w_rem"] == [0] * x_n
        back = m1.poly_add(m1.poly_mul(r1["w"], [p - 1] + [0] * (x_n - 1) + [1], p), r1["x_hat"], p)
        assert back == r1["z_poly"]
        # the quadratic interpolation agrees with the oracle's inverse transform
        for ev in (r1["za_evals"], m1.place(z, h_n, x_n)):
            assert mr.interpolate(ev, dom_h, p) == mr.to_ints(co, field, co.fft(field, mr.to_mont(co, field, ev), inverse=True))
        # the first sumcheck: a zero constant term for the satisfied system and a mask that sums to zero on H ...
        eta = [rnd.randrange(p) for _ in range(3)]
        alpha, beta = rnd.randrange(p), rnd.randrange(p)
        assert alpha not in dom_h and beta != alpha
        mask = m1.zero_sum_mask(rnd, p, h_n, 2 * h_n + 3)
        assert sum(mr.horner(mask, x, p) for x in dom_h) % p == 0
        for s in (None, mask):
            sc = m1.sumcheck1(mats, eta, alpha, r1["za_poly"], r1["zb_poly"], r1["z_poly"], s, h_n, x_n, dom_h, p)
            assert sc["sigma"] == 0 and len(sc["g1"]) == h_n - 1 and len(sc["t_poly"]) == h_n
            assert len(sc["h1"]) == m1.q1_length(h_n, h_n + ks[1], h_n + ks[2], h_n + ks[0], len(s or [])) - h_n
            # ... q_1 on H is the pointwise formula, and the verifier's equation holds at a random point
            r_ev = mr.bivariate_lagrange(alpha, dom_h, p)
            t_ev = mr.t_evals(mats, eta, r_ev, h_n, x_n, p)
            q_h = m1.sumcheck1_q(eta, r1["za_evals"], r1["zb_evals"], r_ev, t_ev, m1.place(z, h_n, x_n), p)
            assert [mr.horner(sc["q1"], x, p) for x in dom_h] == [(a + mr.horner(s or [], x, p)) % p for a, x in zip(q_h, dom_h)]
            assert mr.horner(sc["r_poly"], beta, p) == m1.r_alpha_at(alpha, beta, h_n, p)
            assert m1.verifier_equation_holds(eta, alpha, beta, r1, sc, s, h_n, p)
        # one changed variable breaks the system: the constant term is no longer zero (and the equation still holds with it)
        bad = list(z)
        bad[mats[2][0][1]] = (bad[mats[2][0][1]] + 1) % p  # a variable that C's first row mentions
        rb = m1.round1(mats, bad, h_n, x_n, dom_h, dom_x, blinds, p)
        sb = m1.sumcheck1(mats, eta, alpha, rb["za_poly"], rb["zb_poly"], rb["z_poly"], mask, h_n, x_n, dom_h, p)
        assert sb["sigma"] != 0 and m1.verifier_equation_holds(eta, alpha, beta, rb, sb, mask, h_n, p)


def test_x_equal_h_gives_an_empty_w():
    from oracle import coracle as co
    rnd = random.Random(1120)
    field, p, n = 1, mr.MODULI[1], 8
    dom = mr.domain_elements(co, field, n)
    mats, z = m1.satisfied_system(rnd, p, n, n, n)
    r1 = m1.round1(mats, z, n, n, dom, dom, ([], [], []), p)
    assert r1["w"] == [] and r1["w_rem"] == [0] * n and r1["z_poly"] == r1["x_hat"] and m1.place(z, n, n) == z
    r1 = m1.round1(mats, z, n, n, dom, dom, ([3], [], []), p)
    assert r1["w"] == [3] and r1["w_rem"] == [0] * n
