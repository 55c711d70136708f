"""CPU: pcdhip_kzg_vk_prepare / pcdhip_kzg_check_combinations / pcdhip_kzg_check_scalars (K14: the MarlinKZG10 check on device) as the
header, the Python binding and the library declare them, their argument checks that need no device, and the integer reference of the
GPU test (tests/kzg_check_reference.py) tied down against the oracle's pairing and MSM and against the prover's reference, independently
of the library."""
import ctypes as C
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_rust_boundary as crb  # noqa: E402
import kzg_batch_open_reference as kb  # noqa: E402
import kzg_check_reference as kk  # noqa: E402
import kzg_commit_reference as kc  # noqa: E402
import kzg_reference as kr  # noqa: E402

E_ARG = -1
NAMES = ("pcdhip_kzg_vk_prepare", "pcdhip_kzg_vk_free", "pcdhip_kzg_check_combinations", "pcdhip_kzg_check_scalars",
         "pcdhip_kzg_check_combinations_last_plan")


def test_prototypes_and_exports():
    from pcd_amd import capi
    protos, _ = crb.c_prototypes()
    assert protos.get("pcdhip_kzg_vk_prepare") == ("i32", ["ptr", "i32"] + ["ptr"] * 5 + ["usize", "ptr"])
    assert protos.get("pcdhip_kzg_vk_free") == ("void", ["ptr", "ptr"])
    assert protos.get("pcdhip_kzg_check_combinations") == ("i32", ["ptr", "ptr", "usize"] + ["ptr"] * 5 + ["usize"] + ["ptr"] * 10)
    assert protos.get("pcdhip_kzg_check_scalars") == ("i32", ["ptr", "i32", "usize", "usize", "ptr", "usize"] + ["ptr"] * 9)
    assert protos.get("pcdhip_kzg_check_combinations_last_plan") == ("i32", ["ptr", "ptr"])
    for name in NAMES:
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name)


def test_null_context_is_refused():
    from pcd_amd import capi
    lib = capi.lib()
    out = np.full(64, 0xAB, dtype=np.uint64)
    ok = (C.c_int * 4)(7, 7, 7, 7)
    op = out.ctypes.data_as(C.c_void_p)
    vk = C.c_void_p(0x1234)
    assert lib.pcdhip_kzg_vk_prepare(None, 0, op, op, op, op, op, 1, C.byref(vk)) == E_ARG
    assert vk.value == 0x1234
    assert lib.pcdhip_kzg_check_combinations(None, None, 1, op, None, None, None, None, 1, op, op, None, op, None, None, op, None, None, ok) == E_ARG
    assert lib.pcdhip_kzg_check_combinations(None, None, 0, None, None, None, None, None, 0, None, None, None, None, None, None, None, None, None, ok) == E_ARG
    assert lib.pcdhip_kzg_check_scalars(None, 1, 0, 1, None, 1, op, op, None, op, None, None, None, op, op) == E_ARG
    assert lib.pcdhip_kzg_check_combinations_last_plan(None, op) == E_ARG
    lib.pcdhip_kzg_vk_free(None, None)
    assert list(ok) == [7, 7, 7, 7] and (out == 0xAB).all()


def small_case(srs, rnd, P=2, m=4):
    """random commitments (as exponents), two of them with a degree bound over one shift power, and a valid witness per opening"""
    p = srs.p
    r = lambda: rnd.randrange(1, p)
    case = dict(shift_exps=[r()], comm_exps=[r() for _ in range(m)], shifted_exps=[r() if i in (1, 3) else 0 for i in range(m)],
                shift_index=[0 if i in (1, 3) else -1 for i in range(m)], points=[r() for _ in range(P)],
                a=[[r() for _ in range(m)] for _ in range(P)], s=[[r() if i in (1, 3) else 0 for i in range(m)] for _ in range(P)],
                values=[r() for _ in range(P)], random_v=[r() for _ in range(P)], item_values=[[r() for _ in range(m)] for _ in range(P)])
    case["w_exps"] = []
    for o in range(P):
        c = kk.combined_exponent(srs, case["shift_exps"], case["comm_exps"], case["shifted_exps"], case["shift_index"], case["a"][o], case["s"][o],
                                 case["item_values"][o])
        case["w_exps"].append(kk.solve_witness(srs, c, case["values"][o], case["random_v"][o], case["points"][o]))
    return case


def verdict_of(srs, case, randomizers):
    return kk.verdict(srs, case["shift_exps"], case["comm_exps"], case["shifted_exps"], case["w_exps"], case["shift_index"], case["points"], case["a"],
                      case["s"], case["values"], case["random_v"], case["item_values"], randomizers)


def vector_points(co, srs, case):
    """the check's vector as affine points and flags, by the oracle's double-and-add"""
    xs = kk.vector_exponents(srs, case["shift_exps"], case["comm_exps"], case["shifted_exps"], case["w_exps"])
    pts = [srs.exponent_times_g(co, e) for e in xs]
    return np.stack([xy for xy, _ in pts]), np.array([inf for _, inf in pts], dtype=np.uint8)


def affine_of_msm(co, curve, pts, inf, scalars, L):
    xy, f = co.to_affine(curve, 1, co.msm(curve, 1, pts, kr.limbs_of_ints(scalars, L), inf=inf))
    return xy[0], int(f[0])


def test_verdict_agrees_with_the_oracle_pairing():
    from oracle import coracle as co
    curve = 0
    srs = kc.Srs(co, curve, 2, seed=1401)
    p, rnd, L = srs.p, random.Random(1402), kr.LIMBS[srs.fr]
    case = small_case(srs, rnd)
    spoiled = dict(case, values=[case["values"][0], (case["values"][1] + 1) % p])
    for cs, want in ((case, [True, True]), (spoiled, [True, False])):
        assert verdict_of(srs, cs, None) == want
        pts, inf = vector_points(co, srs, cs)
        n_head = len(pts) - len(cs["w_exps"])
        left, right = kk.collapse(p, 1, cs["shift_index"], cs["points"], cs["a"], cs["s"], cs["values"], cs["random_v"], cs["item_values"], None)
        for e in range(2):
            lxy, linf = affine_of_msm(co, curve, pts, inf, left[e], L)
            rxy, rinf = affine_of_msm(co, curve, pts[n_head:], inf[n_head:], right[e], L)
            assert not linf and not rinf
            same = np.array_equal(co.pairing(curve, lxy, srs.h), co.pairing(curve, rxy, srs.beta_h))
            assert same == want[e], e
    rho = [1, rnd.randrange(1, p)]
    assert verdict_of(srs, case, rho) == [True] and verdict_of(srs, spoiled, rho) == [False]


def test_combined_collapse_is_the_sum_of_the_openings():
    from oracle import coracle as co
    curve = 0
    srs = kc.Srs(co, curve, 2, seed=1411)
    p, rnd, L = srs.p, random.Random(1412), kr.LIMBS[srs.fr]
    case = small_case(srs, rnd, P=3, m=4)
    pts, inf = vector_points(co, srs, case)
    m, P, ns = 4, 3, 1
    rho = [1, rnd.randrange(1, p), rnd.randrange(1, p)]
    left, right = kk.collapse(p, ns, case["shift_index"], case["points"], case["a"], case["s"], case["values"], case["random_v"], case["item_values"], rho)
    assert right == [rho]
    got = affine_of_msm(co, curve, pts, inf, left[0], L)
    # L_o from the equation itself, term by term: sum_i a comm_i + sum_i s (shifted_i - v S_k(i)) - value g - random_v gamma_g + z W_o
    acc = None
    for o in range(P):
        idx, sc = [0, 1, 2 + ns + 2 * m + o], [-case["values"][o], -case["random_v"][o], case["points"][o]]
        for i in range(m):
            idx.append(2 + ns + i)
            sc.append(case["a"][o][i])
            if case["s"][o][i]:
                idx += [2 + ns + m + i, 2 + case["shift_index"][i]]
                sc += [case["s"][o][i], -case["s"][o][i] * case["item_values"][o][i]]
        lxy, linf = affine_of_msm(co, curve, pts[idx], inf[idx], [x % p for x in sc], L)
        assert not linf
        term = co.scalar_mul(curve, 1, lxy, kr.limbs_of_ints([rho[o]], L)[0])
        acc = term if acc is None else co.jac_add(curve, 1, acc, term)
    xy, f = co.to_affine(curve, 1, acc)
    assert got == (got[0], 0) and int(f[0]) == 0 and np.array_equal(xy[0], got[0])


def test_openings_of_the_prover_reference_verify():
    """what kzg_batch_open_reference.witness_exponent produces, with a degree-bound term and a shifted blinding, has verdict true"""
    from oracle import coracle as co
    srs = kc.Srs(co, 0, 16, seed=1421)
    p, rnd = srs.p, random.Random(1422)
    items = [dict(poly=[rnd.randrange(p) for _ in range(9)], blinding=[rnd.randrange(p) for _ in range(2)]),
             dict(poly=[rnd.randrange(p) for _ in range(6)], blinding=[rnd.randrange(p) for _ in range(2)], shifted=True, shifted_offset=3,
                  shifted_blinding=[rnd.randrange(p) for _ in range(2)]),
             dict(poly=[rnd.randrange(p) for _ in range(12)]),
             dict(poly=[rnd.randrange(p) for _ in range(4)], shifted=True, shifted_offset=7)]
    m = len(items)
    ev = lambda c, x: kr.horner(c, x, p)
    b, g = srs.beta, srs.gamma
    comm = [(ev(it["poly"], b) + g * ev(it.get("blinding", []), b)) % p for it in items]
    shifted = [(pow(b, it["shifted_offset"], p) * ev(it["poly"], b) + g * ev(it.get("shifted_blinding", []), b)) % p if it.get("shifted") else 0
               for it in items]
    shift_exps = [pow(b, 3, p), pow(b, 7, p)]
    shift_index = [-1, 0, -1, 1]
    points = [rnd.randrange(p), rnd.randrange(p)]
    a = [[rnd.randrange(1, p) for _ in range(m)], [rnd.randrange(1, p), 0, 0, rnd.randrange(1, p)]]
    s = [[0, rnd.randrange(1, p), 0, 0], [0, rnd.randrange(1, p), 0, rnd.randrange(1, p)]]
    w, values, rvs = zip(*[kb.witness_exponent(srs, items, z, a[o], s[o]) for o, z in enumerate(points)])
    iv = [[ev(it["poly"], z) for it in items] for z in points]
    args = (shift_index, points, a, s, list(values), list(rvs), iv)
    assert kk.verdict(srs, shift_exps, comm, shifted, list(w), *args, None) == [True, True]
    assert kk.verdict(srs, shift_exps, comm, shifted, list(w), *args, [1, rnd.randrange(1, p)]) == [True]
    # ... and a wrong individual value of a degree-bound item, or the other shift power, does not
    bad = [list(r) for r in iv]
    bad[1][3] = (bad[1][3] + 1) % p
    assert kk.verdict(srs, shift_exps, comm, shifted, list(w), shift_index, points, a, s, list(values), list(rvs), bad, None) == [True, False]
    assert kk.verdict(srs, shift_exps, comm, shifted, list(w), [-1, 1, -1, 1], points, a, s, list(values), list(rvs), iv, None) == [False, False]
