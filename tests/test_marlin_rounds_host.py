"""CPU: the K9 entry points (r(alpha, .) on H, the resident matrices and t on H, the rational sumcheck) as the header declares them,
their argument checks without a device, and the exact-integer reference the GPU tests compare against (tests/marlin_reference.py)."""
import ctypes as C
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_rust_boundary as crb  # noqa: E402
import marlin_reference as mr  # noqa: E402

K9 = {
    "pcdhip_domain_bivariate_lagrange": ("i32", ["ptr", "i32", "usize", "ptr", "ptr"]),
    "pcdhip_marlin_mats_upload": ("i32", ["ptr", "i32", "ptr", "ptr", "ptr", "usize", "usize", "usize", "ptr"]),
    "pcdhip_marlin_mats_free": ("void", ["ptr", "ptr"]),
    "pcdhip_marlin_mats_info": ("i32", ["ptr", "ptr"]),
    "pcdhip_marlin_t_evals": ("i32", ["ptr", "ptr", "ptr", "ptr", "ptr"]),
    "pcdhip_marlin_sumcheck_ab": ("i32", ["ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "usize", "ptr", "ptr"]),
    "pcdhip_marlin_sumcheck_f": ("i32", ["ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "usize", "ptr"]),
}


def test_prototypes_and_exports():
    from pcd_amd import capi
    protos, _ = crb.c_prototypes()
    lib = capi.lib()
    for name, sig in K9.items():
        assert protos.get(name) == sig, name
        assert name in capi.EXPORTS
        assert hasattr(lib, name), name


def test_null_context_is_an_argument_error():
    from pcd_amd import capi
    lib = capi.lib()
    E_ARG = -1
    h = C.c_void_p()
    info = (C.c_uint64 * 4)()
    assert lib.pcdhip_domain_bivariate_lagrange(None, 1, 4, None, None) == E_ARG
    assert lib.pcdhip_marlin_mats_upload(None, 1, None, None, None, 0, 4, 4, C.byref(h)) == E_ARG and not h.value
    assert lib.pcdhip_marlin_mats_info(None, info) == E_ARG
    assert lib.pcdhip_marlin_t_evals(None, None, None, None, None) == E_ARG
    assert lib.pcdhip_marlin_sumcheck_ab(None, None, None, None, None, None, None, None, 0, None, None) == E_ARG
    assert lib.pcdhip_marlin_sumcheck_f(None, None, None, None, None, None, None, None, 0, None) == E_ARG
    lib.pcdhip_marlin_mats_free(None, None)  # a null handle is a no-op


def test_reindex_is_a_bijection():
    for h_n, x_n in ((1, 1), (8, 8), (8, 2), (64, 4), (512, 16)):
        image = [mr.reindex(c, h_n, x_n) for c in range(h_n)]
        assert sorted(image) == list(range(h_n)), (h_n, x_n)
        period = h_n // x_n
        assert image[:x_n] == [c * period for c in range(x_n)]                    # X sits on the multiples of the period ...
        assert all(j % period for j in image[x_n:]) and image[x_n:] == sorted(image[x_n:])  # ... the rest fill the gaps in order


def test_reference_sumcheck_forms_agree_and_f_zeroes():
    rnd = random.Random(31)
    for field in range(4):
        p = mr.MODULI[field]
        n = 9
        row, col, val = ([[rnd.randrange(p) for _ in range(n)] for _ in range(3)] for _ in range(3))
        alpha, beta = rnd.randrange(p), rnd.randrange(p)
        coeff = [rnd.randrange(p) for _ in range(3)]
        row[0][4] = beta
        prod = [[r * c % p for r, c in zip(row[m], col[m])] for m in range(3)]
        assert mr.sumcheck_ab(alpha, beta, coeff, row, col, None, val, p) == mr.sumcheck_ab(alpha, beta, coeff, row, col, prod, val, p)
        a, b = mr.sumcheck_ab(alpha, beta, coeff, row, col, None, val, p)
        f = mr.sumcheck_f(alpha, beta, coeff, row, col, None, val, p)
        assert b[4] == 0 and f[4] == 0 and a[4] != 0 and all(f[i] * b[i] % p == a[i] for i in range(n) if i != 4)


def test_reference_sumcheck_sums_to_t_at_beta():
    """sum over K of f = t(beta) with row = w^pi(c), col = w^r, val = v w^pi(c) / |H| and c_M = eta_M v_H(alpha) v_H(beta)"""
    from oracle import coracle as co
    rnd = random.Random(32)
    h_n, x_n, k_n = 8, 2, 16
    for field in range(4):
        p = mr.MODULI[field]
        dom = mr.domain_elements(co, field, h_n)
        assert dom[0] == 1 and len(set(dom)) == h_n and all(pow(w, h_n, p) == 1 for w in dom) and dom[2] == dom[1] * dom[1] % p
        mats = []
        for _ in range(3):
            entries = [(rnd.randrange(6), rnd.randrange(7), rnd.choice([1, p - 1, 2, rnd.randrange(p)])) for _ in range(rnd.randrange(9, 16))]
            entries.append(entries[0])  # a duplicated (r, c)
            mats.append(entries)
        alpha, beta = rnd.randrange(p), rnd.randrange(p)
        assert alpha not in dom and beta not in dom
        eta = [1, rnd.randrange(p), rnd.randrange(p)]
        r_alpha = mr.bivariate_lagrange(alpha, dom, p)
        assert all(r * (alpha - w) % p == (pow(alpha, h_n, p) - 1) % p for r, w in zip(r_alpha, dom))
        t = mr.t_evals(mats, eta, r_alpha, h_n, x_n, p)
        t_beta = mr.horner(mr.interpolate(t, dom, p), beta, p)
        vh = (pow(alpha, h_n, p) - 1) * (pow(beta, h_n, p) - 1) % p
        coeff = [e * vh % p for e in eta]
        rows, cols, vals = zip(*[mr.arithmetize(m, dom, h_n, x_n, k_n, p) for m in mats])
        f = mr.sumcheck_f(alpha, beta, coeff, rows, cols, None, vals, p)
        assert sum(f) % p == t_beta, field
        assert mr.bivariate_lagrange(dom[3], dom, p) == [0] * h_n  # x inside the domain
