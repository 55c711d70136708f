"""CPU: the K8 vector-algebra entry points (batch inversion, pointwise product, division by X^n - 1, polynomial product) as the header
declares them, their argument checks without a device, and the exact-integer reference the GPU tests compare against
(tests/poly_algebra_reference.py)."""
import ctypes as C
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_rust_boundary as crb  # noqa: E402
import poly_algebra_reference as pr  # noqa: E402

K8 = {
    "pcdhip_vec_mul": ("i32", ["ptr", "ptr", "ptr", "usize", "ptr"]),
    "pcdhip_vec_batch_inverse": ("i32", ["ptr", "ptr", "usize", "ptr", "ptr"]),
    "pcdhip_poly_div_vanishing": ("i32", ["ptr", "ptr", "usize", "usize", "ptr", "ptr", "ptr", "ptr"]),
    "pcdhip_poly_mul": ("i32", ["ptr", "ptr", "usize", "ptr", "usize", "ptr", "ptr"]),
}


def test_prototypes_and_exports():
    from pcd_amd import capi
    protos, _ = crb.c_prototypes()
    lib = capi.lib()
    for name, sig in K8.items():
        assert protos.get(name) == sig, name
        assert name in capi.EXPORTS
        assert hasattr(lib, name), name


def test_null_context_is_an_argument_error():
    from pcd_amd import capi
    lib = capi.lib()
    n = C.c_size_t(0)
    E_ARG = -1
    assert lib.pcdhip_vec_mul(None, None, None, 0, None) == E_ARG
    assert lib.pcdhip_vec_batch_inverse(None, None, 0, None, None) == E_ARG
    assert lib.pcdhip_poly_div_vanishing(None, None, 0, 4, None, C.byref(n), None, None) == E_ARG
    assert lib.pcdhip_poly_mul(None, None, 0, None, 0, None, C.byref(n)) == E_ARG


def test_reference_batch_inverse_elementwise():
    rnd = random.Random(21)
    for field in range(4):
        p = pr.MODULI[field]
        for n in (0, 1, 2, 9, 40):
            xs = [rnd.randrange(1, p) for _ in range(n)]
            for i in (0, n - 1, n // 2, n // 2 + 1):  # planted zeros, two of them adjacent
                if 0 <= i < n:
                    xs[i] = 0
            if n == 40:
                xs[5], xs[6] = 1, p - 1
            for scale in (1, rnd.randrange(1, p)):
                want = [scale * pow(x, -1, p) % p if x else 0 for x in xs]
                assert pr.batch_inverse(xs, p, scale) == want
        assert pr.batch_inverse([0, 0, 0], p) == [0, 0, 0]


def test_reference_div_vanishing_against_oracle_products():
    from oracle import coracle as co
    rnd = random.Random(22)
    for field in range(4):
        p = pr.MODULI[field]
        for ln, n in ((0, 4), (3, 4), (4, 4), (5, 4), (8, 4), (9, 4), (23, 1), (37, 5)):
            a = [rnd.randrange(p) for _ in range(ln)]
            q, r = pr.div_vanishing(a, n, p)
            assert len(q) == max(ln - n, 0) and len(r) == min(ln, n)
            if ln == 0:
                continue
            # q (X^n - 1) + r coefficient by coefficient: q_(i-n) - q_i + r_i, the -1 through the oracle's Montgomery product
            qm = pr.to_mont(co, field, q + [0] * (ln - len(q)))
            neg = co.fp_op(field, "mul", qm, np.repeat(pr.to_mont(co, field, [p - 1]), ln, axis=0))
            back = co.fp_op(field, "add", neg, pr.to_mont(co, field, [0] * n + q)[:ln])
            back = co.fp_op(field, "add", back, pr.to_mont(co, field, r + [0] * (ln - len(r))))
            assert pr.to_ints(co, field, back) == a


def test_reference_product_at_a_random_point():
    rnd = random.Random(23)
    for field in range(4):
        p = pr.MODULI[field]
        assert pr.mul_schoolbook([], [1, 2], p) == [] and pr.mul_schoolbook([3], [], p) == []
        for la, lb in ((1, 1), (1, 7), (33, 32), (6, 19)):
            a = [rnd.randrange(p) for _ in range(la)]
            b = [rnd.randrange(p) for _ in range(lb)]
            c = pr.mul_schoolbook(a, b, p)
            z = rnd.randrange(p)
            assert len(c) == la + lb - 1
            assert pr.horner(c, z, p) == pr.horner(a, z, p) * pr.horner(b, z, p) % p
