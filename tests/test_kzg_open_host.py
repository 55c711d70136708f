"""CPU: the K7 open-side entry points (KZG10 / MarlinKZG10 openings) as the header declares them, their argument checks without a
device, and the exact-integer division the GPU tests compare against (tests/kzg_reference.py)."""
import ctypes as C
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_rust_boundary as crb  # noqa: E402
import kzg_reference as kr  # noqa: E402

K7 = {
    "pcdhip_poly_eval": ("i32", ["ptr", "ptr", "ptr", "usize", "ptr", "ptr"]),
    "pcdhip_poly_lincomb": ("i32", ["ptr", "ptr", "ptr", "ptr", "usize", "ptr", "ptr"]),
    "pcdhip_poly_div_linear": ("i32", ["ptr", "ptr", "usize", "ptr", "ptr", "ptr"]),
    "pcdhip_kzg_open": ("i32", ["ptr", "ptr", "ptr", "ptr", "usize", "ptr", "usize", "ptr", "ptr", "ptr", "ptr"]),
    "pcdhip_kzg_check": ("i32", ["ptr", "i32", "ptr", "ptr", "ptr", "ptr", "usize", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr",
                                 "ptr", "ptr"]),
}


def test_prototypes_and_exports():
    from pcd_amd import capi
    protos, _ = crb.c_prototypes()
    for name, sig in K7.items():
        assert protos.get(name) == sig, name
        assert name in capi.EXPORTS


def test_null_context_is_an_argument_error():
    from pcd_amd import capi
    lib = capi.lib()
    z = np.zeros(12, dtype=np.uint64)
    out = np.zeros(64, dtype=np.uint64)
    zp, op = z.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    n = C.c_size_t(0)
    ok = C.c_int(7)
    E_ARG = -1
    assert lib.pcdhip_poly_eval(None, None, None, C.c_size_t(0), zp, op) == E_ARG
    assert lib.pcdhip_poly_lincomb(None, None, None, None, C.c_size_t(0), None, C.byref(n)) == E_ARG
    assert lib.pcdhip_poly_div_linear(None, None, C.c_size_t(0), zp, None, op) == E_ARG
    assert lib.pcdhip_kzg_open(None, None, None, None, C.c_size_t(0), None, C.c_size_t(0), zp, op, op, op) == E_ARG
    assert lib.pcdhip_kzg_check(None, 0, None, None, None, None, C.c_size_t(0), None, None, None, None, None, None, None, None,
                                C.byref(ok)) == E_ARG


def test_reference_division_against_oracle_products():
    from oracle import coracle as co
    rnd = random.Random(11)
    for field in range(4):
        p = kr.MODULI[field]
        for n in (1, 2, 5, 33):
            a = [rnd.randrange(p) for _ in range(n)]
            z = rnd.randrange(p)
            q, v = kr.div_linear(a, z, p)
            assert len(q) == n - 1 and v == kr.horner(a, z, p)
            # q(X) (X - z) + v through the oracle's Montgomery products: coefficient i = q_(i-1) - z q_i (+ v at i = 0)
            qm = kr.to_mont(co, field, q + [0, 0])
            zm = np.repeat(kr.to_mont(co, field, [z]), n + 1, axis=0)
            zq = co.fp_op(field, "mul", zm, qm)
            shifted = np.concatenate([kr.to_mont(co, field, [v]), qm[:n]])
            back = kr.to_ints(co, field, co.fp_op(field, "sub", shifted, zq[:n + 1]))
            assert back[:n] == a and back[n] == 0
