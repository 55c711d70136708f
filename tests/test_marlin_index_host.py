"""CPU: the K10 entry points (the index on device, its commitments, the two device transforms) as the header declares them, their
argument checks without a device, and the exact-integer reference the GPU tests compare against (tests/marlin_index_reference.py)."""
import ctypes as C
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_rust_boundary as crb  # noqa: E402
import marlin_index_reference as mir  # noqa: E402
import marlin_reference as mr  # noqa: E402

K10 = {
    "pcdhip_marlin_index_build": ("i32", ["ptr", "i32", "ptr", "ptr", "ptr", "usize", "usize", "usize", "usize", "usize", "i32", "ptr"]),
    "pcdhip_marlin_index_free": ("void", ["ptr", "ptr"]),
    "pcdhip_marlin_index_info": ("i32", ["ptr", "ptr"]),
    "pcdhip_marlin_index_timings": ("i32", ["ptr", "ptr"]),
    "pcdhip_marlin_index_vec": ("i32", ["ptr", "i32", "i32", "i32", "ptr"]),
    "pcdhip_marlin_index_commit": ("i32", ["ptr", "ptr", "ptr", "ptr", "ptr"]),
    "pcdhip_fft_general_dev": ("i32", ["ptr", "ptr", "usize", "i32", "i32"]),
    "pcdhip_poly_evals_on_domain": ("i32", ["ptr", "ptr", "usize", "usize", "i32", "ptr"]),
}


def test_prototypes_and_exports():
    from pcd_amd import capi
    protos, _ = crb.c_prototypes()
    rust, _ = crb.rust_externs()
    lib = capi.lib()
    for name, sig in K10.items():
        assert protos.get(name) == sig, name
        assert rust.get(name) == sig, name
        assert name in capi.EXPORTS
        assert hasattr(lib, name), name


def test_null_context_and_null_handles_are_argument_errors():
    from pcd_amd import capi
    lib = capi.lib()
    E_ARG = -1
    h, b = C.c_void_p(), C.c_void_p()
    info = (C.c_uint64 * 4)()
    assert lib.pcdhip_marlin_index_build(None, 1, None, None, None, 0, 4, 4, 0, 0, 0, C.byref(h)) == E_ARG and not h.value
    assert lib.pcdhip_marlin_index_info(None, info) == E_ARG
    assert lib.pcdhip_marlin_index_timings(None, (C.c_float * 3)()) == E_ARG
    assert lib.pcdhip_marlin_index_vec(None, 0, 0, 0, C.byref(b)) == E_ARG and not b.value
    assert lib.pcdhip_marlin_index_commit(None, None, None, None, None) == E_ARG
    assert lib.pcdhip_fft_general_dev(None, None, 4, 0, 0) == E_ARG
    assert lib.pcdhip_poly_evals_on_domain(None, None, 1, 4, 0, None) == E_ARG
    lib.pcdhip_marlin_index_free(None, None)  # a null handle is a no-op


def test_index_order_is_row_major_with_a_stable_column_sort():
    # row 2 descending with two equal columns, row 0 after it in the list, an explicit zero and a duplicated (r, c)
    entries = [(2, 9, "a"), (2, 4, "b"), (2, 4, "c"), (2, 1, "d"), (0, 5, 0), (0, 5, 0), (0, 3, "e"), (2, 4, "f"), (1, 0, "g")]
    assert mir.index_order(entries) == [(0, 3, "e"), (0, 5, 0), (0, 5, 0), (1, 0, "g"), (2, 1, "d"), (2, 4, "b"), (2, 4, "c"), (2, 4, "f"), (2, 9, "a")]
    assert mir.csr_order(entries) == [(0, 5, 0), (0, 5, 0), (0, 3, "e"), (1, 0, "g"), (2, 9, "a"), (2, 4, "b"), (2, 4, "c"), (2, 1, "d"), (2, 4, "f")]
    ascending = [(0, 1, 7), (0, 2, 8), (3, 0, 9)]
    assert mir.index_order(ascending) == ascending


def test_val_times_h_is_v_times_row():
    from oracle import coracle as co
    rnd = random.Random(41)
    for field in range(4):
        p = mr.MODULI[field]
        for h_n, x_n in ((8, 2), (16, 16), (4, 1)):
            dom = mr.domain_elements(co, field, h_n)
            entries = [(rnd.randrange(h_n), rnd.randrange(h_n), rnd.choice([0, 1, p - 1, rnd.randrange(p)])) for _ in range(13)]
            k_n = 16
            row, col, rc, val = mir.arithmetize(entries, dom, h_n, x_n, k_n, p)
            for k, (r, c, v) in enumerate(mir.index_order(entries)):
                assert val[k] * h_n % p == v * row[k] % p and col[k] == dom[r] and rc[k] == row[k] * col[k] % p
                assert row[k] == dom[mr.reindex(c, h_n, x_n)] if x_n < h_n else row[k] == dom[c]
            assert row[13:] == [1] * 3 and col[13:] == [1] * 3 and rc[13:] == [1] * 3 and val[13:] == [0] * 3


def test_domain_rules_follow_the_oracle():
    from oracle import coracle as co
    for field in range(4):
        for nnz in ((0, 0, 0), (1, 0, 0), (200, 256, 13), (257, 3, 3), (5, 1 << 17, 9), ((1 << 17) + 1, 2, 2)):
            k_n = mir.domain_k(co, field, nnz)
            assert k_n == co.domain_size(field, max(max(nnz), 1)) and k_n >= max(nnz)
            b_n = mir.domain_b(co, field, k_n)
            assert b_n == co.domain_size(field, max(3 * k_n - 3, 1)) and b_n >= k_n
    assert mir.domain_k(co, 1, (200, 256, 13)) == 256 and mir.domain_b(co, 1, 256) == 1024
    assert mir.domain_k(co, 0, ((1 << 17) + 1, 2, 2)) == 200704 and mir.domain_b(co, 0, 200704) == 802816
    assert mir.odd_part(0, 200704) == 49 and mir.odd_part(0, 802816) == 49 and mir.odd_part(1, 1024) == 1
