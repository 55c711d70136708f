"""CPU: pcdhip_kzg_commit (KZG10::commit / MarlinKZG10::commit over device-resident polynomials) as the header, the Python binding and
the library declare it, its argument checks that need no device, and the integer reference of the GPU test
(tests/kzg_commit_reference.py) against Horner evaluation on a setup with known beta and gamma."""
import ctypes as C
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_rust_boundary as crb  # noqa: E402
import kzg_commit_reference as kc  # noqa: E402
import kzg_reference as kr  # noqa: E402

E_ARG = -1


def test_prototype_struct_and_exports():
    from pcd_amd import capi
    protos, structs = crb.c_prototypes()
    assert protos.get("pcdhip_kzg_commit") == ("i32", ["ptr", "ptr", "ptr", "ptr", "ptr", "usize", "ptr", "ptr", "ptr", "ptr", "ptr"])
    assert structs.get("pcdhip_kzg_commit_item") == ["ptr", "u64", "ptr", "u64", "ptr", "u64", "u64", "u32", "u32"]
    assert "pcdhip_kzg_commit" in capi.EXPORTS
    assert hasattr(capi.lib(), "pcdhip_kzg_commit")
    assert C.sizeof(capi.KzgCommitItem) == 64
    fns, rstructs = crb.rust_externs()
    assert fns.get("pcdhip_kzg_commit") == protos["pcdhip_kzg_commit"]
    assert rstructs.get("pcdhip_kzg_commit_item") == structs["pcdhip_kzg_commit_item"]


def test_argument_errors_without_a_device():
    from pcd_amd import capi
    lib = capi.lib()
    out = np.zeros(64, dtype=np.uint64)
    flags = np.zeros(8, dtype=np.uint8)
    op, fp = out.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p)
    item = (capi.KzgCommitItem * 1)()
    # a NULL context, with and without items
    assert lib.pcdhip_kzg_commit(None, None, None, None, item, 1, op, fp, None, None, None) == E_ARG
    assert lib.pcdhip_kzg_commit(None, None, None, None, None, 0, None, None, None, None, None) == E_ARG
    # k > 0 with NULL items is refused before any handle is looked into (the handles here are zeroed stand-ins, never dereferenced)
    stand_in = np.zeros(1 << 13, dtype=np.uint64)
    sp = stand_in.ctypes.data_as(C.c_void_p)
    assert lib.pcdhip_kzg_commit(sp, sp, None, None, None, 1, op, fp, None, None, None) == E_ARG


def test_reference_commits_to_the_evaluation_at_beta():
    from oracle import coracle as co
    curve = 0
    srs = kc.Srs(co, curve, 12, seed=77)
    p, rnd = srs.p, random.Random(78)
    cases = [([rnd.randrange(p) for _ in range(13)], [rnd.randrange(p) for _ in range(3)]),
             ([rnd.randrange(p) for _ in range(9)] + [0, 0, 0], [rnd.randrange(p)]),      # zeros at the top: trimmed to 9
             ([], [rnd.randrange(p), rnd.randrange(p)]),                                   # the hiding part alone
             ([rnd.randrange(p) for _ in range(5)], None),                                 # not hiding
             ([0, 0, 0, 0], None)]                                                         # the zero polynomial: identity
    for a, bl in cases:
        xy, inf, t = kc.commit(co, curve, srs.powers, a, srs.gpowers, bl)
        assert t == kc.trimmed_len(a, p) and (t == 0 or a[t - 1] != 0) and all(x == 0 for x in a[t:])
        e = kr.horner(a, srs.beta, p) + srs.gamma * kr.horner(bl or [], srs.beta, p)
        want_xy, want_inf = srs.exponent_times_g(co, e)
        assert inf == want_inf and np.array_equal(xy, want_xy), (len(a), bl is not None)
    assert kc.commit(co, curve, srs.powers, [0, 0, 0, 0])[1] == 1
    # the shifted form: p(beta) beta^offset
    a = [rnd.randrange(p) for _ in range(6)]
    xy, inf, _ = kc.commit(co, curve, srs.powers, a, offset=7)
    want_xy, want_inf = srs.exponent_times_g(co, kr.horner(a, srs.beta, p) * pow(srs.beta, 7, p))
    assert inf == want_inf == 0 and np.array_equal(xy, want_xy)
