"""CPU: pcdhip_poly_open_quotients / pcdhip_kzg_batch_open (K13: a round's openings as one queued call) as the header, the Python
binding and the library declare them, their argument checks that need no device, and the integer reference of the GPU test
(tests/kzg_batch_open_reference.py) tied down on a setup whose trapdoor is kept, independently of the library."""
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
import kzg_commit_reference as kc  # noqa: E402
import kzg_reference as kr  # noqa: E402

E_ARG = -1


def test_prototypes_and_exports():
    from pcd_amd import capi
    protos, _ = crb.c_prototypes()
    assert protos.get("pcdhip_poly_open_quotients") == ("i32", ["ptr", "i32", "ptr", "usize", "usize", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr"])
    assert protos.get("pcdhip_kzg_batch_open") == ("i32", ["ptr"] * 5 + ["usize", "usize"] + ["ptr"] * 7)
    assert protos.get("pcdhip_kzg_batch_open_last_plan") == ("i32", ["ptr", "ptr"])
    for name in ("pcdhip_poly_open_quotients", "pcdhip_kzg_batch_open", "pcdhip_kzg_batch_open_last_plan"):
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name)


def test_null_context_is_refused():
    from pcd_amd import capi
    lib = capi.lib()
    out = np.zeros(64, dtype=np.uint64)
    flags = np.zeros(8, dtype=np.uint8)
    lens = (C.c_size_t * 8)()
    op, fp = out.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p)
    item = (capi.KzgCommitItem * 1)()
    assert lib.pcdhip_poly_open_quotients(None, 1, item, 1, 1, op, op, None, None, lens, op) == E_ARG
    assert lib.pcdhip_poly_open_quotients(None, 1, None, 0, 0, None, None, None, None, None, None) == E_ARG
    assert lib.pcdhip_kzg_batch_open(None, None, None, None, item, 1, 1, op, op, None, op, fp, op, op) == E_ARG
    assert lib.pcdhip_kzg_batch_open(None, None, None, None, None, 0, 0, None, None, None, None, None, None, None) == E_ARG
    assert lib.pcdhip_kzg_batch_open_last_plan(None, op) == E_ARG
    assert not out.any() and not flags.any()


def random_round(rnd, p, n_items=6):
    """items of unequal lengths, the first half hiding, two with a degree bound (one of them with a shifted blinding)"""
    items = []
    for i in range(n_items):
        it = dict(poly=[rnd.randrange(p) for _ in range(rnd.randrange(3, 12))])
        if i < n_items // 2:
            it["blinding"] = [rnd.randrange(p) for _ in range(2)]
        items.append(it)
    items[1].update(shifted=True, shifted_offset=3, shifted_blinding=[rnd.randrange(p) for _ in range(2)])
    items[4].update(shifted=True, shifted_offset=0)
    return items


def test_reference_satisfies_the_exponent_identity():
    from oracle import coracle as co
    curve = 0
    srs = kc.Srs(co, curve, 16, seed=1301)
    p, rnd = srs.p, random.Random(1302)
    items = random_round(rnd, p)
    m = len(items)
    for trial in range(4):
        z = rnd.randrange(p)
        a = [rnd.randrange(p) if rnd.random() < 0.7 else 0 for _ in range(m)]
        s = [0] * m
        if trial % 2 == 0:
            s[1] = rnd.randrange(1, p)
        if trial >= 2:
            s[4] = rnd.randrange(1, p)
        w, value, rv = kb.witness_exponent(srs, items, z, a, s)
        lhs, rhs = kb.identity_sides(srs, items, z, a, s, w)
        assert lhs == rhs, trial
        assert value == kr.horner(kr.lincomb([it["poly"] for it in items], a, p), z, p)
        # ... and it fails when one s is changed after the fact
        if any(s):
            i = 1 if s[1] else 4
            bad = list(s)
            bad[i] = (bad[i] + 1) % p or 1
            lhs, rhs = kb.identity_sides(srs, items, z, a, bad, w)
            assert lhs != rhs, trial
    # the point the reference makes with the oracle's MSMs is that exponent times g
    z = rnd.randrange(p)
    a = [rnd.randrange(1, p) for _ in range(m)]
    s = [0, rnd.randrange(1, p), 0, 0, rnd.randrange(1, p), 0]
    got = kb.batch_open(co, curve, srs.powers, srs.gpowers, srs.powers, items, [z], [a], [s])[0]
    w, value, rv = kb.witness_exponent(srs, items, z, a, s)
    want_xy, want_inf = srs.exponent_times_g(co, w)
    assert got[1] == want_inf == 0 and np.array_equal(got[0], want_xy)
    assert got[2] == value and got[3] == rv
    # no coefficient at all: the identity and zero values
    got = kb.batch_open(co, curve, srs.powers, srs.gpowers, srs.powers, items, [z], [[0] * m], [[0] * m])[0]
    assert got[1] == 1 and not got[0].any() and got[2] == 0 and got[3] == 0


def test_collapse_equals_the_openings_one_by_one():
    from oracle import coracle as co
    srs = kc.Srs(co, 0, 16, seed=1311)
    p, rnd = srs.p, random.Random(1312)
    items = random_round(rnd, p)
    m = len(items)
    lcs = [dict(terms=[(rnd.randrange(1, p), 0), (rnd.randrange(1, p), 2), (p - 1, 5)]),
           dict(terms=[(1, 1)], bound=True),
           dict(terms=[(1, 4)], bound=True),
           dict(terms=[(rnd.randrange(1, p), 3), (1, 1)]),     # item 1 again, without its bound
           dict(terms=[(1, 2)])]
    points = [rnd.randrange(p), rnd.randrange(p)]
    queries = [(0, 0), (1, 0), (3, 0), (4, 0), (0, 1), (2, 1), (3, 1)]
    challenges = [(rnd.randrange(1, p), rnd.randrange(1, p)) for _ in queries]
    a, s = kb.collapse(lcs, queries, challenges, m, len(points), p)
    assert s[0][1] == challenges[1][1] and s[1][4] == challenges[5][1] and sum(map(bool, s[0] + s[1])) == 2
    for o, z in enumerate(points):
        w, value, rv = kb.witness_exponent(srs, items, z, a[o], s[o])
        sw = sv = srv = 0
        for (j, oo), (xi, xi_s) in zip(queries, challenges):
            if oo != o:
                continue
            row = [0] * m
            for c, i in lcs[j]["terms"]:
                row[i] = (row[i] + c) % p
            w1, v1, rv1 = kb.witness_exponent(srs, items, z, row, None)   # the combination opened alone
            sw, sv, srv = sw + xi * w1, sv + xi * v1, srv + xi * rv1
            if lcs[j].get("bound"):
                e = [0] * m
                e[lcs[j]["terms"][0][1]] = 1
                w2, _, rv2 = kb.witness_exponent(srs, items, z, [0] * m, e)  # its degree-bound witness alone
                sw, srv = sw + xi_s * w2, srv + xi_s * rv2
        assert (w, value, rv) == (sw % p, sv % p, srv % p), o
