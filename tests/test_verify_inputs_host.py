"""CPU: the case list behind tests/test_gpu_verify_inputs.py (tests/verify_reference.py), without a GPU.  The verdict of every case is
known by construction (trapdoor keys); here the C++ oracle's own pairing check -- co.groth16_verify, which shares nothing with that
construction but the points -- has to agree with it, member by member, and the properties the case names promise are checked in Python
integers.

Nothing is left out on the 753-bit curves: the oracle's verification takes 0.4 - 0.7 s there, a case one to five seconds, the whole
module under a minute on one core."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_reference as vr  # noqa: E402

def _case_ids():
    return [(cid, c.name) for cid in range(4) for c in vr.cases(cid)]


@pytest.mark.parametrize("cid,name", _case_ids(), ids=lambda v: str(v))
def test_oracle_agrees_with_the_construction(co, cid, name):
    case = vr.case_named(cid, name)
    b = vr.build(co, cid, case)
    assert b.key.num_inputs == len(case.s) and b.expect.any()
    for i, m in enumerate(case.members):
        got = co.groth16_verify(b.key, vr.mont(co, cid, m.xs), b.proofs[i].copy(), b.proofs_inf[i].copy())
        assert got == m.expect_accept, (name, i, m.expect_accept)
        # the verdict in integers: u v = a b + S(xs) c + w d with the C actually sent
        k = b.key
        u, v, w = vr.proof_scalars(k, m.proof_xs, (name, m.force_c_infinite), m.force_c_infinite)
        w = k.a if m.c_is_alpha else w
        assert ((u * v - k.a * k.b - k.S(m.xs) * k.c - w * k.d) % k.r == 0) == m.expect_accept, (name, i)
        assert list(b.proofs_inf[i]) == [0, 0, int(w == 0)]


@pytest.mark.parametrize("cid", range(4))
def test_case_list_keeps_its_promises(co, cid):
    r, nwin = vr.scalar_modulus(cid), vr.num_windows(cid)
    assert nwin == {298: 38, 753: 95}[r.bit_length()] and 8 * (nwin - 1) < r.bit_length() <= 8 * nwin
    cs = {c.name: c for c in vr.cases(cid)}
    assert [c.name for c in vr.cases(cid)] == [c.name for c in vr.cases(cid)] and vr.cases(cid) == vr.cases(cid)   # deterministic
    want = {"no_inputs", "zeros", "edges", "lanes_twice", "abc0_infinite", "unused_input", "acc_infinite", "acc_infinite_c_infinite",
            "equal_lanes", "opposite_lanes"}
    assert set(cs) == want | ({"table_limit_256", "table_limit_257"} if cid == 0 else set())
    for c in cs.values():
        assert all(0 <= v < r for v in c.s) and all(len(m.xs) == len(c.s) - 1 and all(0 <= x < r for x in m.xs) for m in c.members)
        kinds = {(m.expect_accept, m.c_is_alpha, m.xs == m.proof_xs) for m in c.members}
        assert (True, False, True) in kinds
        if c.name != "unused_input":   # reject neighbours: C := alpha everywhere; a changed input wherever there is an input
            assert (False, True, True) in kinds and (len(c.s) == 1 or (False, False, False) in kinds)
            assert all(m.expect_accept == (m.xs == m.proof_xs and not m.c_is_alpha) for m in c.members)
    dot = lambda c, xs: (c.s[0] + sum(x * s for x, s in zip(xs, c.s[1:]))) % r

    assert len(cs["no_inputs"].s) == 1 and [m.expect_accept for m in cs["no_inputs"].members] == [True, False]
    assert len(cs["zeros"].s) == 4 and cs["zeros"].members[0].xs == [0, 0, 0]
    e = cs["edges"].members[0].xs
    assert len(cs["edges"].s) == 9 and e[:5] == [0, 1, r - 1, 255, 256] and e[6] == r - 2
    assert e[5].bit_length() == 8 * (nwin - 1) + 1 and e[5] & (e[5] - 1) == 0                       # a single top digit, and that digit is 1
    assert set(e[7].to_bytes(nwin, "little").rstrip(b"\0")) == {255} and e[7] < r <= (e[7] << 8 | 255)  # every digit 255, as many as fit below r
    assert any(m.xs != m.proof_xs and sorted(m.xs) == sorted(m.proof_xs) for m in cs["edges"].members)   # the rotated neighbour
    lt = cs["lanes_twice"]
    items = (len(lt.s) - 1) * nwin
    assert len(lt.s) == 1 + -(-130 // nwin) and items > 64
    assert len(range(0, items, 64)) != len(range(63, items, 64)) and len(range(63, items, 64)) >= 2   # trips of the first and of the last lane
    assert cs["abc0_infinite"].s[0] == 0 and all(cs["abc0_infinite"].s[1:])
    un = cs["unused_input"]
    j = un.s.index(0)
    assert j >= 1 and all(m.expect_accept for m in un.members) and un.members[0].xs[j - 1] != 0
    assert un.members[1].xs[j - 1] != un.members[0].xs[j - 1] and un.members[1].proof_xs == un.members[0].xs
    for name, forced in (("acc_infinite", False), ("acc_infinite_c_infinite", True)):   # S = 0, with C finite and with C infinite as well
        ai = cs[name]
        assert all(ai.s) and all(m.force_c_infinite == forced for m in ai.members) and ai.s == cs["acc_infinite"].s
        for m in ai.members:
            assert dot(ai, m.proof_xs) == 0 and (dot(ai, m.xs) == 0) == (m.xs == m.proof_xs)
        k = vr.build(co, cid, ai).key
        for i, m in enumerate(ai.members):
            u, v, w = vr.proof_scalars(k, m.proof_xs, (name, forced), forced)
            assert (w == 0) == forced and (not forced or u * v % r == k.a * k.b % r)
            assert vr.build(co, cid, ai).proofs_inf[i][2] == (forced and not m.c_is_alpha)
    for name in ("equal_lanes", "opposite_lanes"):
        c = cs[name]
        x = c.members[0].xs
        assert len(x) == vr.EQUAL_BASES == 64 and len(set(x)) == 1 and len(set(x[0].to_bytes(nwin, "little"))) == 1 and x[0] != 0
    assert len(set(cs["equal_lanes"].s[1:])) == 1 and cs["equal_lanes"].s[1] != 0
    op = cs["opposite_lanes"]
    assert all(op.s[j] != 0 and (op.s[j] + op.s[j + 32]) % r == 0 for j in range(1, 33)) and dot(op, op.members[0].xs) == op.s[0] != 0
    if cid == 0:
        lo, hi = cs["table_limit_256"], cs["table_limit_257"]
        assert len(lo.s) == vr.TABLE_LIMIT == 256 and len(hi.s) == 257 and hi.s[:256] == lo.s
        assert hi.members[0].xs[:255] == lo.members[0].xs and hi.s[256] != 0


def test_non_canonical_encodings_are_what_they_say():
    """the values tests/test_gpu_verify_inputs.py submits as x_1 in place of 1: all >= r, all within the scalar's words, and the first
    three are 1 again to a verifier that reduces mod r or reads only nwin digits"""
    for cid in (0, 3):
        r, nwin, L = vr.scalar_modulus(cid), vr.num_windows(cid), vr.O.CURVES[cid].fr.n64
        for name, x in vr.non_canonical(cid):
            assert r <= x < 1 << (64 * L), name
            assert np.array_equal(vr.scalar_words(cid, [x])[0], [(x >> (64 * i)) & (2 ** 64 - 1) for i in range(L)])
        d = dict(vr.non_canonical(cid))
        assert d["r+1"] % r == 1 and d["r"] % r == 0 and d["top word ones"] >> (64 * (L - 1)) == 2 ** 64 - 1
        assert ("1+2^(8 nwin)" in d) == (8 * nwin < 64 * L)
        if "1+2^(8 nwin)" in d:
            assert d["1+2^(8 nwin)"] & ((1 << (8 * nwin)) - 1) == 1
