"""CPU: the case lists and the pure-Python reference behind tests/test_gpu_lanesplit_ops.py and the 753-bit G1 step cases of
tests/test_gpu_field_ops.py (tests/field_reference.py), without a GPU: the generators are deterministic, every (lift, kind) combination
is there for every group, the raw records decode to the points they were made from, and the expected affine points -- computed by
oracle/pyoracle.py in Python integers -- agree with the C++ oracle's Jacobian addition (oracle/coracle.py jac_add + to_affine) on the
same inputs, so that the two references check each other."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_reference as fr  # noqa: E402
from oracle import coracle  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

GROUPS = [(cid, grp) for cid in range(4) for grp in (1, 2)]
KINDS = ["generic", "same", "negative", "infinity"]


def _fld(cid):
    return fr.FLD[O.FIELDS.index(O.CURVES[cid].fq)]


def _jac_words(cid, grp, pt, z):
    """the C++ oracle's Jacobian image (X || Y || Z, Montgomery u64 limbs) of the affine point pt under the coordinate z; None: (0 : 1 : 0)"""
    c = O.CURVES[cid]
    F, _ = c.group(grp)
    coords = (F.zero(), F.one(), F.zero()) if pt is None else fr.jacobian_of(cid, grp, pt, z)
    return O.pack_fp(c.fq, [cf for co in coords for cf in co]).reshape(-1)


def _oracle_affine(cid, grp, xyz):
    xy, inf = coracle.to_affine(cid, grp, xyz)
    return O.unpack_points(O.CURVES[cid], grp, xy, inf)[0]


def _decode(cid, grp, rec, ncoord):
    """the affine point of a raw record as the generators write it (coordinates on any representative, then the flag)"""
    fld = _fld(cid)
    W = (len(rec) - 1) // ncoord
    coords = [tuple(fr.unlimbs(rec[j * W + i:j * W + i + fld.N]) for i in range(0, W, fld.N)) for j in range(ncoord)]
    F, _ = O.CURVES[cid].group(grp)
    if rec[-1] or all(v % fld.p == 0 for v in coords[2]):
        return None
    return fr.affine_of(cid, grp, coords, False)


@pytest.mark.parametrize("cid,grp", GROUPS)
@pytest.mark.parametrize("jac", [False, True], ids=["xyzz", "jacobian"])
def test_step_cases_lifts_kinds_and_oracles(cid, grp, jac):
    cases = fr.step_cases(cid, grp, lz=False, jac=jac)
    assert cases == fr.step_cases(cid, grp, lz=False, jac=jac)                      # deterministic
    ncoord = 3 if jac else 4
    tags = [c[4] for c in cases]
    want_tags = {(k, lift) for k in KINDS for lift in range(1 << ncoord)} | {("identity+generic", 0), ("identity+infinity", 0)}
    assert set(tags) == want_tags and len(tags) == 2 * (len(want_tags) - 2) + 2        # every (lift, kind), for both base points
    F, a = O.CURVES[cid].group(grp)
    fld = _fld(cid)
    for rec, qs_raw, want1, want, tag, (pt, z, qs) in cases:
        assert len(rec) == ncoord * F.d * fld.N + 1 and len(qs_raw) == len(qs) == 9
        assert _decode(cid, grp, rec, ncoord) == pt, tag                            # the record is the point it was made from
        for q, raw in zip(qs, qs_raw):                                              # the affine images: Montgomery residues, zeros for the identity
            got = None if not any(raw) else tuple(tuple(fld.unmont(fr.unlimbs(raw[(j * F.d + i) * fld.N:(j * F.d + i + 1) * fld.N]))
                                                        for i in range(F.d)) for j in range(2))
            assert got == q, tag
        if tag[1] not in (0, (1 << ncoord) - 1):
            continue   # the expected values do not depend on the lift: the C++ oracle checks them on the two extreme ones
        acc = _jac_words(cid, grp, pt, z)
        for i, q in enumerate(qs):
            acc = coracle.jac_add(cid, grp, acc, _jac_words(cid, grp, q, F.one()))
            if i == 0:
                assert _oracle_affine(cid, grp, acc) == want1, tag
        assert _oracle_affine(cid, grp, acc) == want, tag


def test_lazy_step_cases_keep_their_band():
    """madd_lz's X is lifted to [15p, 16p), as before the generalisation"""
    fld = _fld(0)
    for rec, *_rest in fr.step_cases(0, 1, lz=True):
        x = fr.unlimbs(rec[:fld.N])
        assert x < fld.p or 15 * fld.p <= x < 16 * fld.p or rec[-1] == 1


@pytest.mark.parametrize("cid", range(4))
def test_jadd_cases_lifts_kinds_and_oracles(cid):
    cases = fr.jadd_cases(cid, 2)
    assert cases == fr.jadd_cases(cid, 2)
    tags = {c[3] for c in cases}
    assert {(k, lift) for k in ("generic", "same", "negative") for lift in range(16)} <= tags
    for form in ("flag", "Z=0", "Z=p"):
        assert {("identity left " + form, 0), ("identity left " + form, 1), ("identity right " + form, 0), ("identity right " + form, 1),
                ("identity both " + form, 0)} <= tags
    F, a = O.CURVES[cid].group(2)
    for p_rec, q_rec, want, tag, (P, zp, Q, zq) in cases:
        assert _decode(cid, 2, p_rec, 3) == P and _decode(cid, 2, q_rec, 3) == Q, tag
        if tag[0] in ("same", "negative"):   # the H = 0 branch through UNEQUAL coordinates
            assert zp != zq and p_rec[:len(p_rec) - 1] != q_rec[:len(q_rec) - 1]
            assert (want is None) == (tag[0] == "negative")
        got = coracle.jac_add(cid, 2, _jac_words(cid, 2, P, zp), _jac_words(cid, 2, Q, zq))
        assert _oracle_affine(cid, 2, got) == want, tag


@pytest.mark.parametrize("cid", range(4))
def test_jac_unary_cases(cid):
    cases = fr.jac_unary_cases(cid, 2)
    assert cases == fr.jac_unary_cases(cid, 2)
    assert {c[2] for c in cases} == {("finite", lift) for lift in range(8)} | {("identity flag", 0), ("identity Z=0", 0), ("identity Z=p", 0)}
    F, a = O.CURVES[cid].group(2)
    for rec, pt, tag, z in cases:
        assert _decode(cid, 2, rec, 3) == pt, tag
        if pt is not None and tag[1] in (0, 7):
            j = _jac_words(cid, 2, pt, z)
            assert _oracle_affine(cid, 2, coracle.jac_add(cid, 2, j, j)) == O.ec_add(F, a, pt, pt), tag


@pytest.mark.parametrize("fid", range(4))
def test_split_tower_cases(fid):
    p = fr.FLD[fid].p
    d, _ = fr.tower_of(fid)
    cases = fr.split_tower_cases(fid)
    assert cases == fr.split_tower_cases(fid)
    assert len(fr.tower_cases(fid)) == 100
    assert all(len(a) == len(b) == d and all(0 <= c < 2 * p for c in a + b) for a, b in cases)
    zero = fr.split_zero_cases(fid)
    for j in range(d):
        for z in (0, p):   # exactly coefficient j is zero, on the representative z; and a pair whose difference is zero in all but / in only j
            assert any(a[j] == z and all(c % p for i, c in enumerate(a) if i != j) for a, _ in zero)
        assert any([(x - y) % p == 0 for x, y in zip(a, b)] == [i != j for i in range(d)] for a, b in zero)
        assert any([(x - y) % p == 0 for x, y in zip(a, b)] == [i == j for i in range(d)] for a, b in zero)
    mixes = {a for a, _ in zero if all(c % p == 0 for c in a)}
    assert len(mixes) == 1 << d   # every mix of the representatives 0 and p: zero, and raw zero only once


def test_masks_and_packers():
    for n in (1, 19, 66, 138):
        masks = dict(fr.split_masks(n))
        assert masks == dict(fr.split_masks(n))
        assert sum(masks["all"]) == n and sum(masks["random half off"]) == n - n // 2
        assert [i for i, m in enumerate(masks["every third off"]) if not m] == list(range(2, n, 3))
    for fid in range(4):
        fld = fr.FLD[fid]
        for v in fr.unary_cases(fid)[:60]:
            assert fr.unlimbs(fr.limbs(v, fld.N)) == v and fr.is_normal(fr.limbs(v, fld.N))
            w = fr.abi_words(fld, v % fld.p)
            assert len(w) == fld.n32 and sum(x << (32 * i) for i, x in enumerate(w)) * pow(fld.R_abi, -1, fld.p) % fld.p == v % fld.p
            assert np.array_equal(O.pack_fp(O.FIELDS[fid], [v % fld.p]).reshape(-1).view(np.uint32), np.array(w, dtype=np.uint32))
        coords = [(1, 2), (3, 4), (5, 6)]
        rec = fr.lifted_record(fld, coords, 0b101)
        assert rec[-1] == 0 and [fr.unlimbs(rec[i:i + fld.N]) for i in range(0, 6 * fld.N, fld.N)] == [1 + fld.p, 2 + fld.p, 3, 4, 5 + fld.p, 6 + fld.p]
