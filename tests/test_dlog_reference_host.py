"""Host checks of tests/dlog_reference.py (no GPU, no library): the Python exponents ARE the key the C++ oracle's setup makes, every
prover case satisfies the verification equation in the exponent and is the proof both CPU provers make (flags included), the oracle's
pairing check accepts the finite ones, and every MSM input family has the sum the integers say and the coincidences its builder
promises.  tests/test_gpu_dlog_prover.py and tests/test_gpu_dlog_msm.py run the same cases on the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dlog_reference as dr  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

_KEYS = {}


def keys_of(co, circ):
    if circ.name not in _KEYS:
        st = dr.statement(co, circ)
        _KEYS[circ.name] = co.groth16_setup(circ.cid, st.r1cs, st.toxic_mont(), nthreads=4)
    return _KEYS[circ.name]


def same_points(xy, inf, want_xy, want_inf):
    inf, want_inf = np.asarray(inf).reshape(-1), np.asarray(want_inf).reshape(-1)
    xy, want_xy = np.asarray(xy).reshape(len(inf), -1), np.asarray(want_xy).reshape(len(want_inf), -1)
    fin = want_inf == 0
    return np.array_equal(inf != 0, want_inf != 0) and np.array_equal(xy[fin], want_xy[fin])


@pytest.mark.parametrize("circ", dr.CIRCUITS, ids=lambda c: c.name)
def test_setup_is_the_fixed_base_multiples_of_the_exponents(co, circ):
    """every query and every flag of co.groth16_setup's key"""
    st = dr.statement(co, circ)
    keys = keys_of(co, circ)
    e = st.exponents
    assert keys.domain_size == st.n and keys.num_vars == st.m
    for name, grp in (("alpha_g1", 1), ("beta_g1", 1), ("delta_g1", 1), ("beta_g2", 2), ("delta_g2", 2), ("gamma_g2", 2)):
        xy, inf = dr._multiples(co, circ.cid, grp, [e[name]])
        assert not inf[0] and np.array_equal(getattr(keys, name), xy[0]), name
    for name, grp, flags in (("a_query", 1, "a_inf"), ("b_g1_query", 1, "b_g1_inf"), ("b_g2_query", 2, "b_g2_inf"), ("h_query", 1, "h_inf"),
                             ("l_query", 1, "l_inf"), ("gamma_abc_g1", 1, "gamma_abc_inf")):
        xy, inf = dr._multiples(co, circ.cid, grp, e[name])
        assert same_points(getattr(keys, name), getattr(keys, flags), xy, inf), name
    # the variables no row of A (of B) mentions are there: the key has identities for the prover to skip
    assert any(v == 0 for v in e["b_g1_query"])


@pytest.mark.parametrize("circ", dr.CIRCUITS, ids=lambda c: c.name)
def test_cases_verify_in_the_exponent_and_are_the_oracles_proofs(co, circ):
    st = dr.statement(co, circ)
    keys = keys_of(co, circ)
    cases = dr.prover_cases(circ.cid, circ)
    ref = dr.reference_proofs(co, circ)
    names = [c.name for c in cases]
    for must in ("random", "no_zk", "r0", "s0", "ones", "top", "A_inf", "B_inf", "AB_inf", "C_inf", "sA_eq_rB1", "sA_opp_rB1", "t1_eq_l",
                 "t1_opp_l", "t2_eq_h", "l_inf"):
        assert must in names
    assert sum(n.startswith("nibbles") for n in names) == 6
    pub = np.ascontiguousarray(st.r1cs.z[1:st.ni])
    for c in cases:
        assert (c.u * c.v - st.alpha * st.beta - st.S - c.w * st.delta) % st.q == 0, c.name
        rs = dr.mont(co, circ.cid, [c.r, c.s])
        proof, inf = co.groth16_prove(keys, st.r1cs, rs[0], rs[1], nthreads=4)
        want, winf = ref[c.name]
        assert [bool(f) for f in winf] == [c.u == 0, c.v == 0, c.w == 0], c.name
        assert np.array_equal(inf, winf), (c.name, inf, winf)
        w1, w2 = co.point_words(circ.cid, 1), co.point_words(circ.cid, 2)
        for lo, hi, k in ((0, w1, 0), (w1, w1 + w2, 1), (w1 + w2, 2 * w1 + w2, 2)):
            assert winf[k] or np.array_equal(proof[lo:hi], want[lo:hi]), (c.name, k)
        if not winf.any():
            assert co.groth16_verify(keys, pub, want, np.ascontiguousarray(winf)), c.name
    flagged = {n for n in names if ref[n][1].any()}
    assert flagged == {"A_inf", "B_inf", "AB_inf", "C_inf"}


def test_pure_python_prover_agrees_on_the_six_constraint_circuit(co):
    """oracle/pyoracle.py groth16_prove (affine textbook group law, naive MSMs) on curve 0, every case"""
    circ = dr.TINY
    st = dr.statement(co, circ)
    keys = keys_of(co, circ)
    curve = O.CURVES[0]
    pk = {}
    for name, grp in (("alpha_g1", 1), ("beta_g1", 1), ("delta_g1", 1), ("beta_g2", 2), ("delta_g2", 2)):
        pk[name] = O.unpack_points(curve, grp, getattr(keys, name))[0]
    for name, grp, flags in (("a_query", 1, "a_inf"), ("b_g1_query", 1, "b_g1_inf"), ("b_g2_query", 2, "b_g2_inf"), ("h_query", 1, "h_inf"),
                             ("l_query", 1, "l_inf")):
        pk[name] = O.unpack_points(curve, grp, getattr(keys, name), getattr(keys, flags))
    ref = dr.reference_proofs(co, circ)
    for c in dr.prover_cases(0, circ):
        A, B, C = O.groth16_prove(curve, pk, st.py, c.r, c.s)
        want, winf = ref[c.name]
        w1, w2 = co.point_words(0, 1), co.point_words(0, 2)
        wa = O.unpack_points(curve, 1, want[:w1], winf[0:1])[0]
        wb = O.unpack_points(curve, 2, want[w1:w1 + w2], winf[1:2])[0]
        wc = O.unpack_points(curve, 1, want[w1 + w2:], winf[2:3])[0]
        assert (A, B, C) == (wa, wb, wc), c.name


@pytest.mark.parametrize("cid,grp", [(0, 1), (1, 2)])
@pytest.mark.parametrize("c", [6, 11])
def test_msm_families_have_the_sums_the_integers_say(co, cid, grp, c):
    q = dr.scalar_modulus(cid)
    for inp in dr.msm_cases(cid, grp, c):
        xy, inf = dr.dlog_bases(co, cid, grp, inp.ks)
        got = co.to_affine(cid, grp, co.msm(cid, grp, xy, dr.scalar_words(cid, inp.scalars), inf=inf, nthreads=4))
        want_xy, want_inf = dr.expected_msm(co, cid, grp, inp.ks, inp.scalars)
        assert bool(got[1][0]) == bool(want_inf) and (want_inf or np.array_equal(got[0][0], want_xy)), inp.name
        total = sum(s * k for s, k in zip(inp.scalars, inp.ks)) % q
        assert (total == 0) == bool(want_inf) == (inp.name in ("total_cancels", "horner_opposite")), inp.name


@pytest.mark.parametrize("cid,c", [(cid, c) for cid in range(4) for c in (6, 11)] + [(0, 18)])
def test_small_dlog_conditions(cid, c):
    """the builder's conditions, recounted here from the input alone (c = 18 is run on MNT4-298 G1 only); prints the seed and the counts"""
    for n in (600, 5000):
        sd = dr.small_dlog(cid, c, n)
        counts = dr.coincidence_counts(sd.input.ks, sd.input.scalars, c)
        print(f"small_dlog cid={cid} c={c} n={n}: seed {sd.seed}, {counts}")
        assert counts == sd.counts and min(counts.values()) >= 5
        assert sd.input.scalars.count(1) == 100 and sd.input.scalars.count(0) == 100
        assert set(sd.input.ks) <= {-4, -3, -2, -1, 1, 2, 3, 4} and len(set(sd.input.scalars)) > 40
        lim = 1 << (c - 1)
        assert all(2 <= d < lim for s in set(sd.input.scalars) if s > 1 for d in dr.digits_of(s, c))


def test_run_lengths_follow_the_chunk_rule():
    """the derived N of family 3: more than big_limit = 8 chunks of 33, and more than seg_len = 128 of them"""
    assert (dr.RUN_N_BIG, dr.RUN_N_TWO_SEGMENTS) == (265, 4225)
    for N, pieces in ((dr.RUN_N_BIG, 8), (dr.RUN_N_TWO_SEGMENTS, 128)):
        for start in range(33):   # wherever the run starts in its first chunk
            assert (start + N - 1) // 33 + 1 > pieces
        assert any((start + N - 2) // 33 + 1 <= pieces for start in range(33))   # and N - 1 would not do
