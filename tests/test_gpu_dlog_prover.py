"""GPU: pcdhip_groth16_prove at coinciding operands.  The blinding factors r, s of tests/dlog_reference.py prover_cases make an operand of
the proof's assembly (pcd_amd/csrc/inst_g16.hip: g16_finish adds s A + r B_1, then M_l', then M_h; g16_scale_point scales A and B_1 in the
chained form, two more MSMs do in the folded form) the identity, or equal or opposite to the other operand; r = s = 0 is ark-groth16's
create_proof_no_zk.  The expected proof is arithmetic mod the scalar modulus plus one fixed-base multiple per point, independent of the
C++ oracle's prover (which agrees: tests/test_dlog_reference_host.py).  Bit-exact on the affine C-ABI image and the infinity flags."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dlog_reference as dr  # noqa: E402

pytestmark = pytest.mark.gpu

SUBSET = ("A_inf", "C_inf", "sA_eq_rB1", "sA_opp_rB1", "no_zk")
_KEYS = {}


def keys_of(co, circ):
    if circ.name not in _KEYS:
        st = dr.statement(co, circ)
        _KEYS[circ.name] = co.groth16_setup(circ.cid, st.r1cs, st.toxic_mont(), nthreads=8)
    return _KEYS[circ.name]


def check(co, ctx, pk, circ, case, resident, what):
    st = dr.statement(co, circ)
    want, winf = dr.reference_proofs(co, circ)[case.name]
    rs = dr.mont(co, circ.cid, [case.r, case.s])
    proof, inf = ctx.groth16_prove(pk, st.r1cs, rs[0], rs[1], resident_r1cs=resident)
    assert np.array_equal(inf, winf), (circ.name, case.name, what, resident, list(inf), list(winf))
    assert np.array_equal(proof, want), (circ.name, case.name, what, resident)


@pytest.mark.parametrize("assembly", [1, 2, 0], ids=["folded", "chained", "auto"])
@pytest.mark.parametrize("circ", dr.CIRCUITS, ids=lambda c: c.name)
def test_every_case_in_every_assembly_form(co, gpu_ctx, circ, assembly):
    """every case x (matrices handed over, resident); the key is a real one (identities where no row mentions a variable)"""
    st = dr.statement(co, circ)
    cases = dr.prover_cases(circ.cid, circ)
    pk = gpu_ctx.g16_pk_upload(keys_of(co, circ).host_struct(), circ.cid)
    try:
        gpu_ctx.groth16_set_assembly(assembly)
        for c in cases:
            check(co, gpu_ctx, pk, circ, c, False, assembly)
        gpu_ctx.g16_pk_set_r1cs(pk, st.r1cs)
        for c in cases:
            check(co, gpu_ctx, pk, circ, c, True, assembly)
    finally:
        gpu_ctx.groth16_set_assembly(0)
        pk.free()


def subset(cid):
    circ = dr.circuit_of(cid)
    return circ, [c for c in dr.prover_cases(cid, circ) if c.name in SUBSET]


@pytest.mark.parametrize("cid", [0, 2])
def test_subset_on_the_accumulate_lane_schedule(co, gpu_ctx, cid):
    circ, cases = subset(cid)
    assert len(cases) == len(SUBSET)
    pk = gpu_ctx.g16_pk_upload(keys_of(co, circ).host_struct(), cid)
    try:
        gpu_ctx.groth16_set_schedule(2)
        for assembly in (1, 2):
            gpu_ctx.groth16_set_assembly(assembly)
            for c in cases:
                check(co, gpu_ctx, pk, circ, c, False, ("schedule 2", assembly))
    finally:
        gpu_ctx.groth16_set_schedule(0)
        gpu_ctx.groth16_set_assembly(0)
        pk.free()


@pytest.mark.parametrize("cid", [0, 2])
def test_subset_on_the_sparse_window_copies(co, gpu_ctx, cid):
    """a witness-like circuit (at most an eighth of its assignment is neither 0 nor 1) under a key uploaded with the second, 6-bit
    layout of its assignment queries: the chained form runs every checked proof on those copies, the folded form never does"""
    circ = dr.WITNESS_CIRCUITS[cid]
    st = dr.statement(co, circ)
    cases = [c for c in dr.prover_cases(cid, circ) if c.name in SUBSET]
    assert len(cases) == len(SUBSET)
    pk = None
    try:
        gpu_ctx.groth16_set_sparse_window(6)
        pk = gpu_ctx.g16_pk_upload(keys_of(co, circ).host_struct(), cid)
        assert gpu_ctx.g16_pk_memory(pk)["sparse_window"] > 0
        for assembly, sparse in ((2, True), (1, False)):
            gpu_ctx.groth16_set_assembly(assembly)
            for c in cases:
                check(co, gpu_ctx, pk, circ, c, False, ("sparse window 6", assembly))
                used, counted = gpu_ctx.groth16_last_plan()
                assert used == sparse and counted == (st.general if sparse else 0), (c.name, assembly, used, counted, st.general)
    finally:
        gpu_ctx.groth16_set_sparse_window(0)
        gpu_ctx.groth16_set_assembly(0)
        if pk is not None:
            pk.free()


@pytest.mark.parametrize("cid", [0, 2])
def test_subset_on_two_shards(co, gpu_ctx, cid):
    """a two-shard context (two logical shards of one device when only one is visible): the partial results of the shards are summed by
    jac_sum_parts before the assembly -- with A_inf the shards' partials of A are opposite"""
    from pcd_amd import capi
    ndev = capi.lib().pcdhip_device_count()
    _devices = lambda k: [i % ndev for i in range(k)]   # as in tests/test_gpu_multi_device.py
    circ, cases = subset(cid)
    st = dr.statement(co, circ)
    mctx = capi.Context(devices=_devices(2))
    try:
        mpk = mctx.g16_pk_upload(keys_of(co, circ).host_struct(), cid)
        for c in cases:
            check(co, mctx, mpk, circ, c, False, "two shards")
        mctx.g16_pk_set_r1cs(mpk, st.r1cs)
        for c in cases:
            check(co, mctx, mpk, circ, c, True, "two shards")
        mpk.free()
    finally:
        mctx.close()


def _as_int(limbs):
    return sum(int(w) << (64 * k) for k, w in enumerate(limbs))


@pytest.mark.parametrize("cid", [0, 3])
def test_unreduced_blinding_factors_are_refused(co, gpu_ctx, cid):
    """r_mont or s_mont whose C-ABI image, read as an integer, is not below the modulus: PCDHIP_E_ARG (include/pcdhip.h), and the next
    call is clean"""
    from pcd_amd import capi
    circ = dr.circuit_of(cid)
    st = dr.statement(co, circ)
    case = dr.prover_cases(cid, circ)[0]
    rs = dr.mont(co, cid, [case.r, case.s])
    q, L = st.q, rs.shape[1]
    images = [_as_int(rs[0]) + q, q, (1 << (64 * L)) - 1]
    assert all(q <= x < 1 << (64 * L) for x in images)
    pk = gpu_ctx.g16_pk_upload(keys_of(co, circ).host_struct(), cid)
    try:
        for x in images:
            bad = dr.scalar_words(cid, [x])[0]
            for r_m, s_m in ((bad, rs[1]), (rs[0], bad)):
                with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
                    gpu_ctx.groth16_prove(pk, st.r1cs, r_m, s_m)
        top = dr.scalar_words(cid, [q - 1])[0]   # the largest reduced image is an element like any other
        proof, _ = gpu_ctx.groth16_prove(pk, st.r1cs, top, rs[1])
        assert proof.any()
        check(co, gpu_ctx, pk, circ, case, False, "after the refusals")
    finally:
        pk.free()
