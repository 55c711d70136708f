"""GPU: the public-input accumulation of the Groth16 verifications, acc = gamma_abc[0] + sum_j x_j gamma_abc[j], at its edges -- several
trips per lane of fb_inputs_kernel, the doubling / opposite-point / infinity branches of its tree over the lanes, an infinite
accumulation on both pairing routes, flagged infinities in the key and in the proof, the fallback without window tables, the
random-linear-combination route, edge scalars, and unreduced encodings -- through all four entry points and both forms of the pairing
kernels.  The cases and their verdicts come from tests/verify_reference.py (trapdoor keys: known by construction; the C++ oracle agrees
with every one of them in tests/test_verify_inputs_host.py).  Exact booleans, no tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_reference as vr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 1], ids=["wave-per-pairing", "lane-per-pairing"])
def pmode(request, gpu_ctx):
    """both forms of the pairing kernels behind the same entry points (pcdhip_pairing_set_mode), as in tests/test_gpu_pairing_kzg.py"""
    gpu_ctx.pairing_set_mode(request.param)
    yield request.param
    gpu_ctx.pairing_set_mode(0)


def _rho(k, seed):
    return np.random.default_rng(seed).integers(1, 1 << 62, size=(k, 2), dtype=np.uint64)


def _pubs(b):
    return np.stack(b.pubs)   # (members, ni - 1, L)


CASES = [(cid, c.name) for cid in range(4) for c in vr.cases(cid)]


# One test per entry point, so that each stays at a few seconds where a launch is slowest: one lane-per-pairing verification on a 753-bit
# curve is a single-lane kernel of 0.3 s, and groth16_verify is three of them per member (process_vk pairs alpha with beta and takes
# GT's one).  Measured on an MI355X, slowest first: groth16_verify, lane-per-pairing -- 2.2 to 3.0 s per case on MNT6-753, 1.7 s on
# MNT4-753; prepared_and_rlc there 1.6 s; everything in wave-per-pairing mode and everything on the 298-bit curves under 1.3 s.  The 64
# window tables of equal_lanes / opposite_lanes (333 MB on a 753-bit key) are not the slow spot: five process_vk calls on such a key and
# all the verifications of the case took 0.9 s together in wave-per-pairing mode on MNT6-753 (2.3 s for groth16_verify in
# lane-per-pairing mode, no more than cases of three inputs), so these cases keep their 64 bases on every curve.
@pytest.mark.parametrize("entry", ["verify", "verify_batch", "prepared_and_rlc"])
@pytest.mark.parametrize("cid,name", CASES, ids=lambda v: str(v))
def test_entry_points_agree_with_the_case_list(co, gpu_ctx, pmode, cid, name, entry):
    case = vr.case_named(cid, name)
    b = vr.build(co, cid, case)
    key, want, n = b.key, b.expect, len(case.members)
    pubs = _pubs(b)
    ginf = key.gamma_abc_inf
    if entry == "verify":
        single = np.array([gpu_ctx.groth16_verify(*key.args(), b.pubs[i], b.proofs[i], gamma_abc_inf=ginf, proof_inf=b.proofs_inf[i]) for i in range(n)])
        assert np.array_equal(single, want), single
        return
    if entry == "verify_batch":
        batch = gpu_ctx.groth16_verify_batch(*key.args(), pubs, b.proofs, gamma_abc_inf=ginf, proofs_inf=b.proofs_inf)
        assert np.array_equal(batch, want), batch
        return
    pvk = gpu_ctx.process_vk(*key.args(), gamma_abc_inf=ginf)
    try:
        prepared = gpu_ctx.groth16_verify_prepared(pvk, pubs, b.proofs, proofs_inf=b.proofs_inf)
        assert np.array_equal(prepared, want), prepared
        # the random linear combination: the accepting members alone, then with ONE rejecting member behind them (a changed input
        # where the case has inputs)
        good = np.flatnonzero(want)
        assert gpu_ctx.groth16_verify_batch_rlc(pvk, pubs[good], b.proofs[good], _rho(len(good), 5), proofs_inf=b.proofs_inf[good]) is True
        if not want.all():
            idx = np.append(good, np.flatnonzero(~want)[0])
            assert gpu_ctx.groth16_verify_batch_rlc(pvk, pubs[idx], b.proofs[idx], _rho(len(idx), 6), proofs_inf=b.proofs_inf[idx]) is False
    finally:
        pvk.free()


@pytest.mark.parametrize("cid", [0, 3])
def test_one_batch_many_shapes(co, gpu_ctx, pmode, cid):
    """70 proofs under the `edges` key in ONE prepared verification (more than one wave of workgroups in the accumulation, 3 k > 64
    pairings), every proof with its own input vector drawn from the edge values, six of them submitted with one input changed; then the
    same batch reversed, which a result written to the wrong proof's slot cannot survive"""
    k = 70
    case = vr.case_named(cid, "edges")
    key = vr.build(co, cid, case).key
    r, vals = key.r, vr.edge_values(cid)
    g = np.random.default_rng(700 + cid)
    proved = [[vals[i] for i in g.integers(0, len(vals), size=key.num_inputs - 1)] for _ in range(k)]
    proved[0], proved[k - 1] = vals, vals[::-1]
    sent = [list(xs) for xs in proved]
    bad = [3, 17, 31, 32, 64, 69]
    for n, i in enumerate(bad):
        j = (n * 3) % (key.num_inputs - 1)
        sent[i][j] = next(v for v in vals[n % len(vals):] + vals if v != proved[i][j])
    want = np.array([key.S(s) == key.S(p) for s, p in zip(sent, proved)])
    assert list(np.flatnonzero(~want)) == bad          # (every s_j of the key is non-zero: a changed input changes S)
    proofs, pinf = vr.trapdoor_proofs(co, key, proved, seed="many shapes")
    assert not pinf.any()
    pubs = np.stack([vr.scalar_words(cid, xs) for xs in sent])
    pvk = gpu_ctx.process_vk(*key.args(), gamma_abc_inf=key.gamma_abc_inf)
    try:
        got = gpu_ctx.groth16_verify_prepared(pvk, pubs, proofs, proofs_inf=pinf)
        assert np.array_equal(got, want), np.flatnonzero(got != want)
        rev = gpu_ctx.groth16_verify_prepared(pvk, pubs[::-1].copy(), proofs[::-1].copy(), proofs_inf=pinf[::-1].copy())
        assert np.array_equal(rev, want[::-1]), np.flatnonzero(rev != want[::-1])
    finally:
        pvk.free()


def test_routes_agree_at_the_table_limit(co, gpu_ctx, pmode):
    """PVK_TABLE_INPUTS = 256: the key with 256 inputs accumulates through its window tables, the key with 257 has none and runs one MSM
    per proof.  Both give the case list's verdicts; and with the SAME trapdoor, the same s and x prefix and x_256 = 0 the two
    accumulations are the same point, so one proof has to pass under both keys -- and fail under the longer one once x_256 = 1."""
    cid = 0
    lo, hi = vr.case_named(cid, "table_limit_256"), vr.case_named(cid, "table_limit_257")
    assert len(lo.s) == vr.TABLE_LIMIT and len(hi.s) == vr.TABLE_LIMIT + 1 and hi.s[:vr.TABLE_LIMIT] == lo.s
    keys = [vr.trapdoor_key(co, cid, c.s, seed="table limit") for c in (lo, hi)]
    assert (keys[0].a, keys[0].b, keys[0].c, keys[0].d) == (keys[1].a, keys[1].b, keys[1].c, keys[1].d)
    xs = lo.members[0].xs
    proof, pinf = vr.trapdoor_proof(co, keys[0], xs, seed="table limit")
    sent = [(keys[0], xs, True), (keys[1], xs + [0], True), (keys[1], xs + [1], False), (keys[0], xs[:-1] + [(xs[-1] + 1) % keys[0].r], False)]
    for key, x, want in sent:
        assert (key.S(x) == keys[0].S(xs)) == want
        pvk = gpu_ctx.process_vk(*key.args(), gamma_abc_inf=key.gamma_abc_inf)
        try:
            assert gpu_ctx.groth16_verify_prepared(pvk, vr.scalar_words(cid, x)[None], proof[None], proofs_inf=pinf[None])[0] == want, (key.num_inputs, want)
            assert gpu_ctx.groth16_verify_batch_rlc(pvk, vr.scalar_words(cid, x)[None], proof[None], _rho(1, 9), proofs_inf=pinf[None]) == want
        finally:
            pvk.free()
    for c in (lo, hi):   # and the case list's own members (all four entry points run them in test_entry_points_agree_with_the_case_list)
        b = vr.build(co, cid, c)
        got = gpu_ctx.groth16_verify_batch(*b.key.args(), _pubs(b), b.proofs, gamma_abc_inf=b.key.gamma_abc_inf, proofs_inf=b.proofs_inf)
        assert np.array_equal(got, b.expect), c.name


@pytest.mark.parametrize("cid,ni", [(0, 3), (0, 257), (3, 3)])
def test_non_canonical_inputs_are_refused(co, gpu_ctx, pmode, cid, ni):
    """A proof valid for x = (1, 5, ...) and x_1 submitted as r + 1, r, 1 + 2^(8 nwin) or with its top word all ones: every entry point
    raises PcdHipError.  Not True -- before the check in pcdhip_groth16_verify_prepared / _batch_rlc the window tables (ni = 3) read nwin
    digits and dropped the rest, the MSM (ni = 257) refused only what was wider than r, both took x + r for x, and r + 1 verified as 1
    (this test failed on that library with True returned).  Not False either: a caller could not tell a bad encoding from a bad proof."""
    from pcd_amd import capi
    g = vr._rng("non canonical", cid, ni)
    r = vr.scalar_modulus(cid)
    key = vr.trapdoor_key(co, cid, [g.randrange(1, r) for _ in range(ni)], seed="non canonical")
    xs = [1, 5] + [g.randrange(r) for _ in range(ni - 3)]
    proof, pinf = vr.trapdoor_proof(co, key, xs, seed="non canonical")
    other, oinf = vr.trapdoor_proof(co, key, xs, seed="another proof of the same")
    ginf = key.gamma_abc_inf
    pvk = gpu_ctx.process_vk(*key.args(), gamma_abc_inf=ginf)
    try:
        good = vr.scalar_words(cid, xs)
        two, two_inf = np.stack([other, proof]), np.stack([oinf, pinf])
        assert gpu_ctx.groth16_verify(*key.args(), good, proof, gamma_abc_inf=ginf, proof_inf=pinf) is True
        assert gpu_ctx.groth16_verify_prepared(pvk, np.stack([good, good]), two, proofs_inf=two_inf).all()
        for name, x1 in vr.non_canonical(cid):
            assert x1 >= r
            sent = vr.scalar_words(cid, [x1] + xs[1:])
            pair = np.stack([good, sent])   # the unreduced input in the SECOND proof of a batch: the check looks at every proof
            calls = {
                "groth16_verify": lambda: gpu_ctx.groth16_verify(*key.args(), sent, proof, gamma_abc_inf=ginf, proof_inf=pinf),
                "groth16_verify_batch": lambda: gpu_ctx.groth16_verify_batch(*key.args(), pair, two, gamma_abc_inf=ginf, proofs_inf=two_inf),
                "groth16_verify_prepared": lambda: gpu_ctx.groth16_verify_prepared(pvk, pair, two, proofs_inf=two_inf),
                "groth16_verify_batch_rlc": lambda: gpu_ctx.groth16_verify_batch_rlc(pvk, pair, two, _rho(2, 11), proofs_inf=two_inf),
            }
            for entry, call in calls.items():
                with pytest.raises(capi.PcdHipError):
                    got = call()
                    pytest.fail(f"{entry} returned {got} for x_1 = {name} (ni = {ni}, curve {cid}): an unreduced public input must be an error")
    finally:
        pvk.free()
