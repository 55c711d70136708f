"""GPU: K12 -- the second sumcheck.  pcdhip_marlin_sumcheck2_q bit-exact on the ABI Montgomery words against exact integers
(tests/marlin_sumcheck2_reference.py) and, word for word, against the device composition it replaces (sumcheck_ab, vec_mul,
poly_lincomb); the driver pcdhip_marlin_sumcheck2 under both routes against the reference's chain, on a B that the rule makes too
short for route 1, and chained into kzg_commit without a download.  Domain elements and transforms come from the oracle."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marlin_index_reference as mir  # noqa: E402
import marlin_reference as mr  # noqa: E402
import marlin_sumcheck2_reference as m2  # noqa: E402
from test_gpu_marlin_index import planted  # noqa: E402
from test_gpu_marlin_rounds import domain, free, mont, r1cs_of, sumcheck_case, up3, upload  # noqa: E402
from test_marlin_sumcheck2_host import planted_cases  # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    from pcd_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def co():
    from oracle import coracle
    return coracle


def composed_q(ctx, co, field, am, bm, cm, brow, bcol, rc_bufs, bval, bf):
    """q from the launches the fused kernel replaces: a and b stored, b f stored, a - b f"""
    p = mr.MODULI[field]
    a, b = ctx.marlin_sumcheck_ab(am, bm, cm, brow, bcol, rc_bufs, bval)
    prod = ctx.vec_mul(b, bf)
    out = ctx.buf_alloc(field, a.n)
    ctx.poly_lincomb([a, prod], mont(co, field, [1, p - 1]), out)
    words = out.download()
    free(a, b, prod, out)
    return words


# --------------------------------------------------------------------------------------------------------------- the fused kernel
@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_sumcheck2_q_bit_exact(ctx, co, field):
    rnd = random.Random(1300 + field)
    p = mr.MODULI[field]
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
        alpha, beta, coeff, row, col, val = sumcheck_case(rnd, field, n)
        f = [rnd.randrange(p) for _ in range(n)]
        prod = [[r * c % p for r, c in zip(row[m], col[m])] for m in range(3)]
        other = [[rnd.randrange(p) for _ in range(n)] for _ in range(3)]  # NOT row * col: the four-term form is what gets checked
        am, bm, cm = mont(co, field, [alpha])[0], mont(co, field, [beta])[0], mont(co, field, coeff)
        brow, bcol, bval, bprod, bother = (up3(ctx, co, field, v) for v in (row, col, val, prod, other))
        bf = upload(ctx, co, field, f)
        results = {}
        for name, rc_ints, rc_bufs in (("null", None, None), ("product", prod, bprod), ("given", other, bother)):
            want = mont(co, field, m2.sumcheck2_q(alpha, beta, coeff, row, col, rc_ints, val, f, p))
            q = ctx.marlin_sumcheck2_q(am, bm, cm, brow, bcol, rc_bufs, bval, bf)
            results[name] = q.download()
            assert q.n == n and np.array_equal(results[name], want), (field, n, name)
            if n:
                assert np.array_equal(results[name], composed_q(ctx, co, field, am, bm, cm, brow, bcol, rc_bufs, bval, bf)), (field, n, name)
            q.free()
        assert np.array_equal(results["null"], results["product"])
        if n == 257:  # entries of row_col all null are the null array; the inputs are left alone; in place over f
            q = ctx.marlin_sumcheck2_q(am, bm, cm, brow, bcol, [None, None, None], bval, bf)
            assert np.array_equal(q.download(), results["null"])
            q.free()
            for bufs, ints in ((brow, row), (bcol, col), (bval, val), (bother, other)):
                for m in range(3):
                    assert np.array_equal(bufs[m].download(), mont(co, field, ints[m]))
            assert np.array_equal(bf.download(), mont(co, field, f))
            assert ctx.marlin_sumcheck2_q(am, bm, cm, brow, bcol, bother, bval, bf, out=bf) is bf
            assert np.array_equal(bf.download(), results["given"])
        free(bf, *brow, *bcol, *bval, *bprod, *bother)


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_sumcheck2_q_planted_cases(ctx, co, field):
    """every input 0, every input p - 1, d_A = 0, f = 0 and a random list, with and without row_col"""
    rnd = random.Random(1310 + field)
    p = mr.MODULI[field]
    for name, alpha, beta, coeff, row, col, rc, val, f in planted_cases(rnd, p):
        am, bm, cm = mont(co, field, [alpha])[0], mont(co, field, [beta])[0], mont(co, field, coeff)
        brow, bcol, brc, bval = (up3(ctx, co, field, v) for v in (row, col, rc, val))
        bf = upload(ctx, co, field, f)
        for rc_ints, rc_bufs in ((rc, brc), (None, None)):
            want = mont(co, field, m2.sumcheck2_q(alpha, beta, coeff, row, col, rc_ints, val, f, p))
            q = ctx.marlin_sumcheck2_q(am, bm, cm, brow, bcol, rc_bufs, bval, bf)
            got = q.download()
            assert np.array_equal(got, want), (field, name, rc_ints is not None)
            assert np.array_equal(got, composed_q(ctx, co, field, am, bm, cm, brow, bcol, rc_bufs, bval, bf)), (field, name)
            q.free()
        free(bf, *brow, *bcol, *brc, *bval)


def test_sumcheck2_q_argument_errors(ctx, co):
    from pcd_amd import capi
    field, n = 1, 9
    rnd = random.Random(1320)
    p = mr.MODULI[field]
    alpha, beta, coeff, row, col, val = sumcheck_case(rnd, field, n)
    f = [rnd.randrange(p) for _ in range(n)]
    am, bm, cm = mont(co, field, [alpha])[0], mont(co, field, [beta])[0], mont(co, field, coeff)
    brow, bcol, bval, brc = (up3(ctx, co, field, v) for v in (row, col, val, row))
    bf = upload(ctx, co, field, f)
    o1, small, wrong = ctx.buf_alloc(field, n), ctx.buf_alloc(field, n - 1), ctx.buf_alloc(0, n)
    q2 = lambda out, rc=None, k=None, ff=bf, cols=bcol: ctx.marlin_sumcheck2_q(am, bm, cm, brow, cols, rc, bval, ff, n=k, out=out)
    bad = [
        lambda: q2(brow[1]), lambda: q2(bcol[2]), lambda: q2(bval[0]), lambda: q2(brc[1], rc=brc),   # the output on an index vector
        lambda: q2(small), lambda: q2(o1, ff=small, k=n),                                               # short buffers
        lambda: q2(wrong), lambda: q2(o1, ff=wrong), lambda: q2(o1, cols=[bcol[0], bcol[1], wrong]),    # mixed fields
        lambda: q2(o1, rc=[brc[0], brc[1], wrong]),
        lambda: q2(o1, rc=[brc[0], None, brc[2]]),                                                      # mixed null row_col
        lambda: q2(o1, k=n + 1),                                                                        # n beyond a buffer
    ]
    for fn in bad:
        with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
            fn()
    lib = capi.lib()
    three = ctx._three
    assert lib.pcdhip_marlin_sumcheck2_q(ctx._ctx, None, bm.ctypes.data, cm.ctypes.data, three(brow), three(bcol), None, three(bval), bf._h, n,
                                         o1._h) == E_ARG
    assert lib.pcdhip_marlin_sumcheck2_q(ctx._ctx, am.ctypes.data, bm.ctypes.data, cm.ctypes.data, three(brow), three(bcol), None, three(bval),
                                         None, n, o1._h) == E_ARG
    assert np.array_equal(brow[1].download(), mont(co, field, row[1])) and np.array_equal(bf.download(), mont(co, field, f))
    q2(o1)  # and the well-formed call goes through
    assert np.array_equal(o1.download(), mont(co, field, m2.sumcheck2_q(alpha, beta, coeff, row, col, None, val, f, p)))
    free(o1, small, wrong, bf, *brow, *bcol, *bval, *brc)


# ----------------------------------------------------------------------------------------------------------------------- the driver
H_N, X_N, K_N, B_N = 64, 4, 256, 1024
ROWS, COLS = 60, 64
_CASE = {}


def oracle_transforms(co, field):
    """(interp, extend) for marlin_sumcheck2_reference.sumcheck2 by the oracle's transforms over radix-2 or mixed-radix domains"""
    def interp(evals, dom, p):
        return mr.to_ints(co, field, mir.transform(co, field, mont(co, field, evals), inverse=True))

    def extend(coeffs, dom, p):
        return mr.to_ints(co, field, mir.transform(co, field, mont(co, field, list(coeffs) + [0] * (len(dom) - len(coeffs)))))
    return interp, extend


def driver_case(co, field):
    """the planted matrices of test_rounds_from_the_index with the reference's second sumcheck over them: computed once per field"""
    if field not in _CASE:
        rnd = random.Random(1080 + field)
        p = mr.MODULI[field]
        dom_h = domain(co, field, H_N)
        mats = [planted(rnd, p, ROWS, COLS, rnd.randrange(200, 256)) for _ in range(3)]
        alpha, beta = rnd.randrange(p), rnd.randrange(p)
        assert pow(alpha, H_N, p) != 1 and pow(beta, H_N, p) != 1
        eta = [1, rnd.randrange(p), rnd.randrange(p)]
        vh = (pow(alpha, H_N, p) - 1) * (pow(beta, H_N, p) - 1) % p
        coeff = [e * vh % p for e in eta]
        per_matrix = [mir.arithmetize(m, dom_h, H_N, X_N, K_N, p) for m in mats]
        on_k = tuple([per_matrix[m][q] for m in range(3)] for q in range(4))
        interp, extend = oracle_transforms(co, field)
        ref = m2.sumcheck2(alpha, beta, coeff, on_k, domain(co, field, K_N), domain(co, field, B_N), p, interp, extend)
        _CASE[field] = (mats, alpha, beta, coeff, ref)
    return _CASE[field]


def free_outputs(d):
    free(*[v for k, v in d.items() if k not in ("lens", "route")])


@pytest.mark.parametrize("field", [1, 3])
def test_driver_bit_exact_under_both_routes(ctx, co, field):
    mats, alpha, beta, coeff, ref = driver_case(co, field)
    one = lambda x: mont(co, field, [x])[0]
    idx = ctx.marlin_index_build(field, r1cs_of(co, field, mats, ROWS, COLS), H_N, X_N, keep=6)
    assert (idx.info()["domain_k_n"], idx.info()["domain_b_n"]) == (K_N, B_N)
    assert ref["rem"] == [0] * K_N and any(ref["h2"]) and any(ref["g2"])
    h2 = {}
    for route in (0, 1, 2):
        out = ctx.marlin_sumcheck2(idx, one(alpha), one(beta), mont(co, field, coeff), route=route)
        assert out["lens"] == [K_N - 1, 3 * K_N - 3] and out["route"] == (route or 1)
        assert (out["f_poly"].n, out["g2"].n, out["sigma"].n, out["h2"].n, out["h2_rem"].n) == (K_N, K_N - 1, 1, 3 * K_N - 3, K_N)
        for name in ("f_poly", "g2", "h2"):
            assert np.array_equal(out[name].download(), mont(co, field, ref[name])), (field, route, name)
        assert np.array_equal(out["sigma"].download(), mont(co, field, [ref["sigma"]])), (field, route)
        assert not out["h2_rem"].download().any(), (field, route)
        h2[route] = out["h2"].download()
        free_outputs(out)
    assert np.array_equal(h2[1], h2[2]) and np.array_equal(h2[0], h2[1])
    # f_poly and h2_rem are optional
    for route in (1, 2):
        out = ctx.marlin_sumcheck2(idx, one(alpha), one(beta), mont(co, field, coeff), route=route, want_f_poly=False, want_rem=False)
        assert out["f_poly"] is None and out["h2_rem"] is None and out["route"] == route
        assert np.array_equal(out["h2"].download(), h2[1]) and np.array_equal(out["g2"].download(), mont(co, field, ref["g2"]))
        assert np.array_equal(out["sigma"].download(), mont(co, field, [ref["sigma"]]))
        free_outputs(out)
    idx.free()


def test_driver_refusals_leave_the_outputs_unwritten(ctx, co):
    from pcd_amd import capi
    field = 1
    mats, alpha, beta, coeff, _ = driver_case(co, field)
    L = mr.LIMBS[field]
    r1cs = r1cs_of(co, field, mats, ROWS, COLS)
    am, bm, cm = mont(co, field, [alpha])[0], mont(co, field, [beta])[0], mont(co, field, coeff)
    pattern = lambda n: np.full((n, L), 0x5A5A5A5A, dtype=np.uint64)
    sizes = (K_N, K_N - 1, 1, 3 * K_N - 3, K_N)  # f_poly, g2, sigma, h2, h2_rem
    outs = [ctx.buf_upload(field, pattern(n)) for n in sizes]
    lib = capi.lib()

    def call(idx, route, bufs=outs):
        lens = (C.c_size_t * 3)(7, 7, 7)
        rc = lib.pcdhip_marlin_sumcheck2(ctx._ctx, idx._h, am.ctypes.data, bm.ctypes.data, cm.ctypes.data, route, *[b._h if b is not None else None for b in bufs],
                                         lens)
        return rc, list(lens)

    refused = []
    for keep in (1, 2):  # the coefficients alone; the evaluations on K alone
        idx = ctx.marlin_index_build(field, r1cs, H_N, X_N, keep=keep)
        refused += [call(idx, route) for route in (0, 1, 2)]
        idx.free()
    same = ctx.marlin_index_build(field, r1cs, H_N, X_N, domain_k_n=K_N, domain_b_n=K_N, keep=6)  # |B| = |K| < 3 |K| - 2
    refused += [call(same, 1), call(same, 2), call(same, 0)]
    same.free()
    idx = ctx.marlin_index_build(field, r1cs, H_N, X_N, keep=6)
    short = ctx.buf_alloc(field, 3 * K_N - 4)
    wrong = ctx.buf_alloc(0, K_N)
    refused += [call(idx, 3), call(idx, -1), call(idx, 0, [outs[0], outs[1], None, outs[3], outs[4]]),
                call(idx, 0, [outs[0], outs[1], outs[2], short, outs[4]]), call(idx, 0, [wrong] + outs[1:]),
                call(idx, 0, [outs[0], outs[1], outs[2], outs[3], outs[0]])]
    assert refused == [(E_ARG, [7, 7, 7])] * len(refused)
    for b, n in zip(outs, sizes):
        assert np.array_equal(b.download(), pattern(n))
    rc, lens = call(idx, 0)  # and the well-formed call goes through
    assert rc == 0 and lens == [K_N - 1, 3 * K_N - 3, 1]
    assert not outs[4].download().any() and outs[3].download().any()
    free(short, wrong, *outs)
    idx.free()


def test_driver_takes_route_2_on_the_rules_short_b(ctx, co):
    """field 2 (2-adicity 15) with |K| = 2^15: the rule's |B| is mixed-radix and below 4 |K| - 3, so route 1 cannot run there"""
    from pcd_amd import capi
    field = 2
    rnd = random.Random(1340)
    p = mr.MODULI[field]
    h_n, x_n, k_n = 1024, 4, 1 << 15
    rows = cols = h_n
    mats = [[(r, rnd.randrange(cols), rnd.choice([1, p - 1, 2, rnd.randrange(p)])) for r in range(rows) for _ in range(20 - m)] for m in range(3)]
    b_n = co.domain_size(field, 3 * k_n - 3)
    assert b_n == 25 << 12 and 3 * k_n - 2 <= b_n < 4 * k_n - 3
    alpha, beta = rnd.randrange(p), rnd.randrange(p)
    assert pow(alpha, h_n, p) != 1 and pow(beta, h_n, p) != 1
    coeff = [rnd.randrange(1, p) for _ in range(3)]
    one = lambda x: mont(co, field, [x])[0]
    idx = ctx.marlin_index_build(field, r1cs_of(co, field, mats, rows, cols), h_n, x_n)
    assert (idx.info()["domain_k_n"], idx.info()["domain_b_n"]) == (k_n, b_n)
    with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
        ctx.marlin_sumcheck2(idx, one(alpha), one(beta), mont(co, field, coeff), route=1)
    out = ctx.marlin_sumcheck2(idx, one(alpha), one(beta), mont(co, field, coeff))
    assert out["route"] == 2 and out["lens"] == [k_n - 1, 3 * k_n - 3]
    assert not out["h2_rem"].download().any()
    ints = lambda buf: mr.to_ints(co, field, buf.download())
    f_poly, h2 = ints(out["f_poly"]), ints(out["h2"])
    assert ints(out["sigma"]) == f_poly[:1] and ints(out["g2"]) == f_poly[1:] and any(f_poly[1:]) and any(h2)
    polys = [[ints(idx.vec(0, m, q)) for m in range(3)] for q in range(4)]
    z = rnd.randrange(p)
    a_z, b_z = m2.ab_at(alpha, beta, coeff, polys, z, p)
    assert mr.horner(h2, z, p) * (pow(z, k_n, p) - 1) % p == (a_z - b_z * mr.horner(f_poly, z, p)) % p
    free_outputs(out)
    idx.free()


@pytest.mark.parametrize("field", [1, 3])
def test_chain_without_downloads_commits_match(ctx, co, field):
    """marlin_index_build -> marlin_sumcheck2 -> kzg_commit of g_2 and h_2 with nothing downloaded in between; the commitments equal
    those of the reference's coefficients uploaded afresh"""
    curve = {1: 0, 3: 2}[field]  # the curve whose scalar field this is
    mats, alpha, beta, coeff, ref = driver_case(co, field)
    one = lambda x: mont(co, field, [x])[0]
    idx = ctx.marlin_index_build(field, r1cs_of(co, field, mats, ROWS, COLS), H_N, X_N, keep=6)
    powers = ctx.bases_upload(curve, 1, co.gen_points(curve, 1, 3 * K_N, seed=1351))
    out = ctx.marlin_sumcheck2(idx, one(alpha), one(beta), mont(co, field, coeff), want_f_poly=False, want_rem=False)
    comm, inf, _, _, _ = ctx.kzg_commit(powers, [{"poly": out["g2"]}, {"poly": out["h2"]}])
    fresh = [upload(ctx, co, field, ref["g2"]), upload(ctx, co, field, ref["h2"])]
    want, want_inf, _, _, _ = ctx.kzg_commit(powers, [{"poly": b} for b in fresh])
    assert np.array_equal(comm, want) and np.array_equal(inf, want_inf) and not inf.any()
    assert comm[0].tobytes() != comm[1].tobytes()
    free(*fresh)
    free_outputs(out)
    powers.free(), idx.free()
