"""GPU: the K7 open side -- division by (X - z), evaluation, linear combination, KZG10::open and KZG10::check / batch_check --
against exact integers (tests/kzg_reference.py) and the oracle's group operations and pairing."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_reference as kr  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = [1024, 1024, 512, 512]  # coefficients per tile of the division kernels (poly.hip.h PolyCfg)
CURVES = [0, 1, 2, 3]


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


def rand_poly(rnd, field, n):
    p = kr.MODULI[field]
    return [rnd.randrange(p) for _ in range(n)]


def upload(ctx, co, field, ints):
    m = kr.to_mont(co, field, ints) if ints else np.zeros((0, kr.LIMBS[field]), dtype=np.uint64)
    return ctx.buf_upload(field, m)


def affine_eq(co, curve, group, a_xyz, b_xyz):
    a, ai = co.to_affine(curve, group, a_xyz)
    b, bi = co.to_affine(curve, group, b_xyz)
    return bool(ai[0] == bi[0] and (ai[0] or np.array_equal(a, b)))


def check_division(ctx, co, field, a, z):
    p = kr.MODULI[field]
    q_want, v_want = kr.div_linear(a, z, p)
    buf = upload(ctx, co, field, a)
    q, v = ctx.poly_div_linear(buf, kr.to_mont(co, field, [z])[0], length=len(a))
    assert kr.to_ints(co, field, v) == [v_want]
    if len(a) > 1:
        got = q.download()
        assert np.array_equal(got, kr.to_mont(co, field, q_want)), (field, len(a))
        q.free()
    else:
        assert q is None
    buf.free()
    return q_want, v_want


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_div_linear_bit_exact(ctx, co, field):
    rnd = random.Random(100 + field)
    p, T = kr.MODULI[field], TILE[field]
    lens = [0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 7, (1 << 16) + 3]
    for n in lens:
        a = rand_poly(rnd, field, n)
        for z in (0, 1, p - 1, rnd.randrange(p)):
            q, v = check_division(ctx, co, field, a, z)
            if n >= 2 and n <= 65:  # p == q (X - z) + v on the integers as well
                back = [(v - z * q[0]) % p] + [(q[i - 1] - z * (q[i] if i < n - 1 else 0)) % p for i in range(1, n)]
                assert back == a
        if n >= 2:  # a root of p: p = r (X - root)
            root = rnd.randrange(p)
            r = rand_poly(rnd, field, n - 1)
            a = [(-root * r[0]) % p] + [(r[i - 1] - root * (r[i] if i < n - 1 else 0)) % p for i in range(1, n)]
            q, v = check_division(ctx, co, field, a, root)
            assert v == 0 and q == r


@pytest.mark.parametrize("field", [1, 3])
def test_div_linear_2p20(ctx, co, field):
    rnd = random.Random(7 + field)
    a = rand_poly(rnd, field, 1 << 20)
    check_division(ctx, co, field, a, rnd.randrange(kr.MODULI[field]))


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_poly_eval_mixed_lengths(ctx, co, field):
    rnd = random.Random(200 + field)
    p = kr.MODULI[field]
    lens = [0, 1, 5, TILE[field] + 3, 3 * TILE[field], 70, 2]
    polys = [rand_poly(rnd, field, n) for n in lens]
    bufs = [upload(ctx, co, field, a) if a else ctx.buf_upload(field, np.zeros((1, kr.LIMBS[field]), dtype=np.uint64)) for a in polys]
    z = rnd.randrange(p)
    got = ctx.poly_eval(bufs, kr.to_mont(co, field, [z])[0], lens=lens)
    assert kr.to_ints(co, field, got) == [kr.horner(a, z, p) for a in polys]
    for b in bufs:
        b.free()


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_poly_lincomb_bit_exact(ctx, co, field):
    rnd = random.Random(300 + field)
    p = kr.MODULI[field]
    lens = [TILE[field] + 5, 1, 0, 700, 3]
    polys = [rand_poly(rnd, field, n) for n in lens]
    bufs = [upload(ctx, co, field, a) if a else ctx.buf_upload(field, np.zeros((1, kr.LIMBS[field]), dtype=np.uint64)) for a in polys]
    cs = [rnd.randrange(p) for _ in lens]
    out = ctx.buf_upload(field, np.zeros((max(lens), kr.LIMBS[field]), dtype=np.uint64))
    n = ctx.poly_lincomb(bufs, kr.to_mont(co, field, cs), out, lens=lens)
    assert n == max(lens)
    assert np.array_equal(out.download(), kr.to_mont(co, field, kr.lincomb(polys, cs, p)))
    for b in bufs + [out]:
        b.free()


def open_reference(co, curve, bases, gbases, a, bl, z):
    fr = co.CURVE_FR[curve]
    p = kr.MODULI[fr]
    q, v = kr.div_linear(a, z, p)
    w = co.msm(curve, 1, bases[:len(q)], kr.limbs_of_ints(q, kr.LIMBS[fr]), nthreads=8) if q else None
    rv = None
    if bl is not None:
        bq, rv = kr.div_linear(bl, z, p)
        if bq:
            wb = co.msm(curve, 1, gbases[:len(bq)], kr.limbs_of_ints(bq, kr.LIMBS[fr]), nthreads=8)
            w = wb if w is None else co.jac_add(curve, 1, w, wb)
    return w, v, rv


@pytest.mark.parametrize("curve", CURVES)
def test_kzg_open_parity(ctx, co, curve):
    from pcd_amd import capi
    rnd = random.Random(400 + curve)
    fr = co.CURVE_FR[curve]
    p = kr.MODULI[fr]
    N = 300
    pts = co.gen_points(curve, 1, N, seed=41 + curve)
    gpts = co.gen_points(curve, 1, 4, seed=51 + curve)
    bases = ctx.bases_upload(curve, 1, pts)
    gbases = ctx.bases_upload(curve, 1, gpts)
    z = rnd.randrange(p)
    zm = kr.to_mont(co, fr, [z])[0]
    for n, bl_len in ((N + 1, None), (N + 1, 3), (17, 1), (1, 2), (0, None)):
        a = rand_poly(rnd, fr, n)
        bl = rand_poly(rnd, fr, bl_len) if bl_len is not None else None
        buf = upload(ctx, co, fr, a) if a else ctx.buf_upload(fr, np.zeros((1, kr.LIMBS[fr]), dtype=np.uint64))
        bbuf = upload(ctx, co, fr, bl) if bl else None
        w, v, rv = ctx.kzg_open(bases, buf, zm, length=n, powers_of_gamma_g=gbases if bl else None, blinding=bbuf)
        w_want, v_want, rv_want = open_reference(co, curve, pts, gpts, a, bl, z)
        assert kr.to_ints(co, fr, v) == [v_want]
        if w_want is None:
            assert not np.any(w[2 * len(w) // 3:]), "an empty quotient opens to the point at infinity"
        else:
            assert affine_eq(co, curve, 1, w, w_want), (curve, n, bl_len)
        if bl is None:
            assert rv is None
        else:
            assert kr.to_ints(co, fr, rv) == [rv_want]
        buf.free()
        if bbuf is not None:
            bbuf.free()
    # a quotient longer than the bases: upstream's TooManyCoefficients
    a = rand_poly(rnd, fr, N + 2)
    buf = upload(ctx, co, fr, a)
    with pytest.raises(capi.PcdHipError, match="rc=-1"):
        ctx.kzg_open(bases, buf, zm)
    buf.free()
    bases.free()
    gbases.free()


def test_kzg_open_2p20_mnt4_298(ctx, co):
    rnd = random.Random(500)
    curve, fr = 0, 1
    n = 1 << 20
    pts = co.gen_points_mt(0, 1, n, seed=61, threads=16)
    bases = ctx.bases_upload(curve, 1, pts)
    a = rand_poly(rnd, fr, n + 1)
    z = rnd.randrange(kr.MODULI[fr])
    buf = upload(ctx, co, fr, a)
    w, v, _ = ctx.kzg_open(bases, buf, kr.to_mont(co, fr, [z])[0])
    w_want, v_want, _ = open_reference(co, curve, pts, None, a, None, z)
    assert kr.to_ints(co, fr, v) == [v_want]
    assert affine_eq(co, curve, 1, w, w_want)
    buf.free()
    bases.free()


class Srs:
    """KZG10 setup with a known beta: powers_of_g = [beta^i] g, powers_of_gamma_g = [gamma beta^i] g, h, beta h"""

    def __init__(self, co, curve, degree, seed):
        rnd = random.Random(seed)
        fr = co.CURVE_FR[curve]
        p = kr.MODULI[fr]
        self.curve, self.fr, self.p = curve, fr, p
        beta, gamma = rnd.randrange(1, p), rnd.randrange(1, p)
        g, h = co.generator(curve, 1), co.generator(curve, 2)
        L = kr.LIMBS[fr]
        pw = [pow(beta, i, p) for i in range(degree + 1)]
        self.powers, _ = co.fixed_base_mul(curve, 1, g, kr.limbs_of_ints(pw, L), nthreads=8)
        self.gpowers, _ = co.fixed_base_mul(curve, 1, g, kr.limbs_of_ints([gamma * x % p for x in pw], L), nthreads=8)
        bh, _ = co.fixed_base_mul(curve, 2, h, kr.limbs_of_ints([beta], L))
        self.g, self.gamma_g, self.h, self.beta_h = g, self.gpowers[0], h, bh[0]


def commit(ctx, co, srs, bases, gbases, a, bl):
    L = kr.LIMBS[srs.fr]
    c = ctx.msm(bases, kr.limbs_of_ints(a, L))
    c = co.jac_add(srs.curve, 1, c, ctx.msm(gbases, kr.limbs_of_ints(bl, L)))
    return co.to_affine(srs.curve, 1, c)[0][0]


@pytest.mark.parametrize("curve", CURVES)
def test_kzg_check_soundness(ctx, co, curve):
    rnd = random.Random(600 + curve)
    deg = 32
    srs = Srs(co, curve, deg, seed=700 + curve)
    fr, p, L = srs.fr, srs.p, kr.LIMBS[srs.fr]
    bases = ctx.bases_upload(curve, 1, srs.powers)
    gbases = ctx.bases_upload(curve, 1, srs.gpowers)
    m = lambda xs: kr.to_mont(co, fr, xs)

    def opening(a, bl, z):
        buf, bbuf = upload(ctx, co, fr, a), upload(ctx, co, fr, bl)
        w, v, rv = ctx.kzg_open(bases, buf, m([z])[0], powers_of_gamma_g=gbases, blinding=bbuf)
        buf.free()
        bbuf.free()
        return commit(ctx, co, srs, bases, gbases, a, bl), co.to_affine(curve, 1, w)[0][0], v, rv

    def check(cs, zs, vs, ws, rvs, rs=None):
        return ctx.kzg_check(curve, srs.g, srs.h, srs.beta_h, np.array(cs), m(zs), np.array(vs), np.array(ws), gamma_g_xy=srs.gamma_g,
                             random_v_mont=np.array(rvs), randomizers_canonical=None if rs is None else kr.limbs_of_ints(rs, L))

    a, bl, z = rand_poly(rnd, fr, deg + 1), rand_poly(rnd, fr, 2), rnd.randrange(p)
    c, w, v, rv = opening(a, bl, z)
    assert check([c], [z], [v], [w], [rv])
    one = m([1])[0]
    assert not check([c], [z], [co.fp_op(fr, "add", v[None], one[None])[0]], [w], [rv]), "wrong value"
    assert not check([c], [(z + 1) % p], [v], [w], [rv]), "wrong point"
    assert not check([c], [z], [v], [srs.powers[3]], [rv]), "wrong witness"
    assert not check([c], [z], [v], [w], [co.fp_op(fr, "add", rv[None], one[None])[0]]), "wrong random_v"
    c2 = commit(ctx, co, srs, bases, gbases, rand_poly(rnd, fr, deg + 1), bl)
    assert not check([c2], [z], [v], [w], [rv]), "commitment of another polynomial"
    # batch of 16 (randomizers: the first 1, as upstream)
    k = 16
    zs =[z] + [rnd.randrange(p) for _ in range(k - 1)]
    ops = [(c, w, v, rv)]
    for i in range(1, k):
        ops.append(opening(rand_poly(rnd, fr, rnd.randrange(1, deg + 2)), rand_poly(rnd, fr, 2), zs[i]))
    rs = [1] + [rnd.randrange(1, p) for _ in range(k - 1)]
    cs, ws, vs, rvs = [o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops], [o[3] for o in ops]
    ok = check(cs, zs, vs, ws, rvs, rs)
    assert ok
    # the oracle's pairings on the same combination
    g1 = lambda xy, s: co.scalar_mul(curve, 1, xy, kr.limbs_of_ints([s % p], L)[0])
    zi, vi, rvi = zs, kr.to_ints(co, fr, np.array(vs)), kr.to_ints(co, fr, np.array(rvs))
    lhs = g1(srs.g, -sum(r * v for r, v in zip(rs, vi)))
    lhs = co.jac_add(curve, 1, lhs, g1(srs.gamma_g, -sum(r * x for r, x in zip(rs, rvi))))
    rhs = g1(ws[0], rs[0])
    for i in range(k):
        lhs = co.jac_add(curve, 1, lhs, g1(cs[i], rs[i]))
        lhs = co.jac_add(curve, 1, lhs, g1(ws[i], rs[i] * zi[i]))
        if i:
            rhs = co.jac_add(curve, 1, rhs, g1(ws[i], rs[i]))
    la, ra = co.to_affine(curve, 1, lhs)[0][0], co.to_affine(curve, 1, rhs)[0][0]
    assert ok == np.array_equal(co.pairing(curve, la, srs.h), co.pairing(curve, ra, srs.beta_h))
    bad = list(vs)
    bad[9] = co.fp_op(fr, "add", bad[9][None], one[None])[0]
    assert not check(cs, zs, bad, ws, rvs, rs)
    # no opening at all
    assert ctx.kzg_check(curve, srs.g, srs.h, srs.beta_h, np.zeros((0, 1)), [], [], [], gamma_g_xy=srs.gamma_g)
    bases.free()
    gbases.free()
