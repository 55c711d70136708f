"""GPU: pcdhip_msm_set_short -- the small MSMs of KZG10::open (hiding part) and KZG10::check through the short path give what the
bucket pipeline gives: the same witness, values and verdicts, and the openings of tests/kzg_reference.py."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_reference as kr  # noqa: E402
from test_gpu_kzg_open import Srs, affine_eq, commit, open_reference, rand_poly, upload  # noqa: E402

pytestmark = pytest.mark.gpu

CURVES = [0, 1, 2, 3]
SETTINGS = (0, 64)


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


@pytest.mark.parametrize("curve", CURVES)
def test_hiding_open_same_under_both_settings(ctx, co, curve):
    rnd = random.Random(1400 + curve)
    fr = co.CURVE_FR[curve]
    p = kr.MODULI[fr]
    n = 300
    pts = co.gen_points(curve, 1, n, seed=141 + curve)
    gpts = co.gen_points(curve, 1, 4, seed=151 + curve)
    bases = ctx.bases_upload(curve, 1, pts)
    gbases = ctx.bases_upload(curve, 1, gpts)
    z = rnd.randrange(p)
    zm = kr.to_mont(co, fr, [z])[0]
    a = rand_poly(rnd, fr, n)
    buf = upload(ctx, co, fr, a)
    try:
        for bl_len in (2, 3):
            bl = rand_poly(rnd, fr, bl_len)
            bbuf = upload(ctx, co, fr, bl)
            w_want, v_want, rv_want = open_reference(co, curve, pts, gpts, a, bl, z)
            got = {}
            for s in SETTINGS:
                ctx.msm_set_short(s)
                w, v, rv = ctx.kzg_open(bases, buf, zm, length=n, powers_of_gamma_g=gbases, blinding=bbuf)
                assert kr.to_ints(co, fr, v) == [v_want] and kr.to_ints(co, fr, rv) == [rv_want], (curve, bl_len, s)
                assert affine_eq(co, curve, 1, w, w_want), (curve, bl_len, s)
                got[s] = (w, v, rv)
            assert affine_eq(co, curve, 1, got[0][0], got[64][0])
            assert np.array_equal(got[0][1], got[64][1]) and np.array_equal(got[0][2], got[64][2])
            bbuf.free()
        # a polynomial short enough for its own witness MSM to take the short path as well (17 coefficients: 16 pairs)
        short_a = rand_poly(rnd, fr, 17)
        sbuf = upload(ctx, co, fr, short_a)
        bl = rand_poly(rnd, fr, 2)
        bbuf = upload(ctx, co, fr, bl)
        w_want, v_want, rv_want = open_reference(co, curve, pts, gpts, short_a, bl, z)
        for s in SETTINGS:
            ctx.msm_set_short(s)
            w, v, rv = ctx.kzg_open(bases, sbuf, zm, length=17, powers_of_gamma_g=gbases, blinding=bbuf)
            assert kr.to_ints(co, fr, v) == [v_want] and kr.to_ints(co, fr, rv) == [rv_want]
            assert affine_eq(co, curve, 1, w, w_want), (curve, "short polynomial", s)
        sbuf.free()
        bbuf.free()
    finally:
        ctx.msm_set_short(0)
        buf.free()
        bases.free()
        gbases.free()


@pytest.mark.parametrize("curve", CURVES)
def test_check_same_under_both_settings(ctx, co, curve):
    rnd = random.Random(1600 + curve)
    deg = 16
    srs = Srs(co, curve, deg, seed=1700 + curve)
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

    try:
        k = 5
        zs = [rnd.randrange(p) for _ in range(k)]
        ops = {}
        for s in SETTINGS:   # the openings themselves under both settings: the same witnesses and values
            ctx.msm_set_short(s)
            r2 = random.Random(1800 + curve)
            ops[s] = [opening(rand_poly(r2, fr, r2.randrange(2, deg + 2)), rand_poly(r2, fr, 2), zs[i]) for i in range(k)]
        for a, b in zip(ops[0], ops[64]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        cs, ws, vs, rvs = [[o[j] for o in ops[0]] for j in (0, 1, 2, 3)]
        rs = [1] + [rnd.randrange(1, p) for _ in range(k - 1)]
        one = m([1])[0]
        bad1 = [co.fp_op(fr, "add", vs[0][None], one[None])[0]]
        bad5 = list(vs)
        bad5[3] = co.fp_op(fr, "add", bad5[3][None], one[None])[0]
        for s in SETTINGS:
            ctx.msm_set_short(s)
            assert check(cs[:1], zs[:1], vs[:1], ws[:1], rvs[:1]), (curve, s, "one opening")
            assert check(cs, zs, vs, ws, rvs, rs), (curve, s, "five openings")
            assert not check(cs[:1], zs[:1], bad1, ws[:1], rvs[:1]), (curve, s, "tampered value")
            assert not check(cs, zs, bad5, ws, rvs, rs), (curve, s, "tampered value in the batch")
    finally:
        ctx.msm_set_short(0)
        bases.free()
        gbases.free()


def test_check_on_a_multi_device_context_keeps_the_bucket_pipeline(ctx, co):
    """the vector kzg_check uploads through a multi-device context is sharded (the parent handle holds no points): the setter must not
    route it through the short path, and the verdicts are those of setting 0"""
    from pcd_amd import capi
    curve = 0
    rnd = random.Random(1900)
    srs = Srs(co, curve, 8, seed=1901)
    fr, p = srs.fr, srs.p
    bases = ctx.bases_upload(curve, 1, srs.powers)
    gbases = ctx.bases_upload(curve, 1, srs.gpowers)
    m = lambda xs: kr.to_mont(co, fr, xs)
    a, bl, z = rand_poly(rnd, fr, 9), rand_poly(rnd, fr, 2), rnd.randrange(p)
    buf, bbuf = upload(ctx, co, fr, a), upload(ctx, co, fr, bl)
    w, v, rv = ctx.kzg_open(bases, buf, m([z])[0], powers_of_gamma_g=gbases, blinding=bbuf)
    c = commit(ctx, co, srs, bases, gbases, a, bl)
    wa = co.to_affine(curve, 1, w)[0][0]
    for h in (buf, bbuf, bases, gbases):
        h.free()
    bad = co.fp_op(fr, "add", v[None], m([1])[0][None])[0]
    ndev = capi.lib().pcdhip_device_count()
    mctx = capi.Context(devices=[i % ndev for i in range(2)])   # (on one GPU: two logical shards on the same device)
    try:
        verdicts = {}
        for s in SETTINGS:
            mctx.msm_set_short(s)
            verdicts[s] = tuple(bool(mctx.kzg_check(curve, srs.g, srs.h, srs.beta_h, np.array([c]), m([z]), np.array([val]), np.array([wa]),
                                                    gamma_g_xy=srs.gamma_g, random_v_mont=np.array([rv]))) for val in (v, bad))
        assert verdicts[0] == (True, False) and verdicts[64] == verdicts[0]
    finally:
        mctx.close()
