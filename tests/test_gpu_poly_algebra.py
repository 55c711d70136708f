"""GPU: the K8 vector algebra -- batch inversion, pointwise product, division by X^n - 1, polynomial product -- bit-exact on the ABI
Montgomery words against exact integers (tests/poly_algebra_reference.py)."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_reference as kr  # noqa: E402
import poly_algebra_reference as pr  # noqa: E402

pytestmark = pytest.mark.gpu

LANE = [16, 16, 8, 8]           # elements per lane of the inversion kernel (poly.hip.h BinvCfg::E) ...
TILE = [1024, 1024, 512, 512]   # ... and per tile (64 lanes)
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


def rand_vec(rnd, field, n):
    p = kr.MODULI[field]
    return [rnd.randrange(1, p) for _ in range(n)]


def upload(ctx, co, field, ints):
    return ctx.buf_upload(field, kr.to_mont(co, field, ints))


def mont(co, field, ints):
    return kr.to_mont(co, field, ints)


def plant(rnd, field, xs):
    """zeros at the ends, at the first and last element of a lane's chunk, on both sides of a tile boundary, a run longer than a lane's
    chunk; the values 1 and p - 1"""
    n, E, T, p = len(xs), LANE[field], TILE[field], kr.MODULI[field]
    spots = [0, n - 1, E, 2 * E - 1, 5 * E - 1, 5 * E, T - 1, T, 2 * T - 1, 2 * T]
    spots += list(range(3 * E + 2, 3 * E + 2 + E + 3))  # the run: all of one chunk and parts of its neighbours
    for i in spots:
        if 0 <= i < n:
            xs[i] = 0
    for i, v in ((1, 1), (2, p - 1), (T + 1, 1), (n - 2, p - 1)):
        if 0 <= i < n and n > 4:
            xs[i] = v
    return xs


def check_inverse(ctx, co, field, xs, scale, in_place):
    p = kr.MODULI[field]
    want = mont(co, field, pr.batch_inverse(xs, p, 1 if scale is None else scale))
    buf = upload(ctx, co, field, xs)
    sm = None if scale is None else mont(co, field, [scale])[0]
    out = ctx.vec_batch_inverse(buf, scale_mont=sm, out=buf if in_place else None)
    assert np.array_equal(out.download(), want), (field, len(xs), scale is None, in_place)
    if not in_place:
        assert np.array_equal(buf.download(), mont(co, field, xs))  # the input is left alone
        out.free()
    buf.free()


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_batch_inverse_bit_exact(ctx, co, field):
    rnd = random.Random(400 + field)
    p, T = kr.MODULI[field], TILE[field]
    for n in [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 7, (1 << 16) + 3]:
        xs = plant(rnd, field, rand_vec(rnd, field, n))
        check_inverse(ctx, co, field, xs, None, False)
        check_inverse(ctx, co, field, xs, rnd.randrange(1, p), True)
        if n in (65, T + 1):
            check_inverse(ctx, co, field, xs, rnd.randrange(1, p), False)
            check_inverse(ctx, co, field, xs, None, True)
    check_inverse(ctx, co, field, [0] * (T + 1), None, False)
    check_inverse(ctx, co, field, [0] * (T + 1), rnd.randrange(1, p), True)
    check_inverse(ctx, co, field, [1], None, False)   # an unplanted short vector
    check_inverse(ctx, co, field, [p - 1, 1, 2], 2, False)


def test_batch_inverse_2p20(ctx, co):
    rnd = random.Random(9)
    n = 1 << 20
    xs = rand_vec(rnd, 1, n)
    xs[0] = xs[n // 2 + 17] = xs[n - 1] = 0
    check_inverse(ctx, co, 1, xs, None, False)


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_vec_mul_bit_exact(ctx, co, field):
    rnd = random.Random(500 + field)
    p = kr.MODULI[field]
    for n in [0, 1, 255, 256, 257, (1 << 16) + 3]:
        a, b = rand_vec(rnd, field, n), rand_vec(rnd, field, n)
        if n > 2:
            a[0], b[1], a[n - 1] = 0, 0, p - 1
        want = mont(co, field, [x * y % p for x, y in zip(a, b)])
        ba, bb = upload(ctx, co, field, a), upload(ctx, co, field, b)
        out = ctx.vec_mul(ba, bb)
        assert out.n == n and np.array_equal(out.download(), want), (field, n)
        out.free()
        if n in (257, (1 << 16) + 3):
            sq = ctx.vec_mul(ba, ba)
            assert np.array_equal(sq.download(), mont(co, field, [x * x % p for x in a]))
            sq.free()
            assert ctx.vec_mul(ba, bb, out=ba) is ba and np.array_equal(ba.download(), want)  # out = a
            ba.free()
            ba = upload(ctx, co, field, a)
            ctx.vec_mul(ba, bb, out=bb)                                                         # out = b
            assert np.array_equal(bb.download(), want)
        ba.free()
        bb.free()


DIV_CASES = [(0, 4), (3, 4), (4, 4), (5, 4), (8, 4), (9, 4), (1000, 1), (4097, 256), (3 * (1 << 14) + 5, 1 << 14), ((1 << 16) + 3, 1 << 16)]


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_div_vanishing_bit_exact(ctx, co, field):
    rnd = random.Random(600 + field)
    p = kr.MODULI[field]
    for ln, n in DIV_CASES:
        a = [rnd.randrange(p) for _ in range(ln)]
        q_want, r_want = pr.div_vanishing(a, n, p)
        buf = upload(ctx, co, field, a)
        q, ql, r, rl = ctx.poly_div_vanishing(buf, n, length=ln)
        assert (ql, rl) == (len(q_want), len(r_want)) == (max(ln - n, 0), min(ln, n))
        assert (q is None) == (ql == 0)
        if q is not None:
            assert np.array_equal(q.download(), mont(co, field, q_want)), (field, ln, n)
        assert np.array_equal(r.download(), mont(co, field, r_want)), (field, ln, n)
        if ln in (9, 4097):  # without the remainder
            q2, ql2, r2, rl2 = ctx.poly_div_vanishing(buf, n, length=ln, want_r=False)
            assert r2 is None and rl2 is None and ql2 == ql and np.array_equal(q2.download(), q.download())
            q2.free()
        for b in (buf, q, r):
            if b is not None:
                b.free()


def test_div_vanishing_refuses_aliases(ctx, co):
    from pcd_amd import capi
    rnd = random.Random(7)
    a = [rnd.randrange(kr.MODULI[1]) for _ in range(9)]
    buf, other = upload(ctx, co, 1, a), upload(ctx, co, 1, a)
    for q, r in ((buf, other), (other, buf), (other, other)):
        with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
            ctx.poly_div_vanishing(buf, 4, q=q, r=r)
    assert np.array_equal(buf.download(), mont(co, 1, a)) and np.array_equal(other.download(), mont(co, 1, a))
    buf.free()
    other.free()


def check_product(ctx, co, field, rnd, la, lb, alias=False):
    p = kr.MODULI[field]
    a, b = [rnd.randrange(p) for _ in range(la)], [rnd.randrange(p) for _ in range(lb)]
    ol = la + lb - 1 if la and lb else 0
    ba, bb = upload(ctx, co, field, a + ([0] * (ol - la) if alias else [])), upload(ctx, co, field, b)
    out, n = ctx.poly_mul(ba, bb, la=la, lb=lb, out=ba if alias else None)
    assert n == ol and (alias or out.n == ol)
    got = kr.to_ints(co, field, out.download()[:n])
    if max(la, lb) <= 1025:
        assert got == pr.mul_schoolbook(a, b, p), (field, la, lb)
        assert np.array_equal(out.download()[:n], mont(co, field, got))  # canonical Montgomery words
    else:
        for _ in range(3):
            z = rnd.randrange(p)
            assert kr.horner(got, z, p) == kr.horner(a, z, p) * kr.horner(b, z, p) % p, (field, la, lb)
        assert all(0 <= c < p for c in got) and np.array_equal(out.download()[:n], mont(co, field, got))
    for x in {id(ba): ba, id(bb): bb, id(out): out}.values():
        x.free()


@pytest.mark.parametrize("field", [1, 3])
def test_poly_mul(ctx, co, field):
    rnd = random.Random(700 + field)
    for la, lb in [(0, 5), (1, 1), (1, 7), (33, 32), (1024, 1025), ((1 << 15) + 1, 1 << 15)]:
        check_product(ctx, co, field, rnd, la, lb)
    check_product(ctx, co, field, rnd, 33, 32, alias=True)


def test_poly_mul_field0_constant_factor(ctx, co):
    check_product(ctx, co, 0, random.Random(71), 7 * 16, 1)


def test_poly_mul_mixed_radix_domain(ctx, co):
    """2^16 coefficients are beyond the 2-adicity (15) of field 2: the product runs over the mixed-radix domain 5 * 2^14"""
    from pcd_amd import capi
    assert capi.lib().pcdhip_domain_size(2, 1 << 16) == 5 << 14
    check_product(ctx, co, 2, random.Random(72), (1 << 15) + 1, 1 << 15)


def test_marlin_shape_composition(ctx, co):
    """p of length 3n - 2 = q (X^n - 1) + r, put together again on the device"""
    rnd = random.Random(8)
    field, n = 1, 1 << 10
    p = kr.MODULI[field]
    a = [rnd.randrange(p) for _ in range(3 * n - 2)]
    buf = upload(ctx, co, field, a)
    q, ql, r, rl = ctx.poly_div_vanishing(buf, n)
    assert (ql, rl) == (2 * n - 2, n)
    z = upload(ctx, co, field, [p - 1] + [0] * (n - 1) + [1])
    prod, pl = ctx.poly_mul(q, z)
    assert pl == 3 * n - 2
    one = mont(co, field, [1, 1])
    assert ctx.poly_lincomb([prod, r], one, prod) == 3 * n - 2
    assert np.array_equal(prod.download(), mont(co, field, a))
    for b in (buf, q, r, z, prod):
        b.free()


def test_mismatched_fields_and_counts(ctx, co):
    from pcd_amd import capi
    a0, a1, b1 = upload(ctx, co, 0, [1, 2, 3, 4]), upload(ctx, co, 1, [1, 2, 3, 4]), upload(ctx, co, 1, [5, 6, 7, 8])
    small = upload(ctx, co, 1, [9, 9])
    bad = [
        lambda: ctx.vec_mul(a0, a1, out=b1), lambda: ctx.vec_mul(a1, b1, out=a0), lambda: ctx.vec_mul(a1, b1, n=5, out=b1),
        lambda: ctx.vec_mul(a1, b1, n=4, out=small),
        lambda: ctx.vec_batch_inverse(a1, out=a0), lambda: ctx.vec_batch_inverse(a1, n=5, out=b1), lambda: ctx.vec_batch_inverse(a1, out=small),
        lambda: ctx.poly_div_vanishing(a1, 2, q=a0, r=b1), lambda: ctx.poly_div_vanishing(a1, 2, q=b1, r=a0),
        lambda: ctx.poly_div_vanishing(a1, 2, length=5, q=b1, r=small), lambda: ctx.poly_div_vanishing(a1, 1, q=small, r=b1),
        lambda: ctx.poly_div_vanishing(a1, 0, q=b1, r=small),
        lambda: ctx.poly_mul(a0, a1, out=b1), lambda: ctx.poly_mul(a1, b1, out=a0), lambda: ctx.poly_mul(a1, b1, la=5, out=b1),
        lambda: ctx.poly_mul(a1, b1, out=b1),  # 7 coefficients into 4
    ]
    for f in bad:
        with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
            f()
    for b in (a0, a1, b1, small):
        b.free()
