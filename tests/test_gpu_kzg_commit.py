"""GPU: pcdhip_kzg_commit -- KZG10::commit / the loop of MarlinKZG10::commit over device-resident polynomials -- bit-exact on affine
outputs against the integer reference of tests/kzg_commit_reference.py (trimmed length, the oracle's MSM, addition, normalisation)."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_commit_reference as kc  # noqa: E402
import kzg_reference as kr  # noqa: E402

pytestmark = pytest.mark.gpu

B = 256  # coefficients per workgroup of poly_commit_scalars (poly.hip.h POLY_COMMIT_B), the same for the four fields
N = 300  # bases of the small tests
CURVES = [0, 1, 2, 3]
PAD = 7  # every buffer is uploaded this many elements longer than `len`, with non-zero elements there


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


def rand_poly(rnd, p, n):
    return [rnd.randrange(p) for _ in range(n)]


def upload(ctx, co, rnd, fr, ints, pad=PAD):
    """the coefficients followed by `pad` non-zero elements that no call may read"""
    p = kr.MODULI[fr]
    return ctx.buf_upload(fr, kr.to_mont(co, fr, list(ints) + [rnd.randrange(1, p) for _ in range(pad)]))


def assert_point(got_xy, got_inf, want):
    want_xy, want_inf = want[0], want[1]
    assert int(got_inf) == want_inf
    assert np.array_equal(got_xy, want_xy)  # (the identity: zero coordinates on both sides)


def free_all(bufs):
    for b in bufs:
        if b is not None:
            b.free()


@pytest.mark.parametrize("curve", CURVES)
def test_conversion_and_trimming_nine_items(ctx, co, curve):
    fr = co.CURVE_FR[curve]
    p, rnd = kr.MODULI[fr], random.Random(900 + curve)
    pts = co.gen_points(curve, 1, N, seed=41 + curve)
    bases = ctx.bases_upload(curve, 1, pts)
    lens = [0, 1, 2, B - 1, B, B + 1, N]
    polys = [rand_poly(rnd, p, n) for n in lens]
    polys.append(rand_poly(rnd, p, N - (B + 5)) + [0] * (B + 5))  # a whole workgroup of zeros at the top, and part of the one below
    polys.append([0] * 40)
    assert len(polys) == 9  # more than four: the side-stream slots wrap
    bufs = [upload(ctx, co, rnd, fr, a) for a in polys]
    comm, cinf, sh, sinf, tl = ctx.kzg_commit(bases, [dict(poly=b, len=len(a)) for a, b in zip(polys, bufs)])
    want = [kc.commit(co, curve, pts, a) for a in polys]
    assert [int(x) for x in tl] == [w[2] for w in want]
    assert [w[2] for w in want][:7] == lens and want[7][2] == N - (B + 5) and want[8][2] == 0
    for j, w in enumerate(want):
        assert_point(comm[j], cinf[j], w)
    assert [int(x) for x in cinf] == [1, 0, 0, 0, 0, 0, 0, 0, 1], "the empty and the zero polynomial commit to the identity"
    assert all(int(x) == 1 for x in sinf) and not sh.any(), "no item asked for a shifted commitment"
    free_all(bufs)
    bases.free()


@pytest.mark.parametrize("curve", CURVES)
def test_hiding_and_shifted_together(ctx, co, curve):
    fr = co.CURVE_FR[curve]
    p, rnd = kr.MODULI[fr], random.Random(910 + curve)
    pts = co.gen_points(curve, 1, N, seed=41 + curve)
    spts = co.gen_points(curve, 1, N, seed=71 + curve)
    gpts = co.gen_points(curve, 1, 4, seed=51 + curve)
    bases, sbases, gbases = (ctx.bases_upload(curve, 1, x) for x in (pts, spts, gpts))
    # (len, blinding length or None, shifted offset or None, shifted blinding length or None)
    spec = [(0, 1, 0, 2),           # the empty polynomial: both commitments are their hiding parts
            (1, 2, None, None),     # hiding, no degree bound
            (2, 3, 1, None),        # degree bound without a shifted blinding
            (200, 3, 99, 3),
            (137, 1, N - 137, 1),   # exact fit: shifted_offset + t == the shifted powers' n
            (64, None, 0, 2)]       # not hiding, its shifted commitment is
    polys = [rand_poly(rnd, p, n) for n, _, _, _ in spec]
    bls = [None if b is None else rand_poly(rnd, p, b) for _, b, _, _ in spec]
    sbls = [None if s is None else rand_poly(rnd, p, s) for _, _, _, s in spec]
    bufs = [upload(ctx, co, rnd, fr, a) for a in polys]
    bbufs = [None if b is None else upload(ctx, co, rnd, fr, b) for b in bls]
    sbufs = [None if s is None else upload(ctx, co, rnd, fr, s) for s in sbls]
    items = []
    for j, (n, b, off, s) in enumerate(spec):
        it = dict(poly=bufs[j], len=n)
        if b is not None:
            it.update(blinding=bbufs[j], blinding_len=b)
        if off is not None:
            it.update(shifted=True, shifted_offset=off)
        if s is not None:
            it.update(shifted_blinding=sbufs[j], shifted_blinding_len=s)
        items.append(it)
    runs = []
    try:
        for short in (0, 8):
            ctx.msm_set_short(short)
            runs.append(ctx.kzg_commit(bases, items, powers_of_gamma_g=gbases, shifted_powers=sbases))
    finally:
        ctx.msm_set_short(0)
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b), "with and without the short MSMs"
    comm, cinf, sh, sinf, tl = runs[0]
    for j, (n, b, off, s) in enumerate(spec):
        w = kc.commit(co, curve, pts, polys[j], gpts, bls[j])
        assert int(tl[j]) == w[2] == n
        assert_point(comm[j], cinf[j], w)
        if off is None:
            assert int(sinf[j]) == 1 and not sh[j].any()
        else:
            assert_point(sh[j], sinf[j], kc.commit(co, curve, spts, polys[j], gpts, sbls[j], offset=off))
    free_all(bufs + bbufs + sbufs)
    free_all([bases, sbases, gbases])


@pytest.mark.parametrize("curve", CURVES)
def test_degenerate_sums_through_the_epilogue(ctx, co, curve):
    srs = kc.Srs(co, curve, 4, seed=920 + curve)
    fr, p, rnd = srs.fr, srs.p, random.Random(921 + curve)
    bases, gbases = ctx.bases_upload(curve, 1, srs.powers), ctx.bases_upload(curve, 1, srs.gpowers)
    c = rnd.randrange(1, p)
    c_over_gamma = c * pow(srs.gamma, -1, p) % p
    a3, b2 = rand_poly(rnd, p, 3), rand_poly(rnd, p, 2)
    cases = [([c], [(-c_over_gamma) % p], 1),   # c g + (-c) g: the identity from two finite points
             ([c], [c_over_gamma], 1),          # c g + c g: the doubling
             ([], b2, 2),                       # the hiding part alone
             (a3, b2, 0)]                       # a blinding buffer of which no coefficient is used
    bufs = [upload(ctx, co, rnd, fr, a) for a, _, _ in cases]
    bbufs = [upload(ctx, co, rnd, fr, b) for _, b, _ in cases]
    items = [dict(poly=bufs[j], len=len(a), blinding=bbufs[j], blinding_len=bn) for j, (a, _, bn) in enumerate(cases)]
    comm, cinf, _, _, tl = ctx.kzg_commit(bases, items, powers_of_gamma_g=gbases)
    assert [int(x) for x in tl] == [1, 1, 0, 3]
    assert int(cinf[0]) == 1 and not comm[0].any()
    assert_point(comm[1], cinf[1], srs.exponent_times_g(co, 2 * c))
    assert_point(comm[2], cinf[2], srs.exponent_times_g(co, srs.gamma * kr.horner(b2, srs.beta, p)))
    assert_point(comm[3], cinf[3], srs.exponent_times_g(co, kr.horner(a3, srs.beta, p)))
    for j, (a, b, bn) in enumerate(cases):  # and the reference of the other tests says the same
        assert_point(comm[j], cinf[j], kc.commit(co, curve, srs.powers, a, srs.gpowers, b[:bn]))
    free_all(bufs + bbufs + [bases, gbases])


@pytest.mark.parametrize("curve", CURVES)
def test_size_rule_follows_the_trimmed_length(ctx, co, curve):
    from pcd_amd import capi
    fr, fq = co.CURVE_FR[curve], co.CURVE_FQ[curve]
    p, rnd = kr.MODULI[fr], random.Random(930 + curve)
    pts = co.gen_points(curve, 1, N, seed=41 + curve)
    gpts = co.gen_points(curve, 1, 4, seed=51 + curve)
    bases, gbases = ctx.bases_upload(curve, 1, pts), ctx.bases_upload(curve, 1, gpts)
    refused = lambda: pytest.raises(capi.PcdHipError, match="rc=-1")
    a = rand_poly(rnd, p, N) + [0] * 50
    buf = upload(ctx, co, rnd, fr, a)
    comm, cinf, _, _, tl = ctx.kzg_commit(bases, [dict(poly=buf, len=350)])
    w = kc.commit(co, curve, pts, a)
    assert int(tl[0]) == w[2] == N
    assert_point(comm[0], cinf[0], w)
    over = list(a)
    over[N] = 5
    obuf = upload(ctx, co, rnd, fr, over)
    with refused():
        ctx.kzg_commit(bases, [dict(poly=obuf, len=350)])
    # ... also as one item among good ones
    with refused():
        ctx.kzg_commit(bases, [dict(poly=buf, len=350), dict(poly=obuf, len=350), dict(poly=buf, len=10)])
    b200 = rand_poly(rnd, p, 200)
    sbuf = upload(ctx, co, rnd, fr, b200)
    with refused():  # shifted_offset + t == 301
        ctx.kzg_commit(bases, [dict(poly=sbuf, len=200, shifted=True, shifted_offset=101)], shifted_powers=bases)
    comm, cinf, sh, sinf, _ = ctx.kzg_commit(bases, [dict(poly=sbuf, len=200, shifted=True, shifted_offset=100)], shifted_powers=bases)
    assert_point(sh[0], sinf[0], kc.commit(co, curve, pts, b200, offset=100))
    bl = upload(ctx, co, rnd, fr, rand_poly(rnd, p, 5), pad=0)
    with refused():  # a blinding polynomial longer than the gamma powers
        ctx.kzg_commit(bases, [dict(poly=sbuf, len=200, blinding=bl, blinding_len=5)], powers_of_gamma_g=gbases)
    with refused():  # a blinding polynomial without gamma powers
        ctx.kzg_commit(bases, [dict(poly=sbuf, len=200, blinding=bl, blinding_len=2)])
    with refused():  # a degree bound without shifted powers
        ctx.kzg_commit(bases, [dict(poly=sbuf, len=200, shifted=True)])
    with refused():  # len beyond the buffer
        ctx.kzg_commit(bases, [dict(poly=sbuf, len=200 + PAD + 1)])
    qbuf = ctx.buf_upload(fq, kr.to_mont(co, fq, [1, 2, 3]))
    with refused():  # coefficients of the base field
        ctx.kzg_commit(bases, [dict(poly=qbuf, len=3)])
    # an outstanding MSM ticket owns a side stream's workspace
    scal = ctx.buf_upload(fr, kr.limbs_of_ints(rand_poly(rnd, p, 64), kr.LIMBS[fr]))
    ticket = ctx.msm_submit(bases, scal)
    with refused():
        ctx.kzg_commit(bases, [dict(poly=sbuf, len=200)])
    ctx.msm_collect(ticket)
    comm, cinf, _, _, _ = ctx.kzg_commit(bases, [dict(poly=sbuf, len=200)])
    assert_point(comm[0], cinf[0], kc.commit(co, curve, pts, b200))
    # no item at all
    assert ctx.kzg_commit(bases, [])[0].shape[0] == 0
    free_all([buf, obuf, sbuf, bl, qbuf, scal, bases, gbases])


@pytest.mark.parametrize("curve", CURVES)
def test_round_stays_on_the_device(ctx, co, curve):
    """inverse transform -> commit -> open -> check, the polynomial never leaving the device"""
    deg = 32
    srs = kc.Srs(co, curve, deg, seed=940 + curve)
    fr, p, rnd = srs.fr, srs.p, random.Random(941 + curve)
    bases, gbases = ctx.bases_upload(curve, 1, srs.powers), ctx.bases_upload(curve, 1, srs.gpowers)
    m = lambda xs: kr.to_mont(co, fr, xs)
    poly = ctx.fft(fr, ctx.buf_upload(fr, m(rand_poly(rnd, p, 32))), inverse=True)
    other = ctx.fft(fr, ctx.buf_upload(fr, m(rand_poly(rnd, p, 32))), inverse=True)
    bl = ctx.buf_upload(fr, m(rand_poly(rnd, p, 2)))
    comm, cinf, _, _, tl = ctx.kzg_commit(bases, [dict(poly=poly, blinding=bl), dict(poly=other, blinding=bl)], powers_of_gamma_g=gbases)
    assert not cinf.any() and not np.array_equal(comm[0], comm[1])
    # the commitment is that of the coefficients the transform left
    coeffs = kr.to_ints(co, fr, poly.download())
    assert int(tl[0]) == kc.trimmed_len(coeffs, p)
    z = rnd.randrange(p)
    w, v, rv = ctx.kzg_open(bases, poly, m([z])[0], length=int(tl[0]), powers_of_gamma_g=gbases, blinding=bl)
    w_xy = co.to_affine(curve, 1, w)[0][0]
    check = lambda c: ctx.kzg_check(curve, srs.g, srs.h, srs.beta_h, np.array([c]), m([z]), np.array([v]), np.array([w_xy]), gamma_g_xy=srs.gamma_g,
                                    random_v_mont=np.array([rv]))
    assert check(comm[0])
    assert not check(comm[1]), "the commitment of another polynomial"
    free_all([poly, other, bl, bases, gbases])


def test_four_slots_busy_mnt4_298(ctx, co):
    curve, fr = 0, 1
    n = 1 << 16
    pts = co.gen_points_mt(curve, 1, n, seed=61, threads=16)
    spts = co.gen_points_mt(curve, 1, n, seed=62, threads=16)
    bases, sbases = ctx.bases_upload(curve, 1, pts), ctx.bases_upload(curve, 1, spts)
    lens = [n, n - 1, (n >> 1) + 3, n, 70]
    shifted = {2: n - ((n >> 1) + 3), 4: 5}  # item -> shifted_offset (item 2: exact fit)
    monts = [co.gen_field(fr, k, seed=950 + j) for j, k in enumerate(lens)]
    canon = [co.fp_op(fr, "to_canonical", x) for x in monts]
    assert all(c[-1].any() for c in canon), "top coefficients are non-zero"
    bufs = [ctx.buf_upload(fr, x) for x in monts]
    items = [dict(poly=b, shifted=j in shifted, shifted_offset=shifted.get(j, 0)) for j, b in enumerate(bufs)]
    comm, cinf, sh, sinf, tl = ctx.kzg_commit(bases, items, shifted_powers=sbases)
    assert [int(x) for x in tl] == lens
    for j, k in enumerate(lens):
        xy, inf = co.to_affine(curve, 1, co.msm(curve, 1, pts[:k], canon[j], nthreads=16))
        assert int(cinf[j]) == int(inf[0]) == 0 and np.array_equal(comm[j], xy[0]), j
        if j in shifted:
            xy, inf = co.to_affine(curve, 1, co.msm(curve, 1, spts[shifted[j]:shifted[j] + k], canon[j], nthreads=16))
            assert int(sinf[j]) == int(inf[0]) == 0 and np.array_equal(sh[j], xy[0]), j
        else:
            assert int(sinf[j]) == 1
    free_all(bufs + [bases, sbases])
