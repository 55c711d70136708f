"""GPU: K13 -- pcdhip_poly_open_quotients (the three launches of a round's divisions, batched over parts) word for word against the
integer reference, and pcdhip_kzg_batch_open (MarlinKZG10's open_combinations / batch_open as one queued call) against the oracle's MSMs
over those quotients (tests/kzg_batch_open_reference.py), against pcdhip_kzg_check, and against the composition of the existing calls."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_batch_open_reference as kb  # noqa: E402
import kzg_commit_reference as kc  # noqa: E402
import kzg_reference as kr  # noqa: E402

pytestmark = pytest.mark.gpu

TILES = [1024, 1024, 512, 512]  # coefficients per workgroup of the poly_open_* kernels (poly.hip.h PolyCfg), per field
CB = 256                        # lanes of the carry scan
N = 300                         # bases of the small tests
CURVES = [0, 1, 2, 3]
PAD = 7                         # every buffer is uploaded this many elements longer than `len`, with non-zero elements there


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


def free_all(bufs):
    for b in bufs:
        if b is not None:
            b.free()


class Round:
    """reference items (integer lists) uploaded once: .items for the reference, .dev for the library"""

    def __init__(self, ctx, co, rnd, fr, items):
        self.items, self.dev, self.bufs = items, [], []
        for it in items:
            d = dict(len=len(it["poly"]), shifted=bool(it.get("shifted")), shifted_offset=it.get("shifted_offset", 0))
            d["poly"] = self._up(ctx, co, rnd, fr, it["poly"])
            for key in ("blinding", "shifted_blinding"):
                if it.get(key) is not None:
                    d[key] = self._up(ctx, co, rnd, fr, it[key])
                    d[key + "_len"] = len(it[key])
            self.dev.append(d)

    def _up(self, ctx, co, rnd, fr, ints):
        self.bufs.append(upload(ctx, co, rnd, fr, ints))
        return self.bufs[-1]

    def add_uploaded(self, ints, buf):
        """one more item, not hiding, whose buffer (padding included) the caller has made"""
        self.items.append(dict(poly=ints))
        self.dev.append(dict(poly=buf, len=len(ints)))
        self.bufs.append(buf)

    def free(self):
        free_all(self.bufs)


def tables(co, fr, points, a, s):
    L = kr.LIMBS[fr]
    mont = lambda rows: np.stack([kr.to_mont(co, fr, r) for r in rows]) if len(rows[0]) else np.zeros((len(rows), 0, L), dtype=np.uint64)
    return kr.to_mont(co, fr, points), mont(a), (None if s is None else mont(s))


def check_quotients(ctx, co, fr, rd, points, a, s):
    """one call of pcdhip_poly_open_quotients against parts_of_opening, word for word"""
    p, L, m = kr.MODULI[fr], kr.LIMBS[fr], len(rd.items)
    pm, am, sm = tables(co, fr, points, a, s)
    q_bufs, q_lens, vals = ctx.poly_open_quotients(fr, rd.dev, pm, am, sm)
    try:
        for o, z in enumerate(points):
            pt = kb.parts_of_opening(rd.items, z, a[o], s[o] if s is not None else None, p)
            want = {0: None if pt["comb"] is None else (pt["comb"][1], pt["comb"][2]),
                    1: None if pt["rand"] is None else (pt["rand"][1], pt["rand"][2])}
            want.update({2 + i: qv for i, qv in pt["db"].items()})
            for k in range(2 + m):
                w = want.get(k)
                if w is None:
                    assert int(q_lens[o, k]) == 0 and not vals[o, k].any(), (o, k)
                    continue
                assert int(q_lens[o, k]) == len(w[0]), (o, k)
                assert np.array_equal(vals[o, k], kr.to_mont(co, fr, [w[1]])[0]), (o, k)
                if w[0]:
                    got = q_bufs[(o, k)].download()[:len(w[0])]
                    assert np.array_equal(got, kr.limbs_of_ints(w[0], L)), (o, k)
    finally:
        free_all(q_bufs.values())


@pytest.mark.parametrize("fr", [0, 1, 2, 3])
def test_quotients_bit_exact(ctx, co, fr):
    p, T, rnd = kr.MODULI[fr], TILES[fr], random.Random(1300 + fr)
    lens = [0, 1, 2, T - 1, T, T + 1, 2 * T + 3]
    items = [dict(poly=rand_poly(rnd, p, n)) for n in lens]
    twin = rand_poly(rnd, p, 40)
    items += [dict(poly=list(twin)), dict(poly=list(twin))]     # items 7, 8: p_1 = p_2
    items[1]["blinding"] = rand_poly(rnd, p, 2)
    items[2]["blinding"] = rand_poly(rnd, p, 3)
    for i in (0, 1, 3, 4, 6):
        items[i]["shifted"] = True
    items[4]["shifted_blinding"] = rand_poly(rnd, p, 2)
    rd = Round(ctx, co, rnd, fr, items)
    m = len(items)
    c = rnd.randrange(2, p)
    points = [rnd.randrange(2, p), rnd.randrange(2, p), 0, 1]
    a = [[0] * m for _ in points]
    s = [[0] * m for _ in points]
    for i in (1, 2, 5, 6):                 # opening 0: five items of unequal lengths, item 3 with coefficient zero
        a[0][i] = rnd.randrange(2, p)
    s[0][4] = rnd.randrange(2, p)          # ... and a one-term part with scale != 1 (and its shifted blinding in R)
    a[1][7], a[1][8] = c, p - c            # opening 1: the zero polynomial of 40 coefficients
    s[1][0] = rnd.randrange(2, p)          # ... a degree-bound term of the empty item: no part
    a[2][4] = 1                            # opening 2, z = 0: one term with coefficient 1, read from its item
    s[2][6] = rnd.randrange(2, p)
    a[3][6], a[3][0] = c, c                # opening 3, z = 1: one term with another coefficient; the empty item contributes nothing
    s[3][3], s[3][1] = rnd.randrange(2, p), 1   # a quotient of T - 2 scalars; a constant (no quotient) with scale 1
    check_quotients(ctx, co, fr, rd, points, a, s)
    rd.free()


@pytest.mark.parametrize("fr", [0, 2])
def test_carry_scan_second_tile_per_lane(ctx, co, fr):
    """CB * TILE + 5 coefficients: the first length at which a lane of the scan owns two tiles"""
    p, T, rnd = kr.MODULI[fr], TILES[fr], random.Random(1310 + fr)
    n = CB * T + 5
    assert n == (262149 if fr == 0 else 131077)
    long_mont = co.gen_field(fr, n + PAD, seed=1312 + fr)
    long_ints = kr.to_ints(co, fr, long_mont[:n])
    rd = Round(ctx, co, rnd, fr, [])
    rd.add_uploaded(long_ints, ctx.buf_upload(fr, long_mont))
    short = rand_poly(rnd, p, 9)
    rd.add_uploaded(short, upload(ctx, co, rnd, fr, short))
    points = [rnd.randrange(2, p), rnd.randrange(2, p)]
    a = [[rnd.randrange(2, p), rnd.randrange(2, p)], [0, 1]]   # the long part is a combination of two terms; the short one sits beside it
    check_quotients(ctx, co, fr, rd, points, a, None)
    rd.free()


def assert_openings(got, want, co, fr):
    w, winf, v, rv = got
    for o, (xy, inf, value, rvalue) in enumerate(want):
        assert int(winf[o]) == inf, o
        assert np.array_equal(w[o], xy), o
        assert np.array_equal(v[o], kr.to_mont(co, fr, [value])[0]), o
        assert np.array_equal(rv[o], kr.to_mont(co, fr, [rvalue])[0]), o


@pytest.mark.parametrize("curve", CURVES)
def test_openings_three_in_one_call(ctx, co, curve):
    fr = co.CURVE_FR[curve]
    p, rnd = kr.MODULI[fr], random.Random(1320 + curve)
    pts = co.gen_points(curve, 1, N, seed=41 + curve)
    spts = co.gen_points(curve, 1, N, seed=71 + curve)
    gpts = co.gen_points(curve, 1, 4, seed=51 + curve)
    bases, sbases, gbases = (ctx.bases_upload(curve, 1, x) for x in (pts, spts, gpts))
    items = [dict(poly=rand_poly(rnd, p, 137), blinding=rand_poly(rnd, p, 2), shifted=True, shifted_offset=N - 136,
                  shifted_blinding=rand_poly(rnd, p, 2)),      # exact fit: shifted_offset + len - 1 == the shifted handle's n
             dict(poly=rand_poly(rnd, p, 200), blinding=rand_poly(rnd, p, 3)),
             dict(poly=rand_poly(rnd, p, 64)),
             dict(poly=rand_poly(rnd, p, N + 1))]               # exact fit: len - 1 == powers_of_g's n
    rd = Round(ctx, co, rnd, fr, items)
    m = len(items)
    points = [rnd.randrange(p) for _ in range(3)]
    r = lambda: rnd.randrange(2, p)
    a = [[r(), r(), 0, 0], [0, 0, r(), r()], [0] * m]
    s = [[r(), 0, 0, 0], [0] * m, [0] * m]
    pm, am, sm = tables(co, fr, points, a, s)
    runs, plans = [], []
    try:
        for short in (0, 8):
            ctx.msm_set_short(short)
            runs.append(ctx.kzg_batch_open(bases, rd.dev, pm, am, sm, powers_of_gamma_g=gbases, shifted_powers=sbases))
            plans.append(ctx.kzg_batch_open_last_plan())
    finally:
        ctx.msm_set_short(0)
    for x, y in zip(runs[0], runs[1]):
        assert np.array_equal(x, y), "with and without the short MSMs"
    assert plans == [(3, 0, 1, 3), (3, 1, 0, 3)]
    want = kb.batch_open(co, curve, pts, gpts, spts, items, points, a, s)
    assert [w[1] for w in want] == [0, 0, 1]
    assert_openings(runs[0], want, co, fr)
    assert not runs[0][2][2].any() and not runs[0][3][2].any() and not runs[0][3][1].any()
    rd.free()
    free_all([bases, sbases, gbases])


@pytest.mark.parametrize("curve", CURVES)
def test_round_trip_through_commit_and_check(ctx, co, curve):
    deg = 32
    srs = kc.Srs(co, curve, deg, seed=1330 + curve)
    fr, p, rnd = srs.fr, srs.p, random.Random(1331 + curve)
    L = kr.LIMBS[fr]
    bases, gbases = ctx.bases_upload(curve, 1, srs.powers), ctx.bases_upload(curve, 1, srs.gpowers)
    items = [dict(poly=rand_poly(rnd, p, 33), blinding=rand_poly(rnd, p, 2)),
             dict(poly=rand_poly(rnd, p, 20), blinding=rand_poly(rnd, p, 3)),
             dict(poly=rand_poly(rnd, p, 9), shifted=True, shifted_offset=deg + 1 - 8)]
    rd = Round(ctx, co, rnd, fr, items)
    comm, cinf, _, _, _ = ctx.kzg_commit(bases, [dict(d, shifted=False) for d in rd.dev], powers_of_gamma_g=gbases)
    assert not cinf.any()
    z = rnd.randrange(p)
    a = [[rnd.randrange(2, p) for _ in items]]
    pm, am, _ = tables(co, fr, [z], a, None)
    w, winf, v, rv = ctx.kzg_batch_open(bases, rd.dev, pm, am, powers_of_gamma_g=gbases)
    cj = co.msm(curve, 1, comm, kr.limbs_of_ints(a[0], L), nthreads=4)   # sum_i a_i C_i
    cxy = co.to_affine(curve, 1, cj)[0][0]
    check = lambda val: ctx.kzg_check(curve, srs.g, srs.h, srs.beta_h, np.array([cxy]), pm, np.array([val]), w, gamma_g_xy=srs.gamma_g,
                                      random_v_mont=rv, w_inf=winf)
    assert check(v[0])
    assert not check(co.fp_op(fr, "add", v[0][None], kr.to_mont(co, fr, [1]))[0]), "another value"
    # a degree-bound opening, compared as points with the exponent the identity of the host test is about
    s = [[0, 0, rnd.randrange(2, p)]]
    _, _, sm = tables(co, fr, [z], a, s)
    w, winf, v2, rv2 = ctx.kzg_batch_open(bases, rd.dev, pm, am, sm, powers_of_gamma_g=gbases, shifted_powers=bases)
    e, value, rvalue = kb.witness_exponent(srs, items, z, a[0], s[0])
    lhs, rhs = kb.identity_sides(srs, items, z, a[0], s[0], e)
    assert lhs == rhs
    want_xy, want_inf = srs.exponent_times_g(co, e)
    assert int(winf[0]) == want_inf and np.array_equal(w[0], want_xy)
    assert np.array_equal(v2, v) and np.array_equal(rv2, rv)
    rd.free()
    free_all([bases, gbases])


def test_marlin_shaped_round(ctx, co):
    curve = 0
    fr = co.CURVE_FR[curve]
    p, rnd = kr.MODULI[fr], random.Random(1340)
    nb = 80
    pts, spts, gpts = (co.gen_points(curve, 1, n, seed=sd) for n, sd in ((nb, 1341), (nb, 1342), (4, 1343)))
    bases, sbases, gbases = (ctx.bases_upload(curve, 1, x) for x in (pts, spts, gpts))
    lens = [8 + (i * 37) % 63 for i in range(21)]
    assert len(set(lens)) > 15 and min(lens) >= 8 and max(lens) <= 70
    items = [dict(poly=rand_poly(rnd, p, n)) for n in lens]
    for i in range(9):
        items[i]["blinding"] = rand_poly(rnd, p, 2)
    items[4].update(shifted=True, shifted_offset=nb - lens[4] + 1, shifted_blinding=rand_poly(rnd, p, 2))   # g_1, enforced at beta
    items[15].update(shifted=True, shifted_offset=3)                                                        # g_2, enforced at gamma
    rd = Round(ctx, co, rnd, fr, items)
    m = len(items)
    r = lambda: rnd.randrange(2, p)
    lcs = [dict(terms=[(1, 4)], bound=True), dict(terms=[(1, 15)], bound=True),
           dict(terms=[(r(), i) for i in (0, 1, 2, 3, 5, 6)] + [(p - 1, 7)]),           # the outer sumcheck's shape: seven terms
           dict(terms=[(r(), i) for i in range(8, 21)] + [(r(), 4)]),                   # the inner one: fourteen, g_1 among them unbounded
           dict(terms=[(1, 8)]), dict(terms=[(r(), 9), (r(), 10)])]
    points = [r(), r()]
    queries = [(0, 0), (2, 0), (4, 0), (1, 1), (3, 1), (5, 1)]
    challenges = [(r(), r()) for _ in queries]
    a, s = kb.collapse(lcs, queries, challenges, m, 2, p)
    pm, am, sm = tables(co, fr, points, a, s)
    got = ctx.kzg_batch_open(bases, rd.dev, pm, am, sm, powers_of_gamma_g=gbases, shifted_powers=sbases)
    assert ctx.kzg_batch_open_last_plan() == (4, 0, 2, 3)
    assert_openings(got, kb.batch_open(co, curve, pts, gpts, spts, items, points, a, s), co, fr)
    # without the degree bounds the composition of the existing calls exists: poly_lincomb + kzg_open, point for point
    got = ctx.kzg_batch_open(bases, rd.dev, pm, am, powers_of_gamma_g=gbases)
    assert_openings(got, kb.batch_open(co, curve, pts, gpts, spts, items, points, a, None), co, fr)
    out, rout = ctx.buf_alloc(fr, 70), ctx.buf_alloc(fr, 2)
    for o in range(2):
        idx = [i for i in range(m) if a[o][i]]
        n = ctx.poly_lincomb([rd.dev[i]["poly"] for i in idx], kr.to_mont(co, fr, [a[o][i] for i in idx]), out, lens=[lens[i] for i in idx])
        bidx = [i for i in idx if "blinding" in rd.dev[i]]
        bn = ctx.poly_lincomb([rd.dev[i]["blinding"] for i in bidx], kr.to_mont(co, fr, [a[o][i] for i in bidx]), rout, lens=[2] * len(bidx))
        w, v, rv = ctx.kzg_open(bases, out, pm[o], length=n, powers_of_gamma_g=gbases, blinding=rout, blinding_len=bn)
        xy, inf = co.to_affine(curve, 1, w)
        assert int(inf[0]) == int(got[1][o]) == 0 and np.array_equal(xy[0], got[0][o]), o
        assert np.array_equal(v, got[2][o]) and np.array_equal(rv, got[3][o]), o
    free_all([out, rout, bases, sbases, gbases])
    rd.free()


def raw_batch_open(ctx, powers, dev_items, pm, am, sm, gbases=None, sbases=None, fr=None):
    """the C call with sentinel-filled outputs -> (rc, outputs untouched?)"""
    from pcd_amd import capi
    m = len(dev_items)
    fr = capi.CURVE_FR[powers.curve] if fr is None else fr
    arr = ctx._kzg_items(dev_items)
    pts, P, a, s = ctx._open_tables(fr, m, pm, am, sm)
    outs = [np.full((P, capi.point_limbs(powers.curve, 1)), 0xAB, dtype=np.uint64), np.full(P, 0xAB, dtype=np.uint8),
            np.full((P, kr.LIMBS[fr]), 0xAB, dtype=np.uint64), np.full((P, kr.LIMBS[fr]), 0xAB, dtype=np.uint64)]
    h = lambda b: b._h if b is not None else None
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    rc = capi.lib().pcdhip_kzg_batch_open(ctx._ctx, powers._h, h(gbases), h(sbases), arr if m else None, m, P, ptr(pts), ptr(a), ptr(s),
                                          *[ptr(x) for x in outs])
    return rc, all((x == 0xAB).all() for x in outs)


def test_refusals(ctx, co):
    from pcd_amd import capi
    curve = 0
    fr, fq = co.CURVE_FR[curve], co.CURVE_FQ[curve]
    p, rnd = kr.MODULI[fr], random.Random(1350)
    pts = co.gen_points(curve, 1, N, seed=41)
    gpts = co.gen_points(curve, 1, 4, seed=51)
    bases, gbases = ctx.bases_upload(curve, 1, pts), ctx.bases_upload(curve, 1, gpts)
    sbases = ctx.bases_upload(curve, 1, pts[:100])
    other = ctx.bases_upload(1, 1, co.gen_points(1, 1, 4, seed=52))
    g2 = ctx.bases_upload(curve, 2, co.gen_points(curve, 2, 4, seed=53))
    items = [dict(poly=rand_poly(rnd, p, N + 2)),                                              # 0: a quotient of N + 1 scalars
             dict(poly=rand_poly(rnd, p, 50), shifted=True, shifted_offset=52),                # 1: 52 + 49 = 101 > 100
             dict(poly=rand_poly(rnd, p, 50), blinding=rand_poly(rnd, p, 6)),                  # 2: R's quotient of 5 > 4
             dict(poly=rand_poly(rnd, p, 50), blinding=rand_poly(rnd, p, 2)),                  # 3: fine, hiding
             dict(poly=rand_poly(rnd, p, 50), shifted=True, shifted_offset=51)]                # 4: fine, exact fit 51 + 49 = 100
    rd = Round(ctx, co, rnd, fr, items)
    m = len(items)
    z = [rnd.randrange(p)]

    def call(a_on, s_on=(), g=gbases, sb=sbases, pw=bases, dev=None, P=1):
        a = [[1 if i in a_on else 0 for i in range(m)] for _ in range(P)]
        s = [[5 if i in s_on else 0 for i in range(m)] for _ in range(P)] if s_on is not None else None
        pm, am, sm = tables(co, fr, z * P, a, s)
        return raw_batch_open(ctx, pw, dev or rd.dev, pm, am, sm, g, sb)

    refused = (capi.PCDHIP_E_ARG if hasattr(capi, "PCDHIP_E_ARG") else -1, True)
    assert call({3, 4}, {4}) == (0, False), "the good call"
    assert call({0}) == refused                      # TooManyCoefficients
    assert call({3}, {1}) == refused                 # the degree bound's room in the shifted powers
    assert call({2}) == refused                      # R's quotient above powers_of_gamma_g
    assert call({3}, {3}) == refused                 # s != 0 on an item without `shifted`
    assert call({3}, {4}, sb=None) == refused        # ... or with a NULL shifted handle
    assert call({3}, g=None) == refused              # a blinding taken while the gamma handle is NULL
    assert call({4}, g=None) == (0, False)           # (not taken: no blinding among the terms)
    assert call({3}, g=other) == refused             # handles of different curves
    assert call({3}, g=g2) == refused                # not G1
    assert call({3}, pw=g2, g=None) == refused
    qbuf = ctx.buf_upload(fq, kr.to_mont(co, fq, [1, 2, 3]))
    assert call({0}, dev=[dict(poly=qbuf, len=3)] + rd.dev[1:]) == refused       # coefficients of the base field
    assert call({3}, dev=rd.dev[:3] + [dict(rd.dev[3], len=50 + PAD + 1)] + rd.dev[4:]) == refused  # len beyond the buffer
    # an outstanding MSM ticket owns a side stream's workspace
    scal = ctx.buf_upload(fr, kr.limbs_of_ints(rand_poly(rnd, p, 64), kr.LIMBS[fr]))
    ticket = ctx.msm_submit(bases, scal)
    assert call({3}) == refused
    ctx.msm_collect(ticket)
    assert call({3}) == (0, False)
    # the caps: 64 openings, 1024 items, 8 degree-bound terms of one opening
    assert call({3}, P=65) == refused
    assert call({3}, P=64)[0] == 0
    many = [dict(rd.dev[4]) for _ in range(1025)]
    pm, am, sm = tables(co, fr, z, [[0] * 1025], None)
    assert raw_batch_open(ctx, bases, many, pm, am, sm, gbases, sbases) == refused
    nine = [dict(rd.dev[4]) for _ in range(9)]
    pm, am, sm = tables(co, fr, z, [[0] * 9], [[3] * 9])
    assert raw_batch_open(ctx, bases, nine, pm, am, sm, gbases, sbases) == refused
    pm, am, sm = tables(co, fr, z, [[0] * 8], [[3] * 8])
    assert raw_batch_open(ctx, bases, nine[:8], pm, am, sm, gbases, sbases)[0] == 0
    # the quotients call: a missing or short quotient buffer, another field
    pm, am, sm = tables(co, fr, z, [[0, 0, 0, 1, 0]], None)
    short_q = ctx.buf_alloc(fr, 48)
    for q_bufs in ({}, {(0, 0): short_q, (0, 1): short_q}, {(0, 0): qbuf, (0, 1): qbuf}):
        with pytest.raises(capi.PcdHipError, match="rc=-1"):
            ctx.poly_open_quotients(fr, rd.dev, pm, am, sm, q_bufs=q_bufs)
    with pytest.raises(capi.PcdHipError, match="rc=-1"):
        ctx.poly_open_quotients(fq, rd.dev, pm, am, sm)
    # sharded handles (a multi-device context; on one GPU two logical shards on the same device)
    ndev = capi.lib().pcdhip_device_count()
    mctx = capi.Context(devices=[i % ndev for i in range(2)])
    try:
        mb = mctx.bases_upload(curve, 1, pts)
        mbuf = mctx.buf_upload(fr, kr.to_mont(co, fr, rand_poly(rnd, p, 10)))
        pm, am, sm = tables(co, fr, z, [[1]], None)
        assert raw_batch_open(mctx, mb, [dict(poly=mbuf, len=10)], pm, am, sm) == refused
        free_all([mbuf, mb])
    finally:
        mctx.close()
    # no opening at all: success without a launch
    w, winf, v, rv = ctx.kzg_batch_open(bases, rd.dev, np.zeros((0, kr.LIMBS[fr]), dtype=np.uint64), np.zeros((0, m, kr.LIMBS[fr]), dtype=np.uint64))
    assert w.shape[0] == 0
    free_all([qbuf, scal, short_q, bases, gbases, sbases, other, g2])
    rd.free()
