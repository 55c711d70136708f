"""GPU: K14 -- pcdhip_kzg_check_scalars (the scalar collapse of the MarlinKZG10 check) word for word against the integer reference
(tests/kzg_check_reference.py), and pcdhip_kzg_check_combinations (check_combinations / batch_check as one queued call) on what
pcdhip_kzg_commit and pcdhip_kzg_batch_open produce, on points of known exponent, on a Marlin-shaped round against pcdhip_kzg_check, in
both pairing modes, and its refusals.  Every table and point array that goes to the library is followed by elements that no call may
read: all-ones words, which are no reduced field element and no point."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_batch_open_reference as kb  # noqa: E402
import kzg_check_reference as kk  # noqa: E402
import kzg_commit_reference as kc  # noqa: E402
import kzg_reference as kr  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 3
JUNK = 0xFFFFFFFFFFFFFFFF
E_ARG, E_SIZE = -1, -2


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


def padded(arr, dtype=np.uint64):
    """the array in front of PAD more rows of all-ones words; the view that is returned is what a call gets"""
    arr = np.ascontiguousarray(arr, dtype=dtype)
    big = np.full((arr.shape[0] + PAD,) + arr.shape[1:], JUNK if dtype == np.uint64 else 0xFF, dtype=dtype)
    big[:arr.shape[0]] = arr
    return big[:arr.shape[0]]


def mont_rows(co, fr, xs):
    return padded(kr.to_mont(co, fr, xs))


def mont_table(co, fr, rows, junk_where=None):
    """P x m integers -> ABI Montgomery (P, m, L); junk_where[o][i] true: all-ones words there instead (an entry no call may read)"""
    L = kr.LIMBS[fr]
    t = np.stack([kr.to_mont(co, fr, r) for r in rows]) if len(rows[0]) else np.zeros((len(rows), 0, L), dtype=np.uint64)
    if junk_where is not None:
        t[np.array(junk_where, dtype=bool)] = JUNK
    return padded(t)


class Case:
    """one call's tables as integers (the reference's form) and, through .lib(co, fr), as the arrays the library takes"""

    def __init__(self, shift_index, points, a, s, values, random_v, item_values):
        self.shift_index, self.points, self.a, self.s, self.values, self.random_v, self.item_values = shift_index, points, a, s, values, random_v, item_values

    def copy(self, **kw):
        c = Case(self.shift_index, list(self.points), [list(r) for r in self.a], None if self.s is None else [list(r) for r in self.s],
                 list(self.values), None if self.random_v is None else list(self.random_v),
                 None if self.item_values is None else [list(r) for r in self.item_values])
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def ref(self):
        return (self.shift_index, self.points, self.a, self.s, self.values, self.random_v, self.item_values)

    def lib(self, co, fr, randomizers=None):
        s = self.s
        unread = None if s is None else [[x == 0 for x in row] for row in s]
        return dict(points_mont=mont_rows(co, fr, self.points), coeffs_mont=mont_table(co, fr, self.a), values_mont=mont_rows(co, fr, self.values),
                    shifted_coeffs_mont=None if s is None else mont_table(co, fr, s),
                    random_v_mont=None if self.random_v is None else mont_rows(co, fr, self.random_v),
                    item_values_mont=None if self.item_values is None else mont_table(co, fr, self.item_values, unread),
                    randomizers_canonical=None if randomizers is None else padded(kr.limbs_of_ints(randomizers, kr.LIMBS[fr])),
                    shift_index=None if self.shift_index is None else padded(np.array(self.shift_index, dtype=np.int32), np.int32))


# ------------------------------------------------------------------------------------------------------------ 1. the scalars, word for word
def assert_scalars(ctx, co, fr, n_shift, case, randomizers):
    p, L = kr.MODULI[fr], kr.LIMBS[fr]
    left, right = ctx.kzg_check_scalars(fr, n_shift, **case.lib(co, fr, randomizers))
    wl, wr = kk.collapse(p, n_shift, *case.ref(), randomizers)
    assert left.shape[:2] == (len(wl), len(wl[0])) and right.shape[:2] == (len(wr), len(wr[0]))
    for e in range(len(wl)):
        assert np.array_equal(left[e], kr.limbs_of_ints(wl[e], L)), e
        assert np.array_equal(right[e], kr.limbs_of_ints(wr[e], L)), e


@pytest.mark.parametrize("fr", [0, 1, 2, 3])
def test_scalars_word_for_word(ctx, co, fr):
    p, rnd = kr.MODULI[fr], random.Random(1400 + fr)
    r = lambda: rnd.randrange(2, p)
    m, P, n_shift = 5, 3, 3                       # items 1 and 3 share shift power 0, item 4 has power 2; power 1 has no item
    shift_index = [-1, 0, -1, 0, 2]
    a = [[r(), 0, 1, p - 1, r()], [0] * m, [p - 1, p - 1, r(), 1, 0]]              # opening 1: its a row is all zero
    s = [[0, p - 1, 0, 1, r()], [0, r(), 0, 0, p - 1], [0, p - 1, 0, p - 1, 0]]
    v = [[r(), p - 1, r(), 1, 0], [r(), r(), r(), r(), p - 1], [r(), p - 1, r(), p - 1, r()]]
    case = Case(shift_index, [0, 1, p - 1], a, s, [p - 1, 0, p - 1], [1, p - 1, p - 1], v)
    for randomizers in (None, [1, p - 1, p - 1], [1, 0, r()]):
        assert_scalars(ctx, co, fr, n_shift, case, randomizers)
    # neither optional table, no shift power
    assert_scalars(ctx, co, fr, 0, case.copy(shift_index=None, s=None, random_v=None, item_values=None), [1, r(), r()])
    assert_scalars(ctx, co, fr, 0, case.copy(shift_index=None, s=None, random_v=None, item_values=None), None)
    # the longest loop: 64 openings of one item, sums of 64 terms that wrap
    P = 64
    wide = Case([0], [r() for _ in range(P)], [[p - 1] for _ in range(P)], [[p - 1 if o % 2 else r()] for o in range(P)], [p - 1] * P,
                [r() for _ in range(P)], [[p - 1] for _ in range(P)])
    assert_scalars(ctx, co, fr, 1, wide, [1] + [p - 1] * (P - 1))
    assert_scalars(ctx, co, fr, 1, wide, None)


# ------------------------------------------------------------------------------------------------------------ the check itself
class Setup:
    """a key on a setup that keeps its trapdoor, and what a call needs besides its tables: points (affine, flags) from exponents"""

    def __init__(self, ctx, co, curve, seed, shift_exps, gamma=True, degree=1):
        self.co, self.curve = co, curve
        self.srs = kc.Srs(co, curve, degree, seed=seed)
        self.fr, self.p = self.srs.fr, self.srs.p
        self.shift_exps = list(shift_exps)
        sp = np.stack([self.srs.exponent_times_g(co, e)[0] for e in shift_exps]) if shift_exps else None
        self.vk = ctx.kzg_vk_prepare(curve, self.srs.g, self.srs.h, self.srs.beta_h, gamma_g_xy=self.srs.gamma_g if gamma else None,
                                     shift_powers_xy=None if sp is None else padded(sp))

    def points(self, exps):
        pts = [self.srs.exponent_times_g(self.co, e) for e in exps]
        return padded(np.stack([xy for xy, _ in pts])), padded(np.array([inf for _, inf in pts], dtype=np.uint8), np.uint8)


def solve_witnesses(st, comm_exps, shifted_exps, case):
    out = []
    for o, z in enumerate(case.points):
        c = kk.combined_exponent(st.srs, st.shift_exps, comm_exps, shifted_exps, case.shift_index, case.a[o], None if case.s is None else case.s[o],
                                 None if case.item_values is None else case.item_values[o])
        out.append(kk.solve_witness(st.srs, c, case.values[o], 0 if case.random_v is None else case.random_v[o], z))
    return out


def both_modes(ctx, st, comm_exps, shifted_exps, w_exps, case, randomizers, flags=True):
    """-> (combined verdict, per-opening verdicts), each asserted equal to the integer reference's"""
    co, fr = st.co, st.fr
    cxy, cinf = st.points(comm_exps)
    sxy, sinf = st.points(shifted_exps) if shifted_exps is not None else (None, None)
    wxy, winf = st.points(w_exps)
    out = []
    for rho in (randomizers, None):
        got = ctx.kzg_check_combinations(st.vk, cxy, w_xy=wxy, shifted_xy=sxy, comm_inf=cinf if flags else None, shifted_inf=sinf if flags else None,
                                         w_inf=winf if flags else None, **case.lib(co, fr, rho))
        want = kk.verdict(st.srs, st.shift_exps, comm_exps, shifted_exps, w_exps, *case.ref(), rho)
        assert (got if rho is None else [got]) == want, (rho is None, got, want)
        out.append(got)
    return out[0], out[1]


# ---- 2. the round trip through commit and batch_open
def round_trip(ctx, co, curve):
    """pcdhip_kzg_commit (hiding, item 2 with a degree bound and a shifted blinding) -> pcdhip_kzg_batch_open of three openings with s != 0
    in the first two: the arrays a check takes"""
    deg = 32
    srs = kc.Srs(co, curve, deg, seed=1430 + curve)
    fr, p, rnd = srs.fr, srs.p, random.Random(1431 + curve)
    bases, gbases = ctx.bases_upload(curve, 1, srs.powers), ctx.bases_upload(curve, 1, srs.gpowers)
    polys = [dict(poly=[rnd.randrange(p) for _ in range(33)], blinding=[rnd.randrange(p) for _ in range(2)]),
             dict(poly=[rnd.randrange(p) for _ in range(20)], blinding=[rnd.randrange(p) for _ in range(3)]),
             dict(poly=[rnd.randrange(p) for _ in range(9)], blinding=[rnd.randrange(p) for _ in range(2)], shifted=True, shifted_offset=deg + 1 - 9,
                  shifted_blinding=[rnd.randrange(p) for _ in range(2)])]
    bufs, dev = [], []
    for it in polys:
        d = dict(len=len(it["poly"]), shifted=bool(it.get("shifted")), shifted_offset=it.get("shifted_offset", 0))
        for key in ("poly", "blinding", "shifted_blinding"):
            if it.get(key) is not None:
                bufs.append(ctx.buf_upload(fr, kr.to_mont(co, fr, it[key])))
                d[key] = bufs[-1]
        dev.append(d)
    comm, cinf, shifted, sinf, _ = ctx.kzg_commit(bases, dev, powers_of_gamma_g=gbases, shifted_powers=bases)
    assert not cinf.any() and list(sinf) == [1, 1, 0]
    m, P = 3, 3
    points = [rnd.randrange(p) for _ in range(P)]
    a = [[rnd.randrange(2, p) for _ in range(m)] for _ in range(P)]
    s = [[0, 0, rnd.randrange(2, p)], [0, 0, rnd.randrange(2, p)], [0, 0, 0]]
    mont = lambda rows: np.stack([kr.to_mont(co, fr, r) for r in rows])
    w, winf, v, rv = ctx.kzg_batch_open(bases, dev, kr.to_mont(co, fr, points), mont(a), mont(s), powers_of_gamma_g=gbases, shifted_powers=bases)
    assert not winf.any()
    for b in bufs + [bases, gbases]:
        b.free()
    item_values = [[0, 0, kr.horner(polys[2]["poly"], z, p)] for z in points]
    vk = ctx.kzg_vk_prepare(curve, srs.g, srs.h, srs.beta_h, gamma_g_xy=srs.gamma_g,
                            shift_powers_xy=padded(np.stack([srs.powers[deg + 1 - 9], srs.powers[deg + 2 - 9]])))
    case = Case([-1, -1, 0], points, a, s, kr.to_ints(co, fr, v), kr.to_ints(co, fr, rv), item_values)
    return dict(srs=srs, vk=vk, case=case, comm=comm, cinf=cinf, shifted=shifted, sinf=sinf, w=w, winf=winf, rnd=rnd)


@pytest.fixture(scope="module")
def rounds(ctx, co):
    """curve -> its round trip, made once and shared by the tests that check it"""
    cache = {}

    def get(curve):
        if curve not in cache:
            cache[curve] = round_trip(ctx, co, curve)
        return cache[curve]

    yield get
    for rt in cache.values():
        rt["vk"].free()


def run_round(ctx, co, rt, case, randomizers, comm=None, w=None):
    fr = rt["srs"].fr
    return ctx.kzg_check_combinations(rt["vk"], padded(rt["comm"] if comm is None else comm), w_xy=padded(rt["w"] if w is None else w),
                                      shifted_xy=padded(rt["shifted"]), comm_inf=padded(rt["cinf"], np.uint8), shifted_inf=padded(rt["sinf"], np.uint8),
                                      w_inf=padded(rt["winf"], np.uint8), **case.lib(co, fr, randomizers))


def spoilings(rt):
    """name -> (keyword changes of run_round, the per-opening verdicts expected): everything but the global ones hits the middle opening"""
    case, p = rt["case"], rt["srs"].p
    bump = lambda xs, o: [(x + 1) % p if j == o else x for j, x in enumerate(xs)]
    iv = [list(r) for r in case.item_values]
    iv[1][2] = (iv[1][2] + 1) % p
    w = rt["w"].copy()
    w[1] = w[0]
    comm = rt["comm"].copy()
    comm[[0, 1]] = comm[[1, 0]]
    return {"value + 1": (dict(case=case.copy(values=bump(case.values, 1))), [True, False, True]),
            "random_v + 1": (dict(case=case.copy(random_v=bump(case.random_v, 1))), [True, False, True]),
            "the degree-bound item's v + 1": (dict(case=case.copy(item_values=iv)), [True, False, True]),
            "W swapped for another point": (dict(case=case, w=w), [True, False, True]),
            "z + 1": (dict(case=case.copy(points=bump(case.points, 1))), [True, False, True]),
            "two commitments exchanged": (dict(case=case, comm=comm), [False, False, False]),
            "the other shift index": (dict(case=case.copy(shift_index=[-1, -1, 1])), [False, False, True])}


@pytest.mark.parametrize("curve", [0, 1, 2, 3])
def test_round_trip_through_commit_and_batch_open(ctx, co, rounds, curve):
    rt = rounds(curve)
    rho = [1, rt["rnd"].randrange(2, rt["srs"].p), rt["rnd"].randrange(2, rt["srs"].p)]
    assert run_round(ctx, co, rt, rt["case"], rho) is True
    assert run_round(ctx, co, rt, rt["case"], None) == [True, True, True]
    assert ctx.kzg_check_combinations_last_plan() == (3, 2 + 2 + 6 + 3, 7, 1)
    for name, (kw, want) in spoilings(rt).items():
        assert run_round(ctx, co, rt, kw["case"], None, comm=kw.get("comm"), w=kw.get("w")) == want, name
        assert run_round(ctx, co, rt, kw["case"], rho, comm=kw.get("comm"), w=kw.get("w")) is False, name


# ---- 5. pairing mode 1: the lane-per-pairing kernels, on normalised sums
def test_pairing_mode_one_gives_the_same_verdicts(ctx, co, rounds):
    rt = rounds(0)
    rho = [1, 12345, 67890]
    kw, want = spoilings(rt)["the degree-bound item's v + 1"]
    try:
        ctx.pairing_set_mode(1)
        assert run_round(ctx, co, rt, rt["case"], rho) is True
        assert run_round(ctx, co, rt, rt["case"], None) == [True, True, True]
        assert ctx.kzg_check_combinations_last_plan() == (3, 13, 8, 1)
        assert run_round(ctx, co, rt, kw["case"], None) == want
        assert run_round(ctx, co, rt, kw["case"], rho) is False
    finally:
        ctx.pairing_set_mode(0)


# ---- 3. known-exponent edges
@pytest.mark.parametrize("curve", [0, 2])
def test_known_exponent_edges(ctx, co, curve):
    rnd = random.Random(1440 + curve)
    st = Setup(ctx, co, curve, 1441 + curve, shift_exps=[rnd.randrange(1, 1 << 200)])
    p, srs = st.p, st.srs
    r = lambda: rnd.randrange(2, p)
    m, P = 3, 2
    base = Case([-1, 0, -1], [r(), r()], [[r() for _ in range(m)] for _ in range(P)], [[0, r(), 0], [0, 0, 0]], [r(), r()], [r(), r()],
                [[0, r(), 0], [0, 0, 0]])
    rho = [1, r()]
    valid = lambda comm, sh, case: solve_witnesses(st, comm, sh, case)
    cexp = lambda comm, sh, case, o: kk.combined_exponent(srs, st.shift_exps, comm, sh, case.shift_index, case.a[o], case.s[o], case.item_values[o])
    comm, sh = [r(), r(), r()], [0, r(), 0]
    # a commitment flagged infinite (and, in a second call, recognised by its zero coordinates alone)
    c0 = [0] + comm[1:]
    w = valid(c0, sh, base)
    assert both_modes(ctx, st, c0, sh, w, base, rho) == (True, [True, True])
    assert both_modes(ctx, st, c0, sh, w, base, rho, flags=False) == (True, [True, True])
    # a witness flagged infinite with c - v - gamma rv = 0: both sides of opening 0 are the identity
    case = base.copy()
    case.values[0] = (cexp(comm, sh, case, 0) - srs.gamma * case.random_v[0]) % p
    w = valid(comm, sh, case)
    assert w[0] == 0 and w[1] != 0
    assert both_modes(ctx, st, comm, sh, w, case, rho) == (True, [True, True])
    # the left side the identity while the right is not
    w0 = r()
    case.values[0] = (cexp(comm, sh, case, 0) - srs.gamma * case.random_v[0] + case.points[0] * w0) % p
    assert both_modes(ctx, st, comm, sh, [w0, w[1]], case, rho) == (False, [False, True])
    # the same commitment listed twice: equal operands in the tree of the planes
    twice = [comm[0], comm[0], comm[2]]
    assert both_modes(ctx, st, twice, sh, valid(twice, sh, base), base, rho) == (True, [True, True])
    # two openings at one point
    same_z = base.copy(points=[base.points[0], base.points[0]])
    assert both_modes(ctx, st, comm, sh, valid(comm, sh, same_z), same_z, rho) == (True, [True, True])
    # randomizers (1, 1) with W_1 = -W_0: the right side is the identity; the left one too when both openings hold ...
    case = base.copy()
    w = valid(comm, sh, case)
    w[1] = (p - w[0]) % p
    case.values[1] = (cexp(comm, sh, case, 1) - srs.gamma * case.random_v[1] - (srs.beta - case.points[1]) * w[1]) % p
    assert both_modes(ctx, st, comm, sh, w, case, [1, 1]) == (True, [True, True])
    # ... and not when one does not
    case.values[1] = (case.values[1] + 1) % p
    assert both_modes(ctx, st, comm, sh, w, case, [1, 1]) == (False, [True, False])
    st.vk.free()


# ---- 4. a Marlin-shaped round
@pytest.mark.parametrize("curve", [0, 2])
def test_marlin_shaped_round(ctx, co, curve):
    rnd = random.Random(1450 + curve)
    st = Setup(ctx, co, curve, 1451 + curve, shift_exps=[rnd.randrange(1, 1 << 200), rnd.randrange(1, 1 << 200)])
    p, fr, srs = st.p, st.fr, st.srs
    L = kr.LIMBS[fr]
    r = lambda: rnd.randrange(2, p)
    m = 21
    # the linear combinations and the queries of test_gpu_kzg_batch_open.py::test_marlin_shaped_round: g_1 (item 4) and g_2 (item 15) bounded
    lcs = [dict(terms=[(1, 4)], bound=True), dict(terms=[(1, 15)], bound=True),
           dict(terms=[(r(), i) for i in (0, 1, 2, 3, 5, 6)] + [(p - 1, 7)]),
           dict(terms=[(r(), i) for i in range(8, 21)] + [(r(), 4)]),
           dict(terms=[(1, 8)]), dict(terms=[(r(), 9), (r(), 10)])]
    queries = [(0, 0), (2, 0), (4, 0), (1, 1), (3, 1), (5, 1)]
    a, s = kb.collapse(lcs, queries, [(r(), r()) for _ in queries], m, 2, p)
    shift_index = [0 if i == 4 else 1 if i == 15 else -1 for i in range(m)]
    comm = [r() for _ in range(m)]
    sh = [r() if shift_index[i] >= 0 else 0 for i in range(m)]
    case = Case(shift_index, [r(), r()], a, s, [r(), r()], [r(), r()], [[r() if s[o][i] else 0 for i in range(m)] for o in range(2)])
    rho = [1, r()]
    w = solve_witnesses(st, comm, sh, case)
    assert both_modes(ctx, st, comm, sh, w, case, rho) == (True, [True, True])
    assert ctx.kzg_check_combinations_last_plan() == (2, 2 + 2 + 2 * m + 2, 7, 1)
    # without the degree bounds: the existing pcdhip_kzg_check on commitments combined through the oracle's MSM, a true and a false case
    plain = case.copy(shift_index=None, s=None, item_values=None)
    w = solve_witnesses(st, comm, None, plain)
    cxy, cinf = st.points(comm)
    wxy, winf = st.points(w)
    combined = np.stack([co.to_affine(curve, 1, co.msm(curve, 1, cxy, kr.limbs_of_ints(a[o], L), nthreads=4))[0][0] for o in range(2)])
    for cs, want in ((plain, True), (plain.copy(values=[plain.values[0], (plain.values[1] + 1) % p]), False)):
        got = ctx.kzg_check_combinations(st.vk, cxy, w_xy=wxy, comm_inf=cinf, w_inf=winf, **cs.lib(co, fr, rho))
        assert ctx.kzg_check_combinations_last_plan() == (1, 2 + 2 + 2 * m + 2, 7, 1)
        old = ctx.kzg_check(curve, srs.g, srs.h, srs.beta_h, combined, kr.to_mont(co, fr, cs.points), kr.to_mont(co, fr, cs.values), wxy,
                            gamma_g_xy=srs.gamma_g, random_v_mont=kr.to_mont(co, fr, cs.random_v), randomizers_canonical=kr.limbs_of_ints(rho, L),
                            w_inf=winf)
        assert got is want and old is want
    st.vk.free()


# ---- 6. refusals
def raw_check(ctx, vk, cxy, wxy, tables, sxy=None, drop=()):
    """the C call with a sentinel in ok -> (rc, ok afterwards); `drop` names arguments passed as NULL"""
    from pcd_amd import capi
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    t = dict(tables, comm=cxy, w=wxy, shifted=sxy)
    for k in drop:
        t[k] = None
    m, P = cxy.shape[0], wxy.shape[0]
    ok = (C.c_int * 70)(*([7] * 70))
    rc = capi.lib().pcdhip_kzg_check_combinations(ctx._ctx, vk._h if vk is not None else None, m, ptr(t["comm"]), None, ptr(t["shifted"]), None,
                                                  ptr(t["shift_index"]), P, ptr(t["points_mont"]), ptr(t["coeffs_mont"]), ptr(t["shifted_coeffs_mont"]),
                                                  ptr(t["values_mont"]), ptr(t["random_v_mont"]), ptr(t["item_values_mont"]), ptr(t["w"]), None,
                                                  ptr(t["randomizers_canonical"]), None if "ok" in drop else ok)
    return rc, list(ok)


def test_refusals(ctx, co):
    curve = 0
    rnd = random.Random(1460)
    st = Setup(ctx, co, curve, 1461, shift_exps=[rnd.randrange(1, 1 << 200)])
    bare = Setup(ctx, co, curve, 1461, shift_exps=[], gamma=False)
    p, fr = st.p, st.fr
    L = kr.LIMBS[fr]
    r = lambda: rnd.randrange(2, p)
    m, P = 2, 2
    case = Case([0, -1], [r(), r()], [[r(), r()], [r(), r()]], [[r(), 0], [0, 0]], [r(), r()], [r(), r()], [[r(), 0], [0, 0]])
    comm, sh = [r(), r()], [r(), 0]
    w = solve_witnesses(st, comm, sh, case)
    cxy, _ = st.points(comm)
    sxy, _ = st.points(sh)
    wxy, _ = st.points(w)
    rho = [1, r()]
    untouched = [7] * 70
    good = lambda: raw_check(ctx, st.vk, cxy, wxy, case.lib(co, fr, rho), sxy)
    assert good() == (0, [1] + [7] * 69)

    def refused(rc, tables=None, vk=st.vk, drop=(), c=cxy, wp=wxy, s=sxy):
        assert raw_check(ctx, vk, c, wp, tables if tables is not None else case.lib(co, fr, rho), s, drop) == (rc, untouched), (rc, drop)
        assert good() == (0, [1] + [7] * 69)      # the next valid call is clean

    for name in ("comm", "w", "points_mont", "coeffs_mont", "values_mont", "ok"):
        refused(E_ARG, drop=(name,))
    refused(E_ARG, vk=None)
    # an element that is not reduced: r itself, in every table and in the randomizers
    for name in ("points_mont", "coeffs_mont", "shifted_coeffs_mont", "values_mont", "random_v_mont", "item_values_mont", "randomizers_canonical"):
        t = case.lib(co, fr, rho)
        t[name].reshape(-1, L)[0] = kr.limbs_of_ints([p], L)[0]
        refused(E_ARG, tables=t)
    # ... while an item value is not looked at where s == 0
    t = case.lib(co, fr, rho)
    assert (t["item_values_mont"][0, 1] == JUNK).all() and raw_check(ctx, st.vk, cxy, wxy, t, sxy) == (0, [1] + [7] * 69)
    # s != 0 on an item without a usable shift power, or without the arrays that go with it
    refused(E_ARG, tables=case.copy(shift_index=[-1, -1]).lib(co, fr, rho))
    refused(E_ARG, tables=case.copy(shift_index=[1, -1]).lib(co, fr, rho))
    for name in ("shift_index", "shifted", "item_values_mont"):
        refused(E_ARG, drop=(name,))
    # random_v while the key has no gamma_g; without it, and without degree bounds, that key serves
    plain = case.copy(shift_index=None, s=None, item_values=None)
    assert raw_check(ctx, bare.vk, cxy, wxy, plain.lib(co, fr, rho)) == (E_ARG, untouched)
    nv = plain.copy(random_v=None)
    wv, _ = bare.points(solve_witnesses(bare, comm, None, nv))
    assert raw_check(ctx, bare.vk, cxy, wv, nv.lib(co, fr, rho)) == (0, [1] + [7] * 69)
    # the sizes: 65 openings; 1025 points
    many = Case(None, [r()] * 65, [[1, 1]] * 65, None, [r()] * 65, None, None)
    refused(E_SIZE, tables=many.lib(co, fr, None), wp=padded(np.repeat(wxy[:1], 65, axis=0)), s=None)
    big_m = 511                                   # N = 2 + 1 + 2 * 511 + 1 = 1026; 510 items fit exactly (1024)
    for mm, rc in ((big_m, E_SIZE), (big_m - 1, 0)):
        wide = Case(None, [case.points[0]], [[0] * mm], None, [0], None, None)
        got = raw_check(ctx, st.vk, padded(np.repeat(cxy[:1], mm, axis=0)), padded(np.zeros_like(wxy[:1])), wide.lib(co, fr, None))
        assert got == ((rc, untouched) if rc else (0, [1] + [7] * 69)), mm      # (all-zero tables and W = O: 0 == 0, true)
    # no opening at all: true without a launch
    assert ctx.kzg_check_combinations(st.vk, cxy, np.zeros((0, L), dtype=np.uint64), np.zeros((0, m, L), dtype=np.uint64),
                                      np.zeros((0, L), dtype=np.uint64), np.zeros((0, cxy.shape[1]), dtype=np.uint64)) is True
    assert good() == (0, [1] + [7] * 69)
    st.vk.free()
    bare.vk.free()
