"""GPU: K11 -- the forward matrices and z_M on H, the placement of the assignment, the hiding multiples of v_H, the first sumcheck's q in
one launch, and the two drivers round1 / sumcheck1 -- bit-exact on the ABI Montgomery words against exact integers
(tests/marlin_round1_reference.py).  Domain elements come from the oracle's transforms, never from the library."""
import ctypes as C
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marlin_reference as mr  # noqa: E402
import marlin_round1_reference as m1  # noqa: E402

pytestmark = pytest.mark.gpu

LONG_ROW = 16       # a row of more entries than this is a wave's (common.h SPMV_LONG_ROW)
FLUSH = 48          # small coefficients a lane sums before it reduces (inst_field.hip SPMV_FLUSH)
ADICITY = [17, 34, 15, 30]
MIXED_M = {0: 49, 2: 25}  # the odd factor of the mixed-radix D behind |H| = 2^(adicity - 1): 49 * 2^12 (field 0), 25 * 2^11 (field 2)
SHAPES = [(1, 1, 1, 1), (5, 7, 8, 2), (8, 8, 8, 8), (60, 64, 64, 4), (300, 257, 512, 16)]  # rows, cols, |H|, |X|: K9's
BLINDS = [(0, 0, 0), (1, 1, 1), (2, 1, 0)]


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


_DOM = {}


def domain(co, field, n, m=1):
    if (field, n) not in _DOM:
        _DOM[(field, n)] = mr.domain_elements(co, field, n, m)
    return _DOM[(field, n)]


def mont(co, field, ints):
    return mr.to_mont(co, field, ints)


def upload(ctx, co, field, ints):
    return ctx.buf_upload(field, mont(co, field, ints))


def ints_of(co, field, buf, n=None):
    v = mr.to_ints(co, field, buf.download())
    return v if n is None else v[:n]


def free(*bufs):
    for b in bufs:
        if b is not None and not isinstance(b, list):
            b.free()


def oracle_interp(co, field):
    """evaluations on a radix-2 domain -> coefficients by the oracle's inverse transform (the host test ties it to the quadratic one)"""
    def interp(evals, dom, p):
        if len(evals) == 1:
            return list(evals)
        return mr.to_ints(co, field, co.fft(field, mont(co, field, evals), inverse=True))
    return interp


def csr_of(co, field, entries, rows):
    by_row = [[] for _ in range(rows)]
    for r, c, v in entries:
        by_row[r].append((c, v))
    rp = np.zeros(rows + 1, dtype=np.uint64)
    cols, vals = [], []
    for r in range(rows):
        rp[r + 1] = rp[r] + len(by_row[r])
        cols += [c for c, _ in by_row[r]]
        vals += [v for _, v in by_row[r]]
    return rp, np.array(cols, dtype=np.uint32), mont(co, field, vals).reshape(len(vals), mr.LIMBS[field])


def r1cs_of(co, field, mats, rows, cols):
    a, b, c = (csr_of(co, field, m, rows) for m in mats)
    return SimpleNamespace(rp_a=a[0], col_a=a[1], coeff_a=a[2], rp_b=b[0], col_b=b[1], coeff_b=b[2], rp_c=c[0], col_c=c[1], coeff_c=c[2],
                           num_vars=cols)


def planted_matrix(rnd, p, rows, cols, heavy_row):
    """random entries plus: an empty column (1) and an empty row (rows - 2) where the shape allows, one row of more than FLUSH small
    coefficients followed by general ones (more than LONG_ROW entries: the long-row kernel's), the coefficients +-1, +-32, +-33, 0,
    p - 1, and a duplicated (r, c)"""
    special = [1, p - 1, 32, p - 32, 33, p - 33, 0, p - 1]
    entries = []
    for r in range(rows):
        for _ in range(rnd.randrange(0, 4)):
            entries.append((r, rnd.randrange(cols), rnd.choice(special + [rnd.randrange(p)] * 4)))
    entries += [(rnd.randrange(rows), cols - 1, v) for v in special]
    if cols > FLUSH + 5:
        entries += [(heavy_row, c, rnd.choice([1, p - 1, 2, p - 3, 32, p - 32])) for c in range(FLUSH + 5)]
        entries += [(heavy_row, rnd.randrange(cols), rnd.randrange(p)) for _ in range(7)]
    if entries:
        entries.append(entries[0])
        entries.append(entries[len(entries) // 2])
    if cols > 2:
        entries = [e for e in entries if e[1] != 1]
    if rows > 3:
        entries = [e for e in entries if e[0] != rows - 2]
    return entries


# ------------------------------------------------------------------------------------------------------------ the fused kernel
@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_sumcheck1_q_bit_exact(ctx, co, field):
    rnd = random.Random(1200 + field)
    p = mr.MODULI[field]
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
        vecs = [[rnd.randrange(p) for _ in range(n)] for _ in range(5)]
        for k, v in enumerate(vecs):  # 0, 1 and p - 1 planted in every vector, at places that differ from vector to vector
            for j, x in enumerate((0, 1, p - 1)):
                if n:
                    v[(5 * j + k) % n] = x
        bufs = [upload(ctx, co, field, v) for v in vecs]
        for eta in ([rnd.randrange(p) for _ in range(3)], [1, rnd.randrange(p), 0], [0, 0, 0]):
            want = mont(co, field, m1.sumcheck1_q(eta, *vecs, p))
            q = ctx.marlin_sumcheck1_q(mont(co, field, eta), *bufs)
            assert q.n == n and np.array_equal(q.download(), want), (field, n, eta[:1])
            q.free()
        for k in (0, 3):  # q_out aliasing za, then t; the other inputs are left alone
            eta = [rnd.randrange(p) for _ in range(3)]
            want = mont(co, field, m1.sumcheck1_q(eta, *vecs, p))
            alias = upload(ctx, co, field, vecs[k])
            args = list(bufs)
            args[k] = alias
            out = ctx.marlin_sumcheck1_q(mont(co, field, eta), *args, out=alias)
            assert out is alias and np.array_equal(alias.download(), want), (field, n, k)
            assert all(np.array_equal(bufs[j].download(), mont(co, field, vecs[j])) for j in range(5))
            alias.free()
        free(*bufs)


def test_sumcheck1_q_output_on_two_inputs_means_one_vector(ctx, co):
    """the header's rule: buffers never overlap in part, so q_out on two inputs means that both ARE that vector -- legal, za = zb = q"""
    field, n = 1, 300
    rnd = random.Random(1210)
    p = mr.MODULI[field]
    v, r, t, z = ([rnd.randrange(p) for _ in range(n)] for _ in range(4))
    eta = [rnd.randrange(p) for _ in range(3)]
    bv, br, bt, bz = (upload(ctx, co, field, x) for x in (v, r, t, z))
    ctx.marlin_sumcheck1_q(mont(co, field, eta), bv, bv, br, bt, bz, out=bv)
    assert np.array_equal(bv.download(), mont(co, field, m1.sumcheck1_q(eta, v, v, r, t, z, p)))
    free(bv, br, bt, bz)


# ---------------------------------------------------------------------------------------------- placement and the forward mat-vec
@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_place_assignment_and_zm_evals_bit_exact(ctx, co, field):
    rnd = random.Random(1220 + field)
    p = mr.MODULI[field]
    for rows, cols, h_n, x_n in SHAPES:
        z = [rnd.randrange(p) for _ in range(cols)]
        zb = upload(ctx, co, field, z)
        placed = ctx.marlin_place_assignment(field, h_n, x_n, zb)
        assert placed.n == h_n and np.array_equal(placed.download(), mont(co, field, m1.place(z, h_n, x_n))), (field, h_n, x_n)
        if cols > 2:  # fewer variables than the buffer holds: the rest read as zero
            ctx.marlin_place_assignment(field, h_n, x_n, zb, num_cols=cols - 2, out=placed)
            assert np.array_equal(placed.download(), mont(co, field, m1.place(z, h_n, x_n, num_cols=cols - 2)))
        mats = [planted_matrix(rnd, p, rows, cols, heavy_row=min(rows - 1, 2 + k)) for k in range(3)]
        if cols > FLUSH + 5:
            assert max(sum(1 for e in mats[0] if e[0] == r) for r in range(rows)) > FLUSH + 5 > LONG_ROW
        handle = ctx.marlin_mats_upload_ex(field, r1cs_of(co, field, mats, rows, cols), h_n, x_n, 2)
        want = [mont(co, field, m1.zm_evals(m, z, h_n, p)) for m in mats]
        assert rows == h_n or not want[0][rows:].any()
        za, zbv, zc = ctx.marlin_zm_evals(handle, zb)
        for got, w in zip((za, zbv, zc), want):
            assert got.n == h_n and np.array_equal(got.download(), w), (field, rows, cols, h_n)
        ctx.marlin_zm_evals(handle, zb, za=zc, zb=za, want_c=False)  # without C: A into the old zc, B into the old za
        assert np.array_equal(zc.download(), want[0]) and np.array_equal(za.download(), want[1])
        assert np.array_equal(zb.download(), mont(co, field, z))
        free(zb, placed, za, zbv, zc)
        handle.free()


# -------------------------------------------------------------------------------------------------- hiding multiples of v_H
@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_poly_add_vanishing_multiple_bit_exact(ctx, co, field):
    rnd = random.Random(1230 + field)
    p = mr.MODULI[field]
    for n in (8, 300):
        for k in (0, 1, 2):
            for ln in (n + k - 3, n + k, n + k + 5, 2):
                c, blind = [rnd.randrange(p) for _ in range(ln)], [rnd.randrange(p) for _ in range(k)]
                want = m1.add_vanishing_multiple(c, blind, n, p)
                buf = upload(ctx, co, field, c + [rnd.randrange(p) for _ in range(n + 8)])  # stale words beyond len must not leak in
                got_len = ctx.poly_add_vanishing_multiple(buf, mont(co, field, blind) if k else None, n, length=ln)
                assert got_len == len(want) == (max(ln, n + k) if k else ln)
                assert np.array_equal(buf.download()[:got_len], mont(co, field, want)), (field, n, k, ln)
                buf.free()
    # overlapping windows (k > domain_n): every touched coefficient is owned by one lane
    c, blind = [rnd.randrange(p) for _ in range(4)], [rnd.randrange(p) for _ in range(5)]
    buf = upload(ctx, co, field, c + [0] * 8)
    assert ctx.poly_add_vanishing_multiple(buf, mont(co, field, blind), 2, length=4) == 7
    assert np.array_equal(buf.download()[:7], mont(co, field, m1.add_vanishing_multiple(c, blind, 2, p)))
    buf.free()


# ------------------------------------------------------------------------------------------------------------------ the drivers
def check_round1(co, field, got, want, ks, h_n, x_n):
    names = ("x_hat", "z_poly", "w", "za_poly", "zb_poly")
    assert got["lens"] == [len(want[k]) for k in names] == [x_n, h_n + ks[0], h_n + ks[0] - x_n, h_n + ks[1], h_n + ks[2]]
    for name in names + ("w_rem", "za_evals", "zb_evals"):
        if got[name] is None:
            assert want[name] == [], name
            continue
        assert np.array_equal(got[name].download()[:len(want[name])], mont(co, field, want[name])), (field, h_n, ks, name)
    assert not got["w_rem"].download().any()


def check_sumcheck1(co, field, got, want, h_n):
    assert got["lens"] == [h_n, len(want["h1"]), h_n - 1]
    for name in ("t_poly", "h1", "g1"):
        if got[name] is None:
            assert want[name] == [], name
        else:
            assert np.array_equal(got[name].download(), mont(co, field, want[name])), (field, h_n, name)
    assert np.array_equal(got["sigma"].download(), mont(co, field, [want["sigma"]]))


def free_outputs(d):
    free(*[v for k, v in d.items() if k != "lens"])


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_round1_and_sumcheck1_bit_exact(ctx, co, field):
    rnd = random.Random(1240 + field)
    p = mr.MODULI[field]
    interp = oracle_interp(co, field)
    for rows, cols, h_n, x_n in SHAPES[1:]:
        dom_h, dom_x = domain(co, field, h_n), domain(co, field, x_n)
        mats, z = m1.satisfied_system(rnd, p, rows, cols, x_n)
        mats[0] += [(0, c, rnd.choice([1, p - 1, 2])) for c in range(min(cols, LONG_ROW + 4))]  # a long row in A ...
        mats[2][0] = (0, mats[2][0][1], 0)
        c0 = mats[2][0][1]
        az, bz = m1.zm_evals(mats[0], z, h_n, p), m1.zm_evals(mats[1], z, h_n, p)
        mats[2][0] = (0, c0, az[0] * bz[0] % p * pow(z[c0], -1, p) % p)                        # ... and C's row 0 made to fit it again
        handle = ctx.marlin_mats_upload_ex(field, r1cs_of(co, field, mats, rows, cols), h_n, x_n, 3)
        zbuf = upload(ctx, co, field, z)
        bad = list(z)
        bad[c0] = (bad[c0] + 1) % p
        badbuf = upload(ctx, co, field, bad)
        for ks in BLINDS:
            blinds = [[rnd.randrange(p) for _ in range(k)] for k in ks]
            want = m1.round1(mats, z, h_n, x_n, dom_h, dom_x, blinds, p, interp)
            got = ctx.marlin_round1(handle, zbuf, *[mont(co, field, b) if b else None for b in blinds], want_evals=True)
            check_round1(co, field, got, want, ks, h_n, x_n)
            eta = [rnd.randrange(p) for _ in range(3)]
            alpha, beta = rnd.randrange(p), rnd.randrange(p)
            assert pow(alpha, h_n, p) != 1 and alpha != beta
            mask = m1.zero_sum_mask(rnd, p, h_n, 2 * h_n + 3 if ks[0] else 3 * h_n + 5)  # (the longer one outgrows the products)
            mbuf = upload(ctx, co, field, mask)
            for s, sb in ((mask, mbuf), (None, None)):
                wsc = m1.sumcheck1(mats, eta, alpha, want["za_poly"], want["zb_poly"], want["z_poly"], s, h_n, x_n, dom_h, p, interp)
                sc = ctx.marlin_sumcheck1(handle, mont(co, field, eta), mont(co, field, [alpha])[0], got["za_poly"], got["zb_poly"], got["z_poly"],
                                          mask=sb)
                check_sumcheck1(co, field, sc, wsc, h_n)
                assert wsc["sigma"] == 0 and not sc["sigma"].download().any()  # a satisfied system, a mask summing to zero on H
                # the AHP verifier's equation at a random point, from the DOWNLOADED coefficients and Python's Horner
                dl = lambda d, k: ints_of(co, field, d[k]) if d[k] is not None else []
                polys = {k: dl(got, k) for k in ("za_poly", "zb_poly", "z_poly")}
                outs = {k: dl(sc, k) for k in ("t_poly", "h1", "g1")}
                outs["sigma"] = ints_of(co, field, sc["sigma"])[0]
                assert m1.verifier_equation_holds(eta, alpha, beta, polys, outs, s, h_n, p)
                free_outputs(sc)
            # one entry of z changed afterwards: the constant term is no longer zero
            gb = ctx.marlin_round1(handle, badbuf, *[mont(co, field, b) if b else None for b in blinds])
            sb = ctx.marlin_sumcheck1(handle, mont(co, field, eta), mont(co, field, [alpha])[0], gb["za_poly"], gb["zb_poly"], gb["z_poly"], mask=mbuf)
            wb = m1.round1(mats, bad, h_n, x_n, dom_h, dom_x, blinds, p, interp)
            wsb = m1.sumcheck1(mats, eta, alpha, wb["za_poly"], wb["zb_poly"], wb["z_poly"], mask, h_n, x_n, dom_h, p, interp)
            assert wsb["sigma"] != 0 and sb["sigma"].download().any()
            check_sumcheck1(co, field, sb, wsb, h_n)
            free_outputs(got), free_outputs(gb), free_outputs(sb), mbuf.free()
        free(zbuf, badbuf)
        handle.free()


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_round1_divides_by_a_small_x(ctx, co, field):
    """|H| + k_w beyond 64 |X|: the driver forms w by doubling strided suffix sums instead of one stride-|X| column per lane
    (capi_marlin.hip div_vanishing_small_n); 65 |X| is the first length that takes that path, |X| = 1 the longest columns"""
    rnd = random.Random(1250 + field)
    p = mr.MODULI[field]
    interp = oracle_interp(co, field)
    for rows, cols, h_n, x_n, ks in ((300, 257, 512, 4, (0, 0, 0)), (40, 500, 512, 2, (3, 1, 0)), (60, 64, 64, 1, (1, 0, 2)), (9, 30, 128, 2, (0, 1, 1))):
        assert h_n + ks[0] > 64 * x_n or (h_n, x_n) == (128, 2)  # (128 = 64 |X| exactly: the last length of the direct kernel)
        dom_h, dom_x = domain(co, field, h_n), domain(co, field, x_n)
        mats, z = m1.satisfied_system(rnd, p, rows, cols, x_n)
        blinds = [[rnd.randrange(p) for _ in range(k)] for k in ks]
        handle = ctx.marlin_mats_upload_ex(field, r1cs_of(co, field, mats, rows, cols), h_n, x_n, 2)
        zbuf = upload(ctx, co, field, z)
        got = ctx.marlin_round1(handle, zbuf, *[mont(co, field, b) if b else None for b in blinds], want_evals=True)
        check_round1(co, field, got, m1.round1(mats, z, h_n, x_n, dom_h, dom_x, blinds, p, interp), ks, h_n, x_n)
        assert any(ints_of(co, field, got["w"]))
        free_outputs(got)
        zbuf.free()
        handle.free()


@pytest.mark.parametrize("field", [1, 3])
def test_chain_without_downloads_commits_match(ctx, co, field):
    """marlin_index_build -> round1 -> sumcheck1 -> kzg_commit of w, z_A, z_B, t, g_1, h_1 with nothing downloaded in between; the
    commitments equal those of the reference's coefficients uploaded afresh"""
    curve = {1: 0, 3: 2}[field]  # the curve whose scalar field this is
    rnd = random.Random(1260 + field)
    p = mr.MODULI[field]
    rows, cols, h_n, x_n = 60, 64, 64, 4
    dom_h, dom_x = domain(co, field, h_n), domain(co, field, x_n)
    interp = oracle_interp(co, field)
    mats, z = m1.satisfied_system(rnd, p, rows, cols, x_n)
    r1cs = r1cs_of(co, field, mats, rows, cols)
    blinds = [[rnd.randrange(p)], [rnd.randrange(p)], [rnd.randrange(p)]]
    eta, alpha = [rnd.randrange(p) for _ in range(3)], rnd.randrange(p)
    mask = m1.zero_sum_mask(rnd, p, h_n, 3 * h_n)
    idx = ctx.marlin_index_build(field, r1cs, h_n, x_n, keep=1)
    handle = ctx.marlin_mats_upload_ex(field, r1cs, h_n, x_n, 3)
    zbuf, mbuf = upload(ctx, co, field, z), upload(ctx, co, field, mask)
    powers = ctx.bases_upload(curve, 1, co.gen_points(curve, 1, 4 * h_n, seed=1261))
    r1 = ctx.marlin_round1(handle, zbuf, *[mont(co, field, b) for b in blinds])
    sc = ctx.marlin_sumcheck1(handle, mont(co, field, eta), mont(co, field, [alpha])[0], r1["za_poly"], r1["zb_poly"], r1["z_poly"], mask=mbuf)
    items = [r1["w"], r1["za_poly"], r1["zb_poly"], sc["t_poly"], sc["g1"], sc["h1"]]
    comm, inf, _, _, _ = ctx.kzg_commit(powers, [{"poly": b} for b in items])
    # only now the reference, and fresh uploads of ITS coefficients
    w1 = m1.round1(mats, z, h_n, x_n, dom_h, dom_x, blinds, p, interp)
    ws = m1.sumcheck1(mats, eta, alpha, w1["za_poly"], w1["zb_poly"], w1["z_poly"], mask, h_n, x_n, dom_h, p, interp)
    fresh = [upload(ctx, co, field, v) for v in (w1["w"], w1["za_poly"], w1["zb_poly"], ws["t_poly"], ws["g1"], ws["h1"])]
    want, want_inf, _, _, _ = ctx.kzg_commit(powers, [{"poly": b} for b in fresh])
    assert np.array_equal(comm, want) and np.array_equal(inf, want_inf) and not inf.any()
    assert len({comm[k].tobytes() for k in range(6)}) == 6
    free(zbuf, mbuf, *fresh)
    free_outputs(r1), free_outputs(sc)
    powers.free(), handle.free(), idx.free()


@pytest.mark.parametrize("field", [0, 2])
def test_sumcheck1_on_a_mixed_radix_d(ctx, co, field):
    """|H| = 2^(adicity - 1): the rule for D lands beyond the field's 2-adicity, on a mixed-radix size.  The reference goes the
    device's way with the oracle's transforms (fft on H, fft_general on D) and exact integers pointwise: no quadratic interpolation"""
    from pcd_amd import capi
    rnd = random.Random(1270 + field)
    p = mr.MODULI[field]
    h_n, x_n, m = 1 << (ADICITY[field] - 1), 4, MIXED_M[field]
    rows, cols = h_n - 5, h_n - 9
    d_n = capi.lib().pcdhip_domain_size(field, 3 * h_n - 2)
    assert d_n % m == 0 and (d_n // m) & (d_n // m - 1) == 0 and d_n > (1 << ADICITY[field]) and d_n == co.domain_size(field, 3 * h_n - 2)
    dom_h = domain(co, field, h_n)
    mats = [[(rnd.randrange(rows), rnd.randrange(cols), rnd.choice([1, p - 1, rnd.randrange(p)])) for _ in range(2000)] for _ in range(3)]
    seed = 12700 + field
    polys = [co.gen_field(field, h_n, seed=seed + k) for k in range(3)]  # za_poly, zb_poly, z_poly: any coefficients will do here
    eta, alpha = [rnd.randrange(p) for _ in range(3)], rnd.randrange(p)
    handle = ctx.marlin_mats_upload(field, r1cs_of(co, field, mats, rows, cols), h_n, x_n)
    bufs = [ctx.buf_upload(field, v) for v in polys]
    sc = ctx.marlin_sumcheck1(handle, mont(co, field, eta), mont(co, field, [alpha])[0], *bufs)
    # the reference: r and t on H, their coefficients, five forward transforms on D, q pointwise, back, the division
    r_ev = mr.bivariate_lagrange(alpha, dom_h, p)
    t_ev = mr.t_evals(mats, eta, r_ev, h_n, x_n, p)
    ifft_h = lambda ev: co.fft(field, mont(co, field, ev), inverse=True)
    t_poly = ifft_h(t_ev)
    pad = lambda v: np.concatenate([v, np.zeros((d_n - len(v), mr.LIMBS[field]), dtype=np.uint64)])
    on_d = [mr.to_ints(co, field, co.fft_general(field, pad(v), m)) for v in (polys[0], polys[1], ifft_h(r_ev), t_poly, polys[2])]
    q = m1.sumcheck1_q(eta, *on_d, p)
    q_coeffs = mr.to_ints(co, field, co.fft_general(field, mont(co, field, q), m, inverse=True))
    assert not any(q_coeffs[3 * h_n - 2:])
    h1, rem = m1.div_vanishing(q_coeffs[:3 * h_n - 2], h_n, p)
    assert sc["lens"] == [h_n, 2 * h_n - 2, h_n - 1]
    assert np.array_equal(sc["t_poly"].download(), t_poly)
    assert np.array_equal(sc["h1"].download(), mont(co, field, h1))
    assert np.array_equal(sc["g1"].download(), mont(co, field, rem[1:]))
    assert np.array_equal(sc["sigma"].download(), mont(co, field, rem[:1]))
    free(*bufs)
    free_outputs(sc)
    handle.free()


# ------------------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(ctx, co):
    from pcd_amd import capi
    field, p = 1, mr.MODULI[1]
    rnd = random.Random(1290)
    rows, cols, h_n, x_n = 5, 7, 8, 2
    mats, z = m1.satisfied_system(rnd, p, rows, cols, x_n)
    r1cs = r1cs_of(co, field, mats, rows, cols)
    arg = lambda: pytest.raises(capi.PcdHipError, match=r"rc=-1\b")
    for forms in (0, 4, 7):
        with arg():
            ctx.marlin_mats_upload_ex(field, r1cs, h_n, x_n, forms)
    with arg():
        ctx.marlin_mats_upload_ex(field, r1cs, h_n, 3, 3)          # |X| is no domain size
    with arg():
        ctx.marlin_mats_upload_ex(field, r1cs, h_n, x_n, 2, num_cols=6)  # a column index beyond num_cols
    only_t, only_fwd, both = (ctx.marlin_mats_upload_ex(field, r1cs, h_n, x_n, f) for f in (1, 2, 3))
    plain = ctx.marlin_mats_upload(field, r1cs, h_n, x_n)
    assert plain.info() == only_t.info() == both.info()
    zb, other = upload(ctx, co, field, z), ctx.buf_alloc(0, 16)
    h8, h8b = (upload(ctx, co, field, [rnd.randrange(p) for _ in range(h_n)]) for _ in range(2))
    h7, one = ctx.buf_alloc(field, h_n - 1), ctx.buf_alloc(field, 1)
    eta, alpha = mont(co, field, [3, 4, 5]), mont(co, field, [7])[0]
    r_alpha = ctx.domain_bivariate_lagrange(field, h_n, alpha)
    # a handle lacking the form a call needs; t_evals over the handle with both forms equals the plain one
    for f in (lambda: ctx.marlin_zm_evals(only_t, zb), lambda: ctx.marlin_zm_evals(plain, zb), lambda: ctx.marlin_round1(only_t, zb),
              lambda: ctx.marlin_t_evals(only_fwd, eta, r_alpha), lambda: ctx.marlin_sumcheck1(only_fwd, eta, alpha, h8, h8, h8)):
        with arg():
            f()
    t1, t2 = ctx.marlin_t_evals(plain, eta, r_alpha), ctx.marlin_t_evals(both, eta, r_alpha)
    assert np.array_equal(t1.download(), t2.download())
    # short buffers and mixed fields
    bad = [
        lambda: ctx.marlin_zm_evals(both, one),                                   # fewer elements of z than columns
        lambda: ctx.marlin_zm_evals(both, zb, za=h7),                             # fewer outputs than |H|
        lambda: ctx.marlin_zm_evals(both, zb, za=h8, zb=h8),                      # one vector for two outputs
        lambda: ctx.marlin_zm_evals(both, zb, za=other),                          # another field
        lambda: ctx.marlin_place_assignment(field, h_n, x_n, zb, out=h7),
        lambda: ctx.marlin_place_assignment(field, h_n, x_n, zb, num_cols=cols + 1),
        lambda: ctx.marlin_place_assignment(field, h_n, x_n, zb, out=zb),
        lambda: ctx.marlin_place_assignment(field, 12, x_n, zb, out=other),       # no domain size (and another field)
        lambda: ctx.marlin_place_assignment(field, 4, 8, zb, out=h8),             # |X| does not divide |H|
        lambda: ctx.marlin_place_assignment(0, h_n, x_n, zb, out=h8),
        lambda: ctx.poly_add_vanishing_multiple(h8, mont(co, field, [1]), h_n),   # no room for |H| + 1 coefficients
        lambda: ctx.poly_add_vanishing_multiple(h8, mont(co, field, [1]), 4, length=h_n + 1),
        lambda: ctx.poly_add_vanishing_multiple(h8, mont(co, field, [1]), 0),
        lambda: ctx.marlin_sumcheck1_q(eta, h8, h8, h8, h8, h7, n=h_n),
        lambda: ctx.marlin_sumcheck1_q(eta, h8, h8, h8, h8, h8, n=h_n, out=h7),
        lambda: ctx.marlin_sumcheck1_q(eta, h8, other, h8, h8, h8, n=h_n),
        lambda: ctx.marlin_sumcheck1(both, eta, alpha, h8, h8, h8, len_za=h_n + 1),
        lambda: ctx.marlin_sumcheck1(both, eta, alpha, h8, h8, h8, len_z=0),
        lambda: ctx.marlin_sumcheck1(both, eta, alpha, h8, other, h8),
        lambda: ctx.marlin_sumcheck1(both, eta, alpha, h8, h8, h8, domain_d_n=16),  # a domain, but below 3 |H| - 2 = 22
    ]
    for k, f in enumerate(bad):
        with arg():
            f()
    lib, lens = capi.lib(), (C.c_size_t * 5)()
    assert lib.pcdhip_marlin_sumcheck1_q(ctx._ctx, None, h8._h, h8._h, h8._h, h8._h, h8._h, h_n, h8b._h) == -1
    # round1 into buffers that are too short, shared, or of another field
    x2, w6, big = ctx.buf_alloc(field, x_n), ctx.buf_alloc(field, h_n - x_n), [ctx.buf_alloc(field, h_n + 1) for _ in range(3)]
    r1 = lambda **kw: lib.pcdhip_marlin_round1(ctx._ctx, both._h, zb._h, None, 0, None, 0, None, 0, *[kw.get(k, d)._h for k, d in (
        ("x_hat", x2), ("z_poly", big[0]), ("w", w6), ("w_rem", one), ("za_poly", big[1]), ("zb_poly", big[2]))], None, None, lens)
    assert r1() == -1                                  # w_rem of one element
    rem2 = ctx.buf_alloc(field, x_n)
    assert r1(w_rem=rem2) == 0                         # the well-formed call
    assert r1(w_rem=rem2, z_poly=h7) == -1 and r1(w_rem=rem2, za_poly=big[2]) == -1 and r1(w_rem=rem2, x_hat=other) == -1
    blind = mont(co, field, [9])
    assert lib.pcdhip_marlin_round1(ctx._ctx, both._h, zb._h, None, 1, None, 0, None, 0, x2._h, big[0]._h, big[1]._h, rem2._h, big[2]._h,
                                    h8._h, None, None, lens) == -1   # k_w = 1 without coefficients
    assert lib.pcdhip_marlin_round1(ctx._ctx, both._h, zb._h, blind.ctypes.data, 1, None, 0, None, 0, x2._h, h8._h, big[1]._h, rem2._h,
                                    big[2]._h, big[0]._h, None, None, lens) == -1   # z_poly without room for |H| + 1
    # D that is no domain: PCDHIP_E_SIZE_UNSUPPORTED
    with pytest.raises(capi.PcdHipError, match=r"rc=-2\b"):
        ctx.marlin_sumcheck1(both, eta, alpha, h8, h8, h8, domain_d_n=24)
    sc = ctx.marlin_sumcheck1(both, eta, alpha, h8, h8, h8, domain_d_n=64)  # the caller's own, larger D gives the rule's result
    sc2 = ctx.marlin_sumcheck1(both, eta, alpha, h8, h8, h8)
    assert sc["lens"] == sc2["lens"] == [h_n, 2 * h_n - 2, h_n - 1] and np.array_equal(sc["h1"].download(), sc2["h1"].download())
    free(zb, other, h8, h8b, h7, one, r_alpha, t1, t2, x2, w6, rem2, *big)
    free_outputs(sc), free_outputs(sc2)
    for h in (only_t, only_fwd, both, plain):
        h.free()

