"""GPU: K9 -- r(alpha, .) on H, t on H over the resident transposed matrices, the rational sumcheck's a, b and f -- bit-exact on the ABI
Montgomery words against exact integers (tests/marlin_reference.py), and the two rounds end to end on the device.  Domain elements
come from the oracle's transforms, never from the library."""
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marlin_reference as mr  # noqa: E402

pytestmark = pytest.mark.gpu

SEG = 4096          # entries per segment of a long transposed row (common.h MARLIN_T_SEG)
LONG_ROW = 16       # a transposed row of more entries than this is cut into segments (common.h SPMV_LONG_ROW)
FLUSH = 48          # small coefficients a lane sums before it reduces (inst_field.hip SPMV_FLUSH)
ADICITY = [17, 34, 15, 30]
MIXED_M = {0: 49, 2: 5}  # the odd factor of the smallest mixed-radix domain: 49 * 2^12 (field 0), 5 * 2^13 (field 2)
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


_DOM = {}


def domain(co, field, n, m=1):
    if (field, n) not in _DOM:
        _DOM[(field, n)] = mr.domain_elements(co, field, n, m)
    return _DOM[(field, n)]


def upload(ctx, co, field, ints):
    return ctx.buf_upload(field, mr.to_mont(co, field, ints))


def mont(co, field, ints):
    return mr.to_mont(co, field, ints)


def free(*bufs):
    for b in bufs:
        if b is not None:
            b.free()


# ---------------------------------------------------------------------------------------------------------------- r(alpha, .) on H
def check_lagrange(ctx, co, field, dom, rnd):
    p, n = mr.MODULI[field], len(dom)
    xs = [rnd.randrange(p), 0, p - 1, 1, dom[3 % n]]
    for k, x in enumerate(xs):
        want = mr.bivariate_lagrange(x, dom, p)
        if k >= 3 or (x == p - 1 and n % 2 == 0):
            assert want == [0] * n  # 1, w^3 (and -1 in a domain of even size) lie in H
        out = ctx.domain_bivariate_lagrange(field, n, mont(co, field, [x])[0])
        assert np.array_equal(out.download(), mont(co, field, want)), (field, n, k)
        out.free()


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_lagrange_radix2_bit_exact(ctx, co, field):
    rnd = random.Random(900 + field)
    for n in (1, 2, 4, 64, 1024, 2048, 4096):
        check_lagrange(ctx, co, field, domain(co, field, n), rnd)


@pytest.mark.parametrize("field", [0, 2])
def test_lagrange_mixed_radix_bit_exact(ctx, co, field):
    from pcd_amd import capi
    n = capi.lib().pcdhip_domain_size(field, (1 << ADICITY[field]) + 1)
    m = MIXED_M[field]
    assert n % m == 0 and (n // m) & (n // m - 1) == 0 and n == co.domain_size(field, (1 << ADICITY[field]) + 1)
    check_lagrange(ctx, co, field, domain(co, field, n, m), random.Random(910 + field))


def test_lagrange_refuses_non_domain_sizes(ctx, co):
    from pcd_amd import capi
    x = mont(co, 1, [5])[0]
    buf = ctx.buf_alloc(1, 8)
    for n in (3, 0, 6):
        with pytest.raises(capi.PcdHipError, match=r"rc=-2\b"):
            ctx.domain_bivariate_lagrange(1, n, x, out=buf)
    other = ctx.buf_alloc(0, 8)
    for bad in (lambda: ctx.domain_bivariate_lagrange(1, 16, x, out=buf),   # 16 outputs into 8
                lambda: ctx.domain_bivariate_lagrange(1, 8, x, out=other)):  # a buffer of another field
        with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
            bad()
    free(buf, other)


# ---------------------------------------------------------------------------------------------------------------------- t on H
def csr_of(co, field, entries, rows):
    """(rp, col, coeff) of a list of (r, c, v) entries, in the order given inside a row (duplicates stay separate entries)"""
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


def planted_matrix(rnd, p, rows, cols, x_n, heavy_col):
    """random entries plus: an empty column (1) and an empty row (rows - 2) where the shape allows, a column of more than FLUSH small
    coefficients (more than LONG_ROW entries: a wave's), the coefficients +-1, +-32, +-33, 0, p - 1, a duplicated (r, c), and the last
    column (>= |X| when cols > x_n)"""
    special = [1, p - 1, 32, p - 32, 33, p - 33, 0, p - 1]
    entries = []
    for r in range(rows):
        for _ in range(rnd.randrange(0, 4)):
            entries.append((r, rnd.randrange(cols), rnd.choice(special + [rnd.randrange(p)] * 4)))
    entries += [(rnd.randrange(rows), cols - 1, v) for v in special]
    if rows > FLUSH + 5:
        entries += [(r, heavy_col, rnd.choice([1, p - 1, 2, p - 3, 32, p - 32])) for r in range(FLUSH + 5)]
    if entries:
        entries.append(entries[0])
        entries.append(entries[len(entries) // 2])
    if cols > 2:
        entries = [e for e in entries if e[1] != 1]
    if rows > 3:
        entries = [e for e in entries if e[0] != rows - 2]
    return entries


def check_t(ctx, co, field, mats, rows, cols, h_n, x_n, rnd, etas=None):
    p = mr.MODULI[field]
    r_alpha = [rnd.randrange(p) for _ in range(rows)]
    handle = ctx.marlin_mats_upload(field, r1cs_of(co, field, mats, rows, cols), h_n, x_n)
    rbuf = upload(ctx, co, field, r_alpha)
    for eta in etas or ([1, rnd.randrange(p), 0], [rnd.randrange(p) for _ in range(3)]):
        want = mr.t_evals(mats, eta, r_alpha, h_n, x_n, p)
        out = ctx.marlin_t_evals(handle, mont(co, field, eta), rbuf)
        assert out.n == h_n and np.array_equal(out.download(), mont(co, field, want)), (field, rows, cols, h_n, x_n)
        out.free()
    info = handle.info()
    rbuf.free()
    handle.free()
    return info


T_SHAPES = [(1, 1, 1, 1), (5, 7, 8, 2), (8, 8, 8, 8), (60, 64, 64, 4), (300, 257, 512, 16)]


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_t_evals_bit_exact(ctx, co, field):
    rnd = random.Random(920 + field)
    p = mr.MODULI[field]
    for rows, cols, h_n, x_n in T_SHAPES:
        mats = [planted_matrix(rnd, p, rows, cols, x_n, heavy_col=min(cols - 1, 3 + k)) for k in range(3)]
        assert cols == 1 or any(c == cols - 1 for _, c, _ in mats[0])
        info = check_t(ctx, co, field, mats, rows, cols, h_n, x_n, rnd)
        assert info["seg_len"] == SEG and info["launches"] == (3 if info["segments"] else 1)
        if rows > FLUSH + 5:
            assert info["segments"] >= 3  # the heavy columns are beyond a lane's share: a wave each


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_t_evals_long_rows_are_cut_into_segments(ctx, co, field):
    """2 SEG + 3 constraints that all mention variable 0, in all three matrices: two full segments and a partial one per matrix.  Two
    thirds of the coefficients are small and come first in the row, so every lane of the first segment's wave sums SEG / 64 > FLUSH of them"""
    from pcd_amd import capi
    rnd = random.Random(930 + field)
    p = mr.MODULI[field]
    rows, cols = 2 * SEG + 3, 5
    h_n = capi.lib().pcdhip_domain_size(field, rows)
    assert h_n == 16384
    small = [1, p - 1, 2, p - 32, 33, 0]
    mats = []
    for k in range(3):
        m = [(r, 0, rnd.choice(small) if (r + k) % 3 else rnd.randrange(p)) for r in range(rows)]
        m += [(rnd.randrange(rows), 1 + rnd.randrange(cols - 1), rnd.randrange(p)) for _ in range(40)]
        mats.append(m)
    info = check_t(ctx, co, field, mats, rows, cols, h_n, 4, rnd)
    # every row of L > SEG entries is served by ceil(L / SEG) waves: here three per matrix, all owned by output pi(0) = 0
    assert info["segments"] == 9 and info["long_outputs"] == 1 and info["launches"] == 3


def test_t_evals_argument_errors(ctx, co):
    from pcd_amd import capi
    field, p = 1, mr.MODULI[1]
    m = [(0, 0, 1), (1, 2, 5), (3, 6, p - 1)]
    ok = r1cs_of(co, field, [m, m, m], 5, 7)
    bad_uploads = [
        lambda: ctx.marlin_mats_upload(field, ok, 8, 3),    # |X| is no domain size
        lambda: ctx.marlin_mats_upload(field, ok, 12, 4),   # |H| is no domain size
        lambda: ctx.marlin_mats_upload(field, ok, 4, 8),    # |X| does not divide |H|
        lambda: ctx.marlin_mats_upload(field, ok, 4, 2),    # more rows (and columns) than |H|
        lambda: ctx.marlin_mats_upload(field, ok, 8, 2, num_cols=9),   # more columns than |H|
        lambda: ctx.marlin_mats_upload(field, ok, 8, 2, num_cols=6),   # a column index beyond num_cols
        lambda: ctx.marlin_mats_upload(field, r1cs_of(co, field, [m, m, m], 9, 7), 8, 2),  # more rows than |H|
    ]
    for f in bad_uploads:
        with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
            f()
    uneven = r1cs_of(co, field, [m, m, m], 5, 7)
    uneven.rp_c = np.concatenate([uneven.rp_c, uneven.rp_c[-1:]])  # C with one row more than A and B
    with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
        ctx.marlin_mats_upload(field, uneven, 8, 2)
    handle = ctx.marlin_mats_upload(field, ok, 8, 2)
    eta = mont(co, field, [1, 2, 3])
    r5, r4, t8, t7, r0 = (ctx.buf_alloc(field, 5), ctx.buf_alloc(field, 4), ctx.buf_alloc(field, 8), ctx.buf_alloc(field, 7),
                          ctx.buf_alloc(0, 8))
    for f in (lambda: ctx.marlin_t_evals(handle, eta, r4, out=t8),   # fewer elements of r than rows
              lambda: ctx.marlin_t_evals(handle, eta, r5, out=t7),   # fewer outputs than |H|
              lambda: ctx.marlin_t_evals(handle, eta, r0, out=t8),   # another field
              lambda: ctx.marlin_t_evals(handle, eta, t8, out=t8)):  # in place
        with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
            f()
    assert capi.lib().pcdhip_marlin_t_evals(ctx._ctx, handle._h, None, r5._h, t8._h) == E_ARG
    free(r5, r4, t8, t7, r0)
    handle.free()


# ------------------------------------------------------------------------------------------------------------- the rational sumcheck
def sumcheck_case(rnd, field, n):
    p = mr.MODULI[field]
    row, col, val = ([[rnd.randrange(p) for _ in range(n)] for _ in range(3)] for _ in range(3))
    alpha, beta = rnd.randrange(p), rnd.randrange(p)
    coeff = [rnd.randrange(p) for _ in range(3)]
    if n > 2:
        row[0][n // 2] = beta       # d_A = 0 in the product form: b = 0, f = 0
        val[1][1] = 0
        val[0][n - 1] = val[1][n - 1] = val[2][n - 1] = 0
    return alpha, beta, coeff, row, col, val


def up3(ctx, co, field, vecs):
    return [upload(ctx, co, field, v) for v in vecs]


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_sumcheck_ab_and_f_bit_exact(ctx, co, field):
    rnd = random.Random(940 + field)
    p = mr.MODULI[field]
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
        alpha, beta, coeff, row, col, val = sumcheck_case(rnd, field, n)
        prod = [[r * c % p for r, c in zip(row[m], col[m])] for m in range(3)]
        other = [[rnd.randrange(p) for _ in range(n)] for _ in range(3)]  # NOT row * col: the four-term form is what gets checked
        am, bm, cm = mont(co, field, [alpha])[0], mont(co, field, [beta])[0], mont(co, field, coeff)
        brow, bcol, bval, bprod, bother = (up3(ctx, co, field, v) for v in (row, col, val, prod, other))
        results = {}
        for name, rc_ints, rc_bufs in (("null", None, None), ("product", prod, bprod), ("given", other, bother)):
            a_want, b_want = mr.sumcheck_ab(alpha, beta, coeff, row, col, rc_ints, val, p)
            a, b = ctx.marlin_sumcheck_ab(am, bm, cm, brow, bcol, rc_bufs, bval)
            results[name] = (a.download(), b.download())
            assert a.n == n and np.array_equal(results[name][0], mont(co, field, a_want)), (field, n, name)
            assert np.array_equal(results[name][1], mont(co, field, b_want)), (field, n, name)
            f = ctx.marlin_sumcheck_f(am, bm, cm, brow, bcol, rc_bufs, bval)
            f_want = mr.sumcheck_f(alpha, beta, coeff, row, col, rc_ints, val, p)
            assert np.array_equal(f.download(), mont(co, field, f_want)), (field, n, name)
            if n > 2 and name != "given":
                assert b_want[n // 2] == 0 and f_want[n // 2] == 0 and f_want[n - 1] == 0
            free(a, b, f)
        assert np.array_equal(results["null"][0], results["product"][0]) and np.array_equal(results["null"][1], results["product"][1])
        if n == 257:  # entries of row_col all null are the null array; inputs are left alone
            a, b = ctx.marlin_sumcheck_ab(am, bm, cm, brow, bcol, [None, None, None], bval)
            assert np.array_equal(a.download(), results["null"][0]) and np.array_equal(b.download(), results["null"][1])
            assert np.array_equal(brow[0].download(), mont(co, field, row[0])) and np.array_equal(bval[2].download(), mont(co, field, val[2]))
            free(a, b)
        free(*brow, *bcol, *bval, *bprod, *bother)


def test_sumcheck_refuses_aliases_and_mismatches(ctx, co):
    from pcd_amd import capi
    field, n = 1, 9
    rnd = random.Random(95)
    alpha, beta, coeff, row, col, val = sumcheck_case(rnd, field, n)
    am, bm, cm = mont(co, field, [alpha])[0], mont(co, field, [beta])[0], mont(co, field, coeff)
    brow, bcol, bval, brc = (up3(ctx, co, field, v) for v in (row, col, val, row))
    o1, o2, small, wrong = ctx.buf_alloc(field, n), ctx.buf_alloc(field, n), ctx.buf_alloc(field, n - 1), ctx.buf_alloc(0, n)
    ab = lambda a, b, rc=None, k=None: ctx.marlin_sumcheck_ab(am, bm, cm, brow, bcol, rc, bval, n=k, a_out=a, b_out=b)
    bad = [
        lambda: ab(o1, o1), lambda: ab(brow[1], o2), lambda: ab(o1, bcol[2]), lambda: ab(bval[0], o2), lambda: ab(o1, brc[1], rc=brc),
        lambda: ab(o1, small), lambda: ab(wrong, o2), lambda: ab(o1, o2, k=n + 1), lambda: ab(o1, o2, rc=[brc[0], None, brc[2]]),
        lambda: ab(o1, o2, rc=[brc[0], brc[1], wrong]),
        lambda: ctx.marlin_sumcheck_f(am, bm, cm, brow, bcol, None, bval, out=brow[0]),
        lambda: ctx.marlin_sumcheck_f(am, bm, cm, brow, bcol, brc, bval, out=brc[2]),
        lambda: ctx.marlin_sumcheck_f(am, bm, cm, brow, bcol, None, bval, out=small),
        lambda: ctx.marlin_sumcheck_f(am, bm, cm, brow, [bcol[0], bcol[1], wrong], None, bval, out=o1),
    ]
    for f in bad:
        with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
            f()
    assert np.array_equal(brow[1].download(), mont(co, field, row[1]))
    ab(o1, o2)  # and the well-formed call goes through
    a_want, _ = mr.sumcheck_ab(alpha, beta, coeff, row, col, None, val, mr.MODULI[field])
    assert np.array_equal(o1.download(), mont(co, field, a_want))
    free(o1, o2, small, wrong, *brow, *bcol, *bval, *brc)


# ------------------------------------------------------------------------------------------------------------------ rounds 2 and 3
@pytest.mark.parametrize("field", [1, 3])
def test_rounds_end_to_end_on_device(ctx, co, field):
    """r(alpha, .), t, t(beta), f on K with sum f = t(beta); then a, b on B, h_2 = (a - b f) / v_K with a zero remainder"""
    rnd = random.Random(960 + field)
    p = mr.MODULI[field]
    h_n, x_n, k_n = 64, 4, 256
    b_n = 4 * k_n
    dom_h, dom_k = domain(co, field, h_n), domain(co, field, k_n)
    rows, cols = 60, 64
    mats = []
    for _ in range(3):
        m = [(rnd.randrange(rows), rnd.randrange(cols), rnd.choice([1, p - 1, 2, rnd.randrange(p), rnd.randrange(p)])) for _ in range(rnd.randrange(200, 256))]
        m[7] = m[3]
        mats.append(m)
    alpha, beta = rnd.randrange(p), rnd.randrange(p)
    assert pow(alpha, h_n, p) != 1 and pow(beta, h_n, p) != 1
    eta = [1, rnd.randrange(p), rnd.randrange(p)]
    one = lambda x: mont(co, field, [x])[0]

    # round 2: r(alpha, .) on H, t on H, t(beta) through the inverse transform and an evaluation
    handle = ctx.marlin_mats_upload(field, r1cs_of(co, field, mats, rows, cols), h_n, x_n)
    r_alpha = ctx.domain_bivariate_lagrange(field, h_n, one(alpha))
    t = ctx.marlin_t_evals(handle, mont(co, field, eta), r_alpha)
    t_want = mr.t_evals(mats, eta, mr.bivariate_lagrange(alpha, dom_h, p), h_n, x_n, p)
    assert np.array_equal(t.download(), mont(co, field, t_want))
    ctx.fft(field, t, inverse=True)
    t_beta = mr.to_ints(co, field, ctx.poly_eval([t], one(beta)))[0]
    assert t_beta == mr.horner(mr.interpolate(t_want, dom_h, p), beta, p)

    # round 3 on K: the index's evaluations (the arithmetisation of tests/marlin_reference.py), f, and its sum
    vh = (pow(alpha, h_n, p) - 1) * (pow(beta, h_n, p) - 1) % p
    coeff = mont(co, field, [e * vh % p for e in eta])
    rows_k, cols_k, vals_k = zip(*[mr.arithmetize(m, dom_h, h_n, x_n, k_n, p) for m in mats])
    brow, bcol, bval = (up3(ctx, co, field, v) for v in (rows_k, cols_k, vals_k))
    brc = [ctx.vec_mul(r, c) for r, c in zip(brow, bcol)]
    f = ctx.marlin_sumcheck_f(one(alpha), one(beta), coeff, brow, bcol, brc, bval)
    f_ints = mr.to_ints(co, field, f.download())
    assert sum(f_ints) % p == t_beta

    # ... and on B: interpolate everything on K, pad to B, transform, a and b, a - b f, back, divide by v_K
    def to_b(buf):
        ctx.fft(field, buf, inverse=True)
        big = ctx.buf_upload(field, np.concatenate([buf.download(), np.zeros((b_n - k_n, mr.LIMBS[field]), dtype=np.uint64)]))
        ctx.fft(field, big)
        return big
    big = {}
    for name, bufs in (("row", brow), ("col", bcol), ("rc", brc), ("val", bval)):
        big[name] = [to_b(b) for b in bufs]
    f_b = to_b(f)
    f_coeffs = mr.to_ints(co, field, f.download())  # (f holds its coefficients now)
    a_b, b_b = ctx.marlin_sumcheck_ab(one(alpha), one(beta), coeff, big["row"], big["col"], big["rc"], big["val"])
    bf = ctx.vec_mul(b_b, f_b)
    diff = ctx.buf_alloc(field, b_n)
    assert ctx.poly_lincomb([a_b, bf], mont(co, field, [1, p - 1]), diff) == b_n
    a_evals, b_evals = mr.to_ints(co, field, a_b.download()), mr.to_ints(co, field, b_b.download())
    ctx.fft(field, diff, inverse=True)
    h2, ql, rem, rl = ctx.poly_div_vanishing(diff, k_n)
    assert (ql, rl) == (b_n - k_n, k_n)
    assert not rem.download().any()
    # h_2(z) (z^|K| - 1) = a(z) - b(z) f(z) at a random z, with a and b interpolated on B from the device's values
    dom_b = domain(co, field, b_n)
    z = rnd.randrange(p)
    lag = mr.batch_inverse([(z - w) % p for w in dom_b], p, (pow(z, b_n, p) - 1) * pow(b_n, -1, p) % p)   # L_i(z) / w^i
    at = lambda ev: sum(e * l % p * w for e, l, w in zip(ev, lag, dom_b)) % p
    h2_z = mr.horner(mr.to_ints(co, field, h2.download()), z, p)
    assert h2_z * (pow(z, k_n, p) - 1) % p == (at(a_evals) - at(b_evals) * mr.horner(f_coeffs, z, p)) % p
    # a on B is what the formula gives from the transformed inputs
    ints = {k: [mr.to_ints(co, field, b.download()) for b in v] for k, v in big.items()}
    a_want, b_want = mr.sumcheck_ab(alpha, beta, [e * vh % p for e in eta], ints["row"], ints["col"], ints["rc"], ints["val"], p)
    assert a_evals == a_want and b_evals == b_want
    assert ints["rc"][0] != [r * c % p for r, c in zip(ints["row"][0], ints["col"][0])]  # on B row_col is not the pointwise product
    free(r_alpha, t, f, f_b, a_b, b_b, bf, diff, h2, rem, *brow, *bcol, *bval, *brc, *[b for v in big.values() for b in v])
    handle.free()
