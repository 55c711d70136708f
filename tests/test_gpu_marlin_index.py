"""GPU: K10 -- the Marlin index on device.  The twelve vectors on K bit-exact on the ABI Montgomery words against exact integers
(tests/marlin_index_reference.py), the coefficients and the evaluations on B against the C++ oracle's transforms of those integers, the
twelve commitments against pcdhip_kzg_commit over the reference coefficients, and rounds 2 and 3 run from the index handle.  Domain
elements come from the oracle's transform of the unit vector, never from the library."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marlin_index_reference as mir  # noqa: E402
import marlin_reference as mr  # noqa: E402
from test_gpu_marlin_rounds import ADICITY, MIXED_M, domain, free, mont, r1cs_of, upload  # noqa: E402

pytestmark = pytest.mark.gpu

POLYS = ("row", "col", "row_col", "val")


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


def planted(rnd, p, rows, cols, n, empty=()):
    """n entries (n >= 16) over the rows outside `empty`: random places with the coefficients 1, p - 1, 2, an explicit 0 and random
    ones; one row given in descending column order with an equal pair; a duplicated (r, c) whose second coefficient is an explicit
    zero; the last column in the last live row"""
    live = [r for r in range(rows) if r not in empty]
    coeffs = lambda: rnd.choice([1, p - 1, 2, 0, rnd.randrange(p), rnd.randrange(p)])
    entries = [(rnd.choice(live), rnd.randrange(cols), coeffs()) for _ in range(n - 8)]
    mid = live[len(live) // 2]
    entries += [(mid, c, rnd.randrange(1, p)) for c in (cols - 1, cols // 2, cols // 2, min(3, cols - 1), 0)]
    entries += [entries[0], (entries[1][0], entries[1][1], 0), (live[-1], cols - 1, p - 1)]
    assert len(entries) == n
    return entries


def k_mont(co, field, vec, nnz):
    """the ABI image of a vector on K whose tail from nnz on is constant (the padding): the head converted, the tail tiled"""
    if nnz >= len(vec):
        return mont(co, field, vec)
    assert vec[nnz:] == [vec[nnz]] * (len(vec) - nnz)
    head = mont(co, field, vec[:nnz + 1])
    return np.concatenate([head[:nnz], np.tile(head[nnz:], (len(vec) - nnz, 1))])


def reference_forms(co, field, entries, dom_h, h_n, x_n, k_n, b_n, polys=range(4), nthreads=1):
    """{poly: (coefficients, evaluations on K, evaluations on B)} of one matrix as ABI rows"""
    p = mr.MODULI[field]
    vecs = mir.arithmetize(entries, dom_h, h_n, x_n, k_n, p)
    out = {}
    for q in polys:
        on_k = k_mont(co, field, vecs[q], len(entries))
        coeffs = mir.transform(co, field, on_k, inverse=True, nthreads=nthreads)
        padded = np.concatenate([coeffs, np.zeros((b_n - k_n, mr.LIMBS[field]), dtype=np.uint64)])
        out[q] = (coeffs, on_k, mir.transform(co, field, padded, nthreads=nthreads))
    return out


def build_and_check(ctx, co, field, mats, rows, cols, h_n, x_n, h_m=1):
    """build the index of `mats`, check its sizes and all 36 vectors -> (index, {matrix: reference_forms})"""
    dom_h = domain(co, field, h_n, h_m)
    nnz = [len(m) for m in mats]
    k_n = mir.domain_k(co, field, nnz)
    b_n = mir.domain_b(co, field, k_n)
    idx = ctx.marlin_index_build(field, r1cs_of(co, field, mats, rows, cols), h_n, x_n)
    info = idx.info()
    assert (info["domain_k_n"], info["domain_b_n"], info["max_nnz"]) == (k_n, b_n, max(nnz))
    assert info["device_bytes"] == 12 * (2 * k_n + b_n) * mr.LIMBS[field] * 8
    refs = {}
    for m in range(3):
        refs[m] = reference_forms(co, field, mats[m], dom_h, h_n, x_n, k_n, b_n)
        for q in range(4):
            for form in (1, 0, 2):
                v = idx.vec(form, m, q)
                assert v.n == (b_n if form == 2 else k_n)
                assert np.array_equal(v.download(), refs[m][q][form]), (field, h_n, x_n, "ABC"[m], POLYS[q], form)
    return idx, refs


# ------------------------------------------------------------------------------------------------------------------ 1: radix-2
@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_index_radix2_all_vectors(ctx, co, field):
    from pcd_amd import capi
    rnd = random.Random(1000 + field)
    p = mr.MODULI[field]
    rows, cols, h_n, x_n = 60, 64, 64, 4
    empty = (0, 1, 20, 21, 58, 59)  # empty first rows, two consecutive empty rows, empty last rows
    mats = [planted(rnd, p, rows, cols, n, empty) for n in (256, 200, 231)]
    for m in mats:
        order = mir.index_order(m)
        assert order != mir.csr_order(m) and len(set((r, c) for r, c, _ in m)) < len(m) and any(v == 0 for _, _, v in m)
    idx, _ = build_and_check(ctx, co, field, mats, rows, cols, h_n, x_n)
    assert (idx.info()["domain_k_n"], idx.info()["domain_b_n"]) == (256, 1024)
    full = idx.info()["device_bytes"]
    # evaluations on K only: fewer bytes held, the other two forms refused
    only_k = ctx.marlin_index_build(field, r1cs_of(co, field, mats, rows, cols), h_n, x_n, keep=2)
    assert only_k.info()["device_bytes"] == 12 * 256 * mr.LIMBS[field] * 8 < full
    assert np.array_equal(only_k.vec(1, 2, 3).download(), idx.vec(1, 2, 3).download())
    for form in (0, 2):
        with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
            only_k.vec(form, 0, 0)
    only_k.free()
    idx.free()


# ------------------------------------------------------------------------------------------------------------------- 2: shapes
@pytest.mark.parametrize("field", [1, 3])
def test_index_no_padding_and_an_empty_matrix(ctx, co, field):
    """nnz_A = |K| exactly, nnz_B = |K| / 2 + 1, C empty: all padding, whose coefficient vectors are (1, 0, ...) and 0"""
    rnd = random.Random(1010 + field)
    p = mr.MODULI[field]
    rows, cols, h_n, x_n = 60, 64, 64, 4
    mats = [planted(rnd, p, rows, cols, 256), planted(rnd, p, rows, cols, 129), []]
    idx, refs = build_and_check(ctx, co, field, mats, rows, cols, h_n, x_n)
    assert idx.info()["domain_k_n"] == 256
    one, zero = mont(co, field, [1]), mont(co, field, [0])
    for q in range(4):
        c = idx.vec(0, 2, q).download()
        assert np.array_equal(c[:1], zero if q == 3 else one) and not c[1:].any()
        assert np.array_equal(idx.vec(2, 2, q).download(), np.tile(zero if q == 3 else one, (1024, 1)))
    idx.free()


@pytest.mark.parametrize("field", [1, 3])
@pytest.mark.parametrize("x_n", [1, 2048])
def test_index_period_extremes_and_a_long_row(ctx, co, field, x_n):
    """|H| = 2048 with |X| = 1 (period = |H|) and |X| = |H| (period = 1: every column an instance column); one row of 700 entries
    spans several workgroups, about 3 000 entries in all (|K| = 4096: a ragged last workgroup of entries, then padding)"""
    rnd = random.Random(1020 + field)
    p = mr.MODULI[field]
    rows = cols = h_n = 2048
    mats = []
    for k in range(3):
        m = planted(rnd, p, rows, cols, 2300 - 100 * k, empty=(0, 5, 6, 2047))
        m += [(1000 + k, rnd.randrange(cols), rnd.randrange(p)) for _ in range(700)]
        m += [(2046, 2047, 1), (1, 0, p - 1)]
        mats.append(m)
    idx, _ = build_and_check(ctx, co, field, mats, rows, cols, h_n, x_n)
    assert (idx.info()["domain_k_n"], idx.info()["max_nnz"]) == (4096, 3002)
    idx.free()


@pytest.mark.parametrize("field", [1, 3])
def test_index_columns_on_both_sides_of_every_period_boundary(ctx, co, field):
    rnd = random.Random(1030 + field)
    p = mr.MODULI[field]
    rows, cols, h_n, x_n = 60, 64, 64, 4
    period = h_n // x_n
    edge = [3, 4, 4 + period - 2, 4 + period - 1]
    edge += [4 + k * (period - 1) + d for k in range(1, 4) for d in (-1, 0)] + [63]
    assert [mr.reindex(c, h_n, x_n) for c in edge[:4]] == [48, 1, 15, 17]
    mats = [[(rnd.randrange(rows), c, rnd.randrange(p)) for c in edge for _ in range(3)] for _ in range(3)]
    idx, _ = build_and_check(ctx, co, field, mats, rows, cols, h_n, x_n)
    idx.free()


# ------------------------------------------------------------------------------------------------------------- 3: mixed-radix H
@pytest.mark.parametrize("field", [0, 2])
def test_index_mixed_radix_h(ctx, co, field):
    """|H| beyond the field's 2-adicity: the transform keeps |H| / m powers, and rows and columns beyond them take the extra product"""
    from pcd_amd import capi
    rnd = random.Random(1040 + field)
    p = mr.MODULI[field]
    h_n = capi.lib().pcdhip_domain_size(field, (1 << ADICITY[field]) + 1)
    m_odd = MIXED_M[field]
    table = h_n // m_odd
    rows = cols = h_n
    x_n = 4
    first_past = next(c for c in range(cols) if mr.reindex(c, h_n, x_n) == table)
    mats = []
    for k in range(3):
        m = [(rnd.randrange(rows), rnd.randrange(cols), rnd.choice([1, p - 1, 2, rnd.randrange(p)])) for _ in range(290 + k)]
        m += [(h_n - 1, cols - 1, rnd.randrange(p)), (table, first_past, rnd.randrange(p)), (table - 1, first_past - 1, 1), (0, 0, 2),
              (table * (m_odd - 1), 1, rnd.randrange(p))]
        mats.append(m)
    assert mr.reindex(cols - 1, h_n, x_n) == h_n - 1
    idx, _ = build_and_check(ctx, co, field, mats, rows, cols, h_n, x_n, h_m=m_odd)
    assert idx.info()["domain_k_n"] == 512
    idx.free()


# ------------------------------------------------------------------------------------------------------- 4: mixed-radix K and B
def test_index_mixed_radix_k_and_b(ctx, co):
    field = 0
    rnd = random.Random(1050)
    p = mr.MODULI[field]
    h_n, x_n = 1 << 17, 64
    rows = cols = h_n
    nnz_a = (1 << 17) + 1
    a = [(r, rnd.randrange(cols), rnd.choice([1, p - 1, 2, rnd.randrange(p)])) for r in range(rows)] + [(rows - 1, cols - 1, 5)]
    mats = [a, [(3, 9, 1), (3, 2, p - 1), (70000, 131071, 7)], [(0, 0, 2), (131071, 1, rnd.randrange(p))]]
    k_n, b_n = 200704, 802816
    assert len(a) == nnz_a and mir.domain_k(co, field, [len(m) for m in mats]) == k_n and mir.domain_b(co, field, k_n) == b_n
    dom_h = domain(co, field, h_n)
    idx = ctx.marlin_index_build(field, r1cs_of(co, field, mats, rows, cols), h_n, x_n)
    info = idx.info()
    assert (info["domain_k_n"], info["domain_b_n"], info["max_nnz"]) == (k_n, b_n, nnz_a)
    for m in range(3):
        vecs = mir.arithmetize(mats[m], dom_h, h_n, x_n, k_n, p)
        for q in range(4):
            assert np.array_equal(idx.vec(1, m, q).download(), k_mont(co, field, vecs[q], len(mats[m]))), ("ABC"[m], POLYS[q])
    ref = reference_forms(co, field, mats[0], dom_h, h_n, x_n, k_n, b_n, polys=(2, 3), nthreads=16)
    for q in (2, 3):
        assert np.array_equal(idx.vec(0, 0, q).download(), ref[q][0]), POLYS[q]
        assert np.array_equal(idx.vec(2, 0, q).download(), ref[q][2]), POLYS[q]
    idx.free()


def test_fft_general_dev_matches_the_host_entry_point(ctx, co):
    from pcd_amd import capi
    field, n = 0, 200704
    x = co.gen_field(field, n + 5, seed=77)
    for inverse in (False, True):
        for coset in (False, True):
            buf = ctx.buf_upload(field, x)
            ctx.fft_general_dev(buf, n=n, inverse=inverse, coset=coset)
            got = buf.download()
            assert np.array_equal(got[:n], ctx.fft_general(field, x[:n], inverse=inverse, coset=coset)), (inverse, coset)
            assert np.array_equal(got[n:], x[n:])  # the elements past n are left alone
            buf.free()
    buf = ctx.buf_upload(field, x[:100])
    with pytest.raises(capi.PcdHipError, match=r"rc=-2\b"):
        ctx.fft_general_dev(buf, n=3 * 32)      # no domain size
    with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
        ctx.fft_general_dev(buf, n=128)         # more than the buffer holds
    small = ctx.fft_general_dev(buf, n=56)      # 7 * 2^3
    assert np.array_equal(small.download()[:56], co.fft_general(field, x[:56], 7))
    buf.free()


# ------------------------------------------------------------------------------------------------- 5: pcdhip_poly_evals_on_domain
@pytest.mark.parametrize("field,domain_n", [(1, 64), (3, 64), (0, 56), (1, 1)])
def test_poly_evals_on_domain(ctx, co, field, domain_n):
    from pcd_amd import capi
    L = mr.LIMBS[field]
    x = co.gen_field(field, domain_n + 9, seed=80 + field)
    p_buf = ctx.buf_upload(field, x)
    for length in sorted({1, domain_n, max(domain_n // 2 - 3, 1)}):
        for coset in (False, True):
            padded = np.concatenate([x[:length], np.zeros((domain_n - length, L), dtype=np.uint64)])
            m = mir.odd_part(field, domain_n)
            if domain_n == 1:
                want = padded
            else:
                want = co.fft(field, padded, coset=coset) if m == 1 else co.fft_general(field, padded, m, coset=coset)
            out = ctx.poly_evals_on_domain(p_buf, domain_n, length=length, coset=coset)
            assert out.n == domain_n and np.array_equal(out.download(), want), (field, domain_n, length, coset)
            out.free()
    assert np.array_equal(p_buf.download(), x)  # p is left alone ...
    want = co.fft(field, x[:domain_n]) if domain_n == 64 else None
    ctx.poly_evals_on_domain(p_buf, domain_n, length=domain_n, out=p_buf)  # ... unless it is the output
    if want is not None:
        assert np.array_equal(p_buf.download()[:domain_n], want) and np.array_equal(p_buf.download()[domain_n:], x[domain_n:])
    if domain_n == 64:
        short, other = ctx.buf_alloc(field, 63), ctx.buf_alloc(field ^ 1, 64)
        big = ctx.buf_alloc(field, 128)
        for bad, rc in ((lambda: ctx.poly_evals_on_domain(p_buf, 64, length=65, out=big), -1),        # len > domain_n
                        (lambda: ctx.poly_evals_on_domain(p_buf, 128, length=74, out=big), -1),        # len > p's elements
                        (lambda: ctx.poly_evals_on_domain(p_buf, 48, length=8, out=big), -2),          # no domain size
                        (lambda: ctx.poly_evals_on_domain(p_buf, 0, length=0, out=big), -2),
                        (lambda: ctx.poly_evals_on_domain(p_buf, 64, length=8, out=short), -1),        # a short out
                        (lambda: ctx.poly_evals_on_domain(p_buf, 64, length=8, out=other), -1)):       # another field
            with pytest.raises(capi.PcdHipError, match=r"rc=%d\b" % rc):
                bad()
        free(short, other, big)
    p_buf.free()


# ------------------------------------------------------------------------------------------------------------- 6: index_commit
def test_index_commit_matches_kzg_commit(ctx, co):
    from pcd_amd import capi
    curve, field = 0, 1  # MNT4-298 and its scalar field
    rnd = random.Random(1060)
    p = mr.MODULI[field]
    rows, cols, h_n, x_n = 60, 64, 64, 4
    mats = [planted(rnd, p, rows, cols, 250), planted(rnd, p, rows, cols, 140), []]
    idx, refs = build_and_check(ctx, co, field, mats, rows, cols, h_n, x_n)
    powers = ctx.bases_upload(curve, 1, co.gen_points(curve, 1, 256, seed=61))
    comm, inf = idx.commit(powers)
    bufs = [ctx.buf_upload(field, refs[m][q][0]) for m in range(3) for q in range(4)]
    want, want_inf, _, _, _ = ctx.kzg_commit(powers, [{"poly": b} for b in bufs])
    assert np.array_equal(comm, want) and np.array_equal(inf, want_inf)
    assert list(inf) == [0] * 11 + [1] and not comm[11].any()  # C.val of an empty C is the zero polynomial: the identity
    assert len({comm[k].tobytes() for k in range(11)}) == 9     # (C.row = C.col = C.row_col = the constant 1)
    no_coeffs = ctx.marlin_index_build(field, r1cs_of(co, field, mats, rows, cols), h_n, x_n, keep=6)
    with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
        no_coeffs.commit(powers)
    no_coeffs.free()
    free(*bufs)
    powers.free()
    idx.free()


# ---------------------------------------------------------------------------------------------------------- 7: argument errors
def test_index_argument_errors(ctx, co):
    from pcd_amd import capi
    field, p = 1, mr.MODULI[1]
    m = [(0, 0, 1), (1, 2, 5), (3, 6, p - 1), (3, 1, 2), (4, 6, 0)]
    ok = r1cs_of(co, field, [m, m, m[:2]], 5, 7)
    build = ctx.marlin_index_build
    uneven = r1cs_of(co, field, [m, m, m], 5, 7)
    uneven.rp_c = np.concatenate([uneven.rp_c, uneven.rp_c[-1:]])  # C with one row more than A and B
    bad = [
        lambda: build(field, ok, 8, 2, domain_k_n=4),                  # |K| below nnz = 5
        lambda: build(field, ok, 8, 2, domain_k_n=8, domain_b_n=4),    # |B| below |K|
        lambda: build(field, ok, 8, 2, domain_k_n=12),                 # no domain size
        lambda: build(field, ok, 8, 2, domain_b_n=24),
        lambda: build(field, ok, 8, 2, num_cols=6),                    # a column index beyond num_cols
        lambda: build(field, uneven, 8, 2),                            # unequal row counts
        lambda: build(field, ok, 8, 3),                                # |X| does not divide |H| (nor is it a domain size)
        lambda: build(field, ok, 4, 8),
        lambda: build(field, ok, 4, 2),                                # more rows and columns than |H|
        lambda: build(field, ok, 8, 2, keep=8),
    ]
    for f in bad:
        with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
            f()
    idx = build(field, ok, 8, 2, domain_k_n=16, domain_b_n=16)  # a well-formed build afterwards, with the caller's own sizes
    assert (idx.info()["domain_k_n"], idx.info()["domain_b_n"], idx.info()["max_nnz"]) == (16, 16, 5)
    for form, matrix, poly in ((3, 0, 0), (-1, 0, 0), (0, 3, 0), (0, -1, 0), (0, 0, 4), (0, 0, -1)):
        with pytest.raises(capi.PcdHipError, match=r"rc=-1\b"):
            idx.vec(form, matrix, poly)
    dom = domain(co, field, 8)
    row, col, rc, val = mir.arithmetize(m, dom, 8, 2, 16, p)
    for q, want in enumerate((row, col, rc, val)):
        assert np.array_equal(idx.vec(1, 0, q).download(), mont(co, field, want))
    # with |B| = |K| the evaluations on B are the evaluations on K again
    assert np.array_equal(idx.vec(2, 1, 3).download(), idx.vec(1, 1, 3).download())
    idx.free()
    ruled = build(field, ok, 8, 2)
    assert (ruled.info()["domain_k_n"], ruled.info()["domain_b_n"]) == (8, 32)
    ruled.free()


# ------------------------------------------------------------------------------------------- 8: rounds 2 and 3 from the index
@pytest.mark.parametrize("field", [1, 3])
def test_rounds_from_the_index(ctx, co, field):
    """the flow of test_rounds_end_to_end_on_device with the index handle's vectors on K and B; f reaches B through fft and
    poly_evals_on_domain, and no vector is downloaded in between"""
    rnd = random.Random(1080 + field)
    p = mr.MODULI[field]
    h_n, x_n, k_n, b_n = 64, 4, 256, 1024
    dom_h = domain(co, field, h_n)
    rows, cols = 60, 64
    mats = [planted(rnd, p, rows, cols, rnd.randrange(200, 256)) for _ in range(3)]
    alpha, beta = rnd.randrange(p), rnd.randrange(p)
    assert pow(alpha, h_n, p) != 1 and pow(beta, h_n, p) != 1
    eta = [1, rnd.randrange(p), rnd.randrange(p)]
    one = lambda x: mont(co, field, [x])[0]
    r1cs = r1cs_of(co, field, mats, rows, cols)  # the same CSRs for the transposed matrices of t and for the index

    handle = ctx.marlin_mats_upload(field, r1cs, h_n, x_n)
    idx = ctx.marlin_index_build(field, r1cs, h_n, x_n, keep=6)
    assert (idx.info()["domain_k_n"], idx.info()["domain_b_n"]) == (k_n, b_n)
    r_alpha = ctx.domain_bivariate_lagrange(field, h_n, one(alpha))
    t = ctx.marlin_t_evals(handle, mont(co, field, eta), r_alpha)
    ctx.fft(field, t, inverse=True)
    t_beta = mr.to_ints(co, field, ctx.poly_eval([t], one(beta)))[0]
    assert t_beta == mr.horner(mr.interpolate(mr.t_evals(mats, eta, mr.bivariate_lagrange(alpha, dom_h, p), h_n, x_n, p), dom_h, p), beta, p)

    vh = (pow(alpha, h_n, p) - 1) * (pow(beta, h_n, p) - 1) % p
    coeff = mont(co, field, [e * vh % p for e in eta])
    f = ctx.marlin_sumcheck_f(one(alpha), one(beta), coeff, *idx.vecs(1))
    # on B: a and b from the index's vectors as they stand, f through its coefficients
    a_b, b_b = ctx.marlin_sumcheck_ab(one(alpha), one(beta), coeff, *idx.vecs(2))
    f_on_k = ctx.buf_alloc(field, k_n)
    ctx.poly_lincomb([f], mont(co, field, [1]), f_on_k)   # a device copy of f on K, for the sum below
    ctx.fft(field, f, inverse=True)
    f_b = ctx.poly_evals_on_domain(f, b_n, length=k_n)
    bf = ctx.vec_mul(b_b, f_b)
    diff = ctx.buf_alloc(field, b_n)
    assert ctx.poly_lincomb([a_b, bf], mont(co, field, [1, p - 1]), diff) == b_n
    ctx.fft(field, diff, inverse=True)
    h2, ql, rem, rl = ctx.poly_div_vanishing(diff, k_n)
    assert (ql, rl) == (b_n - k_n, k_n)
    # only now does anything come back: sum_K f = t(beta), a zero remainder, and the h_2 identity at a random point
    assert sum(mr.to_ints(co, field, f_on_k.download())) % p == t_beta
    assert not rem.download().any()
    f_coeffs = mr.to_ints(co, field, f.download())
    a_evals, b_evals = mr.to_ints(co, field, a_b.download()), mr.to_ints(co, field, b_b.download())
    dom_b = domain(co, field, b_n)
    z = rnd.randrange(p)
    lag = mr.batch_inverse([(z - w) % p for w in dom_b], p, (pow(z, b_n, p) - 1) * pow(b_n, -1, p) % p)   # L_i(z) / w^i
    at = lambda ev: sum(e * l % p * w for e, l, w in zip(ev, lag, dom_b)) % p
    h2_z = mr.horner(mr.to_ints(co, field, h2.download()), z, p)
    assert h2_z * (pow(z, k_n, p) - 1) % p == (at(a_evals) - at(b_evals) * mr.horner(f_coeffs, z, p)) % p
    assert any(f_coeffs) and any(mr.to_ints(co, field, h2.download()))
    free(r_alpha, t, f, f_on_k, f_b, a_b, b_b, bf, diff, h2, rem)
    idx.free()
    handle.free()
