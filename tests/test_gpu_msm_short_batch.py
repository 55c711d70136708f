"""GPU parity of the batched short MSM (pcdhip_msm_short_batch / _dev: k independent short MSMs over one handle as one chain of two or
three launches) through the C ABI.  Bar: bit-exact affine equality with the CPU oracle AND with k calls of pcdhip_msm_short on the same
handle (integer arithmetic; the Jacobian representative may differ)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GROUPS = [(c, g) for c in range(4) for g in (1, 2)]
NPTS = 300
CAP = 1024
# (base_offset, scalar_offset, n).  85: two parts for the 21-item groups without copies; 257: two parts for the 64-item ones; every n >= 6
# is several parts under copies.  Base offsets 0, 1, 137; the 85- and the 257-pair items overlap; the two-pair item comes twice; the empty
# item sits in the middle.
MIXED = [(0, 5, 1), (1, 0, 2), (137, 9, 0), (137, 20, 85), (1, 30, 257), (0, 7, 3), (1, 0, 2)]

_CASE = {}


def case(co, cid, grp):
    """300 seeded points and scalars per group and the oracle's results per item, computed once and left unchanged"""
    key = (cid, grp)
    if key not in _CASE:
        pts = co.gen_points(cid, grp, NPTS, seed=1300 + 2 * cid + grp)
        sc = co.gen_scalars(co.CURVE_FR[cid], NPTS, seed=1350 + 2 * cid + grp)
        pts.setflags(write=False)
        sc.setflags(write=False)
        _CASE[key] = (pts, sc, {})
    return _CASE[key]


def oracle(co, cid, grp, pts, sc, inf=None):
    return co.to_affine(cid, grp, co.msm(cid, grp, pts, sc, inf=inf, nthreads=8))


def want_of(co, cid, grp, item):
    pts, sc, wants = case(co, cid, grp)
    if item not in wants:
        bo, so, n = item
        wants[item] = oracle(co, cid, grp, pts[bo:bo + n], sc[so:so + n]) if n else None
    return wants[item]


def same(a, b):
    return bool(a[1][0] == b[1][0] and np.array_equal(a[0], b[0]))


def is_identity(co, cid, grp, jac):
    return co.to_affine(cid, grp, jac)[1][0] == 1 and not jac[2 * len(jac) // 3:].any()


def limbs(v, L):
    return np.array([(v >> (64 * i)) & (2**64 - 1) for i in range(L)], dtype=np.uint64)


def r_bits(co, fr):
    L = co.FIELD_N64[fr]
    one = np.array([[1] + [0] * (L - 1)], dtype=np.uint64)
    rm1 = co.fp_op(fr, "to_canonical", co.fp_op(fr, "neg", co.fp_op(fr, "from_canonical", one)))[0]
    return int.from_bytes(rm1.tobytes(), "little").bit_length()


def negated(co, cid, grp, p):
    q = p.copy()
    L = co.FIELD_N64[co.CURVE_FQ[cid]]
    half = len(p) // 2
    q[half:] = co.fp_op(co.CURVE_FQ[cid], "neg", p[half:].reshape(-1, L)).reshape(-1)
    return q


def check_batch(co, ctx, cid, grp, b, sc, items, wants, tag, singles=True):
    """the batch against the oracle's per-item results (None: the identity) and against pcdhip_msm_short item by item"""
    out = ctx.msm_short_batch(b, sc, items)
    assert out.shape[0] == len(items)
    single_of = {}
    for j, (item, want) in enumerate(zip(items, wants)):
        bo, so, n = item
        if want is None or want[1][0]:
            assert is_identity(co, cid, grp, out[j]), ("the identity comes back with Z = 0", tag, j, item)
        got = co.to_affine(cid, grp, out[j])
        if want is not None:
            assert same(got, want), ("batch vs oracle", tag, j, item)
        if singles and n:
            if item not in single_of:
                single_of[item] = co.to_affine(cid, grp, ctx.msm_short(b, np.ascontiguousarray(sc[so:so + n]), offset=bo, n=n))
            assert same(got, single_of[item]), ("batch vs pcdhip_msm_short", tag, j, item)
    return out


@pytest.mark.parametrize("mode", (-1, 0, 2))
@pytest.mark.parametrize("cid,grp", GROUPS)
def test_mixed_batch(co, gpu_ctx, cid, grp, mode):
    pts, sc, _ = case(co, cid, grp)
    wants = [want_of(co, cid, grp, it) for it in MIXED]
    gpu_ctx.set_precompute(mode)
    try:
        b = gpu_ctx.bases_upload(cid, grp, pts)
        check_batch(co, gpu_ctx, cid, grp, b, np.ascontiguousarray(sc), MIXED, wants, mode)
        # the same through resident scalars
        sb = gpu_ctx.buf_upload(co.CURVE_FR[cid], np.ascontiguousarray(sc))
        out = gpu_ctx.msm_short_batch(b, sb, MIXED)
        for j, w in enumerate(wants):
            if w is None:
                assert is_identity(co, cid, grp, out[j])
            else:
                assert same(co.to_affine(cid, grp, out[j]), w), ("device scalars", mode, j)
        sb.free()
        b.free()
    finally:
        gpu_ctx.set_precompute(-1)


@pytest.mark.parametrize("npts", (4, 64))
@pytest.mark.parametrize("cid,grp", GROUPS)
def test_commit_shape(co, gpu_ctx, cid, grp, npts):
    """k = 70 MSMs of two pairs -- more than the items of a wave, more than 64 -- over a 4-point handle (no copies: the chain is the scalar's
    bits) and a 64-point one (the smallest upload that gets copies); six distinct (base, scalar) positions among them.  And k = 1."""
    pts, sc, _ = case(co, cid, grp)
    distinct = [(0, 0, 2), (1, 3, 2), (2, 8, 2), (0, 21, 2), (2, 0, 2), (1, 40, 2)]
    items = [distinct[(5 * j + j // 6) % 6] for j in range(70)]
    wants = [want_of(co, cid, grp, it) for it in items]
    b = gpu_ctx.bases_upload(cid, grp, pts[:npts])
    scc = np.ascontiguousarray(sc[:64])
    check_batch(co, gpu_ctx, cid, grp, b, scc, items, wants, npts)
    check_batch(co, gpu_ctx, cid, grp, b, scc, items[3:4], wants[3:4], (npts, "k = 1"))
    b.free()


@pytest.mark.parametrize("mode", (-1, 0))
@pytest.mark.parametrize("cid,grp", GROUPS)
def test_degenerate_items_between_ordinary_ones(co, gpu_ctx, cid, grp, mode):
    """P next to -P under equal scalars, all-zero scalars, a flagged identity base under a non-zero scalar, one point twice under one
    scalar: each between ordinary items, on a 70-point handle (copies under mode -1)"""
    pts0, sc0, _ = case(co, cid, grp)
    pts, sc = pts0[:70].copy(), np.concatenate([sc0[:70], np.zeros((2, sc0.shape[1]), dtype=np.uint64)])
    pts[3] = negated(co, cid, grp, pts[2])
    assert co.on_curve(cid, grp, pts[3])
    sc[3] = sc[2]
    pts[6] = pts[5]
    sc[6] = sc[5]
    inf = np.zeros(70, dtype=np.uint8)
    inf[8] = 1
    items = [(0, 0, 2), (2, 2, 2), (4, 4, 1), (9, 70, 2), (9, 9, 3), (8, 8, 1), (7, 7, 3), (5, 5, 2), (10, 10, 60)]
    wants = [oracle(co, cid, grp, pts[bo:bo + n], sc[so:so + n], inf=inf[bo:bo + n]) for bo, so, n in items]
    assert [int(w[1][0]) for w in wants] == [0, 1, 0, 1, 0, 1, 0, 0, 0]
    gpu_ctx.set_precompute(mode)
    try:
        b = gpu_ctx.bases_upload(cid, grp, pts, inf)
        check_batch(co, gpu_ctx, cid, grp, b, np.ascontiguousarray(sc), items, wants, mode)
        b.free()
    finally:
        gpu_ctx.set_precompute(-1)


@pytest.mark.parametrize("cid,grp", GROUPS)
def test_back_to_back_calls_reuse_the_workspace(co, gpu_ctx, cid, grp):
    """a large call, a small one, the large one again: the workspace and the table are reused through stream order"""
    pts, sc, _ = case(co, cid, grp)
    b = gpu_ctx.bases_upload(cid, grp, pts)
    scc = np.ascontiguousarray(sc)
    first, second = [MIXED[4], MIXED[3], MIXED[1]], [MIXED[5], MIXED[0]]
    for k, items in enumerate((first, second, first)):
        check_batch(co, gpu_ctx, cid, grp, b, scc, items, [want_of(co, cid, grp, it) for it in items], ("call", k), singles=False)
    b.free()


@pytest.mark.parametrize("cid,grp", GROUPS)
def test_errors(co, gpu_ctx, cid, grp):
    from pcd_amd import capi
    lib = capi.lib()
    ctx = gpu_ctx
    fr = co.CURVE_FR[cid]
    pts, sc, _ = case(co, cid, grp)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    sz = C.c_size_t
    b = ctx.bases_upload(cid, grp, pts)          # 300 points
    scc = np.ascontiguousarray(sc)               # 300 scalars
    sb = ctx.buf_upload(fr, scc)
    out = np.zeros((CAP + 1, 3 * pts.shape[1] // 2), dtype=np.uint64)

    def arr(items):
        a = (capi.MsmShortItem * max(len(items), 1))()
        for e, (bo, so, n) in zip(a, items):
            e.base_offset, e.scalar_offset, e.n = bo, so, n
        return a

    def host(items, scal=scc, bases=b, k=None, outp=out):
        return lib.pcdhip_msm_short_batch(ctx._ctx, bases._h if bases is not None else None, None if scal is None else P(scal),
                                          sz(0 if scal is None else len(scal)), arr(items) if items is not None else None,
                                          sz(len(items) if k is None else k), None if outp is None else P(outp))

    def dev(items, buf=sb, bases=b, k=None, outp=out):
        return lib.pcdhip_msm_short_batch_dev(ctx._ctx, bases._h if bases is not None else None, buf._h if buf is not None else None,
                                              arr(items) if items is not None else None, sz(len(items) if k is None else k),
                                              None if outp is None else P(outp))

    ok = [(0, 0, 2), (5, 7, 3)]
    assert host(ok) == 0 and dev(ok) == 0
    # k = 0 succeeds without a launch, also with nothing else to look at
    assert host([]) == 0 and dev([]) == 0
    assert host(None, k=0, outp=None) == 0 and dev(None, k=0, outp=None) == 0
    assert ctx.msm_short_batch(b, scc, []).shape == (0, out.shape[1])
    # the caps: k, and an item's n (before its range is looked at: the handle has 300 points)
    assert host([(0, 0, 1)] * (CAP + 1)) == -2 and dev([(0, 0, 1)] * (CAP + 1)) == -2
    assert host([(0, 0, 1)] * CAP) == 0
    assert host(ok + [(0, 0, CAP + 1)]) == -2 and dev(ok + [(0, 0, CAP + 1)]) == -2
    # ranges beyond the handle or the scalars
    for bad in ([(299, 0, 2)], [(301, 0, 0)], [(0, 299, 2)], [(0, 301, 0)], ok + [(298, 0, 3)], [(1 << 63, 0, 2)], [(0, 1 << 63, 2)]):
        assert host(bad) == -1 and dev(bad) == -1, bad
    assert host([(0, 0, 2)], scal=scc[:1]) == -1
    # null pointers
    assert host(ok, scal=None) == -1 and host(None, k=2) == -1 and host(ok, outp=None) == -1 and host(ok, bases=None) == -1
    assert dev(ok, buf=None) == -1 and dev(None, k=2) == -1 and dev(ok, outp=None) == -1 and dev(ok, bases=None) == -1
    # the wrong field
    wrong = ctx.buf_upload(co.CURVE_FQ[cid], np.ascontiguousarray(sc[:8]))
    assert dev(ok, buf=wrong) == -1
    # an unreduced scalar in the LAST item: one bit at the scalar field's bit length; the call fails as a whole, the next one is clean
    bits = r_bits(co, fr)
    L = sc.shape[1]
    items = [(0, 0, 2), (1, 30, 257), (0, 0, 0), (20, 290, 3)]
    edge = scc.copy()
    edge[291] = limbs(1 << (bits - 1), L)          # the top bit below the bit length is a legal scalar
    assert host(items, scal=edge) == 0
    edge[291] = limbs(1 << bits, L)
    assert host(items, scal=edge) == -1
    eb = ctx.buf_upload(fr, edge)
    assert dev(items, buf=eb) == -1
    with pytest.raises(capi.PcdHipError, match="rc=-1"):
        ctx.msm_short_batch(b, edge, items)
    assert host(items[:3], scal=edge) == 0        # (the item that reads it is what fails)
    check_batch(co, ctx, cid, grp, b, scc, ok, [want_of(co, cid, grp, it) for it in ok], "clean after the error", singles=False)
    # ... once under a flagged identity base
    inf = np.zeros(NPTS, dtype=np.uint8)
    inf[21] = 1
    bi = ctx.bases_upload(cid, grp, pts, inf)
    assert host(items, scal=edge, bases=bi) == -1
    got = ctx.msm_short_batch(bi, scc, items)
    assert same(co.to_affine(cid, grp, got[3]), oracle(co, cid, grp, pts[20:23], sc[290:293], inf=inf[20:23]))
    for h in (b, bi, sb, eb, wrong):
        h.free()


def test_sharded_handles_are_refused(co, gpu_ctx):
    from pcd_amd import capi
    pts, sc, _ = case(co, 0, 1)
    ndev = capi.lib().pcdhip_device_count()
    mctx = capi.Context(devices=[i % ndev for i in range(2)])   # (on one GPU: two logical shards on the same device)
    try:
        b = mctx.bases_upload(0, 1, pts[:100])
        with pytest.raises(capi.PcdHipError, match="rc=-1"):
            mctx.msm_short_batch(b, np.ascontiguousarray(sc[:100]), [(0, 0, 2)])
        b.free()
    finally:
        mctx.close()
