"""GPU parity of the short MSM (pcdhip_msm_short*: bit-plane sums over the resident copies, no buckets) against the CPU oracle and
against pcdhip_msm on the same handle, through the C ABI.  Bar: bit-exact on affine coordinates (integer arithmetic; the Jacobian
representative may differ)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GROUPS = [(c, g) for c in range(4) for g in (1, 2)]
MODES = (-1, 0, 2, 3)
SIZES = (0, 1, 2, 3, 63, 64, 65, 257, 1024)   # 64: the first size that gets copies; 257: more than one part; 1024: the cap
CAP = 1024

_CASE = {}


def case(co, cid, grp):
    """1025 seeded points and scalars per group and the oracle's results over their prefixes, computed once and left unchanged"""
    key = (cid, grp)
    if key not in _CASE:
        fr = co.CURVE_FR[cid]
        pts = co.gen_points(cid, grp, CAP + 1, seed=900 + 2 * cid + grp)
        sc = co.gen_scalars(fr, CAP + 1, seed=950 + 2 * cid + grp)
        pts.setflags(write=False)
        sc.setflags(write=False)
        _CASE[key] = (pts, sc, {})
    return _CASE[key]


def oracle(co, cid, grp, pts, sc, inf=None):
    return co.to_affine(cid, grp, co.msm(cid, grp, pts, sc, inf=inf, nthreads=8))


def same(a, b):
    return bool(a[1][0] == b[1][0] and np.array_equal(a[0], b[0]))


def r_minus_1(co, fr):
    L = co.FIELD_N64[fr]
    one = np.array([[1] + [0] * (L - 1)], dtype=np.uint64)
    return co.fp_op(fr, "to_canonical", co.fp_op(fr, "neg", co.fp_op(fr, "from_canonical", one)))[0]


def limbs(v, L):
    return np.array([(v >> (64 * i)) & (2**64 - 1) for i in range(L)], dtype=np.uint64)


def span_of(ctx, b, bits):
    c, W, copies = ctx.bases_info(b)
    return c * ((W + copies - 1) // copies) if copies > 1 else bits


def negated(co, cid, grp, p):
    q = p.copy()
    L = co.FIELD_N64[co.CURVE_FQ[cid]]
    half = len(p) // 2
    q[half:] = co.fp_op(co.CURVE_FQ[cid], "neg", p[half:].reshape(-1, L)).reshape(-1)
    return q


def both_paths(co, ctx, cid, grp, b, sc, want, offset=0, n=None, tag=None):
    n = len(sc) if n is None else n
    short = ctx.msm_short(b, sc[:n], offset=offset, n=n)
    got = co.to_affine(cid, grp, short)
    assert same(got, want), ("short vs oracle", cid, grp, n, offset, tag)
    if got[1][0]:
        assert not short[2 * len(short) // 3:].any(), "the identity comes back with Z = 0"
    old = co.to_affine(cid, grp, ctx.msm(b, sc[:n], offset=offset, n=n))
    assert same(got, old), ("short vs pcdhip_msm", cid, grp, n, offset, tag)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cid,grp", GROUPS)
def test_sizes_under_every_layout(co, gpu_ctx, cid, grp, mode):
    pts, sc, wants = case(co, cid, grp)
    gpu_ctx.set_precompute(mode)
    try:
        for n in SIZES:
            if n not in wants:
                wants[n] = oracle(co, cid, grp, pts[:n], sc[:n]) if n else None
            b = gpu_ctx.bases_upload(cid, grp, pts[:max(n, 1)])
            if n == 0:
                out = gpu_ctx.msm_short(b, sc[:0], n=0)
                assert co.to_affine(cid, grp, out)[1][0] == 1 and not out[2 * len(out) // 3:].any()
            else:
                both_paths(co, gpu_ctx, cid, grp, b, sc, wants[n], n=n, tag=mode)
            b.free()
    finally:
        gpu_ctx.set_precompute(-1)


@pytest.mark.parametrize("cid,grp", GROUPS)
def test_offsets_into_a_longer_vector(co, gpu_ctx, cid, grp):
    """the stride between copies is the VECTOR's length, not the range's"""
    pts, sc, _ = case(co, cid, grp)
    N, n = 200, 40
    try:
        for mode in (-1, 0, 2):
            gpu_ctx.set_precompute(mode)
            b = gpu_ctx.bases_upload(cid, grp, pts[:N])
            for off in (0, 1, 137):
                both_paths(co, gpu_ctx, cid, grp, b, sc, oracle(co, cid, grp, pts[off:off + n], sc[:n]), offset=off, n=n, tag=mode)
            b.free()
    finally:
        gpu_ctx.set_precompute(-1)


@pytest.mark.parametrize("cid,grp", GROUPS)
def test_special_scalars(co, gpu_ctx, cid, grp):
    """0, 1, r - 1, one bit at span - 1, span, span + 1 (the seam between two copies) and at the top; all zero; witness-like"""
    fr = co.CURVE_FR[cid]
    L = co.FIELD_N64[fr]
    pts, sc0, _ = case(co, cid, grp)
    n = 70
    rm1 = r_minus_1(co, fr)
    top = int.from_bytes(rm1.tobytes(), "little").bit_length() - 1   # 2^top < r
    try:
        for mode in MODES:
            gpu_ctx.set_precompute(mode)
            b = gpu_ctx.bases_upload(cid, grp, pts[:n])
            span = span_of(gpu_ctx, b, top + 1)
            sc = sc0[:n].copy()
            sc[0] = 0
            sc[1] = 0; sc[1, 0] = 1
            sc[2] = rm1
            for k, pos in enumerate(p for p in (span - 1, span, span + 1, top) if p <= top):
                sc[3 + k] = limbs(1 << pos, L)
            both_paths(co, gpu_ctx, cid, grp, b, sc, oracle(co, cid, grp, pts[:n], sc), tag=("special", mode))
            one_bit = np.zeros_like(sc)
            one_bit[5] = limbs(1 << min(span, top), L)
            both_paths(co, gpu_ctx, cid, grp, b, one_bit, oracle(co, cid, grp, pts[:n], one_bit), tag=("one bit", mode))
            zero = np.zeros_like(sc)
            out = gpu_ctx.msm_short(b, zero)
            assert co.to_affine(cid, grp, out)[1][0] == 1 and not out[2 * len(out) // 3:].any(), ("all zero", mode)
            wl = co.gen_scalars(fr, n, seed=77 + cid, dist=1)
            both_paths(co, gpu_ctx, cid, grp, b, wl, oracle(co, cid, grp, pts[:n], wl), tag=("witness-like", mode))
            b.free()
    finally:
        gpu_ctx.set_precompute(-1)


@pytest.mark.parametrize("cid,grp", GROUPS)
def test_special_bases(co, gpu_ctx, cid, grp):
    """flagged infinities under non-zero scalars, one point at two and at 70 indices (P + P in a lane's sum and in the tree), and P next
    to -P under equal scalars: the identity, Z = 0"""
    pts0, sc0, _ = case(co, cid, grp)
    n = 80
    pts = pts0[:n].copy()
    sc = sc0[:n].copy()
    pts[3] = pts[2]
    pts[8:78] = pts[8]
    sc[3] = sc[2]             # same point, same scalar: every set bit meets its own double
    sc[8:40] = sc[8]
    inf = np.zeros(n, dtype=np.uint8)
    inf[[0, 5, 79]] = 1
    pair = np.stack([pts0[100], negated(co, cid, grp, pts0[100])])
    assert co.on_curve(cid, grp, pair[1])
    pair_sc = np.stack([sc0[100], sc0[100]])
    try:
        for mode in (-1, 0, 2):
            gpu_ctx.set_precompute(mode)
            b = gpu_ctx.bases_upload(cid, grp, pts, inf)
            both_paths(co, gpu_ctx, cid, grp, b, sc, oracle(co, cid, grp, pts, sc, inf=inf), tag=("bases", mode))
            b.free()
            b = gpu_ctx.bases_upload(cid, grp, pair)
            out = gpu_ctx.msm_short(b, pair_sc)
            assert co.to_affine(cid, grp, out)[1][0] == 1 and not out[2 * len(out) // 3:].any(), ("P - P", mode)
            b.free()
        # 70 opposite pairs over a handle with copies
        gpu_ctx.set_precompute(-1)
        many = np.concatenate([np.repeat(pair[:1], 35, axis=0), np.repeat(pair[1:], 35, axis=0)])
        b = gpu_ctx.bases_upload(cid, grp, many)
        out = gpu_ctx.msm_short(b, np.repeat(pair_sc[:1], 70, axis=0))
        assert co.to_affine(cid, grp, out)[1][0] == 1 and not out[2 * len(out) // 3:].any()
        b.free()
    finally:
        gpu_ctx.set_precompute(-1)


@pytest.mark.parametrize("cid,grp", GROUPS)
def test_device_scalars_and_errors(co, gpu_ctx, cid, grp):
    from pcd_amd import capi
    lib = capi.lib()
    ctx = gpu_ctx
    fr = co.CURVE_FR[cid]
    pts, sc, _ = case(co, cid, grp)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    sz = C.c_size_t
    b = ctx.bases_upload(cid, grp, pts)                 # 1025 points
    out = np.zeros(3 * pts.shape[1] // 2, dtype=np.uint64)
    scc = np.ascontiguousarray(sc)
    # the device-scalar form, scalars from element 9 on, bases from point 21 on
    sb = ctx.buf_upload(fr, scc)
    n, so, off = 33, 9, 21
    got = co.to_affine(cid, grp, ctx.msm_short(b, sb, offset=off, n=n, scalar_offset=so))
    assert same(got, oracle(co, cid, grp, pts[off:off + n], sc[so:so + n]))
    assert same(got, co.to_affine(cid, grp, ctx.msm(b, scc[so:so + n], offset=off, n=n)))
    # the cap
    assert lib.pcdhip_msm_short(ctx._ctx, b._h, sz(0), P(scc), sz(CAP + 1), P(out)) == -2
    assert lib.pcdhip_msm_short_dev(ctx._ctx, b._h, sz(0), sb._h, sz(0), sz(CAP + 1), P(out)) == -2
    # ranges, null pointers, the wrong field
    assert lib.pcdhip_msm_short(ctx._ctx, b._h, sz(CAP), P(scc), sz(2), P(out)) == -1
    assert lib.pcdhip_msm_short(ctx._ctx, b._h, sz(0), None, sz(8), P(out)) == -1
    assert lib.pcdhip_msm_short(ctx._ctx, b._h, sz(0), P(scc), sz(8), None) == -1
    assert lib.pcdhip_msm_short(ctx._ctx, None, sz(0), P(scc), sz(8), P(out)) == -1
    assert lib.pcdhip_msm_short_dev(ctx._ctx, b._h, sz(0), sb._h, sz(CAP), sz(2), P(out)) == -1
    assert lib.pcdhip_msm_short_dev(ctx._ctx, b._h, sz(0), None, sz(0), sz(2), P(out)) == -1
    wrong = ctx.buf_upload(co.CURVE_FQ[cid], np.ascontiguousarray(sc[:8]))
    assert lib.pcdhip_msm_short_dev(ctx._ctx, b._h, sz(0), wrong._h, sz(0), sz(8), P(out)) == -1
    assert lib.pcdhip_msm_set_short(ctx._ctx, sz(CAP + 1)) == -1
    # an unreduced scalar: a bit above the scalar field's bit length, also under a base that is the point at infinity
    bad = scc[:64].copy()
    bad[3, -1] = 1 << 60
    assert lib.pcdhip_msm_short(ctx._ctx, b._h, sz(0), P(bad), sz(64), P(out)) == -1
    # the rule's boundary: the top bit below r's bit length is a legal scalar, a bit AT the bit length is not
    rm1 = r_minus_1(co, fr)
    bits = int.from_bytes(rm1.tobytes(), "little").bit_length()
    L = sc.shape[1]
    edge = scc[:64].copy()
    edge[7] = limbs(1 << (bits - 1), L)
    assert same(co.to_affine(cid, grp, ctx.msm_short(b, edge)), oracle(co, cid, grp, pts[:64], edge))
    edge[7] = limbs(1 << bits, L)
    assert lib.pcdhip_msm_short(ctx._ctx, b._h, sz(0), P(edge), sz(64), P(out)) == -1
    assert lib.pcdhip_msm(ctx._ctx, b._h, sz(0), P(edge), sz(64), P(out)) == -1      # (the rule of pcdhip_msm, matched exactly)
    bb = ctx.buf_upload(fr, bad)
    assert lib.pcdhip_msm_short_dev(ctx._ctx, b._h, sz(0), bb._h, sz(0), sz(64), P(out)) == -1
    with pytest.raises(capi.PcdHipError, match="rc=-1"):
        ctx.msm_short(b, bad)
    inf = np.zeros(64, dtype=np.uint8)
    inf[3] = 1
    bi = ctx.bases_upload(cid, grp, pts[:64], inf)
    assert lib.pcdhip_msm_short(ctx._ctx, bi._h, sz(0), P(bad), sz(64), P(out)) == -1
    # ... and the next call is clean again
    assert same(co.to_affine(cid, grp, ctx.msm_short(bi, scc[:64])), oracle(co, cid, grp, pts[:64], sc[:64], inf=inf))
    for h in (b, bi, sb, bb, wrong):
        h.free()


def test_sharded_handles_are_refused(co, gpu_ctx):
    from pcd_amd import capi
    pts, sc, _ = case(co, 0, 1)
    ndev = capi.lib().pcdhip_device_count()
    mctx = capi.Context(devices=[i % ndev for i in range(2)])   # (on one GPU: two logical shards on the same device)
    try:
        b = mctx.bases_upload(0, 1, pts[:100])
        with pytest.raises(capi.PcdHipError, match="rc=-1"):
            mctx.msm_short(b, np.ascontiguousarray(sc[:100]))
        b.free()
    finally:
        mctx.close()
