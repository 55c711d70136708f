"""The staged per-bin sort of the MSM partition sort (pcd_amd/csrc/msm.hip.h: msm_bin_sort_staged_kernel -- a bin of at most `cap` entries
read once, ordered in LDS by the rank its counting atomic returned and written out in whole lines; a larger bin takes the two-read body
inside the same launch) at the smallest shapes of the partition path: n >= 4 096 and c >= 9.

Every case compares the affine result with the CPU oracle (coracle.msm) on the same inputs, and with the same MSM under the two-pass
counting sort (pcdhip_msm_set_sort 2) and under the partition sort with the two-read kernel (pcdhip_msm_set_sort 4, what PCDHIP_BIN_STAGE=0
selects for a whole process).  Bar: bit-exact affine coordinates (integer arithmetic).  Which body a bin takes depends on its load alone;
the cases compute the loads on the CPU (test_msm_bin_staged_host.bin_loads) and assert the situation they were written for, so a change of
the plan cannot silently turn a case about one body into a second test of the other."""
import numpy as np
import pytest

from test_msm_bin_staged_host import bin_loads, bin_stage_constants

pytestmark = pytest.mark.gpu

SCALAR_BITS = {0: 298, 1: 298, 2: 753, 3: 753}
BIN_SHIFT = 9
NMAX = 5000


@pytest.fixture(scope="module")
def cap_default(tmp_path_factory):
    return bin_stage_constants(tmp_path_factory.mktemp("binstage"))["cap"]


@pytest.fixture(scope="module")
def pts298(co):
    return co.gen_points(0, 1, NMAX + 200, seed=911)


def some_staged(loads, cap):
    """at least one non-empty bin takes the staged body at this threshold"""
    return bool(((loads > 0) & (loads <= cap)).any())


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def run_case(co, ctx, cid, grp, pts, sc, *, pre=-1, c=0, inf=None, offset=0, n=None, caps=(-1,), bins=None, partial=False):
    """the MSM under sort modes 0 (once per value of `caps`), 2 and 4 against the oracle; returns the loads of its bins"""
    n = len(sc) if n is None else n
    live = None if inf is None else inf[offset:offset + n] == 0
    want = co.to_affine(cid, grp, co.msm(cid, grp, pts[offset:offset + n], sc[:n], inf=None if inf is None else inf[offset:offset + n], nthreads=8))
    ctx.set_precompute(pre)
    ctx.msm_config(c, 0)
    try:
        b = ctx.bases_upload(cid, grp, pts, inf)
        cc, W, copies = ctx.bases_info(b, n)
        if copies <= 1 and c:
            cc = c
        assert not c or cc == c
        W = (SCALAR_BITS[cid] + cc) // cc
        Wg = -(-W // max(1, copies))
        nbins = (Wg << cc) >> BIN_SHIFT
        assert cc >= BIN_SHIFT and 1 <= nbins <= 8192 and n >= 4096, "not a partition-sort shape"
        assert (Wg < W) if partial else True
        if bins is not None:
            assert nbins == bins, (cc, W, Wg, nbins)
        loads = bin_loads(sc[:n], SCALAR_BITS[cid], cc, Wg, live=live, bin_shift=BIN_SHIFT)
        got = {}
        for cap in caps:
            ctx.msm_set_bin_stage(cap)
            got[("cap", cap)] = co.to_affine(cid, grp, ctx.msm(b, sc[:n], offset=offset, n=n))
        ctx.msm_set_bin_stage(-1)
        for mode in (2, 4):
            ctx.msm_set_sort(mode)
            got[("mode", mode)] = co.to_affine(cid, grp, ctx.msm(b, sc[:n], offset=offset, n=n))
        b.free()
    finally:
        ctx.msm_set_bin_stage(-1)
        ctx.msm_set_sort(0)
        ctx.msm_config(0, 0)
        ctx.set_precompute(-1)
    for k, v in got.items():
        assert same(want, v), (k, "vs oracle")
    return loads


@pytest.mark.parametrize("n", [4096, NMAX])
@pytest.mark.parametrize("c,bins", [(9, 34),       # a bin per window, about n entries each
                                    (16, 2432)])   # about 25 entries a bin, the upper half of every window's bins empty
def test_default_cap_every_bin_staged(co, gpu_ctx, cap_default, pts298, n, c, bins):
    sc = co.gen_scalars(co.CURVE_FR[0], n, seed=171 + n + c, dist=0)
    loads = run_case(co, gpu_ctx, 0, 1, pts298[:n], sc, pre=0, c=c, bins=bins)
    assert 0 < loads.max() <= cap_default
    if c == 16:
        assert (loads == 0).sum() > bins // 3 and (loads > 0).sum() > bins // 3


@pytest.mark.parametrize("n", [4096, NMAX])
def test_default_cap_bin_over_the_compile_time_cap(co, gpu_ctx, cap_default, pts298, n):
    """c = 9 with a copy per window: ONE bin holds every entry, about 34 n of them: the two-read body inside the staged kernel"""
    sc = co.gen_scalars(co.CURVE_FR[0], n, seed=172 + n, dist=0)
    loads = run_case(co, gpu_ctx, 0, 1, pts298[:n], sc, pre=-1, c=9, bins=1)
    assert loads[0] > 130000 > cap_default


@pytest.mark.parametrize("n", [4096, NMAX])
def test_cap_at_a_bins_load_and_one_below(co, gpu_ctx, pts298, n):
    """cap == m: the chosen bin is staged; cap == m - 1: it takes the two-read body; other non-empty bins lie on either side both times, so
    both bodies run in one launch.  cap = 0 is the two-read kernel (mode 4)"""
    sc = co.gen_scalars(co.CURVE_FR[0], n, seed=173 + n, dist=0)
    loads = bin_loads(sc, 298, 9, 34)  # pre = 0, c = 9: 34 windows, a bin each (asserted again by run_case)
    order = np.argsort(loads, kind="stable")
    chosen = int(order[len(order) // 2])
    m = int(loads[chosen])
    others = np.delete(loads, chosen)
    assert m > 1 and ((others > 0) & (others <= m - 1)).any() and (others > m).any(), (m, sorted(loads))
    got = run_case(co, gpu_ctx, 0, 1, pts298[:n], sc, pre=0, c=9, bins=34, caps=(m, m - 1, 0, 1))
    assert np.array_equal(got, loads)


def test_witness_like_scalars(co, gpu_ctx, cap_default, pts298):
    """dist 1: zeros and ones make no entries, the ones go to the pseudo bucket's list behind the sorted one"""
    sc = co.gen_scalars(co.CURVE_FR[0], NMAX, seed=174, dist=1)
    ones = int(((sc[:, 1:] == 0).all(axis=1) & (sc[:, 0] == 1)).sum())
    assert ones > NMAX // 4
    for pre, c in ((-1, 0), (0, 9)):
        loads = run_case(co, gpu_ctx, 0, 1, pts298[:NMAX], sc, pre=pre, c=c)
        assert some_staged(loads, cap_default) and loads.sum() < NMAX * 34 // 3


@pytest.mark.parametrize("pre,c,bins", [(0, 9, 34), (-1, 0, None)])
def test_all_scalars_equal(co, gpu_ctx, cap_default, pts298, pre, c, bins):
    """one key takes a whole window's entries: the rank inside a key reaches the bin's load"""
    n = 4096
    sc = co.gen_scalars(co.CURVE_FR[0], n, seed=175, dist=0)
    sc[:] = sc[5]
    loads = run_case(co, gpu_ctx, 0, 1, pts298[:n], sc, pre=pre, c=c, bins=bins)
    assert set(np.unique(loads).tolist()) <= {n * k for k in range(0, 35)}
    if pre == 0:
        assert loads.max() == n <= cap_default
        # ... and with that bin on the edge of the threshold
        run_case(co, gpu_ctx, 0, 1, pts298[:n], sc, pre=pre, c=c, bins=bins, caps=(n, n - 1))


def test_infinities_and_offset(co, gpu_ctx, cap_default, pts298):
    """a key with 30 % points at infinity (the bitmap filters their entries) and an MSM over a sub-range that starts at base 137"""
    n = 4096
    rng = np.random.default_rng(6)
    inf = (rng.random(len(pts298)) < 0.3).astype(np.uint8)
    inf[[137, 200, 201, 137 + n - 1]] = 1
    sc = co.gen_scalars(co.CURVE_FR[0], n, seed=176, dist=0)
    for pre, c in ((-1, 0), (0, 9)):
        loads = run_case(co, gpu_ctx, 0, 1, pts298, sc, pre=pre, c=c, inf=inf, offset=137, n=n)
        assert some_staged(loads, cap_default)
    m = int(np.sort(loads)[len(loads) // 2])
    run_case(co, gpu_ctx, 0, 1, pts298, sc, pre=0, c=9, inf=inf, offset=137, n=n, caps=(m, m - 1))


def test_partial_precompute(co, gpu_ctx, cap_default, pts298):
    """two copies: Wg < W, two scalar windows share a bucket window and so a bin"""
    sc = co.gen_scalars(co.CURVE_FR[0], NMAX, seed=177, dist=0)
    loads = run_case(co, gpu_ctx, 0, 1, pts298[:NMAX], sc, pre=2, partial=True)
    assert some_staged(loads, cap_default)
    m = int(np.sort(loads[loads > 0])[(loads > 0).sum() // 2])
    run_case(co, gpu_ctx, 0, 1, pts298[:NMAX], sc, pre=2, partial=True, caps=(m, m - 1))


def test_753_bit_group(co, gpu_ctx, cap_default):
    """24-word scalars, 40-odd windows"""
    cid, n = 2, 4096
    pts = co.gen_points(cid, 1, n, seed=912)
    sc = co.gen_scalars(co.CURVE_FR[cid], n, seed=178, dist=0)
    loads = run_case(co, gpu_ctx, cid, 1, pts, sc)
    assert some_staged(loads, cap_default)
    m = int(np.sort(loads[loads > 0])[(loads > 0).sum() // 2])
    run_case(co, gpu_ctx, cid, 1, pts, sc, caps=(m, m - 1))
