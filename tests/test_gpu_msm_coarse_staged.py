"""The staged write pass of the MSM partition sort (pcd_amd/csrc/msm.hip.h: msm_coarse_staged_kernel -- a tile's entries ordered by bin in LDS
and written as whole bin runs) at the smallest shapes that can still go wrong: the partition path needs n >= 4 096 and c >= 9.

Every case compares the affine result with the CPU oracle (coracle.msm) on the same inputs, and with the same MSM under the two-pass
counting sort (pcdhip_msm_set_sort 2) and under the partition sort with the direct write pass (pcdhip_msm_set_sort 3, what
PCDHIP_COARSE_TILE=0 selects for a whole process).  Bar: bit-exact affine coordinates (integer arithmetic).  Which write pass a shape takes
is the tile rule's decision; the cases evaluate the rule on the CPU (tests/hostcheck/msm_stage_tile_check.hip) and assert the tile they
were written for, so a change of the rule cannot silently turn a staged case into a second test of the direct pass."""
import numpy as np
import pytest

from test_msm_coarse_staged_host import build_tile_check, run_tile_check

pytestmark = pytest.mark.gpu

SCALAR_BITS = {0: 298, 1: 298, 2: 753, 3: 753}
BIN_SHIFT = 9
NMAX = 5000


@pytest.fixture(scope="module")
def tile_of(tmp_path_factory):
    exe = build_tile_check(tmp_path_factory.mktemp("stage"))

    def f(W, nbins):
        return run_tile_check(exe, [(W, nbins)])[1][(W, nbins)][0]
    return f


@pytest.fixture(scope="module")
def pts298(co):
    return co.gen_points(0, 1, NMAX + 200, seed=901)


def shape_of(ctx, b, cid, n, c_override):
    """(c, W, Wg, nbins) of the MSM msm_run plans for n pairs over the resident vector b"""
    c, W, copies = ctx.bases_info(b, n)
    if copies <= 1 and c_override:
        c = c_override
    assert copies > 1 or not c_override or c == c_override
    W = (SCALAR_BITS[cid] + c) // c
    Wg = -(-W // max(1, copies))
    return c, W, Wg, (Wg << c) >> BIN_SHIFT


def run_case(co, ctx, tile_of, cid, grp, pts, sc, *, pre=-1, c=0, inf=None, offset=0, n=None, tile=None, bins=None, partial=False):
    """`tile`: the staged tile the case is about (0: the direct pass as the fallback); `bins`: the bin count it was written for"""
    n = len(sc) if n is None else n
    want = co.to_affine(cid, grp, co.msm(cid, grp, pts[offset:offset + n], sc[:n], inf=None if inf is None else inf[offset:offset + n], nthreads=8))
    ctx.set_precompute(pre)
    ctx.msm_config(c, 0)
    try:
        b = ctx.bases_upload(cid, grp, pts, inf)
        cc, W, Wg, nbins = shape_of(ctx, b, cid, n, c)
        assert cc >= BIN_SHIFT and 1 <= nbins <= 8192 and n >= 4096, "not a partition-sort shape"
        assert (Wg < W) if partial else True
        if bins is not None:
            assert nbins == bins, (cc, W, Wg, nbins)
        if tile is not None:
            assert tile_of(W, nbins) == tile, (W, nbins, tile_of(W, nbins))
        got = {}
        for mode in (0, 2, 3):
            ctx.msm_set_sort(mode)
            got[mode] = co.to_affine(cid, grp, ctx.msm(b, sc[:n], offset=offset, n=n))
        b.free()
    finally:
        ctx.msm_set_sort(0)
        ctx.msm_config(0, 0)
        ctx.set_precompute(-1)
    for mode in (0, 2, 3):
        assert np.array_equal(want[0], got[mode][0]) and np.array_equal(want[1], got[mode][1]), ("sort mode", mode, "vs oracle")
    return W, nbins


@pytest.mark.parametrize("dist", [0, 1])
@pytest.mark.parametrize("n", [4096, NMAX])
def test_smallest_and_ragged(co, gpu_ctx, tile_of, pts298, n, dist):
    """n = 4 096: whole tiles; n = 5 000: a partial last tile, no multiple of any tile size.  dist 1: zeros and ones are skipped"""
    sc = co.gen_scalars(co.CURVE_FR[0], n, seed=77 + n, dist=dist)
    W, nbins = run_case(co, gpu_ctx, tile_of, 0, 1, pts298[:n], sc)
    assert tile_of(W, nbins) != 0


@pytest.mark.parametrize("pre,c,bins,tile", [(-1, 9, 1, 1024),      # the smallest c, one copy per window: ONE bin, 34 windows
                                             (0, 9, 34, 1024),       # the smallest c without copies: a bin per window
                                             (0, 16, 2432, 1024),    # many bins: runs of min_run entries on average, still staged
                                             (0, 17, 4608, 0)])      # more bins than a useful tile has entries for: the direct pass
def test_window_override(co, gpu_ctx, tile_of, pts298, pre, c, bins, tile):
    sc = co.gen_scalars(co.CURVE_FR[0], 4096, seed=78 + c, dist=0)
    run_case(co, gpu_ctx, tile_of, 0, 1, pts298[:4096], sc, pre=pre, c=c, bins=bins, tile=tile)


@pytest.mark.parametrize("pre,c,bins", [(-1, 9, 1), (-1, 0, None), (0, 0, None)])
def test_all_scalars_equal(co, gpu_ctx, tile_of, pts298, pre, c, bins):
    """every entry of a window falls into one bin; with one bin for all windows (c = 9, a copy per window) the tile's buffer is a single
    run and the rank inside it reaches tile x W"""
    sc = co.gen_scalars(co.CURVE_FR[0], 4096, seed=79, dist=0)
    sc[:] = sc[5]
    W, nbins = run_case(co, gpu_ctx, tile_of, 0, 1, pts298[:4096], sc, pre=pre, c=c, bins=bins)
    assert tile_of(W, nbins) != 0


def test_infinities_and_offset(co, gpu_ctx, tile_of, pts298):
    """a key with points at infinity (the bitmap filters their entries) and an MSM over a sub-range with a non-zero base offset"""
    n = 4096
    rng = np.random.default_rng(5)
    inf = (rng.random(len(pts298)) < 0.3).astype(np.uint8)
    inf[[0, 63, 64, 4095, 4096]] = 1
    sc = co.gen_scalars(co.CURVE_FR[0], n, seed=80, dist=0)
    for pre in (-1, 0):
        W, nbins = run_case(co, gpu_ctx, tile_of, 0, 1, pts298, sc, pre=pre, inf=inf, offset=0, n=n)
        assert tile_of(W, nbins) != 0
        run_case(co, gpu_ctx, tile_of, 0, 1, pts298, sc, pre=pre, inf=inf, offset=137, n=n)
        run_case(co, gpu_ctx, tile_of, 0, 1, pts298, sc, pre=pre, offset=1000, n=n)


@pytest.mark.parametrize("copies", [2, 3])
def test_partial_precompute(co, gpu_ctx, tile_of, pts298, copies):
    """Wg < W: the group g and the bucket window j of an entry differ from its scalar window"""
    sc = co.gen_scalars(co.CURVE_FR[0], NMAX, seed=81 + copies, dist=0)
    W, nbins = run_case(co, gpu_ctx, tile_of, 0, 1, pts298[:NMAX], sc, pre=copies, partial=True)
    assert tile_of(W, nbins) != 0


def test_753_bit_group(co, gpu_ctx, tile_of):
    """24-word scalars, 40-odd windows: the staged kernel at a small tile (the rule leaves 2 048 and 1 024 out: 4 B x 1 024 x W is over the budget)"""
    cid, n = 2, 4096
    pts = co.gen_points(cid, 1, n, seed=902)
    sc = co.gen_scalars(co.CURVE_FR[cid], n, seed=82, dist=0)
    W, nbins = run_case(co, gpu_ctx, tile_of, cid, 1, pts, sc)
    assert W > 36 and tile_of(W, nbins) == 512, (W, nbins, tile_of(W, nbins))
