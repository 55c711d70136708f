"""The MSM epilogue in XYZZ (pcd_amd/csrc/msm.hip.h, the 298-bit G1 groups): the edge pass sums a run's pieces with EC::add_lz from the
flushed records and leaves the sum as a record in the bucket's slot of the record array, the big-bucket kernel does the same, and the
first reduction level reads every bucket but bucket 1 as a plain record (msm_bucket_lz / msm_bucket_at: no chunk rule) and keeps its
running sums in XYZZ (msm_tail_level_kernel, one lane per item: c = 20; two lanes per item, c = 18, stay Jacobian behind the same reader).
Through the C-ABI, bit-exact against the CPU oracle on the affine image.  The workspace is never cleared, so an MSM over unrelated scalars
with another chunk runs before every checked one: a record read from a slot nobody wrote this time is wrong, not stale-and-right."""
import numpy as np
import pytest

from test_gpu_msm_epilogue import few_valued_scalars

CHUNKS = (33, 100, 128, 0)   # forced, and the device's own choice
LEVEL0 = {"blocks_of_8_one_lane": (20, -1), "blocks_of_8_two_lanes": (18, -1), "pairs": (0, -1), "pairs_horner": (0, 0)}


def scalars_of(co, cid, n, c, kind, seed):
    fr = co.CURVE_FR[cid]
    if kind.startswith("few_"):   # runs over many chunk edges, the big-bucket path; bucket 1 empty / whole / long before the merge
        return few_valued_scalars(co, cid, n, c, seed, kind[4:])
    sc = co.gen_scalars(fr, n, seed=seed, dist=0)
    if kind == "sparse":          # only the two lowest 64-bit words of a few scalars: most buckets of every window stay empty
        sc[:, 1:] = 0
        sc[n // 8:, :] = 0
        sc[n // 8:n // 4, 0] = 1  # and a pseudo bucket
    return sc


def run_case(co, ctx, cid, grp, n, c_forced, precompute, kinds, chunks, seed):
    pts = co.gen_points(cid, grp, n, seed=seed)
    ctx.set_precompute(precompute)
    ctx.msm_config(c_forced, 0)
    b = ctx.bases_upload(cid, grp, pts)
    try:
        c, W, copies = ctx.bases_info(b, n)
        assert (copies > 1) == (precompute != 0) and (c_forced == 0 or c == c_forced), (c, W, copies)
        scrub = co.gen_scalars(co.CURVE_FR[cid], n, seed=seed + 7, dist=0)
        for k, kind in enumerate(kinds):
            sc = scalars_of(co, cid, n, c, kind, seed + 1 + k)
            want = co.to_affine(cid, grp, co.msm(cid, grp, pts, sc, nthreads=8))
            for chunk in (chunks if k % 2 == 0 else chunks[::-1]):
                ctx.msm_config(c_forced, 47 if chunk != 47 else 61)
                ctx.msm(b, scrub)
                ctx.msm_config(c_forced, chunk)
                got = co.to_affine(cid, grp, ctx.msm(b, sc))
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (cid, grp, c, copies, kind, chunk)
    finally:
        ctx.msm_config(0, 0)
        ctx.set_precompute(-1)
        b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("level0", sorted(LEVEL0))
@pytest.mark.parametrize("kinds", [("few_empty", "few_whole", "few_long"), ("uniform", "sparse")], ids=["few_valued", "uniform_sparse"])
def test_g1_298_epilogue_in_xyzz(co, gpu_ctx, cid, level0, kinds):
    c_forced, precompute = LEVEL0[level0]
    run_case(co, gpu_ctx, cid, 1, 5000, c_forced, precompute, kinds, CHUNKS, seed=5100 + 10 * cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,grp", [(0, 2), (2, 1)])
def test_other_groups_keep_their_readers(co, gpu_ctx, cid, grp):
    """MNT4-298 G2 (plain XYZZ records, chunk rule in the first level) and MNT4-753 G1 (Jacobian flush), n = 3 000"""
    run_case(co, gpu_ctx, cid, grp, 3000, 0, -1, ("few_long", "uniform"), (100, 0), seed=5300 + cid)
