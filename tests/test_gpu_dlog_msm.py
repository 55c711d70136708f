"""GPU: the MSM's additions of SUMS at coinciding operands (pcd_amd/csrc/msm.hip.h: the chunk-edge pieces of msm_fixup_kernel, the segment
trees of msm_big_segments_kernel / msm_big_bucket_kernel, msm_merge_ones_kernel, the pair levels msm_tail_pair_item and
msm_tail_level_kernel, msm_horner_kernel) and pcdhip_points_sum[_dev] over equal, opposite and infinite partials.  The bases are k_i G
with known k_i (tests/dlog_reference.py), so partial sums are equal, opposite or the identity on purpose, and the expected result is
(sum s_i k_i mod q) G: integer arithmetic and one fixed-base multiple, no MSM oracle (which agrees: tests/test_dlog_reference_host.py).
Bit-exact on the affine image and the infinity flag."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dlog_reference as dr  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = [(0, 1), (1, 2), (2, 1), (2, 2), (3, 2)]   # lazily reduced XYZZ records; lane-split Fq3; the mailbox G1; Fq2 and Fq3 at 753 bits
FAMILIES = ["small_dlog", "total_cancels", "giant", "ones", "horner"]


def same(got, want_xy, want_inf):
    xy, inf = got
    return bool(inf[0]) == bool(want_inf) and (bool(want_inf) or np.array_equal(xy[0], want_xy))


def run_inputs(co, ctx, cid, grp, inputs, c_forced, precompute, tag, chunks_of=lambda name: (0,)):
    """every input through ctx.msm with the window forced, behind an MSM over unrelated scalars with another chunk (the workspace is never
    cleared between MSMs: whatever a kernel wrongly leaves unwritten is then stale and wrong, as in tests/test_gpu_msm_epilogue.py)"""
    fr = co.CURVE_FR[cid]
    ctx.set_precompute(precompute)
    ctx.msm_config(c_forced, 0)
    try:
        for k, inp in enumerate(inputs):
            n = len(inp.ks)
            xy, inf = dr.dlog_bases(co, cid, grp, inp.ks)
            want_xy, want_inf = dr.expected_msm(co, cid, grp, inp.ks, inp.scalars)
            sc = dr.scalar_words(cid, inp.scalars)
            scrub = co.gen_scalars(fr, n, seed=5200 + k, dist=0)
            ctx.msm_config(c_forced, 0)
            b = ctx.bases_upload(cid, grp, xy, inf)
            try:
                c, W, copies = ctx.bases_info(b, n)
                # (without resident copies the forced window is taken by the MSM itself: bases_info reports the handle's own choice)
                assert (copies > 1) == (precompute != 0) and (copies == 1 or c == c_forced), (c, W, copies)
                for chunk in chunks_of(inp.name):
                    ctx.msm_config(c_forced, 47)
                    ctx.msm(b, scrub)
                    ctx.msm_config(c_forced, chunk)
                    got = co.to_affine(cid, grp, ctx.msm(b, sc))
                    assert same(got, want_xy, want_inf), (cid, grp, inp.name, tag, c, copies, chunk)
            finally:
                b.free()
    finally:
        ctx.msm_config(0, 0)
        ctx.set_precompute(-1)


def family(cid, grp, c, fam):
    out = [i for i in dr.msm_cases(cid, grp, c) if i.name.startswith(fam)]
    assert out
    return out


def chunks_of(name):
    return (33, 128) if name.startswith("giant") else (0,)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("c", [6, 11])
@pytest.mark.parametrize("precompute", [-1, 0], ids=["copies", "horner"])
@pytest.mark.parametrize("cid,grp", GROUPS)
def test_families(co, gpu_ctx, cid, grp, precompute, c, fam):
    run_inputs(co, gpu_ctx, cid, grp, family(cid, grp, c, fam), c, precompute, (precompute, c), chunks_of)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("precompute", [-1, 0], ids=["copies", "horner"])
def test_families_blocks_of_eight(co, gpu_ctx, precompute, fam):
    """c = 18 on MNT4-298 G1: the first reduction level is msm_tail_level_kernel"""
    run_inputs(co, gpu_ctx, 0, 1, family(0, 1, 18, fam), 18, precompute, (precompute, 18), chunks_of)


@pytest.mark.parametrize("fam", FAMILIES)
def test_families_pair_tree_accumulation(co, gpu_ctx, fam):
    """MNT4-753 G1 with the accumulation as a pair tree of affine additions, chunks of 33, from one pair on"""
    gpu_ctx.msm_set_accumulate(2, 33, 1)
    try:
        run_inputs(co, gpu_ctx, 2, 1, family(2, 1, 11, fam), 11, -1, "pair tree", lambda name: (0, 33))
    finally:
        gpu_ctx.msm_set_accumulate(0)


@pytest.mark.parametrize("cid,grp", [(0, 1), (1, 2), (2, 1)])
def test_short_msm_of_small_logarithms(co, gpu_ctx, cid, grp):
    """eight pairs of the small-dlog kind through the bucketless short path (bit-plane sums over the resident copies)"""
    big = dr.small_dlog(cid, 6, 600).input
    at = [i for i, s in enumerate(big.scalars) if s > 1][:6] + [big.scalars.index(1), big.scalars.index(0)]
    ks, scalars = [big.ks[i] for i in at], [big.scalars[i] for i in at]
    xy, inf = dr.dlog_bases(co, cid, grp, ks)
    want_xy, want_inf = dr.expected_msm(co, cid, grp, ks, scalars)
    b = gpu_ctx.bases_upload(cid, grp, xy, inf)
    try:
        got = co.to_affine(cid, grp, gpu_ctx.msm_short(b, dr.scalar_words(cid, scalars)))
        assert same(got, want_xy, want_inf)
        # the same eight bases under scalars that make the total the identity
        q = dr.scalar_modulus(cid)
        sc2 = list(scalars[:7])
        sc2.append(-sum(s * k for s, k in zip(sc2, ks)) * pow(ks[7], -1, q) % q)
        w2 = dr.expected_msm(co, cid, grp, ks, sc2)
        assert w2[1]
        got = co.to_affine(cid, grp, gpu_ctx.msm_short(b, dr.scalar_words(cid, sc2)))
        assert same(got, *w2)
    finally:
        b.free()


def partial_sets(count):
    """logarithms of `count` shard partials: all equal, P next to -P, all infinite, summing to O"""
    alt = [7 if i % 2 == 0 else -7 for i in range(count)]
    to_zero = list(range(1, count)) + [-sum(range(1, count))]
    return {"all_equal": [5] * count, "p_and_minus_p": alt, "all_infinite": [0] * count, "sum_to_zero": to_zero}


@pytest.mark.parametrize("count", [2, 3, 70])
@pytest.mark.parametrize("cid,grp", GROUPS)
def test_points_sum_of_coinciding_partials(co, gpu_ctx, cid, grp, count):
    import torch
    q = dr.scalar_modulus(cid)
    for name, ks in partial_sets(count).items():
        assert name != "sum_to_zero" or sum(ks) == 0
        xy, inf = dr.dlog_bases(co, cid, grp, ks)
        jac = dr.jacobian(co, cid, grp, xy, inf)
        want_xy, want_inf = dr._multiples(co, cid, grp, [sum(ks) % q])
        got = co.to_affine(cid, grp, gpu_ctx.points_sum(cid, grp, jac))
        assert same(got, want_xy[0], want_inf[0]), (name, "host")
        dev = torch.from_numpy(jac.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        got = co.to_affine(cid, grp, gpu_ctx.points_sum_device(cid, grp, dev.data_ptr(), count))
        assert same(got, want_xy[0], want_inf[0]), (name, "device")


@pytest.mark.parametrize("cid,grp", [(0, 1), (1, 2), (2, 1)])
def test_two_shards_with_identical_halves(co, gpu_ctx, cid, grp):
    """the two shards' partial results are the same point: their sum doubles; with the second half's bases negated it is the identity"""
    from pcd_amd import capi
    ndev = capi.lib().pcdhip_device_count()
    half = dr.small_dlog(cid, 11, 600).input
    mctx = capi.Context(devices=[i % ndev for i in range(2)])
    try:
        for name, sign in (("equal", 1), ("opposite", -1)):
            ks = list(half.ks) + [sign * k for k in half.ks]
            scalars = list(half.scalars) * 2
            xy, inf = dr.dlog_bases(co, cid, grp, ks)
            want_xy, want_inf = dr.expected_msm(co, cid, grp, ks, scalars)
            assert bool(want_inf) == (sign == -1)
            b = mctx.bases_upload(cid, grp, xy, inf)
            got = co.to_affine(cid, grp, mctx.msm(b, dr.scalar_words(cid, scalars)))
            b.free()
            assert same(got, want_xy, want_inf), name
    finally:
        mctx.close()
