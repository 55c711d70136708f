"""The epilogue of the MSM accumulation (pcd_amd/csrc/msm.hip.h): chunks of up to 128 entries, the fix-up pass over chunk EDGES
(msm_fixup_kernel: one item per edge; whole buckets stay where the accumulation flushed them, nobody writes empty ones) and the first
bucket-reduction level that takes every bucket from where it lies (msm_bucket_at in msm_tail_level_kernel / msm_tail_pair_first_kernel).
GPU tests through the C-ABI, bit-exact against the CPU oracle on the affine image; the chunk rule itself is checked on the host."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR_BITS = [298, 298, 753, 753]
LANES_MI355X_G1 = 256 * 4 * 2 * 64   # resident accumulate lanes of the 298-bit G1 on 256 compute units: two waves on each of 1024 SIMDs


def limbs(values, L):
    out = np.zeros((len(values), L), dtype=np.uint64)
    for i, v in enumerate(values):
        for k in range(L):
            out[i, k] = (v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


def few_valued_scalars(co, cid, n, c, seed, bucket1):
    """n scalars over 40 distinct values, one of them a third of the vector: bucket runs hundreds of entries long that cross many chunk
    edges, the longest over more than eight chunks of 128 (the big-bucket path).  Every c-bit window of a value lies in
    [2, 2^(c-1) - 1], so the signed digits are the windows themselves and NONE is 1: bucket (window 0, digit 1) is empty before the
    pseudo bucket of the 200 scalars equal to one is merged into it (`bucket1` = "empty").  "whole": three more scalars with digit 1 in
    windows 0 and 1 -- a short run, inside one chunk unless an edge happens to cut it; "long": 300 of them -- a run over several
    chunks.  200 zeros as well."""
    rng = np.random.default_rng(seed)
    L = co.FIELD_N64[co.CURVE_FR[cid]]
    windows = (SCALAR_BITS[cid] - 2) // c   # value < 2^(bits - 2) < r
    assert windows >= 2

    def value(force_one=False):
        d = [int(rng.integers(2, 1 << (c - 1))) for _ in range(windows)]
        if force_one:
            d[0] = d[1] = 1
        return sum(x << (c * w) for w, x in enumerate(d))

    vals = [value() for _ in range(40)]
    assert len(set(vals)) == 40
    weights = np.ones(40)
    weights[0] = 20.0                       # about a third of the draws
    pick = rng.choice(40, size=n, p=weights / weights.sum())
    ints = [vals[k] for k in pick]
    where = rng.permutation(n)
    for i in where[:200]:
        ints[i] = 1
    for i in where[200:400]:
        ints[i] = 0
    extra = {"empty": 0, "whole": 3, "long": 300}[bucket1]
    one_digit = value(force_one=True)
    for i in where[400:400 + extra]:
        ints[i] = one_digit
    return limbs(ints, L)


def run_case(co, ctx, cid, grp, n, c_forced, precompute, chunks, bucket1_cases, seed):
    pts = co.gen_points(cid, grp, n, seed=seed)
    ctx.set_precompute(precompute)
    ctx.msm_config(c_forced, 0)
    b = ctx.bases_upload(cid, grp, pts)
    try:
        c, W, copies = ctx.bases_info(b, n)
        assert (copies > 1) == (precompute != 0) and (c_forced == 0 or c == c_forced), (c, W, copies)
        # The workspace is never cleared between MSMs: without the scrub below a bucket read from the wrong array, or an identity nobody
        # wrote, would find the right value the previous case left there.  An MSM over unrelated uniform scalars with another chunk runs
        # before every checked one, so whatever is stale is wrong.
        scrub = co.gen_scalars(co.CURVE_FR[cid], n, seed=seed + 7, dist=0)
        for k, bucket1 in enumerate(bucket1_cases):
            sc = few_valued_scalars(co, cid, n, c, seed + 1, bucket1)
            want = co.to_affine(cid, grp, co.msm(cid, grp, pts, sc, nthreads=8))   # once per input, whatever the chunk
            for chunk in (chunks if k % 2 == 0 else chunks[::-1]):                 # (longest chunk first in every other case)
                ctx.msm_config(c_forced, 47)
                ctx.msm(b, scrub)
                ctx.msm_config(c_forced, chunk)
                got = co.to_affine(cid, grp, ctx.msm(b, sc))
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (cid, grp, c, copies, bucket1, chunk)
    finally:
        ctx.msm_config(0, 0)
        ctx.set_precompute(-1)
        b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("cid,grp", [(0, 1), (1, 2)])
@pytest.mark.parametrize("level0", ["blocks_of_8", "pairs", "pairs_horner"])
def test_long_and_odd_forced_chunks(co, gpu_ctx, cid, grp, level0):
    """MNT4-298 G1 (lazily reduced XYZZ records, converted as they are read) and the lane-split MNT6-298 G2, n = 5 000, forced chunks
    33, 100 and 128 on lists whose runs cross many chunk edges.  c = 18: the first reduction level is msm_tail_level_kernel (k = 3);
    the default small window: the pair kernel, with one bucket window (resident copies) and with several (no copies, Horner combine).
    Bucket 1 empty, whole and long before the pseudo bucket is merged into it."""
    c_forced, precompute = {"blocks_of_8": (18, -1), "pairs": (0, -1), "pairs_horner": (0, 0)}[level0]
    run_case(co, gpu_ctx, cid, grp, 5000, c_forced, precompute, (33, 100, 128), ("empty", "whole", "long"), seed=4100 + 10 * cid + grp)


@pytest.mark.gpu
def test_753_bit_g1_forced_chunk_100(co, gpu_ctx):
    """the mailbox tail and a Jacobian flush (the flushed buckets ARE the bucket array): MNT4-753 G1, n = 3 000, chunk 100"""
    run_case(co, gpu_ctx, 2, 1, 3000, 0, -1, (100,), ("empty", "whole"), seed=4200)


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "msm_plan_check")
    src = os.path.join(ROOT, "tests", "hostcheck", "msm_plan_check.hip")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", src, "-o", exe])

    def run(lanes, lo, hi, Ms):
        out = subprocess.check_output([exe, str(lanes), str(lo), str(hi)] + [str(m) for m in Ms], text=True)
        rows = [tuple(int(x) for x in line.split()) for line in out.strip().splitlines()]
        assert [r[0] for r in rows] == list(Ms)
        return rows
    return run


def test_plan_function_on_host(plan_check):
    """msm_plan_chunk and its packed word, compiled for the host (no GPU): lo <= chunk <= hi, chunk x lanes x rounds covers the list, the
    word round-trips at hi = 128, the headline list (15 x 2^20 entries over the 131 072 resident lanes of a 256-CU part) gets ONE round of
    120-entry chunks, and a chunk only grows beyond lo to save a round: lists of at most 30 entries per lane keep chunks <= 56."""
    lanes, lo, hi = LANES_MI355X_G1, 40, 128
    Ms = [0, 1, lanes * 56, lanes * 56 + 1, 15 << 20, 15 << 22]
    rows = plan_check(lanes, lo, hi, Ms)
    for M, chunk, rounds, via_word, w_lanes, w_lo, w_hi in rows:
        assert (w_lanes, w_lo, w_hi) == (lanes, lo, hi)
        assert via_word == chunk
        assert lo <= chunk <= hi, (M, chunk)
        assert chunk * lanes * rounds >= M, (M, chunk, rounds)
        assert rounds == -(-M // (lanes * hi))
    by_m = {r[0]: r for r in rows}
    assert by_m[15 << 20][1:3] == (120, 1)
    assert by_m[15 << 22][1:3] == (120, 4)
    assert by_m[lanes * 56][1:3] == (56, 1) and by_m[lanes * 56 + 1][1:3] == (57, 1)
    assert by_m[0][1:3] == (lo, 0) and by_m[1][1:3] == (lo, 1)
    # the lists of tests/test_gpu_msm.py::test_device_chosen_chunk_and_plan_report: n <= 2^18, <= 15 windows -> at most 30 entries per lane;
    # chunk_lo there is max(16, ceil(n W / (4 lanes)))
    for M in (1, 3000 * 15, 70000 * 15, 15 << 18):
        lo_small = max(16, -(-M // (4 * lanes)))
        for frac in (1, 2, 5):
            (_, chunk, rounds, via_word, *_), = plan_check(lanes, lo_small, hi, [M // frac])
            assert 16 <= chunk <= 56 and rounds <= 1 and via_word == chunk, (M, frac, chunk)
    # the same rule at the former bound and for a lane-split group's lane count
    for lanes2, hi2 in ((lanes, 56), (lanes // 2, 128), (lanes // 3, 128)):
        for M, chunk, rounds, via_word, *_ in plan_check(lanes2, 16, hi2, Ms):
            assert 16 <= chunk <= hi2 and chunk * lanes2 * rounds >= M and via_word == chunk
