"""GPU: the routing of pcdhip_kzg_commit's hiding MSMs under pcdhip_msm_set_short -- those of at most that many coefficients run as ONE
batched short chain (msm_short_batch_async) that writes straight into the commit's result slots, the others keep the bucket pipeline;
pcdhip_kzg_commit_last_plan says which path ran.  Outputs equal the integer reference of tests/kzg_commit_reference.py and are
byte-identical between the two routes."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzg_commit_reference as kc  # noqa: E402
import kzg_reference as kr  # noqa: E402

pytestmark = pytest.mark.gpu

N = 128          # powers of g and shifted powers
PAD = 5          # non-zero elements behind every polynomial's `len`, which no call may read
# (len, shifted offset or None): five items, every one hiding with a 2-coefficient blinding; the two with a degree bound carry a shifted
# blinding of 2 coefficients as well -- seven hiding MSMs, seven large ones
SPEC = [(40, None), (100, 28), (57, None), (64, 3), (83, None)]


def upload(ctx, co, rnd, fr, ints):
    p = kr.MODULI[fr]
    return ctx.buf_upload(fr, kr.to_mont(co, fr, list(ints) + [rnd.randrange(1, p) for _ in range(PAD)]))


@pytest.mark.parametrize("gamma_points", (4, 64))
@pytest.mark.parametrize("curve", (0, 2))   # MNT4-298, MNT4-753
def test_hiding_msms_take_the_batch(co, gpu_ctx, curve, gamma_points):
    ctx = gpu_ctx
    fr = co.CURVE_FR[curve]
    p, rnd = kr.MODULI[fr], random.Random(1400 + curve)
    pts = co.gen_points(curve, 1, N, seed=1410 + curve)
    spts = co.gen_points(curve, 1, N, seed=1420 + curve)
    gpts = co.gen_points(curve, 1, gamma_points, seed=1430 + curve)
    bases, sbases, gbases = (ctx.bases_upload(curve, 1, x) for x in (pts, spts, gpts))
    polys = [[rnd.randrange(p) for _ in range(n)] for n, _ in SPEC]
    bls = [[rnd.randrange(p) for _ in range(2)] for _ in SPEC]
    sbls = [None if off is None else [rnd.randrange(p) for _ in range(2)] for _, off in SPEC]
    bufs = [upload(ctx, co, rnd, fr, a) for a in polys]
    bbufs = [upload(ctx, co, rnd, fr, a) for a in bls]
    sbufs = [None if a is None else upload(ctx, co, rnd, fr, a) for a in sbls]
    items = []
    for j, (n, off) in enumerate(SPEC):
        it = dict(poly=bufs[j], len=n, blinding=bbufs[j], blinding_len=2)
        if off is not None:
            it.update(shifted=True, shifted_offset=off, shifted_blinding=sbufs[j], shifted_blinding_len=2)
        items.append(it)
    runs, plans = {}, {}
    try:
        for short in (0, 8, 1):
            ctx.msm_set_short(short)
            runs[short] = ctx.kzg_commit(bases, items, powers_of_gamma_g=gbases, shifted_powers=sbases)
            plans[short] = ctx.kzg_commit_last_plan()
    finally:
        ctx.msm_set_short(0)
    # which path ran: all seven in the batch under 8 (one part each: two launches), none under 0, none under 1 (blindings of two exceed it)
    assert plans[0] == (7, 0, 7, 0)
    assert plans[8] == (7, 7, 0, 2)
    assert plans[1] == (7, 0, 7, 0)
    for short in (8, 1):
        for a, b in zip(runs[0], runs[short]):
            assert np.array_equal(a, b), ("byte-identical with and without the batch", short)
    comm, cinf, sh, sinf, tl = runs[8]
    for j, (n, off) in enumerate(SPEC):
        w = kc.commit(co, curve, pts, polys[j], gpts, bls[j])
        assert int(tl[j]) == w[2] == n
        assert int(cinf[j]) == w[1] and np.array_equal(comm[j], w[0])
        if off is None:
            assert int(sinf[j]) == 1 and not sh[j].any()
        else:
            ws = kc.commit(co, curve, spts, polys[j], gpts, sbls[j], offset=off)
            assert int(sinf[j]) == ws[1] and np.array_equal(sh[j], ws[0])
    for h in bufs + bbufs + [x for x in sbufs if x is not None] + [bases, sbases, gbases]:
        h.free()
