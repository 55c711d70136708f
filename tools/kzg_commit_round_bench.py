"""Measurement of pcdhip_kzg_commit on one round of Marlin-like commitments: k = 9 polynomials over powers of 3n/2 bases -- lengths
n, n, n, 3n/2 and five of n/2 -- every one hiding with a 2-coefficient blinding polynomial, two of them (an n and an n/2) with a degree
bound.  MNT4-298 at n = 2^20 and MNT4-753 at n = 2^18 by default.  Median of REPS after one warm-up, per curve:

  (a) commit_ms         pcdhip_kzg_commit on the resident polynomials: device events (pcdhip_timer_start / stop on the context's stream,
                        which the call's epilogue joins), and the wall clock of the same calls;
  (b) host_driven_ms    what a caller had before: download the coefficients, convert them on the host, upload the scalars,
                        pcdhip_msm_submit / collect four in flight, the hiding MSMs from host scalars, host-driven sums and one
                        pcdhip_to_affine.  Wall clock;
  (c) msm_floor_ms      the same large MSMs through submit / collect over scalars converted beforehand, nothing else: the floor (a) should
                        approach.  Wall clock;
  conversion_upper_ms   the one launch of poly_commit_scalars cannot be called alone, so it is bounded from above in the same run by a
                        commit of all-zero polynomials of the same lengths: the launch with all its loads and stores, plus MSM pipelines
                        over empty bucket lists, the hiding MSMs and the epilogue.  Device events.
  commit_not_hiding_ms  the round without blinding polynomials, and hiding_msms_alone_ms: its 11 hiding MSMs with empty polynomials -- the two
                        parts of (a) apart.  Device events.
  *_short_ms            (a), the bound and the hiding MSMs again after pcdhip_msm_set_short(ctx, 8): the 2-coefficient hiding MSMs skip the buckets.

    python tools/kzg_commit_round_bench.py [--cases 0:20,2:18] [--reps 7] [--out profiles/kzg_commit_bench.json]

--batch measures the batched hiding MSMs instead (device events; median, min and max of REPS after one warm-up), per curve:
  commit_not_hiding     the round without blinding polynomials: what the hiding round should approach;
  commit_default        the hiding round under pcdhip_msm_set_short(ctx, 0): eleven bucket pipelines in sequence;
  commit_short8_gamma4 / _gamma64
                        the hiding round under pcdhip_msm_set_short(ctx, 8) with a 4-point powers_of_gamma_g (no copies: a short chain is the
                        scalar's bits) and a 64-point one (the smallest upload that gets window copies: the chain is about 2c) -- the
                        eleven hiding MSMs as ONE batched chain where the library has it, eleven chains in sequence where it has not;
  short_two_pairs_gamma4 / _gamma64
                        one pcdhip_msm_short_dev of two pairs over each handle, alone;
  batch22_gamma4 / _gamma64
                        22 such MSMs through pcdhip_msm_short_batch_dev (libraries that have it): about one of the above by count, not 22.

    python tools/kzg_commit_round_bench.py --batch [--cases 0:20,2:18] [--reps 7] [--out profiles/kzg_commit_bench_batch.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oracle import coracle as co  # noqa: E402
from pcd_amd import capi  # noqa: E402


def median_of(fn, reps):
    fn()
    ts = [fn() for _ in range(reps)]
    if isinstance(ts[0], tuple):
        return tuple(round(statistics.median(t[i] for t in ts), 3) for i in range(len(ts[0])))
    return round(statistics.median(ts), 3)


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def bench_curve(ctx, curve, log_n, reps):
    fr = co.CURVE_FR[curve]
    n = 1 << log_n
    npow = 3 * n // 2
    lens = [n, n, n, npow] + [n // 2] * 5
    shifted = {1: npow - n, 4: 7}  # item -> shifted_offset
    pts = co.gen_points_mt(curve, 1, npow, seed=161, threads=16)
    bases = ctx.bases_upload(curve, 1, pts)
    sbases = ctx.bases_upload(curve, 1, pts[::-1].copy())
    gbases = ctx.bases_upload(curve, 1, co.gen_points(curve, 1, 4, seed=162))
    del pts
    polys = [ctx.buf_upload(fr, co.gen_field(fr, m, seed=170 + j)) for j, m in enumerate(lens)]
    zeros = [ctx.buf_upload(fr, np.zeros((m, capi.FIELD_LIMBS[fr]), dtype=np.uint64)) for m in lens]
    bl_mont = [co.gen_field(fr, 2, seed=190 + j) for j in range(len(lens))]
    bls = [ctx.buf_upload(fr, x) for x in bl_mont]
    items = lambda ps: [dict(poly=p, blinding=bls[j], shifted=j in shifted, shifted_offset=shifted.get(j, 0),
                             shifted_blinding=bls[j] if j in shifted else None) for j, p in enumerate(ps)]
    res = {"curve": co.CURVE_NAMES[curve], "n": n, "powers": npow, "lens": lens, "shifted_items": sorted(shifted)}

    def commit(ps):
        ctx.timer_start()
        t = time.perf_counter()
        out = ctx.kzg_commit(bases, ps, powers_of_gamma_g=gbases, shifted_powers=sbases)
        w = (time.perf_counter() - t) * 1e3
        return ctx.timer_stop(), w, out

    res["commit_ms"], res["commit_wall_ms"] = median_of(lambda: commit(items(polys))[:2], reps)
    res["conversion_upper_ms"] = median_of(lambda: commit(items(zeros))[0], reps)
    want = commit(items(polys))[2]
    # where the distance to (c) goes: the same round without any blinding polynomial (the large MSMs, the conversion and the epilogue
    # remain), and the 11 hiding MSMs alone (empty polynomials: no conversion to speak of, no large MSM)
    bare = [dict(poly=p, shifted=j in shifted, shifted_offset=shifted.get(j, 0)) for j, p in enumerate(polys)]
    res["commit_not_hiding_ms"] = median_of(lambda: commit(bare)[0], reps)
    empty = [dict(it, len=0) for it in items(polys)]
    res["hiding_msms_alone_ms"] = median_of(lambda: commit(empty)[0], reps)
    # the same with the hiding MSMs (2 coefficients each) on the path without buckets: pcdhip_msm_set_short
    ctx.msm_set_short(8)
    res["commit_short_ms"], res["commit_short_wall_ms"] = median_of(lambda: commit(items(polys))[:2], reps)
    res["conversion_upper_short_ms"] = median_of(lambda: commit(items(zeros))[0], reps)
    res["hiding_msms_alone_short_ms"] = median_of(lambda: commit(empty)[0], reps)
    res["short_agrees"] = bool(all(np.array_equal(a, b) for a, b in zip(want, commit(items(polys))[2])))
    ctx.msm_set_short(0)

    # the MSMs as (bases, offset, scalars): the large ones, four in flight
    def large_msms(scal):
        jobs = [(bases, 0, s) for s in scal] + [(sbases, shifted[j], scal[j]) for j in sorted(shifted)]
        out, flight = [None] * len(jobs), []
        for i, (b, off, s) in enumerate(jobs):
            if len(flight) == 4:
                k, t = flight.pop(0)
                out[k] = ctx.msm_collect(t)
            flight.append((i, ctx.msm_submit(b, s, offset=off)))
        for k, t in flight:
            out[k] = ctx.msm_collect(t)
        return out

    canon_bl = [co.fp_op(fr, "to_canonical", x) for x in bl_mont]
    got = {}

    def host_driven():
        scal = [ctx.buf_upload(fr, co.fp_op(fr, "to_canonical", p.download())) for p in polys]
        big = large_msms(scal)
        hid = [ctx.msm(gbases, c) for c in canon_bl]
        k = len(lens)
        sums = [ctx.points_sum(curve, 1, np.stack([big[j], hid[j]])) for j in range(k)]
        sums += [ctx.points_sum(curve, 1, np.stack([big[k + i], hid[j]])) for i, j in enumerate(sorted(shifted))]
        got["aff"] = ctx.to_affine(curve, 1, np.stack(sums))
        for s in scal:
            s.free()

    res["host_driven_ms"] = median_of(lambda: wall(host_driven), reps)
    scal = [ctx.buf_upload(fr, co.fp_op(fr, "to_canonical", p.download())) for p in polys]
    res["msm_floor_ms"] = median_of(lambda: wall(lambda: large_msms(scal)), reps)
    # the two paths agree
    k = len(lens)
    aff = got["aff"][0]
    same = np.array_equal(aff[:k], want[0]) and all(np.array_equal(aff[k + i], want[2][j]) for i, j in enumerate(sorted(shifted)))
    res["paths_agree"] = bool(same)
    res["commit_over_floor"] = round(res["commit_wall_ms"] / res["msm_floor_ms"], 3)
    res["commit_short_over_floor"] = round(res["commit_short_wall_ms"] / res["msm_floor_ms"], 3)
    res["host_driven_over_commit"] = round(res["host_driven_ms"] / res["commit_wall_ms"], 2)
    for x in polys + zeros + bls + scal + [bases, sbases, gbases]:
        x.free()
    return res


def spread_of(fn, reps):
    fn()
    ts = [fn() for _ in range(reps)]
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def bench_batch(ctx, curve, log_n, reps):
    fr = co.CURVE_FR[curve]
    n = 1 << log_n
    npow = 3 * n // 2
    lens = [n, n, n, npow] + [n // 2] * 5
    shifted = {1: npow - n, 4: 7}  # item -> shifted_offset
    pts = co.gen_points_mt(curve, 1, npow, seed=161, threads=16)
    bases = ctx.bases_upload(curve, 1, pts)
    sbases = ctx.bases_upload(curve, 1, pts[::-1].copy())
    del pts
    gpts = co.gen_points(curve, 1, 64, seed=162)
    gammas = {4: ctx.bases_upload(curve, 1, gpts[:4]), 64: ctx.bases_upload(curve, 1, gpts)}
    polys = [ctx.buf_upload(fr, co.gen_field(fr, m, seed=170 + j)) for j, m in enumerate(lens)]
    bl_mont = [co.gen_field(fr, 2, seed=190 + j) for j in range(len(lens))]
    bls = [ctx.buf_upload(fr, x) for x in bl_mont]
    hiding = [dict(poly=p, blinding=bls[j], shifted=j in shifted, shifted_offset=shifted.get(j, 0),
                   shifted_blinding=bls[j] if j in shifted else None) for j, p in enumerate(polys)]
    bare = [dict(poly=p, shifted=j in shifted, shifted_offset=shifted.get(j, 0)) for j, p in enumerate(polys)]
    has_batch = hasattr(ctx, "msm_short_batch")
    res = {"curve": co.CURVE_NAMES[curve], "n": n, "powers": npow, "lens": lens, "shifted_items": sorted(shifted), "hiding_msms": 11,
           "library_has_batch": has_batch}
    out = {}

    def commit(items, g, tag=None):
        ctx.timer_start()
        r = ctx.kzg_commit(bases, items, powers_of_gamma_g=gammas[g], shifted_powers=sbases)
        ms = ctx.timer_stop()
        if tag:
            out[tag] = r
        return ms

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    res["commit_not_hiding"] = spread_of(lambda: commit(bare, 4), reps)
    res["commit_default"] = spread_of(lambda: commit(hiding, 4, "default4"), reps)
    commit(hiding, 64, "default64")
    ctx.msm_set_short(8)
    try:
        for g in (4, 64):
            res[f"commit_short8_gamma{g}"] = spread_of(lambda: commit(hiding, g, f"short{g}"), reps)
            if has_batch:
                res[f"commit_short8_gamma{g}_plan"] = list(ctx.kzg_commit_last_plan())
            res[f"short8_gamma{g}_agrees"] = bool(all(np.array_equal(a, b) for a, b in zip(out[f"default{g}"], out[f"short{g}"])))
    finally:
        ctx.msm_set_short(0)
    # the standalone short MSM of two pairs, and 22 of them as one batch: scalars = the 9 blinding polynomials, canonical, back to back
    canon = ctx.buf_upload(fr, np.concatenate([co.fp_op(fr, "to_canonical", x) for x in bl_mont]))
    items22 = [(0, 2 * (j % len(lens)), 2) for j in range(22)]
    for g in (4, 64):
        res[f"short_two_pairs_gamma{g}"] = spread_of(lambda: timed(lambda: ctx.msm_short(gammas[g], canon, n=2)), reps)
        if has_batch:
            res[f"batch22_gamma{g}"] = spread_of(lambda: timed(lambda: ctx.msm_short_batch(gammas[g], canon, items22)), reps)
            one = co.to_affine(curve, 1, ctx.msm_short(gammas[g], canon, n=2, scalar_offset=2))
            got = co.to_affine(curve, 1, ctx.msm_short_batch(gammas[g], canon, items22)[1])
            res[f"batch22_gamma{g}_agrees"] = bool(np.array_equal(one[0], got[0]))
    for x in polys + bls + [canon, bases, sbases] + list(gammas.values()):
        x.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", action="store_true", help="the batched hiding MSMs (see above) instead of the round's three paths")
    ap.add_argument("--cases", default="0:20,2:18", help="curve:log_n, comma separated")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = capi.Context(0)
    results = []
    for case in a.cases.split(","):
        c, l = case.split(":")
        results.append((bench_batch if a.batch else bench_curve)(ctx, int(c), int(l), a.reps))
        print(json.dumps(results[-1]), flush=True)
    ctx.close()
    line = json.dumps({"tool": "kzg_commit_round_bench", "mode": "batch" if a.batch else "round", "reps": a.reps, "results": results})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
