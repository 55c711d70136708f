"""Measurement of K13, pcdhip_kzg_batch_open, on the shape of a Marlin proof's last round at n = 2^20 on MNT4-298 and MNT4-753 G1:
2 points, a combination of 7 items at the first and of 14 at the second, one degree-bound term per point, blinding polynomials of two
coefficients.  The one call is timed against the same openings COMPOSED from the calls the library had before, in the same process:
per point poly_lincomb (combined polynomial) + poly_lincomb (combined blinding) + kzg_open, and for the degree-bound term poly_lincomb
(the polynomial times its challenge) + kzg_open over a handle that starts at the item's offset.  The composition's host-side additions
of its two witnesses per point are NOT timed (they would only add to it).

Outputs are compared first.  Then the two alternate, sample by sample: device events (pcdhip_timer_start / stop) for the queued part,
wall clock for the whole call -- the composition's cost is host waits, which device events do not see.  One warm-up each, median of REPS
with the smallest and the largest.  "faster" is claimed only when the new call's slowest sample is below the composition's fastest.
Beside them the three launches alone (pcdhip_poly_open_quotients) and the bare pcdhip_msm_dev of the same lengths (the four large MSMs
of the round, one after the other): the floor the call cannot go below -- and the one call again under pcdhip_msm_set_short(8), where
its two hiding MSMs (one scalar each) leave the bucket pipeline for the batched short chain.  Random points stand in for the powers of
an SRS (the timings do not depend on them).

    python tools/kzg_batch_open_bench.py [--log-n 20] [--reps 7] [--out profiles/kzg_batch_open_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import kzg_reference as kr  # noqa: E402
from oracle import coracle as co  # noqa: E402
from pcd_amd import capi  # noqa: E402

OFFSET = 16  # shifted_offset of the two degree-bound items (their polynomials are that much shorter)


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def bench_curve(ctx, curve, log_n, reps, threads):
    fr = co.CURVE_FR[curve]
    L = kr.LIMBS[fr]
    n = 1 << log_n
    pts = co.gen_points_mt(curve, 1, n, seed=81 + curve, threads=threads)
    gpts = co.gen_points(curve, 1, 2, seed=91 + curve)
    P, G = ctx.bases_upload(curve, 1, pts), ctx.bases_upload(curve, 1, gpts)
    PO = ctx.bases_upload(curve, 1, pts[OFFSET:])  # what the composition needs for a degree-bound witness: a handle from the offset on
    m, groups, bound = 21, [list(range(7)), list(range(7, 21))], [0, 7]
    lens = [n - OFFSET if i in bound else n for i in range(m)]
    polys = [ctx.buf_upload(fr, co.gen_field(fr, lens[i], seed=100 + i)) for i in range(m)]
    blinds = [ctx.buf_upload(fr, co.gen_field(fr, 2, seed=140 + i)) for i in range(m)]
    items = [dict(poly=polys[i], blinding=blinds[i]) for i in range(m)]
    for i in bound:
        items[i].update(shifted=True, shifted_offset=OFFSET)
    z = co.gen_field(fr, 2, seed=122)
    ch = co.gen_field(fr, m, seed=123)
    xs = co.gen_field(fr, 2, seed=124)
    a = np.zeros((2, m, L), dtype=np.uint64)
    s = np.zeros((2, m, L), dtype=np.uint64)
    for o in range(2):
        a[o, groups[o]] = ch[groups[o]]
        s[o, bound[o]] = xs[o]
    out, rout, sout = ctx.buf_alloc(fr, n), ctx.buf_alloc(fr, 2), ctx.buf_alloc(fr, n)

    def one_call():
        return ctx.kzg_batch_open(P, items, z, a, s, powers_of_gamma_g=G, shifted_powers=P)

    def composed():
        res = []
        for o in range(2):
            g = groups[o]
            k = ctx.poly_lincomb([polys[i] for i in g], ch[g], out)
            ctx.poly_lincomb([blinds[i] for i in g], ch[g], rout)
            w, v, rv = ctx.kzg_open(P, out, z[o], length=k, powers_of_gamma_g=G, blinding=rout)
            i = bound[o]
            k = ctx.poly_lincomb([polys[i]], xs[o:o + 1], sout)
            w2, _, _ = ctx.kzg_open(PO, sout, z[o], length=k)
            res.append((w, w2, v, rv))
        return res

    # outputs first
    w, winf, v, rv = one_call()
    for o, (w1, w2, v1, rv1) in enumerate(composed()):
        xy, inf = co.to_affine(curve, 1, co.jac_add(curve, 1, w1, w2))
        assert int(inf[0]) == int(winf[o]) == 0 and np.array_equal(xy[0], w[o]), "the witness differs from the composition's"
        assert np.array_equal(v1, v[o]) and np.array_equal(rv1, rv[o]), "a value differs from the composition's"
    plan = ctx.kzg_batch_open_last_plan()
    samples = {"batch_open": ([], []), "composed": ([], [])}
    for rep in range(reps + 1):  # (the first round is the warm-up of both)
        for name, fn in (("batch_open", one_call), ("composed", composed)):
            t = time.perf_counter()
            ctx.timer_start()
            fn()
            dev = ctx.timer_stop()
            wall = (time.perf_counter() - t) * 1e3
            if rep:
                samples[name][0].append(dev)
                samples[name][1].append(wall)
    r = {"curve": co.CURVE_NAMES[curve], "n": n, "items": m, "points": 2, "terms": [7, 14], "degree_bound_terms": [1, 1], "plan": list(plan)}
    for name, (dev, wall) in samples.items():
        r[name + "_device_ms"] = stats(dev)
        r[name + "_wall_ms"] = stats(wall)
    r["faster_wall"] = bool(max(samples["batch_open"][1]) < min(samples["composed"][1]))
    r["faster_device"] = bool(max(samples["batch_open"][0]) < min(samples["composed"][0]))
    # the same call with its hiding MSMs in the batched short chain
    ctx.msm_set_short(8)
    try:
        short = []
        for rep in range(reps + 1):
            ctx.timer_start()
            one_call()
            dev = ctx.timer_stop()
            if rep:
                short.append(dev)
        r["batch_open_short8_device_ms"] = stats(short)
        r["plan_short8"] = list(ctx.kzg_batch_open_last_plan())
    finally:
        ctx.msm_set_short(0)
    # the three launches alone (pcdhip_poly_open_quotients into buffers allocated once): the call's share that is not MSM
    q_bufs, _, _ = ctx.poly_open_quotients(fr, items, z, a, s)
    chain = []
    for rep in range(reps + 1):
        ctx.timer_start()
        ctx.poly_open_quotients(fr, items, z, a, s, q_bufs=q_bufs)
        dev = ctx.timer_stop()
        if rep:
            chain.append(dev)
    r["quotients_device_ms"] = stats(chain)
    for b in q_bufs.values():
        b.free()
    # the floor: the round's four large MSMs, bare, one after the other
    scal = ctx.buf_upload(fr, co.gen_scalars(fr, n, seed=121))
    floor = []
    for rep in range(reps + 1):
        ctx.timer_start()
        for k in (n - 1, n - OFFSET - 1, n - 1, n - OFFSET - 1):
            ctx.msm(P, scal, n=k)
        if rep:
            floor.append(ctx.timer_stop())
        else:
            ctx.timer_stop()
    r["bare_msm_dev_x4_ms"] = stats(floor)
    for b in polys + blinds + [out, rout, sout, scal, P, G, PO]:
        b.free()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--curves", default="0,2")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = capi.Context(0)
    res = {"tool": "kzg_batch_open_bench", "reps": a.reps, "results": [bench_curve(ctx, int(c), a.log_n, a.reps, a.threads) for c in a.curves.split(",")]}
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
