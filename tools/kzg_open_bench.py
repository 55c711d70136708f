"""Measurement of the K7 open side (KZG10 / MarlinKZG10 openings) at n = 2^20 on MNT4-298 and MNT4-753 G1: device-event times
(pcdhip_timer_start / stop around each call, one warm-up, median of REPS) of

  poly_div_linear (one polynomial), poly_eval (10 polynomials), poly_lincomb (10 polynomials), kzg_open without and with a 2-coefficient
  blinding polynomial, the bare pcdhip_msm_dev of the same length, kzg_check of 1 and of 16 openings,

and the division's effective bandwidth against its three-vector traffic (p read twice, q written once).  Random points stand in for
the powers of an SRS (the timings do not depend on them).  The exact-integer division of tests/kzg_reference.py is timed on the host
once per field for comparison (labelled as such: a Python loop, not ark-poly).

    python tools/kzg_open_bench.py [--log-n 20] [--reps 7] [--out FILE.json]"""
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


def timed(ctx, fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return round(statistics.median(ts), 4)


def bench_curve(ctx, curve, log_n, reps, threads):
    fr = co.CURVE_FR[curve]
    L = kr.LIMBS[fr]
    n = 1 << log_n
    t = time.time()
    pts = co.gen_points_mt(curve, 1, n, seed=81 + curve, threads=threads)
    gpts = co.gen_points(curve, 1, 2, seed=91 + curve)
    gen_s = time.time() - t
    P = ctx.bases_upload(curve, 1, pts)
    G = ctx.bases_upload(curve, 1, gpts)
    polys = [ctx.buf_upload(fr, co.gen_field(fr, n, seed=100 + j)) for j in range(10)]
    p = polys[0]
    blind = ctx.buf_upload(fr, co.gen_field(fr, 2, seed=120))
    scal = ctx.buf_upload(fr, co.gen_scalars(fr, n, seed=121))
    q = ctx.buf_upload(fr, np.zeros((n - 1, L), dtype=np.uint64))
    out = ctx.buf_upload(fr, np.zeros((n, L), dtype=np.uint64))
    z = co.gen_field(fr, 1, seed=122)[0]
    coeffs = co.gen_field(fr, 10, seed=123)
    r = {"curve": co.CURVE_NAMES[curve], "n": n, "points_gen_s": round(gen_s, 1)}
    r["poly_div_linear_ms"] = timed(ctx, lambda: ctx.poly_div_linear(p, z, q=q), reps)
    r["poly_eval_10_ms"] = timed(ctx, lambda: ctx.poly_eval(polys, z), reps)
    r["poly_lincomb_10_ms"] = timed(ctx, lambda: ctx.poly_lincomb(polys, coeffs, out), reps)
    r["kzg_open_ms"] = timed(ctx, lambda: ctx.kzg_open(P, p, z), reps)
    r["kzg_open_hiding_ms"] = timed(ctx, lambda: ctx.kzg_open(P, p, z, powers_of_gamma_g=G, blinding=blind), reps)
    r["msm_dev_ms"] = timed(ctx, lambda: ctx.msm(P, scal, n=n - 1), reps)
    r["division_share_of_open"] = round(r["poly_div_linear_ms"] / r["kzg_open_hiding_ms"], 4)
    # three vectors of n ABI elements: p read by the tile pass and by the quotient pass, q written once
    traffic = 3 * n * L * 8
    r["division_traffic_bytes"] = traffic
    r["division_effective_GBps"] = round(traffic / (r["poly_div_linear_ms"] * 1e-3) / 1e9, 1)
    # kzg_check: random G1 points stand in for commitments and witnesses (the timing does not depend on them)
    g, h = co.generator(curve, 1), co.generator(curve, 2)
    for k in (1, 16):
        cs = co.gen_points(curve, 1, k, seed=130)
        ws = co.gen_points(curve, 1, k, seed=131)
        vals = co.gen_field(fr, 3 * k, seed=132)
        rs = co.gen_scalars(fr, k, seed=133)
        rs[0] = 0
        rs[0, 0] = 1
        r[f"kzg_check_{k}_ms"] = timed(ctx, lambda: ctx.kzg_check(curve, g, h, h, cs, vals[:k], vals[k:2 * k], ws, gamma_g_xy=g,
                                                                  random_v_mont=vals[2 * k:], randomizers_canonical=rs), reps)
    # the host-side comparison: the exact-integer recurrence in Python on the same polynomial
    ints = kr.to_ints(co, fr, p.download())
    zi = kr.to_ints(co, fr, z)[0]
    t = time.perf_counter()
    kr.div_linear(ints, zi, kr.MODULI[fr])
    r["host_python_division_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    for b in polys + [blind, scal, q, out]:
        b.free()
    P.free()
    G.free()
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
    res = {"tool": "kzg_open_bench", "reps": a.reps, "results": [bench_curve(ctx, int(c), a.log_n, a.reps, a.threads) for c in a.curves.split(",")]}
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
