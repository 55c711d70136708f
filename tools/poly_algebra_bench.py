"""Measurement of the K8 vector algebra (Marlin's AHP rounds) at n = 2^log_n over the 298-bit and the 753-bit scalar field (fields 1
and 3): device-event times (pcdhip_timer_start / stop around each call, one warm-up, median of REPS) of

  vec_batch_inverse without and with a scale, vec_mul, poly_div_vanishing of 3n coefficients by X^n - 1, poly_mul of two polynomials
  of n/2 coefficients (a domain of n), and poly_div_linear of n coefficients as the yardstick of the same run,

with the effective bandwidth of the streaming kernels against their traffic, the ratio of the inversion to the yardstick, and the
exact-integer references of tests/poly_algebra_reference.py timed once on the host (labelled as such: Python loops, not ark-ff).

    python tools/poly_algebra_bench.py [--log-n 20] [--reps 7] [--out FILE.json]"""
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

import poly_algebra_reference as pr  # noqa: E402
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


def gbps(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 1e9, 1)


def bench_field(ctx, field, log_n, reps):
    L = pr.LIMBS[field]
    n = 1 << log_n
    eb = L * 8
    a = ctx.buf_upload(field, co.gen_field(field, n, seed=140))
    b = ctx.buf_upload(field, co.gen_field(field, n, seed=141))
    big = ctx.buf_upload(field, co.gen_field(field, 3 * n, seed=142))
    out, q, r = ctx.buf_alloc(field, n), ctx.buf_alloc(field, 2 * n), ctx.buf_alloc(field, n)
    z = co.gen_field(field, 1, seed=143)[0]
    res = {"field": field, "bits": 298 if field < 2 else 753, "n": n}
    res["poly_div_linear_ms"] = timed(ctx, lambda: ctx.poly_div_linear(a, z, q=q), reps)
    res["vec_batch_inverse_ms"] = timed(ctx, lambda: ctx.vec_batch_inverse(a, out=out), reps)
    res["vec_batch_inverse_scaled_ms"] = timed(ctx, lambda: ctx.vec_batch_inverse(a, scale_mont=z, out=out), reps)
    res["batch_inverse_over_div_linear"] = round(res["vec_batch_inverse_ms"] / res["poly_div_linear_ms"], 2)
    res["vec_mul_ms"] = timed(ctx, lambda: ctx.vec_mul(a, b, out=out), reps)
    res["vec_mul_effective_GBps"] = gbps(3 * n * eb, res["vec_mul_ms"])                    # a, b read, out written
    res["poly_div_vanishing_3n_ms"] = timed(ctx, lambda: ctx.poly_div_vanishing(big, n, q=q, r=r), reps)
    res["poly_div_vanishing_effective_GBps"] = gbps(6 * n * eb, res["poly_div_vanishing_3n_ms"])  # 3n read, 2n + n written
    res["poly_mul_half_n_ms"] = timed(ctx, lambda: ctx.poly_mul(a, b, la=n // 2, lb=n // 2, out=out), reps)
    # the host-side comparison: the exact-integer references in Python on the same vectors (the product on a 2^10 slice: quadratic)
    p = pr.MODULI[field]
    ai = pr.to_ints(co, field, a.download())
    t = time.perf_counter()
    pr.batch_inverse(ai, p)
    res["host_python_batch_inverse_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    bi = pr.to_ints(co, field, big.download())
    t = time.perf_counter()
    pr.div_vanishing(bi, n, p)
    res["host_python_div_vanishing_3n_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    t = time.perf_counter()
    pr.mul_schoolbook(ai[:1024], ai[1024:2048], p)
    res["host_python_schoolbook_1024_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    for x in (a, b, big, out, q, r):
        x.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fields", default="1,3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = capi.Context(0)
    res = {"tool": "poly_algebra_bench", "reps": a.reps, "results": [bench_field(ctx, int(f), a.log_n, a.reps) for f in a.fields.split(",")]}
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
