"""Measurement of K12 (Marlin's second sumcheck) over the 298-bit and the 753-bit scalar field (fields 1 and 3).  Device-event times
(pcdhip_timer_start / stop around each call, one warm-up, median of REPS with the smallest and largest sample beside it) of

  a. marlin_sumcheck2_q on 2^log_n elements against the same q composed from the calls that were there before it --
     pcdhip_marlin_sumcheck_ab, pcdhip_vec_mul, pcdhip_poly_lincomb -- the two alternating sample by sample, both outputs compared for
     equality before a time is accepted; the kernel counts as faster only if its slowest sample is below the composition's fastest;
  b. its effective bandwidth, counting fourteen vectors (thirteen read, one written);
  c. pcdhip_marlin_sumcheck2 whole under route 1 and under route 2 (into buffers allocated beforehand) on the index of
     coracle.witness_r1cs at |H| = 2^log_h (|K| = 2^22 and |B| = 2^24 at log_h = 20), and the share of the transforms in each: the
     same transforms timed alone through pcdhip_fft_general_dev / pcdhip_poly_evals_on_domain, conversions of image included.

    python tools/marlin_sumcheck2_bench.py [--log-n 24] [--log-h 20] [--reps 7] [--fields 1,3] [--log-k-cap 0]
                                           [--out profiles/marlin_sumcheck2_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import kzg_reference as kr  # noqa: E402
from marlin_index_bench import NUM_INPUTS, capped  # noqa: E402
from oracle import coracle as co  # noqa: E402
from pcd_amd import capi  # noqa: E402


def sample(ctx, fn):
    ctx.timer_start()
    fn()
    return ctx.timer_stop()


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def timed(ctx, fn, reps):
    fn()
    return stats([sample(ctx, fn) for _ in range(reps)])


def bench_q(ctx, field, n, reps):
    L, p = kr.LIMBS[field], kr.MODULI[field]
    mont = lambda xs: kr.to_mont(co, field, xs)
    vecs = [ctx.buf_upload(field, co.gen_field(field, n, seed=280))]
    for _ in range(12):
        vecs.append(ctx.vec_mul(vecs[-1], vecs[0]))
    row, col, rc, val, f = vecs[0:3], vecs[3:6], vecs[6:9], vecs[9:12], vecs[12]
    consts = co.gen_field(field, 5, seed=281)
    alpha, beta, coeff = consts[0], consts[1], consts[2:5]
    q, q2, a, b, bf = (ctx.buf_alloc(field, n) for _ in range(5))
    pm = mont([1, p - 1])
    res = {"elements": n, "composed_calls": 3}
    for name, rcv in (("with_row_col", rc), ("without_row_col", None)):
        def fused():
            ctx.marlin_sumcheck2_q(alpha, beta, coeff, row, col, rcv, val, f, out=q)

        def composed():
            ctx.marlin_sumcheck_ab(alpha, beta, coeff, row, col, rcv, val, a_out=a, b_out=b)
            ctx.vec_mul(b, f, out=bf)
            ctx.poly_lincomb([a, bf], pm, q2)

        fused(), composed()
        ctx.sync()
        assert np.array_equal(q.download(), q2.download()), "the composition differs from the fused kernel"
        tf, tc = [], []
        for _ in range(reps):  # alternating, so that whatever else the machine does falls on both
            tf.append(sample(ctx, fused))
            tc.append(sample(ctx, composed))
        one = {"outputs_equal": True, "fused": stats(tf), "composed": stats(tc)}
        one["fused_over_composed"] = round(one["fused"]["median_ms"] / one["composed"]["median_ms"], 3)
        one["beats_composed_beyond_spread"] = one["fused"]["max_ms"] < one["composed"]["min_ms"]
        streams = 14 if rcv is not None else 11  # the vectors read, and the one written
        one["fused_effective_GBps"] = round(streams * n * L * 8 / (one["fused"]["median_ms"] * 1e-3) / 1e9, 1)
        res[name] = one
    for x in vecs + [q, q2, a, b, bf]:
        x.free()
    return res


def bench_driver(ctx, field, log_h, reps, log_k_cap):
    lib = capi.lib()
    L = kr.LIMBS[field]
    h_n = 1 << log_h
    r = co.witness_r1cs(field, h_n - NUM_INPUTS - 4, NUM_INPUTS, seed=150)
    if log_k_cap:
        r = capped(r, 1 << log_k_cap)
    idx = ctx.marlin_index_build(field, r, h_n, NUM_INPUTS, keep=6)
    info = idx.info()
    k_n, b_n = info["domain_k_n"], info["domain_b_n"]
    consts = co.gen_field(field, 5, seed=282)
    alloc = lambda n: ctx.buf_alloc(field, n)
    f_poly, g2, sigma, h2, rem = alloc(k_n), alloc(k_n - 1), alloc(1), alloc(3 * k_n - 3), alloc(k_n)
    lens = (C.c_size_t * 3)()
    res = {"H": h_n, "K": k_n, "B": b_n, "index_device_bytes": info["device_bytes"]}
    words = {}
    for route in (1, 2):
        if b_n < (4 * k_n - 3 if route == 1 else 3 * k_n - 2):
            res["route%d" % route] = None
            continue

        def whole():
            ctx._check(lib.pcdhip_marlin_sumcheck2(ctx._ctx, idx._h, consts[0].ctypes.data, consts[1].ctypes.data, consts[2:5].ctypes.data, route,
                                                   f_poly._h, g2._h, sigma._h, h2._h, rem._h, lens))
        res["route%d" % route] = timed(ctx, whole, reps)
        assert list(lens) == [k_n - 1, 3 * k_n - 3, route]
        words[route] = h2.download()
        res["route%d_remainder_is_zero" % route] = not rem.download().any()
    if len(words) == 2:
        res["h2_equal_under_both_routes"] = bool(np.array_equal(words[1], words[2]))
    # the transforms alone: inverse on K (in place), forward on B from |K| coefficients, inverse on B, and route 2's product domain
    big = alloc(b_n)
    inv_k = timed(ctx, lambda: ctx.fft_general_dev(f_poly, k_n, inverse=True), reps)
    fwd_b = timed(ctx, lambda: ctx.poly_evals_on_domain(f_poly, b_n, length=k_n, out=big), reps)
    inv_b = timed(ctx, lambda: ctx.fft_general_dev(big, b_n, inverse=True), reps)
    res["inverse_on_K"], res["forward_on_B"], res["inverse_on_B"] = inv_k, fwd_b, inv_b
    big.free()
    m_n = lib.pcdhip_domain_size(field, 4 * k_n - 3)
    prod = alloc(m_n)
    tr_m = timed(ctx, lambda: ctx.fft_general_dev(prod, m_n, inverse=True), reps)
    prod.free()
    res["product_domain"], res["transform_on_product_domain"] = m_n, tr_m
    if res.get("route1"):
        tr = inv_k["median_ms"] + fwd_b["median_ms"] + inv_b["median_ms"]
        res["route1_transform_share"] = round(tr / res["route1"]["median_ms"], 3)
    if res.get("route2"):
        tr = inv_k["median_ms"] + 2 * inv_b["median_ms"] + 3 * tr_m["median_ms"]
        res["route2_transform_share"] = round(tr / res["route2"]["median_ms"], 3)
    res["bytes_of_one_B_vector"] = b_n * L * 8
    for x in (f_poly, g2, sigma, h2, rem):
        x.free()
    idx.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=24)
    ap.add_argument("--log-h", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fields", default="1,3")
    ap.add_argument("--log-k-cap", type=int, default=0)
    ap.add_argument("--skip-driver", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marlin_sumcheck2_bench.json"))
    a = ap.parse_args()
    ctx = capi.Context(0)
    res = {"tool": "marlin_sumcheck2_bench", "reps": a.reps, "results": []}
    for f in a.fields.split(","):
        one = {"field": int(f), "bits": 298 if int(f) < 2 else 753, "sumcheck2_q": bench_q(ctx, int(f), 1 << a.log_n, a.reps)}
        print(json.dumps(one), flush=True)
        if not a.skip_driver:
            one["driver"] = bench_driver(ctx, int(f), a.log_h, a.reps, a.log_k_cap)
            print(json.dumps(one["driver"]), flush=True)
        res["results"].append(one)
    ctx.close()
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
