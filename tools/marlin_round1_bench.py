"""Measurement of K11 (Marlin's round 1 and the first sumcheck) at |H| = 2^log_h, |D| = pcdhip_domain_size(3 |H|) over the 298-bit and
the 753-bit scalar field (fields 1 and 3).  Device-event times (pcdhip_timer_start / stop around each call, one warm-up, median of
REPS with the smallest and largest sample beside it) of

  a. marlin_sumcheck1_q on |D| elements against the same q composed from calls that were there before it -- three pcdhip_vec_mul and
     two pcdhip_poly_lincomb -- the two alternating sample by sample, both outputs compared for equality before a time is accepted;
  b. its effective bandwidth, counting six vectors of |D| elements (five read, one written);
  c. marlin_zm_evals on the matrices of coracle.witness_r1cs and coracle.skewed_r1cs (2^log_h variables) against the forward mat-vecs
     of the same matrices inside the witness map (out_ms[0] of pcdhip_g16_witness_map_resident), with the two conversions of image
     that zm_evals adds timed on their own;
  d. marlin_round1 and marlin_sumcheck1 whole (into buffers allocated beforehand), and the share of the transforms in each: the same
     transforms timed alone through pcdhip_fft_general_dev / pcdhip_poly_evals_on_domain, conversions of image included as in the drivers.

    python tools/marlin_round1_bench.py [--log-h 20] [--reps 7] [--fields 1,3] [--out profiles/marlin_round1_bench.json]"""
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
from marlin_rounds_bench import NUM_INPUTS, placeholder_key  # noqa: E402
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
    vecs = [ctx.buf_upload(field, co.gen_field(field, n, seed=260))]
    for _ in range(4):
        vecs.append(ctx.vec_mul(vecs[-1], vecs[0]))
    za, zb, r, t, z = vecs
    eta = kr.to_ints(co, field, co.gen_field(field, 3, seed=261))
    eta_m = mont(eta)
    q, q2 = ctx.buf_alloc(field, n), ctx.buf_alloc(field, n)
    m, inner, p2 = (ctx.buf_alloc(field, n) for _ in range(3))
    pm = mont([1, p - 1])

    def fused():
        ctx.marlin_sumcheck1_q(eta_m, za, zb, r, t, z, out=q)

    def composed():
        ctx.vec_mul(za, zb, out=m)
        ctx.poly_lincomb([za, zb, m], eta_m, inner)
        ctx.vec_mul(r, inner, out=inner)
        ctx.vec_mul(t, z, out=p2)
        ctx.poly_lincomb([inner, p2], pm, q2)

    fused(), composed()
    ctx.sync()
    assert np.array_equal(q.download(), q2.download()), "the composition differs from the fused kernel"
    tf, tc = [], []
    for _ in range(reps):  # alternating, so that whatever else the machine does falls on both
        tf.append(sample(ctx, fused))
        tc.append(sample(ctx, composed))
    res = {"elements": n, "outputs_equal": True, "composed_calls": 5, "fused": stats(tf), "composed": stats(tc)}
    res["fused_over_composed"] = round(res["fused"]["median_ms"] / res["composed"]["median_ms"], 3)
    res["beats_composed_beyond_spread"] = res["fused"]["max_ms"] < res["composed"]["min_ms"]
    res["fused_effective_GBps"] = round(6 * n * L * 8 / (res["fused"]["median_ms"] * 1e-3) / 1e9, 1)  # five vectors read, one written
    for x in vecs + [q, q2, m, inner, p2]:
        x.free()
    return res


def bench_zm(ctx, field, log_h, reps, shape):
    h_n = 1 << log_h
    nc = h_n - NUM_INPUTS - 4  # num_vars = nc + num_inputs + 4 = |H|
    r = (co.witness_r1cs if shape == "witness" else co.skewed_r1cs)(field, nc, NUM_INPUTS, seed=150)
    assert r.num_vars == h_n and capi.lib().pcdhip_domain_size(field, r.num_vars) == h_n
    res = {"shape": shape + "_r1cs", "constraints": nc, "variables": r.num_vars, "nnz": [int(rp[-1]) for rp in (r.rp_a, r.rp_b, r.rp_c)]}
    curve = co.CURVE_FR.index(field)
    ctx.set_precompute(0)
    keys = placeholder_key(curve, r)
    pk = ctx.g16_pk_upload(keys.host_struct(), curve)
    ctx.g16_pk_set_r1cs(pk, r)
    ctx.witness_map_resident(pk, r, want_h=False)
    res["forward_spmv3"] = stats([ctx.witness_map_resident(pk, r, want_h=False)[1]["spmv"] for _ in range(reps)])
    pk.free()
    ctx.set_precompute(-1)
    mats = ctx.marlin_mats_upload_ex(field, r, h_n, NUM_INPUTS, 3)
    zbuf = ctx.buf_upload(field, r.z)
    outs = [ctx.buf_alloc(field, h_n) for _ in range(3)]
    res["zm_evals"] = timed(ctx, lambda: ctx.marlin_zm_evals(mats, zbuf, *outs), reps)
    res["zm_evals_without_c"] = timed(ctx, lambda: ctx.marlin_zm_evals(mats, zbuf, outs[0], outs[1], want_c=False), reps)
    # what zm_evals adds to the mat-vecs: z into the device image and three vectors of |H| elements out of it, four conversions of one
    # read and one write each.  No call converts alone; for scale, the pointwise product of the same length (two reads, one write)
    res["vec_mul_same_length"] = timed(ctx, lambda: ctx.vec_mul(outs[0], outs[1], out=outs[2]), reps)
    res["zm_evals_over_forward"] = round(res["zm_evals"]["median_ms"] / res["forward_spmv3"]["median_ms"], 3)
    for x in outs:
        x.free()
    return res, r, mats, zbuf


def bench_drivers(ctx, field, log_h, reps, r, mats, zbuf):
    lib = capi.lib()
    L = kr.LIMBS[field]
    h_n, x_n = 1 << log_h, NUM_INPUTS
    d_n = lib.pcdhip_domain_size(field, 3 * h_n)
    blind = co.gen_field(field, 3, seed=270)
    alloc = lambda n: ctx.buf_alloc(field, n)
    x_hat, z_poly, w, w_rem, za_poly, zb_poly = alloc(x_n), alloc(h_n + 1), alloc(h_n + 1 - x_n), alloc(x_n), alloc(h_n + 1), alloc(h_n + 1)
    lens5, lens3 = (C.c_size_t * 5)(), (C.c_size_t * 3)()
    bp = lambda k: blind[k:k + 1].ctypes.data

    def round1():
        ctx._check(lib.pcdhip_marlin_round1(ctx._ctx, mats._h, zbuf._h, bp(0), 1, bp(1), 1, bp(2), 1, x_hat._h, z_poly._h, w._h, w_rem._h,
                                            za_poly._h, zb_poly._h, None, None, lens5))
    res = {"H": h_n, "X": x_n, "D": d_n, "blinding": [1, 1, 1], "round1": timed(ctx, round1, reps)}
    assert list(lens5) == [x_n, h_n + 1, h_n + 1 - x_n, h_n + 1, h_n + 1] and not w_rem.download().any()
    eta, alpha = co.gen_field(field, 3, seed=271), co.gen_field(field, 1, seed=272)
    t_poly, h1, g1, sigma = alloc(h_n), alloc(2 * h_n), alloc(h_n - 1), alloc(1)

    def sumcheck1():
        ctx._check(lib.pcdhip_marlin_sumcheck1(ctx._ctx, mats._h, eta.ctypes.data, alpha.ctypes.data, za_poly._h, h_n + 1, zb_poly._h, h_n + 1,
                                               z_poly._h, h_n + 1, None, 0, 0, t_poly._h, h1._h, g1._h, sigma._h, lens3))
    res["sumcheck1"] = timed(ctx, sumcheck1, reps)
    assert list(lens3) == [h_n, 2 * h_n, h_n - 1]
    res["sigma_is_zero"] = not sigma.download().any()  # the benchmark's systems are satisfied ones
    # the transforms alone: inverse on H (in place), forward on D from |H| + 1 coefficients, inverse on D
    big = alloc(d_n)
    inv_h = timed(ctx, lambda: ctx.fft_general_dev(t_poly, h_n, inverse=True), reps)
    fwd_d = timed(ctx, lambda: ctx.poly_evals_on_domain(za_poly, d_n, length=h_n + 1, out=big), reps)
    inv_d = timed(ctx, lambda: ctx.fft_general_dev(big, d_n, inverse=True), reps)
    res["inverse_on_H"], res["forward_on_D"], res["inverse_on_D"] = inv_h, fwd_d, inv_d
    r1_tr = 3 * inv_h["median_ms"]  # (the inverse transform on X, of four elements, is not counted)
    s1_tr = 2 * inv_h["median_ms"] + 5 * fwd_d["median_ms"] + inv_d["median_ms"]
    res["round1_transform_share"] = round(r1_tr / res["round1"]["median_ms"], 3)
    res["sumcheck1_transform_share"] = round(s1_tr / res["sumcheck1"]["median_ms"], 3)
    res["bytes_of_one_D_vector"] = d_n * L * 8
    for x in (x_hat, z_poly, w, w_rem, za_poly, zb_poly, t_poly, h1, g1, sigma, big):
        x.free()
    return res


def bench_field(ctx, field, log_h, reps):
    h_n = 1 << log_h
    res = {"field": field, "bits": 298 if field < 2 else 753, "H": h_n, "zm_evals": []}
    res["sumcheck1_q"] = bench_q(ctx, field, capi.lib().pcdhip_domain_size(field, 3 * h_n), reps)
    for shape in ("witness", "skewed"):
        zm, r, mats, zbuf = bench_zm(ctx, field, log_h, reps, shape)
        res["zm_evals"].append(zm)
        if shape == "witness":
            res["drivers"] = bench_drivers(ctx, field, log_h, reps, r, mats, zbuf)
        zbuf.free()
        mats.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-h", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fields", default="1,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marlin_round1_bench.json"))
    a = ap.parse_args()
    ctx = capi.Context(0)
    res = {"tool": "marlin_round1_bench", "reps": a.reps, "results": []}
    for f in a.fields.split(","):
        res["results"].append(bench_field(ctx, int(f), a.log_h, a.reps))
        print(json.dumps(res["results"][-1]), flush=True)
    ctx.close()
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
