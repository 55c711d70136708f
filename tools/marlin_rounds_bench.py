"""Measurement of K9 (Marlin's AHP rounds 2 and 3) at |H| = 2^log_h and |K| = pcdhip_domain_size(nnz) over the 298-bit and the 753-bit
scalar field (fields 1 and 3): device-event times (pcdhip_timer_start / stop around each call, one warm-up, median of REPS) of

  marlin_t_evals on the matrices of coracle.witness_r1cs and coracle.skewed_r1cs (2^log_h variables), for the segment lengths
      1024 / 4096 / 16384 of the long transposed rows, against the forward mat-vecs of the same matrices (out_ms[0] of
      pcdhip_g16_witness_map_resident, over a key of placeholder points: only its resident matrices take part);
  marlin_sumcheck_ab on 4 |K| elements against the same a and b composed from pcdhip_poly_lincomb and pcdhip_vec_mul calls, both
      outputs compared for equality;
  domain_bivariate_lagrange on H against pcdhip_vec_batch_inverse of the same length.

    python tools/marlin_rounds_bench.py [--log-h 20] [--reps 7] [--fields 1,3] [--out profiles/marlin_rounds_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import kzg_reference as kr  # noqa: E402
from oracle import coracle as co  # noqa: E402
from pcd_amd import capi  # noqa: E402

SEGS = (1024, 4096, 16384)
NUM_INPUTS = 4


def timed(ctx, fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return round(statistics.median(ts), 4)


def placeholder_key(curve, r):
    """a proving key of the right shape whose points are all the point at infinity: pcdhip_g16_witness_map_resident reads its resident
    matrices only"""
    m, ni = r.num_vars, r.num_inputs
    n = co.domain_size(r.field, r.num_constraints + ni)
    w1, w2 = capi.point_limbs(curve, capi.G1), capi.point_limbs(curve, capi.G2)
    z = lambda k, w: np.zeros((k, w), dtype=np.uint64)
    one = lambda k: np.ones(k, dtype=np.uint8)
    arrays = dict(a_query=z(m, w1), b_g1_query=z(m, w1), b_g2_query=z(m, w2), h_query=z(n - 1, w1), l_query=z(m - ni, w1),
                  a_inf=one(m), b_g1_inf=one(m), b_g2_inf=one(m), h_inf=one(n - 1), l_inf=one(m - ni),
                  alpha_g1=np.zeros(w1, dtype=np.uint64), beta_g1=np.zeros(w1, dtype=np.uint64), delta_g1=np.zeros(w1, dtype=np.uint64),
                  beta_g2=np.zeros(w2, dtype=np.uint64), delta_g2=np.zeros(w2, dtype=np.uint64))
    keys = co.Keys(curve, r, arrays)
    keys.domain_size = n
    return keys


def bench_t(ctx, field, log_h, reps, shape):
    h_n = 1 << log_h
    nc = h_n - NUM_INPUTS - 4  # num_vars = nc + num_inputs + 4 = |H|
    r = (co.witness_r1cs if shape == "witness" else co.skewed_r1cs)(field, nc, NUM_INPUTS, seed=150)
    assert r.num_vars == h_n and capi.lib().pcdhip_domain_size(field, r.num_vars) == h_n
    nnz = [int(rp[-1]) for rp in (r.rp_a, r.rp_b, r.rp_c)]
    res = {"shape": shape + "_r1cs", "constraints": nc, "variables": r.num_vars, "nnz": nnz}
    # the yardstick: the three forward mat-vecs of the witness map over the same matrices
    curve = co.CURVE_FR.index(field) if field in (1, 3) else None
    ctx.set_precompute(0)
    keys = placeholder_key(curve, r)
    pk = ctx.g16_pk_upload(keys.host_struct(), curve)
    ctx.g16_pk_set_r1cs(pk, r)
    ctx.witness_map_resident(pk, r, want_h=False)
    fwd = [ctx.witness_map_resident(pk, r, want_h=False)[1]["spmv"] for _ in range(reps)]
    pk.free()
    ctx.set_precompute(-1)
    res["forward_spmv3_ms"] = round(statistics.median(fwd), 4)
    r_alpha = ctx.buf_upload(field, co.gen_field(field, nc, seed=151))
    eta = co.gen_field(field, 3, seed=152)
    out = ctx.buf_alloc(field, h_n)
    first = None
    res["t_evals_ms_by_seg"] = {}
    for seg in SEGS:
        os.environ["PCDHIP_MARLIN_SEG"] = str(seg)
        mats = ctx.marlin_mats_upload(field, r, h_n, NUM_INPUTS)
        info = mats.info()
        assert info["seg_len"] == seg
        res["t_evals_ms_by_seg"][str(seg)] = timed(ctx, lambda: ctx.marlin_t_evals(mats, eta, r_alpha, out=out), reps)
        res.setdefault("segments_by_seg", {})[str(seg)] = info["segments"]
        res["long_outputs"] = info["long_outputs"]
        got = out.download()
        first = got if first is None else first
        assert np.array_equal(got, first), "t differs between segment lengths"
        mats.free()
    del os.environ["PCDHIP_MARLIN_SEG"]
    res["t_evals_over_forward"] = {k: round(v / res["forward_spmv3_ms"], 2) for k, v in res["t_evals_ms_by_seg"].items()}
    r_alpha.free()
    out.free()
    return res, max(nnz)


def bench_sumcheck(ctx, field, k_n, reps):
    L, p = kr.LIMBS[field], kr.MODULI[field]
    n = 4 * k_n
    # twelve distinct random vectors: one from the host, the others its successive powers (made on the device)
    vecs = [ctx.buf_upload(field, co.gen_field(field, n, seed=160))]
    for _ in range(11):
        vecs.append(ctx.vec_mul(vecs[-1], vecs[0]))
    row, col, rc, val = (vecs[3 * j:3 * j + 3] for j in range(4))
    alpha, beta = (kr.to_ints(co, field, co.gen_field(field, 1, seed=s))[0] for s in (170, 171))
    coeff = kr.to_ints(co, field, co.gen_field(field, 3, seed=172))
    mont = lambda xs: kr.to_mont(co, field, xs)
    am, bm, cm = mont([alpha])[0], mont([beta])[0], mont(coeff)
    a, b = ctx.buf_alloc(field, n), ctx.buf_alloc(field, n)
    res = {"elements": n, "K": k_n}
    res["sumcheck_ab_ms"] = timed(ctx, lambda: ctx.marlin_sumcheck_ab(am, bm, cm, row, col, rc, val, a_out=a, b_out=b), reps)
    res["sumcheck_ab_product_form_ms"] = timed(ctx, lambda: ctx.marlin_sumcheck_ab(am, bm, cm, row, col, None, val, a_out=a, b_out=b), reps)
    ctx.marlin_sumcheck_ab(am, bm, cm, row, col, rc, val, a_out=a, b_out=b)
    res["sumcheck_ab_effective_GBps"] = round(14 * n * L * 8 / (res["sumcheck_ab_ms"] * 1e-3) / 1e9, 1)  # twelve vectors read, two written
    # the same a and b from the K7 / K8 calls: d_M by one linear combination each (against a vector of ones), then pointwise products
    ones = ctx.buf_upload(field, np.repeat(mont([1]), n, axis=0))
    d = [ctx.buf_alloc(field, n) for _ in range(3)]
    t = [ctx.buf_alloc(field, n) for _ in range(3)]
    a2, b2 = ctx.buf_alloc(field, n), ctx.buf_alloc(field, n)
    dc = mont([alpha * beta % p, p - alpha, p - beta, 1])

    def composed():
        for m in range(3):
            ctx.poly_lincomb([ones, row[m], col[m], rc[m]], dc, d[m])
        ctx.vec_mul(d[1], d[2], out=t[0])
        ctx.vec_mul(d[0], d[2], out=t[1])
        ctx.vec_mul(d[0], d[1], out=t[2])
        ctx.vec_mul(t[2], d[2], out=b2)
        for m in range(3):
            ctx.vec_mul(val[m], t[m], out=t[m])
        ctx.poly_lincomb(t, cm, a2)
    res["composed_calls"] = 11
    res["composed_ms"] = timed(ctx, composed, reps)
    assert np.array_equal(a.download(), a2.download()) and np.array_equal(b.download(), b2.download()), "composition differs"
    res["outputs_equal"] = True
    res["sumcheck_ab_over_composed"] = round(res["sumcheck_ab_ms"] / res["composed_ms"], 3)
    f = ctx.buf_alloc(field, n)
    res["sumcheck_f_ms"] = timed(ctx, lambda: ctx.marlin_sumcheck_f(am, bm, cm, row, col, rc, val, out=f), reps)
    for x in row + col + rc + val + d + t + [a, b, a2, b2, ones, f]:
        x.free()
    return res


def bench_lagrange(ctx, field, h_n, reps):
    x = co.gen_field(field, 1, seed=180)[0]
    out = ctx.buf_alloc(field, h_n)
    v = ctx.buf_upload(field, co.gen_field(field, h_n, seed=181))
    res = {"n": h_n}
    res["domain_bivariate_lagrange_ms"] = timed(ctx, lambda: ctx.domain_bivariate_lagrange(field, h_n, x, out=out), reps)
    res["vec_batch_inverse_ms"] = timed(ctx, lambda: ctx.vec_batch_inverse(v, scale_mont=x, out=v), reps)
    res["lagrange_over_batch_inverse"] = round(res["domain_bivariate_lagrange_ms"] / res["vec_batch_inverse_ms"], 3)
    out.free()
    v.free()
    return res


def bench_field(ctx, field, log_h, reps):
    res = {"field": field, "bits": 298 if field < 2 else 753, "H": 1 << log_h, "t_evals": []}
    worst = 0
    for shape in ("witness", "skewed"):
        t, nnz = bench_t(ctx, field, log_h, reps, shape)
        res["t_evals"].append(t)
        worst = max(worst, nnz)
    k_n = capi.lib().pcdhip_domain_size(field, worst)
    res["sumcheck"] = bench_sumcheck(ctx, field, k_n, reps)
    res["lagrange"] = bench_lagrange(ctx, field, 1 << log_h, reps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-h", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fields", default="1,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marlin_rounds_bench.json"))
    a = ap.parse_args()
    ctx = capi.Context(0)
    res = {"tool": "marlin_rounds_bench", "reps": a.reps, "results": []}
    for f in a.fields.split(","):
        res["results"].append(bench_field(ctx, int(f), a.log_h, a.reps))
        print(json.dumps(res["results"][-1]), flush=True)
    ctx.close()
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
