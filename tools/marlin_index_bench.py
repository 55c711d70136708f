"""Measurement of K10 (the Marlin index on device) on the shapes of tools/marlin_rounds_bench.py -- coracle.witness_r1cs and
coracle.skewed_r1cs at 2^log_h - 8 constraints (|H| = 2^log_h variables), over the 298-bit and the 753-bit scalar field (fields 1 and
3).  Per shape, medians of REPS after one warm-up:

  the parts of pcdhip_marlin_index_build from the events the build records on the context's stream (pcdhip_marlin_index_timings):
      the arithmetisation launch, the 12 inverse transforms on K, the 12 extensions to B;
  the whole build between pcdhip_timer_start / stop (host work of the call included: the order check, the upload of the CSRs);
  pcdhip_marlin_index_commit over placeholder powers (random points: an MSM's time does not depend on which);
  beside them, in the same run: a pcdhip_vec_mul over |K| elements -- the streaming yardstick for the arithmetisation's gather -- and
      12 plain inverse transforms of |K| elements called one by one (pcdhip_fft_general_dev), the composition the build replaces.

|B| follows the library's rule unless --log-k-cap caps |K| (the entries beyond the cap are dropped from every matrix, row by row):
what to use when |B| at the full size does not fit the device.

    python tools/marlin_index_bench.py [--log-h 20] [--reps 7] [--fields 1,3] [--log-k-cap 0] [--out profiles/marlin_index_bench.json]"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oracle import coracle as co  # noqa: E402
from pcd_amd import capi  # noqa: E402

NUM_INPUTS = 4
LIMBS = [5, 5, 12, 12]


def timed(ctx, fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return round(statistics.median(ts), 4)


def capped(r, cap):
    """the constraint system with every matrix cut to its first `cap` entries (whole rows stay rows: the row pointers are clamped)"""
    out = SimpleNamespace(num_vars=r.num_vars)
    for k in "abc":
        rp = np.minimum(getattr(r, "rp_" + k), np.uint64(cap)).astype(np.uint64)
        n = int(rp[-1])
        setattr(out, "rp_" + k, rp)
        setattr(out, "col_" + k, np.ascontiguousarray(getattr(r, "col_" + k)[:n]))
        setattr(out, "coeff_" + k, np.ascontiguousarray(getattr(r, "coeff_" + k)[:n]))
    return out


def bench_shape(ctx, field, log_h, reps, shape, log_k_cap):
    h_n = 1 << log_h
    nc = h_n - NUM_INPUTS - 4  # num_vars = nc + num_inputs + 4 = |H|
    r = (co.witness_r1cs if shape == "witness" else co.skewed_r1cs)(field, nc, NUM_INPUTS, seed=150)
    assert r.num_vars == h_n
    if log_k_cap:
        r = capped(r, 1 << log_k_cap)
    nnz = [int(rp[-1]) for rp in (r.rp_a, r.rp_b, r.rp_c)]
    res = {"shape": shape + "_r1cs", "H": h_n, "X": NUM_INPUTS, "nnz": nnz, "k_cap": (1 << log_k_cap) if log_k_cap else None}
    parts = {"arith_ms": [], "inverse_ms": [], "extend_ms": [], "build_ms": []}
    idx = None
    for rep in range(reps + 1):
        if idx is not None:
            idx.free()
        ctx.timer_start()
        idx = ctx.marlin_index_build(field, r, h_n, NUM_INPUTS)
        whole = ctx.timer_stop()
        if rep == 0:
            continue  # warm-up: the transform tables of K and B are made here
        t = idx.timings()
        for k in ("arith_ms", "inverse_ms", "extend_ms"):
            parts[k].append(t[k])
        parts["build_ms"].append(whole)
    info = idx.info()
    res.update(K=info["domain_k_n"], B=info["domain_b_n"], device_bytes=info["device_bytes"])
    for k, v in parts.items():
        res[k] = round(statistics.median(v), 4)
    k_n = info["domain_k_n"]
    # twelve vectors written (and the CSR read) by the arithmetisation
    res["arith_written_GBps"] = round(12 * k_n * LIMBS[field] * 8 / (res["arith_ms"] * 1e-3) / 1e9, 1)
    curve = co.CURVE_FR.index(field)
    ctx.set_precompute(0)
    some = co.gen_points(curve, 1, min(k_n, 1 << 12), seed=7)   # placeholder powers: 4096 random points, repeated
    powers = ctx.bases_upload(curve, 1, np.tile(some, (k_n // some.shape[0], 1)))
    res["index_commit_ms"] = timed(ctx, lambda: idx.commit(powers), reps)
    powers.free()
    ctx.set_precompute(-1)
    # the yardsticks, in the same run
    a, b = idx.vec(1, 0, 0), idx.vec(1, 0, 1)
    out = ctx.buf_alloc(field, k_n)
    res["vec_mul_K_ms"] = timed(ctx, lambda: ctx.vec_mul(a, b, out=out), reps)
    res["arith_over_vec_mul"] = round(res["arith_ms"] / res["vec_mul_K_ms"], 2)

    def twelve():
        for _ in range(12):
            ctx.fft_general_dev(out, n=k_n, inverse=True)
    res["twelve_plain_inverse_ms"] = timed(ctx, twelve, reps)
    res["inverse_over_plain"] = round(res["inverse_ms"] / res["twelve_plain_inverse_ms"], 3)
    res["arith_over_inverse"] = round(res["arith_ms"] / res["inverse_ms"], 3)
    out.free()
    idx.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-h", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fields", default="1,3")
    ap.add_argument("--shapes", default="witness,skewed")
    ap.add_argument("--log-k-cap", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marlin_index_bench.json"))
    a = ap.parse_args()
    ctx = capi.Context(0)
    res = {"tool": "marlin_index_bench", "reps": a.reps, "results": []}
    for f in a.fields.split(","):
        for shape in a.shapes.split(","):
            one = {"field": int(f), "bits": 298 if int(f) < 2 else 753}
            try:
                one.update(bench_shape(ctx, int(f), a.log_h, a.reps, shape, a.log_k_cap))
            except capi.PcdHipError as e:  # e.g. out of memory at |B| = 2^24 over 753 bits: recorded, not hidden
                one.update(shape=shape + "_r1cs", error=str(e))
            res["results"].append(one)
            print(json.dumps(one), flush=True)
    ctx.close()
    with open(a.out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
