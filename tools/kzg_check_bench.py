"""Measurement of K14, pcdhip_kzg_check_combinations, on the shape of a Marlin proof's opening round on MNT4-298 and MNT4-753: 21
commitments, two of them with a degree bound, 2 points, the collapse of test_gpu_kzg_check.py::test_marlin_shaped_round, valid openings
on a setup that keeps its trapdoor -- in combined mode (one verdict) and in per-opening mode (one per point).

Beside it, in the same process and sample by sample:
  * pcdhip_kzg_check of the parent commit on the P = 2 commitments PRE-COMBINED on the host (the oracle's MSM, not timed, no degree
    bounds: LESS work than the new call does), under the default and under pcdhip_msm_set_short(1024);
  * pcdhip_groth16_verify_prepared of one proof of a small circuit, for scale.
Wall clock around each call (the old path's cost is host waits, which device events do not see), one warm-up, median of REPS with the
smallest and the largest.  "faster" is claimed only when the new call's slowest sample is below the other's fastest.

    python tools/kzg_check_bench.py [--reps 7] [--curves 0,2] [--out profiles/kzg_check_bench.json]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import kzg_batch_open_reference as kb  # noqa: E402
import kzg_check_reference as kk  # noqa: E402
import kzg_commit_reference as kc  # noqa: E402
import kzg_reference as kr  # noqa: E402
from oracle import coracle as co  # noqa: E402
from pcd_amd import capi  # noqa: E402


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def bench_curve(ctx, curve, reps):
    srs = kc.Srs(co, curve, 1, seed=1470 + curve)
    fr, p, rnd = srs.fr, srs.p, random.Random(1471 + curve)
    L = kr.LIMBS[fr]
    r = lambda: rnd.randrange(2, p)
    m, P = 21, 2
    lcs = [dict(terms=[(1, 4)], bound=True), dict(terms=[(1, 15)], bound=True),
           dict(terms=[(r(), i) for i in (0, 1, 2, 3, 5, 6)] + [(p - 1, 7)]),
           dict(terms=[(r(), i) for i in range(8, 21)] + [(r(), 4)]),
           dict(terms=[(1, 8)]), dict(terms=[(r(), 9), (r(), 10)])]
    queries = [(0, 0), (2, 0), (4, 0), (1, 1), (3, 1), (5, 1)]
    a, s = kb.collapse(lcs, queries, [(r(), r()) for _ in queries], m, P, p)
    shift_index = [0 if i == 4 else 1 if i == 15 else -1 for i in range(m)]
    shift_exps, comm = [r(), r()], [r() for _ in range(m)]
    shifted = [r() if shift_index[i] >= 0 else 0 for i in range(m)]
    points, values, rvs = [r(), r()], [r(), r()], [r(), r()]
    iv = [[r() if s[o][i] else 0 for i in range(m)] for o in range(P)]
    rho = [1, r()]

    def witnesses(s_rows):
        out = []
        for o in range(P):
            c = kk.combined_exponent(srs, shift_exps, comm, shifted, shift_index, a[o], None if s_rows is None else s_rows[o], iv[o])
            out.append(kk.solve_witness(srs, c, values[o], rvs[o], points[o]))
        return out

    pts = lambda exps: np.stack([srs.exponent_times_g(co, e)[0] for e in exps])
    flags = lambda exps: np.array([1 if e % p == 0 else 0 for e in exps], dtype=np.uint8)
    mont = lambda rows: np.stack([kr.to_mont(co, fr, row) for row in rows])
    cxy, sxy, w, w_plain = pts(comm), pts(shifted), pts(witnesses(s)), pts(witnesses(None))
    vk = ctx.kzg_vk_prepare(curve, srs.g, srs.h, srs.beta_h, gamma_g_xy=srs.gamma_g, shift_powers_xy=pts(shift_exps))
    tables = dict(points_mont=kr.to_mont(co, fr, points), coeffs_mont=mont(a), values_mont=kr.to_mont(co, fr, values), shifted_coeffs_mont=mont(s),
                  random_v_mont=kr.to_mont(co, fr, rvs), item_values_mont=mont(iv), shift_index=np.array(shift_index, dtype=np.int32))
    rho_c = kr.limbs_of_ints(rho, L)

    def new_combined():
        return ctx.kzg_check_combinations(vk, cxy, w_xy=w, shifted_xy=sxy, shifted_inf=flags(shifted), randomizers_canonical=rho_c, **tables)

    def new_each():
        return ctx.kzg_check_combinations(vk, cxy, w_xy=w, shifted_xy=sxy, shifted_inf=flags(shifted), **tables)

    combined = np.stack([co.to_affine(curve, 1, co.msm(curve, 1, cxy, kr.limbs_of_ints(a[o], L), nthreads=4))[0][0] for o in range(P)])

    def old_check():
        return ctx.kzg_check(curve, srs.g, srs.h, srs.beta_h, combined, tables["points_mont"], tables["values_mont"], w_plain,
                             gamma_g_xy=srs.gamma_g, random_v_mont=tables["random_v_mont"], randomizers_canonical=rho_c)

    def old_check_short():
        ctx.msm_set_short(1024)
        try:
            return old_check()
        finally:
            ctx.msm_set_short(0)

    # a prepared Groth16 verification of one proof, for scale
    r1 = co.synthetic_r1cs(fr, 60, 3, seed=50 + curve)
    keys = co.groth16_setup(curve, r1, co.gen_field(fr, 5, seed=51), nthreads=16)
    pk = ctx.g16_pk_upload(keys.host_struct(), curve)
    proof = np.stack([ctx.groth16_prove(pk, r1, *co.gen_field(fr, 2, seed=60))[0]])
    pk.free()
    pub = np.stack([co.fp_op(fr, "to_canonical", np.ascontiguousarray(r1.z[1:r1.num_inputs]))])
    pvk = ctx.process_vk(curve, keys.alpha_g1, keys.beta_g2, keys.gamma_g2, keys.delta_g2, keys.gamma_abc_g1)

    def g16_verify():
        return bool(ctx.groth16_verify_prepared(pvk, pub, proof).all())

    calls = (("check_combined", new_combined), ("check_per_opening", new_each), ("parent_kzg_check", old_check),
             ("parent_kzg_check_short1024", old_check_short), ("groth16_verify_prepared", g16_verify))
    # verdicts first
    assert new_combined() is True and new_each() == [True, True] and old_check() is True and old_check_short() is True and g16_verify()
    plans = {}
    samples = {name: [] for name, _ in calls}
    for rep in range(reps + 1):  # (the first round is the warm-up of all)
        for name, fn in calls:
            t = time.perf_counter()
            fn()
            wall = (time.perf_counter() - t) * 1e3
            if rep:
                samples[name].append(wall)
            if name.startswith("check_"):
                plans[name] = list(ctx.kzg_check_combinations_last_plan())
    res = {"curve": co.CURVE_NAMES[curve], "items": m, "degree_bounds": 2, "points": P, "plans": plans}
    for name, xs in samples.items():
        res[name + "_wall_ms"] = stats(xs)
    for other in ("parent_kzg_check", "parent_kzg_check_short1024"):
        res["combined_faster_than_" + other] = bool(max(samples["check_combined"]) < min(samples[other]))
    vk.free()
    pvk.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--curves", default="0,2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = capi.Context(0)
    res = {"tool": "kzg_check_bench", "reps": a.reps, "results": [bench_curve(ctx, int(c), a.reps) for c in a.curves.split(",")]}
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
