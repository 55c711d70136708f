"""Measurement of the short MSM (pcdhip_msm_short_dev) against the bucket pipeline (pcdhip_msm_dev) in the same run: device-event
times (pcdhip_timer_start / stop around each call, warm-up first, median and minimum of REPS) over slices of one resident vector of
2^LOG_N points, uploaded with full copies and with none,

  G1 of MNT4-298 and MNT4-753, G2 of MNT4-298;  n in 1, 2, 4, 16, 64, 256, 1024

then a hiding kzg_open at 2^KZG_LOG_N and kzg_check of 1 and of 16 openings with pcdhip_msm_set_short at 0 and at --short-max.
The crossover of a (group, layout) is the largest measured n at which the short median is at or below the old median.  Every step
runs in a child process of its own under a time limit; a step that fails or runs out of time ends the run.

    python tools/msm_short_bench.py [--log-n 16] [--kzg-log-n 20] [--reps 7] [--short-max 64] [--out FILE.json]
    python tools/msm_short_bench.py --step msm:0:1:-1        (one step, in this process: what the driver starts)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1, 2, 4, 16, 64, 256, 1024)
GROUPS = ((0, 1), (2, 1), (0, 2))   # (curve, group)
LAYOUTS = (-1, 0)                   # set_precompute: full copies, none


def timed(ctx, fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return round(statistics.median(ts), 4), round(min(ts), 4)


def step_msm(curve, group, layout, log_n, reps):
    from oracle import coracle as co
    from pcd_amd import capi
    ctx = capi.Context(0)
    fr = co.CURVE_FR[curve]
    n_vec = 1 << log_n
    ctx.set_precompute(layout)
    B = ctx.bases_upload(curve, group, co.gen_points_mt(curve, group, n_vec, seed=31 + curve, threads=16))
    S = ctx.buf_upload(fr, co.gen_scalars(fr, max(SIZES), seed=32))
    c, W, copies = ctx.bases_info(B)
    r = {"kind": "msm", "curve": co.CURVE_NAMES[curve], "group": group, "layout": "full copies" if layout < 0 else "no copies",
         "vector": n_vec, "window_bits": c, "windows": W, "copies": copies, "rows": []}
    for n in SIZES:
        old_med, old_min = timed(ctx, lambda: ctx.msm(B, S, offset=5, n=n), reps)
        new_med, new_min = timed(ctx, lambda: ctx.msm_short(B, S, offset=5, n=n), reps)
        a = co.to_affine(curve, group, ctx.msm(B, S, offset=5, n=n))
        b = co.to_affine(curve, group, ctx.msm_short(B, S, offset=5, n=n))
        assert a[1][0] == b[1][0] and (a[0] == b[0]).all(), "the two paths disagree"
        r["rows"].append({"n": n, "msm_dev_median_ms": old_med, "msm_dev_min_ms": old_min, "msm_short_median_ms": new_med,
                          "msm_short_min_ms": new_min})
    wins = [row["n"] for row in r["rows"] if row["msm_short_median_ms"] <= row["msm_dev_median_ms"]]
    r["crossover_n"] = max(wins) if wins else 0
    r["short_below_old_min_at_1_and_4"] = all(row["msm_short_median_ms"] < row["msm_dev_min_ms"] for row in r["rows"] if row["n"] in (1, 4))
    B.free()
    S.free()
    ctx.close()
    return r


def step_kzg(curve, log_n, reps, short_max):
    from oracle import coracle as co
    from pcd_amd import capi
    ctx = capi.Context(0)
    fr = co.CURVE_FR[curve]
    n = 1 << log_n
    P = ctx.bases_upload(curve, 1, co.gen_points_mt(curve, 1, n, seed=81 + curve, threads=16))
    G = ctx.bases_upload(curve, 1, co.gen_points(curve, 1, 2, seed=91 + curve))
    p = ctx.buf_upload(fr, co.gen_field(fr, n, seed=100))
    blind = ctx.buf_upload(fr, co.gen_field(fr, 2, seed=120))
    z = co.gen_field(fr, 1, seed=122)[0]
    g, h = co.generator(curve, 1), co.generator(curve, 2)
    r = {"kind": "kzg", "curve": co.CURVE_NAMES[curve], "n": n, "short_max": short_max}
    for s in (0, short_max):
        ctx.msm_set_short(s)
        tag = f"set_short_{s}"
        r[f"kzg_open_hiding_ms/{tag}"] = timed(ctx, lambda: ctx.kzg_open(P, p, z, powers_of_gamma_g=G, blinding=blind), reps)
        for k in (1, 16):
            cs = co.gen_points(curve, 1, k, seed=130)
            ws = co.gen_points(curve, 1, k, seed=131)
            vals = co.gen_field(fr, 3 * k, seed=132)
            rs = co.gen_scalars(fr, k, seed=133)
            rs[0] = 0
            rs[0, 0] = 1
            r[f"kzg_check_{k}_ms/{tag}"] = timed(ctx, lambda: ctx.kzg_check(curve, g, h, h, cs, vals[:k], vals[k:2 * k], ws, gamma_g_xy=g,
                                                                           random_v_mont=vals[2 * k:], randomizers_canonical=rs), reps)
    ctx.msm_set_short(0)
    for b in (p, blind, P, G):
        b.free()
    ctx.close()
    return r


def run_step(step, a):
    parts = step.split(":")
    if parts[0] == "msm":
        return step_msm(int(parts[1]), int(parts[2]), int(parts[3]), a.log_n, a.reps)
    return step_kzg(int(parts[1]), a.kzg_log_n, a.reps, a.short_max)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--kzg-log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--short-max", type=int, default=64)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--steps", default=None, help="comma-separated steps instead of the full list")
    ap.add_argument("--step", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(run_step(a.step, a)))
        return 0
    steps = a.steps.split(",") if a.steps else [f"msm:{c}:{g}:{l}" for c, g in GROUPS for l in LAYOUTS] + ["kzg:0", "kzg:2"]
    res = {"tool": "msm_short_bench", "reps": a.reps, "results": []}
    rc = 0
    for s in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--log-n", str(a.log_n), "--kzg-log-n", str(a.kzg_log_n), "--reps", str(a.reps),
               "--short-max", str(a.short_max)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"step {s}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
            rc = 1
            break
        line = [x for x in out.stdout.splitlines() if x.startswith("RESULT ")]
        if out.returncode != 0 or not line:
            print(f"step {s}: exit {out.returncode}; stopping\n{out.stderr[-2000:]}", file=sys.stderr)
            rc = 1
            break
        res["results"].append(json.loads(line[0][7:]))
        print(f"step {s}: done", file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
