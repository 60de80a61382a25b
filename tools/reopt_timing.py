#!/usr/bin/env python3
"""Timing of dlp_session_set_objective: the objective-row rebuild kernel at the
bench geometries, and a warm against a cold re-solve at C2.

    tools/reopt_timing.py [--reps 12] [--skip-c3] [--out-dir profiles/reopt]

Rebuild kernel (HIP events around the one launch, the time dlp_session_set_objective returns;
2 warm-up calls, then --reps calls on the same unchanged tableau; no profiler attached):
  C3  32768 x 32768 on its default path (condensed, K = 64, lookahead) after the bench window's
      1,620 pivots (64 * (5 + 20) + 20), next to the same session's rank-64 pass time
      (dlp_session_update_stats, timing = 1);
  C2  4096 x 4096 (tableau 4097 x 8193) on its default path (condensed, K = 16) after 420
      pivots (16 * (5 + 20) + 20) and at the optimum.
Bytes read = contributing rows x stored width x 8; the share is of 8 TB/s.

End to end at C2: solve c, set_objective(c2 = c (1 + 0.02 u)), run to the optimum (warm); against
a fresh session given c2 before its first pivot and run to the optimum (cold: bit-identical to a
session created with c2, tests/test_gpu_reopt.py).  The two alternate, --e2e-reps times each;
wall time of the re-solve alone (the set_objective call + the run), session creation apart.

Writes reopt.json into --out-dir.  The costs c of a generated problem are read back from a fresh
session's objective row (z_j = -c_j)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402

import distributedlpsolver_amd as dlp   # noqa: E402
from distributedlpsolver_amd import _lib as L   # noqa: E402

HBM_BYTES_PER_S = 8e12


def spread(v):
    s = sorted(v)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1], "n": len(s)}


def perturbed(c, seed):
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, len(c))
    return np.ascontiguousarray(c * (1.0 + 0.02 * u))


def costs_of(sess):
    return -sess.read_rows(sess.rows, 1)[0, :sess.problem.n].copy()


def rebuild_stats(sess, c2, reps):
    """reps timed set_objective(c2) calls on the tableau as it stands (no pivot in between)."""
    basis = sess.result().basis
    rows = int(((basis < sess.problem.n) & (c2[np.minimum(basis, len(c2) - 1)] != 0.0)).sum())
    for _ in range(2):
        sess.set_objective(c2)
    ms = [sess.set_objective(c2) for _ in range(reps)]
    width = sess.storage_ncols + 1
    nbytes = rows * width * 8
    k = spread(ms)
    return {"kernel_ms": k, "kernel_ms_all": ms, "contributing_rows": rows, "stored_width": width,
            "stored_ld": sess.storage_ld, "condensed": sess.condensed, "bytes_read": nbytes,
            "gb_per_s_at_median": nbytes / (k["median"] * 1e-3) / 1e9 if k["median"] > 0 else None,
            "share_of_8tb_s_at_median": nbytes / (k["median"] * 1e-3) / HBM_BYTES_PER_S if k["median"] > 0 else None,
            "waves": -(-width // 64), "row_loads_in_flight_per_lane": 32}


def kernel_at(m, n, seed, K, reps, to_optimum):
    prob = dlp.Problem.random(m, n, seed)
    out = {"m": m, "n": n, "seed": seed}
    with dlp.Session(prob, check_interval=K * 20, timing=1, max_pivots=10**7, log_pivots=0) as s:
        c = costs_of(s)
        c2 = perturbed(c, 7)
        assert s.update_stats()[2] == K, s.update_stats()
        s.run(K * 5)
        s.reset_timings()
        s.run(K * 20)
        launches, ms, _ = s.update_stats()
        s.run(20)
        out.update(K=K, lookahead=s.lookahead(), pivots=s.status()[1], passes_timed=launches,
                   pass_ms_mean=ms / max(launches, 1), defer_form=s.defer_form())
        out["after_bench_window"] = rebuild_stats(s, c2, reps)
        out["after_bench_window"]["rebuild_over_pass"] = \
            out["after_bench_window"]["kernel_ms"]["median"] / out["pass_ms_mean"]
        if to_optimum:
            s.set_objective(c)   # (the generated costs again: the cold optimum of the bench LP)
            st, _ = s.run(10**7)
            assert st == L.OK, st
            out["at_optimum"] = dict(rebuild_stats(s, c2, reps), pivots=s.status()[1])
            out["at_optimum"]["rebuild_over_pass"] = out["at_optimum"]["kernel_ms"]["median"] / out["pass_ms_mean"]
    return out


def end_to_end(m, n, seed, reps):
    prob = dlp.Problem.random(m, n, seed)
    runs = {"warm": [], "cold": []}
    for k in range(reps):
        with dlp.Session(prob, max_pivots=10**7, log_pivots=0) as s:   # warm: solve c, then c2
            c = costs_of(s)
            c2 = perturbed(c, 100 + k)
            st, first = s.run(10**7)
            assert st == L.OK
            t0 = time.perf_counter()
            kms = s.set_objective(c2)
            st, piv = s.run(10**7)
            wall = time.perf_counter() - t0
            assert st == L.OK
            runs["warm"].append({"pivots": piv, "wall_ms": 1e3 * wall, "rebuild_kernel_ms": kms,
                                 "first_solve_pivots": first, "objective": s.result().objective})
        with dlp.Session(prob, max_pivots=10**7, log_pivots=0) as s:   # cold: c2 from the slack basis
            t0 = time.perf_counter()
            s.set_objective(c2)
            st, piv = s.run(10**7)
            wall = time.perf_counter() - t0
            assert st == L.OK
            runs["cold"].append({"pivots": piv, "wall_ms": 1e3 * wall, "objective": s.result().objective})
        w, cd = runs["warm"][-1], runs["cold"][-1]
        w["objective_rel_diff_to_cold"] = abs(w["objective"] - cd["objective"]) / (1.0 + abs(cd["objective"]))
    out = {"m": m, "n": n, "seed": seed, "change": "c2 = c (1 + 0.02 u), u ~ U(-1, 1), a new u per repeat",
           "runs": runs}
    for k, v in runs.items():
        out[k + "_wall_ms"] = spread([r["wall_ms"] for r in v])
        out[k + "_pivots"] = spread([r["pivots"] for r in v])
    return out


def _kernel_lines(name, k):
    out = []
    for where in ("after_bench_window", "at_optimum"):
        if where not in k:
            continue
        r = k[where]
        ms = r["kernel_ms"]
        verdict = "below" if r["rebuild_over_pass"] <= 1.0 else "ABOVE"
        out.append(
            f"- **{name}, {where.replace('_', ' ')}** ({r.get('pivots', k['pivots'])} pivots): "
            f"{r['contributing_rows']} contributing rows x {r['stored_width']} stored columns = "
            f"{r['bytes_read'] / 1e6:.1f} MB read; kernel {ms['min']:.4f} / {ms['median']:.4f} / {ms['max']:.4f} ms "
            f"(min / median / max of {ms['n']}), {r['gb_per_s_at_median']:.0f} GB/s = "
            f"{100 * r['share_of_8tb_s_at_median']:.1f} % of 8 TB/s; the session's rank-{k['K']} pass "
            f"(form {k['defer_form']}, {k['passes_timed']} timed) takes {k['pass_ms_mean']:.3f} ms: the rebuild is "
            f"{verdict} it ({r['rebuild_over_pass']:.3f} x).  Column parallelism: {r['waves']} waves of 64 "
            f"columns, {r['row_loads_in_flight_per_lane']} row loads in flight per lane.")
    return out


def write_readme(report, path):
    lines = ["# Objective-row rebuild (dlp_session_set_objective)", "",
             "Written by `tools/reopt_timing.py` (figures in `reopt.json`).  " + report["method"] + ".", ""]
    if "c3_kernel" in report:
        lines += _kernel_lines("C3 32768 x 32768, condensed, K = 64, lookahead", report["c3_kernel"])
    lines += _kernel_lines("C2 4096 x 4096, condensed, K = 16", report["c2_kernel"])
    ld2 = report["c2_kernel"]["after_bench_window"]["stored_ld"]
    lines += ["", f"The C2 stored tableau (4097 rows of {ld2} doubles, {4097 * ld2 * 8 / 1e6:.0f} MB) is partly "
              "resident in the 256 MiB "
              "Infinity Cache, so its GB/s is not an HBM figure.  Where few rows contribute the kernel is "
              "latency-bound (one dependent add chain per column, a launch of a few microseconds), not "
              "bandwidth-bound: the fold order is fixed by the rule and is not split over rows.", ""]
    e = report["c2_end_to_end"]
    lines += ["End to end at C2 (" + e["change"] + "; warm and cold alternate; wall time of set_objective + "
              "the run to the optimum, session creation apart):", "",
              "| | pivots min / median / max | wall ms min / median / max |", "|---|---|---|"]
    for k in ("warm", "cold"):
        p, w = e[k + "_pivots"], e[k + "_wall_ms"]
        lines.append(f"| {k} | {p['min']} / {p['median']} / {p['max']} | "
                     f"{w['min']:.1f} / {w['median']:.1f} / {w['max']:.1f} |")
    worst = max(r["objective_rel_diff_to_cold"] for r in e["runs"]["warm"])
    lines += ["", f"Warm and cold objectives agree to {worst:.1e} relative."]
    if "bench" in report:
        lines += ["", report["bench"]]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--skip-c3", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "reopt"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    report = {"method": "HIP events around the rebuild launch (dlp_session_set_objective's kernel_ms); "
                        "2 warm-up calls, then --reps calls; no profiler attached",
              "reps": a.reps}
    report["c2_kernel"] = kernel_at(4096, 4096, 2, 16, a.reps, True)
    print(json.dumps({"c2_kernel": {k: v for k, v in report["c2_kernel"].items()}}, default=str)[:2000], flush=True)
    report["c2_end_to_end"] = end_to_end(4096, 4096, 2, a.e2e_reps)
    print(json.dumps({k: v for k, v in report["c2_end_to_end"].items() if k != "runs"}), flush=True)
    if not a.skip_c3:
        report["c3_kernel"] = kernel_at(32768, 32768, 3, 64, a.reps, False)
        print(json.dumps(report["c3_kernel"])[:2000], flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "reopt.json"), "w") as f:
        json.dump(report, f, indent=1)
    write_readme(report, os.path.join(a.out_dir, "README.md"))


if __name__ == "__main__":
    main()
