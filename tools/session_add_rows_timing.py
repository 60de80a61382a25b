#!/usr/bin/env python3
"""Timing of dlp_session_add_rows: constraint rows added to a cold-solved C2-shaped
session and the warm dual re-solve, against a cold solve of the stacked LP.

    tools/session_add_rows_timing.py [--reps 3] [--out-dir profiles/session_add_rows]

Workload: the C2 bench LP, 4096 x 4096, generated on the device (seed 2), on the default path of
that size (defer = 16, condensed).  Each repeat runs in a child process of its own (a fresh HIP
context, no buffer-pool carry-over):
  warm  the session solves the LP cold, then add_rows(G, h) + run to the end: the call's kernel time
        (grow copy + row fold together), its wall time (the read-backs, the allocation and the
        uploads included), the dual pivots and the run's wall time; then the call once more with
        slack rows, whose kernel time has no first-launch code load in it;
  cold  a default-options session of the stacked LP [A; G], [b; h] given densely, run to the
        optimum: pivots and wall time of the run, session creation apart.  A, b and c are read
        back from a fresh session's tableau.
The rows: tests/rows_ref.py's cuts at the session's x*, G ~ U[0, 1) with 30 % zeros, h = (G x*)(1 -
depth u); r in --rows, depth in --depths, a new seed per repeat; and "slack" rows, h = 2 G x*, which
need no pivot: the floor of the call.  The two kernels are also set against a hipMemcpyDtoDAsync of
the old tableau's bytes timed in the same process; the fold reads R x width x 8 B per group of 4 rows.
Writes session_add_rows.json with every run and min / median / max per case; prints one summary
line per case."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

M, N_STRUCT, SEED = 4096, 4096, 2
RT = 4   # kFoldRT of dlp_addrows.hip


def spread(v):
    s = sorted(v)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1], "n": len(s)}


def child(r, depth, rep, cold=True):
    import numpy as np
    import rows_ref as AR
    from session_set_defer_timing import copy_ms
    import distributedlpsolver_amd as dlp
    from distributedlpsolver_amd import _lib as L

    m, n = M, N_STRUCT
    prob = dlp.Problem.random(m, n, SEED)
    out = {"r": r, "depth": depth, "rep": rep}
    with dlp.Session(prob, small_lp=-1, max_pivots=10**7, log_pivots=0) as s:
        out["path"] = {"K": s.get_defer_tuning()[2], "condensed": s.condensed, "lookahead": s.lookahead()}
        T = s.tableau()
        A = np.ascontiguousarray(T[:m, :n])
        b = T[:m, n + m].copy()
        c = -T[m, :n].copy()
        del T
        t0 = time.perf_counter()
        st, first = s.run(10**7)
        out["first_cold_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        assert st == L.OK, st
        out["first_cold_pivots"] = first
        res = s.result()
        x = res.x
        G, h = AR.cuts(x, n, r, 7800 + 100 * rep + r, depth=abs(depth))
        if depth < 0:   # slack rows: the floor
            h = 2.0 * (G @ x)
        R = int(sum(1 for v in res.basis if v < n and (G[:, v] != 0.0).any()))
        old_bytes = (m + 1) * s.storage_ld * 8
        width = s.storage_ld
        t0 = time.perf_counter()
        kms = s.add_rows(G, h)
        t1 = time.perf_counter()
        st, piv = s.run(10**7)
        t2 = time.perf_counter()
        assert s.m == m + r and s.get_defer_tuning()[2] == out["path"]["K"]
        objective = s.result().objective
        # the same call again (slack rows at the new optimum): both kernels are loaded by now, so this
        # is their device time without the first launch's code-object load between the two events
        kms2 = None
        if st == L.OK:
            x2 = s.result().x
            G2, _ = AR.cuts(x2, n, r, 7900 + 100 * rep + r)
            kms2 = s.add_rows(G2, 2.0 * (G2 @ x2))
            assert s.run(10**7) == (L.OK, 0)
        cms = copy_ms(old_bytes)
        out["warm"] = {"status": st, "dual_pivots": piv, "kernel_ms": kms, "add_rows_wall_ms": 1e3 * (t1 - t0),
                       "run_wall_ms": 1e3 * (t2 - t1), "wall_ms": 1e3 * (t2 - t0), "objective": objective,
                       "kernel_ms_second_call": kms2, "contributing_rows": R, "old_tableau_bytes": old_bytes,
                       "fold_read_bytes": R * width * 8 * ((r + RT - 1) // RT),
                       "copy_ms": cms, "kernel_ms_over_copy_ms": kms / cms}
    if cold:
        with dlp.Session(dlp.Problem.dense(np.vstack([A, G]), np.r_[b, h], c), max_pivots=10**7, log_pivots=0) as s:
            out["cold_defer"] = s.get_defer_tuning()[2]
            t0 = time.perf_counter()
            st, piv = s.run(10**7)
            wall = time.perf_counter() - t0
            out["cold"] = {"status": st, "pivots": piv, "wall_ms": 1e3 * wall, "objective": s.result().objective}
        w, cd = out["warm"], out["cold"]
        w["objective_rel_diff_to_cold"] = abs(w["objective"] - cd["objective"]) / (1.0 + abs(cd["objective"]))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--depths", type=float, nargs="+", default=[0.02, 0.1],
                    help="cut depths; the slack rows (no pivot) are always run besides")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "session_add_rows"))
    ap.add_argument("--no-cold", action="store_true", help="leave the cold solve of the stacked LP out")
    ap.add_argument("--child", nargs=3, metavar=("R", "DEPTH", "REP"), default=None)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), float(a.child[1]), int(a.child[2]), not a.no_cold)
        return
    report = {"workload": f"C2: {M} x {N_STRUCT} (+{M} slack), device-generated, seed {SEED}, default path",
              "rows": "rows_ref.cuts at x*: G ~ U[0, 1) with 30 % zeros, h = (G x*)(1 - depth u); depth < 0: "
                      "slack rows h = 2 G x*",
              "method": "one child process per repeat; warm = add_rows + run on the session that solved the LP; "
                        "cold = run of a default-options session created with the stacked LP (creation apart); "
                        "wall time; kernel_ms = both kernels of the call by device events; copy_ms = "
                        "hipMemcpyDtoDAsync of the old tableau's bytes in the same process",
              "cases": {}}
    for r in a.rows:
        for depth in [-1.0] + list(a.depths):
            runs = []
            for rep in range(a.reps):
                slack = depth < 0
                p = subprocess.run([sys.executable, os.path.abspath(__file__),
                                    *(["--no-cold"] if (a.no_cold or slack) else []),
                                    "--child", str(r), str(depth), str(rep)],
                                   capture_output=True, text=True, timeout=900)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                    raise SystemExit(f"child (r {r}, depth {depth}, repeat {rep}) failed with status {p.returncode}")
                runs.append(json.loads(line[-1][len("RESULT "):]))
            w = [x["warm"] for x in runs]
            e = {"runs": runs,
                 "kernel_ms": spread([x["kernel_ms"] for x in w]),
                 "kernel_ms_second_call": spread([x["kernel_ms_second_call"] for x in w
                                                  if x["kernel_ms_second_call"] is not None] or [float("nan")]),
                 "copy_ms": spread([x["copy_ms"] for x in w]),
                 "add_rows_wall_ms": spread([x["add_rows_wall_ms"] for x in w]),
                 "run_wall_ms": spread([x["run_wall_ms"] for x in w]),
                 "warm_wall_ms": spread([x["wall_ms"] for x in w]),
                 "dual_pivots": spread([x["dual_pivots"] for x in w]),
                 "contributing_rows": spread([x["contributing_rows"] for x in w]),
                 "first_cold_wall_ms": spread([x["first_cold_wall_ms"] for x in runs]),
                 "first_cold_pivots": spread([x["first_cold_pivots"] for x in runs]),
                 "warm_statuses": sorted({x["status"] for x in w})}
            if "cold" in runs[0]:
                e["cold_wall_ms"] = spread([x["cold"]["wall_ms"] for x in runs])
                e["cold_pivots"] = spread([x["cold"]["pivots"] for x in runs])
                e["objective_rel_diff_max"] = max(x["objective_rel_diff_to_cold"] for x in w)
                e["warm_over_cold_wall_at_median"] = e["warm_wall_ms"]["median"] / e["cold_wall_ms"]["median"]
            key = f"r{r}_" + ("slack" if depth < 0 else f"depth{depth}")
            report["cases"][key] = e
            print(json.dumps({"case": key, **{k: v for k, v in e.items() if k != "runs"}}), flush=True)
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, "session_add_rows.json"), "w") as f:
                json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
