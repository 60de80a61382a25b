#!/usr/bin/env python3
"""Timing of dlp_session_add_cols: variables added to a cold-solved C2-shaped
session and the warm primal re-solve, against a cold solve of the stacked LP.

    tools/session_add_cols_timing.py [--reps 3] [--out-dir profiles/session_add_cols]

Workload: the C2 bench LP, 4096 x 4096, generated on the device (seed 2), on the default path of
that size (defer = 16, condensed).  Each repeat runs in a child process of its own (a fresh HIP
context, no buffer-pool carry-over):
  warm  the session solves the LP cold, then add_cols(P, d) + run to the end: the call's kernel time
        (widening copy + column fold together), its wall time (the read-backs, the allocation and
        the uploads included), the primal pivots and the run's wall time; then the call once more
        with unattractive columns, whose kernel time has no first-launch code load in it; then
        set_rhs(b, in_place) twice with the creation b: the second call's kernel time is one RHS
        rebuild, the same fold for one column (the yardstick of the fold);
  cold  a default-options session of the stacked LP [A | P], [c d] given densely, run to the
        optimum: pivots and wall time of the run, session creation apart.  A, b and c are read
        back from a fresh session's tableau.
The columns: tests/cols_ref.py's columns at the session's y*, P ~ U[0, 1) with 30 % zeros,
d = (y* . P)(1 + depth u); k in --cols (cold solves for --cold-cols only), depth in --depths, a new
seed per repeat; and "dull" columns (depth -0.1: reduced cost > 0), which need no pivot: the floor
of the call.  The two kernels are also set against a hipMemcpyDtoDAsync of the old tableau's bytes
timed in the same process.  Writes session_add_cols.json with every run and min / median / max per
case; prints one summary line per case."""
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
CT = 4   # kColCT of dlp_addcols.hip


def spread(v):
    s = sorted(v)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1], "n": len(s)}


def child(k, depth, rep, cold=True):
    import numpy as np
    import cols_ref as CR
    from session_set_defer_timing import copy_ms
    import distributedlpsolver_amd as dlp
    from distributedlpsolver_amd import _lib as L

    m, n = M, N_STRUCT
    prob = dlp.Problem.random(m, n, SEED)
    out = {"k": k, "depth": depth, "rep": rep}
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
        y = s.result().y
        P, d = CR.columns(y, k, 7700 + 100 * rep + k, depth=depth if depth > 0 else -0.1)
        R = int((P != 0.0).any(axis=1).sum())
        old_bytes = (m + 1) * s.storage_ld * 8
        t0 = time.perf_counter()
        kms = s.add_cols(P, d)
        t1 = time.perf_counter()
        st, piv = s.run(10**7)
        t2 = time.perf_counter()
        assert s.n == n + k and s.get_defer_tuning()[2] == out["path"]["K"]
        objective = s.result().objective
        # the same call again (unattractive columns at the new optimum): both kernels are loaded by now,
        # so this is their device time without the first launch's code-object load between the events
        kms2 = rhs_ms = None
        if st == L.OK:
            P2, d2 = CR.columns(s.result().y, k, 7900 + 100 * rep + k, depth=-0.1)
            kms2 = s.add_cols(P2, d2)
            assert s.run(10**7) == (L.OK, 0)
            # one RHS rebuild on the same session (the creation b: no pivot), second call
            for _ in range(2):
                rhs_ms = s.set_rhs(b, in_place=True)
                assert s.run(10**7)[0] == L.OK
        cms = copy_ms(old_bytes)
        out["warm"] = {"status": st, "primal_pivots": piv, "kernel_ms": kms, "add_cols_wall_ms": 1e3 * (t1 - t0),
                       "run_wall_ms": 1e3 * (t2 - t1), "wall_ms": 1e3 * (t2 - t0), "objective": objective,
                       "kernel_ms_second_call": kms2, "rhs_rebuild_ms": rhs_ms, "contributing_slacks": R,
                       "old_tableau_bytes": old_bytes, "column_groups": (k + CT - 1) // CT,
                       "copy_ms": cms, "kernel_ms_over_copy_ms": kms / cms}
    if cold:
        with dlp.Session(dlp.Problem.dense(np.hstack([A, P]), b, np.r_[c, d]), max_pivots=10**7, log_pivots=0) as s:
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
    ap.add_argument("--cols", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--cold-cols", type=int, nargs="+", default=[1, 16],
                    help="the k that also run the attractive depths and the cold solve of the stacked LP")
    ap.add_argument("--depths", type=float, nargs="+", default=[0.02, 0.1],
                    help="pricing depths; the dull columns (no pivot) are always run besides")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "session_add_cols"))
    ap.add_argument("--no-cold", action="store_true", help="leave the cold solve of the stacked LP out")
    ap.add_argument("--child", nargs=3, metavar=("K", "DEPTH", "REP"), default=None)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), float(a.child[1]), int(a.child[2]), not a.no_cold)
        return
    report = {"workload": f"C2: {M} x {N_STRUCT} (+{M} slack), device-generated, seed {SEED}, default path",
              "columns": "cols_ref.columns at y*: P ~ U[0, 1) with 30 % zeros, d = (y* . P)(1 + depth u); depth < 0: "
                         "dull columns (reduced cost > 0)",
              "method": "one child process per repeat; warm = add_cols + run on the session that solved the LP; "
                        "cold = run of a default-options session created with the stacked LP (creation apart); "
                        "wall time; kernel_ms = both kernels of the call by device events; rhs_rebuild_ms = the "
                        "kernel_ms of the second set_rhs(b, in_place) on the same session; copy_ms = "
                        "hipMemcpyDtoDAsync of the old tableau's bytes in the same process",
              "cases": {}}
    for k in a.cols:
        for depth in [-1.0] + (list(a.depths) if k in a.cold_cols else []):
            runs = []
            for rep in range(a.reps):
                dull = depth < 0
                p = subprocess.run([sys.executable, os.path.abspath(__file__),
                                    *(["--no-cold"] if (a.no_cold or dull) else []),
                                    "--child", str(k), str(depth), str(rep)],
                                   capture_output=True, text=True, timeout=900)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                    raise SystemExit(f"child (k {k}, depth {depth}, repeat {rep}) failed with status {p.returncode}")
                runs.append(json.loads(line[-1][len("RESULT "):]))
            w = [x["warm"] for x in runs]

            def some(key):
                return spread([x[key] for x in w if x[key] is not None] or [float("nan")])
            e = {"runs": runs,
                 "kernel_ms": some("kernel_ms"),
                 "kernel_ms_second_call": some("kernel_ms_second_call"),
                 "rhs_rebuild_ms": some("rhs_rebuild_ms"),
                 "copy_ms": some("copy_ms"),
                 "add_cols_wall_ms": some("add_cols_wall_ms"),
                 "run_wall_ms": some("run_wall_ms"),
                 "warm_wall_ms": some("wall_ms"),
                 "primal_pivots": some("primal_pivots"),
                 "contributing_slacks": some("contributing_slacks"),
                 "first_cold_wall_ms": spread([x["first_cold_wall_ms"] for x in runs]),
                 "first_cold_pivots": spread([x["first_cold_pivots"] for x in runs]),
                 "warm_statuses": sorted({x["status"] for x in w})}
            e["second_call_over_rhs_rebuild_at_median"] = \
                e["kernel_ms_second_call"]["median"] / e["rhs_rebuild_ms"]["median"]
            if "cold" in runs[0]:
                e["cold_wall_ms"] = spread([x["cold"]["wall_ms"] for x in runs])
                e["cold_pivots"] = spread([x["cold"]["pivots"] for x in runs])
                e["objective_rel_diff_max"] = max(x["objective_rel_diff_to_cold"] for x in w)
                e["warm_over_cold_wall_at_median"] = e["warm_wall_ms"]["median"] / e["cold_wall_ms"]["median"]
            key = f"k{k}_" + ("dull" if depth < 0 else f"depth{depth}")
            report["cases"][key] = e
            print(json.dumps({"case": key, **{kk: v for kk, v in e.items() if kk != "runs"}}), flush=True)
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, "session_add_cols.json"), "w") as f:
                json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
