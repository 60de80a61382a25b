#!/usr/bin/env python3
"""Timing of dlp_session_set_rhs: a warm dual re-solve of a C2-shaped LP after its
right-hand sides moved, against a cold solve of the same new b.

    tools/session_rhs_timing.py [--reps 3] [--scales 0.02 0.1] [--out-dir profiles/session_rhs]

Workload: the C2 bench LP, 4096 x 4096 (tableau 4097 x 8193), generated on the device (seed 2).
Each repeat runs in a child process of its own (a fresh HIP context, no buffer-pool carry-over):
  warm  a defer = 1 session solves b cold (the only path dlp_session_set_rhs accepts at this
        size), then set_rhs(b2) + run to the end: wall time of those two calls, the dual pivots,
        the rebuild kernel's device time;
  cold  a default-options session (the deferred path: what a caller would otherwise run) of the
        same LP given densely with b2, run to the optimum: wall time of the run, session creation
        apart.  A and c are read back from a fresh session's tableau.
b2 = b (1 + s u), u ~ U(-1, 1), a new u per repeat, s from --scales.  Writes session_rhs.json with
every run and min / median / max per scale; prints one summary line per scale.

--route picks how the warm re-solve runs; the default is the eager route above:
  eager     a defer = 1 session from the start, set_rhs + run;
  in_place  a defer = 16, condensed session solves b cold and stays on its path:
            set_rhs(b2, in_place=True) + run (dlp_session_set_rhs_in_place);
  switch    the same session through DESIGN.md §22's route: set_defer(1), set_rhs + run,
            set_defer(16, condensed) back; the wall time covers all four calls.
The same (scale, repeat) gives the same b2 on every route, so their dual pivot counts must agree.
--no-cold leaves the cold solve of b2 out (a comparison of two routes needs it once)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M, N_STRUCT, SEED = 4096, 4096, 2


def spread(v):
    s = sorted(v)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1], "n": len(s)}


DEFER_PATH = dict(defer=16, condensed=1)


def child(scale, rep, route="eager", cold=True):
    import numpy as np
    import distributedlpsolver_amd as dlp
    from distributedlpsolver_amd import _lib as L

    m, n = M, N_STRUCT
    prob = dlp.Problem.random(m, n, SEED)
    out = {"scale": scale, "rep": rep, "route": route}
    path = dict(defer=1) if route == "eager" else DEFER_PATH
    with dlp.Session(prob, small_lp=-1, max_pivots=10**7, log_pivots=0, **path) as s:
        T = s.tableau()
        A = np.ascontiguousarray(T[:m, :n])
        b = T[:m, n + m].copy()
        c = -T[m, :n].copy()
        del T
        u = np.random.default_rng(1000 * rep + int(round(scale * 1000))).uniform(-1.0, 1.0, m)
        b2 = np.ascontiguousarray(b * (1.0 + scale * u))
        t0 = time.perf_counter()
        st, first = s.run(10**7)
        out["eager_cold_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        assert st == L.OK, st
        out["eager_cold_pivots"] = first
        t0 = time.perf_counter()
        if route == "switch":
            s.set_defer(1)
        kms = s.set_rhs(b2, in_place=(route == "in_place"))
        t1 = time.perf_counter()
        st, piv = s.run(10**7)
        if route == "switch":
            s.set_defer(**DEFER_PATH)
        t2 = time.perf_counter()
        if route != "eager":
            assert s.condensed and s.get_defer_tuning()[2] == DEFER_PATH["defer"]
        out["warm"] = {"status": st, "dual_pivots": piv, "wall_ms": 1e3 * (t2 - t0),
                       "set_rhs_wall_ms": 1e3 * (t1 - t0), "rebuild_kernel_ms": kms,
                       "objective": s.result().objective}
    if cold:
        with dlp.Session(dlp.Problem.dense(A, b2, c), max_pivots=10**7, log_pivots=0) as s:
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
    ap.add_argument("--scales", type=float, nargs="+", default=[0.02, 0.1])
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "session_rhs"))
    ap.add_argument("--route", choices=("eager", "in_place", "switch"), default="eager")
    ap.add_argument("--no-cold", action="store_true", help="leave the cold solve of b2 out")
    ap.add_argument("--child", nargs=2, metavar=("SCALE", "REP"), default=None)
    a = ap.parse_args()
    if a.child:
        child(float(a.child[0]), int(a.child[1]), a.route, not a.no_cold)
        return
    report = {"route": a.route, "workload": f"C2: {M} x {N_STRUCT} (+{M} slack), device-generated, seed {SEED}",
              "change": "b2 = b (1 + s u), u ~ U(-1, 1), a new u per repeat",
              "method": "one child process per repeat; warm = set_rhs + run on the defer = 1 session that solved b; "
                        "cold = run of a default-options session created with b2 (creation apart); wall time",
              "scales": {}}
    for scale in a.scales:
        runs = []
        for rep in range(a.reps):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", a.route,
                                *(["--no-cold"] if a.no_cold else []), "--child", str(scale), str(rep)],
                               capture_output=True, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                raise SystemExit(f"child (scale {scale}, repeat {rep}) failed with status {p.returncode}")
            runs.append(json.loads(line[-1][len("RESULT "):]))
        e = {"runs": runs,
             "warm_wall_ms": spread([r["warm"]["wall_ms"] for r in runs]),
             "warm_dual_pivots": spread([r["warm"]["dual_pivots"] for r in runs]),
             "rebuild_kernel_ms": spread([r["warm"]["rebuild_kernel_ms"] for r in runs]),
             "eager_cold_wall_ms": spread([r["eager_cold_wall_ms"] for r in runs]),
             "warm_statuses": sorted({r["warm"]["status"] for r in runs})}
        e["warm_us_per_dual_pivot_at_median"] = \
            1e3 * e["warm_wall_ms"]["median"] / max(e["warm_dual_pivots"]["median"], 1)
        if not a.no_cold:
            e["cold_wall_ms"] = spread([r["cold"]["wall_ms"] for r in runs])
            e["cold_pivots"] = spread([r["cold"]["pivots"] for r in runs])
            e["objective_rel_diff_max"] = max(r["warm"]["objective_rel_diff_to_cold"] for r in runs)
            e["warm_over_cold_wall_at_median"] = e["warm_wall_ms"]["median"] / e["cold_wall_ms"]["median"]
            e["cold_us_per_pivot_at_median"] = 1e3 * e["cold_wall_ms"]["median"] / max(e["cold_pivots"]["median"], 1)
        report["scales"][str(scale)] = e
        print(json.dumps({"scale": scale, **{k: v for k, v in e.items() if k != "runs"}}), flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    name = "session_rhs.json" if a.route == "eager" else f"session_rhs_{a.route}.json"
    with open(os.path.join(a.out_dir, name), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
