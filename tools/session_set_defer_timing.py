#!/usr/bin/env python3
"""Timing of dlp_session_set_defer: the round trip cold-deferred -> eager dual phase
-> deferred again on a C2-shaped LP, against §21's eager-first route and a cold solve of the new b;
and the two relayout kernels against a device-to-device copy.

    tools/session_set_defer_timing.py [--reps 3] [--scales 0.02 0.1] [--c3] [--out-dir profiles/session_set_defer]

Workload: the C2 bench LP, 4096 x 4096 (full tableau 4097 x 8193), generated on the device (seed 2).
Each repeat runs in a child process of its own (a fresh HIP context, no buffer-pool carry-over):
  switch  a default-options session (deferred, condensed) solves b cold; set_defer(1); set_rhs(b2) +
          run to the end; set_defer(0) back.  Wall time of each of the four and their sum; the
          relayout kernels' device time;
  eager   §21's route: a defer = 1 session solves b cold, then set_rhs(b2) + run (first solve included);
  cold    a default-options session created with b2, run to the optimum (creation apart).
b2 = b (1 + s u), u ~ U(-1, 1), a new u per repeat, s from --scales.
Relayout rate: kernel ms of the expand (condensed -> full) and the pack (full -> condensed) from the
switch route, bytes = source read + destination written; the yardstick is a device-to-device copy of
the destination's byte count in the same process (it reads and writes that count).  --c3 adds one
child at the C3 shape (32768 x 32768, seed 3; 256 pivots, no solve): expand, pack and the copy.
Writes session_set_defer.json with every run and min / median / max; prints one line per scale."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C2 = (4096, 4096, 2)
C3 = (32768, 32768, 3)


def spread(v):
    s = sorted(v)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1], "n": len(s)}


def copy_ms(nbytes, reps=5):
    """hipMemcpyDtoD of nbytes in this process (the HIP runtime libdlp.so runs on), best of reps, by
    device events."""
    import ctypes as C
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with hipError {rc}")

    src, dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipMalloc(C.byref(src), C.c_size_t(nbytes)), "hipMalloc")
    ok(hip.hipMalloc(C.byref(dst), C.c_size_t(nbytes)), "hipMalloc")
    ok(hip.hipMemset(src, 0, C.c_size_t(nbytes)), "hipMemset")
    ok(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    best = None
    for _ in range(reps + 1):   # (the first one warms up)
        ok(hip.hipEventRecord(e0, None), "hipEventRecord")
        ok(hip.hipMemcpyDtoDAsync(dst, src, C.c_size_t(nbytes), None), "hipMemcpyDtoDAsync")
        ok(hip.hipEventRecord(e1, None), "hipEventRecord")
        ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        if _ > 0:
            best = ms.value if best is None else min(best, ms.value)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    for p in (src, dst):
        hip.hipFree(p)
    return best


def rate(kernel_ms, src_bytes, dst_bytes):
    cms = copy_ms(dst_bytes)
    return {"kernel_ms": kernel_ms, "src_bytes": src_bytes, "dst_bytes": dst_bytes,
            "kernel_gbs": (src_bytes + dst_bytes) / kernel_ms / 1e6,
            "copy_ms": cms, "copy_gbs": 2 * dst_bytes / cms / 1e6,
            "kernel_ms_over_copy_ms": kernel_ms / cms}


def child_c3():
    import distributedlpsolver_amd as dlp
    from distributedlpsolver_amd import _lib as L
    m, n, seed = C3
    out = {"shape": [m, n]}
    with dlp.Session(dlp.Problem.random(m, n, seed), max_pivots=10**7, log_pivots=0) as s:
        out["path"] = {"K": s.get_defer_tuning()[2], "condensed": s.condensed, "lookahead": s.lookahead()}
        assert s.run(256) == (L.RUNNING, 256)
        cond_bytes = (m + 1) * s.storage_ld * 8
        t0 = time.perf_counter()
        ems = s.set_defer(1)
        out["to_eager_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        full_bytes = (m + 1) * s.storage_ld * 8
        t0 = time.perf_counter()
        pms = s.set_defer(0)
        out["back_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        assert s.condensed and ems > 0 and pms > 0
        assert s.run(256) == (L.RUNNING, 256)
    out["expand"] = rate(ems, cond_bytes, full_bytes)
    out["pack"] = rate(pms, full_bytes, cond_bytes)
    print("RESULT " + json.dumps(out), flush=True)


def child(scale, rep):
    import numpy as np
    import distributedlpsolver_amd as dlp
    from distributedlpsolver_amd import _lib as L

    m, n, seed = C2
    prob = dlp.Problem.random(m, n, seed)
    out = {"scale": scale, "rep": rep}
    u = np.random.default_rng(1000 * rep + int(round(scale * 1000))).uniform(-1.0, 1.0, m)
    # ---- the switch route
    with dlp.Session(prob, max_pivots=10**7, log_pivots=0) as s:
        T = s.tableau()
        A = np.ascontiguousarray(T[:m, :n])
        b = T[:m, n + m].copy()
        c = -T[m, :n].copy()
        del T
        b2 = np.ascontiguousarray(b * (1.0 + scale * u))
        sw = {"path": {"K": s.get_defer_tuning()[2], "condensed": s.condensed, "lookahead": s.lookahead()}}
        t0 = time.perf_counter()
        st, piv = s.run(10**7)
        t1 = time.perf_counter()
        assert st == L.OK, st
        cond_bytes = (m + 1) * s.storage_ld * 8
        ems = s.set_defer(1)
        t2 = time.perf_counter()
        full_bytes = (m + 1) * s.storage_ld * 8
        rms = s.set_rhs(b2)
        st, dpiv = s.run(10**7)
        t3 = time.perf_counter()
        pms = s.set_defer(0)
        t4 = time.perf_counter()
        assert s.condensed == sw["path"]["condensed"] and s.get_defer_tuning()[2] == sw["path"]["K"]
        sw.update({"cold_wall_ms": 1e3 * (t1 - t0), "cold_pivots": piv,
                   "to_eager_wall_ms": 1e3 * (t2 - t1), "expand_kernel_ms": ems,
                   "dual_wall_ms": 1e3 * (t3 - t2), "dual_pivots": dpiv, "dual_status": st, "rebuild_kernel_ms": rms,
                   "back_wall_ms": 1e3 * (t4 - t3), "pack_kernel_ms": pms,
                   "sum_wall_ms": 1e3 * (t4 - t0), "resolve_wall_ms": 1e3 * (t4 - t1),
                   "objective": s.result().objective})
        out["switch"] = sw
    out["expand"] = rate(ems, cond_bytes, full_bytes)
    out["pack"] = rate(pms, full_bytes, cond_bytes)
    # ---- §21's route: eager from the start
    with dlp.Session(prob, defer=1, small_lp=-1, max_pivots=10**7, log_pivots=0) as s:
        t0 = time.perf_counter()
        st, piv = s.run(10**7)
        t1 = time.perf_counter()
        assert st == L.OK, st
        s.set_rhs(b2)
        st, dpiv = s.run(10**7)
        t2 = time.perf_counter()
        out["eager"] = {"cold_wall_ms": 1e3 * (t1 - t0), "cold_pivots": piv, "dual_wall_ms": 1e3 * (t2 - t1),
                        "dual_pivots": dpiv, "dual_status": st, "sum_wall_ms": 1e3 * (t2 - t0),
                        "objective": s.result().objective}
    # ---- a cold default-path solve of b2
    with dlp.Session(dlp.Problem.dense(A, b2, c), max_pivots=10**7, log_pivots=0) as s:
        t0 = time.perf_counter()
        st, piv = s.run(10**7)
        out["cold"] = {"status": st, "pivots": piv, "wall_ms": 1e3 * (time.perf_counter() - t0),
                       "objective": s.result().objective}
    assert out["switch"]["objective"] == out["eager"]["objective"], "the two warm routes differ"
    out["objective_rel_diff_to_cold"] = abs(out["switch"]["objective"] - out["cold"]["objective"]) / \
        (1.0 + abs(out["cold"]["objective"]))
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args, timeout=1100):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", *args],
                       capture_output=True, text=True, timeout=timeout)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit(f"child {args} failed with status {p.returncode}")
    return json.loads(line[-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scales", type=float, nargs="+", default=[0.02, 0.1])
    ap.add_argument("--c3", action="store_true", help="also time the relayout kernels at the C3 shape")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "session_set_defer"))
    ap.add_argument("--child", nargs="+", metavar="ARG", default=None)
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "c3":
            child_c3()
        else:
            child(float(a.child[0]), int(a.child[1]))
        return
    m, n, seed = C2
    report = {"workload": f"C2: {m} x {n} (+{m} slack), device-generated, seed {seed}",
              "change": "b2 = b (1 + s u), u ~ U(-1, 1), a new u per repeat",
              "method": "one child process per repeat, no profiler; wall time; switch = cold solve on default options, "
                        "set_defer(1), set_rhs + run, set_defer(0); eager = defer = 1 from the start; cold = a "
                        "default-options session created with b2 (creation apart)",
              "scales": {}}
    for scale in a.scales:
        runs = [run_child([str(scale), str(rep)]) for rep in range(a.reps)]
        sw = lambda k: spread([r["switch"][k] for r in runs])
        e = {"runs": runs,
             "switch_cold_wall_ms": sw("cold_wall_ms"), "switch_to_eager_wall_ms": sw("to_eager_wall_ms"),
             "switch_expand_kernel_ms": sw("expand_kernel_ms"), "switch_dual_wall_ms": sw("dual_wall_ms"),
             "switch_dual_pivots": sw("dual_pivots"), "switch_back_wall_ms": sw("back_wall_ms"),
             "switch_pack_kernel_ms": sw("pack_kernel_ms"), "switch_sum_wall_ms": sw("sum_wall_ms"),
             "switch_resolve_wall_ms": sw("resolve_wall_ms"),
             "eager_cold_wall_ms": spread([r["eager"]["cold_wall_ms"] for r in runs]),
             "eager_dual_wall_ms": spread([r["eager"]["dual_wall_ms"] for r in runs]),
             "eager_sum_wall_ms": spread([r["eager"]["sum_wall_ms"] for r in runs]),
             "cold_wall_ms": spread([r["cold"]["wall_ms"] for r in runs]),
             "expand_gbs": spread([r["expand"]["kernel_gbs"] for r in runs]),
             "pack_gbs": spread([r["pack"]["kernel_gbs"] for r in runs]),
             "expand_ms_over_copy_ms": spread([r["expand"]["kernel_ms_over_copy_ms"] for r in runs]),
             "pack_ms_over_copy_ms": spread([r["pack"]["kernel_ms_over_copy_ms"] for r in runs]),
             "objective_rel_diff_max": max(r["objective_rel_diff_to_cold"] for r in runs)}
        report["scales"][str(scale)] = e
        print(json.dumps({"scale": scale, **{k: v for k, v in e.items() if k != "runs"}}), flush=True)
    if a.c3:
        report["c3_relayout"] = run_child(["c3"])
        print(json.dumps({"c3_relayout": report["c3_relayout"]}), flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "session_set_defer.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
