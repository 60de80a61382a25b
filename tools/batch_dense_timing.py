#!/usr/bin/env python3
"""Timing of dlp_batched_solve_dense against the generated batch path ("Batched
solve of caller-supplied LPs"): C5's shapes, 4,096 x (64 x 128) and 4,096 x (64 x 64), the
generator's own LPs handed in as device tensors, so all runs do the same pivots on the same
values and differ only in the prologue loads and the x / y epilogue.

    tools/batch_dense_timing.py [--other-lib PATH/libdlp.so] [--reps 7] [--out FILE.json]

Every measurement runs in a child process of its own, alternating between the libraries:
`generated` children call dlp_batched_solve through plain ctypes (so they also run a library
built from an older commit, --other-lib), the `dense` child goes through the package.  Not a
product file: the LPs come from the test oracle's generator."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIS_LIB = os.path.join(ROOT, "distributedlpsolver_amd", "libdlp.so")
NLP, SEED, WARM = 4096, 5000, 3
SHAPES = ((64, 128), (64, 64))


def child_generated(lib_path, m, n, reps):
    import numpy as np
    lib = C.CDLL(lib_path)
    obj, st, npv, ms = np.zeros(NLP), np.zeros(NLP, np.int32), np.zeros(NLP, np.int64), C.c_double()
    dp = C.POINTER(C.c_double)

    def run():
        rc = lib.dlp_batched_solve(C.c_int(0), C.c_int64(NLP), C.c_int64(m), C.c_int64(n), C.c_uint64(SEED),
                                   None, obj.ctypes.data_as(dp), st.ctypes.data_as(C.c_void_p),
                                   npv.ctypes.data_as(C.c_void_p), None, None, C.c_int64(0), C.byref(ms))
        assert rc == 0, rc
        return ms.value
    for _ in range(WARM):
        run()
    kms = [run() for _ in range(reps)]
    return {"kernel_ms": kms, "pivots": int(npv.sum()), "all_optimal": bool((st == 0).all()),
            "objective_sha256": hashlib.sha256(obj.tobytes()).hexdigest()}


def child_dense(m, n, reps):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import oracle_py as O
    import distributedlpsolver_amd as dlp
    lps = [O.gen_dense(m, n, SEED + k) for k in range(NLP)]
    A, b, c = (np.stack([p[i] for p in lps]) for i in range(3))
    tA, tb, tc = (torch.from_numpy(v).cuda() for v in (A, b, c))
    out = {"input_bytes": int(A.nbytes + b.nbytes + c.nbytes)}
    variants = {"xy": dict(want_x=True, want_y=True), "no_xy": dict(want_x=False, want_y=False)}
    for name, kw in variants.items():
        for _ in range(WARM):
            r = dlp.batched_solve_dense(tA, tb, tc, **kw)
        kms, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = dlp.batched_solve_dense(tA, tb, tc, **kw)
            wall.append((time.perf_counter() - t0) * 1e3)
            kms.append(r.kernel_ms)
        out["device_" + name] = {"kernel_ms": kms, "wall_ms": wall}
    gen = dlp.batched_solve(NLP, m, n, SEED)
    out["objectives_bit_identical_to_generated"] = r.objective.tobytes() == gen.objective.tobytes() and \
        r.num_pivots.tobytes() == gen.num_pivots.tobytes() and r.status.tobytes() == gen.status.tobytes()
    out["objective_sha256"] = hashlib.sha256(r.objective.tobytes()).hexdigest()
    out["pivots"] = int(r.num_pivots.sum())
    dlp.batched_solve_dense(A, b, c)   # warm: the staging buffer
    kms, wall = [], []
    for _ in range(max(3, reps // 2)):
        t0 = time.perf_counter()
        rh = dlp.batched_solve_dense(A, b, c)
        wall.append((time.perf_counter() - t0) * 1e3)
        kms.append(rh.kernel_ms)
    out["host_xy"] = {"kernel_ms": kms, "wall_ms": wall,
                      "same_bytes_as_device": rh.objective.tobytes() == r.objective.tobytes()}
    out["occupancy"] = dlp.batched_occupancy(m, n)
    return out


def spawn(args):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True,
                       timeout=600)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"child {args} failed with status {p.returncode}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def spread(v):
    return {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v), "spread": max(v) - min(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", help="libdlp.so of the commit to compare with (the yardstick)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs="+", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kind, m, n = a.child[0], int(a.child[1]), int(a.child[2])
        res = child_generated(a.child[3], m, n, a.reps) if kind == "generated" else child_dense(m, n, a.reps)
        print(json.dumps(res))
        return
    reps = ["--reps", str(a.reps)]
    report = {"nlp": NLP, "seed": SEED, "warmup": WARM, "reps_per_child": a.reps, "shapes": {}}
    for m, n in SHAPES:
        runs = {"generated_this": [], "generated_other": []}
        dense = None
        for rnd in range(2):   # other, this, (dense), other, this: the libraries alternate
            if a.other_lib:
                runs["generated_other"].append(spawn(reps + ["--child", "generated", str(m), str(n), a.other_lib]))
            runs["generated_this"].append(spawn(reps + ["--child", "generated", str(m), str(n), THIS_LIB]))
            if rnd == 0:
                dense = spawn(reps + ["--child", "dense", str(m), str(n)])
        sh = {"dense": dense, "runs": runs}
        for k, v in runs.items():
            if v:
                sh[k + "_kernel_ms"] = spread([x for r in v for x in r["kernel_ms"]])
        for k in ("device_xy", "device_no_xy", "host_xy"):
            sh["dense_" + k + "_kernel_ms"] = spread(dense[k]["kernel_ms"])
            sh["dense_" + k + "_wall_ms"] = spread(dense[k]["wall_ms"])
        yard = sh.get("generated_other_kernel_ms") or sh["generated_this_kernel_ms"]
        sh["yardstick"] = "generated_other" if a.other_lib else "generated_this"
        lo, hi = yard["min"], yard["max"]
        sh["generated_this_inside_yardstick_spread"] = lo <= sh["generated_this_kernel_ms"]["median"] <= hi
        sh["dense_inside_yardstick_spread"] = lo <= sh["dense_device_xy_kernel_ms"]["median"] <= hi
        sh["dense_over_yardstick_median"] = sh["dense_device_xy_kernel_ms"]["median"] / yard["median"]
        sh["objectives_identical_everywhere"] = len(
            {r["objective_sha256"] for v in runs.values() for r in v} | {dense["objective_sha256"]}) == 1
        report["shapes"][f"{m}x{n}"] = sh
        print(json.dumps({f"{m}x{n}": {k: v for k, v in sh.items() if k not in ("runs", "dense")}}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
