#!/usr/bin/env python3
"""Timing of the resident batch: C5's shapes, 4,096 x (64 x 128) and
4,096 x (64 x 64), the generator's own LPs as device tensors, one MI355X, HIP events around the
kernel, 3 warm-ups, min / median / max over --reps repeats, no profiler attached.

    tools/batch_resolve_timing.py [--other-lib PATH/libdlp.so] [--reps 7] [--out FILE.json]

1. The yardstick: dlp_batched_solve_dense of the parent commit (--other-lib) against this
   commit's, in child processes of their own that alternate between the two libraries (plain
   ctypes, so the child also runs a library built from an older commit).  dlp_batch_create_dense
   is reported beside them: its extra time is the store of the resident state.
2. Warm against cold for c2 = c * (1 + 0.02 u), a new u per repeat: warm is
   dlp_batch_resolve(c2) from the optimum of c, cold is dlp_batched_solve_dense(A, b, c2).

Not a product file: the LPs come from the test oracle's generator."""
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
HBM_BYTES_PER_S = 8e12


def _inputs(m, n):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    torch.cuda.init()   # torch's HIP runtime first: the library then shares it
    import oracle_py as O
    lps = [O.gen_dense(m, n, SEED + k) for k in range(NLP)]
    A, b, c = (np.stack([p[i] for p in lps]) for i in range(3))
    return np, torch, (A, b, c), tuple(torch.from_numpy(v).cuda() for v in (A, b, c))


def child_dense(lib_path, m, n, reps):
    """dlp_batched_solve_dense of the library at lib_path, device tensors, x and y wanted."""
    np, torch, _, (tA, tb, tc) = _inputs(m, n)
    from distributedlpsolver_amd import _lib as L   # the argument structs only
    lib = C.CDLL(lib_path)
    obj, st, npv = np.zeros(NLP), np.zeros(NLP, np.int32), np.zeros(NLP, np.int64)
    x, y, ms = np.zeros((NLP, n)), np.zeros((NLP, m)), C.c_double()
    dp = C.POINTER(C.c_double)
    din = L.BatchDenseIn(tA.data_ptr(), tb.data_ptr(), tc.data_ptr(), m * n, m, n, 1, 0)
    out = L.BatchOut(obj.ctypes.data_as(dp), st.ctypes.data_as(C.POINTER(C.c_int32)),
                     npv.ctypes.data_as(C.POINTER(C.c_int64)), None, None, 0, x.ctypes.data_as(dp),
                     y.ctypes.data_as(dp), C.pointer(ms))
    torch.cuda.synchronize()

    def run():
        rc = lib.dlp_batched_solve_dense(C.c_int64(NLP), C.c_int64(m), C.c_int64(n), C.byref(din), None,
                                         C.byref(out))
        assert rc == 0, rc
        return ms.value
    for _ in range(WARM):
        run()
    kms = [run() for _ in range(reps)]
    return {"kernel_ms": kms, "pivots": int(npv.sum()), "all_optimal": bool((st == 0).all()),
            "objective_sha256": hashlib.sha256(obj.tobytes()).hexdigest()}


def child_batch(m, n, reps):
    """This commit's resident batch: creation, then warm re-solves against cold solves."""
    np, torch, (A, b, c), (tA, tb, tc) = _inputs(m, n)
    import distributedlpsolver_amd as dlp
    out = {}
    kms, wall = [], []
    for i in range(WARM + reps):
        t0 = time.perf_counter()
        bt = dlp.Batch(tA, tb, tc)
        w = (time.perf_counter() - t0) * 1e3
        if i >= WARM:
            kms.append(bt.result.kernel_ms)
            wall.append(w)
        info, first = bt.info(), bt.result
        bt.close()
    state_bytes = 8 * NLP * ((m + 1) * (n + 1) + (n + m + 3) // 2)
    out["create"] = {"kernel_ms": kms, "wall_ms": wall, "device_bytes": info["device_bytes"],
                     "state_bytes": state_bytes, "objective_sha256": hashlib.sha256(first.objective.tobytes()).hexdigest(),
                     "pivots": int(first.num_pivots.sum())}
    rng = np.random.default_rng(SEED)
    res = {k: [] for k in ("warm_kernel_ms", "warm_wall_ms", "warm_pivots", "cold_kernel_ms", "cold_wall_ms",
                           "cold_pivots", "max_rel_objective_diff", "back_kernel_ms", "back_pivots")}
    with dlp.Batch(tA, tb, tc) as bt:
        for i in range(WARM + reps):
            c2 = c * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, c.shape))
            t2 = torch.from_numpy(c2).cuda()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            warm = bt.resolve(t2)
            t1 = time.perf_counter()
            cold = dlp.batched_solve_dense(tA, tb, t2)
            t3 = time.perf_counter()
            back = bt.resolve(tc)   # to an optimum of c again, for the next repeat
            assert (warm.status == 0).all() and (cold.status == 0).all() and (back.status == 0).all()
            rel = float(np.max(np.abs(warm.objective - cold.objective) / (1.0 + np.abs(cold.objective))))
            assert rel <= 1e-9, rel
            if i >= WARM:
                for k, v in (("warm_kernel_ms", warm.kernel_ms), ("warm_wall_ms", (t1 - t0) * 1e3),
                             ("warm_pivots", int(warm.num_pivots.sum())), ("cold_kernel_ms", cold.kernel_ms),
                             ("cold_wall_ms", (t3 - t1) * 1e3), ("cold_pivots", int(cold.num_pivots.sum())),
                             ("max_rel_objective_diff", rel), ("back_kernel_ms", back.kernel_ms),
                             ("back_pivots", int(back.num_pivots.sum()))):
                    res[k].append(v)
        # the floor of a re-solve: the state load, the fused rebuild, pricing once, the state store
        same = [bt.resolve(tc).kernel_ms for _ in range(WARM + reps)][WARM:]
        idle = [bt.resolve(None).kernel_ms for _ in range(WARM + reps)][WARM:]
    res["same_c_kernel_ms"], res["resume_kernel_ms"] = same, idle
    out["resolve"] = res
    out["occupancy"] = dlp.batched_occupancy(m, n)
    return out


def spawn(args):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True,
                       timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"child {args} failed with status {p.returncode}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def spread(v):
    return {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v), "spread": max(v) - min(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", help="libdlp.so of the parent commit (the yardstick)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs="+", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kind, m, n = a.child[0], int(a.child[1]), int(a.child[2])
        print(json.dumps(child_dense(a.child[3], m, n, a.reps) if kind == "dense" else child_batch(m, n, a.reps)))
        return
    reps = ["--reps", str(a.reps)]
    report = {"nlp": NLP, "seed": SEED, "warmup": WARM, "reps_per_child": a.reps, "shapes": {}}
    for m, n in SHAPES:
        runs = {"dense_this": [], "dense_other": []}
        batch = None
        for rnd in range(2):   # other, this, (batch), other, this: the libraries alternate
            if a.other_lib:
                runs["dense_other"].append(spawn(reps + ["--child", "dense", str(m), str(n), a.other_lib]))
            runs["dense_this"].append(spawn(reps + ["--child", "dense", str(m), str(n), THIS_LIB]))
            if rnd == 0:
                batch = spawn(reps + ["--child", "batch", str(m), str(n)])
        sh = {"batch": batch, "runs": runs}
        for k, v in runs.items():
            if v:
                sh[k + "_kernel_ms"] = spread([x for r in v for x in r["kernel_ms"]])
        yard = sh.get("dense_other_kernel_ms") or sh["dense_this_kernel_ms"]
        sh["yardstick"] = "dense_other" if a.other_lib else "dense_this"
        sh["dense_this_inside_yardstick_spread"] = yard["min"] <= sh["dense_this_kernel_ms"]["median"] <= yard["max"]
        sh["create_kernel_ms"] = spread(batch["create"]["kernel_ms"])
        sh["create_wall_ms"] = spread(batch["create"]["wall_ms"])
        extra_ms = sh["create_kernel_ms"]["median"] - sh["dense_this_kernel_ms"]["median"]
        sh["create_extra_ms"] = extra_ms
        sh["state_bytes"] = batch["create"]["state_bytes"]
        sh["state_store_fraction_of_8TBps"] = (batch["create"]["state_bytes"] / (extra_ms * 1e-3) / HBM_BYTES_PER_S
                                               if extra_ms > 0 else None)
        r = batch["resolve"]
        for k in ("warm_kernel_ms", "warm_wall_ms", "cold_kernel_ms", "cold_wall_ms", "warm_pivots", "cold_pivots",
                  "back_kernel_ms", "back_pivots", "same_c_kernel_ms", "resume_kernel_ms"):
            sh[k] = spread(r[k])
        sh["max_rel_objective_diff"] = max(r["max_rel_objective_diff"])
        sh["cold_over_warm_kernel_median"] = sh["cold_kernel_ms"]["median"] / sh["warm_kernel_ms"]["median"]
        sh["cold_over_warm_pivots_median"] = sh["cold_pivots"]["median"] / max(1, sh["warm_pivots"]["median"])
        sh["objectives_identical_everywhere"] = len(
            {x["objective_sha256"] for v in runs.values() for x in v} | {batch["create"]["objective_sha256"]}) == 1
        report["shapes"][f"{m}x{n}"] = sh
        print(json.dumps({f"{m}x{n}": {k: v for k, v in sh.items() if k not in ("runs", "batch")}}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
