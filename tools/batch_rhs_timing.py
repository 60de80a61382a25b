#!/usr/bin/env python3
"""Timing of dlp_batch_resolve_rhs: C5's shapes, 4,096 x (64 x 128) and
4,096 x (64 x 64), the generator's own LPs as device tensors, one MI355X, HIP events around the
kernel, 3 warm-ups, min / median / max over --reps repeats, no profiler attached.

    tools/batch_rhs_timing.py [--other-lib PATH/libdlp.so] [--reps 7] [--out FILE.json]

1. Warm against cold for b2 = b * (1 + s u), s = 0.02 and 0.3, a new u per repeat: warm is
   dlp_batch_resolve_rhs(b2) from the optimum of b, cold is dlp_batched_solve_dense(A, b2, c).
2. The floor: dlp_batch_resolve_rhs with the unchanged b (load, rebuild, one eligibility test,
   store) beside dlp_batch_resolve(NULL) (load, store).
   With --other-lib the same child also runs the parent commit's library, alternating with this
   commit's (other, this, other, this; the same b2 sequence in each), and the report says
   whether this commit's median warm time lies below the parent's minimum.
3. Nothing existing got slower: dlp_batched_solve_dense and dlp_batch_resolve(c2) of the
   parent commit's library (--other-lib) against this commit's, in child processes of their
   own that alternate between the two libraries (plain ctypes, so a child also runs a library
   built from an older commit).

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
SCALES = (0.02, 0.3)


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


def child_existing(lib_path, m, n, reps):
    """The two existing paths of the library at lib_path through its C ABI: the one-shot
    dlp_batched_solve_dense, then dlp_batch_resolve(c2) from the optimum (c2 = c (1 + 0.02 u),
    the same u in every child; resolve(c) takes the batch back between repeats)."""
    np, torch, (A, b, c), (tA, tb, tc) = _inputs(m, n)
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
    i64 = C.c_int64

    def dense():
        rc = lib.dlp_batched_solve_dense(i64(NLP), i64(m), i64(n), C.byref(din), None, C.byref(out))
        assert rc == 0 and (st == 0).all(), rc
        return ms.value
    for _ in range(WARM):
        dense()
    dense_ms = [dense() for _ in range(reps)]
    res = {"dense_kernel_ms": dense_ms, "dense_pivots": int(npv.sum()),
           "dense_objective_sha256": hashlib.sha256(obj.tobytes()).hexdigest()}
    h = C.c_void_p()
    rc = lib.dlp_batch_create_dense(i64(NLP), i64(m), i64(n), C.byref(din), None, C.byref(out), C.byref(h))
    assert rc == 0, rc
    rng = np.random.default_rng(SEED)
    warm_ms, digest, pivots = [], hashlib.sha256(), 0
    for i in range(WARM + reps):
        t2 = torch.from_numpy(c * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, c.shape))).cuda()
        torch.cuda.synchronize()
        for ptr in (t2.data_ptr(), tc.data_ptr()):
            rc = lib.dlp_batch_resolve(h, C.c_void_p(ptr), i64(n), 1, i64(10 ** 6), C.byref(out))
            assert rc == 0 and (st == 0).all(), rc
            if ptr == t2.data_ptr() and i >= WARM:
                warm_ms.append(ms.value)
                pivots += int(npv.sum())
                digest.update(obj.tobytes())
    lib.dlp_batch_free(h)
    res.update({"resolve_c_kernel_ms": warm_ms, "resolve_c_pivots": pivots, "resolve_c_objective_sha256": digest.hexdigest()})
    return res


def child_rhs(m, n, reps, lib_path=None):
    """dlp_batch_resolve_rhs of the library at lib_path (default: this commit's) through the
    package: warm against cold for both scales, then the floor.  A library of an older commit
    is bound with the entry points it has."""
    np, torch, (A, b, c), (tA, tb, tc) = _inputs(m, n)
    from distributedlpsolver_amd import _lib as L
    if lib_path:
        probe = C.CDLL(lib_path)
        L.LIB_PATH = lib_path
        L.SIGNATURES = [sig for sig in L.SIGNATURES if hasattr(probe, sig[0])]
    import distributedlpsolver_amd as dlp
    out = {"library": lib_path or THIS_LIB, "occupancy": dlp.batched_occupancy(m, n)}
    rng = np.random.default_rng(SEED)
    with dlp.Batch(tA, tb, tc) as bt:
        assert (bt.result.status == 0).all()
        out["register_kernel_of_creation"] = bt.info()["register_kernel"]
        # (the kernel of the dual call: libraries before dlp_batch_rhs_kernel ran the LDS kernel)
        out["rhs_kernel"] = bt.rhs_kernel() if hasattr(L.lib(), "dlp_batch_rhs_kernel") else None
        for scale in SCALES:
            res = {k: [] for k in ("warm_kernel_ms", "warm_wall_ms", "warm_pivots", "warm_max_pivots", "cold_kernel_ms",
                                   "cold_wall_ms", "cold_pivots", "max_rel_objective_diff", "back_kernel_ms",
                                   "back_pivots")}
            for i in range(WARM + reps):
                b2 = b * (1.0 + scale * rng.uniform(-1.0, 1.0, b.shape))
                t2 = torch.from_numpy(b2).cuda()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                warm = bt.resolve_rhs(t2)
                t1 = time.perf_counter()
                cold = dlp.batched_solve_dense(tA, t2, tc)
                t3 = time.perf_counter()
                back = bt.resolve_rhs(tb)   # to an optimum of b again, for the next repeat
                assert (warm.status == 0).all() and (cold.status == 0).all() and (back.status == 0).all()
                rel = float(np.max(np.abs(warm.objective - cold.objective) / np.maximum(1.0, np.abs(cold.objective))))
                assert rel <= 1e-9, rel
                if i >= WARM:
                    for k, v in (("warm_kernel_ms", warm.kernel_ms), ("warm_wall_ms", (t1 - t0) * 1e3),
                                 ("warm_pivots", int(warm.num_pivots.sum())),
                                 ("warm_max_pivots", int(warm.num_pivots.max())),
                                 ("cold_kernel_ms", cold.kernel_ms), ("cold_wall_ms", (t3 - t1) * 1e3),
                                 ("cold_pivots", int(cold.num_pivots.sum())), ("max_rel_objective_diff", rel),
                                 ("back_kernel_ms", back.kernel_ms), ("back_pivots", int(back.num_pivots.sum()))):
                        res[k].append(v)
            out[f"scale_{scale}"] = res
        # the floor: load, rebuild, one eligibility test, store; beside load, store
        same = [bt.resolve_rhs(tb) for _ in range(WARM + reps)][WARM:]
        assert all(not r.num_pivots.any() and (r.status == 0).all() for r in same)
        idle = [bt.resolve(None).kernel_ms for _ in range(WARM + reps)][WARM:]
        out["floor"] = {"same_b_kernel_ms": [r.kernel_ms for r in same], "resume_kernel_ms": idle}
    return out


def spawn(args):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True,
                       timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"child {args} failed with status {p.returncode}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def spread(v):
    return {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", help="libdlp.so of the parent commit (the yardstick)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--child", nargs="+", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kind, m, n = a.child[0], int(a.child[1]), int(a.child[2])
        print(json.dumps(child_existing(a.child[3], m, n, a.reps) if kind == "existing"
                         else child_rhs(m, n, a.reps, a.child[3] if len(a.child) > 3 else None)))
        return
    reps = ["--reps", str(a.reps)]
    report = {"nlp": NLP, "seed": SEED, "warmup": WARM, "reps_per_child": a.reps, "shapes": {}}
    for m, n in SHAPES:
        # the dual call itself, the same b2 sequence in every child: other, this, other, this
        rhs = {"this": [], "other": []}
        for _ in range(2 if a.other_lib else 1):
            if a.other_lib:
                rhs["other"].append(spawn(reps + ["--child", "rhs", str(m), str(n), a.other_lib]))
            rhs["this"].append(spawn(reps + ["--child", "rhs", str(m), str(n)]))
        sh = {"rhs": rhs}
        for who, tag in (("this", ""), ("other", "_other")):
            if not rhs[who]:
                continue
            for scale in SCALES:
                keys = rhs[who][0][f"scale_{scale}"].keys()
                sh[f"scale_{scale}{tag}"] = {k: spread([x for r in rhs[who] for x in r[f"scale_{scale}"][k]])
                                             for k in keys}
            sh[f"floor{tag}"] = {k: spread([x for r in rhs[who] for x in r["floor"][k]])
                                 for k in rhs[who][0]["floor"]}
        if a.other_lib:   # the yardstick of DESIGN.md §23: this median below the parent's minimum
            for scale in SCALES:
                sh[f"scale_{scale}_warm_median_below_parent_min"] = (
                    sh[f"scale_{scale}"]["warm_kernel_ms"]["median"] < sh[f"scale_{scale}_other"]["warm_kernel_ms"]["min"])
                sh[f"scale_{scale}_warm_pivots_identical"] = (
                    rhs["this"][0][f"scale_{scale}"]["warm_pivots"] == rhs["other"][0][f"scale_{scale}"]["warm_pivots"])
        runs = {"this": [], "other": []}
        for _ in range(2):   # other, this, other, this: the libraries alternate
            if a.other_lib:
                runs["other"].append(spawn(reps + ["--child", "existing", str(m), str(n), a.other_lib]))
            runs["this"].append(spawn(reps + ["--child", "existing", str(m), str(n), THIS_LIB]))
        sh["runs"] = runs
        for path in ("dense", "resolve_c"):
            for who, v in runs.items():
                if v:
                    sh[f"{path}_{who}_kernel_ms"] = spread([x for r in v for x in r[f"{path}_kernel_ms"]])
            yard = sh.get(f"{path}_other_kernel_ms")
            if yard:
                med = sh[f"{path}_this_kernel_ms"]["median"]
                sh[f"{path}_this_median_inside_parent_spread"] = yard["min"] <= med <= yard["max"]
            sh[f"{path}_results_identical"] = len({x[f"{path}_objective_sha256"] for v in runs.values() for x in v}) == 1
        report["shapes"][f"{m}x{n}"] = sh
        print(json.dumps({f"{m}x{n}": {k: v for k, v in sh.items() if k not in ("runs", "rhs")}}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
