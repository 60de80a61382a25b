#!/usr/bin/env python3
"""Timing of dlp_batch_add_cols, by the protocol of tools/batch_add_rows_timing.py:
C5's shapes, 4,096 x (64 x 128) and 4,096 x (64 x 64), the generator's own LPs as device tensors,
one MI355X, HIP events around the kernel, 3 warm-ups, min / median / max over --reps repeats per
child process, no profiler attached.

    tools/batch_add_cols_timing.py [--other-lib PATH/libdlp.so] [--reps 7] [--shapes 64x128,64x64] [--out FILE.json]

1. Warm against cold: every repeat builds a fresh batch outside the timed part (the call widens
   it), then times add_cols of k = 1 and k = 4 columns priced 2 % and 10 % above y* . p
   (P ~ U[0, 1) with 30 % zeros, new per repeat; d = (1 + depth) y* . P) against
   dlp_batched_solve_dense of the stacked m x (n + k) LPs.
2. The floor: add_cols of columns priced below y* . p (load, re-stride, fold, one pricing, store).
   Then what a widened batch pays afterwards: resolve(c2) and resolve_rhs(b2), +-2 %, on a batch
   widened by one such column beside the same change on a batch that was not widened.
3. Nothing existing got slower (--other-lib: the parent commit's library): the children of
   tools/batch_rhs_timing.py for dlp_batched_solve_dense / resolve(c2) and for resolve_rhs(b2),
   and a child of this file for add_rows (one cut at 2 %), the two libraries alternating (other,
   this, other, this); accepted when this commit's median lies inside the parent's own min-max
   spread.

Not a product file: the LPs come from the test oracle's generator."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_rhs_timing as BT   # noqa: E402  (the shared protocol: inputs, the children of the existing paths)

NLP, SEED, WARM = BT.NLP, BT.SEED, BT.WARM
COLS = (1, 4)
DEPTHS = (0.02, 0.10)


def child_cols(m, n, reps):
    np, torch, (A, b, c), (tA, tb, tc) = BT._inputs(m, n)
    import distributedlpsolver_amd as dlp
    out = {"occupancy": dlp.batched_occupancy(m, n)}
    rng = np.random.default_rng(SEED)
    with dlp.Batch(tA, tb, tc) as bt:
        assert (bt.result.status == 0).all()
        y = bt.result.y
        out["register_kernel_of_creation"] = bt.info()["register_kernel"]

    def cols(k):
        P = rng.uniform(0.0, 1.0, (NLP, m, k)) * (rng.uniform(size=(NLP, m, k)) >= 0.3)
        return P, np.einsum("ki,kit->kt", y, P)

    for k in COLS:
        for depth in DEPTHS + (None,):   # None: the floor, columns that do not price out
            keys = ("warm_kernel_ms", "warm_wall_ms", "warm_pivots", "warm_max_pivots", "cold_kernel_ms",
                    "cold_wall_ms", "cold_pivots", "max_rel_objective_diff")
            res = {key: [] for key in keys}
            for i in range(WARM + reps):
                P, yp = cols(k)
                d = 0.9 * yp - 1e-3 if depth is None else (1.0 + depth) * yp
                tP, td = torch.from_numpy(P).cuda(), torch.from_numpy(d).cuda()
                tA2, tc2 = torch.cat([tA, tP], dim=2).contiguous(), torch.cat([tc, td], dim=1).contiguous()
                with dlp.Batch(tA, tb, tc) as bt:   # a fresh batch, outside the timed part
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    warm = bt.add_cols(tP, td)
                    t1 = time.perf_counter()
                    after = bt.info()
                cold = dlp.batched_solve_dense(tA2, tb, tc2)
                t2 = time.perf_counter()
                assert (warm.status == 0).all() and (cold.status == 0).all()
                rel = float(np.max(np.abs(warm.objective - cold.objective) / np.maximum(1.0, np.abs(cold.objective))))
                assert rel <= 1e-9, rel
                if depth is None:
                    assert not warm.num_pivots.any()
                if i >= WARM:
                    for key, v in zip(keys, (warm.kernel_ms, (t1 - t0) * 1e3, int(warm.num_pivots.sum()),
                                             int(warm.num_pivots.max()), cold.kernel_ms, (t2 - t1) * 1e3,
                                             int(cold.num_pivots.sum()), rel)):
                        res[key].append(v)
            res["register_kernel_afterwards"] = after["register_kernel"]
            out[f"k{k}_" + ("floor" if depth is None else f"depth_{depth}")] = res
    # what a widened batch pays afterwards: resolve(c2) and resolve_rhs(b2), +-2 %, on a batch widened
    # by one column that does not price out (still the register kernel at these shapes) beside the
    # same change on a batch that was not widened
    keys = ("wide_c_kernel_ms", "wide_c_pivots", "plain_c_kernel_ms", "plain_c_pivots", "wide_rhs_kernel_ms",
            "wide_rhs_pivots", "plain_rhs_kernel_ms", "plain_rhs_pivots")
    res = {key: [] for key in keys}
    for i in range(WARM + reps):
        P, yp = cols(1)
        d = 0.5 * yp - 1.0
        c2 = c * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, c.shape))
        t2 = torch.from_numpy(c2).cuda()
        t2w = torch.from_numpy(np.concatenate([c2, d], axis=1)).cuda()
        tb2 = torch.from_numpy(b * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, b.shape))).cuda()
        with dlp.Batch(tA, tb, tc) as bt:
            bt.add_cols(torch.from_numpy(P).cuda(), torch.from_numpy(d).cuda())
            wc, wr = bt.resolve(t2w), bt.resolve_rhs(tb2)
            res["wide_register_kernel"] = bt.info()["register_kernel"]
        with dlp.Batch(tA, tb, tc) as bt:
            pc, pr = bt.resolve(t2), bt.resolve_rhs(tb2)
            res["plain_register_kernel"] = bt.info()["register_kernel"]
        assert all((r.status == 0).all() for r in (wc, wr, pc, pr))
        if i >= WARM:
            for key, v in zip(keys, (wc.kernel_ms, int(wc.num_pivots.sum()), pc.kernel_ms, int(pc.num_pivots.sum()),
                                     wr.kernel_ms, int(wr.num_pivots.sum()), pr.kernel_ms, int(pr.num_pivots.sum()))):
                res[key].append(v)
    out["after_growth"] = res
    return out


def child_add_rows(lib_path, m, n, reps):
    """dlp_batch_add_rows of the library at lib_path through the package (an older library is bound
    with the entry points it has): one cut per LP that removes 2 % of g . x*, a fresh batch per
    repeat, the same cuts in every child."""
    np, torch, (A, b, c), (tA, tb, tc) = BT._inputs(m, n)
    from distributedlpsolver_amd import _lib as L
    probe = C.CDLL(lib_path)
    L.LIB_PATH = lib_path
    L.SIGNATURES = [sig for sig in L.SIGNATURES if hasattr(probe, sig[0])]
    import distributedlpsolver_amd as dlp
    rng = np.random.default_rng(SEED)
    ms, pivots = [], 0
    x = None
    for i in range(WARM + reps):
        with dlp.Batch(tA, tb, tc) as bt:
            x = bt.result.x if x is None else x
            G = rng.uniform(0.0, 1.0, (NLP, 1, n)) * (rng.uniform(size=(NLP, 1, n)) >= 0.3)
            h = 0.98 * np.einsum("krj,kj->kr", G, x)
            r = bt.add_rows(torch.from_numpy(G).cuda(), torch.from_numpy(h).cuda())
        assert (r.status == 0).all()
        if i >= WARM:
            ms.append(r.kernel_ms)
            pivots += int(r.num_pivots.sum())
    return {"library": lib_path, "add_rows_kernel_ms": ms, "add_rows_pivots": pivots}


def spawn(script, args):
    p = subprocess.run([sys.executable, script] + args, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"child {args} failed with status {p.returncode}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", help="libdlp.so of the parent commit (the yardstick)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(f"{m}x{n}" for m, n in BT.SHAPES))
    ap.add_argument("--out")
    ap.add_argument("--child", nargs="+", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "add_rows":
            print(json.dumps(child_add_rows(a.child[3], int(a.child[1]), int(a.child[2]), a.reps)))
        else:
            print(json.dumps(child_cols(int(a.child[0]), int(a.child[1]), a.reps)))
        return
    me, rhs_tool = os.path.abspath(__file__), os.path.abspath(BT.__file__)
    reps = ["--reps", str(a.reps)]
    report = {"nlp": NLP, "seed": SEED, "warmup": WARM, "reps_per_child": a.reps, "shapes": {}}
    for m, n in (tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")):
        raw = spawn(me, reps + ["--child", str(m), str(n)])
        sh = {"cols": raw}
        for key, res in raw.items():
            if isinstance(res, dict) and ("warm_kernel_ms" in res or "wide_c_kernel_ms" in res):
                sh[key] = {k: (BT.spread(v) if isinstance(v, list) else v) for k, v in res.items()}
        if a.other_lib:
            runs = {"this": [], "other": []}
            rhs = {"this": [], "other": []}
            rows = {"this": [], "other": []}
            for _ in range(2):   # other, this, other, this: the libraries alternate
                runs["other"].append(spawn(rhs_tool, reps + ["--child", "existing", str(m), str(n), a.other_lib]))
                runs["this"].append(spawn(rhs_tool, reps + ["--child", "existing", str(m), str(n), BT.THIS_LIB]))
                rhs["other"].append(spawn(rhs_tool, reps + ["--child", "rhs", str(m), str(n), a.other_lib]))
                rhs["this"].append(spawn(rhs_tool, reps + ["--child", "rhs", str(m), str(n)]))
                rows["other"].append(spawn(me, reps + ["--child", "add_rows", str(m), str(n), a.other_lib]))
                rows["this"].append(spawn(me, reps + ["--child", "add_rows", str(m), str(n), BT.THIS_LIB]))
            sh["runs"], sh["rhs"], sh["add_rows"] = runs, rhs, rows
            series = {"dense": lambda x: x["dense_kernel_ms"], "resolve_c": lambda x: x["resolve_c_kernel_ms"]}
            for who in ("this", "other"):
                for path, get in series.items():
                    sh[f"{path}_{who}_kernel_ms"] = BT.spread([v for x in runs[who] for v in get(x)])
                for scale in BT.SCALES:
                    sh[f"resolve_rhs_{scale}_{who}_kernel_ms"] = BT.spread(
                        [v for x in rhs[who] for v in x[f"scale_{scale}"]["warm_kernel_ms"]])
                sh[f"add_rows_{who}_kernel_ms"] = BT.spread([v for x in rows[who] for v in x["add_rows_kernel_ms"]])
            for path in list(series) + [f"resolve_rhs_{s}" for s in BT.SCALES] + ["add_rows"]:
                yard, med = sh[f"{path}_other_kernel_ms"], sh[f"{path}_this_kernel_ms"]["median"]
                sh[f"{path}_this_median_inside_parent_spread"] = yard["min"] <= med <= yard["max"]
            for path in series:
                sh[f"{path}_results_identical"] = len({x[f"{path}_objective_sha256"] for v in runs.values() for x in v}) == 1
            for scale in BT.SCALES:
                sh[f"resolve_rhs_{scale}_pivots_identical"] = \
                    rhs["this"][0][f"scale_{scale}"]["warm_pivots"] == rhs["other"][0][f"scale_{scale}"]["warm_pivots"]
            sh["add_rows_pivots_identical"] = len({x["add_rows_pivots"] for v in rows.values() for x in v}) == 1
        report["shapes"][f"{m}x{n}"] = sh
        print(json.dumps({f"{m}x{n}": {k: v for k, v in sh.items() if k not in ("runs", "rhs", "cols", "add_rows")}}),
              flush=True)
        if a.out:   # (after every shape: a run cut short keeps what it has)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
