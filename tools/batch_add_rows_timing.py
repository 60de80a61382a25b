#!/usr/bin/env python3
"""Timing of dlp_batch_add_rows, by the protocol of tools/batch_rhs_timing.py:
C5's shapes, 4,096 x (64 x 128) and 4,096 x (64 x 64), the generator's own LPs as device tensors,
one MI355X, HIP events around the kernel, 3 warm-ups, min / median / max over --reps repeats per
child process, no profiler attached.

    tools/batch_add_rows_timing.py [--other-lib PATH/libdlp.so] [--reps 7] [--shapes 64x128,64x64] [--out FILE.json]

1. Warm against cold: every repeat builds a fresh batch outside the timed part (the call grows
   it), then times add_rows of r = 1 and r = 4 cuts that remove 2 % and 10 % of g . x*
   (G ~ U[0, 1) with 30 % zeros, new per repeat; h = (1 - depth) G x*) against
   dlp_batched_solve_dense of the stacked (m + r)-row LPs.
2. The floor: add_rows of cuts no LP violates (load, fold, one eligibility test, store).
   Then what a grown batch pays afterwards: resolve_rhs(b2), +-2 %, on a batch grown by one such
   cut beside the same b2 on a batch that was not grown.
3. Nothing existing got slower (--other-lib: the parent commit's library): the children of
   tools/batch_rhs_timing.py for dlp_batched_solve_dense / resolve(c2) and for resolve_rhs(b2),
   the two libraries alternating (other, this, other, this); accepted when this commit's median
   lies inside the parent's own min-max spread.

Not a product file: the LPs come from the test oracle's generator."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_rhs_timing as BT   # noqa: E402  (the shared protocol: inputs, the children of the existing paths)

NLP, SEED, WARM = BT.NLP, BT.SEED, BT.WARM
ROWS = (1, 4)
DEPTHS = (0.02, 0.10)


def child_rows(m, n, reps):
    np, torch, (A, b, c), (tA, tb, tc) = BT._inputs(m, n)
    import distributedlpsolver_amd as dlp
    out = {"occupancy": dlp.batched_occupancy(m, n)}
    rng = np.random.default_rng(SEED)
    with dlp.Batch(tA, tb, tc) as bt:
        assert (bt.result.status == 0).all()
        x = bt.result.x
        out["register_kernel_of_creation"] = bt.info()["register_kernel"]

    def rows(r):
        G = rng.uniform(0.0, 1.0, (NLP, r, n)) * (rng.uniform(size=(NLP, r, n)) >= 0.3)
        return G, np.einsum("krj,kj->kr", G, x)

    for r in ROWS:
        for depth in DEPTHS + (None,):   # None: the floor, cuts no LP violates
            keys = ("warm_kernel_ms", "warm_wall_ms", "warm_pivots", "warm_max_pivots", "cold_kernel_ms",
                    "cold_wall_ms", "cold_pivots", "max_rel_objective_diff")
            res = {k: [] for k in keys}
            for i in range(WARM + reps):
                G, gx = rows(r)
                h = gx + 1.0 if depth is None else (1.0 - depth) * gx
                tG, th = torch.from_numpy(G).cuda(), torch.from_numpy(h).cuda()
                tA2, tb2 = torch.cat([tA, tG], dim=1).contiguous(), torch.cat([tb, th], dim=1).contiguous()
                with dlp.Batch(tA, tb, tc) as bt:   # a fresh batch, outside the timed part
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    warm = bt.add_rows(tG, th)
                    t1 = time.perf_counter()
                    after = bt.info()
                cold = dlp.batched_solve_dense(tA2, tb2, tc)
                t2 = time.perf_counter()
                assert (warm.status == 0).all() and (cold.status == 0).all()
                rel = float(np.max(np.abs(warm.objective - cold.objective) / np.maximum(1.0, np.abs(cold.objective))))
                assert rel <= 1e-9, rel
                if depth is None:
                    assert not warm.num_pivots.any()
                if i >= WARM:
                    for k, v in zip(keys, (warm.kernel_ms, (t1 - t0) * 1e3, int(warm.num_pivots.sum()),
                                           int(warm.num_pivots.max()), cold.kernel_ms, (t2 - t1) * 1e3,
                                           int(cold.num_pivots.sum()), rel)):
                        res[k].append(v)
            res["register_kernel_afterwards"] = after["register_kernel"]
            out[f"r{r}_" + ("floor" if depth is None else f"depth_{depth}")] = res
    # what a batch grown past m = 64 pays afterwards: resolve_rhs(+-2 %) on a batch grown by one
    # cut far from every optimum (the LDS kernel from then on) beside the same b2 on a batch that
    # was not grown; the grown call is held to the cold solve of the stacked LPs
    res = {k: [] for k in ("grown_kernel_ms", "grown_pivots", "ungrown_kernel_ms", "ungrown_pivots",
                           "max_rel_objective_diff")}
    for i in range(WARM + reps):
        G, gx = rows(1)
        tG, th = torch.from_numpy(G).cuda(), torch.from_numpy(2.0 * gx + 1.0).cuda()
        t2 = torch.from_numpy(b * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, b.shape))).cuda()
        t2g = torch.cat([t2, th], dim=1).contiguous()
        with dlp.Batch(tA, tb, tc) as bt:
            bt.add_rows(tG, th)
            grown = bt.resolve_rhs(t2g)
            res["grown_register_kernel"] = bt.rhs_kernel()["register_kernel"]
        with dlp.Batch(tA, tb, tc) as bt:
            plain = bt.resolve_rhs(t2)
            res["ungrown_register_kernel"] = bt.rhs_kernel()["register_kernel"]
        cold = dlp.batched_solve_dense(torch.cat([tA, tG], dim=1).contiguous(), t2g, tc)
        assert (grown.status == 0).all() and (plain.status == 0).all() and (cold.status == 0).all()
        rel = float(np.max(np.abs(grown.objective - cold.objective) / np.maximum(1.0, np.abs(cold.objective))))
        assert rel <= 1e-9, rel
        if i >= WARM:
            for k, v in (("grown_kernel_ms", grown.kernel_ms), ("grown_pivots", int(grown.num_pivots.sum())),
                         ("ungrown_kernel_ms", plain.kernel_ms), ("ungrown_pivots", int(plain.num_pivots.sum())),
                         ("max_rel_objective_diff", rel)):
                res[k].append(v)
    out["after_growth"] = res
    return out


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
        print(json.dumps(child_rows(int(a.child[0]), int(a.child[1]), a.reps)))
        return
    me, rhs_tool = os.path.abspath(__file__), os.path.abspath(BT.__file__)
    reps = ["--reps", str(a.reps)]
    report = {"nlp": NLP, "seed": SEED, "warmup": WARM, "reps_per_child": a.reps, "shapes": {}}
    for m, n in (tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")):
        raw = spawn(me, reps + ["--child", str(m), str(n)])
        sh = {"rows": raw}
        for key, res in raw.items():
            if isinstance(res, dict) and ("warm_kernel_ms" in res or "grown_kernel_ms" in res):
                sh[key] = {k: (BT.spread(v) if isinstance(v, list) else v) for k, v in res.items()}
        if a.other_lib:
            runs = {"this": [], "other": []}
            rhs = {"this": [], "other": []}
            for _ in range(2):   # other, this, other, this: the libraries alternate
                runs["other"].append(spawn(rhs_tool, reps + ["--child", "existing", str(m), str(n), a.other_lib]))
                runs["this"].append(spawn(rhs_tool, reps + ["--child", "existing", str(m), str(n), BT.THIS_LIB]))
                rhs["other"].append(spawn(rhs_tool, reps + ["--child", "rhs", str(m), str(n), a.other_lib]))
                rhs["this"].append(spawn(rhs_tool, reps + ["--child", "rhs", str(m), str(n)]))
            sh["runs"], sh["rhs"] = runs, rhs
            series = {"dense": lambda x: x["dense_kernel_ms"], "resolve_c": lambda x: x["resolve_c_kernel_ms"]}
            for who in ("this", "other"):
                for path, get in series.items():
                    sh[f"{path}_{who}_kernel_ms"] = BT.spread([v for x in runs[who] for v in get(x)])
                for scale in BT.SCALES:
                    sh[f"resolve_rhs_{scale}_{who}_kernel_ms"] = BT.spread(
                        [v for x in rhs[who] for v in x[f"scale_{scale}"]["warm_kernel_ms"]])
            for path in list(series) + [f"resolve_rhs_{s}" for s in BT.SCALES]:
                yard, med = sh[f"{path}_other_kernel_ms"], sh[f"{path}_this_kernel_ms"]["median"]
                sh[f"{path}_this_median_inside_parent_spread"] = yard["min"] <= med <= yard["max"]
            for path in series:
                sh[f"{path}_results_identical"] = len({x[f"{path}_objective_sha256"] for v in runs.values() for x in v}) == 1
            for scale in BT.SCALES:
                sh[f"resolve_rhs_{scale}_pivots_identical"] = \
                    rhs["this"][0][f"scale_{scale}"]["warm_pivots"] == rhs["other"][0][f"scale_{scale}"]["warm_pivots"]
        report["shapes"][f"{m}x{n}"] = sh
        print(json.dumps({f"{m}x{n}": {k: v for k, v in sh.items() if k not in ("runs", "rhs", "rows")}}), flush=True)
        if a.out:   # (after every shape: a run cut short keeps what it has)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
