"""GPU: a plain `bench.py --gpus 1 --steps S --warmup W --dump-outputs DIR` run (the C2 LP, the
smallest streaming workload): the result line's fields, S really setting the timed steps, the
moved legs absent, and the dumped arrays equal to what the same pivots of the same seeded LP give
through the session API in this process (bit for bit: the path is deterministic)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import distributedlpsolver_amd as dlp
from conftest import ROOT

pytestmark = pytest.mark.gpu

STEPS, WARMUP = 3, 1


def test_plain_bench_line_and_dump(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c2",
                        "--steps", str(STEPS), "--warmup", str(WARMUP), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    K = d["K"]
    assert d["unit"] == "pivots/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == STEPS and d["pivots_timed"] == STEPS * K and d["passes_in_window"] == STEPS
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(K / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert d["full"] is False
    for leg in ("pivot_step_window", "rank1_update_roofline", "cpu_baseline", "pivot_log_vs_oracle",
                "alt_exchange_window"):
        assert d[leg] is None, leg

    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["num_pivots", "objective", "pivot_log", "tableau_row_index", "tableau_rows", "x", "y"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64e6
    pivots = (WARMUP + STEPS) * K
    with dlp.Session(dlp.Problem.random(4096, 4096, 2), check_interval=64, max_pivots=pivots + 1,
                     log_pivots=1) as s:
        st, done = s.run(pivots)
        assert done == pivots
        res = s.result()
        idx = got["tableau_row_index"]
        assert idx[-1] == -1 and len(idx) == len(got["tableau_rows"])
        rows = np.stack([s.read_rows(int(i) if i >= 0 else s.rows, 1)[0] for i in idx])
    assert got["num_pivots"].tolist() == [pivots] and got["objective"].tolist() == [res.objective]
    assert got["x"].tobytes() == res.x.tobytes() and got["y"].tobytes() == res.y.tobytes()
    log = np.stack([res.pivot_log[f].astype(np.float64) for f in ("q", "p", "leaving", "ratio", "objective")], axis=1)
    assert got["pivot_log"].tobytes() == log.tobytes()
    assert got["tableau_rows"].tobytes() == rows.tobytes()
