"""CPU checks of bench.py's host-side pieces (no GPU): the CPU-baseline leg
(the oracle on a bounded sample, all usable threads then 1 thread) and the
committed-PMC lookup, so that a bench run on the box cannot die in them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_cpu_baseline_small():
    cb = bench.cpu_baseline(1500, 1500, 3, 0.2)
    assert cb["unit"] == "pivots/s" and cb["kind"] == "port"
    assert cb["value"] > 0 and cb["single_thread"]["value"] > 0
    assert cb["cores"] >= 1 and cb["single_thread"]["cores"] == 1
    assert cb["cpu_model"] and cb["nproc"] >= 1 and cb["cpus_usable"] >= 1


def test_cpu_baseline_like_for_like():
    """The deferred rank-K leg (the GPU's algorithm on the host): whole blocks, labelled."""
    cb = bench.cpu_baseline(1500, 1500, 3, 0.2, K=16)
    lf = cb["like_for_like"]
    assert lf["unit"] == "pivots/s" and lf["value"] > 0 and lf["cores"] == cb["cores"]
    assert "deferred rank-16" in lf["algorithm"]


def test_committed_traffic_unknown_geometry():
    val, src = bench.committed_traffic({"workload": "none", "kernel": "pass", "K": -1})
    assert val is None and src is None


def test_committed_traffic_for_the_default_bench_geometry():
    """The default bench (C3, K = 32, form 4) finds its committed PMC summary, and
    profiles/ travels to the GPU box (bench.py reads it there)."""
    geo = {"workload": "c3", "kernel": "pass", "K": 32, "form": 4, "rows_per_block": 256,
           "nontemporal": 1, "ld": 66048, "rows_local": 32768}
    val, src = bench.committed_traffic(geo)
    assert val and 3.0e10 < val < 4.5e10 and src.startswith("profiles/")
    with open(os.path.join(ROOT, ".gpurunignore")) as f:
        pats = [line.strip() for line in f if line.strip()]
    assert not any(p.strip("./").startswith("profiles") for p in pats)


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_window_only(monkeypatch):
    """Without --full every leg beside the timed window is off; --full turns them on again and
    each keeps its own switch."""
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu_baseline and a.no_eager_window and a.no_pivot_window
    a = _parse(monkeypatch, "--full", "--no-eager-window", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"
    assert not a.no_cpu_baseline and not a.no_pivot_window and a.no_eager_window


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: one float64 .npy per array, integers exact; the tableau sample is the same
    seeded choice of rows on every run, the objective row last."""
    import numpy as np

    class Sess:   # the two calls session_outputs makes on a rank that is not rank 0
        rows, row_first, ld = 100, 300, 8

        def read_rows(self, first, count):
            return np.full((count, self.ld), float(first))

    outs = [bench.session_outputs(Sess(), 1, 2) for _ in range(2)]
    assert sorted(outs[0]) == ["tableau_row_index_rank1", "tableau_rows_rank1"]
    idx, rows = outs[0]["tableau_row_index_rank1"], outs[0]["tableau_rows_rank1"]
    assert (idx == outs[1]["tableau_row_index_rank1"]).all() and idx[-1] == -1
    assert rows.shape == (bench.DUMP_ROWS + 1, 8) and len(set(idx)) == bench.DUMP_ROWS + 1
    assert (rows[:-1, 0] == idx[:-1] - 300).all() and rows[-1, 0] == 100   # local rows, then the objective row
    bench.write_outputs(str(tmp_path / "o"), {"a": np.arange(3, dtype=np.int64) + 2 ** 40, "b": [1.5]})
    a, b = np.load(tmp_path / "o" / "a.npy"), np.load(tmp_path / "o" / "b.npy")
    assert a.dtype == b.dtype == np.float64 and a.tolist() == [2 ** 40, 2 ** 40 + 1, 2 ** 40 + 2] and b.tolist() == [1.5]
