"""bench.py's options: a plain run prints the headline line only (the secondary measurements sit behind --full), and
--dump-outputs writes the last timed step's batch (a fixed, seeded sample of its rows) as float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _load(d, name):
    a = np.load(os.path.join(d, name + ".npy"))
    assert a.dtype == np.float64
    return a.astype(np.int64)


def test_options_default_to_a_plain_run():
    a = bench.parse_args([])
    assert a.full is False and a.dump_outputs is None and a.steps == 10 and a.warmup == 3
    a = bench.parse_args(["--full", "--dump-outputs", "out", "--steps", "7"])
    assert a.full is True and a.dump_outputs == "out" and a.steps == 7


@pytest.mark.parametrize("rows,max_edges", [(1000, 12), (200_000, 30), (50_000, 400)])
def test_dump_writes_the_sampled_rows_of_the_batch(tmp_path, rows, max_edges):
    """CPU tensors stand in for the device batch: every written array is the exact slice of the batch it names, the same
    rows are picked from run to run, and the files stay within the byte budget (rows with many edges: fewer rows)."""
    import torch
    rng = np.random.default_rng(rows)
    k = 8
    cnt = rng.integers(0, max_edges, rows)
    eptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    cap = int(eptr[-1]) + 777                                     # edge buffers longer than the batch's edges, as on the device
    eidx = rng.integers(0, 1 << 40, (2, cap))
    esrc = rng.integers(0, k, cap)
    nodes = rng.integers(-1, 1 << 40, (rows, k))
    batch = tuple(torch.from_numpy(x) for x in (nodes, eidx, eptr, esrc))
    info = bench.dump_outputs(torch, np, str(tmp_path / "a"), batch)
    again = bench.dump_outputs(torch, np, str(tmp_path / "b"), batch)
    assert info["bytes"] <= bench.DUMP_BYTES and info["rows"] == again["rows"] > 0
    d = str(tmp_path / "a")
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) < 64 << 20
    r = _load(d, "rows")
    assert np.array_equal(r, _load(str(tmp_path / "b"), "rows")) and np.all(np.diff(r) > 0) and r[0] >= 0 and r[-1] < rows
    if max_edges == 400:                                           # about 4.8 kB per row: the budget, not DUMP_ROWS, sets the count
        assert len(r) < rows and info["bytes"] > bench.DUMP_BYTES * 0.9
    else:
        assert len(r) == min(rows, bench.DUMP_ROWS)
    assert np.array_equal(_load(d, "nodes"), nodes[r])
    ep, cc = _load(d, "edge_ptr"), _load(d, "edge_count")
    assert np.array_equal(ep[:-1], eptr[r]) and ep[-1] == eptr[-1] and np.array_equal(cc, cnt[r])
    sel = np.concatenate([np.arange(eptr[i], eptr[i + 1]) for i in r])
    assert np.array_equal(_load(d, "edge_index"), eidx[:, sel]) and np.array_equal(_load(d, "edge_src"), esrc[sel])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run on the PROTEINS-shaped batch (8192 rows: all of them dumped): the headline keys and nothing of --full,
    and the dumped batch is the CPU oracle's for the last timed step's seed (42 + warmup + steps - 1)."""
    import oracle
    import ugs_workloads as wl
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c3_proteins_b8192", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", out], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(key in line for key in HEADLINE) and line["steps"] == 3 and line["ms_per_step"] > 0 and line["full"] is False
    assert not any(key in line for key in ("roofline", "cpu_baseline", "other_workloads", "drop_in_call", "summary"))
    ei, ptr, m, k = wl.workload("c3_proteins_b8192")
    nodes, eidx, eptr, _, esrc = oracle.sample_batch(ei, ptr, m, k, "sample", 42 + 2 + 3 - 1)
    rows = _load(out, "rows")
    assert np.array_equal(rows, np.arange(nodes.shape[0]))
    assert np.array_equal(_load(out, "nodes"), nodes) and np.array_equal(_load(out, "edge_ptr"), eptr)
    assert np.array_equal(_load(out, "edge_count"), np.diff(eptr))
    ne = int(eptr[-1])
    assert np.array_equal(_load(out, "edge_index"), eidx[:, :ne]) and np.array_equal(_load(out, "edge_src"), esrc[:ne])
