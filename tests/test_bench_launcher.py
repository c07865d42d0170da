"""bench.py's rank launcher: `python bench.py --gpus N` as a plain command must start N
ranks itself (never a silent 1-GPU run), and a WORLD_SIZE that disagrees with --gpus is an
error.  The CPU half checks launcher and rank plumbing (--rendezvous-only: the ranks meet
on gloo and build their rank-local cases); the GPU half runs the real measurement with
two ranks sharing cuda:0 over the host-staged gloo transport."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(argv, env=None, timeout=900):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + argv, env=e, timeout=timeout,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.parametrize("workload", ["lusgs", "dplur8"])
def test_plain_command_launches_n_ranks(workload):
    r = _run(["--gpus", "2", "--backend", "gloo", "--size", "16", "--workload", workload,
              "--rendezvous-only"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 2 and line["rendezvous_only"] is True
    # chain: one block per rank, one connection between them; dplur8: 8 blocks over 2 ranks
    assert line["blocks_held"] == (2 if workload == "lusgs" else 8)
    assert line["remote_connections"] >= 1


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "4", "--rendezvous-only"], env={"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
    r = _run(["--gpus", "1", "--rendezvous-only"], env={"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_failing_rank_fails_the_command():
    """The ranks are launched and fail there: --size 0 passes the parent's argument parser
    and divides by zero in each rank's rank_local_chain_case (the thin neighbour's thickness
    over n).  The launcher relays the children's failure -- a non-zero return code, the
    child's traceback on stderr."""
    r = _run(["--gpus", "2", "--backend", "gloo", "--size", "0", "--workload", "rk4",
              "--rendezvous-only"], timeout=300)
    assert r.returncode != 0
    assert "ZeroDivisionError" in r.stderr and "rank_local_chain_case" in r.stderr, \
        r.stderr[-2000:]
    # (the parent itself refuses nothing here: its own refusals never reach a rank)
    assert "usage:" not in r.stderr


def test_dump_outputs_writes_state_and_norms(oracle, tmp_path, monkeypatch):
    """--dump-outputs (bench.dump_outputs), here after one oracle iteration of the 8-block
    DPLUR case: every block's physical cells as [cell, equation] and the norms, float64; a
    block above its share of DUMP_CELLS gives the same seeded sample of cells every time."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from aither_amd.solver import Solver
    case = bench.rank_local_chain_case(0, 1, 8, "dplur8")       # 8 blocks of 4^3 cells
    sol = Solver(oracle, case)
    sol.store_time_n(0)
    l2, linf, mres = sol.iterate(0, case.deck.cfl(0))
    bench.dump_outputs(str(tmp_path / "all"), sol, case, 0, 1, l2, linf, mres)
    monkeypatch.setattr(bench, "DUMP_CELLS", 8 * 10)                # 10 of 64 per block
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), sol, case, 0, 1, l2, linf, mres)
    names = sorted(os.listdir(tmp_path / "all"))
    assert names == sorted(["residual_l2sq.npy", "residual_linf.npy", "matrix_residual.npy"]
                           + [f"state_block{b}.npy" for b in range(8)])
    assert sorted(os.listdir(tmp_path / "a")) == names
    for b in range(8):
        full = np.load(tmp_path / "all" / f"state_block{b}.npy")
        g = case.blocks[b].geom.ng
        want = sol.download("state", b)[g:-g, g:-g, g:-g].reshape(64, 5)
        assert full.dtype == np.float64 and np.array_equal(full, want)
        a = np.load(tmp_path / "a" / f"state_block{b}.npy")
        assert a.shape == (10, 5) and np.array_equal(a, np.load(tmp_path / "b" /
                                                                f"state_block{b}.npy"))
        rows = [int(np.flatnonzero((full == r).all(axis=1))[0]) for r in a]
        assert rows == sorted(set(rows))         # distinct cells, in storage order
    assert np.array_equal(np.load(tmp_path / "all" / "residual_l2sq.npy"), l2)
    assert np.load(tmp_path / "all" / "residual_linf.npy")[0] == linf.linf
    assert np.load(tmp_path / "all" / "matrix_residual.npy")[0] == mres
    sol.close()


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_outputs(tmp_path):
    """A plain run measures the headline only (no extra, no cpu_baseline), times exactly
    --steps steps and writes the last one's outputs where --dump-outputs says."""
    import numpy as np
    r = _run(["--gpus", "1", "--size", "32", "--steps", "3", "--warmup", "1",
              "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-3000:]
    line = _json_line(r.stdout)
    assert line["steps"] == 3 and "extra" not in line and "cpu_baseline" not in line
    assert line["value"] * line["ms_per_step"] == pytest.approx(32 ** 3 / 1e3)
    s = np.load(tmp_path / "state_block0.npy")
    assert s.shape == (32 ** 3, 5) and s.dtype == np.float64 and np.all(np.isfinite(s))
    l2 = np.load(tmp_path / "residual_l2sq.npy")
    assert l2.shape == (5,) and np.all(np.isfinite(l2)) and l2.max() > 0


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_plain_command():
    r = _run(["--gpus", "2", "--backend", "gloo", "--size", "32", "--steps", "2",
              "--warmup", "1", "--no-cpu-baseline", "--full"])
    assert r.returncode == 0, r.stderr[-3000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 2 and line["steps"] == 2
    assert "gloo" in line["config"]["halo"]
    assert line["value"] > 0 and line["config"]["cells_per_gpu"] == 32 ** 3
    # the 8-block DPLUR case (strong scaling) rides along for N > 1
    d8 = line["extra"]["dplur8"]
    assert d8["n_gpus"] == 2 and d8["scaling"] == "strong" and d8["value"] > 0
