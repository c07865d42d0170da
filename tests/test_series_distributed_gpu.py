"""Time series across ranks: two processes share cuda:0, each holds one block of a stacked
pair (tests/test_distributed_gpu.py's set-up, slabs over gloo).  Each rank locates the
caller's points in its own block, the ranks join what they found (solver.pool_series), each
plans and samples the points it owns, and the pooled record has the points back in the
caller's order."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import series_ref
from aither_amd.case import synthetic
from aither_amd.solver import DistExchange, Solver, pool_series

NAMES = ["pressure", "vel_x", "density"]
N = (7, 5, 3)


def _case(ranks):
    return synthetic.stacked_blocks_case(N, nblocks=2, axis="k", stretch=1.1, ranks=ranks,
                                         time_integration="rk4", cfl=0.5)


def _points():
    """ten points over the box of both blocks, drawn so that the caller's order alternates
    between the blocks"""
    rng = np.random.default_rng(21)
    pts = rng.random((10, 3))
    pts[0::2, 2] *= 0.9                      # (block b spans b <= z <= b + 1)
    pts[1::2, 2] = 1.1 + 0.9 * pts[1::2, 2]
    return pts


def _worker(rank, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    import aither_amd
    case = _case([0, 1])
    sol = Solver(aither_amd.load(5), case, rank=rank, exchange=DistExchange(2))
    (gb,) = sol.block_ids
    local = sol.series_locate(_points())
    parts = [None, None]
    dist.all_gather_object(parts, local)
    where = pool_series(parts)
    mine = sol.series_plan_located(where, NAMES, 4)
    packs = []
    for nn in range(2):
        sol.step(nn)
        sol.series_sample(0.5 * nn)
        packs.append(sol.output_pack(gb, NAMES))
    g = case.ng
    q.put((rank, gb, local, where, {b: sol.series_rows(b) for b in mine}, packs,
           sol.download("center", gb)[g:-g, g:-g, g:-g]))
    dist.barrier()
    sol.close()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_sample_their_own_points_and_pool_them():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        got = q.get(timeout=300)
        res[got[0]] = got[1:]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    pts = _points()
    # every rank located the points in its own block as the reference does, and joined alike
    ref = series_ref.join({res[r][0]: series_ref.nearest(res[r][5], pts) for r in range(2)})
    for r in range(2):
        gb, local, where = res[r][0], res[r][1], res[r][2]
        assert gb == r and np.array_equal(local[:, 0], np.full(len(pts), float(gb)))
        assert np.array_equal(where[:, :4], ref[:, :4])
        assert np.allclose(where[:, 4], ref[:, 4], rtol=4 * 2.0 ** -52, atol=0.0)
    assert np.array_equal(res[0][2], res[1][2])
    where = res[0][2]
    assert where[:, 0].tolist() == [0.0, 1.0] * 5          # the caller's order alternates
    # the pooled record: the points in the caller's order, whichever rank sampled them
    w2, t, vals = pool_series([res[0][1], res[1][1]], records=[res[0][3], res[1][3]])
    assert np.array_equal(w2, where) and t.tolist() == [0.0, 0.5]
    assert vals.shape == (2, len(NAMES), len(pts)) and np.isfinite(vals).all()
    for p, (gb, i, j, k) in enumerate(where[:, :4].astype(int)):
        for row in range(2):
            assert np.array_equal(vals[row, :, p], res[gb][4][row][:, k, j, i]), (p, row)
