"""Time one Solver.stats_sample (the time statistics of aither_amd/csrc/agx_stats.hpp) on the
bench's blocks: stream-synchronised wall clock around the call, median of the repeats after a
warm-up.  Recorded in DESIGN section 8 "Time statistics" and profiles/, no threshold.

    python tools/stats_timing.py [--size 256] [--repeats 30] [--out FILE]

Cases (bench.py builds them):
  lusgs_farfield  BASELINE configs[2]'s block and scheme with far-field boundaries all round:
                  no wall faces, the sample is k_stats_cells alone
  lusgs           configs[2] as the bench runs it (viscousWall on j-min): the ghost refill of
                  a wall read and k_stats_wall besides
  rans4           the four rans blocks (7 equations, 21 planes)
Per case: ms per sample, bytes per cell (state planes read once, accumulator planes read and
written), the share of the 8 TB/s roofline that is, and the accumulators' device memory.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def timed(sol, repeats, warmup=5):
    api = sol.api
    out = []
    for r in range(warmup + repeats):
        api.check(api.sync(sol.ctx))
        t0 = time.perf_counter()
        sol.stats_sample(1.0)
        api.check(api.sync(sol.ctx))
        if r >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--cases", default="lusgs_farfield,lusgs,rans4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import aither_amd
    import bench
    from aither_amd.case import synthetic
    from aither_amd.solver import Solver
    n = args.size
    out = {"size": n, "repeats": args.repeats, "unit": "ms per stats_sample, all blocks",
           "roofline_bytes_per_s": HBM_BYTES_PER_S}
    for name in args.cases.split(","):
        if name == "lusgs_farfield":
            case = synthetic.single_block_case((n, n, n), stretch=1.2, amplitude=0.05,
                                               **bench.deck_kwargs("lusgs"))
        else:
            case = bench.rank_local_chain_case(0, 1, n, name)
        print(f"{name}: case built", file=sys.stderr, flush=True)
        sol = Solver(aither_amd.load(case.n_eq), case)
        sol.step(0)          # (an iteration first: eddy viscosity, wall data, ghost cells)
        t = timed(sol, args.repeats)
        cells = sum(b.geom.n[0] * b.geom.n[1] * b.geom.n[2] for b in case.blocks)
        planes, wall, _, _ = sol._stat_dims(0)
        state_planes = case.n_eq + (1 if planes - 18 >= 1 else 0)
        bytes_cell = 8 * state_planes + 16 * planes
        med = statistics.median(t)
        out[name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "cells": cells,
                     "blocks": len(case.blocks), "planes": planes,
                     "wall_values_per_face": wall, "bytes_per_cell": bytes_cell,
                     "share_of_roofline": bytes_cell * cells / (med * 1e-3) / HBM_BYTES_PER_S,
                     "accumulator_bytes": planes * 8 * cells, "all_ms": t}
        sol.close()
        del sol, case
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
