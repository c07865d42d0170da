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

    python tools/stats_timing.py --collapse [--size 256] [--repeats 30] [--host-repeats 3]
                                 [--out profiles/stats_collapse_timing.json]

times Solver.stats_collapse of every id the context keeps on the lusgs block (configs[2]:
navierStokes, 18 planes) for over = "k", "i", "ik" and "ijk", against what the library offered
before it: Solver.stats_pack of the same ids and the numpy reduction of
tests/collapse_ref.two_pass in float64 on the host (host-repeats after one warm-up: a pass over
2.4 GB takes seconds).  Per direction set: both medians, the bytes the device moves (the
planes and the volumes read once, the chunk records written and read) with their share of the
roofline, and the bytes that cross PCIe on either path.  A record, no threshold.
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


def timed_call(sol, call, repeats, warmup):
    api = sol.api
    out = []
    for r in range(warmup + repeats):
        api.check(api.sync(sol.ctx))
        t0 = time.perf_counter()
        call()
        api.check(api.sync(sol.ctx))
        if r >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def collapse_timing(args):
    import numpy as np
    import aither_amd
    import bench
    from aither_amd import abi
    from aither_amd.solver import Solver
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import collapse_ref
    n = args.size
    case = bench.rank_local_chain_case(0, 1, n, "lusgs")
    print("lusgs: case built", file=sys.stderr, flush=True)
    sol = Solver(aither_amd.load(case.n_eq), case)
    sol.step(0)
    for w in (1.0, 0.5):
        sol.stats_sample(w)
    planes, _, cells, _ = sol._stat_dims(0)
    names = list(abi.STAT_OUT)[:9] + list(abi.STAT_OUT)[12:]
    assert len(names) == planes
    ni, nj, nk = case.blocks[0].geom.n
    g = case.ng
    vol = np.ascontiguousarray(sol.download("volume", 0)[g:-g, g:-g, g:-g, 0]) * \
        sol.cfg.gas.l_ref ** 3
    out = {"size": n, "cells": cells, "ids": len(names), "repeats": args.repeats,
           "host_repeats": args.host_repeats, "unit": "ms per call, stream-synchronised",
           "roofline_bytes_per_s": HBM_BYTES_PER_S, "chunk": abi.CSTAT_CHUNK}

    def host_path(mask):
        cell = dict(zip(names, sol.stats_pack(0, names)))
        means = {k: collapse_ref.to_bins(v, mask) for k, v in cell.items() if k.startswith("mean_")}
        coms = {abi.STAT_PAIRS[k]: collapse_ref.to_bins(v, mask) for k, v in cell.items()
                if k in abi.STAT_PAIRS}
        return collapse_ref.two_pass(collapse_ref.to_bins(vol, mask), means, coms,
                                     dtype=np.float64)

    for over in ("k", "i", "ik", "ijk"):
        mask = abi.cstat_mask(over)
        t = timed_call(sol, lambda: sol.stats_collapse(0, names, over), args.repeats, 5)
        th = timed_call(sol, lambda: host_path(mask), args.host_repeats, 1)
        tp = timed_call(sol, lambda: sol.stats_pack(0, names), args.host_repeats, 1)
        nbin = cells // ((ni if mask & 1 else 1) * (nj if mask & 2 else 1) * (nk if mask & 4 else 1))
        steps = (nj if mask & 2 else 1) * (nk if mask & 4 else 1)
        nchunk = -(-steps // abi.CSTAT_CHUNK)
        records = nchunk * nbin * (1 + 9 + 18)
        moved = 8 * ((planes + 1) * cells + 2 * records)
        med = statistics.median(t)
        out[over] = {"device_median_ms": med, "device_min_ms": min(t), "device_max_ms": max(t),
                     "bins": nbin, "chunks": nchunk, "device_bytes_moved": moved,
                     "share_of_roofline": moved / (med * 1e-3) / HBM_BYTES_PER_S,
                     "device_bytes_to_host": 8 * len(names) * nbin,
                     "host_median_ms": statistics.median(th), "host_all_ms": th,
                     "host_stats_pack_median_ms": statistics.median(tp),
                     "host_bytes_to_host": 8 * len(names) * cells,
                     "speedup": statistics.median(th) / med, "device_all_ms": t}
        print(over, json.dumps({k: v for k, v in out[over].items() if not k.endswith("all_ms")}),
              file=sys.stderr, flush=True)
    sol.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--collapse", action="store_true")
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--cases", default="lusgs_farfield,lusgs,rans4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.collapse:
        text = json.dumps(collapse_timing(args), indent=1)
        print(text, flush=True)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(text + "\n")
        return
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
