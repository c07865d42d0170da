"""Time the boundary-flux call and the block-balance call (aither_amd/csrc/agx_flux.hpp) on the
bench's blocks: stream-synchronised wall clock around the call, median of the repeats after a
warm-up.  Recorded in DESIGN section 8 "Boundary fluxes and the block balance" and profiles/,
no threshold.

    python tools/flux_timing.py [--size 256] [--repeats 30] [--host-repeats 3]
                                [--cases lusgs,rans4] [--out profiles/surface_flux_timing.json]

Cases (bench.py builds them): lusgs, BASELINE configs[2]'s block (WENO + AUSMPW+ + viscous,
the headline workload), and rans4, the four rans blocks.  Per case, over all blocks:
  flux       Solver.surface_fluxes of every id the library gives (11 or 15)
  budget     Solver.block_budget of every id
  host       the only alternative a caller had: Solver.output_pack of the state and the
             residual variables, the download, and the sums in numpy (the balance only; the
             boundary fluxes cannot be had that way at all)
  iteration  one Solver.step of the same case, for scale
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def summary(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "all_ms": t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--cases", default="lusgs,rans4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import aither_amd
    import bench
    from aither_amd import abi
    from aither_amd.solver import Solver
    out = {"size": args.size, "repeats": args.repeats, "host_repeats": args.host_repeats,
           "unit": "ms per call over all blocks, stream-synchronised"}
    for name in args.cases.split(","):
        case = bench.rank_local_chain_case(0, 1, args.size, name)
        print(f"{name}: case built", file=sys.stderr, flush=True)
        sol = Solver(aither_amd.load(case.n_eq), case)
        step = [0]

        def iteration():
            sol.step(step[0])
            step[0] += 1

        t_iter = timed_call(sol, iteration, 5, 2)
        blocks = sorted(sol.block_ids)
        eqs = abi.EQUATIONS[:case.n_eq]
        state_names = ["density", "vel_x", "vel_y", "vel_z", "pressure"] + \
            (["tke", "sdr"] if case.n_eq == 7 else [])
        resid_names = ["resid_" + e for e in eqs]

        def host_path():
            for gb in blocks:
                s = sol.output_pack(gb, state_names + resid_names)
                vol = sol.download("volume", gb)
                g = case.ng
                v = vol[g:-g, g:-g, g:-g, 0]
                rho = s[0]
                sums = [float((rho * v).sum())] + [float((rho * s[c] * v).sum()) for c in (1, 2, 3)]
                sums += [float(r.sum()) for r in s[len(state_names):]]
            return sums

        rec = {"blocks": len(blocks),
               "cells": sum(b.geom.n[0] * b.geom.n[1] * b.geom.n[2] for b in case.blocks),
               "flux_surfaces": sum(len(sol.flux_surfaces(gb)) for gb in blocks),
               "boundary_faces": sum(int(np.prod(s["shape"])) for gb in blocks
                                     for s in sol.flux_surfaces(gb)),
               "flux_ids": len(sol.flux_names()),
               "iteration": summary(t_iter),
               "flux": summary(timed_call(
                   sol, lambda: [sol.surface_fluxes(gb) for gb in blocks], args.repeats, 5)),
               "budget": summary(timed_call(
                   sol, lambda: [sol.block_budget(gb) for gb in blocks], args.repeats, 5)),
               "host": summary(timed_call(sol, host_path, args.host_repeats, 1))}
        out[name] = rec
        print(name, json.dumps({k: (v if not isinstance(v, dict) else v["median_ms"])
                                for k, v in rec.items()}), file=sys.stderr, flush=True)
        sol.close()
        del sol, case
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
