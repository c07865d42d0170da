"""Time the time series of aither_amd/csrc/agx_series.hpp on the bench's 256^3 LU-SGS block
(BASELINE configs[2]).  Recorded in DESIGN section 8 "Time series" and
profiles/series_timing.json; a record, no threshold.

    python tools/series_timing.py [--size 256] [--repeats 30] [--out FILE]

  sample     one Solver.series_sample of three plans -- 256 cells x 5 variables, the same with
             the nine velocity gradients, 256 wall faces x 5 wall variables.  host_ms: the
             call alone, no synchronisation (what the time loop pays).  device_ms: `batch`
             samples enqueued back to back, one synchronisation, per sample (what the stream
             pays: the kernel, and for gradient and wall plans the ghost refill before it).
             synced_ms: one sample between two synchronisations (launch latency included).
  iteration  `steps` iterations of the block with a sample of the first plan after every
             iteration against the same without, one synchronisation at the end of each run,
             alternating, median of the runs.
  locate     Solver.series_locate of 1000 points, upload, search and download.

    python tools/series_timing.py --baseline [--size 256] [--repeats 5] [--out FILE]

what a tree without the time series offers for the same numbers (this mode calls nothing of
them, so it runs on the parent commit): Solver.output_pack of the V planes, or wall_pack, and a
numpy gather of the 256 points.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAIN = ["pressure", "vel_x", "vel_y", "vel_z", "density"]
VELGRAD = ["velGrad_" + c for c in ("ux", "vx", "wx", "uy", "vy", "wy", "uz", "vz", "wz")]
WALLV = ["pressure", "shearStress_x", "shearStress_y", "shearStress_z", "heatFlux"]


def points(n, count=256, seed=11):
    import numpy as np
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, size=(count, 3))


def med(values):
    return {"median_ms": statistics.median(values), "min_ms": min(values), "max_ms": max(values)}


def timed(sol, call, repeats, warmup):
    out = []
    for r in range(warmup + repeats):
        sol.api.check(sol.api.sync(sol.ctx))
        t0 = time.perf_counter()
        call()
        sol.api.check(sol.api.sync(sol.ctx))
        if r >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def build(size):
    import aither_amd
    import bench
    from aither_amd.solver import Solver
    case = bench.rank_local_chain_case(0, 1, size, "lusgs")
    print("case built", file=sys.stderr, flush=True)
    sol = Solver(aither_amd.load(case.n_eq), case)
    for nn in range(2):
        sol.step(nn)
    return case, sol


def baseline(args):
    import numpy as np
    case, sol = build(args.size)
    pts = points(args.size)
    faces = np.sort(np.random.default_rng(12).choice(args.size * args.size, 256, replace=False))
    out = {"size": args.size, "repeats": args.repeats,
           "unit": "ms per call, stream-synchronised wall clock"}

    def cells(names):
        return sol.output_pack(0, names)[:, pts[:, 2], pts[:, 1], pts[:, 0]]

    def wall():
        got = sol.wall_pack(0, WALLV)
        return np.stack([np.concatenate([r.ravel() for r in got[n]]) for n in WALLV])[:, faces]

    for key, call in (("cells_5", lambda: cells(PLAIN)),
                      ("cells_5_velgrad_9", lambda: cells(PLAIN + VELGRAD)),
                      ("wall_5", wall)):
        out[key] = med(timed(sol, call, args.repeats, 1))
        print(key, json.dumps(out[key]), file=sys.stderr, flush=True)
    sol.close()
    return out


def tree(args):
    import numpy as np
    case, sol = build(args.size)
    n = args.size
    pts = points(n)
    faces = np.sort(np.random.default_rng(12).choice(n * n, 256, replace=False))
    out = {"size": n, "repeats": args.repeats, "batch": args.batch, "steps": args.steps,
           "unit": "ms"}
    plans = (("cells_5", PLAIN, pts, "cells"),
             ("cells_5_velgrad_9", PLAIN + VELGRAD, pts, "cells"),
             ("wall_5", WALLV, faces, "wall"))
    for key, names, where, kind in plans:
        sol.series_plan(0, names, where, args.batch + 8, kind=kind)
        host, dev = [], []
        for r in range(3 + args.repeats):
            sol.series_drop(0)
            sol.api.check(sol.api.sync(sol.ctx))
            t0 = time.perf_counter()
            for q in range(args.batch):
                sol.series_sample(float(q))
            t1 = time.perf_counter()
            sol.api.check(sol.api.sync(sol.ctx))
            t2 = time.perf_counter()
            if r >= 3:
                host.append((t1 - t0) * 1e3 / args.batch)
                dev.append((t2 - t0) * 1e3 / args.batch)

        def one():
            sol.series_drop(0)
            sol.series_sample(0.0)

        out[key] = {"host_ms": med(host), "device_ms": med(dev),
                    "synced_ms": med(timed(sol, one, args.repeats, 3))}
        print(key, json.dumps(out[key]), file=sys.stderr, flush=True)

    # the benchmark's iteration with and without a sample after every iteration
    sol.series_plan(0, PLAIN, pts, args.steps + 1)
    d = case.deck
    runs = {"plain": [], "sampled": []}
    nn = 2
    for r in range(2 * (1 + args.runs)):
        which = "sampled" if r % 2 else "plain"
        sol.series_drop(0)
        sol.api.check(sol.api.sync(sol.ctx))
        t0 = time.perf_counter()
        for q in range(args.steps):
            sol.step(nn)
            nn += 1
            if which == "sampled":
                sol.series_sample(float(q))
        sol.api.check(sol.api.sync(sol.ctx))
        if r >= 2:
            runs[which].append((time.perf_counter() - t0) * 1e3 / args.steps)
    out["iteration"] = {"nonlinear_iterations": d.nonlinear_iterations,
                        "plain_ms_per_step": med(runs["plain"]),
                        "sampled_ms_per_step": med(runs["sampled"]),
                        "difference_ms": statistics.median(runs["sampled"]) -
                        statistics.median(runs["plain"]),
                        "all_plain": runs["plain"], "all_sampled": runs["sampled"]}
    print("iteration", json.dumps(out["iteration"]), file=sys.stderr, flush=True)

    # locate: 1000 points inside the block's box
    g = case.ng
    cen = sol.download("center", 0)[g:-g, g:-g, g:-g].reshape(-1, 3)
    lo, hi = cen.min(0), cen.max(0)
    cloud = lo + (hi - lo) * np.random.default_rng(13).random((1000, 3))
    del cen
    t = timed(sol, lambda: sol.series_locate(cloud), max(3, args.repeats // 6), 1)
    out["locate_1000"] = dict(med(t), points=1000, cells=n ** 3,
                              state_from_cloud_scale_ms=69.0)
    print("locate", json.dumps(out["locate_1000"]), file=sys.stderr, flush=True)
    sol.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 5 if args.baseline else 30
    text = json.dumps(baseline(args) if args.baseline else tree(args), indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
