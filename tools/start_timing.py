#!/usr/bin/env python3
"""Wall time of the start-and-resume entries on one node-built euler block, host arrays in,
call returned (the calls synchronise): medians of `repeats` (3), after one untimed call.
python tools/start_timing.py cloud [n] [npts] [repeats]
    agx_state_from_cloud on n^3 cells (128) x npts points (100000), a seeded uniform cloud;
    the work is cells x points.  AGX_LIB=<library> times another build of the library
    (-DAGX_CLOUD_CPT=1, 4: cells of a thread).
python tools/start_timing.py unpack [n] [repeats]
    agx_restart_unpack of an n^3 payload (256) against agx_state_upload of the ghost-padded
    array it stands for."""
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import aither_amd
from aither_amd.case import synthetic
from aither_amd.solver import Solver

what = sys.argv[1] if len(sys.argv) > 1 else "cloud"
args = [int(a) for a in sys.argv[2:]]
api = aither_amd.load(5)


def timed(fn, repeats):
    fn()
    runs = []
    for _ in range(repeats):
        t0 = time.time()
        fn()
        runs.append(time.time() - t0)
    return statistics.median(runs), min(runs), max(runs)


def block(n):
    case = synthetic.single_block_case((n, n, n), stretch=1.2, geometry="device",
                                       initial="device", time_integration="implicitEuler")
    return case, Solver(api, case)


if what == "cloud":
    n, npts, repeats = (args + [128, 100000, 3][len(args):])[:3]
    case, s = block(n)
    rng = np.random.default_rng(1)
    pts = rng.uniform(0.0, 1.0, size=(npts, 3))
    st = rng.uniform(0.5, 1.5, size=(npts, 5))
    far = []
    med, lo, hi = timed(lambda: far.append(s.state_from_cloud(0, pts, st)), repeats)
    print(f"agx_state_from_cloud {n}^3 cells x {npts} points: median {med:.3f} s "
          f"(min {lo:.3f}, max {hi:.3f}); {n ** 3 * npts / med:.3e} cell-point pairs / s; "
          f"max_dist {far[-1]:.6f}", flush=True)
else:
    n, repeats = (args + [256, 3][len(args):])[:2]
    case, s = block(n)
    g = case.ng
    payload = s.restart_pack(0, 0)
    state = s.download("state", 0)
    med, lo, hi = timed(lambda: s.restart_unpack(0, payload, 0), repeats)
    same = np.array_equal(s.download("state", 0)[g:-g, g:-g, g:-g], state[g:-g, g:-g, g:-g])
    print(f"agx_restart_unpack {n}^3 ({payload.nbytes / 1e9:.2f} GB payload): median "
          f"{med:.3f} s (min {lo:.3f}, max {hi:.3f}); unpack(pack(state)) == state: {same}",
          flush=True)
    med, lo, hi = timed(lambda: s.upload("state", 0, state), repeats)
    print(f"agx_state_upload   {n}^3 ({state.nbytes / 1e9:.2f} GB padded array): median "
          f"{med:.3f} s (min {lo:.3f}, max {hi:.3f})", flush=True)
s.close()
