#!/usr/bin/env python3
"""Wall time of the grid set-up, from node coordinates in host memory to a finalized context:
the host pipeline with the library's helpers (build_case(setup=DeviceSetup): device metrics and
wall search, ghost geometry in numpy, nine arrays through agx_block_create) against
build_case(geometry="device") (the nodes alone; everything formed on the device), and that
with initial="device" as well (no state array either: the uniform icState through
agx_state_fill).
python tools/setup_timing.py [n] [repeats]
Two viscous cases: one n^3 block (BASELINE configs[2]; default n = 256) and 2 x 2 x 2 blocks
of (n/2)^3 (configs[3]), each `repeats` (3) times per path in one process: median and spread,
and the peak host RSS.  The peak is the process's high-water mark, so both cases run on the
device paths first, the one without a state array before the other: each path's figures are
its own or an earlier, smaller path's; the host path's are the largest.
Under `rocprofv3 --kernel-trace --stats` the k_ghost_geom / k_edge_geom / k_geo_* /
k_cell_widths / k_metrics_planes / k_nearest_wall_planes rows are the device path."""
import os
import resource
import statistics
import sys
import time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import aither_amd
from aither_amd.case import synthetic
from aither_amd.solver import DeviceSetup, Solver

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
api = aither_amd.load(5)
WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
        4: ("characteristic", 1)}
KW = dict(bcs=WALL, equation_set="navierStokes", time_integration="implicitEuler",
          matrix_solver="dplur", matrix_sweeps=4, cfl=10.0, amplitude=0.0)
CASES = (
    (f"1 x {n}^3", lambda **kw: synthetic.single_block_case((n, n, n), stretch=1.2, **KW, **kw)),
    (f"8 x {n // 2}^3", lambda **kw: synthetic.cube_blocks_case((n // 2,) * 3, (2, 2, 2),
                                                                 **KW, **kw)),
)


def rss_gb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1048576.0


def one(make, path):
    t0 = time.time()
    if path in ("device", "start"):
        case = make(geometry="device", initial="device" if path == "start" else "host")
        t1 = time.time()
        s = Solver(api, case)
    else:
        setup = DeviceSetup(api)
        case = make(setup=setup)
        setup.close()
        t1 = time.time()
        s = Solver(api, case)
    api.check(api.sync(s.ctx), "sync")
    t2 = time.time()
    s.close()
    return t2 - t0, t1 - t0, t2 - t1


for path in ("start", "device", "host"):
    for name, make in CASES:
        runs = [one(make, path) for _ in range(repeats)]
        tot = [r[0] for r in runs]
        print(f"{name} {path:6s}: median {statistics.median(tot):7.2f} s "
              f"(min {min(tot):.2f}, max {max(tot):.2f}; build_case "
              f"{statistics.median(r[1] for r in runs):.2f} s, Solver "
              f"{statistics.median(r[2] for r in runs):.2f} s), peak host RSS so far "
              f"{rss_gb():.2f} GB", flush=True)
