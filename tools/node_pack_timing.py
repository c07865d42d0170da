"""Time the nodal function file against its yardsticks (recorded in DESIGN section 8 f1, no
threshold): the nodal call (k_node_grads + k_node_pack), the cell call of the same names
(k_cell_grads + k_output_pack), and the host alternative -- download("state") plus the numpy
gather of tests/node_ref.py for the five state variables.  One viscous laminar block of 128^3
and of 256^3, the five state variables plus the nine velocity gradients; medians of three after
one untimed call.  Prints one JSON line per shape with the times and the bytes over PCIe.

    python tools/node_pack_timing.py [--sizes 128 256]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ["density", "vel_x", "vel_y", "vel_z", "pressure"] + \
    ["velGrad_" + c for c in ("ux", "vx", "wx", "uy", "vy", "wy", "uz", "vz", "wz")]
WALL = {3: ("viscousWall", 2), 1: ("characteristic", 1), 2: ("characteristic", 1),
        4: ("characteristic", 1), 5: ("characteristic", 1), 6: ("characteristic", 1)}


def median3(fn):
    fn()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    args = ap.parse_args()
    import aither_amd
    import node_ref
    from aither_amd.case import synthetic
    from aither_amd.solver import Solver
    lib = aither_amd.load(5)
    for n in args.sizes:
        case = synthetic.single_block_case((n, n, n), stretch=1.1, bcs=WALL,
                                           equation_set="navierStokes",
                                           time_integration="implicitEuler",
                                           matrix_solver="lusgs", cfl=5.0)
        sol = Solver(lib, case)
        sol.step(0)
        ng = case.ng

        def host():
            st = node_ref._ijk(sol.download("state", 0))
            cells = node_ref.assign_corner_ghosts(node_ref.first_layer(st, ng))
            return node_ref.gather8(cells) * 0.125

        t_node = median3(lambda: sol.node_pack(0, NAMES))
        t_cell = median3(lambda: sol.output_pack(0, NAMES))
        t_host = median3(host)
        print(json.dumps({
            "shape": [n, n, n], "variables": len(NAMES),
            "node_pack_s": t_node, "cell_pack_s": t_cell, "host_state_gather_s": t_host,
            "node_pack_pcie_bytes": 8 * len(NAMES) * (n + 1) ** 3,
            "cell_pack_pcie_bytes": 8 * len(NAMES) * n ** 3,
            "host_pcie_bytes": 8 * 5 * (n + 2 * ng) ** 3}), flush=True)
        sol.close()


if __name__ == "__main__":
    main()
