"""Time the viscous group (agx_timing_get, group G_VISC: the viscous residual kernels, here
k_visc_tile) of one block as navierStokes and as largeEddySimulation (WALE), alternated in
one process after a warm-up: RK4, MUSCL + Roe, central viscous reconstruction.
Recorded in DESIGN section 8 "Large-eddy simulation (WALE)" and profiles/, no threshold.

    python tools/les_visc_timing.py [--size 256] [--iters 10] [--repeats 5]
                                    [--baseline-lib PATH] [--out FILE]

--baseline-lib: a libaither_gfx950.so of another commit (the parent); its navierStokes run is
alternated with the two others in the same call.  Prints one JSON object: per run the median
of the repeats' average milliseconds per viscous launch, the smallest and the largest, and the
two ratios.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G_VISC = 4          # agx_api.hip: the timing group of the viscous residual kernels
CHAR = {s: ("characteristic", 1) for s in range(1, 7)}


def visc_ms(sol, iters, nn0):
    """average milliseconds per launch of the viscous group over `iters` RK4 iterations"""
    api = sol.api
    api.check(api.timing_reset(sol.ctx))
    api.check(api.timing_enable(sol.ctx, 1))
    for nn in range(nn0, nn0 + iters):
        sol.step(nn)
    api.check(api.timing_enable(sol.ctx, 0))
    ms, cnt = ctypes.c_double(0.0), ctypes.c_int64(0)
    api.check(api.timing_get(sol.ctx, G_VISC, ctypes.byref(ms), ctypes.byref(cnt)))
    assert cnt.value == 4 * iters, cnt.value
    return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import aither_amd
    from aither_amd import abi
    from aither_amd.case import synthetic
    from aither_amd.solver import Solver
    n = args.size
    case = synthetic.single_block_case((n, n, n), stretch=1.1, bcs=CHAR,
                                       equation_set="navierStokes", time_integration="rk4",
                                       face_reconstruction="thirdOrder", limiter="vanAlbada",
                                       inviscid_flux="roe", cfl=0.4)
    print(f"case {n}^3 built", file=sys.stderr, flush=True)
    lib = aither_amd.load(5)
    runs = {"navierStokes": Solver(lib, case)}
    if args.baseline_lib:
        base = abi.Api(ctypes.CDLL(os.path.abspath(args.baseline_lib)), "agx_")
        runs["navierStokes_baseline"] = Solver(base, case)
    # (the configuration is read when the context is made: the same case, another equation set)
    case.deck.equation_set, case.deck.turbulence_model = "largeEddySimulation", "wale"
    runs["largeEddySimulation"] = Solver(lib, case)
    times = {k: [] for k in runs}
    for key, sol in runs.items():                              # warm-up, untimed
        sol.step(0)
        print(f"{key}: warm", file=sys.stderr, flush=True)
    for r in range(args.repeats):
        for key, sol in runs.items():
            times[key].append(visc_ms(sol, args.iters, 1 + r * args.iters))
    out = {"shape": [n, n, n], "scheme": "rk4, thirdOrder + vanAlbada + roe, central",
           "iterations_per_repeat": args.iters, "repeats": args.repeats,
           "unit": "ms per viscous launch (one RK4 stage)"}
    for key, t in times.items():
        out[key] = {"median": statistics.median(t), "min": min(t), "max": max(t), "all": t}
    out["les_over_navierStokes"] = out["largeEddySimulation"]["median"] / \
        out["navierStokes"]["median"]
    if args.baseline_lib:
        out["navierStokes_over_baseline"] = out["navierStokes"]["median"] / \
            out["navierStokes_baseline"]["median"]
    for sol in runs.values():
        sol.close()
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
