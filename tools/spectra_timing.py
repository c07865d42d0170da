"""Time the spectra of aither_amd/csrc/agx_spectra.hpp on the bench's 256^3 LU-SGS block
(BASELINE configs[2]).  Recorded in DESIGN section 8 "Spectra" and
profiles/spectra_timing.json; a record, no threshold.

    python tools/spectra_timing.py [--size 256] [--repeats 30] [--out FILE]

  sample    one Solver.spectra_sample of vel_x, vel_y, vel_z and their three pairs, along i
            and along k, each pooled over one other direction and over both: stream-
            synchronised wall clock around the call, median of `repeats` after 5 warm-ups with
            min and max; flops = lines x modes x N x variables x 4 against the fp64 vector
            peak, bytes (the three planes read once) against 8 TB/s.
  host      what a tree without the spectra offers, in the same session: Solver.output_pack
            of the three variables, numpy.fft.rfft along the direction and the pooling on the
            host (median of `host_repeats`).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UVW = ["vel_x", "vel_y", "vel_z"]
PAIRS = [(0, 1), (0, 2), (1, 2)]
PLANS = [("i", "j"), ("i", "jk"), ("k", "i"), ("k", "ij")]
PEAK_FP64_VECTOR = 78.6e12      # MI355X, flop/s
PEAK_HBM = 8.0e12               # bytes/s


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


def host_spectra(sol, along, over):
    """output_pack of the three variables, rfft and the pooling in numpy"""
    import numpy as np
    pack = sol.output_pack(0, UVW)
    axis = {"i": 3, "j": 2, "k": 1}
    n = pack.shape[axis[along]]
    y = pack - pack.mean(axis=axis[along], keepdims=True)
    f = np.fft.rfft(y, axis=axis[along])
    cm = np.full(n // 2 + 1, 2.0)
    cm[0] = 1.0
    if n % 2 == 0:
        cm[-1] = 1.0
    cm = cm.reshape([-1 if a == axis[along] else 1 for a in range(4)])
    spec = [cm * (f[a] * np.conj(f[b])).real[None] / n ** 2
            for a, b in [(0, 0), (1, 1), (2, 2)] + PAIRS]
    pooled = tuple(axis[d] for d in over)
    return [s.mean(axis=pooled) for s in spec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectra_timing.json"))
    args = ap.parse_args()
    import aither_amd
    import bench
    from aither_amd.solver import Solver
    case = bench.rank_local_chain_case(0, 1, args.size, "lusgs")
    sol = Solver(aither_amd.load(case.n_eq), case)
    for nn in range(2):
        sol.step(nn)
    n = case.blocks[0].geom.n
    cells = n[0] * n[1] * n[2]
    result = {"block": list(n), "variables": UVW, "pairs": PAIRS, "repeats": args.repeats,
              "plans": []}
    for along, over in PLANS:
        big_n = n["ijk".index(along)]
        sol.spectra_plan(0, UVW, PAIRS, along, over)
        t = med(timed(sol, lambda: sol.spectra_sample(1.0), args.repeats, 5))
        flops = (cells // big_n) * (big_n // 2) * big_n * len(UVW) * 4
        nbytes = cells * len(UVW) * 8
        sec = t["median_ms"] * 1e-3
        h = med(timed(sol, lambda: host_spectra(sol, along, over), args.host_repeats, 1))
        entry = {"along": along, "over": over, "sample": t, "flops": flops,
                 "share_of_fp64_vector_peak": flops / sec / PEAK_FP64_VECTOR, "bytes": nbytes,
                 "share_of_hbm_peak": nbytes / sec / PEAK_HBM,
                 "host_output_pack_rfft_pool": dict(h, repeats=args.host_repeats)}
        print(json.dumps(entry), flush=True)
        result["plans"].append(entry)
    sol.close()
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
