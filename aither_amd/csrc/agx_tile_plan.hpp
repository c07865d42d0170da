// agx_tile_plan.hpp -- which persistent workgroup visits which (column tile, k) step, and when.
//
// k_residual_tile (agx_kernels.hpp) and k_visc_tile (agx_visc_tile.hpp) run one workgroup
// per CU; each marches a share of the block's (column tile, k) steps.  This header is the
// one statement of that share: the number of column tiles, the step sequence, its cut into
// one range per workgroup, the decoding of a range into (column, k0, k1) segments and the
// dealing of ranges to XCDs.  Plain C++ for host and device: the kernels decode with it, the
// host sizes the launch with it and tests/cpp/tile_plan.cpp checks it without a GPU.
//
// Two orders of the same steps:
//   column  the sequence (column, k) cut into P equal ranges: a workgroup marches down one
//           column and on into the next.  Neighbouring columns are then worked on S/P - nk
//           planes apart, so a halo line that two tiles share is long gone from every cache
//           when its second reader arrives.
//   step    the sequence (k-chunk, column, k within the chunk) with a chunk length L chosen
//           so that one column run is one workgroup's share: all columns run at the same k
//           at the same time, and since consecutive ranges go to the same XCD (tile_range_of)
//           neighbours meet in one L2.
// A segment is a run of consecutive k in one column; it ends at the chunk's end, the column's
// end or the range's end, and every segment primes its window.  A priming loads `c` k-planes
// before its first productive step (the per-kernel charges below), so the cut weighs it: every
// column run carries c virtual steps at its head and the VIRTUAL sequence is cut into P equal
// parts.  The column order is the same decoder with L = nk and no virtual steps.
#pragma once

#if defined(__HIPCC__)
#define AGX_TP_HD __host__ __device__
#else
#define AGX_TP_HD
#endif

namespace agx {

enum { TILE_ORDER_COLUMN = 0, TILE_ORDER_STEP = 1 };

// Priming charges: k-planes of state a new segment loads before its first productive step.
// They stand for the cost of a priming in units of a step; that cost has NOT been measured
// (a priming also loads areas and widths, and its loads are not overlapped with arithmetic).
constexpr int TILE_CHARGE_VISC = 3;      // k_visc_tile<false>: planes k0-1, k0, k0+1
constexpr int TILE_CHARGE_VISC_F4 = 5;   // k_visc_tile<true>: planes k0-2 .. k0+2
AGX_TP_HD inline int tile_charge_inviscid(int halo) { return 2 * halo; }   // k_residual_tile: 2H

// cells a workgroup owns per k-step: k_residual_tile 64 x 6, k_visc_tile 62 x 6 (60 x 6 with
// centralFourth, whose window gives two more lanes to the halo)
constexpr int TILE_INV_I = 64, TILE_VISC_I = 62, TILE_VISC_I_F4 = 60, TILE_J = 6;
// column tiles along one direction: n cells, `owned` per tile
AGX_TP_HD inline int tile_count(int n, int owned) { return (n + owned - 1) / owned; }

// The plan as the kernels take it.  c == 0 and L == nk is the column order.
struct TilePlan {
  int tiles;   // column tiles, gx * gy (column = ty * gx + tx)
  int nk;
  int L;       // chunk length, 1 .. nk
  int c;       // virtual steps at the head of every column run
};
struct TileSeg { int col, k0, k1; };
// what is left of a range, in virtual steps.  32 bits: the kernels hold it in two SGPRs across
// their march, and a block of 2^31 steps does not fit a device (tile_plan_make checks)
struct TileWalk { int v, v1; };

AGX_TP_HD inline int tile_plan_chunks(const TilePlan& p) { return (p.nk + p.L - 1) / p.L; }
// length of the virtual sequence
AGX_TP_HD inline long tile_plan_span(const TilePlan& p) {
  return (long)p.tiles * (p.nk + (long)p.c * tile_plan_chunks(p));
}
AGX_TP_HD inline bool tile_plan_is_column(const TilePlan& p) { return p.c == 0 && p.L == p.nk; }
AGX_TP_HD inline TilePlan tile_plan_column(int tiles, int nk) { return TilePlan{tiles, nk, nk, 0}; }

// Workgroup n runs on XCD n % 8: ranges are dealt so that an XCD gets P / 8 consecutive ones
AGX_TP_HD inline int tile_range_of(int wg, int P) {
  return P % 8 == 0 ? (wg % 8) * (P / 8) + wg / 8 : wg;
}
// the XCD group of a range (-1: no dealing, P is no multiple of 8)
AGX_TP_HD inline int tile_xcd_of_range(int r, int P) { return P % 8 == 0 ? r / (P / 8) : -1; }

// range r of P: equal parts of the virtual sequence
AGX_TP_HD inline TileWalk tile_plan_range(const TilePlan& p, int r, int P) {
  const long V = tile_plan_span(p);
  return TileWalk{(int)(V * r / P), (int)(V * (r + 1) / P)};
}
// the next segment of a range; false when the range is done
AGX_TP_HD inline bool tile_plan_next(const TilePlan& p, TileWalk& w, TileSeg& s) {
  const int full = p.tiles * (p.L + p.c);              // virtual steps of a full chunk
  while (w.v < w.v1) {
    const int m = w.v / full;                          // chunk (the last one may be shorter)
    const int kb = m * p.L;
    const int Lm = p.L < p.nk - kb ? p.L : p.nk - kb;
    const int run = (w.v - m * full) / (Lm + p.c);     // column
    const int rs = m * full + run * (Lm + p.c);        // the run's first virtual step
    const int o = w.v - rs - p.c, e = w.v1 - rs - p.c;
    const int ks = o > 0 ? o : 0, ke = e < Lm ? e : Lm;
    w.v = rs + Lm + p.c < w.v1 ? rs + Lm + p.c : w.v1;
    if (ke > ks) {                                     // (else: only virtual steps were left)
      s.col = run; s.k0 = kb + ks; s.k1 = kb + ke;
      return true;
    }
  }
  return false;
}

// cost of the dearest range: steps + charge x segments, a range's own start included
inline long tile_plan_cost(const TilePlan& p, int P, int charge) {
  long worst = 0;
  for (int r = 0; r < P; ++r) {
    TileWalk w = tile_plan_range(p, r, P);
    TileSeg s;
    long cost = 0;
    while (tile_plan_next(p, w, s)) cost += (s.k1 - s.k0) + charge;
    if (cost > worst) worst = cost;
  }
  return worst;
}

// The plan for gx * gy column tiles of nk steps on P workgroups.  The step order is taken
// where it keeps neighbours together at no more than one charge over the column order:
//   * tiles <= P: L is the chunk length for which a run with its charge, L + c, is nearest
//     to one range's share V / P -- and within a step of it, else the ranges drift against
//     the columns and no two neighbours stay in step;
//   * tiles > P: a share q = ceil(S / P) spans ceil(q / nk) runs, L = ceil(q / ceil(q / nk));
//   * the dearest range costs at most the column plan's dearest plus one charge.
// A single column, P < 8 (no XCD dealing worth the name), L >= nk and whatever breaks these
// rules fall back to the column plan.
inline TilePlan tile_plan_make(int gx, int gy, int nk, int P, int charge, int order) {
  const int tiles = gx * gy;
  const TilePlan column = tile_plan_column(tiles, nk);
  if (order != TILE_ORDER_STEP || tiles < 2 || P < 8 || nk < 2) return column;
  // (the virtual sequence is at most (1 + c) times the steps: kept inside TileWalk's 32 bits)
  if ((long)tiles * nk * (1 + charge) > 0x7fffffffL) return column;
  int L = 0;
  if (tiles > P) {
    const long S = (long)tiles * nk, q = (S + P - 1) / P, runs = (q + nk - 1) / nk;
    L = (int)((q + runs - 1) / runs);
  } else {
    long best = -1;
    for (int l = 1; l < nk; ++l) {
      const long d = (long)(l + charge) * P - tile_plan_span(TilePlan{tiles, nk, l, charge});
      const long ad = d < 0 ? -d : d;
      if (best < 0 || ad < best) { best = ad; L = l; }
    }
    if (best > P) return column;                       // |L + c - V / P| > 1
  }
  if (L < 1 || L >= nk) return column;
  const TilePlan step{tiles, nk, L, charge};
  if (tile_plan_cost(step, P, charge) > tile_plan_cost(column, P, charge) + charge) return column;
  return step;
}

}  // namespace agx
