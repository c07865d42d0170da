// tile_plan.cpp -- the tile kernels' plan (aither_amd/csrc/agx_tile_plan.hpp) on the host.
//
// For both orders, the kernels' charges and a range of workgroup counts: every (column, k)
// step is in exactly one segment of one range, segments are runs of k inside one column
// (and, in the step order, inside one chunk), the column order is the equal cut of the
// (column, k) sequence, the dearest range stays within one charge of the column plan's, and
// at the headline shape the step order brings neighbouring columns together in time and on
// one XCD.  Built with -fsanitize=address,undefined by tests/test_tile_plan_host.py.
#include "../../aither_amd/csrc/agx_tile_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <random>
#include <vector>

using namespace agx;

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (++g_fail <= 20) {                               \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__);  \
        std::printf(__VA_ARGS__);                         \
        std::printf("\n");                                \
      }                                                   \
    }                                                     \
  } while (0)

struct Visit { int range; long time; };

// walks every range of the plan; visits[col * nk + k] = (range, modelled time: a range's
// clock starts at 0, a segment costs `charge` before its first step, a step costs 1)
static bool walk(const TilePlan& p, int P, int charge, std::vector<Visit>& visits,
                 std::vector<long>* col_pos, long* worst) {
  const long S = (long)p.tiles * p.nk;
  visits.assign((size_t)S, Visit{-1, 0});
  bool ok = true;
  *worst = 0;
  for (int r = 0; r < P; ++r) {
    TileWalk w = tile_plan_range(p, r, P);
    TileSeg s;
    long t = 0;
    while (tile_plan_next(p, w, s)) {
      if (!(s.col >= 0 && s.col < p.tiles && s.k0 >= 0 && s.k0 < s.k1 && s.k1 <= p.nk)) {
        CHECK(false, "segment (%d, %d, %d) outside %d columns x %d", s.col, s.k0, s.k1, p.tiles, p.nk);
        return false;
      }
      // inside one chunk
      if (s.k0 / p.L != (s.k1 - 1) / p.L) {
        CHECK(false, "segment (%d, %d, %d) crosses a chunk of %d", s.col, s.k0, s.k1, p.L);
        ok = false;
      }
      t += charge;
      for (int k = s.k0; k < s.k1; ++k, ++t) {
        Visit& v = visits[(size_t)s.col * p.nk + k];
        if (v.range != -1) {
          CHECK(false, "step (%d, %d) visited twice (ranges %d and %d)", s.col, k, v.range, r);
          ok = false;
        }
        v = Visit{r, t};
        if (col_pos) col_pos->push_back((long)s.col * p.nk + k);
      }
    }
    if (t > *worst) *worst = t;
    if (col_pos) col_pos->push_back(-1 - r);           // end of range r
  }
  for (long q = 0; q < S; ++q)
    if (visits[(size_t)q].range == -1) {
      CHECK(false, "step (%ld, %ld) of %d x %d not visited (P = %d, L = %d, c = %d)", q / p.nk,
            q % p.nk, p.tiles, p.nk, P, p.L, p.c);
      return false;
    }
  return ok;
}

static long g_plans = 0, g_step_plans = 0;

static void check_plan(int gx, int gy, int nk, int P, int charge) {
  const int tiles = gx * gy;
  const long S = (long)tiles * nk;
  std::vector<Visit> vis;
  long cost_col = 0, cost_step = 0;
  // ---- column: the equal cut [S r / P, S (r + 1) / P) of the (column, k) sequence ----
  const TilePlan col = tile_plan_make(gx, gy, nk, P, charge, TILE_ORDER_COLUMN);
  CHECK(tile_plan_is_column(col) && col.tiles == tiles && col.nk == nk, "column plan malformed");
  std::vector<long> pos;
  walk(col, P, charge, vis, &pos, &cost_col);
  {
    size_t n = 0;
    for (int r = 0; r < P; ++r) {
      for (long s = S * r / P; s < S * (r + 1) / P; ++s, ++n)
        CHECK(n < pos.size() && pos[n] == s, "column range %d of %d: step %ld out of place", r, P, s);
      CHECK(n < pos.size() && pos[n] == -1 - r, "column range %d of %d has more steps than its cut", r, P);
      ++n;
    }
  }
  CHECK(cost_col == tile_plan_cost(col, P, charge), "tile_plan_cost disagrees with the walk");
  // ---- step ----
  const TilePlan st = tile_plan_make(gx, gy, nk, P, charge, TILE_ORDER_STEP);
  CHECK(st.tiles == tiles && st.nk == nk && st.L >= 1 && st.L <= nk, "step plan malformed");
  walk(st, P, charge, vis, nullptr, &cost_step);
  CHECK(cost_step <= cost_col + charge, "%d x %d x %d, P %d, c %d: dearest range %ld > %ld + %d",
        gx, gy, nk, P, charge, cost_step, cost_col, charge);
  ++g_plans;
  if (!tile_plan_is_column(st)) {
    ++g_step_plans;
    CHECK(st.c == charge && st.L < nk, "step plan with L = %d, c = %d", st.L, st.c);
    if (tiles <= P) {
      // a chunk-0 run plus its charge is one range's share to within a step
      const double share = (double)tile_plan_span(st) / P;
      CHECK(std::fabs(st.L + charge - share) <= 1.0, "%d x %d x %d, P %d: L + c = %d, share %.2f",
            gx, gy, nk, P, st.L + charge, share);
    }
  }
}

// share of (tile, k, i- or j-neighbour) pairs whose modelled times differ by at most two
// steps, and the share that is moreover dealt to one XCD
static void neighbours(const TilePlan& p, int gx, int gy, int P, int charge, double* near,
                       double* near_xcd) {
  std::vector<Visit> vis;
  long worst;
  walk(p, P, charge, vis, nullptr, &worst);
  long pairs = 0, n_near = 0, n_xcd = 0;
  for (int ty = 0; ty < gy; ++ty)
    for (int tx = 0; tx < gx; ++tx)
      for (int d = 0; d < 2; ++d) {
        const int ux = tx + (d == 0), uy = ty + (d == 1);
        if (ux >= gx || uy >= gy) continue;
        for (int k = 0; k < p.nk; ++k) {
          const Visit& a = vis[(size_t)(ty * gx + tx) * p.nk + k];
          const Visit& b = vis[(size_t)(uy * gx + ux) * p.nk + k];
          ++pairs;
          if (std::labs(a.time - b.time) <= 2) {
            ++n_near;
            if (tile_xcd_of_range(a.range, P) == tile_xcd_of_range(b.range, P)) ++n_xcd;
          }
        }
      }
  *near = (double)n_near / pairs;
  *near_xcd = (double)n_xcd / pairs;
}

int main() {
  const int Ps[] = {1, 3, 8, 24, 27, 256};
  const int charges[] = {TILE_CHARGE_VISC, TILE_CHARGE_VISC_F4, tile_charge_inviscid(2),
                         tile_charge_inviscid(3)};
  const int shapes[][3] = {{131, 15, 9}, {65, 5, 3}, {1, 1, 40}, {2, 3, 1}, {300, 40, 7},
                           {256, 256, 256}, {512, 512, 512}};
  const int owned_i[] = {TILE_VISC_I, TILE_VISC_I_F4, TILE_INV_I};
  for (int P : Ps)
    for (int c : charges) {
      for (const auto& s : shapes)
        for (int oi : owned_i)
          check_plan(tile_count(s[0], oi), tile_count(s[1], TILE_J), s[2], P, c);
      // the headline plans spelled out: 5 x 43 tiles of 62 x 6, 4 x 43 tiles of 64 x 6
      check_plan(5, 43, 256, P, c);
      check_plan(4, 43, 256, P, c);
    }
  std::mt19937 rng(20240611u);
  for (int n = 0; n < 400; ++n) {
    const int gx = 1 + (int)(rng() % 12), gy = 1 + (int)(rng() % 50);
    const int nkmax = 60000 / (gx * gy);
    const int nk = 1 + (int)(rng() % (unsigned)std::min(nkmax, n % 2 ? 600 : 40));
    const int P = Ps[rng() % 6], c = charges[rng() % 4];
    check_plan(gx, gy, nk, P, c);
  }
  // ---- the shapes tests/test_tile_order_gpu.py runs under both orders do take the step
  // order: (131, 15, 9) on 8 workgroups (nine tiles, q = 11, L = 6: two chunks, ranges that
  // cross columns) with the viscous and the MUSCL charge, (65, 7, 20) with centralFourth's ----
  {
    const TilePlan a = tile_plan_make(3, 3, 9, 8, TILE_CHARGE_VISC, TILE_ORDER_STEP);
    CHECK(a.L == 6 && a.c == TILE_CHARGE_VISC, "(131, 15, 9) viscous on 8: L = %d, c = %d", a.L, a.c);
    const TilePlan m = tile_plan_make(3, 3, 9, 8, tile_charge_inviscid(2), TILE_ORDER_STEP);
    CHECK(m.L == 6 && m.c == 4, "(131, 15, 9) MUSCL on 8: L = %d, c = %d", m.L, m.c);
    const TilePlan f = tile_plan_make(2, 2, 20, 8, TILE_CHARGE_VISC_F4, TILE_ORDER_STEP);
    CHECK(f.L == 10 && f.c == TILE_CHARGE_VISC_F4, "(65, 7, 20) centralFourth on 8: L = %d, c = %d",
          f.L, f.c);
  }
  // ---- the headline shape, 256^3 on 256 workgroups ----
  double near, near_xcd;
  {
    const TilePlan v = tile_plan_make(5, 43, 256, 256, TILE_CHARGE_VISC, TILE_ORDER_STEP);
    neighbours(v, 5, 43, 256, TILE_CHARGE_VISC, &near, &near_xcd);
    std::printf("viscous 256^3: L = %d, neighbour pairs within two steps %.3f, and on one XCD %.3f\n",
                v.L, near, near_xcd);
    CHECK(!tile_plan_is_column(v), "the viscous headline plan fell back to column");
    CHECK(near >= 0.75, "viscous pairs within two steps: %.3f < 0.75", near);
    CHECK(near_xcd >= 0.7, "viscous pairs on one XCD: %.3f < 0.7", near_xcd);
    const TilePlan vc = tile_plan_make(5, 43, 256, 256, TILE_CHARGE_VISC, TILE_ORDER_COLUMN);
    neighbours(vc, 5, 43, 256, TILE_CHARGE_VISC, &near, &near_xcd);
    std::printf("viscous 256^3, column: %.3f\n", near);
  }
  {
    const int c = tile_charge_inviscid(3);
    const TilePlan v = tile_plan_make(4, 43, 256, 256, c, TILE_ORDER_STEP);
    neighbours(v, 4, 43, 256, c, &near, &near_xcd);
    std::printf("inviscid 256^3: L = %d, neighbour pairs within two steps %.3f, and on one XCD %.3f\n",
                v.L, near, near_xcd);
    CHECK(!tile_plan_is_column(v), "the inviscid headline plan fell back to column");
    CHECK(near >= 0.6, "inviscid pairs within two steps: %.3f < 0.6", near);
  }
  std::printf("%ld plans checked, %ld of them in the step order\n", g_plans, g_step_plans);
  CHECK(g_step_plans > 50, "too few shapes took the step order for the checks to mean much");
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("tile plan OK\n");
  return 0;
}
