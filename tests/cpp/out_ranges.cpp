// The id ranges of agx_output_pack (aither_amd/csrc/agx_out_ranges.hpp) under the address and
// undefined-behaviour sanitizers.  The reference is the classification agx_output_pack held
// before the table: eight counters over nine hand-written ranges and a cascade of five blocks,
// transcribed here with its literal format strings.  It gives the refusal's text or the name
// of the handler; the table's classifier has to give the same, text for text, over every list
// of one, two and three ids drawn from the ranges' boundaries and over every count of one id
// of each range.  What a transcription cannot say is checked beside it: the rows do not
// overlap, and they stand in the order of precedence.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../aither_amd/csrc/agx_out_ranges.hpp"

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("out_ranges: %s failed at line %d\n", #cond, __LINE__);    \
      return 1;                                                              \
    }                                                                        \
  } while (0)

static std::string text(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return buf;
}

// ---- the cascade as it stood (fail(...) -> text(...), a handler's call -> its name) ---------
static std::string cascade(int nvar, const int32_t* vars) {
  if (nvar < 1 || nvar > AGX_OUT_COUNT) return text("agx_output_pack: nvar %d out of range", nvar);
  int n_wall = 0, n_node = 0, n_load = 0, n_stat = 0, n_wstat = 0, n_cstat = 0;
  int n_flux = 0, n_budget = 0;
  for (int v = 0; v < nvar; ++v) {
    const bool flux = vars[v] >= AGX_FLUX_BASE && vars[v] < AGX_FLUX_END;
    const bool budget = vars[v] >= AGX_BUDGET_BASE && vars[v] < AGX_BUDGET_END;
    n_flux += flux;
    n_budget += budget;
    if (flux || budget) continue;
    const bool cell = vars[v] >= 0 && vars[v] < AGX_OUT_COUNT;
    const bool wall = vars[v] >= AGX_WALL_YPLUS && vars[v] < AGX_WALL_END;
    const bool node = vars[v] >= AGX_NODE_BASE && vars[v] < AGX_NODE_END;
    const bool load = vars[v] >= AGX_LOAD_BASE && vars[v] < AGX_LOAD_END;
    const bool stat = vars[v] >= AGX_STAT_BASE && vars[v] < AGX_STAT_END;
    const bool wstat = vars[v] >= AGX_WSTAT_BASE && vars[v] < AGX_WSTAT_END;
    const bool cstat = vars[v] >= AGX_CSTAT_BASE && vars[v] < AGX_CSTAT_END;
    if (!cell && !wall && !node && !load && !stat && !wstat && !cstat)
      return text("unknown output variable %d", vars[v]);
    n_cstat += cstat;
    n_wall += wall;
    n_node += node;
    n_load += load;
    n_stat += stat;
    n_wstat += wstat;
  }
  if (n_flux > 0 || n_budget > 0) {
    const bool is_flux = n_flux > 0;
    const int mine = is_flux ? n_flux : n_budget;
    const char* other = is_flux && n_budget > 0 ? "budget"
                        : n_cstat > 0 ? "collapsed statistics" : n_wstat > 0 ? "wall statistics"
                        : n_stat > 0 ? "statistics" : n_load > 0 ? "load" : n_node > 0 ? "node"
                        : n_wall > 0 ? "wall" : mine != nvar ? "cell" : nullptr;
    if (other)
      return text("agx_output_pack: %s and %s variables in one call (a call holds ids of one "
                  "range)", other, is_flux ? "flux" : "budget");
    if (nvar > AGX_FLUX_END - AGX_FLUX_BASE)
      return text("agx_output_pack: nvar %d out of range", nvar);
    return is_flux ? "surface_fluxes" : "block_budget";
  }
  if (n_cstat > 0) {
    const char* other = n_wstat > 0 ? "wall statistics" : n_stat > 0 ? "statistics"
                        : n_load > 0 ? "load" : n_node > 0 ? "node" : n_wall > 0 ? "wall"
                        : n_cstat != nvar ? "cell" : nullptr;
    if (other)
      return text("agx_output_pack: %s and collapsed statistics variables in one call (a call "
                  "holds ids of one range)", other);
    if (nvar > AGX_CSTAT_COUNT) return text("agx_output_pack: nvar %d out of range", nvar);
    return "stats_collapse";
  }
  if (n_stat > 0 || n_wstat > 0) {
    const char* mine = n_stat > 0 ? "statistics" : "wall statistics";
    if (n_stat > 0 && n_wstat > 0)
      return text("agx_output_pack: statistics and wall statistics variables in one call (a "
                  "call holds ids of one range)");
    const char* other = n_load > 0 ? "load" : n_node > 0 ? "node" : n_wall > 0 ? "wall"
                        : n_stat + n_wstat != nvar ? "cell" : nullptr;
    if (other)
      return text("agx_output_pack: %s and %s variables in one call (a call holds ids of one "
                  "range)", other, mine);
    if (nvar > (n_stat > 0 ? AGX_STAT_END - AGX_STAT_BASE : AGX_WSTAT_END - AGX_WSTAT_BASE))
      return text("agx_output_pack: nvar %d out of range", nvar);
    return n_wstat > 0 ? "stats_pack(wall)" : "stats_pack";
  }
  if (n_load > 0) {
    if (n_node > 0)
      return text("agx_output_pack: node and load variables in one call (a call holds ids of "
                  "one range)");
    if (n_wall > 0)
      return text("agx_output_pack: wall and load variables in one call (a call holds ids of "
                  "one range)");
    if (n_load != nvar)
      return text("agx_output_pack: cell and load variables in one call (a call holds ids of "
                  "one range)");
    if (nvar > AGX_LOAD_END - AGX_LOAD_BASE)
      return text("agx_output_pack: nvar %d out of range", nvar);
    return "wall_loads";
  }
  if (n_node > 0) {
    if (n_wall > 0)
      return text("agx_output_pack: node and wall variables in one call (a function file holds "
                  "one kind)");
    if (n_node != nvar)
      return text("agx_output_pack: cell and node variables in one call (a function file holds "
                  "one kind)");
    return "point_pack(node)";
  }
  if (n_wall > 0) {
    if (n_wall != nvar)
      return text("agx_output_pack: cell and wall variables in one call (a function file holds "
                  "one kind)");
    if (nvar > AGX_WALL_END - AGX_WALL_YPLUS)
      return text("agx_output_pack: nvar %d out of range", nvar);
    return "wall_pack";
  }
  return "point_pack";
}

// ---- the table's answer in the same words: the switch of agx_output_pack ---------------------
static std::string table(int nvar, const int32_t* vars) {
  const agx::OutCall call = agx::out_classify(nvar, vars);
  switch (call.range) {
    case agx::OUT_FLUX: return "surface_fluxes";
    case agx::OUT_BUDGET: return "block_budget";
    case agx::OUT_CSTAT: return "stats_collapse";
    case agx::OUT_WSTAT: return "stats_pack(wall)";
    case agx::OUT_STAT: return "stats_pack";
    case agx::OUT_LOAD: return "wall_loads";
    case agx::OUT_NODE: return "point_pack(node)";
    case agx::OUT_WALL: return "wall_pack";
    case agx::OUT_CELL: return "point_pack";
  }
  return call.refusal;
}

static long g_lists = 0;
static int same(int nvar, const int32_t* vars) {
  const std::string want = cascade(nvar, vars), got = table(nvar, vars);
  ++g_lists;
  if (want == got) return 0;
  std::printf("out_ranges: nvar %d, ids", nvar);
  for (int v = 0; v < nvar && v < 4; ++v) std::printf(" %d", vars[v]);
  std::printf(":\n  the cascade: %s\n  the table:   %s\n", want.c_str(), got.c_str());
  return 1;
}

int main() {
  using agx::OUT_RANGE;
  using agx::OUT_RANGES;
  // the rows: well formed, no two overlap, in the order of precedence
  static const char* const ORDER[] = {"flux", "budget", "collapsed statistics", "wall statistics",
                                      "statistics", "load", "node", "wall", "cell"};
  REQUIRE(OUT_RANGES == (int)(sizeof ORDER / sizeof ORDER[0]));
  for (int a = 0; a < OUT_RANGES; ++a) {
    REQUIRE(std::strcmp(OUT_RANGE[a].word, ORDER[a]) == 0);
    REQUIRE(OUT_RANGE[a].base < OUT_RANGE[a].end);
    REQUIRE(OUT_RANGE[a].max_nvar >= 1 && OUT_RANGE[a].max_nvar <= AGX_OUT_COUNT);
    REQUIRE(OUT_RANGE[a].function_file == (a >= agx::OUT_NODE));
    for (int b = a + 1; b < OUT_RANGES; ++b)
      REQUIRE(OUT_RANGE[a].end <= OUT_RANGE[b].base || OUT_RANGE[b].end <= OUT_RANGE[a].base);
    REQUIRE(agx::out_range_of(OUT_RANGE[a].base) == a);
    REQUIRE(agx::out_range_of(OUT_RANGE[a].end - 1) == a);
  }
  REQUIRE(agx::OUT_FLUX == 0 && agx::OUT_CELL == OUT_RANGES - 1);

  // every list of 1, 2 and 3 boundary ids
  std::vector<int32_t> ids = {-1};
  for (int a = 0; a < OUT_RANGES; ++a)
    for (int id : {OUT_RANGE[a].base - 1, OUT_RANGE[a].base, OUT_RANGE[a].end - 1, OUT_RANGE[a].end})
      ids.push_back(id);
  int32_t list[3];
  for (int32_t x : ids) {
    list[0] = x;
    if (same(1, list)) return 1;
    for (int32_t y : ids) {
      list[1] = y;
      if (same(2, list)) return 1;
      for (int32_t z : ids) {
        list[2] = z;
        if (same(3, list)) return 1;
      }
    }
  }
  // one id of each range n times: both bounds on nvar
  for (int a = 0; a < OUT_RANGES; ++a)
    for (int n = 0; n <= 56; ++n) {
      const std::vector<int32_t> rep((size_t)n, OUT_RANGE[a].base);
      if (same(n, rep.data())) return 1;
    }

  // the field ranges: each field of the header in exactly the range its name says
  int nstat = 0, nseries = 0, nspectra = 0;
  for (int f = -1; f <= AGX_FIELD_SPECTRA_VALUES + 1; ++f) {
    REQUIRE(agx::field_is_stats(f) + agx::field_is_series(f) + agx::field_is_spectra(f) <= 1);
    nstat += agx::field_is_stats(f);
    nseries += agx::field_is_series(f);
    nspectra += agx::field_is_spectra(f);
  }
  REQUIRE(nstat == 2 && nseries == 4 && nspectra == 4);
  REQUIRE(agx::field_is_stats(AGX_FIELD_STAT_SAMPLE) && agx::field_is_stats(AGX_FIELD_STAT_ACCUM));
  REQUIRE(agx::field_is_series(AGX_FIELD_SERIES_PLAN) && agx::field_is_series(AGX_FIELD_SERIES_LOCATE));
  REQUIRE(agx::field_is_spectra(AGX_FIELD_SPECTRA_PLAN) && agx::field_is_spectra(AGX_FIELD_SPECTRA_VALUES));
  REQUIRE(!agx::field_is_stats(AGX_FIELD_STAT_SAMPLE - 1));

  std::printf("out_ranges: %ld lists compared\n", g_lists);
  return 0;
}
