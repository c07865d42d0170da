// agx_out_ranges.hpp -- the one statement of the id ranges of agx_output_pack (their words,
// bounds and precedence) and of the field ranges of agx_field_upload / agx_field_download
// that are not solver fields.  Host decisions only, plain C++17: the entry points dispatch on
// what is said here, and tests/cpp/out_ranges.cpp holds it to the cascade it replaced under
// the host sanitizers.
#pragma once

#include <cstdint>
#include <cstdio>

#include "../../include/aither_gfx950.h"

namespace agx {

// The ranges of agx_output_pack in precedence order: a call holds ids of one range, and of a
// call that mixes two the refusal names the range of highest precedence last ("mine") and the
// next one present first ("other"), but for node with wall ids.  A new range is one row here, one enumerator and one case
// of agx_output_pack's switch.
enum OutRangeId {
  OUT_FLUX, OUT_BUDGET, OUT_CSTAT, OUT_WSTAT, OUT_STAT, OUT_LOAD, OUT_NODE, OUT_WALL, OUT_CELL,
  OUT_RANGES
};
struct OutRange {
  const char* word;     // as the messages say it
  int base, end;        // ids base ... end - 1
  int max_nvar;         // the most ids of a call
  bool function_file;   // WriteFunFile's kinds: "a function file holds one kind"
};
constexpr OutRange OUT_RANGE[OUT_RANGES] = {
    {"flux", AGX_FLUX_BASE, AGX_FLUX_END, AGX_FLUX_END - AGX_FLUX_BASE, false},
    {"budget", AGX_BUDGET_BASE, AGX_BUDGET_END, AGX_BUDGET_END - AGX_BUDGET_BASE, false},
    // (repeated ids are allowed: the bound is the count of variables, not the width)
    {"collapsed statistics", AGX_CSTAT_BASE, AGX_CSTAT_END, AGX_CSTAT_COUNT, false},
    {"wall statistics", AGX_WSTAT_BASE, AGX_WSTAT_END, AGX_WSTAT_END - AGX_WSTAT_BASE, false},
    {"statistics", AGX_STAT_BASE, AGX_STAT_END, AGX_STAT_END - AGX_STAT_BASE, false},
    {"load", AGX_LOAD_BASE, AGX_LOAD_END, AGX_LOAD_END - AGX_LOAD_BASE, false},
    {"node", AGX_NODE_BASE, AGX_NODE_END, AGX_NODE_END - AGX_NODE_BASE, true},
    {"wall", AGX_WALL_YPLUS, AGX_WALL_END, AGX_WALL_END - AGX_WALL_YPLUS, true},
    {"cell", 0, AGX_OUT_COUNT, AGX_OUT_COUNT, true},
};

// the range an id lies in, -1 for none
inline int out_range_of(int var) {
  for (int k = 0; k < OUT_RANGES; ++k)
    if (var >= OUT_RANGE[k].base && var < OUT_RANGE[k].end) return k;
  return -1;
}

// The one range of a call, or (range < 0) the text of its refusal.  In this order: nvar
// outside 1 ... AGX_OUT_COUNT; the first id in list order that lies in no range; ids of two
// ranges; more ids than the range allows.
struct OutCall {
  int range;
  char refusal[160];
};
inline OutCall out_classify(int nvar, const int32_t* vars) {
  OutCall r;
  r.range = -1;
  r.refusal[0] = 0;
  if (nvar < 1 || nvar > AGX_OUT_COUNT) {
    std::snprintf(r.refusal, sizeof r.refusal, "agx_output_pack: nvar %d out of range", nvar);
    return r;
  }
  bool present[OUT_RANGES] = {};
  for (int v = 0; v < nvar; ++v) {
    const int k = out_range_of(vars[v]);
    if (k < 0) {
      std::snprintf(r.refusal, sizeof r.refusal, "unknown output variable %d", vars[v]);
      return r;
    }
    present[k] = true;
  }
  int mine = -1, other = -1;
  for (int k = OUT_RANGES - 1; k >= 0; --k)
    if (present[k]) { other = mine; mine = k; }
  if (other >= 0) {
    // (the one pair the messages have always named the other way round: "node and wall")
    if (mine == OUT_NODE && other == OUT_WALL) { mine = OUT_WALL; other = OUT_NODE; }
    std::snprintf(r.refusal, sizeof r.refusal,
                  "agx_output_pack: %s and %s variables in one call (%s)", OUT_RANGE[other].word,
                  OUT_RANGE[mine].word, OUT_RANGE[mine].function_file
                      ? "a function file holds one kind" : "a call holds ids of one range");
    return r;
  }
  if (nvar > OUT_RANGE[mine].max_nvar) {
    std::snprintf(r.refusal, sizeof r.refusal, "agx_output_pack: nvar %d out of range", nvar);
    return r;
  }
  r.range = mine;
  return r;
}

// The fields of agx_field_upload / agx_field_download that are no solver fields: the time
// statistics, the time series, the spectra.  They write nothing the solver reads.
inline bool field_is_stats(int field) {
  return field == AGX_FIELD_STAT_SAMPLE || field == AGX_FIELD_STAT_ACCUM;
}
inline bool field_is_series(int field) {
  return field >= AGX_FIELD_SERIES_PLAN && field <= AGX_FIELD_SERIES_LOCATE;
}
inline bool field_is_spectra(int field) {
  return field >= AGX_FIELD_SPECTRA_PLAN && field <= AGX_FIELD_SPECTRA_VALUES;
}

}  // namespace agx
