// agx_switches.hpp -- the AGX_* diagnostic switches: their values, one table, one parser.
//
// No HIP in here: the table is read by agx_ctx_create (agx_api.hip) from the environment and
// by tests/cpp/host_switches.cpp from a map.  This header parses.  Which kernel serves which
// pass is decided where it always was (tile_ok, use_d2, can_fuse, ... in agx_api.hip).
//
// DESIGN.md section 4 carries the same table for readers, one row per variable;
// host_switches.cpp holds the two against each other.
#pragma once
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>

namespace agx {

// What the switches select, with the defaults of a context created in an empty environment.
struct Switches {
  bool use_gather = false;   // AGX_KERNEL=gather: one-thread-per-cell gather kernel
  bool use_tile = true;      // AGX_KERNEL=tile (default) | march
  bool visc_gather = false;  // AGX_VISC=gather: one-thread-per-cell viscous kernel
  bool visc_march = false;   // AGX_VISC=march: face-once form without LDS staging
  bool no_fuse = false;      // AGX_NO_FUSE=1: separate update kernel
  int lusgs_mode = 1;        // AGX_LUSGS=plane (0: launch per hyperplane on the SoA
                             // planes, comparison form) | kp (1, default: agx_lusgs.hpp)
  bool sweep_pipe = true;    // AGX_SWEEP_PIPE=0: one launch per hyperplane
  bool sweep_all_launch = true;  // AGX_SWEEP_ALL=0: the branch streams
  bool sweep_three = true;   // AGX_SWEEP_THREE=0: one lane per cell in the hyperplane sweeps
  bool sweep_records = true; // AGX_SWEEP_RECORDS=0: the hyperplane sweeps read the plane-major arrays
  bool use_graphs = true;    // AGX_GRAPHS=0: launch the hyperplane sweeps one by one
  int spin_limit = 4000000;  // AGX_SPIN_LIMIT: polls before a waiting plane gives up
  bool mresid_march = true;  // AGX_MRESID=plane: one plane position per thread (comparison form)
  int mresid_split = 1;      // bands of diagonals per XCD in k_matrix_resid_d2 (AGX_MRESID_SPLIT)
  // AGX_D2_STATE=update (default): k_update_d2 writes the D2 state of the next iteration and
  // prepare skips the physical cells | prepare: prepare re-lays the state every iteration
  bool d2_state_update = true;
  // AGX_RESID_NORMS=prepare (default): k_lusgs_prepare folds the residual norms and the
  // update does not read the residual | update: k_update_d2 reads it for the norms
  bool resid_norms_prepare = true;
  // AGX_HALO_BATCH=1 (default): local connections exchanged in one gather + one scatter launch
  // per level | 0: a launch pair per connection | require: finalize fails where no batch forms
  bool halo_batch = true;
  bool halo_batch_required = false;
  // AGX_OVERLAP=0: the slabs of x travel before a DPLUR sweep starts (default: while its
  // interior cells are relaxed)
  bool overlap = true;
  bool eager_ghosts = true;  // AGX_EAGER_GHOSTS=0: fill ghost cells at the start of agx_iterate
  int workgroups = 0;        // AGX_WORKGROUPS: persistent workgroups (0: one per CU)
  // the order in which the tile kernels' workgroups visit their (column, k) steps
  // (agx_tile_plan.hpp: 1 TILE_ORDER_STEP, 0 TILE_ORDER_COLUMN); AGX_TILE_ORDER=step|column
  // sets both.  Each kernel's default is the order that measured faster at 256^3
  int tile_order_inv = 1;    // k_residual_tile
  int tile_order_visc = 1;   // k_visc_tile
  bool no_lazy_consn = false;  // AGX_NO_LAZY_CONSN=1: AssignSolToTimeN always a pass of its own
  int ablate = 0;            // AGX_ABLATE (-DAGX_ABLATION builds only): MarchArgs::ablate
};

#ifdef AGX_ABLATION
constexpr bool SWITCHES_ABLATION_BUILD = true;
#else
constexpr bool SWITCHES_ABLATION_BUILD = false;
#endif

// a member of Switches a table entry sets (flags are bool, counts and modes int)
struct SwitchMember {
  bool Switches::*b = nullptr;
  int Switches::*i = nullptr;
  constexpr SwitchMember() {}
  constexpr SwitchMember(bool Switches::*p) : b(p) {}
  constexpr SwitchMember(int Switches::*p) : i(p) {}
  void set(Switches& s, int v) const {
    if (b) s.*b = v != 0;
    else if (i) s.*i = v;
  }
  int get(const Switches& s) const { return b ? (s.*b ? 1 : 0) : i ? s.*i : 0; }
};

enum SwitchKind {
  SWITCH_FLAG,   // atoi(value) != 0
  SWITCH_INT,    // atoi(value) clamped to [lo, hi]
  SWITCH_WORD    // one of `words`, anything else is refused
};

struct SwitchWord { const char* word; int value[2]; };   // what member[0], member[1] become

struct Switch {
  const char* name;
  SwitchKind kind;
  SwitchMember member[2];    // (a word may set two)
  int lo, hi;                // SWITCH_INT
  SwitchWord words[3];       // SWITCH_WORD: the accepted words, the default first
  bool ablation_only;        // read in -DAGX_ABLATION builds only
};

typedef Switches S_;
constexpr Switch SWITCH_TABLE[] = {
  {"AGX_KERNEL", SWITCH_WORD, {&S_::use_gather, &S_::use_tile}, 0, 0,
   {{"tile", {0, 1}}, {"march", {0, 0}}, {"gather", {1, 0}}}, false},
  {"AGX_VISC", SWITCH_WORD, {&S_::visc_gather, &S_::visc_march}, 0, 0,
   {{"tile", {0, 0}}, {"march", {0, 1}}, {"gather", {1, 0}}}, false},
  {"AGX_NO_FUSE", SWITCH_FLAG, {&S_::no_fuse, {}}, 0, 0, {}, false},
  {"AGX_LUSGS", SWITCH_WORD, {&S_::lusgs_mode, {}}, 0, 0,
   {{"kp", {1, 0}}, {"plane", {0, 0}}, {nullptr, {0, 0}}}, false},
  {"AGX_SWEEP_PIPE", SWITCH_FLAG, {&S_::sweep_pipe, {}}, 0, 0, {}, false},
  {"AGX_SWEEP_ALL", SWITCH_FLAG, {&S_::sweep_all_launch, {}}, 0, 0, {}, false},
  {"AGX_SWEEP_THREE", SWITCH_FLAG, {&S_::sweep_three, {}}, 0, 0, {}, false},
  {"AGX_SWEEP_RECORDS", SWITCH_FLAG, {&S_::sweep_records, {}}, 0, 0, {}, false},
  {"AGX_GRAPHS", SWITCH_FLAG, {&S_::use_graphs, {}}, 0, 0, {}, false},
  {"AGX_SPIN_LIMIT", SWITCH_INT, {&S_::spin_limit, {}}, 1, INT_MAX, {}, false},
  {"AGX_MRESID", SWITCH_WORD, {&S_::mresid_march, {}}, 0, 0,
   {{"march", {1, 0}}, {"plane", {0, 0}}, {nullptr, {0, 0}}}, false},
  {"AGX_MRESID_SPLIT", SWITCH_INT, {&S_::mresid_split, {}}, 1, 64, {}, false},
  {"AGX_D2_STATE", SWITCH_WORD, {&S_::d2_state_update, {}}, 0, 0,
   {{"update", {1, 0}}, {"prepare", {0, 0}}, {nullptr, {0, 0}}}, false},
  {"AGX_RESID_NORMS", SWITCH_WORD, {&S_::resid_norms_prepare, {}}, 0, 0,
   {{"prepare", {1, 0}}, {"update", {0, 0}}, {nullptr, {0, 0}}}, false},
  {"AGX_HALO_BATCH", SWITCH_WORD, {&S_::halo_batch, &S_::halo_batch_required}, 0, 0,
   {{"1", {1, 0}}, {"0", {0, 0}}, {"require", {1, 1}}}, false},
  {"AGX_OVERLAP", SWITCH_FLAG, {&S_::overlap, {}}, 0, 0, {}, false},
  {"AGX_EAGER_GHOSTS", SWITCH_FLAG, {&S_::eager_ghosts, {}}, 0, 0, {}, false},
  {"AGX_WORKGROUPS", SWITCH_INT, {&S_::workgroups, {}}, 1, INT_MAX, {}, false},
  {"AGX_TILE_ORDER", SWITCH_WORD, {&S_::tile_order_inv, &S_::tile_order_visc}, 0, 0,
   {{"step", {1, 1}}, {"column", {0, 0}}, {nullptr, {0, 0}}}, false},
  {"AGX_NO_LAZY_CONSN", SWITCH_FLAG, {&S_::no_lazy_consn, {}}, 0, 0, {}, false},
  {"AGX_ABLATE", SWITCH_INT, {&S_::ablate, {}}, INT_MIN, INT_MAX, {}, true},
};
constexpr int N_SWITCHES = (int)(sizeof SWITCH_TABLE / sizeof SWITCH_TABLE[0]);

// A word switch that was given a word it does not know: the variable, the word, and what it
// accepts ("step or column", "tile, march or gather").  `sw` null: every switch parsed.
struct BadSwitch {
  const Switch* sw = nullptr;
  std::string given;
  explicit operator bool() const { return sw != nullptr; }
  std::string accepted() const {
    int n = 0;
    while (n < 3 && sw->words[n].word) ++n;
    std::string r;
    for (int q = 0; q < n; ++q) {
      if (q > 0) r += q == n - 1 ? " or " : ", ";
      r += sw->words[q].word;
    }
    return r;
  }
  std::string message() const {
    return std::string(sw->name) + " is '" + given + "': " + accepted();
  }
};

// Reads every entry of the table through get(name) -> const char* (null: not set), which is
// getenv or a stand-in for it.  A variable that is not set leaves its members as they are.
template <class Get>
BadSwitch parse_switches(Get get, Switches& s) {
  for (const Switch& e : SWITCH_TABLE) {
    if (e.ablation_only && !SWITCHES_ABLATION_BUILD) continue;
    const char* w = get(e.name);
    if (!w) continue;
    if (e.kind == SWITCH_FLAG) {
      e.member[0].set(s, atoi(w) != 0);
    } else if (e.kind == SWITCH_INT) {
      const int v = atoi(w);
      e.member[0].set(s, v < e.lo ? e.lo : v > e.hi ? e.hi : v);
    } else {
      const SwitchWord* hit = nullptr;
      for (const SwitchWord& k : e.words)
        if (k.word && !strcmp(k.word, w)) hit = &k;
      if (!hit) {
        BadSwitch bad;
        bad.sw = &e;
        bad.given = w;
        return bad;
      }
      for (int q = 0; q < 2; ++q) e.member[q].set(s, hit->value[q]);
    }
  }
  return BadSwitch();
}

}  // namespace agx
