// host_switches.cpp -- the switch table of aither_amd/csrc/agx_switches.hpp, fed from a map:
// defaults, every accepted word and what it sets, the refusal of any other word, atoi
// semantics of the flags, the clamps, and the table of DESIGN.md section 4 against the
// code's (argv[1]: DESIGN.md).  Built with the address and undefined-behaviour sanitizers;
// exits non-zero unless every property holds.
#include "../../aither_amd/csrc/agx_switches.hpp"
#include <cstdio>
#include <fstream>
#include <map>
#include <set>
#include <string>
#include <vector>

using namespace agx;

namespace {
int failures = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) { printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

typedef std::map<std::string, std::string> Env;
struct Parsed { Switches s; BadSwitch bad; };
Parsed parse(const Env& env) {
  Parsed p;
  p.bad = parse_switches(
      [&](const char* name) -> const char* {
        auto it = env.find(name);
        return it == env.end() ? nullptr : it->second.c_str();
      },
      p.s);
  return p;
}
const Switch* entry(const std::string& name) {
  for (const Switch& e : SWITCH_TABLE)
    if (name == e.name) return &e;
  return nullptr;
}

// what a context held before any switch was read, per variable: the members the entry sets
// (the second one of an entry that sets one member: 0)
struct Default { const char* name; int v0, v1; };
const Default DEFAULTS[] = {
  {"AGX_KERNEL", 0, 1},          // use_gather = false, use_tile = true
  {"AGX_VISC", 0, 0},            // visc_gather = false, visc_march = false
  {"AGX_NO_FUSE", 0, 0},         // no_fuse = false (was: allow_fuse = true)
  {"AGX_LUSGS", 1, 0},           // lusgs_mode = 1
  {"AGX_SWEEP_PIPE", 1, 0},      // sweep_pipe = true
  {"AGX_SWEEP_ALL", 1, 0},       // sweep_all_launch = true
  {"AGX_SWEEP_THREE", 1, 0},     // sweep_three = true
  {"AGX_SWEEP_RECORDS", 1, 0},   // sweep_records = true
  {"AGX_GRAPHS", 1, 0},          // use_graphs = true
  {"AGX_SPIN_LIMIT", 4000000, 0},
  {"AGX_MRESID", 1, 0},          // mresid_march = true
  {"AGX_MRESID_SPLIT", 1, 0},
  {"AGX_D2_STATE", 1, 0},        // d2_state_update = true
  {"AGX_RESID_NORMS", 1, 0},     // resid_norms_prepare = true
  {"AGX_HALO_BATCH", 1, 0},      // halo_batch = true, halo_batch_required = false
  {"AGX_OVERLAP", 1, 0},         // overlap = true
  {"AGX_EAGER_GHOSTS", 1, 0},    // eager_ghosts = true
  {"AGX_WORKGROUPS", 0, 0},      // num_cu: the device's CU count (0: not given)
  {"AGX_TILE_ORDER", 1, 1},      // tile_order_inv = tile_order_visc = TILE_ORDER_STEP (1)
  {"AGX_NO_LAZY_CONSN", 0, 0},   // lazy = true
  {"AGX_ABLATE", 0, 0},          // ma.ablate = 0
};

// every word of every word switch, and the members it gives
struct WordCase { const char* name; const char* word; int v0, v1; };
const WordCase WORDS[] = {
  {"AGX_KERNEL", "tile", 0, 1},      {"AGX_KERNEL", "march", 0, 0},
  {"AGX_KERNEL", "gather", 1, 0},    {"AGX_VISC", "tile", 0, 0},
  {"AGX_VISC", "march", 0, 1},       {"AGX_VISC", "gather", 1, 0},
  {"AGX_LUSGS", "kp", 1, 0},         {"AGX_LUSGS", "plane", 0, 0},
  {"AGX_MRESID", "march", 1, 0},     {"AGX_MRESID", "plane", 0, 0},
  {"AGX_HALO_BATCH", "1", 1, 0},     {"AGX_HALO_BATCH", "0", 0, 0},
  {"AGX_HALO_BATCH", "require", 1, 1},
  {"AGX_TILE_ORDER", "step", 1, 1},  {"AGX_TILE_ORDER", "column", 0, 0},
  {"AGX_D2_STATE", "update", 1, 0},  {"AGX_D2_STATE", "prepare", 0, 0},
  {"AGX_RESID_NORMS", "prepare", 1, 0}, {"AGX_RESID_NORMS", "update", 0, 0},
};
const char* const WORD_SWITCHES[] = {"AGX_KERNEL", "AGX_VISC", "AGX_LUSGS", "AGX_MRESID",
                                     "AGX_HALO_BATCH", "AGX_TILE_ORDER", "AGX_D2_STATE",
                                     "AGX_RESID_NORMS"};

// the variables of the rows of DESIGN.md's switch table: `| \`AGX_NAME\` | ... |` lines after
// the "**Diagnostic switches**" paragraph, up to the end of the table
std::vector<std::string> design_rows(const char* path) {
  std::vector<std::string> rows;
  std::ifstream f(path);
  std::string line;
  bool in_section = false, in_table = false;
  while (std::getline(f, line)) {
    if (line.find("**Diagnostic switches**") != std::string::npos) in_section = true;
    if (!in_section) continue;
    const bool row = line.compare(0, 1, "|") == 0;
    if (in_table && !row) break;
    if (!row) continue;
    in_table = true;
    if (line.compare(0, 3, "| `") != 0) continue;        // (the header and the rule)
    const size_t a = 3, b = line.find('`', a);
    const std::string cell = line.substr(a, b == std::string::npos ? b : b - a);
    const size_t bar = line.find('|', 1);
    // one variable per row: nothing but the name in the first cell
    CHECK(bar != std::string::npos && line.substr(0, bar) == "| `" + cell + "` ");
    rows.push_back(cell);
  }
  return rows;
}
}  // namespace

int main(int argc, char** argv) {
  {   // defaults: an empty environment leaves every member what a context always started with
    const Parsed p = parse({});
    CHECK(!p.bad);
    CHECK(sizeof DEFAULTS / sizeof DEFAULTS[0] == (size_t)N_SWITCHES);
    for (const Default& d : DEFAULTS) {
      const Switch* e = entry(d.name);
      CHECK(e != nullptr);
      if (!e) continue;
      if (e->member[0].get(p.s) != d.v0 || e->member[1].get(p.s) != d.v1) {
        printf("default of %s: %d %d\n", d.name, e->member[0].get(p.s), e->member[1].get(p.s));
        ++failures;
      }
    }
    for (const Switch& e : SWITCH_TABLE) {
      bool listed = false;
      for (const Default& d : DEFAULTS) listed = listed || std::string(d.name) == e.name;
      CHECK(listed);
    }
  }
  {   // every accepted word, and no word of the table that the list above does not hold
    size_t in_table = 0;
    for (const Switch& e : SWITCH_TABLE)
      if (e.kind == SWITCH_WORD)
        for (const SwitchWord& w : e.words) in_table += w.word != nullptr;
    CHECK(in_table == sizeof WORDS / sizeof WORDS[0]);
    for (const WordCase& w : WORDS) {
      const Switch* e = entry(w.name);
      CHECK(e && e->kind == SWITCH_WORD);
      if (!e) continue;
      const Parsed p = parse({{w.name, w.word}});
      CHECK(!p.bad);
      if (e->member[0].get(p.s) != w.v0 || e->member[1].get(p.s) != w.v1) {
        printf("%s=%s: %d %d\n", w.name, w.word, e->member[0].get(p.s), e->member[1].get(p.s));
        ++failures;
      }
      // (and nothing else moved)
      const Parsed d = parse({});
      for (const Switch& o : SWITCH_TABLE)
        if (&o != e)
          CHECK(o.member[0].get(p.s) == o.member[0].get(d.s) &&
                o.member[1].get(p.s) == o.member[1].get(d.s));
    }
  }
  {   // an unknown word is refused by every word switch: name, word and accepted words
    size_t n_word = 0;
    for (const Switch& e : SWITCH_TABLE) n_word += e.kind == SWITCH_WORD;
    CHECK(n_word == sizeof WORD_SWITCHES / sizeof WORD_SWITCHES[0]);
    for (const char* name : WORD_SWITCHES) {
      const Switch* e = entry(name);
      CHECK(e && e->kind == SWITCH_WORD);
      for (const char* word : {"tiled", "", "2", "Tile", "plane "}) {
        const Parsed p = parse({{name, word}});
        CHECK(bool(p.bad));
        if (!p.bad) continue;
        const std::string m = p.bad.message();
        CHECK(p.bad.sw == e && p.bad.given == word);
        CHECK(m.find(name) == 0 && m.find(std::string("'") + word + "'") != std::string::npos);
        for (const SwitchWord& w : e->words)
          if (w.word) CHECK(m.find(w.word, strlen(name)) != std::string::npos);
      }
    }
    // the wording of the three refusals the library always had, and of a three-word one
    CHECK(parse({{"AGX_TILE_ORDER", "diagonal"}}).bad.message() ==
          "AGX_TILE_ORDER is 'diagonal': step or column");
    CHECK(parse({{"AGX_D2_STATE", "sweep"}}).bad.message() ==
          "AGX_D2_STATE is 'sweep': update or prepare");
    CHECK(parse({{"AGX_RESID_NORMS", "1"}}).bad.message() ==
          "AGX_RESID_NORMS is '1': prepare or update");
    CHECK(parse({{"AGX_VISC", "tiled"}}).bad.message() ==
          "AGX_VISC is 'tiled': tile, march or gather");
    CHECK(parse({{"AGX_HALO_BATCH", "yes"}}).bad.message() ==
          "AGX_HALO_BATCH is 'yes': 1, 0 or require");
  }
  {   // flags: atoi(value) != 0, whatever their default
    const struct { const char* text; int on; } forms[] = {
        {"", 0}, {"0", 0}, {"1", 1}, {"2", 1}, {"-1", 1}, {"on", 0}, {"1x", 1}};
    int n_flag = 0;
    for (const Switch& e : SWITCH_TABLE) {
      if (e.kind != SWITCH_FLAG) continue;
      ++n_flag;
      for (const auto& f : forms) {
        const Parsed p = parse({{e.name, f.text}});
        CHECK(!p.bad && e.member[0].get(p.s) == f.on);
      }
    }
    CHECK(n_flag == 9);
    CHECK(!parse({{"AGX_NO_FUSE", ""}}).s.no_fuse);      // (an empty AGX_NO_FUSE: fused)
  }
  {   // integers: atoi, clamped
    auto spin = [](const char* w) { return parse({{"AGX_SPIN_LIMIT", w}}).s.spin_limit; };
    CHECK(spin("1") == 1 && spin("0") == 1 && spin("-7") == 1 && spin("") == 1 &&
          spin("250") == 250 && spin("4000000") == 4000000);
    auto wg = [](const char* w) { return parse({{"AGX_WORKGROUPS", w}}).s.workgroups; };
    CHECK(wg("0") == 1 && wg("-3") == 1 && wg("x") == 1 && wg("1") == 1 && wg("64") == 64 &&
          wg("1000") == 1000);
    auto split = [](const char* w) { return parse({{"AGX_MRESID_SPLIT", w}}).s.mresid_split; };
    CHECK(split("0") == 1 && split("-1") == 1 && split("1") == 1 && split("8") == 8 &&
          split("64") == 64 && split("65") == 64 && split("1000") == 64);
  }
  {   // AGX_ABLATE is read by -DAGX_ABLATION builds only
    const Parsed p = parse({{"AGX_ABLATE", "3"}});
    CHECK(!p.bad && p.s.ablate == (SWITCHES_ABLATION_BUILD ? 3 : 0));
    const Switch* e = entry("AGX_ABLATE");
    CHECK(e && e->ablation_only);
    for (const Switch& o : SWITCH_TABLE) CHECK(o.ablation_only == (&o == e));
  }
  {   // several at once; a refusal names the one at fault
    const Parsed p = parse({{"AGX_KERNEL", "gather"}, {"AGX_GRAPHS", "0"}, {"AGX_SPIN_LIMIT", "9"}});
    CHECK(!p.bad && p.s.use_gather && !p.s.use_tile && !p.s.use_graphs && p.s.spin_limit == 9);
    const Parsed q = parse({{"AGX_KERNEL", "gather"}, {"AGX_LUSGS", "planes"}});
    CHECK(q.bad && std::string(q.bad.sw->name) == "AGX_LUSGS");
  }
  if (argc > 1) {   // DESIGN.md's table: the same variables, one row each
    const std::vector<std::string> rows = design_rows(argv[1]);
    const std::set<std::string> doc(rows.begin(), rows.end());
    CHECK(rows.size() == doc.size());                     // (no variable twice)
    CHECK(rows.size() == (size_t)N_SWITCHES);
    for (const std::string& r : rows)
      if (!entry(r)) { printf("DESIGN.md row %s: not in the code's table\n", r.c_str()); ++failures; }
    for (const Switch& e : SWITCH_TABLE)
      if (!doc.count(e.name)) { printf("%s: no row in DESIGN.md\n", e.name); ++failures; }
  } else {
    printf("usage: host_switches DESIGN.md\n");
    ++failures;
  }
  if (failures) { printf("host_switches: %d failure(s)\n", failures); return 1; }
  printf("host_switches OK\n");
  return 0;
}
