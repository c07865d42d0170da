// agx_api.hip -- C-ABI of libaither_gfx950.so (include/aither_gfx950.h).
//
// Host side of the library: owns device-resident SoA mirrors of every block,
// converts the reference's AoS host arrays at upload/download, precomputes the
// halo index maps and launches the kernels of agx_kernels.hpp in the order of
// mgSolution::Iterate (src/mgSolution.cpp:246-269).  There is no CPU compute
// path here: every entry point fails loudly if HIP is unavailable.
#include "agx_kernels.hpp"
#include "agx_geometry.hpp"
#include "agx_start.hpp"
#include "agx_stats.hpp"
#include "agx_series.hpp"
#include "agx_series_ring.hpp"
#include "agx_out_ranges.hpp"
#include "agx_spectra.hpp"
#include "agx_flux.hpp"
#include "agx_mem.hpp"
#include "agx_switches.hpp"
#include <rccl/rccl.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <vector>
#include <array>
#include <map>
#include <string>
#include <algorithm>
#include <memory>
#include <type_traits>

using namespace agx;

static char g_err[512] = "";
static int fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return 1;
}
#define HIPCHK(call)                                                       \
  do {                                                                     \
    hipError_t e_ = (call);                                                \
    if (e_ != hipSuccess)                                                  \
      return fail("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),   \
                  __FILE__, __LINE__);                                     \
  } while (0)

namespace {

// A run-time value as a template argument: f is called with the std::integral_constant of
// the value, which a generic lambda puts into a template argument list -- so the launch of a
// kernel that is templated on run-time choices is written once, with one argument list.
// by_int takes the constants a value may have; one that matches none of them gets the last
// (the `default:` of a switch).  Only what f names is instantiated: where a template argument
// is meant for some values of another only, nest the calls accordingly.  (Inside a nested
// lambda the constant is named through its type, decltype(x)::value: a captured x is no
// constant expression.)
template <class F>
auto by_bool(bool v, F f) {
  return v ? f(std::true_type{}) : f(std::false_type{});
}
template <int V0, int... Vs, class F>
auto by_int(int v, F f) {
  if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V0>{});
  else return v == V0 ? f(std::integral_constant<int, V0>{}) : by_int<Vs...>(v, f);
}

// The sweep graphs of one block, or of all blocks in one launch: a slot per direction,
// triangle set and value of un_is_u.  They hold the BlockDev they were captured with.
struct SweepGraphs {
  hipGraphExec_t g[2][2][2] = {};
  SweepGraphs() = default;
  SweepGraphs(SweepGraphs&& o) noexcept { memcpy(g, o.g, sizeof g); memset(o.g, 0, sizeof g); }
  ~SweepGraphs() { drop(); }
  hipGraphExec_t& at(bool forward, bool full, bool un_is_u) { return g[forward][full][un_is_u]; }
  void drop() {
    for (auto& g1 : g) for (auto& g2 : g1) for (auto& g3 : g2)
      if (g3) { hipGraphExecDestroy(g3); g3 = nullptr; }
  }
};

// Block, Conn and agx_ctx own their device and pinned memory through DevBuf / PinnedBuf
// (agx_mem.hpp); BlockDev and HaloSide are views of it that travel to the kernels
struct Block {
  BlockDev d;
  int global_pos = 0;
  DevBuf<double> slab;
  DevBuf<double> d2;          // D2 arrays of the LU-SGS path (agx_lusgs.hpp)
  DevBuf<double> blockmat;    // block-matrix solvers: a_ | aInv_ | velocityGrad_ planes
  DevBuf<double> sweep_rec;   // plane-by-plane sweeps: geo | dyn | rhs records (k_sweep_records)
  bool sweep_geo_built = false; // the (static) geometry records exist
  // Which derived data of the D2 path are current.  Assigned by the events below agx_ctx
  // ("what happened") and nowhere else; DESIGN.md section 4 has the table of event x flag.
  bool x_planes_current = false; // the planes of x equal the D2 arrays (multigrid calls)
  // agx_phase_implicit_begin left x_ = 0 unwritten (the first half sweep does not read it);
  // until that sweep has run a download of x returns the zeros the reference holds
  bool x_is_zero = false;
  // PA_S and vf() of the physical cells hold the state planes' values (k_update_d2 wrote both
  // last), so the next prepare takes its lean form.  A cleared flag costs a full prepare,
  // never a result.
  bool d2_state_current = false;
  // k_lusgs_prepare folded the norms of the residual planes as they are now into its slot of
  // norm_out, so the update neither reads the residual nor folds.
  bool resid_norms_current = false;
  // the viscous tile kernel of this residual took its RHS form: b, 1 / a and the aInv_ plane
  // are what k_lusgs_prepare would write from the residual planes as they are now, and the
  // block's norms lie in prepare's slot of norm_out.  agx_phase_residual sets it inside
  // agx_iterate, the implicit_begin that follows takes it (and skips the pass).
  bool rhs_in_d2 = false;
  // multigrid: forcing | matrix residual | saved update planes (each allocated on first
  // use); the transfer maps of this block as the FINE side (device copies, keyed by the
  // host pointers they were uploaded from); node values of this block as the coarse side
  DevBuf<double> mg_forcing, mg_mres, mg_xsave, mg_nodes;
  DevBuf<int> mg_tc, mg_start;
  DevBuf<double> mg_vf, mg_cf;
  const void *mg_tc_key = nullptr, *mg_vf_key = nullptr, *mg_cf_key = nullptr;
  // node-built blocks (agx_block_geom.nodes): the node coordinates and the face-centre
  // planes, both on the device until agx_setup_finalize has completed the geometry
  bool node_built = false;
  DevBuf<double> nodes_dev, fcen;
  DevBuf<int> d2_tab;         // device: dstart[Pi + Pj] | ij_of_pos[Pi * Pj]
  std::vector<int> dstart;    // host copy (halo index maps)
  SweepGraphs sweep_graph;    // hyperplane-per-launch sweeps captured as graphs
  DevBuf<int> kp_mem;         // k_lusgs_kp: ticket counter
  unsigned kp_epoch = 0;      // writer launches of the D2 x so far (its low bits tag the values)
  // D2 index of padded cell (i, j, k), host side
  long d2idx(int i, int j, int k) const {
    const int ie = i + d.ng, je = j + d.ng, de = ie + je;
    return (long)(k + d.ng) * d.d2.ps + dstart[de] + je - std::max(0, de - (d.d2.Pi - 1));
  }
  bool state_is_a = true;
  DevBuf<agx_bc_surface> surf_dev;
  std::vector<agx_bc_surface> surf_host;
  // nonreflecting inlet / outlet surfaces: offsets | gradients | Mach (BlockDev)
  DevBuf<int> nr_off_dev;
  DevBuf<double> nr_mem;
  long nr_max = 0;            // cells of the largest such surface (0: none)
  // wall-law surfaces (rans): offsets | wallData_ of their faces (BlockDev)
  DevBuf<int> wall_off_dev;
  DevBuf<WallVars> wall_mem;
  // viscousWall surfaces in the order given (the order of wallData_): what k_wall_pack
  // walks, and the faces of all of them
  std::vector<WallSurfDev> wall_tab;
  DevBuf<WallSurfDev> wall_tab_dev;
  long wall_faces = 0;
  // load surfaces (viscousWall and slipWall) in the order given: what k_wall_loads walks,
  // their faces and chunks, the chunk records of a call, and -- node-built blocks, from
  // agx_setup_finalize on -- the centres of their faces (k_load_centres)
  std::vector<LoadSurfDev> load_tab;
  DevBuf<LoadSurfDev> load_tab_dev;
  long load_faces = 0, load_chunks = 0;
  DevBuf<double> load_partial, load_fcen;
  // flux surfaces (agx_flux.hpp): every surface in the order given but the connections to
  // other ranks -- which the connections decide, so the table is made by the first flux call
  // after the last agx_block_set_bcs / agx_conn_create -- their chunks and the chunk records
  // of a call; the chunk records of the block balance
  std::vector<FluxSurfDev> flux_tab;
  DevBuf<FluxSurfDev> flux_tab_dev;
  bool flux_tab_built = false;
  long flux_chunks = 0;
  DevBuf<double> flux_partial, budget_partial;
  // time statistics (agx_stats.hpp): the cell accumulator planes (null before the first
  // sample: a context that never samples allocates nothing), the wall rows of a viscous block
  // with viscousWall faces, the sum of weights and the number of samples
  DevBuf<double> stat_cells, stat_wall;
  double stat_W = 0.0, stat_n = 0.0;
  // the chunk records of a collapse (AGX_CSTAT_BASE): allocated by the first one, grown by a
  // larger one, freed with the statistics
  DevBuf<double> stat_part;
  // time series (agx_series.hpp): the plan as uploaded (empty: no plan), its ids and points,
  // the ring of rows on the device and the rows' time stamps on the host; wall_epoch counts
  // the agx_block_set_bcs calls (a wall plan is of the wall payload it was uploaded for)
  struct Series {
    std::vector<double> payload;
    int kind = 0, V = 0;
    long P = 0, wall_epoch = 0;
    bool grads = false;
    int32_t var[AGX_OUT_COUNT] = {};
    DevBuf<long> pts;
    DevBuf<double> rows;
    SeriesRing ring;
    std::vector<double> t;
  } series;
  long wall_epoch = 0;
  // spectra (agx_spectra.hpp): the plan as uploaded (empty: no plan), its shape, the twiddle
  // table, the lines of each record, the records of a sample and the accumulators S
  // [spectrum][bin][mode], nondimensional; W and the sample count are the host's
  struct Spectra {
    std::vector<double> payload;
    SpectraDev dev;
    double factor[SPECTRA_MAX_VAR + SPECTRA_MAX_PAIR] = {};
    DevBuf<double> tw, lines, part, S;
    double W = 0.0, samples = 0.0;
  } spectra;
  // the result of the last AGX_FIELD_SERIES_LOCATE upload, 4 doubles per point
  DevBuf<double> locate_out;
  long locate_n = 0;
};

struct ConnSide {          // what side s receives / sends
  std::vector<long> h_dst, h_src;   // host copies (SoA index space) until agx_setup_finalize is done
  long n = 0;              // cells inserted into side s
  // device, per index space (0: SoA planes, 1: the D2 arrays, x of the LU-SGS path;
  // halo_in_d2): ghost cells of side s (this rank's block) and the partner cells that fill them
  struct { DevBuf<long> dst, src; } map[2];
};
struct Conn {
  agx_connection c;
  ConnSide side[2];
  // for remote connections: cells of MY block that the partner's ghosts read
  long n_send = 0;
  DevBuf<long> send_src[2];   // per index space, as ConnSide::map
};

// timing groups of agx_timing_get (include/aither_gfx950.h)
enum { G_RESID = 0, G_UPDATE = 1, G_BC = 2, G_SWEEP = 3, G_VISC = 4, G_PREPARE = 5,
       G_MRESID = 6, G_NGROUP = 7 };

}  // namespace

// (the values of the AGX_* switches are its base: c->use_gather, c->spin_limit, ... as
// agx_ctx_create parsed them, agx_switches.hpp)
struct agx_ctx : agx::Switches {
  int device = 0, rank = 0;
  hipStream_t stream = nullptr;
  bool have_cfg = false, finalized = false;
  agx_config cfg;
  GasDev gas;
  SolverDev sp;
  std::vector<Block> blocks;
  std::vector<Conn> conns;
  // multi-rank: the installed exchange, one persistent slab pair per remote
  // connection, and the norm records of all ranks
  agx_exchange ex = {};
  bool have_ex = false;
  struct Remote { int cid; long count; DevBuf<double> send, recv;
                  PinnedBuf<double> hsend, hrecv; };
  std::vector<Remote> remote;
  std::vector<agx_slab> slabs;
  struct NormRecord { double l2[8]; double mres, linf; int32_t block, i, j, k, eqn, status;
                      double fill[3]; };     // 128 bytes
  DevBuf<NormRecord> rec_dev;           // [1 + nranks] (RCCL)
  PinnedBuf<NormRecord> rec_host;       // [1 + nranks]
  ncclComm_t nccl = nullptr;
  DevBuf<NormPartial> partials;
  long n_partials = 0;
  // norm_out, four regions for nb blocks: the update's norms (the matrix residual of the
  // phase API lands there between prepare and update) | NORM_FOLD partials, scratch of the
  // two-level fold | the matrix residual agx_iterate reads back with the update's norms | the
  // residual norms k_lusgs_prepare folds.  norm_host: what the update's read-back brings | the
  // matrix residual that rides with it.
  static constexpr size_t NORM_FOLD = 64;
  DevBuf<NormPartial> norm_out;
  PinnedBuf<NormPartial> norm_host;
  size_t norm_nb() const { return std::max<size_t>(blocks.size(), 1); }
  NormPartial* norm_update() const { return norm_out.get(); }
  NormPartial* norm_fold() const { return norm_update() + norm_nb(); }
  NormPartial* norm_mres() const { return norm_fold() + NORM_FOLD; }
  NormPartial* norm_prepare() const { return norm_mres() + norm_nb(); }
  NormPartial* norm_end() const { return norm_prepare() + norm_nb(); }
  NormPartial* host_update() const { return norm_host.get(); }
  NormPartial* host_mres() const { return host_update() + norm_nb(); }
  NormPartial* host_end() const { return host_mres() + norm_nb(); }
  DevBuf<int> err_dev;
  PinnedBuf<int> err_host;
  DevBuf<double> halo_buf;
  DevBuf<double> stage_buf;      // AoS staging of uploads / downloads (stage_buffer)
  DevBuf<double> rans_rec;       // face records of the rans viscous residual (k_rans_faces),
                                 // sized for the largest block, shared by all of them
  int num_cu = 256;          // persistent workgroups of the tile kernel (AGX_WORKGROUPS, or one per CU)
  // the DPLUR sweeps that overlap the exchange of x (AGX_OVERLAP) run it on ov_stream
  hipStream_t ov_stream = nullptr;
  hipEvent_t ov_ready = nullptr, ov_done = nullptr;
  bool fused_pending = false;
  hipStream_t cap_stream = nullptr;   // stream the sweep graphs are recorded on
  // several blocks swept hyperplane by hyperplane: the blocks of a half sweep are
  // independent (ghost x comes from the exchange before it), so their chains of
  // launches run side by side on up to 8 branch streams
  std::vector<hipStream_t> branch_streams;
  std::vector<hipEvent_t> branch_events;
  // ... or, hyperplane step by step, all blocks in one launch (k_lusgs_plane_all) from a
  // table of their BlockDev in device memory, one graph per direction / triangle set /
  // un_is_u (AGX_SWEEP_ALL=0: the branch streams)
  DevBuf<BlockDev> blocks_tab;
  PinnedBuf<BlockDev> blocks_tab_host;
  SweepGraphs sweep_graph_all;
  // the pipelined half sweep (k_lusgs_pipe): a workgroup per k-plane of every block
  bool mg_coarse = false;                // a coarse multigrid level (agx_mg_restrict made it one)
  bool mres_plane_form = false;          // agx_mg_matrix_residual: k_matrix_resid on every block
  DevBuf<PipeJob> pipe_jobs[2];          // pipeline order back / forward
  DevBuf<int> pipe_slot0;
  DevBuf<long long> pipe_progress;       // 16 words per plane
  DevBuf<unsigned long long> pipe_ticket;
  size_t pipe_nblocks = 0;
  int pipe_njobs = 0, pipe_maxsteps = 0, pipe_waves = 4;
  long long pipe_launches = 0;
  // local connections exchanged in one gather + one scatter launch (AGX_HALO_BATCH=0: a
  // launch pair per connection).  Legal when no slice reads a cell another connection's
  // insert writes (checked at agx_setup_finalize, which clears halo_batch where no batch
  // forms); tables per halo selector in device memory
  int halo_batch_sides = 0;
  long halo_batch_nmax = 0;
  // levels of the batched exchange (halo_batch_plan): the local connections in table order,
  // and per level its first table entry, its entries and its longest side
  std::vector<int> halo_conn_order;
  struct HaloLevel { int first, sides; long nmax; };
  std::vector<HaloLevel> halo_levels;
  // the state (fused explicit stages) and x (DPLUR) alternate between two sets of planes:
  // one table pair per set, built once each
  DevBuf<HaloSide> halo_tab_dev[5][2][2];   // [what][plane set][gather | scatter]
  bool halo_tab_valid[5][2] = {};
  int halo_set[5] = {};
  PinnedBuf<HaloSide> halo_tab_host;      // staging, 2 * sides entries
  // the tile kernels' plans per shape, charge and order (AGX_TILE_ORDER), made once each
  std::map<std::array<int, 6>, TilePlan> tile_plans;
  bool have_time_n = false;  // agx_store_time_n has run (nonreflecting BCs read consVarsN)
  bool have_wall_data = false;   // a residual's viscous ghost fill has stored the wall-law data
  bool have_residual = false;    // the residual planes hold a residual (agx_phase_residual, or
                                 // an upload of AGX_FIELD_RESIDUAL): AGX_BUDGET_RESIDUAL
  // agx_iterate fills the ghost cells for the NEXT call right after the update,
  // behind the norm read-back the host waits for, so that the GPU does not idle
  // while the host turns the iteration around
  bool in_iterate = false, ghosts_prefilled = false;
  // the transport's swap has failed (halo_exchange_remote): agx_iterate ends the call there
  // wherever the exchange was posted from -- the update's eager ghost fill included
  bool swap_failed = false;
  // the caller's own agx_phase_bc_faces has run and the agx_phase_residual that reads its
  // ghost cells has not: the output paths that refill the ghost cells are refused
  bool ghost_fill_open = false;
  // inside agx_iterate the matrix residual is not read back by a host synchronisation of
  // its own (the update would wait for the host): it rides with the update's norms
  bool mres_deferred = false;
  hipEvent_t norm_event = nullptr;
  bool consn_pending = false;   // AssignSolToTimeN deferred into the first residual launch of the step
  bool state_is_time_n = false; // nothing has changed the state since agx_store_time_n
  long fused_parts = 0;
  // timing: hipEvent pairs recorded on the library's stream around each
  // kernel group, resolved lazily in agx_timing_get (no sync while running)
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  std::vector<std::pair<int, int>> ev_used;   // (group, pool index)
  double t_ms[G_NGROUP] = {};
  long t_n[G_NGROUP] = {};
};

// ---- what the file uses before it defines it (the entry points: aither_gfx950.h) ----
static int my_side(const agx_ctx* c, const Conn& k);
static int implicit_begin(agx_ctx* c, int write_x);
static int halo_exchange_remote(agx_ctx* c, int what);
#if AGX_FAST
static int d2_prepare(agx_ctx* c, Block& blk, int write_x, int again, int norms);
#endif
namespace {
void resolve_timing(agx_ctx* c);
int lusgs_sweep(agx_ctx* c, Block& blk, bool forward, int full, hipStream_t st = nullptr);
}  // namespace

namespace {
// ---- what happened, and which derived data it leaves stale or current ---------------------
// The only statements that assign Block::x_planes_current, x_is_zero, d2_state_current,
// resid_norms_current, rhs_in_d2 and agx_ctx::ghosts_prefilled, state_is_time_n: a writer says
// what it did.  DESIGN.md section 4 has the table of event x flag with the reasons.
//
// x: something is about to write it where it lives (the D2 arrays on the diagonal-ordered
// path) / k_d2_x_copy made a block's planes and its D2 arrays equal
void x_changed(agx_ctx* c) {
  for (auto& blk : c->blocks) blk.x_planes_current = false;
}
void x_planes_copied(Block& b) { b.x_planes_current = true; }
// prepare left a block's x = 0 unwritten (or not) / an upload wrote a block's x / the first
// half sweep writes every block's
void x_prepared(Block& b, bool left_zero) { b.x_is_zero = left_zero; }
void x_uploaded(Block& b) { b.x_is_zero = false; }
void x_swept(agx_ctx* c) {
  for (auto& blk : c->blocks) blk.x_is_zero = false;
}
// the state planes of physical cells: something other than k_update_d2 is about to write
// those of all blocks / of one block / k_update_d2 stored a block's new state, and with
// wrote_d2 (AGX_D2_STATE=update) the D2 state of the next prepare as well
void state_written(agx_ctx* c) {
  for (auto& blk : c->blocks) blk.d2_state_current = false;
}
void state_written(Block& b) { b.d2_state_current = false; }
void state_updated_d2(Block& b, bool wrote_d2) { b.d2_state_current = wrote_d2; }
// the residual planes: something is about to write them / k_lusgs_prepare folded a block's
// norms of them / the update took the folded norms (one use: a second update on the same
// residual reads it itself)
void resid_written(agx_ctx* c) {
  for (auto& blk : c->blocks) blk.resid_norms_current = blk.rhs_in_d2 = false;
}
void resid_norms_folded(Block& b) { b.resid_norms_current = true; }
void resid_norms_used(Block& b) { b.resid_norms_current = false; }
// the viscous tile kernel finished a block's cells for the sweeps (its RHS form) /
// implicit_begin took that in place of the prepare pass
void rhs_written_by_residual(Block& b) { b.rhs_in_d2 = true; }
void rhs_taken(Block& b) { b.rhs_in_d2 = false; }
// an upload or a multigrid restriction wrote planes of a block: whichever they were, its D2
// state and its folded norms are taken for stale
void planes_uploaded(Block& b) {
  b.d2_state_current = false;
  b.resid_norms_current = false;
  b.rhs_in_d2 = false;
}
// the ghost cells: the fill for the next agx_iterate was queued behind the update's norms /
// it is used up, or something wrote ghost cells or the state since
void ghosts_filled_ahead(agx_ctx* c) { c->ghosts_prefilled = true; }
void ghost_fill_gone(agx_ctx* c) { c->ghosts_prefilled = false; }
// the state became time level n (agx_store_time_n; nonreflecting ghost states read
// consVarsN, ghostStates.cpp:435-462: a ghost fill queued behind the last update saw the old
// time level) / an update is about to advance it
void state_became_time_n(agx_ctx* c) {
  for (auto& blk : c->blocks)
    if (blk.nr_max > 0) c->ghosts_prefilled = false;
  c->state_is_time_n = true;
}
void state_left_time_n(agx_ctx* c) { c->state_is_time_n = false; }
// the caller wrote a field of a block (an upload of whichever field, a restriction of the
// state): the ghost cells and consVarsN no longer belong to the state
void field_written_by_caller(agx_ctx* c) {
  ghost_fill_gone(c);
  state_left_time_n(c);
}
// --------------------------------------------------------------------------------------------


struct Timer {   // hipEvents on the library's stream around one kernel group
  agx_ctx* c;
  int slot = -1;
  Timer(agx_ctx* ctx, int g) : c(ctx) {
    if (!c->timing) return;
    if (c->ev_used.size() >= 8192) resolve_timing(c);
    slot = (int)c->ev_used.size();
    if (slot >= (int)c->ev_pool.size()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
        slot = -1;
        return;
      }
      c->ev_pool.emplace_back(a, b);
    }
    c->ev_used.emplace_back(g, slot);
    hipEventRecord(c->ev_pool[slot].first, c->stream);
  }
  ~Timer() {
    if (slot >= 0) hipEventRecord(c->ev_pool[slot].second, c->stream);
  }
};

void resolve_timing(agx_ctx* c) {
  if (c->ev_used.empty()) return;
  hipStreamSynchronize(c->stream);
  for (auto& u : c->ev_used) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev_pool[u.second].first,
                            c->ev_pool[u.second].second) == hipSuccess) {
      c->t_ms[u.first] += ms;
      c->t_n[u.first] += 1;
    }
  }
  c->ev_used.clear();
}

int derive_gas(const agx_config& cfg, GasDev& g) {
  const agx_gas& a = cfg.gas;
  g.R = a.gas_constant;
  g.n = a.n;
  g.inv_n = 1.0 / a.n;
  g.hf = a.heat_of_formation;
  g.cp = a.gas_constant * (a.n + 1.0);   // thermodynamic.hpp:108-113
  g.cv = a.gas_constant * a.n;
  g.gamma = g.cp / g.cv;
  g.prandtl = (4.0 * g.gamma) / (9.0 * g.gamma - 5.0);
  g.inv_prandtl = 1.0 / g.prandtl;
  g.visc_c1 = a.visc_c1; g.visc_s = a.visc_s;
  g.cond_c1 = a.cond_c1; g.cond_s = a.cond_s;
  g.t_ref = a.t_ref;
  g.mu_ref = a.visc_c1 * pow(a.t_ref, 1.5) / (a.t_ref + a.visc_s);  // transport.cpp:58-59
  g.k_nondim = (a.a_ref * a.a_ref * g.mu_ref) / a.t_ref;            // :67
  g.scaling = g.mu_ref / (a.rho_ref * a.a_ref * a.l_ref);            // transport.hpp:43-46
#if AGX_TPG
  // thermallyPerfect (thermodynamic.hpp:125-189): cp, cv, gamma, Pr above are the frozen
  // (n_vib = 0) values and are not read; the kernels take them from T
  g.n_vib = a.n_vib;
  for (int m = 0; m < AGX_MAX_VIB; ++m) g.theta_v[m] = m < a.n_vib ? a.theta_v[m] : 0.0;
#endif
  return 0;
}

dim3 cell_grid(const BlockDev& b, dim3 blk) {
  return dim3((b.ni + blk.x - 1) / blk.x, (b.nj + blk.y - 1) / blk.y, b.nk);
}
const dim3 CELL_BLOCK(64, 4, 1);

Planes5 planes(double* const* p, int n = AGX_NEQ) {
  Planes5 r;
  r.rec = nullptr;
  for (int e = 0; e < AGX_NEQ; ++e) r.p[e] = e < n ? p[e] : nullptr;
  r.stride = 1;
  return r;
}

// upload an AoS host array (dims (ci,cj,ck) incl. gsrc ghosts, ncomp per cell)
// device staging of the AoS <-> SoA conversions: one buffer per context that only grows
// (an output step downloads a dozen fields per block; no allocation per call)
static int stage_buffer(agx_ctx* c, size_t doubles, double** out) {
  if (doubles > c->stage_buf.size()) {
    HIPCHK(hipStreamSynchronize(c->stream));     // (before the old one is freed)
    HIPCHK(c->stage_buf.alloc(doubles));
  }
  *out = c->stage_buf.get();
  return 0;
}
// the tail of a call that hands a payload out: the launches' error, n doubles to the host,
// synchronise
static int copy_out(agx_ctx* c, double* out, const double* dev, size_t n) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, dev, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
int upload_aos(agx_ctx* c, Block& b, const double* host, double* const* dst,
               int ncomp, int ci, int cj, int ck, int gsrc) {
  const long n = (long)ci * cj * ck;
  double* tmp = nullptr;
  planes_uploaded(b);
  if (stage_buffer(c, (size_t)n * ncomp, &tmp)) return 1;
  HIPCHK(hipMemcpyAsync(tmp, host, sizeof(double) * n * ncomp,
                        hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_aos_to_soa, dim3((n + 255) / 256), dim3(256), 0,
                     c->stream, tmp, planes(dst, ncomp), ncomp, ci, cj, ck, gsrc, b.d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
int download_aos(agx_ctx* c, Block& b, double* host, double* const* src,
                 int ncomp, int ci, int cj, int ck, int gsrc) {
  const long n = (long)ci * cj * ck;
  double* tmp = nullptr;
  if (stage_buffer(c, (size_t)n * ncomp, &tmp)) return 1;
  hipLaunchKernelGGL(k_soa_to_aos, dim3((n + 255) / 256), dim3(256), 0,
                     c->stream, tmp, planes(src, ncomp), ncomp, ci, cj, ck, gsrc, b.d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(host, tmp, sizeof(double) * n * ncomp,
                        hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- halo index maps: restates connection::First/SecondSliceIndices
// (boundaryConditions.cpp:1016-1150), AdjustForSlice (:833-860), InsertSlice
// (multiArray3d.hpp:868-918) and GetSwapLoc (boundaryConditions.cpp:3006-3181)
// directly in device-index space.
struct Dims { int n[3]; };
struct MapOut { std::vector<long> dst, src; };

void dirs_of(int boundary, int& d1, int& d2, int& d3) {
  d3 = (boundary - 1) / 2;
  d1 = (d3 + 1) % 3;
  d2 = (d3 + 2) % 3;
}
// receiver = side `recv`; idxR/idxS give device indices for (i,j,k) in the
// receiving / sending block
template <class FR, class FS>
void build_side_map(const agx_connection& cc, int recv, int ng, FR idxR, FS idxS,
                    MapOut& out) {
  const int snd = 1 - recv;
  int orient = cc.orientation;
  if (recv == 1) {                       // connection::SwapOrder :341-364
    if (orient == 4) orient = 5; else if (orient == 5) orient = 4;
  }
  int rd1, rd2, rd3, sd1, sd2, sd3;
  dirs_of(cc.boundary[recv], rd1, rd2, rd3);
  dirs_of(cc.boundary[snd], sd1, sd2, sd3);
  const int r_d1s = cc.d1_start[recv] - ng, r_d1e = cc.d1_end[recv] + ng;
  const int r_d2s = cc.d2_start[recv] - ng, r_d2e = cc.d2_end[recv] + ng;
  const bool r_upper = cc.boundary[recv] % 2 == 0;
  const int blk_start = r_upper ? cc.const_surf[recv] : -ng;
  const bool s_upper = cc.boundary[snd] % 2 == 0;
  const int s_d3s = cc.const_surf[snd] + (s_upper ? -ng : 0);
  const int s_d1s = cc.d1_start[snd] - ng, s_d2s = cc.d2_start[snd] - ng;
  const int s_len1 = cc.d1_end[snd] - cc.d1_start[snd] + 2 * ng;
  const int s_len2 = cc.d2_end[snd] - cc.d2_start[snd] + 2 * ng;
  const int len1 = r_d1e - r_d1s, len2 = r_d2e - r_d2s;
  const int32_t* pb = cc.patch_border + (recv == 0 ? 0 : 4);
  const int aS1 = pb[0] ? ng : 0, aE1 = pb[1] ? ng : 0;
  const int aS2 = pb[2] ? ng : 0, aE2 = pb[3] ? ng : 0;
  const bool llu = (cc.boundary[0] + cc.boundary[1]) % 2 == 0;
  for (int l3 = 0; l3 < ng; ++l3)
    for (int l2 = aS2; l2 < len2 - aE2; ++l2)
      for (int l1 = aS1; l1 < len1 - aE1; ++l1) {
        int a[3], s[3], q1, q2;
        a[rd1] = r_d1s + l1;
        a[rd2] = r_d2s + l2;
        a[rd3] = blk_start + l3;
        if (orient == 2 || orient == 4 || orient == 5 || orient == 7) {
          q2 = (orient == 5 || orient == 7) ? s_len2 - 1 - l1 : l1;
          q1 = (orient == 4 || orient == 7) ? s_len1 - 1 - l2 : l2;
        } else if (sd3 == 0) {           // i-patch rule, cpp:3064-3073
          q1 = (orient == 6 || orient == 8) ? s_len1 - 1 - l1 : l1;
          q2 = (orient == 3 || orient == 8) ? s_len2 - 1 - l2 : l2;
        } else {
          q1 = (orient == 3 || orient == 8) ? s_len1 - 1 - l1 : l1;
          q2 = (orient == 6 || orient == 8) ? s_len2 - 1 - l2 : l2;
        }
        const int q3 = llu ? ng - l3 - 1 : l3;
        s[sd1] = s_d1s + q1;
        s[sd2] = s_d2s + q2;
        s[sd3] = s_d3s + q3;
        out.dst.push_back(idxR(a[0], a[1], a[2]));
        out.src.push_back(idxS(s[0], s[1], s[2]));
      }
}

int ensure_halo_buf(agx_ctx* c, long ndoubles) {
  bool grew;
  HIPCHK(c->halo_buf.reserve((size_t)ndoubles, &grew));
  if (grew)   // (the tables hold slices of this buffer)
    for (auto& v : c->halo_tab_valid) v[0] = v[1] = false;
  return 0;
}

// what a halo exchange moves: the state planes, or x -- which the D2 LU-SGS path
// keeps in its own arrays and index space (1; 0: the planes -- the index of ConnSide::map)
int halo_in_d2(const Block& b, int what) { return what == AGX_HALO_UPDATE && b.d.d2.base ? 1 : 0; }
Planes5 halo_planes(Block& b, int what) {
  Planes5 r;
  // (the scatter of an exchange of x also refreshes the sweep records' copy)
  r.rec = what == AGX_HALO_UPDATE ? b.d.sw_dyn : nullptr;
  const bool z2 = halo_in_d2(b, what) != 0;
  r.stride = z2 ? 2 : 1;     // x of the D2 path sits in pair arrays (x0,x1) (x2,x3) (x4,-)
#if AGX_NEQ == 7
  if (what == AGX_HALO_TURB) {     // eddyViscosity_, f1_, f2_ in the first three slots
    for (int e = 0; e < AGX_NEQ; ++e) r.p[e] = b.d.turb3[e < 3 ? e : 2];
    return r;
  }
#endif
  if (what == AGX_HALO_VELGRAD_A || what == AGX_HALO_VELGRAD_B) {
    // velocityGrad_ (9 planes) in two halves of five slots; the fifth slot of the
    // second half repeats component 8
    for (int e = 0; e < AGX_NEQ; ++e) {
      const int comp = what == AGX_HALO_VELGRAD_A ? e : std::min(5 + e, 8);
      r.p[e] = b.d.vg + (long)comp * b.d.nplane;
    }
    return r;
  }
  for (int e = 0; e < AGX_NEQ; ++e)
    r.p[e] = what == AGX_HALO_STATE ? b.d.state[e]
             : (z2 ? b.d.d2.base + 2L * (PA_X + (e >> 1)) * b.d.d2.nd2 + (e & 1) : b.d.x[e]);
  return r;
}

int check_device_error(agx_ctx* c) {
  int* const err_host = c->err_host.get();
  if (*err_host) {
    const int code = *err_host;
    *err_host = 0;
    hipMemsetAsync(c->err_dev.get(), 0, sizeof(int), c->stream);
    if (code == 3)
      return fail("Singular matrix in Gauss-Jordan elimination!");   // matrix.cpp:81
    if (code == AGX_ERR_TPG_ENERGY)
      return fail("thermallyPerfect: the temperature of a cell's specific energy was not "
                  "found (Newton's method did not converge in %d steps, or the energy lies "
                  "below the heat of formation)", AGX_TPG_NEWTON_MAX);
    if (code == 2) {
      c->pipe_nblocks = 0;   // (the progress words of an abandoned launch: set up afresh)
      return fail("LU-SGS pipeline: a k-plane waited beyond the spin limit for its "
                  "predecessor (AGX_LUSGS=plane / AGX_SWEEP_PIPE=0 select the "
                  "launch-per-hyperplane forms)");
    }
    return fail("a boundary-condition variant outside this build's coverage was requested");
  }
  return 0;
}

struct MarchPlan { dim3 grid; int kchunk; long nparts; TilePlan tile; };
int g_march_tj = 6;   // cell rows per workgroup (512 threads)
// the tile kernel addresses a plane with 32-bit byte offsets (SlabDev::ldb)
bool tile_ok(const agx_ctx* c, const BlockDev& b) {
  return AGX_FAST && c->use_tile && !c->use_gather && (double)b.nplane * 8.0 < 4294967296.0;
}
bool all_tile_ok(const agx_ctx* c) {
  for (const auto& blk : c->blocks)
    if (!tile_ok(c, blk.d)) return false;
  return true;
}
// the plan of gx x gy column tiles on P workgroups, made once per shape and charge
TilePlan tile_plan_of(agx_ctx* c, int gx, int gy, int nk, int P, int charge, int order) {
  const std::array<int, 6> key = {gx, gy, nk, P, charge, order};
  auto it = c->tile_plans.find(key);
  if (it == c->tile_plans.end())
    it = c->tile_plans.emplace(key, tile_plan_make(gx, gy, nk, P, charge, order)).first;
  return it->second;
}
// the cells the configured reconstruction reaches across a face
int recon_reach(const agx_ctx* c) {
  return c->cfg.recon == AGX_RECON_CONSTANT ? 1 : c->cfg.recon == AGX_RECON_MUSCL ? 2 : 3;
}
MarchPlan march_plan(agx_ctx* c, const BlockDev& b) {
  MarchPlan p;
  const int gx = tile_count(b.ni, TILE_INV_I), gy = tile_count(b.nj, g_march_tj);
  p.tile = tile_plan_column(gx * gy, b.nk);
  if (tile_ok(c, b)) {
    // persistent workgroups, one per CU (LDS allows no more); small blocks get
    // fewer so that a range is at least ~8 steps long
    const long steps = (long)gx * gy * b.nk;
    long np = std::min<long>(c->num_cu, std::max<long>(1, steps / 8));
    if (np >= 8) np -= np % 8;
    p.kchunk = 0;
    p.grid = dim3((unsigned)np);
    p.nparts = np;
    p.tile = tile_plan_of(c, gx, gy, b.nk, (int)np, tile_charge_inviscid(recon_reach(c)),
                          c->tile_order_inv);
    return p;
  }
  // aim at >= ~2048 workgroups so that all 256 CUs stay busy to the end
  int nz = std::max(1, (int)std::lround(2048.0 / (gx * gy)));
  nz = std::min(nz, std::max(1, b.nk / 4));
  p.kchunk = (b.nk + nz - 1) / nz;
  nz = (b.nk + p.kchunk - 1) / p.kchunk;
  p.grid = dim3(gx, gy, nz);
  p.nparts = (long)gx * gy * nz;
  return p;
}

// does the block have a connection (interblock / periodic) on any side?
static bool has_connection(const BlockDev& b) {
  bool conn = false;
  for (int q = 0; q < 6; ++q) conn = conn || b.side_conn[q] != 0;
  return conn;
}

SlabDev make_slab(const BlockDev& b) {
  SlabDev sd;
  sd.base = b.vol - (long)PL_VOL * b.nplane;
  sd.nplane = b.nplane; sd.sx = b.sx; sd.sxy = b.sxy;
  sd.ni = b.ni; sd.nj = b.nj; sd.nk = b.nk; sd.ng = b.ng; sd.ioff = b.ioff;
  sd.st = (int)((b.state[0] - sd.base) / b.nplane);
  sd.sn = (int)((b.state2[0] - sd.base) / b.nplane);
  return sd;
}
template <int RECON, int LIM, int FLUX>
void launch_inv_kernel(agx_ctx* c, const BlockDev& b, double cfl, bool fuse,
                       const MarchArgs& ma, const MarchPlan& mp) {
  const SlabDev sd = make_slab(b);
  if (c->use_gather || AGX_NEQ != 5) {   // (the 7-equation build runs the gather form)
    hipLaunchKernelGGL((k_inv_residual<RECON, LIM, FLUX>), cell_grid(b, CELL_BLOCK),
                       CELL_BLOCK, 0, c->stream, b, c->gas, c->sp, cfl);
    return;
  }
  const dim3 tb(64, g_march_tj + 2);
#if AGX_FAST
  if (tile_ok(c, b)) {
    // FUSE: 0 residual only, 1 + explicit stage update, 2 + AssignSolToTimeN (stage 0)
    by_int<2, 1, 0>(!fuse ? 0 : ma.store_consn ? 2 : 1, [&](auto fuse_mode) {
      hipLaunchKernelGGL((k_residual_tile<RECON, LIM, FLUX, fuse_mode, 6>), mp.grid, tb, 0,
                         c->stream, sd, c->gas, c->sp, cfl, ma);
    });
    return;
  }
#endif
  by_bool(fuse, [&](auto fused) {
    hipLaunchKernelGGL((k_residual_march<RECON, LIM, FLUX, fused, 6>), mp.grid, tb, 0,
                       c->stream, sd, c->gas, c->sp, cfl, ma);
  });
}
template <int RECON, int LIM>
void launch_inv_flux(agx_ctx* c, const BlockDev& b, double cfl, bool fuse,
                     const MarchArgs& ma, const MarchPlan& mp) {
  if (c->cfg.inviscid_flux == AGX_FLUX_ROE)
    launch_inv_kernel<RECON, LIM, AGX_FLUX_ROE>(c, b, cfl, fuse, ma, mp);
  else
    launch_inv_kernel<RECON, LIM, AGX_FLUX_AUSM>(c, b, cfl, fuse, ma, mp);
}
template <int RECON>
void launch_inv_lim(agx_ctx* c, const BlockDev& b, double cfl, bool fuse,
                    const MarchArgs& ma, const MarchPlan& mp) {
  switch (c->cfg.limiter) {
    case AGX_LIMITER_VANALBADA: launch_inv_flux<RECON, AGX_LIMITER_VANALBADA>(c, b, cfl, fuse, ma, mp); break;
    case AGX_LIMITER_MINMOD: launch_inv_flux<RECON, AGX_LIMITER_MINMOD>(c, b, cfl, fuse, ma, mp); break;
    default: launch_inv_flux<RECON, AGX_LIMITER_NONE>(c, b, cfl, fuse, ma, mp); break;
  }
}
void launch_inv(agx_ctx* c, const BlockDev& b, double cfl, bool fuse,
                const MarchArgs& ma, const MarchPlan& mp) {
  switch (c->cfg.recon) {
    case AGX_RECON_CONSTANT: launch_inv_flux<AGX_RECON_CONSTANT, AGX_LIMITER_NONE>(c, b, cfl, fuse, ma, mp); break;
    case AGX_RECON_MUSCL: launch_inv_lim<AGX_RECON_MUSCL>(c, b, cfl, fuse, ma, mp); break;
    case AGX_RECON_WENO: launch_inv_flux<AGX_RECON_WENO, AGX_LIMITER_NONE>(c, b, cfl, fuse, ma, mp); break;
    default: launch_inv_flux<AGX_RECON_WENOZ, AGX_LIMITER_NONE>(c, b, cfl, fuse, ma, mp); break;
  }
}

// block-matrix solvers: the inviscid part of the main diagonal (k_block_diag_inv)
// (every reconstruction is built with every limiter here; only MUSCL reads the configured one)
void launch_block_diag(agx_ctx* c, const BlockDev& b) {
  by_int<AGX_RECON_CONSTANT, AGX_RECON_MUSCL, AGX_RECON_WENO, AGX_RECON_WENOZ>(
      c->cfg.recon, [&](auto recon) {
        constexpr int RECON = decltype(recon)::value;
        by_int<AGX_LIMITER_VANALBADA, AGX_LIMITER_MINMOD, AGX_LIMITER_NONE>(
            RECON == AGX_RECON_MUSCL ? c->cfg.limiter : AGX_LIMITER_NONE, [&](auto lim) {
              hipLaunchKernelGGL((k_block_diag_inv<RECON, decltype(lim)::value>),
                                 cell_grid(b, CELL_BLOCK), CELL_BLOCK, 0, c->stream, b, c->gas,
                                 c->sp);
            });
      });
}

bool can_fuse(const agx_ctx* c) {
  // (nonreflecting surfaces read the gradients of the residual's own state after it)
  for (const auto& blk : c->blocks) if (blk.nr_max > 0) return false;
  return !c->no_fuse && !c->use_gather && !c->sp.implicit && !c->sp.viscous;
}

// the D2 LU-SGS path (agx_lusgs.hpp) serves scalar LU-SGS unless AGX_LUSGS=plane
bool is_block_solver(const agx_ctx* c) {   // input::IsBlockMatrix input.cpp:713
  return c->cfg.matrix_solver == AGX_SOLVER_BLUSGS || c->cfg.matrix_solver == AGX_SOLVER_BDPLUR;
}
bool is_lusgs_solver(const agx_ctx* c) {   // input.cpp:847
  return c->cfg.matrix_solver == AGX_SOLVER_LUSGS || c->cfg.matrix_solver == AGX_SOLVER_BLUSGS;
}
bool use_d2(const agx_ctx* c) {
  // (the Roe off-diagonal needs the state on both sides of a face: served by the
  // hyperplane-per-launch form on the SoA planes)
  return AGX_FAST && c->sp.implicit && c->cfg.matrix_solver == AGX_SOLVER_LUSGS && c->lusgs_mode == 1 &&
         c->cfg.inv_flux_jacobian == AGX_JACOBIAN_RUSANOV;
}
#if AGX_FAST
// what the D2 kernels take of a block (k_lusgs_kp, k_matrix_resid_d2m)
KpBlk kp_blk_of(const BlockDev& b) {
  KpBlk kb;
  kb.base = b.d2.base; kb.dstart = b.d2.dstart; kb.surf = b.surf;
  kb.nd2 = b.d2.nd2; kb.ps = b.d2.ps; kb.Pi = b.d2.Pi; kb.Pj = b.d2.Pj;
  kb.ni = b.ni; kb.nj = b.nj; kb.nk = b.nk; kb.ng = b.ng;
  kb.nsurf = b.nsurf; kb.nsurf_i = b.nsurf_i; kb.nsurf_j = b.nsurf_j; kb.nsurf_k = b.nsurf_k;
  for (int q = 0; q < 6; ++q) kb.side_conn[q] = b.side_conn[q];
  return kb;
}
// One LU-SGS half sweep over a block, one launch: a workgroup per k-plane marches
// the plane's diagonals, the planes follow each other one step apart (k_lusgs_kp).
template <bool FWD, bool FULL, bool CONN, int CH>
int lusgs_kp_launch(agx_ctx* c, Block& blk) {
  const BlockDev& b = blk.d;
  if (!blk.kp_mem) {                      // the ticket counter
    HIPCHK(blk.kp_mem.alloc(32));
    HIPCHK(hipMemsetAsync(blk.kp_mem.get(), 0, sizeof(int) * 32, c->stream));
  }
  KpArgs kp;
  kp.ticket = blk.kp_mem.get();
  kp.err = c->err_dev.get();
  // the launch's tag of the values it stores (agx_lusgs_kernels.hpp: KpArgs); every
  // writer of x advances the block's epoch
  kp.tag = (unsigned)(++blk.kp_epoch) & 3u;
  kp.spin_limit = c->spin_limit;
  kp.trace = nullptr;
#ifdef AGX_KP_TRACE
  static long long* trace_dev = nullptr;
  const size_t trace_n = 6 * (size_t)(b.ni + b.nj + 2);
  if (getenv("AGX_KP_TRACE")) {
    if (!trace_dev) hipMalloc((void**)&trace_dev, sizeof(long long) * 6 * 8192);
    hipMemsetAsync(trace_dev, 0, sizeof(long long) * trace_n, c->stream);
    kp.trace = trace_dev;
  }
#endif
  HIPCHK(hipMemsetAsync(kp.ticket, 0, sizeof(int), c->stream));
  // LDS: two buffers of 14-double records for the cells of a diagonal (+ 2 slots)
  int nsl = std::min(b.ni, b.nj) + 2;
  nsl += nsl & 1;
  const size_t lds = sizeof(double) * 2 * KP_NV * (size_t)nsl;
  const void* fn = reinterpret_cast<const void*>(&k_lusgs_kp<FWD, FULL, CONN, CH>);
  if (lds > 48 * 1024)
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // persistent: never more workgroups than are resident at once (a plane waits
  // for its predecessor, which must therefore be running or finished)
  int per_cu = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds) != hipSuccess ||
      per_cu < 1)
    per_cu = 1;
  const int wgs = std::min(per_cu * c->num_cu, b.nk);
  const KpBlk kb = kp_blk_of(b);
  const KpGas kg{c->gas.hf, c->gas.n, c->gas.inv_n};
  hipLaunchKernelGGL((k_lusgs_kp<FWD, FULL, CONN, CH>), dim3(wgs), dim3(256), lds, c->stream,
                     kb, kg, c->sp.viscous, nsl, kp);
#ifdef AGX_KP_TRACE
  if (kp.trace) {   // diagnostic build only: dump the step timestamps of this launch
    std::vector<long long> h(trace_n);
    hipStreamSynchronize(c->stream);
    hipMemcpy(h.data(), kp.trace, sizeof(long long) * trace_n, hipMemcpyDeviceToHost);
    FILE* f = fopen(getenv("AGX_KP_TRACE"), "a");
    if (f) {
      fprintf(f, "# %s ni %d nj %d nk %d wgs %d\n", FWD ? "fwd" : "bwd", b.ni, b.nj, b.nk, wgs);
      for (size_t t = 0; t + 6 <= trace_n; t += 6)
        fprintf(f, "%lld %lld %lld %lld %lld %lld\n", h[t], h[t + 1], h[t + 2], h[t + 3],
                h[t + 4], h[t + 5]);
      fclose(f);
    }
  }
#endif
  return 0;
}
// diagonals longer than 256 cells are walked in CH chunks per step
constexpr int KP_MAX_DIAG = 512;   // LDS: 2 * 19 * 8 * (n + 2) bytes <= 160 KiB

#else
constexpr int KP_MAX_DIAG = 1 << 30;
#endif

static void launch_plane_sweep(agx_ctx* c, const BlockDev& b, bool forward, int full,
                               hipStream_t st) {
  // with the cell-major records: three lanes per cell (k_lusgs_plane3), 21 cells per wave row
  const bool three = b.sw_geo != nullptr && c->sweep_three;
  const dim3 tb(64, 4), grid(three ? (b.nj + PL3_CELLS - 1) / PL3_CELLS : (b.nj + 63) / 64,
                             (b.nk + 3) / 4);
  const int nplanes = b.ni + b.nj + b.nk - 2;
  for (int t = 0; t < nplanes; ++t) {
    const int p = forward ? t : nplanes - 1 - t;
    if (three)
      by_bool(forward, [&](auto fwd) {
        hipLaunchKernelGGL((k_lusgs_plane3<fwd>), grid, tb, 0, st, b, c->gas, c->sp, p, full);
      });
    else
      by_bool(forward, [&](auto fwd) {
        hipLaunchKernelGGL((k_lusgs_plane<fwd>), grid, tb, 0, st, b, c->gas, c->sp, p, full);
      });
  }
}

// every block of this rank side by side (see branch_streams); false: not applicable
// (one block, a diagonal-ordered block, graphs switched off)
static bool plane_sweep_all_applicable(const agx_ctx* c) {
  if (!c->use_graphs || c->blocks.size() < 2) return false;
  for (auto& blk : c->blocks)
    if (blk.d.d2.base || blk.d.ni + blk.d.nj + blk.d.nk - 2 < 8) return false;
  return true;
}
// The launches of a half sweep are the same every iteration: captured once into the slot's
// hipGraph, replayed on st.  (Recorded on a stream of its own: the library's stream may be
// the legacy default stream, which cannot capture; a graph is launched on any stream.)
template <class F>
static int replay_captured(agx_ctx* c, hipGraphExec_t& ge, F launch_all, hipStream_t st) {
  if (!ge) {
    if (!c->cap_stream) HIPCHK(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal));
    launch_all(c->cap_stream);
    HIPCHK(hipStreamEndCapture(c->cap_stream, &graph));
    HIPCHK(hipGraphInstantiate(&ge, graph, nullptr, nullptr, 0));
    HIPCHK(hipGraphDestroy(graph));
  }
  HIPCHK(hipGraphLaunch(ge, st));
  return 0;
}
// the device copy of the blocks' descriptors, for kernels that serve all blocks in one launch
static int sync_blocks_tab(agx_ctx* c) {
  const size_t nb = c->blocks.size();
  if (c->blocks_tab && c->blocks_tab.size() != nb) {   // (blocks were added since)
    HIPCHK(hipStreamSynchronize(c->stream));
    c->sweep_graph_all.drop();                       // (their grids cover nb blocks)
  }
  if (c->blocks_tab.size() != nb) {
    HIPCHK(c->blocks_tab.alloc(nb));
    HIPCHK(c->blocks_tab_host.alloc(nb));
    memset(c->blocks_tab_host.get(), 0, sizeof(BlockDev) * nb);
  }
  BlockDev* const host = c->blocks_tab_host.get();
  // the table follows the blocks (pointers that change roles, new surfaces): if it
  // differs from what the device holds, upload it
  bool same = true;
  for (size_t n = 0; n < nb; ++n)
    same = same && memcmp(&host[n], &c->blocks[n].d, sizeof(BlockDev)) == 0;
  if (!same) {
    HIPCHK(hipStreamSynchronize(c->stream));      // (nobody reads the pinned copy any more)
    for (size_t n = 0; n < nb; ++n) memcpy(&host[n], &c->blocks[n].d, sizeof(BlockDev));
    HIPCHK(hipMemcpyAsync(c->blocks_tab.get(), host, sizeof(BlockDev) * nb,
                          hipMemcpyHostToDevice, c->stream));
  }
  return 0;
}
// Pipelined half sweep of all blocks (k_lusgs_pipe): applicable to blocks on the cell-major
// records (the 7-equation and block-matrix builds; the 5-equation scalar solver has its own
// diagonal-ordered pipeline, k_lusgs_kp)
static bool pipe_sweep_applicable(const agx_ctx* c) {
  if (!c->sweep_pipe || c->blocks.empty()) return false;
  for (auto& blk : c->blocks)
    if (blk.d.d2.base || !blk.d.sw_geo) return false;
  return true;
}
static int pipe_setup(agx_ctx* c) {
  const size_t nb = c->blocks.size();
  HIPCHK(hipStreamSynchronize(c->stream));
  c->pipe_nblocks = 0; c->pipe_njobs = 0; c->pipe_launches = 0;
  // pipeline order: plane k of every block before plane k + 1 of any (going back: from the top)
  std::vector<PipeJob> fwd, bwd;
  std::vector<int> slot0(nb);
  int nk_max = 0, slots = 0, diag = 1;
  c->pipe_maxsteps = 0;
  for (size_t n = 0; n < nb; ++n) {
    const BlockDev& b = c->blocks[n].d;
    slot0[n] = slots;
    slots += b.nk;
    nk_max = std::max(nk_max, b.nk);
    c->pipe_maxsteps = std::max(c->pipe_maxsteps, b.ni + b.nj - 1);
    diag = std::max(diag, std::min(b.ni, b.nj));
  }
  for (int k = 0; k < nk_max; ++k)
    for (size_t n = 0; n < nb; ++n) {
      const int nk = c->blocks[n].d.nk;
      if (k < nk) { fwd.push_back({(int)n, k}); bwd.push_back({(int)n, nk - 1 - k}); }
    }
  c->pipe_njobs = (int)fwd.size();
  c->pipe_waves = std::max(1, std::min(8, (diag + PL3_CELLS - 1) / PL3_CELLS));
  for (int dir = 0; dir < 2; ++dir) HIPCHK(c->pipe_jobs[dir].upload(dir ? fwd : bwd));
  HIPCHK(c->pipe_slot0.upload(slot0));
  HIPCHK(c->pipe_progress.alloc((size_t)16 * slots));
  HIPCHK(hipMemset(c->pipe_progress.get(), 0, sizeof(long long) * 16 * slots));
  HIPCHK(c->pipe_ticket.alloc(16));           // (a 128-byte line of its own)
  HIPCHK(hipMemset(c->pipe_ticket.get(), 0, 128));
  c->pipe_nblocks = nb;
  return 0;
}
static int lusgs_sweep_pipe(agx_ctx* c, bool forward, int full) {
  const size_t nb = c->blocks.size();
  bool same = c->pipe_nblocks == nb;
  if (same) {
    int slots = 0, steps = 0;
    for (auto& blk : c->blocks) { slots += blk.d.nk; steps = std::max(steps, blk.d.ni + blk.d.nj - 1); }
    same = slots == c->pipe_njobs && steps == c->pipe_maxsteps;
  }
  if (!same && pipe_setup(c)) return 1;
  if (sync_blocks_tab(c)) return 1;
  PipeArgs pa;
  pa.jobs = c->pipe_jobs[forward ? 1 : 0].get();
  pa.slot0 = c->pipe_slot0.get();
  pa.progress = c->pipe_progress.get();
  pa.ticket = c->pipe_ticket.get();
  pa.base = c->pipe_launches * (long long)(c->pipe_maxsteps + 1);
  pa.tbase = (unsigned long long)c->pipe_launches * (unsigned long long)c->pipe_njobs;
  pa.njobs = c->pipe_njobs;
  pa.spin_limit = c->spin_limit;
  pa.err = c->err_dev.get();
  pa.trace = nullptr;
#ifdef AGX_PIPE_TRACE
  static long long* trace_dev = nullptr;
  const size_t trace_n = 5 * (size_t)(c->pipe_maxsteps + 1);
  if (getenv("AGX_PIPE_TRACE")) {
    if (!trace_dev) hipMalloc((void**)&trace_dev, sizeof(long long) * 5 * 65536);
    hipMemsetAsync(trace_dev, 0, sizeof(long long) * trace_n, c->stream);
    pa.trace = trace_dev;
  }
#endif
  ++c->pipe_launches;
  const dim3 grid((unsigned)c->pipe_njobs);
  const dim3 tb(64, c->pipe_waves);
  by_bool(forward, [&](auto fwd) {
    hipLaunchKernelGGL((k_lusgs_pipe<fwd>), grid, tb, 0, c->stream, c->blocks_tab.get(), c->gas,
                       c->sp, full, pa);
  });
  HIPCHK(hipGetLastError());
#ifdef AGX_PIPE_TRACE
  if (pa.trace) {   // diagnostic build only: dump the step timestamps of this launch
    std::vector<long long> h(trace_n);
    hipStreamSynchronize(c->stream);
    hipMemcpy(h.data(), pa.trace, sizeof(long long) * trace_n, hipMemcpyDeviceToHost);
    if (FILE* f = fopen(getenv("AGX_PIPE_TRACE"), "a")) {
      fprintf(f, "# %s jobs %d\n", forward ? "fwd" : "bwd", c->pipe_njobs);
      for (size_t t = 0; t + 5 <= trace_n; t += 5)
        fprintf(f, "%lld %lld %lld %lld %lld\n", h[t], h[t + 1], h[t + 2], h[t + 3], h[t + 4]);
      fclose(f);
    }
  }
#endif
  return 0;
}
static int lusgs_sweep_all_one_launch(agx_ctx* c, bool forward, int full) {
  const size_t nb = c->blocks.size();
  if (sync_blocks_tab(c)) return 1;
  int steps = 0;
  unsigned gx = 1, gy = 1;
  bool three = c->sweep_three;
  for (auto& blk : c->blocks) three = three && blk.d.sw_geo != nullptr;
  for (auto& blk : c->blocks) {
    steps = std::max(steps, blk.d.ni + blk.d.nj + blk.d.nk - 2);
    gx = std::max(gx, three ? (unsigned)(blk.d.nj + PL3_CELLS - 1) / PL3_CELLS
                            : (unsigned)(blk.d.nj + 63) / 64);
    gy = std::max(gy, (unsigned)(blk.d.nk + 3) / 4);
  }
  const dim3 tb(64, 4), grid(gx, gy, (unsigned)nb);
  const BlockDev* const tab = c->blocks_tab.get();
  auto launch_all = [&](hipStream_t st) {
    for (int t = 0; t < steps; ++t) {
      if (three)
        by_bool(forward, [&](auto fwd) {
          hipLaunchKernelGGL((k_lusgs_plane_all3<fwd>), grid, tb, 0, st, tab, c->gas, c->sp, t,
                             full);
        });
      else
        by_bool(forward, [&](auto fwd) {
          hipLaunchKernelGGL((k_lusgs_plane_all<fwd>), grid, tb, 0, st, tab, c->gas, c->sp, t,
                             full);
        });
    }
  };
  return replay_captured(c, c->sweep_graph_all.at(forward, full != 0, c->sp.un_is_u != 0),
                         launch_all, c->stream);
}
static int lusgs_sweep_all(agx_ctx* c, bool forward, int full) {
  if (c->sweep_all_launch) return lusgs_sweep_all_one_launch(c, forward, full);
  const size_t ns = std::min<size_t>(c->blocks.size(), 8);
  while (c->branch_streams.size() < ns) {
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    c->branch_streams.push_back(st);
  }
  while (c->branch_events.size() < ns + 1) {
    hipEvent_t ev;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    c->branch_events.push_back(ev);
  }
  // fork from the library's stream, one chain of hyperplane launches (the block's own
  // graph) per branch stream, join
  HIPCHK(hipEventRecord(c->branch_events[ns], c->stream));
  for (size_t q = 0; q < ns; ++q)
    HIPCHK(hipStreamWaitEvent(c->branch_streams[q], c->branch_events[ns], 0));
  for (size_t n = 0; n < c->blocks.size(); ++n)
    if (lusgs_sweep(c, c->blocks[n], forward, full, c->branch_streams[n % ns])) return 1;
  for (size_t q = 0; q < ns; ++q) {
    HIPCHK(hipEventRecord(c->branch_events[q], c->branch_streams[q]));
    HIPCHK(hipStreamWaitEvent(c->stream, c->branch_events[q], 0));
  }
  return 0;
}

#if AGX_FAST
// the form of k_lusgs_kp for a half sweep of this block: direction, triangle set, connections
// on any side, chunks per step (2 x 2 x 2 x 2 forms)
int lusgs_kp_variant(agx_ctx* c, Block& blk, bool forward, int full) {
  const bool conn = has_connection(blk.d);
  const int chunks = std::min(blk.d.ni, blk.d.nj) <= 256 ? 1 : 2;
  return by_bool(forward, [&](auto fwd) {
    return by_bool(full != 0, [&](auto fl) {
      return by_bool(conn, [&](auto cn) {
        return by_int<1, 2>(chunks, [&](auto ch) {
          return lusgs_kp_launch<decltype(fwd)::value, decltype(fl)::value,
                                 decltype(cn)::value, decltype(ch)::value>(c, blk);
        });
      });
    });
  });
}
#endif

int lusgs_sweep(agx_ctx* c, Block& blk, bool forward, int full, hipStream_t st) {
  const BlockDev& b = blk.d;
  if (!st) st = c->stream;
  if (!b.d2.base) {
    // One launch per hyperplane i + j + k = p: ni + nj + nk - 2 short launches per half
    // sweep, bound by launch latency: replayed as a graph (per direction / triangle set /
    // value of un_is_u, the one solver parameter that changes between iterations).
    const int nplanes = b.ni + b.nj + b.nk - 2;
    auto launch_all = [&](hipStream_t st) { launch_plane_sweep(c, b, forward, full, st); };
    if (!c->use_graphs || nplanes < 8) {
      launch_all(st);
      return 0;
    }
    return replay_captured(c, blk.sweep_graph.at(forward, full != 0, c->sp.un_is_u != 0),
                           launch_all, st);
  }
#if AGX_FAST
  return lusgs_kp_variant(c, blk, forward, full);
#else
  return fail("no diagonal-ordered sweep in this build");
#endif
}

// consVarsN = cons(state) that agx_store_time_n deferred (see there)
int flush_consn(agx_ctx* c) {
  if (!c->consn_pending) return 0;
  c->consn_pending = false;
  for (auto& blk : c->blocks)
    hipLaunchKernelGGL(k_store_time_n, cell_grid(blk.d, CELL_BLOCK), CELL_BLOCK,
                       0, c->stream, blk.d, c->gas, 0);
  HIPCHK(hipGetLastError());
  return 0;
}


int bc_pass(agx_ctx* c, bool faces, int viscous) {
  for (auto& blk : c->blocks) {
    const BlockDev& b = blk.d;
    if (faces) {
      long nmax = 0;
      for (int sn = 0; sn < b.nsurf; ++sn) {
        const agx_bc_surface& s = blk.surf_host[sn];
        if (s.bc_type == AGX_BC_INTERBLOCK || s.bc_type == AGX_BC_PERIODIC) continue;
        if (viscous && s.bc_type != AGX_BC_VISCOUSWALL) continue;
        const int st = surface_type(s);
        const int d3 = (st - 1) / 2, d1 = (d3 + 1) % 3, d2 = (d3 + 2) % 3;
        const int lo[3] = {s.imin, s.jmin, s.kmin}, hi[3] = {s.imax, s.jmax, s.kmax};
        nmax = std::max(nmax, (long)(hi[d1] - lo[d1]) * (hi[d2] - lo[d2]));
      }
      if (!viscous && blk.nr_max > 0) {
        if (!c->have_time_n)
          return fail("nonreflecting boundary: the state at time n has not been stored");
        if (flush_consn(c)) return 1;   // (its ghost states read consVarsN)
        hipLaunchKernelGGL(k_nr_mach, dim3(b.nsurf), dim3(256), 0, c->stream, b, c->gas);
      }
      if (nmax > 0)
        hipLaunchKernelGGL(k_bc_faces, dim3((nmax + 255) / 256, b.nsurf), dim3(256), 0,
                           c->stream, b, c->gas, viscous, c->err_dev.get());
    } else {
      const long n = 4L * (b.ni + b.nj + b.nk);
      hipLaunchKernelGGL(k_bc_edges, dim3((n + 127) / 128), dim3(128), 0,
                         c->stream, b, c->gas, viscous, c->err_dev.get());
    }
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int reduce_norms(agx_ctx* c, size_t blk_index, long nparts, NormPartial* out = nullptr) {
  if (!out) out = c->norm_update() + blk_index;
  if (nparts > 4096) {
    // two levels: NORM_FOLD workgroups fold slices into the scratch region of norm_out
    NormPartial* tmp = c->norm_fold();
    hipLaunchKernelGGL(k_norm_final, dim3((unsigned)agx_ctx::NORM_FOLD), dim3(256), 0, c->stream,
                       c->partials.get(), nparts, tmp);
    hipLaunchKernelGGL(k_norm_final, dim3(1), dim3(256), 0, c->stream, tmp,
                       (long)agx_ctx::NORM_FOLD, out);
  } else {
    hipLaunchKernelGGL(k_norm_final, dim3(1), dim3(256), 0, c->stream,
                       c->partials.get(), nparts, out);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// the inviscid ghost fill as the library's own callers make it: agx_phase_bc_faces is the
// caller's, and opens the interval in which ghosts_for_output refuses (ghost_fill_open)
int bc_faces(agx_ctx* c) { Timer t(c, G_BC); return bc_pass(c, true, 0); }
int bc_edges(agx_ctx* c) { Timer t(c, G_BC); return bc_pass(c, false, 0); }

// gridLevel::GetBoundaryConditions gridLevel.cpp:287-319 for the blocks of this rank
int fill_ghosts(agx_ctx* c) {
  if (bc_faces(c)) return 1;
  if (agx_halo_exchange(c, AGX_HALO_STATE)) return 1;
  return bc_edges(c);
}
int update_pass(agx_ctx* c, int mode, int mm, double* l2, agx_linf* linf) {
  state_left_time_n(c);
  const double alpha[4] = {0.25, 1.0 / 3.0, 0.5, 1.0};   // procBlock.cpp:938
  const size_t nb = c->blocks.size();
  // blocks whose norms sit in prepare's region of norm_out
  std::vector<size_t> from_prepare;
  if (mode != 2 && c->fused_pending) {
    // the marching kernel already advanced the state into the second buffer
    // and left one norm partial per workgroup: fold them and swap buffers
    Timer t(c, G_UPDATE);
    state_written(c);
    long off = 0;
    for (size_t n = 0; n < c->blocks.size(); ++n) {
      BlockDev& b = c->blocks[n].d;
      const MarchPlan mp = march_plan(c, b);
      hipLaunchKernelGGL(k_norm_final, dim3(1), dim3(256), 0, c->stream,
                         c->partials.get() + off, mp.nparts, c->norm_update() + n);
      off += mp.nparts;
      for (int e = 0; e < AGX_NEQ; ++e) std::swap(b.state[e], b.state2[e]);
    }
    c->halo_set[AGX_HALO_STATE] ^= 1;              // (the tables hold plane pointers)
    c->fused_pending = false;
    HIPCHK(hipGetLastError());
  } else {
    Timer t(c, G_UPDATE);
    for (size_t n = 0; n < c->blocks.size(); ++n) {
      Block& blk = c->blocks[n];
      const BlockDev& b = blk.d;
      const int last = mm == c->cfg.nonlinear_iterations - 1;
#if AGX_FAST
      if (mode == 2 && b.d2.base) {
        const dim3 tg((b.ni + TT - 1) / TT, (b.nj + TT - 1) / TT, b.nk);
        // the D2 state of the next prepare from here (AGX_D2_STATE); the norms from
        // k_lusgs_prepare where it folded those of this residual (AGX_RESID_NORMS)
        const bool ws = c->d2_state_update, pn = blk.resid_norms_current;
        by_bool(ws, [&](auto write_s) {
          by_bool(pn, [&](auto from_prep) {     // (NORMS: the update folds them itself)
            hipLaunchKernelGGL((k_update_d2<decltype(write_s)::value, !from_prep>), tg, dim3(256),
                               0, c->stream, b, c->gas, c->sp, last, c->partials.get());
          });
        });
        state_updated_d2(blk, ws);
        if (pn) {
          resid_norms_used(blk);
          from_prepare.push_back(n);
        } else if (reduce_norms(c, n, (long)tg.x * tg.y * tg.z)) {
          return 1;
        }
        continue;
      }
#endif
      state_written(blk);
      const dim3 grid = cell_grid(b, CELL_BLOCK);
      hipLaunchKernelGGL(k_update, grid, CELL_BLOCK, 0, c->stream, b, c->gas,
                         c->sp, mode, mode == 1 ? alpha[mm & 3] : 1.0, last,
                         c->partials.get());
      if (reduce_norms(c, n, (long)grid.x * grid.y * grid.z)) return 1;
    }
  }
  // the same layout either way: every block's norms from prepare's slots, or from the
  // update's (a mix -- an upload into one block between the two -- is gathered there first)
  const NormPartial* norm_src = c->norm_update();
  if (from_prepare.size() == nb && nb > 0) norm_src = c->norm_prepare();
  else
    for (size_t n : from_prepare)
      HIPCHK(hipMemcpyAsync(c->norm_update() + n, c->norm_prepare() + n, sizeof(NormPartial),
                            hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->host_update(), norm_src, sizeof(NormPartial) * nb,
                        hipMemcpyDeviceToHost, c->stream));
  if (c->mres_deferred)
    HIPCHK(hipMemcpyAsync(c->host_mres(), c->norm_mres(), sizeof(NormPartial) * nb,
                          hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(c->err_host.get(), c->err_dev.get(), sizeof(int),
                        hipMemcpyDeviceToHost, c->stream));
  if (c->in_iterate && c->eager_ghosts) {
    // the host waits for the norms only; the ghost fill of the next iteration is
    // already queued behind them
    if (!c->norm_event) HIPCHK(hipEventCreateWithFlags(&c->norm_event, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->norm_event, c->stream));
    if (fill_ghosts(c)) return 1;
    ghosts_filled_ahead(c);
    HIPCHK(hipEventSynchronize(c->norm_event));
  } else {
    HIPCHK(hipStreamSynchronize(c->stream));   // the one sync per iteration
  }
  if (check_device_error(c)) return 1;
  for (size_t n = 0; n < c->blocks.size(); ++n) {
    const NormPartial& p = c->host_update()[n];
    const BlockDev& b = c->blocks[n].d;
    for (int e = 0; e < AGX_NEQ; ++e) l2[e] += p.l2[e];
    if (p.vmax > linf->linf) {           // procBlock.cpp:863-866
      long cell = p.lin / AGX_NEQ;
      linf->linf = p.vmax;
      linf->eqn = (int)(p.lin % AGX_NEQ) + 1;
      linf->i = (int)(cell % b.ni);
      linf->j = (int)((cell / b.ni) % b.nj);
      linf->k = (int)(cell / ((long)b.ni * b.nj));
      linf->block = b.parent;
    }
  }
  return 0;
}

}  // namespace

// ===========================================================================

// ---- node-built blocks (agx_block_geom.nodes): the whole geometry on the device ----------
// Kernels: agx_geometry.hpp.  The order is that of the host set-up (main.cpp:100-203 as
// aither_amd/case/builder.py restates it).
namespace {
GeoPlanes geo_planes(Block& b) {
  GeoPlanes g;
  const BlockDev& d = b.d;
  g.vol = d.vol; g.wdist = d.wdist;
  for (int q = 0; q < 3; ++q) {
    g.cen[q] = d.cen[q];
    for (int cc = 0; cc < 4; ++cc) g.fa[q][cc] = d.fa[q][cc];
    for (int cc = 0; cc < 3; ++cc)
      g.fc[q][cc] = b.fcen ? b.fcen.get() + (long)(3 * q + cc) * d.nplane : nullptr;
  }
  return g;
}
inline dim3 geo_grid(long n) { return dim3((unsigned)((std::max<long>(n, 1) + 255) / 256)); }

// cell range of a surface as boundarySurface::RangeI/J/K give it (lo == hi: one plane)
void surface_range(const agx_bc_surface& s, int* lo, int* hi) {
  lo[0] = s.imin; lo[1] = s.jmin; lo[2] = s.kmin;
  hi[0] = s.imax; hi[1] = s.jmax; hi[2] = s.kmax;
  for (int q = 0; q < 3; ++q) if (lo[q] == hi[q]) hi[q] = lo[q] + 1;
}

// agx_block_create: the nodes go to the device and stay there until agx_setup_finalize;
// volume, centre and face areas of the physical cells straight into the block's planes
int geo_block_metrics(agx_ctx* c, Block& b, const double* nodes) {
  const BlockDev& d = b.d;
  const long nn = (long)(d.ni + 1) * (d.nj + 1) * (d.nk + 1);
  HIPCHK(b.nodes_dev.alloc((size_t)3 * nn));
  HIPCHK(hipMemcpyAsync(b.nodes_dev.get(), nodes, sizeof(double) * 3 * nn, hipMemcpyHostToDevice,
                        c->stream));
  HIPCHK(hipMemsetAsync(c->err_dev.get(), 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(k_metrics_planes, geo_grid(nn), dim3(256), 0, c->stream, d,
                     b.nodes_dev.get(), geo_planes(b), 1, c->err_dev.get());
  hipLaunchKernelGGL(k_geo_fill, geo_grid(d.nplane), dim3(256), 0, c->stream, d.wdist,
                     (long)d.nplane, 1.0e10);                  // DEFAULT_WALL_DIST
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c->err_host.get(), c->err_dev.get(), sizeof(int), hipMemcpyDeviceToHost,
                        c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  const int code = *c->err_host.get();
  if (code) {
    *c->err_host.get() = 0;
    hipMemsetAsync(c->err_dev.get(), 0, sizeof(int), c->stream);
    if (code == 4) return fail("negative volume in PLOT3D block");
    return fail("negative %c-face area in PLOT3D block", "ijk"[(code - 5) % 3]);
  }
  return 0;
}

// SwapGeomSlice of one interblock connection (utility.cpp:212-255; PutGeomSlice
// procBlock.cpp:3165-3600 as connections.py restates it).  The copy records of both sides
// are built here from the connection's index map; the sender's volumes of the slice come
// back to the host (surface-sized) for the T-intersection test.
int geo_swap(agx_ctx* c, Conn& k) {
  const int ng = c->cfg.n_ghost;
  const agx_connection cc = k.c;           // (the borders as they are before this swap)
  std::vector<GeoCopy> rec[2];
  bool adj[2][4] = {};
  for (int recv = 0; recv < 2; ++recv) {
    const int snd = 1 - recv;
    Block& R = c->blocks[cc.local_block[recv]];
    Block& S = c->blocks[cc.local_block[snd]];
    std::vector<int> ca, cs;
    auto idxR = [&](int i, int j, int kk) { ca.push_back(i); ca.push_back(j); ca.push_back(kk);
                                            return R.d.idx(i, j, kk); };
    auto idxS = [&](int i, int j, int kk) { cs.push_back(i); cs.push_back(j); cs.push_back(kk);
                                            return S.d.idx(i, j, kk); };
    MapOut m;
    build_side_map(cc, recv, ng, idxR, idxS, m);
    const long n = (long)m.dst.size();
    if (n == 0) continue;
    // the sender's volume of every cell of the slice
    std::vector<double> svol(n);
    DevBuf<long> idx_dev;
    DevBuf<double> buf;
    HIPCHK(idx_dev.upload(m.src));
    HIPCHK(buf.alloc((size_t)n));
    hipLaunchKernelGGL(k_geo_gather1, geo_grid(n), dim3(256), 0, c->stream, S.d.vol,
                       idx_dev.get(), n, buf.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(svol.data(), buf.get(), sizeof(double) * n, hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int orient = cc.orientation;
    if (recv == 1) { if (orient == 4) orient = 5; else if (orient == 5) orient = 4; }
    int rd1, rd2, rd3, sd1, sd2, sd3;
    dirs_of(cc.boundary[recv], rd1, rd2, rd3);
    dirs_of(cc.boundary[snd], sd1, sd2, sd3);
    const int len1 = cc.d1_end[recv] - cc.d1_start[recv] + 2 * ng;
    const int len2 = cc.d2_end[recv] - cc.d2_start[recv] + 2 * ng;
    const int blk_start = cc.boundary[recv] % 2 == 0 ? cc.const_surf[recv] : -ng;
    const bool lluu = (cc.boundary[0] + cc.boundary[1]) % 2 == 0;
    const bool neg1 = orient == 3 || orient == 4 || orient == 7 || orient == 8;
    const bool neg2 = orient >= 5 && orient <= 8;
    const int nr[3] = {R.d.ni, R.d.nj, R.d.nk};
    auto& out = rec[recv];
    for (long q = 0; q < n; ++q) {
      const int* a = &ca[3 * q];
      const int* sc = &cs[3 * q];
      if (svol[q] == 0.0) {
        // T-intersection (procBlock.cpp:3213-3262): an empty sender cell on a line that is
        // physical in one in-plane direction only marks the patch border it lies on
        bool ph[3];
        for (int d = 0; d < 3; ++d) ph[d] = a[d] >= 0 && a[d] < nr[d];
        for (int d = 0; d < 3; ++d) {
          if (!(ph[d] && !ph[(d + 1) % 3] && !ph[(d + 2) % 3])) continue;
          if (d == rd1) adj[recv][a[rd2] < cc.d2_start[recv] ? 2 : 3] = true;
          else if (d == rd2) adj[recv][a[rd1] < cc.d1_start[recv] ? 0 : 1] = true;
        }
        continue;
      }
      const int l1 = a[rd1] - (cc.d1_start[recv] - ng), l2 = a[rd2] - (cc.d2_start[recv] - ng),
                l3 = a[rd3] - blk_start;
      out.push_back(GeoCopy{m.dst[q], m.src[q], 0, 0, 0, 0});
      out.push_back(GeoCopy{m.dst[q], m.src[q], 1, 0, 0, 0});
      auto put = [&](int dr, int ds, int a_off, int s_off, bool flip) {
        int ai[3] = {a[0], a[1], a[2]}, si[3] = {sc[0], sc[1], sc[2]};
        ai[dr] += a_off; si[ds] += s_off;
        out.push_back(GeoCopy{R.d.idx(ai[0], ai[1], ai[2]), S.d.idx(si[0], si[1], si[2]), 2, dr,
                              ds, flip ? 1 : 0});
      };
      // direction 3 (procBlock.cpp:3276-3300): lower/lower or upper/upper pairs take the
      // sender's face above the cell, running backwards, normal flipped
      const int s3 = lluu ? 1 : 0, fac3 = lluu ? -1 : 1;
      put(rd3, sd3, 0, s3, lluu);
      if (l3 == ng - 1) put(rd3, sd3, 1, s3 + fac3, lluu);
      const int drs[2] = {rd1, rd2}, dss[2] = {sd1, sd2}, lc[2] = {l1, l2},
                le[2] = {len1 - 1, len2 - 1};
      const bool ng_[2] = {neg1, neg2};
      for (int w = 0; w < 2; ++w) {
        if (!ng_[w]) {
          put(drs[w], dss[w], 0, 0, false);
          if (lc[w] == le[w]) put(drs[w], dss[w], 1, 1, false);
        } else {               // reversed: upper / lower faces swap
          put(drs[w], dss[w], 0, 1, true);
          if (lc[w] == le[w]) put(drs[w], dss[w], 1, 0, true);
        }
      }
    }
  }
  // both slices are taken (gathered) before either insert (utility.cpp:232-233)
  DevBuf<GeoCopy> rec_dev[2];
  DevBuf<double> buf_dev[2];
  for (int recv = 0; recv < 2; ++recv) {
    const long n = (long)rec[recv].size();
    if (n == 0) continue;
    Block& S = c->blocks[cc.local_block[1 - recv]];
    HIPCHK(rec_dev[recv].alloc((size_t)n));
    HIPCHK(buf_dev[recv].alloc((size_t)7 * n));
    HIPCHK(hipMemcpyAsync(rec_dev[recv].get(), rec[recv].data(), sizeof(GeoCopy) * n,
                          hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_geo_gather, geo_grid(n), dim3(256), 0, c->stream, geo_planes(S),
                       rec_dev[recv].get(), n, buf_dev[recv].get());
  }
  for (int recv = 0; recv < 2; ++recv) {
    const long n = (long)rec[recv].size();
    if (n == 0) continue;
    Block& R = c->blocks[cc.local_block[recv]];
    hipLaunchKernelGGL(k_geo_scatter, geo_grid(n), dim3(256), 0, c->stream, geo_planes(R),
                       rec_dev[recv].get(), n, buf_dev[recv].get());
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int recv = 0; recv < 2; ++recv)
    for (int q = 0; q < 4; ++q)
      if (adj[recv][q]) k.c.patch_border[4 * recv + q] = 1;
  return 0;
}

// SwapWallDist (gridLevel.cpp:261-285) of one connection, with its borders as SwapGeomSlice
// left them
int geo_swap_wall_dist(agx_ctx* c, Conn& k) {
  const int ng = c->cfg.n_ghost;
  const agx_connection& cc = k.c;
  DevBuf<long> dst_dev[2], src_dev[2];
  DevBuf<double> buf[2];
  long n[2] = {0, 0};
  for (int recv = 0; recv < 2; ++recv) {
    Block& R = c->blocks[cc.local_block[recv]];
    Block& S = c->blocks[cc.local_block[1 - recv]];
    auto idxR = [&](int i, int j, int kk) { return R.d.idx(i, j, kk); };
    auto idxS = [&](int i, int j, int kk) { return S.d.idx(i, j, kk); };
    MapOut m;
    build_side_map(cc, recv, ng, idxR, idxS, m);
    n[recv] = (long)m.dst.size();
    if (n[recv] == 0) continue;
    HIPCHK(dst_dev[recv].upload(m.dst));
    HIPCHK(src_dev[recv].upload(m.src));
    HIPCHK(buf[recv].alloc((size_t)n[recv]));
    hipLaunchKernelGGL(k_geo_gather1, geo_grid(n[recv]), dim3(256), 0, c->stream, S.d.wdist,
                       src_dev[recv].get(), n[recv], buf[recv].get());
  }
  for (int recv = 0; recv < 2; ++recv) {
    if (n[recv] == 0) continue;
    Block& R = c->blocks[cc.local_block[recv]];
    hipLaunchKernelGGL(k_geo_scatter1, geo_grid(n[recv]), dim3(256), 0, c->stream, R.d.wdist,
                       dst_dev[recv].get(), n[recv], buf[recv].get());
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));     // (the buffers go out of scope)
  return 0;
}

// agx_setup_finalize, node-built blocks: everything between the metrics and the index maps
int geo_complete(agx_ctx* c) {
  const int ng = c->cfg.n_ghost;
  for (auto& k : c->conns) {
    const agx_connection& cc = k.c;
    const bool l0 = cc.rank[0] == c->rank, l1 = cc.rank[1] == c->rank;
    if (!l0 && !l1) continue;
    if (!(l0 && l1))
      return fail("agx_setup_finalize: node-built blocks with a connection whose partner is on "
                  "another rank (blocks %d and %d): ghost geometry and wall points would have "
                  "to cross ranks; create the blocks from arrays for multi-rank runs",
                  cc.block[0], cc.block[1]);
    for (int s = 0; s < 2; ++s)
      if (cc.local_block[s] < 0 || cc.local_block[s] >= (int)c->blocks.size())
        return fail("connection refers to unknown block");
  }
  // face centres of the physical faces, for the pass only
  for (auto& b : c->blocks) {
    const BlockDev& d = b.d;
    if (!b.nodes_dev) return fail("agx_setup_finalize: the geometry of this context is complete");
    HIPCHK(b.fcen.alloc((size_t)9 * d.nplane));
    HIPCHK(hipMemsetAsync(b.fcen.get(), 0, sizeof(double) * 9 * d.nplane, c->stream));
    const long nn = (long)(d.ni + 1) * (d.nj + 1) * (d.nk + 1);
    hipLaunchKernelGGL(k_metrics_planes, geo_grid(nn), dim3(256), 0, c->stream, d,
                       b.nodes_dev.get(), geo_planes(b), 2, c->err_dev.get());
  }
  HIPCHK(hipGetLastError());
  // 1. AssignGhostCellsGeom: layer by layer, surface by surface in the given order
  for (auto& b : c->blocks) {
    const BlockDev& d = b.d;
    const int nd[3] = {d.ni, d.nj, d.nk};
    for (int layer = 1; layer <= ng; ++layer)
      for (const agx_bc_surface& s : b.surf_host) {
        if (s.bc_type == AGX_BC_INTERBLOCK) continue;
        GhostGeomOp o;
        const int st = surface_type(s);
        o.d3 = (st - 1) / 2; o.upper = st % 2 == 0; o.layer = layer;
        surface_range(s, o.lo, o.hi);
        o.n3 = nd[o.d3];
        const int da = o.d3 == 0 ? 1 : 0, db = o.d3 == 2 ? 1 : 2;
        const long n = (long)(o.hi[da] - o.lo[da] + 1) * (o.hi[db] - o.lo[db] + 1);
        hipLaunchKernelGGL(k_ghost_geom, geo_grid(n), dim3(256), 0, c->stream, d, geo_planes(b), o);
      }
  }
  HIPCHK(hipGetLastError());
  // 2. SwapGeomSlice, connection by connection in creation order
  for (auto& k : c->conns)
    if (k.c.is_interblock && k.c.rank[0] == c->rank && geo_swap(c, k)) return 1;
  // 3. AssignGhostCellsGeomEdge, then CalcCellWidths over the whole padded array
  for (auto& b : c->blocks) {
    const BlockDev& d = b.d;
    const int nd[3] = {d.ni, d.nj, d.nk};
    const GeoPlanes g = geo_planes(b);
    for (int dir = 0; dir < 3; ++dir) {
      EdgeGeomOp o;
      o.d = dir; o.two = (dir + 1) % 3; o.three = (dir + 2) % 3; o.nd = nd[dir];
      const int max2 = nd[o.two], max3 = nd[o.three];
      for (int layer3 = 1; layer3 <= ng; ++layer3)
        for (int layer2 = 1; layer2 <= ng; ++layer2)
          for (int cn = 0; cn < 4; ++cn) {
            o.u2 = cn > 1; o.u3 = cn % 2 == 1;
            o.p2 = o.u2 ? max2 + layer2 - 2 : 1 - layer2;
            o.g2 = o.u2 ? o.p2 + 1 : o.p2 - 1;
            o.i2 = o.u2 ? max2 - layer2 : layer2 - 1;
            o.p3 = o.u3 ? max3 + layer3 - 2 : 1 - layer3;
            o.g3 = o.u3 ? o.p3 + 1 : o.p3 - 1;
            hipLaunchKernelGGL(k_edge_geom, geo_grid(o.nd + 1), dim3(256), 0, c->stream, d, g, o);
          }
    }
    const long ncell = (long)(d.ni + 2 * ng) * (d.nj + 2 * ng) * (d.nk + 2 * ng);
    hipLaunchKernelGGL(k_cell_widths, geo_grid(ncell), dim3(256), 0, c->stream, d, g, d.wid[0],
                       d.wid[1], d.wid[2]);
  }
  HIPCHK(hipGetLastError());
  // 4. wall distance (main.cpp:191-203, procBlock::CalcWallDistance, SwapWallDist)
  if (c->cfg.is_viscous) {
    long nwall = 0;
    for (auto& b : c->blocks)
      for (const agx_bc_surface& s : b.surf_host) {
        if (s.bc_type != AGX_BC_VISCOUSWALL) continue;
        int lo[3], hi[3];
        surface_range(s, lo, hi);
        nwall += (long)(hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]);
      }
    if (nwall > 0) {
      DevBuf<double> wall_pts;
      HIPCHK(wall_pts.alloc((size_t)3 * nwall));
      double* const wall = wall_pts.get();
      long off = 0;
      for (auto& b : c->blocks)
        for (const agx_bc_surface& s : b.surf_host) {
          if (s.bc_type != AGX_BC_VISCOUSWALL) continue;
          int lo[3], hi[3];
          surface_range(s, lo, hi);
          const long n = (long)(hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]);
          hipLaunchKernelGGL(k_wall_points, geo_grid(n), dim3(256), 0, c->stream, b.d,
                             geo_planes(b), (surface_type(s) - 1) / 2, lo[0], lo[1], lo[2], hi[0],
                             hi[1], hi[2], wall + 3 * off);
          off += n;
        }
      for (auto& b : c->blocks) {
        const BlockDev& d = b.d;
        const long ncell = (long)d.ni * d.nj * d.nk;
        hipLaunchKernelGGL(k_nearest_wall_planes, geo_grid(ncell), dim3(256), 0, c->stream, d,
                           geo_planes(b), nwall, wall);
        for (const agx_bc_surface& s : b.surf_host) {
          int lo[3], hi[3];
          surface_range(s, lo, hi);
          const int st = surface_type(s);
          const long n = (long)(hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]) * ng;
          hipLaunchKernelGGL(k_wall_dist_ghosts, geo_grid(n), dim3(256), 0, c->stream, d, d.wdist,
                             (st - 1) / 2, st % 2 == 0 ? 1 : 0,
                             s.bc_type == AGX_BC_VISCOUSWALL ? 1 : 0, lo[0], lo[1], lo[2], hi[0],
                             hi[1], hi[2]);
        }
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(c->stream));
      wall_pts.reset();
      for (auto& k : c->conns)
        if (k.c.rank[0] == c->rank && geo_swap_wall_dist(c, k)) return 1;
    }
  }
  // 5. what agx_block_create does after its uploads
#if AGX_FAST
  for (auto& b : c->blocks)
    if (b.d.d2.base) {
      const long n = (long)b.d.d2.Pi * b.d.d2.Pj * (b.d.nk + 2 * b.d.ng);
      hipLaunchKernelGGL(k_d2_geo, dim3((n + 255) / 256), dim3(256), 0, c->stream, b.d);
    }
  HIPCHK(hipGetLastError());
#endif
  // 6. the moments of the integrated wall loads keep the centres of the load-surface faces
  for (auto& b : c->blocks) {
    if (b.load_faces == 0) continue;
    HIPCHK(b.load_fcen.alloc((size_t)3 * b.load_faces));
    hipLaunchKernelGGL(k_load_centres, geo_grid(b.load_faces), dim3(256), 0, c->stream, b.d,
                       b.fcen.get(), b.load_tab_dev.get(), (int)b.load_tab.size(), b.load_faces,
                       b.load_fcen.get());
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  for (auto& b : c->blocks) {
    b.fcen.reset();
    b.nodes_dev.reset();
  }
  return 0;
}
}  // namespace

extern "C" {

const char* agx_last_error(void) { return g_err; }
const char* agx_version(void) {
#if AGX_TPG
  return "aither_gfx950 0.1 (HIP, gfx950, thermallyPerfect)";
#else
  return "aither_gfx950 0.1 (HIP, gfx950)";
#endif
}

int agx_ctx_create(int device, int rank, agx_ctx** out) {
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail("no HIP device available (%s): the gfx950 library has no CPU "
                "path", hipGetErrorString(e));
  if (device < 0 || device >= ndev) return fail("device %d out of range", device);
  HIPCHK(hipSetDevice(device));
  // (the half-built context goes with every failing return)
  std::unique_ptr<agx_ctx> c(new agx_ctx());
  c->device = device;
  c->rank = rank;
  if (const BadSwitch bad = parse_switches(getenv, *c)) return fail("%s", bad.message().c_str());
  static_assert(TILE_ORDER_STEP == 1 && TILE_ORDER_COLUMN == 0, "AGX_TILE_ORDER's table values");
  int ncu = 0;
  HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
  if (ncu > 0) c->num_cu = ncu;
  if (c->workgroups > 0) c->num_cu = c->workgroups;
  HIPCHK(c->err_dev.alloc(1));
  HIPCHK(hipMemset(c->err_dev.get(), 0, sizeof(int)));
  HIPCHK(c->err_host.alloc(1));
  *c->err_host.get() = 0;
  *out = c.release();
  return 0;
}

void agx_ctx_destroy(agx_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  if (c->nccl) ncclCommDestroy(c->nccl);
  for (auto& e : c->ev_pool) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
  if (c->cap_stream) hipStreamDestroy(c->cap_stream);
  if (c->ov_stream) {
    hipStreamSynchronize(c->ov_stream);
    hipStreamDestroy(c->ov_stream);
    hipEventDestroy(c->ov_ready);
    hipEventDestroy(c->ov_done);
  }
  for (auto ev : c->branch_events) hipEventDestroy(ev);
  for (auto st : c->branch_streams) hipStreamDestroy(st);
  delete c;     // (memory and graphs go with their owners, on the context's device)
}

int agx_ctx_set_stream(agx_ctx* c, void* s) {
  // at any time: what was queued on the old stream (set-up memsets, a previous iteration)
  // is finished before work is issued on the new one
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->stream = (hipStream_t)s;
  return 0;
}

int agx_config_set(agx_ctx* c, const agx_config* cfg) {
  // allocations (block-matrix planes, sweep records, D2 arrays) and the captured sweep
  // graphs are decided from the configuration a block was created under
  if (!c->blocks.empty())
    return fail("agx_config_set: the configuration is fixed after the first "
                "agx_block_create (make a new context for another scheme)");
  if (cfg->n_eq != AGX_NEQ)
    return fail("n_eq = %d: this library is built for %d equations (5: euler / "
                "navierStokes, libaither_gfx950.so; 7: rans, libaither_gfx950_rans.so)",
                cfg->n_eq, AGX_NEQ);
  if (cfg->n_ghost < 1 || cfg->n_ghost > 3) return fail("n_ghost out of range");
#if AGX_TPG
  if (cfg->thermodynamic_model != AGX_THERMO_THERMALLY_PERFECT)
    return fail("thermodynamic_model %d: this library is built for the thermally perfect gas "
                "(caloricallyPerfect: %s)", cfg->thermodynamic_model,
                AGX_NEQ == 7 ? "libaither_gfx950_rans.so" : "libaither_gfx950.so");
  if (cfg->gas.n_vib < 0 || cfg->gas.n_vib > AGX_MAX_VIB)
    return fail("gas.n_vib = %d: 0 to %d vibrational modes are built", cfg->gas.n_vib,
                AGX_MAX_VIB);
  for (int m = 0; m < cfg->gas.n_vib; ++m)
    if (!(cfg->gas.theta_v[m] > 0.0))
      return fail("gas.theta_v[%d] = %g: vibrational temperatures are positive", m,
                  cfg->gas.theta_v[m]);
#else
  if (cfg->thermodynamic_model != AGX_THERMO_CALORICALLY_PERFECT)
    return fail("thermodynamic_model %d: this library is built for the calorically perfect "
                "gas (thermallyPerfect: %s)", cfg->thermodynamic_model,
                AGX_NEQ == 7 ? "libaither_gfx950_rans_tp.so" : "libaither_gfx950_tp.so");
#endif
  // Never substitute: a scheme this build does not implement is an error here,
  // not a different scheme silently (mgSolution.hpp:112-115 must mean the same).
#if AGX_NEQ == 7
  if (cfg->equation_set != AGX_EQN_RANS || !cfg->is_viscous)
    return fail("the 7-equation library serves equation_set rans (viscous) only");
  if (cfg->turbulence_model != AGX_TURB_SST2003 && cfg->turbulence_model != AGX_TURB_KW_WILCOX2006 &&
      cfg->turbulence_model != AGX_TURB_SST_DES)
    return fail("turbulence_model %d: sst2003, sstdes and kOmegaWilcox2006 are built",
                cfg->turbulence_model);
  if (cfg->inv_flux_jacobian == AGX_JACOBIAN_APPROX_ROE)
    return fail("rans: approximateRoe is not built");
#else
  const bool les = cfg->equation_set == AGX_EQN_LES;
  if (cfg->equation_set != AGX_EQN_EULER && cfg->equation_set != AGX_EQN_NAVIER_STOKES && !les)
    return fail("equation_set %d: this library covers euler, navierStokes and "
                "largeEddySimulation (rans: libaither_gfx950_rans.so)", cfg->equation_set);
  if ((cfg->equation_set == AGX_EQN_NAVIER_STOKES || les) != (cfg->is_viscous != 0))
    return fail("equation_set %d contradicts is_viscous %d", cfg->equation_set, cfg->is_viscous);
  // input::CheckTurbulenceModel input.cpp:965-979
  if (les && cfg->turbulence_model != AGX_TURB_WALE)
    return fail("equation_set largeEddySimulation with turbulence_model %d: it accepts wale "
                "only, and needs it (input.cpp:965-969, :979-982)", cfg->turbulence_model);
  if (!les && cfg->turbulence_model == AGX_TURB_WALE)
    return fail("turbulence_model wale with equation_set %d: wale is the model of "
                "largeEddySimulation and of no other equation set (input.cpp:970-978)",
                cfg->equation_set);
  if (cfg->turbulence_model != AGX_TURB_NONE && !les)
    return fail("turbulence_model %d is not built (laminar / inviscid, or wale with "
                "largeEddySimulation)", cfg->turbulence_model);
  if (les && cfg->time_integration >= AGX_TIME_IMPLICIT_EULER)
    return fail("largeEddySimulation with an implicit time_integration (%d: implicitEuler, "
                "crankNicholson, bdf2) is not built: the scalar and block off-diagonals and "
                "diagonals with an eddy viscosity in a 5-equation run have no independent "
                "reference while the oracle does not carry the model; explicitEuler and rk4 "
                "are built", cfg->time_integration);
#endif
  if (cfg->inv_flux_jacobian != AGX_JACOBIAN_RUSANOV &&
      cfg->inv_flux_jacobian != AGX_JACOBIAN_APPROX_ROE)
    return fail("inv_flux_jacobian %d is not one of rusanov / approximateRoe",
                cfg->inv_flux_jacobian);
  if (cfg->inv_flux_jacobian == AGX_JACOBIAN_APPROX_ROE && cfg->is_viscous)
    return fail("approximateRoe with viscous terms is not built: the reference hands dist and "
                "f1 to RoeOffDiagonal in swapped order (fluxJacobian.cpp:232 vs :240) and "
                "divides by f1 = 0 in laminar runs");
  if (cfg->viscous_recon != AGX_VISC_RECON_CENTRAL &&
      cfg->viscous_recon != AGX_VISC_RECON_CENTRAL_4TH)
    return fail("viscous_recon %d is not one of central / centralFourth", cfg->viscous_recon);
  if (cfg->viscous_recon == AGX_VISC_RECON_CENTRAL_4TH && cfg->n_ghost < 2)
    return fail("centralFourth needs two ghost layers (input::NumberGhostLayers, "
                "input.cpp:1127-1143)");
  if (cfg->matrix_solver < AGX_SOLVER_LUSGS || cfg->matrix_solver > AGX_SOLVER_BDPLUR)
    return fail("matrix_solver %d is not one of lusgs / dplur / blusgs / bdplur",
                cfg->matrix_solver);
  if ((cfg->matrix_solver == AGX_SOLVER_BLUSGS || cfg->matrix_solver == AGX_SOLVER_BDPLUR) &&
      cfg->inv_flux_jacobian == AGX_JACOBIAN_APPROX_ROE)
    return fail("block-matrix solvers are built for inviscidFluxJacobian rusanov only");
  c->cfg = *cfg;
  derive_gas(*cfg, c->gas);
  c->gas.wilcox = cfg->turbulence_model == AGX_TURB_KW_WILCOX2006 ? 1 : 0;
  c->gas.sstdes = cfg->turbulence_model == AGX_TURB_SST_DES ? 1 : 0;
  c->gas.turb_prandtl = c->gas.wilcox ? 8.0 / 9.0 : 0.9;
#if AGX_TPG
  c->gas.err = c->err_dev.get();
#endif
  SolverDev& sp = c->sp;
  sp.diag_add = 0;
  sp.kappa = cfg->kappa;
  sp.theta = cfg->theta;
  sp.zeta = cfg->zeta;
  sp.relax = cfg->matrix_relaxation;
  sp.dual_time_cfl = cfg->dual_time_cfl;
  sp.dt_fixed = cfg->dt_nondim;
  sp.visc_cfl_coeff = cfg->viscous_cfl_coeff;
  sp.viscous = cfg->is_viscous;
  sp.implicit = cfg->time_integration >= AGX_TIME_IMPLICIT_EULER;
  sp.bdf2 = cfg->time_integration == AGX_TIME_BDF2;
  // input::MatrixRequiresInitialization input.cpp:1120-1125
  sp.requires_init = cfg->matrix_solver == AGX_SOLVER_DPLUR ||
                     cfg->matrix_solver == AGX_SOLVER_BDPLUR || cfg->matrix_sweeps > 1;
  sp.block = (cfg->matrix_solver == AGX_SOLVER_BLUSGS || cfg->matrix_solver == AGX_SOLVER_BDPLUR) ? 1 : 0;
  sp.time_integration = cfg->time_integration;
  sp.roe_jacobian = cfg->inv_flux_jacobian == AGX_JACOBIAN_APPROX_ROE;
  sp.les = cfg->equation_set == AGX_EQN_LES ? 1 : 0;
  c->have_cfg = true;
  return 0;
}

int agx_block_create(agx_ctx* c, const agx_block_geom* g, int* block_id) {
  if (!c->have_cfg) return fail("agx_config_set must precede agx_block_create");
  if (g->ng != c->cfg.n_ghost) return fail("block ghost layers != config n_ghost");
  if (g->ni < 1 || g->nj < 1 || g->nk < 1) return fail("empty block");
  const bool from_nodes = g->nodes != nullptr;
  if (from_nodes) {
    const double* arr[9] = {g->farea_i, g->farea_j, g->farea_k, g->vol, g->center, g->width_i,
                            g->width_j, g->width_k, g->wall_dist};
    const char* nm[9] = {"farea_i", "farea_j", "farea_k", "vol", "center", "width_i", "width_j",
                         "width_k", "wall_dist"};
    for (int q = 0; q < 9; ++q)
      if (arr[q])
        return fail("agx_block_create: nodes given together with %s (a block is built from "
                    "its nodes or from the nine arrays)", nm[q]);
  }
  if (!c->blocks.empty() && c->blocks[0].node_built != from_nodes)
    return fail("agx_block_create: a context holds node-built or array-built blocks, not both");
  HIPCHK(hipSetDevice(c->device));
  c->blocks.emplace_back();
  Block& b = c->blocks.back();
  BlockDev& d = b.d;
  memset(&d, 0, sizeof d);
  d.ni = g->ni; d.nj = g->nj; d.nk = g->nk; d.ng = g->ng;
  d.parent = g->parent_block;
  b.global_pos = g->global_pos;
  d.ioff = 16;                               // physical i = 0 on a 128-B line
  const long row = d.ioff + d.ni + d.ng + 1; // +1: upper i-face
  d.sx = (row + 15) / 16 * 16;
  d.sxy = d.sx * (d.nj + 2 * d.ng + 1);
  d.nplane = d.sxy * (d.nk + 2 * d.ng + 1);
  // one slab for all planes of the block (see SlabDev in agx_kernels.hpp)
  // (largeEddySimulation: one plane more, eddyViscosity_ of the cells; every other run keeps
  // its footprint)
  const int nplanes = PL_COUNT + (c->sp.les ? 1 : 0);
  HIPCHK(b.slab.alloc((size_t)d.nplane * nplanes));
  HIPCHK(hipMemsetAsync(b.slab.get(), 0, sizeof(double) * d.nplane * nplanes, c->stream));
  auto pl = [&](int id) { return b.slab.get() + (long)id * d.nplane; };
  d.vol = pl(PL_VOL); d.specrad = pl(PL_SPECRAD); d.dt = pl(PL_DT);
  d.a = pl(PL_A); d.ainv = pl(PL_AINV); d.wdist = pl(PL_WDIST);
  for (int e = 0; e < AGX_NEQ; ++e) {
    d.state[e] = pl(PL_STATE_A + e); d.state2[e] = pl(PL_STATE_B + e);
    d.resid[e] = pl(PL_RESID + e); d.consn[e] = pl(PL_CONSN + e);
    d.consnm1[e] = pl(PL_CONSNM1 + e); d.x[e] = pl(PL_X + e);
    d.xold[e] = pl(PL_XOLD + e);
  }
  for (int q = 0; q < 3; ++q) {
    d.cen[q] = pl(PL_CEN + q);
    d.wid[q] = pl(PL_WID + q);
    for (int cc = 0; cc < 4; ++cc) d.fa[q][cc] = pl(PL_FA + 4 * q + cc);
  }
  b.state_is_a = true;
#if AGX_NEQ == 7
  d.specrad_t = pl(PL_SPECRAD_T); d.a_t = pl(PL_A_T); d.ainv_t = pl(PL_AINV_T);
  d.viscp = pl(PL_VISC);
  for (int q = 0; q < 3; ++q) d.turb3[q] = pl(PL_TURB3 + q);
#else
  if (c->sp.les) d.turb3[0] = pl(PL_EDDY_LES);
#endif
  if (c->sp.implicit && is_block_solver(c)) {
    // a_, aInv_ (25 planes each) and velocityGrad_ (9) of the block-matrix solvers
    // (+ 2 x 2 planes: diagonal of the turbulence block in the rans build)
    const size_t n = (size_t)d.nplane * (2 * AGX_NJ + 9 + 4);
    HIPCHK(b.blockmat.alloc(n));
    HIPCHK(hipMemsetAsync(b.blockmat.get(), 0, sizeof(double) * n, c->stream));
    d.am = b.blockmat.get();
    d.aminv = d.am + (size_t)d.nplane * AGX_NJ;
    d.vg = d.am + (size_t)d.nplane * 2 * AGX_NJ;
    d.am_t = d.vg + (size_t)d.nplane * 9;
    d.aminv_t = d.am_t + (size_t)d.nplane * 2;
  }
  d.sw_geo = d.sw_dyn = d.sw_rhs = nullptr;
  d.mg_forcing = d.mg_mres = d.mg_xsave = nullptr;
  if (c->sp.implicit && is_lusgs_solver(c) && !use_d2(c) && c->sweep_records) {
    const size_t n = (size_t)d.nplane * (SW_GEO + SW_DYN + SW_RHS);
    HIPCHK(b.sweep_rec.alloc(n));
    HIPCHK(hipMemsetAsync(b.sweep_rec.get(), 0, sizeof(double) * n, c->stream));
    d.sw_geo = b.sweep_rec.get();
    d.sw_dyn = d.sw_geo + (size_t)d.nplane * SW_GEO;
    d.sw_rhs = d.sw_dyn + (size_t)d.nplane * SW_DYN;
  }
  if (use_d2(c) && std::min(d.ni, d.nj) > KP_MAX_DIAG)
    return fail("LU-SGS: a block with min(ni, nj) = %d exceeds the %d cells per diagonal "
                "the sweep kernel holds in LDS (AGX_LUSGS=plane has no such limit)",
                std::min(d.ni, d.nj), KP_MAX_DIAG);
  if (use_d2(c)) {
    // diagonal-ordered arrays of the LU-SGS path (agx_lusgs.hpp)
    D2Dev& z = d.d2;
    z.Pi = d.ni + 2 * d.ng; z.Pj = d.nj + 2 * d.ng;
    z.ps = ((long)z.Pi * z.Pj + 15) / 16 * 16;
    z.nd2 = z.ps * (d.nk + 2 * d.ng);
    b.dstart.assign(z.Pi + z.Pj + 1, 0);
    std::vector<int> tab(z.Pi + z.Pj + 1 + (size_t)z.Pi * z.Pj);
    for (int de = 0; de < z.Pi + z.Pj - 1; ++de) {
      const int jl = std::max(0, de - (z.Pi - 1)), jh = std::min(z.Pj - 1, de);
      b.dstart[de + 1] = b.dstart[de] + (jh - jl + 1);
      for (int je = jl; je <= jh; ++je)
        tab[z.Pi + z.Pj + 1 + b.dstart[de] + (je - jl)] = (de - je) | (je << 16);
    }
    b.dstart[z.Pi + z.Pj] = b.dstart[z.Pi + z.Pj - 1];
    std::copy(b.dstart.begin(), b.dstart.end(), tab.begin());
    HIPCHK(b.d2_tab.upload(tab));
    z.dstart = b.d2_tab.get();
    z.ij_of_pos = z.dstart + z.Pi + z.Pj + 1;
    HIPCHK(b.d2.alloc((size_t)z.nd2 * D2_DOUBLES));
    HIPCHK(hipMemsetAsync(b.d2.get(), 0, sizeof(double) * z.nd2 * D2_DOUBLES, c->stream));
    z.base = b.d2.get();
  }
  b.node_built = from_nodes;
  if (from_nodes) {
    if (geo_block_metrics(c, b, g->nodes)) return 1;
    *block_id = (int)c->blocks.size() - 1;
    return 0;
  }
  const int ci = d.ni + 2 * d.ng, cj = d.nj + 2 * d.ng, ck = d.nk + 2 * d.ng;
  if (upload_aos(c, b, g->farea_i, d.fa[0], 4, ci + 1, cj, ck, d.ng)) return 1;
  if (upload_aos(c, b, g->farea_j, d.fa[1], 4, ci, cj + 1, ck, d.ng)) return 1;
  if (upload_aos(c, b, g->farea_k, d.fa[2], 4, ci, cj, ck + 1, d.ng)) return 1;
  double* volp[1] = {d.vol};
  if (upload_aos(c, b, g->vol, volp, 1, ci, cj, ck, d.ng)) return 1;
  if (upload_aos(c, b, g->center, d.cen, 3, ci, cj, ck, d.ng)) return 1;
  const double* wsrc[3] = {g->width_i, g->width_j, g->width_k};
  for (int q = 0; q < 3; ++q) {
    double* wp[1] = {d.wid[q]};
    if (upload_aos(c, b, wsrc[q], wp, 1, ci, cj, ck, d.ng)) return 1;
  }
#if AGX_FAST
  if (d.d2.base) {
    const long n = (long)d.d2.Pi * d.d2.Pj * (d.nk + 2 * d.ng);
    hipLaunchKernelGGL(k_d2_geo, dim3((n + 255) / 256), dim3(256), 0, c->stream, d);
  }
#endif
  HIPCHK(hipGetLastError());
  if (g->wall_dist) {
    double* wp[1] = {d.wdist};
    if (upload_aos(c, b, g->wall_dist, wp, 1, ci, cj, ck, d.ng)) return 1;
  }
  *block_id = (int)c->blocks.size() - 1;
  return 0;
}

int agx_block_set_bcs(agx_ctx* c, int id, int n, const agx_bc_surface* s) {
  if (id < 0 || id >= (int)c->blocks.size()) return fail("bad block id %d", id);
  Block& b = c->blocks[id];
  b.sweep_graph.drop();                      // (they hold the old BlockDev)
  b.flux_tab_built = false;
  b.surf_host.assign(s, s + n);
  // (a view in b.d follows its owner only once the owner holds the new memory: a failing
  // call leaves none dangling)
  b.d.surf = nullptr;
  b.d.nsurf = 0;
  HIPCHK(b.surf_dev.alloc(n > 0 ? n : 1));
  HIPCHK(hipMemcpy(b.surf_dev.get(), s, sizeof(agx_bc_surface) * n, hipMemcpyHostToDevice));
  b.d.surf = b.surf_dev.get();
  b.d.nsurf = n;
  b.d.nsurf_i = b.d.nsurf_j = b.d.nsurf_k = 0;
  int n_conn[6] = {0, 0, 0, 0, 0, 0}, n_other[6] = {0, 0, 0, 0, 0, 0};
  for (int q = 0; q < n; ++q) {
    const int st = surface_type(s[q]);
    if (st <= 2) b.d.nsurf_i++; else if (st <= 4) b.d.nsurf_j++; else b.d.nsurf_k++;
    const int t = s[q].bc_type;
    if (t < AGX_BC_SLIPWALL || t > AGX_BC_PERIODIC) return fail("unknown bc type %d", t);
    if (t == AGX_BC_INTERBLOCK || t == AGX_BC_PERIODIC) n_conn[st - 1]++; else n_other[st - 1]++;
    if (t == AGX_BC_VISCOUSWALL && s[q].state.is_wall_law) {
      // wall functions: the 7-equation library (wallLaw::AdiabaticBCs / HeatFluxBCs / IsothermalBCs)
      if (AGX_NEQ == 5) return fail("wallTreatment=wallLaw needs the rans library");
    }
  }
  for (int q = 0; q < 6; ++q)
    b.d.side_conn[q] = n_conn[q] == 0 ? 0 : (n_other[q] == 0 ? 1 : 2);
  // nonreflecting inlet / outlet surfaces keep the gradients of their adjacent cells
  // and their Mach mean / maximum between a residual and the next ghost fills
  b.d.nr_off = nullptr; b.d.nr_grad = nullptr; b.d.nr_mach = nullptr;
  b.nr_off_dev.reset();
  b.nr_mem.reset();
  b.nr_max = 0;
  std::vector<int> off(n > 0 ? n : 1, -1);
  long total = 0, nr_max = 0;
  for (int q = 0; q < n; ++q) {
    const int t = s[q].bc_type;
    if (!s[q].state.is_nonreflecting || (t != AGX_BC_INLET && t != AGX_BC_PRESSURE_OUTLET)) continue;
    const int st = surface_type(s[q]);
    const int d3 = (st - 1) / 2, d1 = (d3 + 1) % 3, d2 = (d3 + 2) % 3;
    const int lo[3] = {s[q].imin, s[q].jmin, s[q].kmin}, hi[3] = {s[q].imax, s[q].jmax, s[q].kmax};
    const long cells = (long)(hi[d1] - lo[d1]) * (hi[d2] - lo[d2]);
    off[q] = (int)total;
    total += cells;
    nr_max = std::max(nr_max, cells);
  }
  if (total > 0) {
    HIPCHK(b.nr_off_dev.upload(off.data(), (size_t)n));
    const size_t nd = (size_t)12 * total + 2 * (size_t)n;
    HIPCHK(b.nr_mem.alloc(nd));
    HIPCHK(hipMemset(b.nr_mem.get(), 0, sizeof(double) * nd));   // gradients before the first residual
    b.d.nr_off = b.nr_off_dev.get();
    b.d.nr_grad = b.nr_mem.get();
    b.d.nr_mach = b.nr_mem.get() + 12 * total;
    b.nr_max = nr_max;
  }
  // wall-law surfaces keep the wall data of their faces (wallData_, wallData.hpp:33-62)
  // from the viscous ghost fill to the viscous fluxes of the same residual
  b.d.wall_off = nullptr; b.d.wallv = nullptr;
  b.wall_off_dev.reset();
  b.wall_mem.reset();
  std::fill(off.begin(), off.end(), -1);
  total = 0;
  for (int q = 0; q < n; ++q) {
    if (s[q].bc_type != AGX_BC_VISCOUSWALL || !s[q].state.is_wall_law) continue;
    const int st = surface_type(s[q]);
    const int d3 = (st - 1) / 2, d1 = (d3 + 1) % 3, d2 = (d3 + 2) % 3;
    const int lo[3] = {s[q].imin, s[q].jmin, s[q].kmin}, hi[3] = {s[q].imax, s[q].jmax, s[q].kmax};
    off[q] = (int)total;
    total += (long)(hi[d1] - lo[d1]) * (hi[d2] - lo[d2]);
  }
  if (total > 0) {
    HIPCHK(b.wall_off_dev.upload(off.data(), (size_t)n));
    HIPCHK(b.wall_mem.alloc((size_t)total));
    // y+ = 0: low-Re until the first ghost fill
    HIPCHK(hipMemset(b.wall_mem.get(), 0, sizeof(WallVars) * (size_t)total));
    b.d.wall_off = b.wall_off_dev.get();
    b.d.wallv = b.wall_mem.get();
    c->have_wall_data = false;
  }
  // the table of the wall-surface output (agx_output_pack with AGX_WALL_*)
  b.wall_tab_dev.reset();
  b.wall_tab.clear();
  b.wall_faces = 0;
  ++b.wall_epoch;
  for (int q = 0; q < n; ++q) {
    if (s[q].bc_type != AGX_BC_VISCOUSWALL) continue;
    WallSurfDev w;
    const int lo[3] = {s[q].imin, s[q].jmin, s[q].kmin}, hi[3] = {s[q].imax, s[q].jmax, s[q].kmax};
    const int nn[3] = {b.d.ni, b.d.nj, b.d.nk};
    w.side = surface_type(s[q]);
    const int d3 = (w.side - 1) / 2;
    for (int d = 0; d < 3; ++d) {
      w.lo[d] = lo[d];
      w.n[d] = d == d3 ? 1 : hi[d] - lo[d];
      // (the kernel indexes the planes from these: they must lie on the block)
      if (lo[d] < 0 || hi[d] > nn[d] || w.n[d] < 1 || (d == d3 && lo[d] != 0 && lo[d] != nn[d]))
        return fail("viscousWall surface %d does not lie on a side of block %d", q, id);
    }
    w.off = b.wall_faces;
    b.wall_faces += (long)w.n[0] * w.n[1] * w.n[2];
    b.wall_tab.push_back(w);
  }
  HIPCHK(b.wall_tab_dev.upload(b.wall_tab));
  // the table of the integrated wall loads (agx_output_pack with AGX_LOAD_*): viscousWall
  // and slipWall surfaces, each cut into chunks of LOAD_CHUNK faces of its own
  b.load_tab_dev.reset();
  b.load_partial.reset();
  b.load_fcen.reset();
  b.load_tab.clear();
  b.load_faces = b.load_chunks = 0;
  for (int q = 0; q < n; ++q) {
    if (s[q].bc_type != AGX_BC_VISCOUSWALL && s[q].bc_type != AGX_BC_SLIPWALL) continue;
    LoadSurfDev w;
    const int lo[3] = {s[q].imin, s[q].jmin, s[q].kmin}, hi[3] = {s[q].imax, s[q].jmax, s[q].kmax};
    const int nn[3] = {b.d.ni, b.d.nj, b.d.nk};
    w.side = surface_type(s[q]);
    w.visc = s[q].bc_type == AGX_BC_VISCOUSWALL ? 1 : 0;
    const int d3 = (w.side - 1) / 2;
    for (int d = 0; d < 3; ++d) {
      w.lo[d] = lo[d];
      w.n[d] = d == d3 ? 1 : hi[d] - lo[d];
      if (lo[d] < 0 || hi[d] > nn[d] || w.n[d] < 1 || (d == d3 && lo[d] != 0 && lo[d] != nn[d]))
        return fail("wall surface %d does not lie on a side of block %d", q, id);
    }
    const long faces = (long)w.n[0] * w.n[1] * w.n[2];
    w.off = b.load_faces;
    w.chunk0 = b.load_chunks;
    b.load_faces += faces;
    b.load_chunks += (faces + LOAD_CHUNK - 1) / LOAD_CHUNK;
    b.load_tab.push_back(w);
  }
  HIPCHK(b.load_tab_dev.upload(b.load_tab));
  if (b.load_chunks > 0) HIPCHK(b.load_partial.alloc((size_t)b.load_chunks * LOAD_NQ));
  return 0;
}

int agx_conn_create(agx_ctx* c, const agx_connection* cc, int* conn_id) {
  c->conns.emplace_back();
  c->conns.back().c = *cc;
  for (auto& b : c->blocks) b.flux_tab_built = false;   // (remote connections leave the table)
  *conn_id = (int)c->conns.size() - 1;
  return 0;
}

// workgroups of k_matrix_resid_d2m: (patch, k-chunk) pairs as agx_mresid_plan.hpp deals them;
// of k_matrix_resid_d2: 8 XCDs x mresid_split bands x chunks per band x nk
#ifndef AGX_MRESID_KC
#define AGX_MRESID_KC 32
#endif
constexpr int MRESID_KC = AGX_MRESID_KC;   // planes a workgroup of k_matrix_resid_d2m marches
long mresid_wgs(const agx_ctx* c, const BlockDev& b) {
  if (c->mresid_march)
    return mrp_wgs(mrp_patches(MrpPlane{b.d2.Pi, b.d2.Pj, b.ng}), b.nk, MRESID_KC);
  const long nchunk = ((long)b.d2.Pi * b.d2.Pj + 255) / 256;
  const long bands = 8L * c->mresid_split;
  return bands * ((nchunk + bands - 1) / bands) * b.nk;
}

namespace {
// The local connections exchanged in as few launches as their order allows.  The reference
// takes them one after the other (multiArray3d.hpp:790-828: slice both sides, insert both):
// where patches border other connections a later slice reads ghost cells an earlier insert
// wrote, and two inserts write the same edge ghost cells.  Connections are therefore put
// into levels -- "all slices of the level, then all its inserts", one gather and one scatter
// launch per level -- such that a connection comes after (a higher level than) every earlier
// one whose insert it reads or overwrites, and not before (the same level will do: slices
// precede inserts) an earlier one whose slice reads what it inserts; checked cell by cell.
int halo_batch_plan(agx_ctx* c, long* max_halo) {
  int sides = 0;
  long total = 0;
  std::vector<std::vector<unsigned char>> wlev(c->blocks.size()), rlev(c->blocks.size());
  auto flags = [&](std::vector<std::vector<unsigned char>>& v, int blk) -> std::vector<unsigned char>& {
    if (v[blk].empty()) v[blk].assign((size_t)c->blocks[blk].d.nplane, 0);
    return v[blk];
  };
  std::vector<std::pair<int, int>> order;        // (level, connection)
  int nlev = 0;
  for (size_t n = 0; n < c->conns.size(); ++n) {
    auto& k = c->conns[n];
    const agx_connection& cc = k.c;
    if (!(cc.rank[0] == c->rank && cc.rank[1] == c->rank)) continue;
    int lev = 1;
    for (int sd = 0; sd < 2; ++sd) {
      // side sd is filled from cells of the partner block
      const auto& wr = flags(wlev, cc.local_block[1 - sd]);
      for (long q : k.side[sd].h_src) lev = std::max(lev, wr[(size_t)q] + 1);
      const auto& ww = flags(wlev, cc.local_block[sd]);
      const auto& rr = flags(rlev, cc.local_block[sd]);
      for (long q : k.side[sd].h_dst)
        lev = std::max(lev, std::max<int>(ww[(size_t)q] + 1, rr[(size_t)q]));
    }
    lev = std::min(lev, 250);
    for (int sd = 0; sd < 2; ++sd) {
      auto& rr = flags(rlev, cc.local_block[1 - sd]);
      for (long q : k.side[sd].h_src) rr[(size_t)q] = std::max<unsigned char>(rr[(size_t)q], lev);
      auto& ww = flags(wlev, cc.local_block[sd]);
      for (long q : k.side[sd].h_dst) ww[(size_t)q] = (unsigned char)lev;
      total += k.side[sd].n;
    }
    order.emplace_back(lev, (int)n);
    nlev = std::max(nlev, lev);
    sides += 2;
  }
  for (auto& k : c->conns)
    for (int sd = 0; sd < 2; ++sd) {
      std::vector<long>().swap(k.side[sd].h_dst);
      std::vector<long>().swap(k.side[sd].h_src);
    }
  // (250 levels: a chain this long gains nothing over the pairwise launches)
  c->halo_batch = c->halo_batch && sides >= 4 && nlev < 250 && 2 * nlev < sides;
  if (!c->halo_batch && c->halo_batch_required)
    return fail("AGX_HALO_BATCH=require: %d local connections in %d levels", sides / 2, nlev);
  if (!c->halo_batch) return 0;
  std::stable_sort(order.begin(), order.end(),
                   [](const std::pair<int, int>& x, const std::pair<int, int>& y) { return x.first < y.first; });
  c->halo_conn_order.clear();
  c->halo_levels.assign(nlev, agx_ctx::HaloLevel{0, 0, 0});
  long nmax_all = 0;
  for (auto& o : order) {
    auto& L = c->halo_levels[o.first - 1];
    if (L.sides == 0) L.first = 2 * (int)c->halo_conn_order.size();
    L.sides += 2;
    const auto& k = c->conns[o.second];
    L.nmax = std::max(L.nmax, std::max(k.side[0].n, k.side[1].n));
    nmax_all = std::max(nmax_all, L.nmax);
    c->halo_conn_order.push_back(o.second);
  }
  c->halo_batch_sides = sides;
  c->halo_batch_nmax = nmax_all;
  *max_halo = std::max(*max_halo, (total * AGX_NEQ + 1) / 2);     // (the buffer is 2 * max_halo)
  HIPCHK(c->halo_tab_host.alloc((size_t)2 * sides));
  return 0;
}
// The four records of local connection k for a halo selector: g[0], g[1] what sides 0 and 1
// receive, gathered from the partner's block; p[0], p[1] their inserts.  buf0 / buf1: where
// the two halves of the connection's buffer start.
void halo_sides(agx_ctx* c, Conn& k, int what, double* buf0, double* buf1, HaloSide* g,
                HaloSide* p) {
  Block& b0 = c->blocks[k.c.local_block[0]];
  Block& b1 = c->blocks[k.c.local_block[1]];
  const int z = halo_in_d2(b0, what);
  const auto &m0 = k.side[0].map[z], &m1 = k.side[1].map[z];
  g[0] = HaloSide{halo_planes(b1, what), m0.src.get(), k.side[0].n, buf0};
  g[1] = HaloSide{halo_planes(b0, what), m1.src.get(), k.side[1].n, buf1};
  p[0] = HaloSide{halo_planes(b0, what), m0.dst.get(), k.side[0].n, buf0};
  p[1] = HaloSide{halo_planes(b1, what), m1.dst.get(), k.side[1].n, buf1};
}
// the gather / scatter tables of one halo selector (plane pointers of every side)
int halo_batch_tables(agx_ctx* c, int what) {
  const int set = c->halo_set[what];
  if (c->halo_tab_valid[what][set]) return 0;
  const int sides = c->halo_batch_sides;
  auto& tab = c->halo_tab_dev[what][set];
  for (int q = 0; q < 2; ++q)
    if (!tab[q]) HIPCHK(tab[q].alloc((size_t)sides));
  // (the staging entries may still be read by an earlier copy)
  HIPCHK(hipStreamSynchronize(c->stream));
  HaloSide* g = c->halo_tab_host.get();
  HaloSide* p = g + sides;
  double* buf = c->halo_buf.get();
  int n = 0;
  for (int cid : c->halo_conn_order) {            // (level by level)
    auto& k = c->conns[cid];
    const long n0 = k.side[0].n, n1 = k.side[1].n;
    halo_sides(c, k, what, buf, buf + n0 * AGX_NEQ, g + n, p + n);
    buf += (n0 + n1) * AGX_NEQ;
    n += 2;
  }
  HIPCHK(hipMemcpyAsync(tab[0].get(), g, sizeof(HaloSide) * sides, hipMemcpyHostToDevice,
                        c->stream));
  HIPCHK(hipMemcpyAsync(tab[1].get(), p, sizeof(HaloSide) * sides, hipMemcpyHostToDevice,
                        c->stream));
  c->halo_tab_valid[what][set] = true;
  return 0;
}
}  // namespace

namespace {
// index of padded cell (i, j, k) of a block in an index space (0: the SoA planes, 1: D2); no
// block -- the partner lives on another rank -- : 0
struct CellIndex {
  const Block* b;
  int space;
  long operator()(int i, int j, int k) const {
    return !b ? 0L : space ? b->d2idx(i, j, k) : b->d.idx(i, j, k);
  }
};
// The maps of side s of a connection in one index space: the ghost cells of my block and,
// from a partner of this rank, the cells that fill them.  For a partner on another rank, the
// cells of my block its ghost cells read, in its insertion order (what agx_halo_pack sends).
int halo_maps(Conn& k, int s, int space, int ng, CellIndex idx_mine, CellIndex idx_partner,
              bool partner_local, long* max_halo) {
  MapOut m;
  build_side_map(k.c, s, ng, idx_mine, idx_partner, m);
  if (!partner_local) {
    MapOut ms;
    build_side_map(k.c, 1 - s, ng, idx_partner, idx_mine, ms);
    k.n_send = (long)ms.src.size();
    HIPCHK(k.send_src[space].upload(ms.src));
    *max_halo = std::max(*max_halo, (long)ms.src.size() * AGX_NEQ);
  }
  ConnSide& sd = k.side[s];
  sd.n = (long)m.dst.size();
  HIPCHK(sd.map[space].dst.upload(m.dst));
  if (partner_local) HIPCHK(sd.map[space].src.upload(m.src));
  *max_halo = std::max(*max_halo, (long)m.dst.size() * AGX_NEQ);
  if (space == 0) {      // (halo_batch_plan reads, then drops them)
    sd.h_dst = std::move(m.dst);
    if (partner_local) sd.h_src = std::move(m.src);
  }
  return 0;
}
}  // namespace

int agx_setup_finalize(agx_ctx* c) {
  HIPCHK(hipSetDevice(c->device));
  const int ng = c->cfg.n_ghost;
  if (!c->blocks.empty() && c->blocks[0].node_built && geo_complete(c)) return 1;
  long max_parts = 1, max_halo = 1;
  long march_parts = 0;
  for (auto& blk : c->blocks) {
    const dim3 g = cell_grid(blk.d, CELL_BLOCK);
    max_parts = std::max(max_parts, (long)g.x * g.y * g.z);
    march_parts += march_plan(c, blk.d).nparts;
    if (blk.d.d2.base) {  // k_matrix_resid_d2: one partial per 256 plane positions
      max_parts = std::max(max_parts, mresid_wgs(c, blk.d));
#if AGX_FAST
      // k_lusgs_prepare: one per tile of the padded box
      max_parts = std::max(max_parts, (long)((blk.d.d2.Pi + TT - 1) / TT) *
                                          ((blk.d.d2.Pj + TT - 1) / TT) * (blk.d.nk + 2 * blk.d.ng));
      // k_visc_tile's RHS form: one per wave of its persistent workgroups
      max_parts = std::max(max_parts, (long)c->num_cu * VT_R);
#endif
    }
  }
  max_parts = std::max(max_parts, march_parts);
  for (auto& k : c->conns) {
    const agx_connection& cc = k.c;
    const bool l0 = cc.rank[0] == c->rank, l1 = cc.rank[1] == c->rank;
    if (!l0 && !l1) continue;
    for (int s = 0; s < 2; ++s) {
      const bool mine = s == 0 ? l0 : l1, partner_mine = s == 0 ? l1 : l0;
      if (!mine) continue;
      const int lb = cc.local_block[s];
      if (lb < 0 || lb >= (int)c->blocks.size()) return fail("connection refers to unknown block");
      const Block* partner = partner_mine ? &c->blocks[cc.local_block[1 - s]] : nullptr;
      // in the planes' index space and, where x of the LU-SGS path lives there, in D2's
      for (int space = 0; space < (use_d2(c) ? 2 : 1); ++space)
        if (halo_maps(k, s, space, ng, CellIndex{&c->blocks[lb], space},
                      CellIndex{partner, space}, partner_mine, &max_halo))
          return 1;
    }
  }
  if (halo_batch_plan(c, &max_halo)) return 1;
  if (ensure_halo_buf(c, 2 * max_halo)) return 1;
  // persistent slab pairs of the connections to other ranks (sorted by connection
  // id on every rank: the order RCCL's p2p matching relies on)
  std::vector<std::pair<int, int>> per_peer;   // (peer, connections seen so far)
  for (size_t n = 0; n < c->conns.size(); ++n) {
    if (my_side(c, c->conns[n]) < 0) continue;
    agx_ctx::Remote r;
    r.cid = (int)n;
    r.count = (long)agx_halo_count(c, (int)n, AGX_HALO_STATE);
    const bool hb = c->have_ex && c->ex.host_buffers;
    const size_t cap = (size_t)std::max<long>(r.count, 1);
    HIPCHK(r.send.alloc(cap));
    HIPCHK(r.recv.alloc(cap));
    if (hb) {
      HIPCHK(r.hsend.alloc(cap));
      HIPCHK(r.hrecv.alloc(cap));
    }
    const int s = my_side(c, c->conns[n]);
    agx_slab sl;
    sl.peer = c->conns[n].c.rank[1 - s];
    // tag: ordinal among the connections with this peer (hosts create connections
    // in the global order on every rank, so both sides count alike)
    sl.tag = 0;
    bool seen = false;
    for (auto& pp : per_peer)
      if (pp.first == sl.peer) { sl.tag = pp.second++; seen = true; }
    if (!seen) per_peer.emplace_back(sl.peer, 1);
    sl.count = r.count;
    sl.send = hb ? r.hsend.get() : r.send.get();
    sl.recv = hb ? r.hrecv.get() : r.recv.get();
    c->slabs.push_back(sl);
    c->remote.push_back(std::move(r));
  }
  if (c->have_ex) {
    const size_t nrec = 1 + (size_t)c->ex.nranks;
    HIPCHK(c->rec_dev.alloc(nrec));
    HIPCHK(c->rec_host.alloc(nrec));
  }
  c->n_partials = max_parts;
  HIPCHK(c->partials.alloc((size_t)max_parts));
  // (the regions of both: agx_ctx::norm_update() ... host_end())
  HIPCHK(c->norm_out.alloc((size_t)(c->norm_end() - c->norm_update())));
  HIPCHK(c->norm_host.alloc((size_t)(c->host_end() - c->host_update())));
  c->finalized = true;
  return 0;
}

int agx_state_upload(agx_ctx* c, int id, const double* state) {
  field_written_by_caller(c);
  if (flush_consn(c)) return 1;
  if (id < 0 || id >= (int)c->blocks.size()) return fail("bad block id %d", id);
  Block& b = c->blocks[id];
  const BlockDev& d = b.d;
  if (upload_aos(c, b, state, d.state, AGX_NEQ, d.ni + 2 * d.ng,
                 d.nj + 2 * d.ng, d.nk + 2 * d.ng, d.ng))
    return 1;
#if AGX_NEQ == 7
  // gridLevel::AuxillaryAndWidths main.cpp:169: viscosity_ before the first iteration
  // (the rans wall ghost states read the viscosity_ of the LAST UpdateAuxillaryVariables)
  hipLaunchKernelGGL(k_aux_field, dim3((d.nplane + 255) / 256), dim3(256), 0, c->stream, d,
                     c->gas, 1, d.viscp);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

static int field_info(Block& b, int field, double* const** p, int* ncomp, int* ghost) {
  BlockDev& d = b.d;
  static thread_local double* one[1];
  switch (field) {
    case AGX_FIELD_STATE: *p = d.state; *ncomp = AGX_NEQ; *ghost = 1; return 0;
    case AGX_FIELD_RESIDUAL: *p = d.resid; *ncomp = AGX_NEQ; *ghost = 0; return 0;
    case AGX_FIELD_CONS_N: *p = d.consn; *ncomp = AGX_NEQ; *ghost = 0; return 0;
    case AGX_FIELD_CONS_NM1: *p = d.consnm1; *ncomp = AGX_NEQ; *ghost = 0; return 0;
    case AGX_FIELD_UPDATE: *p = d.x; *ncomp = AGX_NEQ; *ghost = 1; return 0;
    case AGX_FIELD_DT: one[0] = d.dt; *p = one; *ncomp = 1; *ghost = 0; return 0;
    case AGX_FIELD_SPEC_RADIUS: one[0] = d.specrad; *p = one; *ncomp = 1; *ghost = 0; return 0;
    case AGX_FIELD_DIAGONAL: one[0] = d.a; *p = one; *ncomp = 1; *ghost = 0; return 0;
  }
  return 1;
}
// the geometry planes (download only): `face` = the direction with one more entry, or -1
static int geom_field_info(Block& b, int field, double* const** p, int* ncomp, int* face) {
  BlockDev& d = b.d;
  static thread_local double* one[1];
  *face = -1;
  switch (field) {
    case AGX_FIELD_VOLUME: one[0] = d.vol; *p = one; *ncomp = 1; return 0;
    case AGX_FIELD_CENTER: *p = d.cen; *ncomp = 3; return 0;
    case AGX_FIELD_FAREA_I: case AGX_FIELD_FAREA_J: case AGX_FIELD_FAREA_K:
      *face = field - AGX_FIELD_FAREA_I; *p = d.fa[*face]; *ncomp = 4; return 0;
    case AGX_FIELD_WIDTH_I: case AGX_FIELD_WIDTH_J: case AGX_FIELD_WIDTH_K:
      one[0] = d.wid[field - AGX_FIELD_WIDTH_I]; *p = one; *ncomp = 1; return 0;
    case AGX_FIELD_WALL_DIST: one[0] = d.wdist; *p = one; *ncomp = 1; return 0;
  }
  return 1;
}

// x of the D2 LU-SGS path <-> the SoA planes the field transfers use
static int d2_x_copy(agx_ctx* c, Block& b, int to_d2) {
#if AGX_FAST
  x_planes_copied(b);
  const long n = (long)b.d.d2.Pi * b.d.d2.Pj * (b.d.nk + 2 * b.d.ng);
  hipLaunchKernelGGL(k_d2_x_copy, dim3((n + 255) / 256), dim3(256), 0, c->stream, b.d, to_d2,
                     to_d2 ? (unsigned)(++b.kp_epoch) & 3u : 0u);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

// The gradients an output step asks for reach into the ghost cells: they are formed with
// the ghost cells the NEXT residual would see -- the inviscid fill of the state as it is now
// (already queued behind the last update unless something touched the state since), then
// the viscous-wall fill (gridLevel.cpp:287-319, procBlock.cpp:6131-6136).  Ghost cells of
// connections to other ranks stay as last exchanged (an output step is not a collective).
// The viscous-wall fill stays in the ghost cells, so between the caller's agx_phase_bc_faces
// and the agx_phase_residual that follows it -- whose inviscid fluxes would read it -- the
// call is refused (include/aither_gfx950.h "reads between phases").
// (in its two halves for the boundary fluxes, which read the ghost cells of both fills: the
// inviscid flux of a residual sees a viscousWall as a slip wall)
static int ghosts_for_output_inviscid(agx_ctx* c, const char* who) {
  if (c->ghost_fill_open)
    return fail("%s: gradients, node and wall variables refill the ghost cells, which are "
                "being filled for the coming residual (agx_phase_bc_faces was called, "
                "agx_phase_residual not yet); legal from agx_phase_residual to the next "
                "agx_phase_bc_faces and between agx_iterate calls", who);
  if (!c->ghosts_prefilled) {
    if (bc_faces(c)) return 1;
    if (agx_halo_swap_local(c, AGX_HALO_STATE)) return 1;
    if (bc_edges(c)) return 1;
  }
  return 0;
}
static int ghosts_for_output_viscous(agx_ctx* c) {
  if (c->cfg.is_viscous) {
    if (bc_pass(c, true, 2)) return 1;     // (2: the stored wall-law data stay the last residual's)
    if (bc_pass(c, false, 1)) return 1;
  }
  ghost_fill_gone(c);   // (the next iteration starts from its own inviscid fill)
  return 0;
}
static int ghosts_for_output(agx_ctx* c, const char* who) {
  return ghosts_for_output_inviscid(c, who) || ghosts_for_output_viscous(c);
}

// ---- output: WriteFunFile / WriteRestart payloads packed on the device ------
namespace {
OutSpec out_spec(const agx_ctx* c, const Block& b, int nvar = 0, const int32_t* vars = nullptr) {
  OutSpec sp;
  memset(&sp, 0, sizeof sp);
  sp.nvar = nvar;
  for (int v = 0; v < nvar; ++v) sp.var[v] = vars[v];
  const agx_gas& a = c->cfg.gas;
  sp.rho_ref = a.rho_ref; sp.a_ref = a.a_ref; sp.l_ref = a.l_ref; sp.t_ref = a.t_ref;
  sp.mu_ref = c->gas.mu_ref;                  // transport::MuRef, transport.cpp:58-66
  sp.rank = c->rank;
  sp.global_pos = b.global_pos;
  return sp;
}
// ---- what the output and sampling paths share, each stated once; a caller keeps its message
// the flags of wall_face_vars: bit 0 the fourth-order viscous reconstruction, bit 1 a
// largeEddySimulation run (the iteration path passes bit 0 alone)
int wall_eval_flags(const agx_ctx* c) {
  return (c->cfg.viscous_recon == AGX_VISC_RECON_CENTRAL_4TH ? 1 : 0) | (c->sp.les ? 2 : 0);
}
// wall-law surfaces take their wall data from a residual; field: the caller's, if it names one
int wall_data_missing(const agx_ctx* c, const Block& b, const char* call, const char* field = "") {
  if (!b.d.wallv || c->have_wall_data) return 0;
  return fail("%s: %s%sthe wall-law surfaces hold no wall data before the first residual", call,
              field, *field ? ": " : "");
}
// plan: the field that uploads the plan of the series or of the spectra
int no_plan(const char* call, const char* field, int id, const char* plan) {
  return fail("%s: %s: block %d has no plan (upload %s first)", call, field, id, plan);
}
int no_statistics(const char* who, int id) {
  return fail("%s: block %d has no statistics: no sample has been taken (AGX_FIELD_STAT_SAMPLE)",
              who, id);
}
// what a 5-equation library keeps, a predicate per kind of id (it has no tke, sdr, f1, f2):
// cell ids AGX_OUT_*, wall ids AGX_WALL_*, n of AGX_STAT_BASE + n, and q of AGX_FLUX_BASE + q
// or AGX_BUDGET_BASE + q (1 + e and 8 + e carry equation e)
bool kept_cell_id(int var) {
  return AGX_NEQ != 5 || !(var == AGX_OUT_TKE || var == AGX_OUT_SDR || var == AGX_OUT_F1 ||
                           var == AGX_OUT_F2 || (var >= AGX_OUT_TKEGRAD && var < AGX_OUT_RESID) ||
                           var >= AGX_OUT_RESID + 5);
}
bool kept_wall_id(int var) {
  return AGX_NEQ != 5 || !(var == AGX_WALL_TKE || var == AGX_WALL_SDR);
}
bool kept_stat_index(int n) { return AGX_NEQ != 5 || !(n == 10 || n == 11); }
bool kept_flux_equation(int q) { return AGX_NEQ != 5 || !(q > 0 && (q - 1) % FLUX_NE >= AGX_NEQ); }
// entry `at` of a field payload as an integer in [lo, hi]; refuses by name, saying which entry
int payload_entry(const char* field, const double* in, long at, const char* what, double lo,
                  double hi, long* out) {
  const double x = in[at];
  if (!std::isfinite(x) || x != std::floor(x) || x < lo || x > hi)
    return fail("agx_field_upload: %s: entry %ld (%s) is %g: an integer from %.0f to %.0f is "
                "expected", field, at, what, x, lo, hi);
  *out = (long)x;
  return 0;
}
// WriteWallFun's payload of one block (the ids are wall ids, nvar is in their range)
int wall_pack(agx_ctx* c, int id, int nvar, const int32_t* vars, double* out) {
  Block& b = c->blocks[id];
  if (!c->cfg.is_viscous)
    return fail("agx_output_pack: wall variables need a viscous context (an inviscid run keeps "
                "no wallData_)");
  if (b.wall_tab.empty())
    return fail("agx_output_pack: block %d has no viscousWall surface", id);
  if (!c->finalized) return fail("agx_setup_finalize has not been called");
  if (wall_data_missing(c, b, "agx_output_pack")) return 1;
  const long total = b.wall_faces;
  double* tmp = nullptr;
  if (stage_buffer(c, (size_t)nvar * total, &tmp)) return 1;
  if (ghosts_for_output(c, "agx_output_pack")) return 1;
  hipLaunchKernelGGL(k_wall_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream,
                     b.d, c->gas, out_spec(c, b, nvar, vars), b.wall_tab_dev.get(),
                     (int)b.wall_tab.size(), total, wall_eval_flags(c), tmp);
  return copy_out(c, out, tmp, (size_t)nvar * total);
}
// The integrated wall loads of one block's load surfaces (the ids are load ids, nvar is in
// their range): k_wall_loads' chunk records, then k_wall_loads_sum
int wall_loads(agx_ctx* c, int id, int nvar, const int32_t* vars, double* out) {
  Block& b = c->blocks[id];
  if (b.load_tab.empty())
    return fail("agx_output_pack: block %d has no viscousWall or slipWall surface", id);
  if (!c->finalized) return fail("agx_setup_finalize has not been called");
  const bool viscous = c->cfg.is_viscous != 0;
  if (viscous && wall_data_missing(c, b, "agx_output_pack")) return 1;
  if (!b.load_fcen)
    for (int v = 0; v < nvar; ++v)
      if (vars[v] >= AGX_LOAD_PRESSURE_MOMENT_X) {
        if (!b.node_built)
          return fail("agx_output_pack: load variable %d is a moment, and block %d was built "
                      "from arrays: agx_block_geom carries no face centres (a block built from "
                      "agx_block_geom.nodes keeps those of its wall faces)", vars[v], id);
        return fail("agx_output_pack: load variable %d is a moment, and the face centres of "
                    "block %d went with an agx_block_set_bcs after agx_setup_finalize",
                    vars[v], id);
      }
  const int nsurf = (int)b.load_tab.size();
  double* tmp = nullptr;
  if (stage_buffer(c, (size_t)nvar * nsurf, &tmp)) return 1;
  // a viscous context evaluates its viscousWall faces with the ghost cells the next residual
  // would see; an inviscid one reads physical cells only
  if (viscous && ghosts_for_output(c, "agx_output_pack")) return 1;
  hipLaunchKernelGGL(k_wall_loads, dim3((unsigned)b.load_chunks), dim3(LOAD_CHUNK), 0, c->stream,
                     b.d, c->gas, b.load_tab_dev.get(), nsurf, b.load_faces, viscous ? 1 : 0,
                     wall_eval_flags(c), b.load_fcen.get(), b.load_partial.get());
  hipLaunchKernelGGL(k_wall_loads_sum, dim3((unsigned)((nvar * nsurf + 63) / 64)), dim3(64), 0,
                     c->stream, out_spec(c, b, nvar, vars), b.load_tab_dev.get(), nsurf,
                     b.load_chunks, 1.0 / c->gas.scaling, b.load_partial.get(), tmp);
  return copy_out(c, out, tmp, (size_t)nvar * nsurf);
}
// Does surface s of block id belong to a connection whose partner is on another rank?  (The
// ranges of a connection are cell ranges along d1 = d3 + 1 and d2 = d3 + 2, dirs_of.)
bool surface_is_remote(const agx_ctx* c, int id, const agx_bc_surface& s) {
  if (s.bc_type != AGX_BC_INTERBLOCK && s.bc_type != AGX_BC_PERIODIC) return false;
  const int st = surface_type(s);
  int d1, d2, d3;
  dirs_of(st, d1, d2, d3);
  const int lo[3] = {s.imin, s.jmin, s.kmin}, hi[3] = {s.imax, s.jmax, s.kmax};
  for (const auto& k : c->conns) {
    const int m = my_side(c, k);
    if (m < 0 || k.c.local_block[m] != id || k.c.boundary[m] != st) continue;
    if (k.c.d1_start[m] < hi[d1] && k.c.d1_end[m] > lo[d1] && k.c.d2_start[m] < hi[d2] &&
        k.c.d2_end[m] > lo[d2])
      return true;
  }
  return false;
}
// the table of the flux surfaces of a block (agx_flux.hpp), from its surfaces and the
// connections as they are now
int flux_table(agx_ctx* c, int id) {
  Block& b = c->blocks[id];
  if (b.flux_tab_built) return 0;
  b.flux_tab.clear();
  b.flux_chunks = 0;
  const int nn[3] = {b.d.ni, b.d.nj, b.d.nk};
  for (size_t q = 0; q < b.surf_host.size(); ++q) {
    const agx_bc_surface& s = b.surf_host[q];
    if (surface_is_remote(c, id, s)) continue;
    FluxSurfDev w;
    const int lo[3] = {s.imin, s.jmin, s.kmin}, hi[3] = {s.imax, s.jmax, s.kmax};
    w.side = surface_type(s);
    const int d3 = (w.side - 1) / 2;
    for (int d = 0; d < 3; ++d) {
      w.lo[d] = lo[d];
      w.n[d] = d == d3 ? 1 : hi[d] - lo[d];
      // (the kernel indexes the planes from these: they must lie on the block)
      if (lo[d] < 0 || hi[d] > nn[d] || w.n[d] < 1 ||
          (d == d3 && (lo[d] != (w.side % 2 == 1 ? 0 : nn[d]) || hi[d] != lo[d])))
        return fail("agx_output_pack: surface %d does not lie on a side of block %d", (int)q, id);
    }
    w.chunk0 = b.flux_chunks;
    b.flux_chunks += ((long)w.n[0] * w.n[1] * w.n[2] + FLUX_CHUNK - 1) / FLUX_CHUNK;
    b.flux_tab.push_back(w);
  }
  HIPCHK(hipStreamSynchronize(c->stream));     // (before the old table and records are freed)
  HIPCHK(b.flux_tab_dev.upload(b.flux_tab));
  b.flux_partial.reset();
  if (b.flux_chunks > 0) HIPCHK(b.flux_partial.alloc((size_t)b.flux_chunks * FLUX_NQ));
  b.flux_tab_built = true;
  return 0;
}
// equations 5 and 6 (rho k, rho omega) of the flux and budget ranges in a 5-equation library
int flux_eq_refused(const char* range, int q, int var) {
  return !kept_flux_equation(q)
             ? fail("agx_output_pack: %s variable %d (tke, sdr) is not kept by the 5-equation "
                    "libraries", range, var)
             : 0;
}
// The fluxes through the flux surfaces of one block (the ids are flux ids, nvar is in their
// range): k_surface_flux's chunk records, then k_surface_flux_sum
int surface_fluxes(agx_ctx* c, int id, int nvar, const int32_t* vars, double* out) {
  Block& b = c->blocks[id];
  if (!c->finalized) return fail("agx_setup_finalize has not been called");
  for (int v = 0; v < nvar; ++v)
    if (flux_eq_refused("flux", vars[v] - AGX_FLUX_BASE, vars[v])) return 1;
  if (flux_table(c, id)) return 1;
  if (b.flux_tab.empty())
    return fail("agx_output_pack: block %d has no flux surface (every surface it has is a "
                "connection to another rank)", id);
  const bool viscous = c->cfg.is_viscous != 0;
  if (viscous && wall_data_missing(c, b, "agx_output_pack")) return 1;
  const int halo = recon_reach(c);
  if (halo > b.d.ng)
    return fail("agx_output_pack: flux variables: the reconstruction reaches %d cells across a "
                "face, the blocks have %d ghost layers", halo, b.d.ng);
  const int nsurf = (int)b.flux_tab.size();
  double* tmp = nullptr;
  if (stage_buffer(c, (size_t)nvar * nsurf, &tmp)) return 1;
  // viscous or not, a boundary face's flux reads the ghost cells, those the next residual
  // would see: its inviscid fill for the inviscid flux (a viscousWall is a slip wall there),
  // then its viscous-wall fill for the viscous one
  if (ghosts_for_output_inviscid(c, "agx_output_pack")) return 1;
  const dim3 grid((unsigned)b.flux_chunks), tb(FLUX_CHUNK);
  // (reconstruction, limiter, flux) as launch_inv instantiates the gather-form residual
  by_int<AGX_RECON_CONSTANT, AGX_RECON_MUSCL, AGX_RECON_WENO, AGX_RECON_WENOZ>(
      c->cfg.recon, [&](auto recon) {
        constexpr int RECON = decltype(recon)::value;
        auto launch = [&](auto lim) {
          by_int<AGX_FLUX_ROE, AGX_FLUX_AUSM>(c->cfg.inviscid_flux, [&](auto flux) {
            hipLaunchKernelGGL(
                (k_surface_flux<RECON, decltype(lim)::value, decltype(flux)::value>), grid, tb,
                0, c->stream, b.d, c->gas, c->sp.kappa, b.flux_tab_dev.get(), nsurf,
                b.flux_partial.get());
          });
        };
        if constexpr (RECON == AGX_RECON_MUSCL)
          by_int<AGX_LIMITER_VANALBADA, AGX_LIMITER_MINMOD, AGX_LIMITER_NONE>(c->cfg.limiter,
                                                                               launch);
        else
          launch(std::integral_constant<int, AGX_LIMITER_NONE>{});
      });
  if (ghosts_for_output_viscous(c)) return 1;
  if (viscous)
    hipLaunchKernelGGL(k_surface_flux_visc, grid, tb, 0, c->stream, b.d, c->gas,
                       b.flux_tab_dev.get(), nsurf, wall_eval_flags(c), b.flux_partial.get());
  hipLaunchKernelGGL(k_surface_flux_sum, dim3((unsigned)((nvar * nsurf + 63) / 64)), dim3(64), 0,
                     c->stream, out_spec(c, b, nvar, vars), b.flux_tab_dev.get(), nsurf,
                     b.flux_chunks, viscous ? 1 : 0, b.flux_partial.get(), tmp);
  return copy_out(c, out, tmp, (size_t)nvar * nsurf);
}
// The balance of one block (the ids are budget ids, nvar is in their range): physical cells
// only, legal at every position
int block_budget(agx_ctx* c, int id, int nvar, const int32_t* vars, double* out) {
  Block& b = c->blocks[id];
  for (int v = 0; v < nvar; ++v) {
    if (flux_eq_refused("budget", vars[v] - AGX_BUDGET_BASE, vars[v])) return 1;
    if (vars[v] >= AGX_BUDGET_RESIDUAL && !c->have_residual)
      return fail("agx_output_pack: budget variable %d is a sum of the residual, and no residual "
                  "has been formed yet (agx_phase_residual, agx_iterate)", vars[v]);
  }
  const long rows = (long)b.d.nj * b.d.nk;
  const long nchunk = (rows + BUDGET_CHUNK - 1) / BUDGET_CHUNK;
  if (!b.budget_partial) HIPCHK(b.budget_partial.alloc((size_t)nchunk * FLUX_NQ));
  double* tmp = nullptr;
  if (stage_buffer(c, (size_t)nvar, &tmp)) return 1;
  hipLaunchKernelGGL(k_block_budget, dim3((unsigned)((nchunk * 64 + 255) / 256)), dim3(256), 0,
                     c->stream, b.d, c->gas, nchunk, c->have_residual ? 1 : 0,
                     b.budget_partial.get());
  hipLaunchKernelGGL(k_block_budget_sum, dim3(1), dim3(64), 0, c->stream,
                     out_spec(c, b, nvar, vars), nchunk, b.budget_partial.get(), tmp);
  return copy_out(c, out, tmp, (size_t)nvar);
}
// WriteFunFile's payload of one block, or (node) WriteNodeFun's: one value per physical cell
// or per node; vars: cell ids
int point_pack(agx_ctx* c, int id, bool node, int nvar, const int32_t* vars, double* out) {
  Block& b = c->blocks[id];
  if (node && !c->finalized) return fail("agx_setup_finalize has not been called");
  bool need_grads = false;
  for (int v = 0; v < nvar; ++v) {
    const int var = vars[v];
    if (var == AGX_OUT_VISCOSITY && !c->sp.viscous)
      return fail("viscosity_ is only kept for viscous runs (procBlock.cpp:6171)");
    if ((AGX_NEQ == 7 || c->sp.les) && node &&
        (var == AGX_OUT_VISCOSITY_RATIO || var == AGX_OUT_TURB_VISCOSITY ||
         var == AGX_OUT_F1 || var == AGX_OUT_F2))
      return fail("agx_output_pack: node variable %d (viscosityRatio, turbulentViscosity, f1, f2) "
                  "is not formed at nodes: the reference averages eddyViscosity_, f1_, f2_ with "
                  "their ghost cells, which hold what the residual's accumulation at boundary "
                  "faces and the corner initial values left; the library keeps them in physical "
                  "cells and connection ghost cells only", AGX_NODE_BASE + var);
    need_grads = need_grads || (var >= AGX_OUT_VELGRAD && var < AGX_OUT_RESID);
  }
  const int n1 = node ? 1 : 0;      // one node more than cells along each direction
  const long npoint = (long)(b.d.ni + n1) * (b.d.nj + n1) * (b.d.nk + n1);
  double* tmp = nullptr;
  const size_t gdoubles = need_grads ? (size_t)3 * NGF * npoint : 0;
  if (stage_buffer(c, gdoubles + (size_t)nvar * npoint, &tmp)) return 1;
  // every nodal variable reads ghost cells, of the cell variables the gradients do: those the
  // next residual would see
  if ((node || need_grads) && ghosts_for_output(c, "agx_output_pack")) return 1;
  const dim3 grid((b.d.ni + n1 + CELL_BLOCK.x - 1) / CELL_BLOCK.x,
                  (b.d.nj + n1 + CELL_BLOCK.y - 1) / CELL_BLOCK.y, b.d.nk + n1);
  if (need_grads)
    hipLaunchKernelGGL(node ? k_node_grads : k_cell_grads, grid, CELL_BLOCK, 0, c->stream, b.d,
                       c->gas, tmp);
  double* packed = tmp + gdoubles;
  hipLaunchKernelGGL(node ? k_node_pack : k_output_pack, grid, CELL_BLOCK, 0, c->stream, b.d,
                     c->gas, out_spec(c, b, nvar, vars), need_grads ? tmp : nullptr, packed);
  return copy_out(c, out, packed, (size_t)nvar * npoint);
}
}  // namespace

// ---- time statistics (agx_stats.hpp; include/aither_gfx950.h at AGX_STAT_BASE) ---------------
namespace {
// extras of the sampled cell vector: the eddy viscosity (largeEddySimulation, 7 equations),
// k and omega (7 equations); the cell planes and the wall values per face of a block
int stat_nx(const agx_ctx* c) { return AGX_NEQ == 7 ? 3 : (c->sp.les ? 1 : 0); }
int stat_planes(const agx_ctx* c) { return 9 + stat_nx(c) + STAT_NSECOND; }
int stat_wall_values(const agx_ctx* c, const Block& b) {
  return c->cfg.is_viscous && !b.wall_tab.empty() ? STAT_NWALL : 0;
}
long stat_ncell(const Block& b) { return (long)b.d.ni * b.d.nj * b.d.nk; }
long stat_pitch(const Block& b) { return (stat_ncell(b) + 1) & ~1L; }
void stats_reset(Block& b) {
  b.stat_cells.reset();
  b.stat_wall.reset();
  b.stat_part.reset();
  b.stat_W = b.stat_n = 0.0;
}
// zeroed accumulators (the first sample, or an upload into a block without)
int stats_alloc(agx_ctx* c, Block& b) {
  const size_t nc = (size_t)stat_planes(c) * stat_pitch(b);
  const size_t nw = (size_t)stat_wall_values(c, b) * b.wall_faces;
  HIPCHK(b.stat_cells.alloc(nc));
  HIPCHK(hipMemsetAsync(b.stat_cells.get(), 0, sizeof(double) * nc, c->stream));
  if (nw) {
    // (both or neither: a block is never left with the cell planes alone)
    if (b.stat_wall.alloc(nw) != hipSuccess) {
      stats_reset(b);
      return fail("time statistics: no device memory for the wall rows of %zu doubles", nw);
    }
    HIPCHK(hipMemsetAsync(b.stat_wall.get(), 0, sizeof(double) * nw, c->stream));
  }
  return 0;
}
// the accumulators a block holds are the size its surfaces ask for now (an agx_block_set_bcs
// after the first sample may have changed its wall faces)
bool stats_fit(const agx_ctx* c, const Block& b) {
  return b.stat_cells.size() == (size_t)stat_planes(c) * stat_pitch(b) &&
         b.stat_wall.size() == (size_t)stat_wall_values(c, b) * b.wall_faces;
}
int stats_misfit(const char* who, int id) {
  return fail("%s: the wall surfaces of block %d changed since its statistics began; discard "
              "them first (AGX_FIELD_STAT_SAMPLE with w == 0)", who, id);
}
// the cell statistics a library or a context does not keep (n relative to AGX_STAT_BASE; var:
// the id as the caller gave it)
int stat_not_kept(bool refused, int var) {
  return refused ? fail("agx_output_pack: statistics variable %d (mean tke, mean sdr) is not "
                        "kept by the 5-equation libraries", var) : 0;
}
int stat_cell_refused(const agx_ctx* c, int n, int var) {
  if (stat_not_kept(!kept_stat_index(n), var)) return 1;
  if (n == 9 && stat_nx(c) == 0)
    return fail("agx_output_pack: statistics variable %d (mean turbulentViscosity): this "
                "context has no eddy viscosity (largeEddySimulation and the rans libraries "
                "have)", var);
  return 0;
}
int stats_sample(agx_ctx* c, int id, double w) {
  Block& b = c->blocks[id];
  if (!std::isfinite(w) || w < 0.0)
    return fail("agx_field_upload: AGX_FIELD_STAT_SAMPLE: the weight %g is negative or not "
                "finite (w > 0 samples, w == 0 discards the block's statistics)", w);
  if (w == 0.0) { stats_reset(b); return 0; }
  if (!c->finalized) return fail("agx_setup_finalize has not been called");
  const bool wall = stat_wall_values(c, b) > 0;
  if (wall) {
    if (wall_data_missing(c, b, "agx_field_upload", "AGX_FIELD_STAT_SAMPLE")) return 1;
    // the wall faces are evaluated with the ghost cells the next residual would see
    if (ghosts_for_output(c, "agx_field_upload")) return 1;
  }
  if (b.stat_cells && !stats_fit(c, b)) return stats_misfit("agx_field_upload", id);
  if (!b.stat_cells && stats_alloc(c, b)) return 1;
  const double W = b.stat_W + w, r = w / W, cf = w * (1.0 - r);
  const long ncell = stat_ncell(b), pitch = stat_pitch(b);
  const dim3 grid((unsigned)((pitch / 2 + 255) / 256));
  by_int<0, 1, 3>(stat_nx(c), [&](auto nx) {
    // (a library holds the forms its contexts can ask for)
    if constexpr ((AGX_NEQ == 7) == (decltype(nx)::value == 3))
      hipLaunchKernelGGL(k_stats_cells<decltype(nx)::value>, grid, dim3(256), 0, c->stream, b.d,
                         c->gas, ncell, pitch, r, cf, b.stat_cells.get());
    return 0;
  });
  if (wall)
    hipLaunchKernelGGL(k_stats_wall, dim3((unsigned)((b.wall_faces + 255) / 256)), dim3(256), 0,
                       c->stream, b.d, c->gas, b.wall_tab_dev.get(), (int)b.wall_tab.size(),
                       b.wall_faces, wall_eval_flags(c), r, cf, b.stat_wall.get());
  HIPCHK(hipGetLastError());
  b.stat_W = W;
  b.stat_n += 1.0;
  return 0;
}
}  // namespace

// (agx_field_upload has flushed and has checked the block id and the pointer, for the series
// and the spectra below as well)
static int stats_field_upload(agx_ctx* c, int id, int field, const double* in) {
  if (!c->have_cfg) return fail("agx_config_set has not been called");
  if (field == AGX_FIELD_STAT_SAMPLE) return stats_sample(c, id, in[0]);
  if (!c->finalized) return fail("agx_setup_finalize has not been called");
  Block& b = c->blocks[id];
  const int np = stat_planes(c), nwv = stat_wall_values(c, b);
  if (in[0] != (double)np || in[1] != (double)nwv)
    return fail("agx_field_upload: AGX_FIELD_STAT_ACCUM: the payload holds %g cell planes and %g "
                "wall values per face, this library and context keep %d and %d for block %d",
                in[0], in[1], np, nwv, id);
  if (!std::isfinite(in[2]) || in[2] < 0.0 || !std::isfinite(in[3]) || in[3] < 0.0)
    return fail("agx_field_upload: AGX_FIELD_STAT_ACCUM: the sum of weights %g or the sample "
                "count %g is negative or not finite", in[2], in[3]);
  // (an upload replaces the statistics: accumulators of another size go)
  if (b.stat_cells && !stats_fit(c, b)) stats_reset(b);
  if (!b.stat_cells && stats_alloc(c, b)) return 1;
  const long ncell = stat_ncell(b), pitch = stat_pitch(b);
  const double* planes_in = in + 4;
  HIPCHK(hipMemcpy2DAsync(b.stat_cells.get(), sizeof(double) * pitch, planes_in,
                          sizeof(double) * ncell, sizeof(double) * ncell, np,
                          hipMemcpyHostToDevice, c->stream));
  if (nwv)
    HIPCHK(hipMemcpyAsync(b.stat_wall.get(), planes_in + (size_t)np * ncell,
                          sizeof(double) * nwv * b.wall_faces, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  b.stat_W = in[2];
  b.stat_n = in[3];
  return 0;
}

static int stats_field_download(agx_ctx* c, int id, int field, double* out) {
  if (field == AGX_FIELD_STAT_SAMPLE)
    return fail("agx_field_download: AGX_FIELD_STAT_SAMPLE is upload only (a sample's weight); "
                "AGX_FIELD_STAT_ACCUM holds the accumulators");
  Block& b = c->blocks[id];
  if (!b.stat_cells) return no_statistics("agx_field_download: AGX_FIELD_STAT_ACCUM", id);
  if (!stats_fit(c, b)) return stats_misfit("agx_field_download", id);
  const int np = stat_planes(c), nwv = stat_wall_values(c, b);
  const long ncell = stat_ncell(b), pitch = stat_pitch(b);
  out[0] = np; out[1] = nwv; out[2] = b.stat_W; out[3] = b.stat_n;
  HIPCHK(hipMemcpy2DAsync(out + 4, sizeof(double) * ncell, b.stat_cells.get(),
                          sizeof(double) * pitch, sizeof(double) * ncell, np,
                          hipMemcpyDeviceToHost, c->stream));
  if (nwv)
    HIPCHK(hipMemcpyAsync(out + 4 + (size_t)np * ncell, b.stat_wall.get(),
                          sizeof(double) * nwv * b.wall_faces, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// the statistics of one block's cells or (wall) wall faces; the ids are of that range
static int stats_pack(agx_ctx* c, int id, bool wall, int nvar, const int32_t* vars, double* out) {
  Block& b = c->blocks[id];
  if (wall) {
    if (!c->cfg.is_viscous)
      return fail("agx_output_pack: wall statistics need a viscous context (an inviscid run "
                  "keeps no wallData_)");
    if (b.wall_tab.empty())
      return fail("agx_output_pack: block %d has no viscousWall surface", id);
  }
  int32_t ids[AGX_OUT_COUNT];
  for (int v = 0; v < nvar; ++v) {
    ids[v] = vars[v] - (wall ? AGX_WSTAT_BASE : AGX_STAT_BASE);
    if (wall ? stat_not_kept(!kept_wall_id(AGX_WALL_YPLUS + ids[v]), vars[v])
             : stat_cell_refused(c, ids[v], vars[v]))
      return 1;
  }
  if (!b.stat_cells) return no_statistics("agx_output_pack", id);
  if (!stats_fit(c, b)) return stats_misfit("agx_output_pack", id);
  const long n = wall ? b.wall_faces : stat_ncell(b);
  double* tmp = nullptr;
  if (stage_buffer(c, (size_t)nvar * n, &tmp)) return 1;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (wall)
    hipLaunchKernelGGL(k_stats_wall_pack, grid, dim3(256), 0, c->stream, n, b.stat_W, c->gas,
                       out_spec(c, b, nvar, ids), b.stat_wall.get(), tmp);
  else
    hipLaunchKernelGGL(k_stats_pack, grid, dim3(256), 0, c->stream, n, stat_pitch(b),
                       9 + stat_nx(c), b.stat_W, out_spec(c, b, nvar, ids), b.stat_cells.get(),
                       tmp);
  return copy_out(c, out, tmp, (size_t)nvar * n);
}

// the cell statistics of one block pooled over the collapsed index directions of a mask; the
// ids are of AGX_CSTAT_BASE, of no other range, and at most AGX_CSTAT_COUNT
static int stats_collapse(agx_ctx* c, int id, int nvar, const int32_t* vars, double* out) {
  Block& b = c->blocks[id];
  const int nm = 9 + stat_nx(c);
  CstatSpec cs;
  memset(&cs, 0, sizeof cs);
  int32_t ids[AGX_OUT_COUNT];
  for (int v = 0; v < nvar; ++v) {
    const int mask = (vars[v] - AGX_CSTAT_BASE) / 32, n = (vars[v] - AGX_CSTAT_BASE) % 32;
    if (mask < 1 || mask > 7)
      return fail("agx_output_pack: collapsed statistics variable %d: mask %d (the collapsed "
                  "directions are bit 0 = i, bit 1 = j, bit 2 = k: 1 ... 7)", vars[v], mask);
    if (n >= AGX_CSTAT_COUNT)
      return fail("agx_output_pack: collapsed statistics variable %d: n = %d (0 ... 20 are the "
                  "variables of AGX_STAT_BASE, 21 is the volume)", vars[v], n);
    if (v > 0 && mask != cs.mask)
      return fail("agx_output_pack: collapsed statistics of masks %d and %d in one call (a call "
                  "collapses one set of directions)", cs.mask, mask);
    cs.mask = mask;
    ids[v] = n;
    if (stat_cell_refused(c, n, vars[v])) return 1;
    // a mean carries its own plane, a second moment its plane and its two means
    if (n < 12) cs.means |= 1u << n;
    else if (n < CSTAT_VOLUME) {
      cs.seconds |= 1u << (n - 12);
      cs.means |= 1u << stat_second_a(n - 12) | 1u << stat_second_b(n - 12);
    }
  }
  if (!b.stat_cells) return no_statistics("agx_output_pack", id);
  if (!stats_fit(c, b)) return stats_misfit("agx_output_pack", id);
  const long ni = b.d.ni, nj = b.d.nj, nk = b.d.nk;
  cs.pitch = stat_pitch(b);
  cs.nbin = (cs.mask & 1 ? 1 : ni) * (cs.mask & 2 ? 1 : nj) * (cs.mask & 4 ? 1 : nk);
  cs.steps = (cs.mask & 2 ? nj : 1) * (cs.mask & 4 ? nk : 1);
  cs.nchunk = (cs.steps + CSTAT_CHUNK - 1) / CSTAT_CHUNK;
  const size_t np = (size_t)cs.nchunk * cstat_nq(nm) * cs.nbin;
  if (np > b.stat_part.size()) {
    HIPCHK(hipStreamSynchronize(c->stream));     // (before the old one is freed)
    if (b.stat_part.alloc(np) != hipSuccess)
      return fail("agx_output_pack: no device memory for the chunk records of %zu doubles", np);
  }
  double* tmp = nullptr;
  if (stage_buffer(c, (size_t)nvar * cs.nbin, &tmp)) return 1;
  const long units = cs.nbin * cs.nchunk, threads = cs.mask & 1 ? units * 64 : units;
  const dim3 grid((unsigned)((threads + 255) / 256));
  by_int<0, 1, 3>(stat_nx(c), [&](auto nx) {
    if constexpr ((AGX_NEQ == 7) == (decltype(nx)::value == 3))
      hipLaunchKernelGGL(k_cstat_partial<decltype(nx)::value>, grid, dim3(256), 0, c->stream, b.d,
                         cs, b.stat_cells.get(), b.stat_part.get());
    return 0;
  });
  hipLaunchKernelGGL(k_cstat_join, dim3((unsigned)((cs.nbin + 63) / 64), (unsigned)nvar), dim3(64),
                     0, c->stream, cs, nm, b.stat_W, out_spec(c, b, nvar, ids),
                     b.stat_part.get(), tmp);
  return copy_out(c, out, tmp, (size_t)nvar * cs.nbin);
}

// ---- time series (agx_series.hpp; include/aither_gfx950.h at AGX_FIELD_SERIES_PLAN) ----------
namespace {
constexpr double SERIES_MAX_COUNT = 16777216.0;     // points of a plan or a locate, rows of a ring
// ids of a plan that this library does not keep (the 5-equation libraries: the rans variables)
int series_id_refused(const agx_ctx* c, const Block& b, int id, int kind, int var) {
  if (kind == 0) {
    if (!kept_cell_id(var))
      return fail("agx_field_upload: AGX_FIELD_SERIES_PLAN: variable %d (tke, sdr, f1, f2, "
                  "their gradients and residuals) is not kept by the 5-equation libraries", var);
    if (var == AGX_OUT_VISCOSITY && !c->sp.viscous)
      return fail("viscosity_ is only kept for viscous runs (procBlock.cpp:6171)");
    return 0;
  }
  if (!kept_wall_id(var))
    return fail("agx_field_upload: AGX_FIELD_SERIES_PLAN: wall variable %d (tke, sdr) is not "
                "kept by the 5-equation libraries", var);
  if (!c->cfg.is_viscous)
    return fail("agx_field_upload: AGX_FIELD_SERIES_PLAN: wall variables need a viscous context "
                "(an inviscid run keeps no wallData_)");
  if (b.wall_tab.empty())
    return fail("agx_field_upload: AGX_FIELD_SERIES_PLAN: block %d has no viscousWall surface",
                id);
  return 0;
}
int series_plan_upload(agx_ctx* c, int id, const double* in) {
  static const char F[] = "AGX_FIELD_SERIES_PLAN";
  Block& b = c->blocks[id];
  long kind, P, V, cap;
  if (payload_entry(F, in, 0, "kind: 0 cells, 1 wall faces", 0, 1, &kind)) return 1;
  if (payload_entry(F, in, 1, "P, the points", 0, SERIES_MAX_COUNT, &P)) return 1;
  if (P == 0) {
    HIPCHK(hipStreamSynchronize(c->stream));     // (before the rows are freed)
    b.series = Block::Series();
    return 0;
  }
  if (payload_entry(F, in, 2, "V, the variables", 1, AGX_OUT_COUNT, &V)) return 1;
  if (payload_entry(F, in, 3, "capacity, the rows of the record", 1, SERIES_MAX_COUNT, &cap))
    return 1;
  Block::Series s;
  s.kind = (int)kind; s.V = (int)V; s.P = P; s.wall_epoch = b.wall_epoch;
  for (long v = 0; v < V; ++v) {
    long var;
    if (payload_entry(F, in, 4 + v, "a variable id", 0, 2147483647.0, &var)) return 1;
    if (kind == 0 ? var >= AGX_OUT_COUNT : var < AGX_WALL_YPLUS || var >= AGX_WALL_END)
      return fail("agx_field_upload: %s: entry %ld: unknown output variable %ld (a plan of "
                  "kind %ld holds %s)", F, 4 + v, var, kind,
                  kind == 0 ? "cell ids < AGX_OUT_COUNT" : "wall ids AGX_WALL_*");
    if (series_id_refused(c, b, id, (int)kind, (int)var)) return 1;
    s.var[v] = (int32_t)var;
    s.grads = s.grads || (kind == 0 && var >= AGX_OUT_VELGRAD && var < AGX_OUT_RESID);
  }
  const int per = kind == 0 ? 3 : 1;
  std::vector<long> pts((size_t)P);
  const int nn[3] = {b.d.ni, b.d.nj, b.d.nk};
  for (long p = 0; p < P; ++p) {
    if (kind == 0) {
      long ijk[3];
      for (int d = 0; d < 3; ++d)
        if (payload_entry(F, in, 4 + V + 3 * p + d, d == 0 ? "i of a cell" : d == 1 ? "j of a cell"
                         : "k of a cell", 0, nn[d] - 1, &ijk[d])) return 1;
      pts[p] = (ijk[2] * b.d.nj + ijk[1]) * b.d.ni + ijk[0];
    } else if (payload_entry(F, in, 4 + V + p, "a face of the wall payload", 0,
                            (double)(b.wall_faces - 1), &pts[p])) {
      return 1;
    }
  }
  const size_t nrow = (size_t)V * P;
  if (s.pts.upload(pts) != hipSuccess || s.rows.alloc((size_t)cap * nrow) != hipSuccess)
    return fail("agx_field_upload: %s: no device memory for %ld rows of %zu doubles", F, cap,
                nrow);
  s.payload.assign(in, in + 4 + V + per * P);
  s.ring.reset(cap);
  s.t.assign((size_t)cap, 0.0);
  HIPCHK(hipStreamSynchronize(c->stream));       // (before the old rows are freed)
  b.series = std::move(s);
  return 0;
}
int series_sample(agx_ctx* c, int id, double t) {
  static const char F[] = "AGX_FIELD_SERIES_SAMPLE";
  Block& b = c->blocks[id];
  Block::Series& s = b.series;
  if (s.payload.empty()) return no_plan("agx_field_upload", F, id, "AGX_FIELD_SERIES_PLAN");
  if (!std::isfinite(t)) return fail("agx_field_upload: %s: the time %g is not finite", F, t);
  if (s.ring.full())
    return fail("agx_field_upload: %s: the record of block %d is full (%ld rows, its capacity): "
                "collect the rows first (download AGX_FIELD_SERIES_ROWS, then upload the number "
                "of rows to drop); nothing is overwritten", F, id, s.ring.count);
  const bool wall = s.kind == 1;
  if (wall) {
    if (s.wall_epoch != b.wall_epoch)
      return fail("agx_field_upload: %s: the wall surfaces of block %d changed since its plan was "
                  "uploaded; upload the plan again (AGX_FIELD_SERIES_PLAN)", F, id);
    if (wall_data_missing(c, b, "agx_field_upload", F)) return 1;
  }
  // gradients and wall faces are evaluated with the ghost cells the next residual would see
  if ((wall || s.grads) && ghosts_for_output(c, "agx_field_upload")) return 1;
  double* row = s.rows.get() + (size_t)s.ring.next() * s.V * s.P;
  const dim3 grid((unsigned)((s.P * s.V + 255) / 256));
  const OutSpec sp = out_spec(c, b, s.V, s.var);
  if (wall)
    hipLaunchKernelGGL(k_series_wall, grid, dim3(256), 0, c->stream, b.d, c->gas, sp,
                       b.wall_tab_dev.get(), (int)b.wall_tab.size(), wall_eval_flags(c),
                       s.pts.get(), s.P, row);
  else
    hipLaunchKernelGGL(k_series_cells, grid, dim3(256), 0, c->stream, b.d, c->gas, sp,
                       s.pts.get(), s.P, row);
  HIPCHK(hipGetLastError());
  s.t[(size_t)s.ring.next()] = t;
  s.ring.push();
  return 0;
}
int series_drop(agx_ctx* c, int id, double n) {
  static const char F[] = "AGX_FIELD_SERIES_ROWS";
  Block::Series& s = c->blocks[id].series;
  if (s.payload.empty()) return no_plan("agx_field_upload", F, id, "AGX_FIELD_SERIES_PLAN");
  if (!std::isfinite(n) || n != std::floor(n) || n < 0.0 || n > (double)s.ring.count)
    return fail("agx_field_upload: %s: cannot drop %g rows: the record of block %d holds %ld "
                "(an integer from 0 to that)", F, n, id, s.ring.count);
  s.ring.drop((long)n);
  return 0;
}
int series_locate(agx_ctx* c, int id, const double* in) {
  static const char F[] = "AGX_FIELD_SERIES_LOCATE";
  Block& b = c->blocks[id];
  long P;
  if (payload_entry(F, in, 0, "P, the points", 1, SERIES_MAX_COUNT, &P)) return 1;
  for (long n = 0; n < 3 * P; ++n)
    if (!(std::fabs(in[1 + n]) <= 1e150))
      return fail("agx_field_upload: %s: entry %ld (coordinate %ld of point %ld) is %g: a finite "
                  "value of at most 1e150 in magnitude is expected", F, 1 + n, n % 3, n / 3,
                  in[1 + n]);
  double* dp = nullptr;
  if (stage_buffer(c, (size_t)3 * P, &dp)) return 1;
  if ((size_t)4 * P > b.locate_out.size()) {
    HIPCHK(hipStreamSynchronize(c->stream));     // (before the old one is freed)
    b.locate_n = 0;
    if (b.locate_out.alloc((size_t)4 * P) != hipSuccess)
      return fail("agx_field_upload: %s: no device memory for the result of %ld points", F, P);
  }
  HIPCHK(hipMemcpyAsync(dp, in + 1, sizeof(double) * 3 * P, hipMemcpyHostToDevice, c->stream));
  constexpr int PPW = SERIES_LOCATE_PPW;
  hipLaunchKernelGGL(k_series_locate<PPW>, dim3((unsigned)((P + PPW - 1) / PPW)), dim3(256), 0,
                     c->stream, b.d, P, dp, b.locate_out.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));       // (the caller's points have been read)
  b.locate_n = P;
  return 0;
}
}  // namespace

static int series_field_upload(agx_ctx* c, int id, int field, const double* in) {
  if (!c->finalized) return fail("agx_setup_finalize has not been called");
  switch (field) {
    case AGX_FIELD_SERIES_PLAN: return series_plan_upload(c, id, in);
    case AGX_FIELD_SERIES_SAMPLE: return series_sample(c, id, in[0]);
    case AGX_FIELD_SERIES_ROWS: return series_drop(c, id, in[0]);
  }
  return series_locate(c, id, in);
}

static int series_field_download(agx_ctx* c, int id, int field, double* out) {
  Block& b = c->blocks[id];
  const Block::Series& s = b.series;
  if (field == AGX_FIELD_SERIES_SAMPLE)
    return fail("agx_field_download: AGX_FIELD_SERIES_SAMPLE is upload only (a sample's time); "
                "AGX_FIELD_SERIES_ROWS holds the record");
  if (field == AGX_FIELD_SERIES_LOCATE) {
    if (b.locate_n == 0)
      return fail("agx_field_download: AGX_FIELD_SERIES_LOCATE: block %d has located no points "
                  "yet (upload the points first)", id);
    return copy_out(c, out, b.locate_out.get(), (size_t)4 * b.locate_n);
  }
  if (s.payload.empty())
    return no_plan("agx_field_download", field == AGX_FIELD_SERIES_PLAN
                   ? "AGX_FIELD_SERIES_PLAN" : "AGX_FIELD_SERIES_ROWS", id, "AGX_FIELD_SERIES_PLAN");
  if (field == AGX_FIELD_SERIES_PLAN) {
    std::copy(s.payload.begin(), s.payload.end(), out);
    return 0;
  }
  const size_t nrow = (size_t)s.V * s.P;
  out[0] = (double)s.P; out[1] = s.V; out[2] = (double)s.ring.count;
  out[3] = (double)s.ring.capacity;
  // oldest first: the run from the head to the end of the ring, then the run that wrapped
  long n[2];
  s.ring.runs(&n[0], &n[1]);
  const long first[2] = {s.ring.head, 0};
  double* dst = out + 4;
  for (int r = 0; r < 2; ++r) {
    if (n[r] == 0) continue;
    HIPCHK(hipMemcpy2DAsync(dst + 1, sizeof(double) * (nrow + 1),
                            s.rows.get() + (size_t)first[r] * nrow, sizeof(double) * nrow,
                            sizeof(double) * nrow, (size_t)n[r], hipMemcpyDeviceToHost,
                            c->stream));
    dst += (size_t)n[r] * (nrow + 1);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  for (long r = 0; r < s.ring.count; ++r)
    out[4 + (size_t)r * (nrow + 1)] = s.t[(size_t)s.ring.slot(r)];
  return 0;
}

// ---- spectra (agx_spectra.hpp; include/aither_gfx950.h at AGX_FIELD_SPECTRA_PLAN) ------------
namespace {
// doubles of a plan payload; the header of an accumulator payload follows it
size_t spectra_plan_size(const SpectraShape& s) { return 4 + (size_t)s.nvar + 2 * (size_t)s.npair; }
int spectra_plan_upload(agx_ctx* c, int id, const double* in) {
  static const char F[] = "AGX_FIELD_SPECTRA_PLAN";
  Block& b = c->blocks[id];
  long along, over, nvar, npair;
  if (payload_entry(F, in, 2, "nvar, the variables", 0, 2147483647.0, &nvar)) return 1;
  if (nvar == 0) {
    HIPCHK(hipStreamSynchronize(c->stream));     // (before the memory is freed)
    b.spectra = Block::Spectra();
    return 0;
  }
  if (nvar > SPECTRA_MAX_VAR)
    return fail("agx_field_upload: %s: nvar = %ld: a plan holds at most %d variables", F, nvar,
                SPECTRA_MAX_VAR);
  if (payload_entry(F, in, 0, "along: 0 i, 1 j, 2 k", 0, 2, &along)) return 1;
  if (payload_entry(F, in, 1, "over, the mask of the pooled directions", 0, 7, &over)) return 1;
  if (payload_entry(F, in, 3, "npair, the pairs", 0, SPECTRA_MAX_PAIR, &npair)) return 1;
  if (over >> along & 1)
    return fail("agx_field_upload: %s: over (mask %ld) contains along (%ld): a direction is "
                "transformed or pooled, not both", F, over, along);
  Block::Spectra sp;
  SpectraDev& d = sp.dev;
  memset(&d, 0, sizeof d);
  const agx_gas& a = c->cfg.gas;
  const double fac[6] = {a.rho_ref, a.a_ref, a.a_ref, a.a_ref, a.rho_ref * a.a_ref * a.a_ref,
                         a.t_ref};
  static const int OUT_ID[6] = {AGX_OUT_DENSITY, AGX_OUT_VEL_X, AGX_OUT_VEL_Y, AGX_OUT_VEL_Z,
                                AGX_OUT_PRESSURE, AGX_OUT_TEMPERATURE};
  for (long v = 0; v < nvar; ++v) {
    long var;
    if (payload_entry(F, in, 4 + v, "a variable id", 0, 2147483647.0, &var)) return 1;
    int code = -1;
    for (int n = 0; n < 6; ++n)
      if (var == OUT_ID[n]) code = n;
    if (code < 0)
      return fail("agx_field_upload: %s: entry %ld: variable %ld is not one of density, vel_x, "
                  "vel_y, vel_z, pressure, temperature", F, 4 + v, var);
    for (long u = 0; u < v; ++u)
      if (d.var[u] == code)
        return fail("agx_field_upload: %s: entry %ld: variable %ld is repeated", F, 4 + v, var);
    d.var[v] = code;
    sp.factor[v] = fac[code] * fac[code];
  }
  for (int n = 0; n < SPECTRA_MAX_PAIR; ++n) d.pair_spec[n] = -1;
  for (long p = 0; p < npair; ++p) {
    long ab[2];
    for (int e = 0; e < 2; ++e)
      if (payload_entry(F, in, 4 + nvar + 2 * p + e, "a variable of a pair, an index into the "
                       "plan's variables", 0, (double)(nvar - 1), &ab[e])) return 1;
    if (ab[0] == ab[1])
      return fail("agx_field_upload: %s: pair %ld is (%ld, %ld): the auto-spectrum of a variable "
                  "is kept already", F, p, ab[0], ab[1]);
    const int lo = (int)(ab[0] < ab[1] ? ab[0] : ab[1]), hi = (int)(ab[0] < ab[1] ? ab[1] : ab[0]);
    int& slot = d.pair_spec[spectra_pair_index(lo, hi)];
    if (slot >= 0)
      return fail("agx_field_upload: %s: pair %ld, (%ld, %ld), is repeated (in this or in the "
                  "other order)", F, p, ab[0], ab[1]);
    slot = (int)(nvar + p);
    sp.factor[nvar + p] = fac[d.var[ab[0]]] * fac[d.var[ab[1]]];
  }
  const int ext[3] = {b.d.ni, b.d.nj, b.d.nk};
  if (ext[along] < 2)
    return fail("agx_field_upload: %s: block %d has N = %d cells along direction %ld: a spectrum "
                "needs N >= 2", F, id, ext[along], along);
  if (!spectra_shape(ext, (int)along, (int)over, (int)nvar, (int)npair, &d.s))
    return fail("agx_field_upload: %s: block %d has N = %d cells along direction %ld: the line "
                "kernel holds lines of at most AGX_SPECTRA_MAX_N = %d cells", F, id, ext[along],
                along, SPECTRA_MAX_N);
  const SpectraShape& s = d.s;
  std::vector<double> tw(2 * (size_t)s.n), lines((size_t)s.nrec);
  for (int q = 0; q < s.n; ++q) {
    const long double ang = 2.0L * 3.14159265358979323846264338327950288L * q / s.n;
    tw[2 * q] = (double)cosl(ang);
    tw[2 * q + 1] = (double)sinl(ang);
  }
  for (long r = 0; r < s.nrec; ++r) lines[r] = (double)spectra_record_lines(s, r);
  const size_t nval = (size_t)spectra_values(s);
  if (sp.tw.upload(tw) != hipSuccess || sp.lines.upload(lines) != hipSuccess ||
      sp.part.alloc((size_t)s.nrec * nval) != hipSuccess || sp.S.alloc(nval) != hipSuccess)
    return fail("agx_field_upload: %s: no device memory for %ld records of %zu doubles", F,
                s.nrec, nval);
  HIPCHK(hipMemsetAsync(sp.S.get(), 0, sizeof(double) * nval, c->stream));
  sp.payload.assign(in, in + spectra_plan_size(s));
  HIPCHK(hipStreamSynchronize(c->stream));       // (before the old memory is freed)
  b.spectra = std::move(sp);
  return 0;
}
int spectra_sample(agx_ctx* c, int id, double w) {
  static const char F[] = "AGX_FIELD_SPECTRA_SAMPLE";
  Block& b = c->blocks[id];
  Block::Spectra& sp = b.spectra;
  if (sp.payload.empty()) return no_plan("agx_field_upload", F, id, "AGX_FIELD_SPECTRA_PLAN");
  if (!std::isfinite(w) || w < 0.0)
    return fail("agx_field_upload: %s: the weight %g is negative or not finite (w > 0 samples, "
                "w == 0 resets the block's spectra)", F, w);
  const SpectraShape& s = sp.dev.s;
  const long nval = spectra_values(s);
  if (w == 0.0) {
    HIPCHK(hipMemsetAsync(sp.S.get(), 0, sizeof(double) * nval, c->stream));
    sp.W = sp.samples = 0.0;
    return 0;
  }
  const double W = sp.W + w, r = w / W;
  const dim3 grid((unsigned)(s.nchunk * s.nfix));
  const bool small = spectra_lds_doubles(s.n, s.nvar, s.tl) <= SPECTRA_LDS_SMALL;
  by_int<1, 2, 3, 4, 5, 6>(s.nvar, [&](auto nv) {
    constexpr int NV = decltype(nv)::value;
    if (small)
      hipLaunchKernelGGL((k_spectra_lines<NV, SPECTRA_LDS_SMALL>), grid, dim3(256), 0, c->stream,
                         b.d, c->gas, sp.dev, sp.tw.get(), sp.part.get());
    else
      hipLaunchKernelGGL((k_spectra_lines<NV, SPECTRA_LDS_DOUBLES>), grid, dim3(256), 0,
                         c->stream, b.d, c->gas, sp.dev, sp.tw.get(), sp.part.get());
    return 0;
  });
  hipLaunchKernelGGL(k_spectra_join, dim3((unsigned)((nval + 255) / 256)), dim3(256), 0, c->stream,
                     nval, s.nrec, sp.lines.get(), sp.part.get(), r, sp.S.get());
  HIPCHK(hipGetLastError());
  sp.W = W;
  sp.samples += 1.0;
  return 0;
}
int spectra_accum_upload(agx_ctx* c, int id, const double* in) {
  static const char F[] = "AGX_FIELD_SPECTRA_ACCUM";
  Block::Spectra& sp = c->blocks[id].spectra;
  if (sp.payload.empty()) return no_plan("agx_field_upload", F, id, "AGX_FIELD_SPECTRA_PLAN");
  const SpectraShape& s = sp.dev.s;
  const size_t np = spectra_plan_size(s);
  for (size_t n = 0; n < np; ++n)
    if (!(in[n] == sp.payload[n]))
      return fail("agx_field_upload: %s: entry %zu of the payload's plan is %g, the plan of block "
                  "%d holds %g: an average is carried on under the plan it was taken with", F, n,
                  in[n], id, sp.payload[n]);
  const double* h = in + np;
  if (h[2] != (double)s.nbin || h[3] != (double)s.nmode)
    return fail("agx_field_upload: %s: the payload holds %g bins of %g modes, the plan of block "
                "%d gives %ld of %d", F, h[2], h[3], id, s.nbin, s.nmode);
  if (!std::isfinite(h[0]) || h[0] < 0.0 || !std::isfinite(h[1]) || h[1] < 0.0)
    return fail("agx_field_upload: %s: the sum of weights %g or the sample count %g is negative "
                "or not finite", F, h[0], h[1]);
  HIPCHK(hipMemcpyAsync(sp.S.get(), h + 4, sizeof(double) * spectra_values(s),
                        hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  sp.W = h[0];
  sp.samples = h[1];
  return 0;
}
}  // namespace

static int spectra_field_upload(agx_ctx* c, int id, int field, const double* in) {
  if (!c->finalized) return fail("agx_setup_finalize has not been called");
  switch (field) {
    case AGX_FIELD_SPECTRA_PLAN: return spectra_plan_upload(c, id, in);
    case AGX_FIELD_SPECTRA_SAMPLE: return spectra_sample(c, id, in[0]);
    case AGX_FIELD_SPECTRA_ACCUM: return spectra_accum_upload(c, id, in);
  }
  if (c->blocks[id].spectra.payload.empty())
    return no_plan("agx_field_upload", "AGX_FIELD_SPECTRA_VALUES", id, "AGX_FIELD_SPECTRA_PLAN");
  return fail("agx_field_upload: AGX_FIELD_SPECTRA_VALUES is download only (the dimensional "
              "spectra); AGX_FIELD_SPECTRA_ACCUM carries an average on");
}

static int spectra_field_download(agx_ctx* c, int id, int field, double* out) {
  if (!out) return fail("agx_field_download: null pointer");
  const Block::Spectra& sp = c->blocks[id].spectra;
  if (field == AGX_FIELD_SPECTRA_PLAN || field == AGX_FIELD_SPECTRA_SAMPLE)
    return fail("agx_field_download: %s is upload only; AGX_FIELD_SPECTRA_ACCUM holds the plan "
                "and the accumulators", field == AGX_FIELD_SPECTRA_PLAN
                ? "AGX_FIELD_SPECTRA_PLAN" : "AGX_FIELD_SPECTRA_SAMPLE");
  const bool raw = field == AGX_FIELD_SPECTRA_ACCUM;
  if (sp.payload.empty())
    return no_plan("agx_field_download", raw ? "AGX_FIELD_SPECTRA_ACCUM"
                   : "AGX_FIELD_SPECTRA_VALUES", id, "AGX_FIELD_SPECTRA_PLAN");
  const SpectraShape& s = sp.dev.s;
  const size_t nval = (size_t)spectra_values(s);
  if (raw) {
    out = std::copy(sp.payload.begin(), sp.payload.end(), out);
    out[0] = sp.W; out[1] = sp.samples; out[2] = (double)s.nbin; out[3] = s.nmode;
    return copy_out(c, out + 4, sp.S.get(), nval);
  }
  if (copy_out(c, out, sp.S.get(), nval)) return 1;
  // dimensional: the product of the two variables' output factors, as k_stats_pack's second
  // moments
  const size_t per = (size_t)s.nbin * s.nmode;
  for (int n = 0; n < s.nvar + s.npair; ++n)
    for (size_t e = 0; e < per; ++e) out[n * per + e] = out[n * per + e] * sp.factor[n];
  return 0;
}

// ---- the entry points of the output: what they dispatch to is defined above ------------------
int agx_field_download(agx_ctx* c, int id, int field, double* out) {
  if (flush_consn(c)) return 1;
  if (id < 0 || id >= (int)c->blocks.size()) return fail("bad block id %d", id);
  if (agx::field_is_stats(field)) return stats_field_download(c, id, field, out);
  if (agx::field_is_series(field)) return series_field_download(c, id, field, out);
  if (agx::field_is_spectra(field)) return spectra_field_download(c, id, field, out);
  Block& b = c->blocks[id];
  // (the D2 arrays hold x with the writer's tag in its two lowest mantissa bits: while the
  // planes are current -- an upload or a multigrid transfer wrote them last -- they are the
  // untagged x itself, zero ghost cells of a restriction included)
  if (field == AGX_FIELD_UPDATE && b.x_is_zero) {
    const int g = b.d.ng;
    memset(out, 0, sizeof(double) * AGX_NEQ * (size_t)(b.d.ni + 2 * g) * (b.d.nj + 2 * g) *
                       (b.d.nk + 2 * g));
    return 0;
  }
  if (field == AGX_FIELD_UPDATE && b.d.d2.base && !b.x_planes_current && d2_x_copy(c, b, 0))
    return 1;
  // (k_lusgs_prepare forms the diagonal inside the D2 arrays, as 1 / a beside x: the plane
  // d.a keeps the spectral radii the residual summed, without the time term)
  if (field == AGX_FIELD_DIAGONAL && b.d.d2.base)
    return fail("agx_field_download: the diagonal-ordered LU-SGS path keeps the scalar diagonal "
                "a_ only as 1 / a inside its sweep arrays, not as a field (AGX_LUSGS=plane, the "
                "hyperplane form, keeps it)");
  if (field >= AGX_FIELD_VEL_GRAD && field <= AGX_FIELD_PRESS_GRAD) {
    // cell-centre gradients: formed on demand into a temporary (an output path)
    const long ncell = (long)b.d.ni * b.d.nj * b.d.nk;
    double* tmp = nullptr;
    if (ghosts_for_output(c, "agx_field_download")) return 1;
    if (stage_buffer(c, (size_t)3 * NGF * ncell, &tmp)) return 1;
    hipLaunchKernelGGL(k_cell_grads, cell_grid(b.d, CELL_BLOCK), CELL_BLOCK, 0, c->stream, b.d,
                       c->gas, tmp);
    HIPCHK(hipGetLastError());
    const int off = field == AGX_FIELD_VEL_GRAD ? 0 : 9 + 3 * (field - AGX_FIELD_TEMP_GRAD);
    const int nc = field == AGX_FIELD_VEL_GRAD ? 9 : 3;
    // strided device -> host copy of the requested columns
    HIPCHK(hipMemcpy2DAsync(out, sizeof(double) * nc, tmp + off, sizeof(double) * 3 * NGF,
                            sizeof(double) * nc, ncell, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
  }
  if (field == AGX_FIELD_TEMPERATURE || field == AGX_FIELD_VISCOSITY) {
    // formed on demand from the current state into a scratch plane (the x_old
    // plane of DPLUR: rebuilt at the start of every implicit iteration)
    if (field == AGX_FIELD_VISCOSITY && !c->sp.viscous)
      return fail("viscosity_ is only kept for viscous runs (procBlock.cpp:6171)");
    double* scratch = b.d.xold[0];
    hipLaunchKernelGGL(k_aux_field, dim3((b.d.nplane + 255) / 256), dim3(256), 0, c->stream,
                       b.d, c->gas, field == AGX_FIELD_VISCOSITY ? 1 : 0, scratch);
    HIPCHK(hipGetLastError());
    double* one[1] = {scratch};
    const int g = b.d.ng;
    return download_aos(c, b, out, one, 1, b.d.ni + 2 * g, b.d.nj + 2 * g, b.d.nk + 2 * g, g);
  }
  double* const* p; int nc, gh;
  if (!geom_field_info(b, field, &p, &nc, &gh)) {      // (gh: the face direction here)
    if (b.node_built && !c->finalized)
      return fail("the geometry of a node-built block is complete after agx_setup_finalize");
    const int g = b.d.ng;
    return download_aos(c, b, out, p, nc, b.d.ni + 2 * g + (gh == 0), b.d.nj + 2 * g + (gh == 1),
                        b.d.nk + 2 * g + (gh == 2), g);
  }
  if (field_info(b, field, &p, &nc, &gh))
    return fail("unknown field %d", field);
  const int g = gh ? b.d.ng : 0;
  return download_aos(c, b, out, p, nc, b.d.ni + 2 * g, b.d.nj + 2 * g, b.d.nk + 2 * g, g);
}

// The ids of a call are of one range of agx_out_ranges.hpp: its table holds the ranges, their
// precedence and their bounds on nvar, its classifier the refusals of a call that has none
int agx_output_pack(agx_ctx* c, int id, int nvar, const int32_t* vars, double* out) {
  if (flush_consn(c)) return 1;
  if (id < 0 || id >= (int)c->blocks.size()) return fail("bad block id %d", id);
  const agx::OutCall call = agx::out_classify(nvar, vars);
  switch (call.range) {
    case agx::OUT_FLUX: return surface_fluxes(c, id, nvar, vars, out);
    case agx::OUT_BUDGET: return block_budget(c, id, nvar, vars, out);
    case agx::OUT_CSTAT: return stats_collapse(c, id, nvar, vars, out);
    case agx::OUT_WSTAT: return stats_pack(c, id, true, nvar, vars, out);
    case agx::OUT_STAT: return stats_pack(c, id, false, nvar, vars, out);
    case agx::OUT_LOAD: return wall_loads(c, id, nvar, vars, out);
    case agx::OUT_NODE: {
      int32_t ids[AGX_OUT_COUNT];
      for (int v = 0; v < nvar; ++v) ids[v] = vars[v] - AGX_NODE_BASE;
      return point_pack(c, id, true, nvar, ids, out);
    }
    case agx::OUT_WALL: return wall_pack(c, id, nvar, vars, out);
    case agx::OUT_CELL: return point_pack(c, id, false, nvar, vars, out);
  }
  return fail("%s", call.refusal);
}

int agx_restart_pack(agx_ctx* c, int id, int which, double* out) {
  if (flush_consn(c)) return 1;
  if (id < 0 || id >= (int)c->blocks.size()) return fail("bad block id %d", id);
  if (which != 0 && which != 1) return fail("agx_restart_pack: which is 0 (state) or 1 (consVarsNm1)");
  Block& b = c->blocks[id];
  const long ncell = (long)b.d.ni * b.d.nj * b.d.nk;
  double* tmp = nullptr;
  if (stage_buffer(c, (size_t)(AGX_NEQ + 1) * ncell, &tmp)) return 1;
  hipLaunchKernelGGL(k_restart_pack, cell_grid(b.d, CELL_BLOCK), CELL_BLOCK, 0, c->stream, b.d,
                     out_spec(c, b), which, tmp);
  return copy_out(c, out, tmp, (size_t)(AGX_NEQ + 1) * ncell);
}

// ---- start and resume on the device (agx_start.hpp) ------------------------------------------
namespace {
// what the three entries refuse alike, in this order; nothing has been touched when they do
int start_refused(agx_ctx* c, int id, const char* who, const void* p0, const void* p1 = "") {
  if (!c->finalized) return fail("%s: agx_setup_finalize has not been called", who);
  if (id < 0 || id >= (int)c->blocks.size()) return fail("bad block id %d", id);
  if (!p0 || !p1) return fail("%s: null pointer", who);
  return 0;
}
// the reference's "nonphysical density / pressure" asserts (procBlock.cpp:304-305, :329-330)
// on one nondimensional primitive state; row < 0: the state of agx_state_fill
int start_state_refused(const char* who, const double* s, long row) {
  char where[48] = "";
  if (row >= 0) snprintf(where, sizeof where, " (cloud state %ld)", row);
  for (int e = 0; e < AGX_NEQ; ++e)
    if (!std::isfinite(s[e])) return fail("%s: non-finite value%s", who, where);
  if (!(s[0] > 0.0)) return fail("%s: nonphysical density%s", who, where);
  if (!(s[4] > 0.0)) return fail("%s: nonphysical pressure%s", who, where);
  return 0;
}
// the bookkeeping of agx_state_upload before it writes, and its tail after the state planes
// have been written by a kernel here
int start_state_begin(agx_ctx* c, Block& b) {
  field_written_by_caller(c);
  if (flush_consn(c)) return 1;
  planes_uploaded(b);
  return 0;
}
int start_state_end(agx_ctx* c, Block& b) {
  HIPCHK(hipGetLastError());
#if AGX_NEQ == 7
  // (agx_state_upload: viscosity_ before the first iteration)
  hipLaunchKernelGGL(k_aux_field, dim3((b.d.nplane + 255) / 256), dim3(256), 0, c->stream, b.d,
                     c->gas, 1, b.d.viscp);
  HIPCHK(hipGetLastError());
#endif
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
void start_fill(agx_ctx* c, Block& b, const StartPrim& prim, int physical) {
  const BlockDev& d = b.d;
  const long n = (long)(d.nk + 2 * d.ng) * (d.nj + 2 * d.ng) * d.sx;
  hipLaunchKernelGGL(k_state_fill, geo_grid(n), dim3(256), 0, c->stream, d, prim, physical);
}
// the divisors of ReadSolFromRestart (output.cpp:1197-1222) / ReadSolNm1FromRestart
// (:1262-1287), formed in the reference's order
RestartDiv restart_divisors(const agx_ctx* c, int which) {
  const double rR = c->cfg.gas.rho_ref, aR = c->cfg.gas.a_ref, muR = c->gas.mu_ref;
  const double prim[7] = {rR, aR, aR, aR, rR * aR * aR, aR * aR, aR * aR * rR / muR};
  const double cons[7] = {rR, aR * rR, aR * rR, aR * rR, rR * aR * aR, aR * aR * rR,
                          aR * aR * rR * rR / muR};
  RestartDiv dv;
  dv.rho = rR;
  for (int e = 0; e < AGX_NEQ; ++e) dv.v[e] = which == 0 ? prim[e] : cons[e];
  return dv;
}
}  // namespace

int agx_state_fill(agx_ctx* c, int id, const double* prim) {
  if (start_refused(c, id, "agx_state_fill", prim)) return 1;
  if (start_state_refused("agx_state_fill", prim, -1)) return 1;
  Block& b = c->blocks[id];
  if (start_state_begin(c, b)) return 1;
  StartPrim pv;
  for (int e = 0; e < AGX_NEQ; ++e) pv.v[e] = prim[e];
  start_fill(c, b, pv, 1);
  return start_state_end(c, b);
}

int agx_state_from_cloud(agx_ctx* c, int id, int64_t npts, const double* points,
                         const double* states, double* max_dist) {
  if (start_refused(c, id, "agx_state_from_cloud", points, states)) return 1;
  if (npts < 1) return fail("agx_state_from_cloud: npts %lld < 1", (long long)npts);
  for (int64_t r = 0; r < npts; ++r)
    if (start_state_refused("agx_state_from_cloud", states + AGX_NEQ * r, (long)r)) return 1;
  Block& b = c->blocks[id];
  const BlockDev& d = b.d;
  const long ncell = (long)d.ni * d.nj * d.nk;
  constexpr int CPT = AGX_CLOUD_CPT;           // cells of a thread (k_cloud_nearest)
  const long nwg = (ncell + 256 * CPT - 1) / (256 * CPT);
  if (start_state_begin(c, b)) return 1;
  double* buf = nullptr;
  if (stage_buffer(c, (size_t)((3 + AGX_NEQ) * npts + nwg), &buf)) return 1;
  double *dp = buf, *ds = buf + 3 * npts, *part = ds + AGX_NEQ * npts;
  HIPCHK(hipMemcpyAsync(dp, points, sizeof(double) * 3 * npts, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(ds, states, sizeof(double) * AGX_NEQ * npts, hipMemcpyHostToDevice,
                        c->stream));
  start_fill(c, b, StartPrim{}, 0);
  hipLaunchKernelGGL(k_cloud_nearest<CPT>, dim3((unsigned)nwg), dim3(256), 0, c->stream, d,
                     (long)npts, dp, ds, part);
  if (max_dist) {
    std::vector<double> host((size_t)nwg);
    if (copy_out(c, host.data(), part, (size_t)nwg)) return 1;
    *max_dist = *std::max_element(host.begin(), host.end());
  }
  return start_state_end(c, b);
}

int agx_restart_unpack(agx_ctx* c, int id, int which, const double* in) {
  if (start_refused(c, id, "agx_restart_unpack", in)) return 1;
  if (which != 0 && which != 1)
    return fail("agx_restart_unpack: which is 0 (state) or 1 (consVarsNm1)");
  Block& b = c->blocks[id];
  if (which == 1) {       // (what agx_field_upload refuses of this field, in its words)
    double* const* p; int nc, gh;
    if (field_info(b, AGX_FIELD_CONS_NM1, &p, &nc, &gh))
      return fail("field %d cannot be uploaded", AGX_FIELD_CONS_NM1);
  }
  const BlockDev& d = b.d;
  const long ncell = (long)d.ni * d.nj * d.nk;
  if (start_state_begin(c, b)) return 1;
  // the payload through the staging buffer of upload_aos
  double* tmp = nullptr;
  if (stage_buffer(c, (size_t)RST_NV * ncell, &tmp)) return 1;
  HIPCHK(hipMemcpyAsync(tmp, in, sizeof(double) * RST_NV * ncell, hipMemcpyHostToDevice,
                        c->stream));
  if (which == 0) start_fill(c, b, StartPrim{}, 0);
  hipLaunchKernelGGL(k_restart_unpack, geo_grid(ncell), dim3(256), 0, c->stream, d,
                     restart_divisors(c, which), which, tmp);
  if (which == 0) return start_state_end(c, b);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- set-up helpers -------------------------------------------------
int agx_plot3d_metrics(agx_ctx* c, int ni, int nj, int nk, const double* nodes, double* vol,
                       double* center, double* fai, double* faj, double* fak, double* fci,
                       double* fcj, double* fck) {
  if (ni < 1 || nj < 1 || nk < 1) return fail("empty block");
  HIPCHK(hipSetDevice(c->device));
  const long nn = (long)(ni + 1) * (nj + 1) * (nk + 1), ncell = (long)ni * nj * nk;
  const long nf[3] = {(long)(ni + 1) * nj * nk, (long)ni * (nj + 1) * nk, (long)ni * nj * (nk + 1)};
  double* host_out[8] = {vol, center, fai, faj, fak, fci, fcj, fck};
  const long count[8] = {ncell, 3 * ncell, 4 * nf[0], 4 * nf[1], 4 * nf[2], 3 * nf[0], 3 * nf[1],
                         3 * nf[2]};
  size_t total = (size_t)3 * nn;
  for (int q = 0; q < 8; ++q) if (host_out[q]) total += (size_t)count[q];
  double* buf = nullptr;
  if (stage_buffer(c, total, &buf)) return 1;
  HIPCHK(hipMemcpyAsync(buf, nodes, sizeof(double) * 3 * nn, hipMemcpyHostToDevice, c->stream));
  double* dev_out[8];
  double* cur = buf + 3 * nn;
  for (int q = 0; q < 8; ++q) { dev_out[q] = host_out[q] ? cur : nullptr; if (host_out[q]) cur += count[q]; }
  MetricsOut o;
  o.vol = dev_out[0]; o.center = dev_out[1];
  for (int d = 0; d < 3; ++d) { o.fa[d] = dev_out[2 + d]; o.fc[d] = dev_out[5 + d]; }
  HIPCHK(hipMemsetAsync(c->err_dev.get(), 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(k_plot3d_metrics, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, c->stream,
                     ni, nj, nk, buf, o, c->err_dev.get());
  HIPCHK(hipGetLastError());
  for (int q = 0; q < 8; ++q)
    if (host_out[q])
      HIPCHK(hipMemcpyAsync(host_out[q], dev_out[q], sizeof(double) * count[q],
                            hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(c->err_host.get(), c->err_dev.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (*c->err_host.get() == 4) {
    *c->err_host.get() = 0;
    hipMemsetAsync(c->err_dev.get(), 0, sizeof(int), c->stream);
    return fail("negative volume in PLOT3D block");
  }
  return 0;
}

int agx_nearest_wall_distance(agx_ctx* c, int64_t ncell, const double* cen, int64_t nwall,
                              const double* wall, double* dist) {
  if (ncell < 1) return 0;
  if (nwall < 1) return fail("no wall points");
  HIPCHK(hipSetDevice(c->device));
  double* buf = nullptr;
  if (stage_buffer(c, (size_t)(4 * ncell + 3 * nwall), &buf)) return 1;
  double *dc = buf, *dw = buf + 3 * ncell, *dd = dw + 3 * nwall;
  HIPCHK(hipMemcpyAsync(dc, cen, sizeof(double) * 3 * ncell, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dw, wall, sizeof(double) * 3 * nwall, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_nearest_wall, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, c->stream,
                     (long)ncell, dc, (long)nwall, dw, dd);
  return copy_out(c, dist, dd, (size_t)ncell);
}

int agx_field_upload(agx_ctx* c, int id, int field, const double* in) {
  // (an upload of x writes this block's planes and, on the D2 path, copies them to its D2
  // arrays below: the planes of this block are current afterwards, those of the other blocks
  // are what they were)
  // (the statistics, the time series and the spectra write nothing the solver reads: a sample
  // is a read of the run and leaves every flag as a read would, a plan, a locate and an upload
  // of accumulators own their memory)
  const bool stats = agx::field_is_stats(field), series = agx::field_is_series(field);
  if (stats || series || agx::field_is_spectra(field)) {
    if (flush_consn(c)) return 1;
    if (id < 0 || id >= (int)c->blocks.size()) return fail("bad block id %d", id);
    if (!in) return fail("agx_field_upload: null pointer");
    return stats    ? stats_field_upload(c, id, field, in)
           : series ? series_field_upload(c, id, field, in)
                    : spectra_field_upload(c, id, field, in);
  }
  field_written_by_caller(c);
  if (flush_consn(c)) return 1;
  if (id < 0 || id >= (int)c->blocks.size()) return fail("bad block id %d", id);
  Block& b = c->blocks[id];
  double* const* p; int nc, gh;
  if (field >= AGX_FIELD_VOLUME && field <= AGX_FIELD_WALL_DIST)
    return fail("field %d (geometry) cannot be uploaded: it is set when the block is created",
                field);
  if (field_info(b, field, &p, &nc, &gh)) return fail("field %d cannot be uploaded", field);
  const int g = gh ? b.d.ng : 0;
  if (upload_aos(c, b, in, p, nc, b.d.ni + 2 * g, b.d.nj + 2 * g, b.d.nk + 2 * g, g)) return 1;
  if (field == AGX_FIELD_UPDATE) x_uploaded(b);
  if (field == AGX_FIELD_RESIDUAL) c->have_residual = true;
  if (field == AGX_FIELD_UPDATE && b.d.d2.base) return d2_x_copy(c, b, 1);
  return 0;
}

// ---- geometric multigrid (include/aither_gfx950.h) -------------------------------------------
namespace {
int mg_solver_ok(agx_ctx* c) {
  if (!c->sp.implicit) return fail("multigrid: implicit time integration only");
  return 0;
}
// On the diagonal-ordered LU-SGS path x lives in the D2 arrays; the multigrid kernels work on
// the planes: current planes before they read, the D2 arrays (tagged) after they wrote.
// (x_planes_current: nothing wrote the D2 x since the last copy -- sweeps, exchanges and the
// prepare kernel clear it, x_changed; an upload of x copies the block's planes itself)
int mg_x_to_planes(agx_ctx* c, Block& b) {
  return b.d.d2.base && !b.x_planes_current ? d2_x_copy(c, b, 0) : 0;
}
int mg_x_from_planes(agx_ctx* c, Block& b) { return b.d.d2.base ? d2_x_copy(c, b, 1) : 0; }
// x of a block's planes changed outside sweeps and exchanges: the records' copy follows
void mg_x_records(agx_ctx* c, Block& b) {
  if (b.d.sw_dyn)
    hipLaunchKernelGGL(k_mg_x_records, dim3((unsigned)((b.d.nplane + 255) / 256)), dim3(256), 0,
                       c->stream, b.d);
}
int mg_check(agx_ctx* f, agx_ctx* cz, int blk) {
  if (!f || !cz) return fail("mg: null context");
  if (blk < 0 || blk >= (int)f->blocks.size() || blk >= (int)cz->blocks.size())
    return fail("mg: bad block %d", blk);
  if (f->device != cz->device) return fail("mg: the two levels live on different devices");
  for (agx_ctx* c : {f, cz})
    if (mg_solver_ok(c)) return 1;
  return 0;
}
// AGX_NEQ zeroed planes, once; *view: the BlockDev member that shows them to the kernels
int mg_planes(agx_ctx* c, Block& b, DevBuf<double>& p, double** view) {
  if (!p) {
    HIPCHK(p.alloc((size_t)AGX_NEQ * b.d.nplane));
    HIPCHK(hipMemsetAsync(p.get(), 0, sizeof(double) * AGX_NEQ * b.d.nplane, c->stream));
  }
  *view = p.get();
  return 0;
}
// the device copies of a fine block's transfer maps (uploaded when the host pointer changes)
int mg_maps(agx_ctx* f, Block& b, const int32_t* tc, const double* vf, const double* cf,
            int cni, int cnj, int cnk, MgMap* m) {
  const BlockDev& d = b.d;
  const size_t ncell = (size_t)d.ni * d.nj * d.nk;
  if (tc && b.mg_tc_key != tc) {
    HIPCHK(hipStreamSynchronize(f->stream));
    if (!b.mg_tc) HIPCHK(b.mg_tc.alloc(3 * ncell));
    HIPCHK(hipMemcpy(b.mg_tc.get(), tc, sizeof(int) * 3 * ncell, hipMemcpyHostToDevice));
    // first fine index of every coarse cell, per direction (the map is a product of three
    // monotone 1-D maps: procBlock.cpp:6556-6581)
    std::vector<int> st((size_t)cni + cnj + cnk + 3, 0);
    int* s0 = st.data();
    int* s1 = s0 + cni + 1;
    int* s2 = s1 + cnj + 1;
    const int n[3] = {d.ni, d.nj, d.nk}, cn[3] = {cni, cnj, cnk};
    int* ss[3] = {s0, s1, s2};
    for (int dir = 0; dir < 3; ++dir) {
      int cc = 0;
      ss[dir][0] = 0;
      for (int q = 0; q < n[dir]; ++q) {
        const size_t cell = dir == 0 ? (size_t)q : dir == 1 ? (size_t)q * d.ni : (size_t)q * d.ni * d.nj;
        const int to = tc[3 * cell + dir];
        if (to < 0 || to >= cn[dir] || to < cc) return fail("mg: to_coarse is not a monotone map onto the coarse block");
        while (cc < to) ss[dir][++cc] = q;
      }
      while (cc < cn[dir]) ss[dir][++cc] = n[dir];
    }
    HIPCHK(b.mg_start.upload(st));
    b.mg_tc_key = tc;
  }
  if (vf && b.mg_vf_key != vf) {
    HIPCHK(hipStreamSynchronize(f->stream));
    if (!b.mg_vf) HIPCHK(b.mg_vf.alloc(ncell));
    HIPCHK(hipMemcpy(b.mg_vf.get(), vf, sizeof(double) * ncell, hipMemcpyHostToDevice));
    b.mg_vf_key = vf;
  }
  if (cf && b.mg_cf_key != cf) {
    HIPCHK(hipStreamSynchronize(f->stream));
    if (!b.mg_cf) HIPCHK(b.mg_cf.alloc(7 * ncell));
    HIPCHK(hipMemcpy(b.mg_cf.get(), cf, sizeof(double) * 7 * ncell, hipMemcpyHostToDevice));
    b.mg_cf_key = cf;
  }
  if (!b.mg_tc) return fail("mg: no fine-to-coarse map for this block yet");
  m->tc = b.mg_tc.get();
  m->start[0] = b.mg_start.get();
  m->start[1] = m->start[0] + cni + 1;
  m->start[2] = m->start[1] + cnj + 1;
  m->vf = b.mg_vf.get();
  m->cf = b.mg_cf.get();
  return 0;
}
// the other level's stream has finished what it was given (the two contexts may run on
// different streams)
int mg_order(agx_ctx* producer, agx_ctx* consumer) {
  if (producer->stream != consumer->stream) HIPCHK(hipStreamSynchronize(producer->stream));
  return 0;
}
}  // namespace

int agx_mg_restrict(agx_ctx* f, agx_ctx* cz, int blk, int what, const int32_t* tc,
                    const double* vf) {
  if (mg_check(f, cz, blk)) return 1;
  Block &bf = f->blocks[blk], &bc = cz->blocks[blk];
  if (what < AGX_MG_STATE || what > AGX_MG_FORCING) return fail("mg_restrict: bad selector %d", what);
  if (what != AGX_MG_FORCING && !vf) return fail("mg_restrict: volume weights missing");
  if (flush_consn(f) || flush_consn(cz)) return 1;
  // (AGX_MG_STATE writes the coarse block's state planes; the other selectors leave them)
  planes_uploaded(bc);
  MgMap m;
  if (mg_maps(f, bf, tc, vf, nullptr, bc.d.ni, bc.d.nj, bc.d.nk, &m)) return 1;
  if (what == AGX_MG_UPDATE && mg_x_to_planes(f, bf)) return 1;
  if (what == AGX_MG_FORCING && mg_x_to_planes(cz, bc)) return 1;   // (ghosts of the exchange)
  if (mg_order(f, cz)) return 1;
  if (what == AGX_MG_STATE) {
    // (coarse.Zero(): ghost cells included, procBlock.hpp:641)
    for (int e = 0; e < AGX_NEQ; ++e)
      HIPCHK(hipMemsetAsync(bc.d.state[e], 0, sizeof(double) * bc.d.nplane, cz->stream));
    field_written_by_caller(cz);
    cz->mg_coarse = true;
  } else if (what == AGX_MG_UPDATE) {
    for (int e = 0; e < AGX_NEQ; ++e)
      HIPCHK(hipMemsetAsync(bc.d.x[e], 0, sizeof(double) * bc.d.nplane, cz->stream));
  } else {
    if (!bf.d.mg_mres) return fail("mg_restrict: the fine level has no matrix residual yet");
    if (mg_planes(cz, bc, bc.mg_forcing, &bc.d.mg_forcing)) return 1;
  }
  hipLaunchKernelGGL(k_mg_restrict, cell_grid(bc.d, CELL_BLOCK), CELL_BLOCK, 0, cz->stream, bf.d,
                     bc.d, m, what);
  if (what == AGX_MG_FORCING)
    hipLaunchKernelGGL(k_mg_axmb, cell_grid(bc.d, CELL_BLOCK), CELL_BLOCK, 0, cz->stream, bc.d,
                       cz->gas, cz->sp);
  if (what == AGX_MG_UPDATE) {
    mg_x_records(cz, bc);
    if (mg_x_from_planes(cz, bc)) return 1;
  }
#if AGX_FAST
  // (b of the diagonal-ordered sweeps: formed again, now with the forcing term)
  if (what == AGX_MG_FORCING && bc.d.d2.base && d2_prepare(cz, bc, 0, 1, 0)) return 1;
#endif
  HIPCHK(hipGetLastError());
  return 0;
}

int agx_mg_matrix_residual(agx_ctx* c, double* mr) {
  if (mg_solver_ok(c)) return 1;
  for (auto& blk : c->blocks) {
    if (mg_planes(c, blk, blk.mg_mres, &blk.d.mg_mres)) return 1;
    if (mg_x_to_planes(c, blk)) return 1;
  }
  // (the plane form: the diagonal-ordered reductions form the norm only)
  c->mres_plane_form = true;
  const int rc = agx_phase_matrix_residual(c, mr);
  c->mres_plane_form = false;
  return rc;
}

int agx_mg_invert_diagonal(agx_ctx* c) { return implicit_begin(c, 0); }

// gridLevel::ResetDiagonal (gridLevel.cpp:408-412) of a coarse level, whose residual adds to the
// diagonal (SolverDev::diag_add); the finest level's kernels overwrite theirs
int agx_mg_reset_diagonal(agx_ctx* c) {
  for (auto& blk : c->blocks) {
    HIPCHK(hipMemsetAsync(blk.d.a, 0, sizeof(double) * blk.d.nplane, c->stream));
    if (blk.d.am)
      HIPCHK(hipMemsetAsync(blk.d.am, 0, sizeof(double) * AGX_NJ * blk.d.nplane, c->stream));
    if (AGX_NEQ > 5) {
      HIPCHK(hipMemsetAsync(blk.d.a_t, 0, sizeof(double) * blk.d.nplane, c->stream));
      if (blk.d.am_t)
        HIPCHK(hipMemsetAsync(blk.d.am_t, 0, sizeof(double) * 2 * blk.d.nplane, c->stream));
    }
  }
  return 0;
}

int agx_mg_save_update(agx_ctx* c) {
  for (auto& blk : c->blocks) {
    if (mg_planes(c, blk, blk.mg_xsave, &blk.d.mg_xsave)) return 1;
    if (mg_x_to_planes(c, blk)) return 1;
    hipLaunchKernelGGL(k_mg_axpy, dim3((unsigned)((blk.d.nplane + 255) / 256)), dim3(256), 0,
                       c->stream, blk.d, 1);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int agx_mg_prolong(agx_ctx* cz, agx_ctx* f, int blk, const int32_t* tc, const double* cf) {
  if (mg_check(f, cz, blk)) return 1;
  Block &bf = f->blocks[blk], &bc = cz->blocks[blk];
  if (!bc.d.mg_xsave) return fail("mg_prolong: no saved update on the coarse level");
  if (!cf) return fail("mg_prolong: interpolation coefficients missing");
  MgMap m;
  if (mg_maps(f, bf, tc, nullptr, cf, bc.d.ni, bc.d.nj, bc.d.nk, &m)) return 1;
  const long nn = (long)(bc.d.ni + 1) * (bc.d.nj + 1) * (bc.d.nk + 1);
  if (!bc.mg_nodes) HIPCHK(bc.mg_nodes.alloc((size_t)AGX_NEQ * nn));
  if (mg_x_to_planes(cz, bc) || mg_x_to_planes(f, bf)) return 1;
  hipLaunchKernelGGL(k_mg_axpy, dim3((unsigned)((bc.d.nplane + 255) / 256)), dim3(256), 0,
                     cz->stream, bc.d, 0);
  const dim3 tb = CELL_BLOCK;
  hipLaunchKernelGGL(k_mg_nodes, dim3((bc.d.ni + tb.x) / tb.x, (bc.d.nj + tb.y) / tb.y, bc.d.nk + 1),
                     tb, 0, cz->stream, bc.d, bc.mg_nodes.get());
  HIPCHK(hipGetLastError());
  if (mg_order(cz, f)) return 1;
  hipLaunchKernelGGL(k_mg_prolong, cell_grid(bf.d, tb), tb, 0, f->stream, bf.d, m,
                     (const double*)bc.mg_nodes.get(), bc.d.ni, bc.d.nj, bc.d.nk);
  mg_x_records(cz, bc);
  mg_x_records(f, bf);
  if (mg_x_from_planes(cz, bc) || mg_x_from_planes(f, bf)) return 1;
  HIPCHK(hipGetLastError());
  return 0;
}

int agx_store_time_n(agx_ctx* c, int also_nm1) {
  if (flush_consn(c)) return 1;
  c->have_time_n = true;
  state_became_time_n(c);
  // Explicit fused path: the stage-0 launch of k_residual_tile forms
  // cons(state) anyway and writes it to consVarsN itself (5 stores instead of a
  // separate 5-load/5-store pass); anything else that touches consVarsN or the
  // state first calls flush_consn().  (AGX_NO_LAZY_CONSN: always the pass of its own)
  if (!c->no_lazy_consn && !also_nm1 && !c->use_gather && all_tile_ok(c)) { c->consn_pending = true; return 0; }
  for (auto& blk : c->blocks)
    hipLaunchKernelGGL(k_store_time_n, cell_grid(blk.d, CELL_BLOCK), CELL_BLOCK,
                       0, c->stream, blk.d, c->gas, also_nm1);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- phases ---------------------------------------------------------------
int agx_phase_bc_faces(agx_ctx* c) {
  if (bc_faces(c)) return 1;
  c->ghost_fill_open = true;      // (until the residual has read these ghost cells)
  return 0;
}
int agx_phase_bc_edges(agx_ctx* c) { return bc_edges(c); }

#if AGX_FAST
// May the viscous tile kernel of this residual finish the block's cells for the sweeps (its
// RHS form), so that implicit_begin skips k_lusgs_prepare?  Only where that pass would be the
// lean one with the norm fold, would write no x, and forms b from the residual alone.  (A
// dual-time term is excluded rather than formed: the kernel would have to keep the spectral
// radius beside a.)  The caller adds: only inside agx_iterate -- through the phase API a
// caller may read or change the residual between the phases, so there the kernel folds the
// norms (an upload of the residual makes them stale: planes_uploaded) and the pass stays.
static bool rhs_form_applies(const agx_ctx* c, const Block& blk) {
  const BlockDev& b = blk.d;
  return b.d2.base && blk.d2_state_current && c->d2_state_update &&
         c->resid_norms_prepare && !has_connection(b) && !c->sp.requires_init && c->state_is_time_n &&
         !c->sp.bdf2 && !b.mg_forcing && !c->sp.diag_add && !c->mg_coarse &&
         !(c->sp.dual_time_cfl > 0.0) && !c->sp.les;
}
#endif

// The viscous residual of one block, behind its inviscid one (launch_inv).
#if AGX_NEQ == 7
static int launch_visc(agx_ctx* c, Block& blk, double cfl) {
  const int fourth = c->cfg.viscous_recon == AGX_VISC_RECON_CENTRAL_4TH ? 1 : 0;
  const BlockDev& vb = blk.d;
  if (c->visc_gather) {
    hipLaunchKernelGGL(k_visc_residual_rans, cell_grid(vb, CELL_BLOCK), CELL_BLOCK,
                       0, c->stream, vb, c->gas, c->sp, cfl, fourth);
    return 0;
  }
  // face-once form: every face evaluated by one thread, records through memory (the
  // blocks run one after the other on the stream and share the record buffer)
  RansRec rec;
  rec.ni1 = vb.ni + 1; rec.nj1 = vb.nj + 1;
  rec.nf = (long)rec.ni1 * rec.nj1 * (vb.nk + 1);
  const size_t need = (size_t)3 * RANS_REC * rec.nf;
  if (need > c->rans_rec.size()) {
    HIPCHK(hipStreamSynchronize(c->stream));     // (before the old one is freed)
    HIPCHK(c->rans_rec.alloc(need));
  }
  rec.p = c->rans_rec.get();
  const dim3 tb = CELL_BLOCK;
  auto fgrid = [&](int di, int dj, int dk) {
    return dim3((vb.ni + di + tb.x - 1) / tb.x, (vb.nj + dj + tb.y - 1) / tb.y, vb.nk + dk);
  };
  hipLaunchKernelGGL(k_rans_faces<0>, fgrid(1, 0, 0), tb, 0, c->stream, vb, c->gas, fourth, rec);
  hipLaunchKernelGGL(k_rans_faces<1>, fgrid(0, 1, 0), tb, 0, c->stream, vb, c->gas, fourth, rec);
  hipLaunchKernelGGL(k_rans_faces<2>, fgrid(0, 0, 1), tb, 0, c->stream, vb, c->gas, fourth, rec);
  hipLaunchKernelGGL(k_rans_cells, cell_grid(vb, tb), tb, 0, c->stream, vb, c->gas, c->sp,
                     cfl, fourth, rec);
  return 0;
}
#else
#if AGX_FAST
static int launch_visc_tile(agx_ctx* c, Block& blk, double cfl, bool fourth) {
  const BlockDev& vb = blk.d;
  // 62 x 6 owned cells per workgroup and k-step (centralFourth: 60 x 6); persistent
  // workgroups, one per CU (the kernel's LDS windows fill a CU), each marching its share
  // of the (column tile, k) steps by the plan (agx_tile_plan.hpp)
  const int gx = tile_count(vb.ni, fourth ? TILE_VISC_I_F4 : TILE_VISC_I);
  const int gy = tile_count(vb.nj, TILE_J);
  const long steps = (long)gx * gy * vb.nk;
  const int nwg = (int)std::min<long>(c->num_cu, std::max<long>(1, steps / 8));
  const TilePlan tp = tile_plan_of(c, gx, gy, vb.nk, nwg,
                                   fourth ? TILE_CHARGE_VISC_F4 : TILE_CHARGE_VISC,
                                   c->tile_order_visc);
  if (!fourth && rhs_form_applies(c, blk)) {
    // the RHS forms: the residual norms from here, VT_R partials per workgroup, folded
    // into prepare's slot right behind the launch (the partials are one area for all
    // blocks) -- and inside agx_iterate b, 1 / a and the aInv_ plane as well
    if (c->in_iterate) {
      c->sp.un_is_u = 1;        // (as implicit_begin sets it: state_is_time_n holds)
      VtRhs<VT_RHS_FULL> rz;
      rz.partials = c->partials.get();
      rz.pab = reinterpret_cast<char*>(vb.d2.base + 2L * PA_B * vb.d2.nd2);
      rz.arr16 = vb.d2.nd2 * 16;
      rz.ps16 = vb.d2.ps * 16;
      rz.Pi = vb.d2.Pi;
      rz.Pj = vb.d2.Pj;
      hipLaunchKernelGGL((k_visc_tile<false, false, VT_RHS_FULL>), dim3(nwg),
                         dim3(VT_L, VT_R), 0, c->stream, make_slab(vb), c->gas, c->sp, cfl,
                         gx, tp, rz);
      rhs_written_by_residual(blk);
    } else {
      hipLaunchKernelGGL((k_visc_tile<false, false, VT_RHS_NORMS>), dim3(nwg),
                         dim3(VT_L, VT_R), 0, c->stream, make_slab(vb), c->gas, c->sp, cfl,
                         gx, tp, VtRhs<VT_RHS_NORMS>{c->partials.get()});
    }
    const size_t n = (size_t)(&blk - c->blocks.data());
    if (reduce_norms(c, n, (long)nwg * VT_R, c->norm_prepare() + n)) return 1;
    resid_norms_folded(blk);
    return 0;
  }
  // (largeEddySimulation: the instantiations with the WALE arm, which also write the
  // run's eddy-viscosity plane)
  by_bool(c->sp.les != 0, [&](auto les) {
    by_bool(fourth, [&](auto f4) {
      hipLaunchKernelGGL((k_visc_tile<f4, decltype(les)::value>), dim3(nwg),
                         dim3(VT_L, VT_R), 0, c->stream, make_slab(vb), c->gas, c->sp, cfl,
                         gx, tp, VtRhs<VT_RHS_NONE>{});
    });
  });
  return 0;
}
#endif
static int launch_visc(agx_ctx* c, Block& blk, double cfl) {
  const bool fourth = c->cfg.viscous_recon == AGX_VISC_RECON_CENTRAL_4TH;
  const bool wide_plane = (double)blk.d.nplane * 8.0 >= 4294967296.0;
  if (!AGX_FAST || c->visc_gather || ((fourth || c->sp.les) && (c->visc_march || wide_plane))) {
    // (one thread per cell, the stencil straight from the planes: AGX_VISC=gather, and
    // centralFourth or largeEddySimulation -- k_visc_march has no WALE arm -- where the
    // tile kernel's 32-bit plane offsets do not reach)
    hipLaunchKernelGGL(c->sp.les ? k_visc_residual_les : k_visc_residual,
                       cell_grid(blk.d, CELL_BLOCK), CELL_BLOCK, 0, c->stream, blk.d, c->gas,
                       c->sp, cfl, fourth ? 1 : 0);
    return 0;
  }
  const BlockDev& vb = blk.d;
  if (c->visc_march || wide_plane) {
    const int gx = (vb.ni + VTI - 1) / VTI, gy = (vb.nj + VTJ - 1) / VTJ;
    int nz = std::max(1, std::min(vb.nk / 8, (int)std::lround(2048.0 / (gx * gy))));
    const int kchunk = (vb.nk + nz - 1) / nz;
    nz = (vb.nk + kchunk - 1) / kchunk;
    hipLaunchKernelGGL(k_visc_march, dim3(gx, gy, nz), dim3(64, VTJ + 1), 0, c->stream,
                       vb, c->gas, c->sp, cfl, kchunk);
    return 0;
  }
#if AGX_FAST    // (no other build has the tile kernel; there the first arm took every block)
  return launch_visc_tile(c, blk, cfl, fourth);
#else
  return 0;
#endif
}
#endif  // AGX_NEQ == 7

int agx_phase_residual(agx_ctx* c, int mm, double cfl) {
  if (c->cfg.dt_nondim <= 0.0 && cfl <= 0.0)
    return fail("Neither dt or cfl was specified!");   // procBlock.cpp:813-816
  c->ghost_fill_open = false;
  c->sp.diag_add = c->mg_coarse ? 1 : 0;
  const bool fuse = can_fuse(c);
  resid_written(c);
  if (fuse) state_written(c);      // (the fused stage advances the state as it goes)
  const int store_consn = !c->use_gather && all_tile_ok(c) && c->consn_pending && mm == 0;
  if (store_consn) c->consn_pending = false;
  else if (flush_consn(c)) return 1;
  {
    Timer t(c, G_RESID);
    long off = 0;
    for (auto& blk : c->blocks) {
      const MarchPlan mp = march_plan(c, blk.d);
      MarchArgs ma;
      memset(&ma, 0, sizeof ma);
      ma.kchunk = mp.kchunk;
      ma.mode = c->cfg.time_integration == AGX_TIME_RK4 ? 1 : 0;
      ma.store_consn = store_consn;
      const double rk_alpha[4] = {0.25, 1.0 / 3.0, 0.5, 1.0};   // procBlock.cpp:938
      ma.alpha = rk_alpha[mm & 3];
      ma.partials = c->partials.get() + off;
      ma.ablate = c->ablate;      // (0 unless this is a -DAGX_ABLATION build: AGX_ABLATE)
      ma.plan = mp.tile;
      launch_inv(c, blk.d, cfl, fuse, ma, mp);
      off += mp.nparts;
      if (c->sp.implicit && c->sp.block) launch_block_diag(c, blk.d);
    }
  }
  HIPCHK(hipGetLastError());
  c->fused_pending = fuse;
  c->have_residual = true;
  if (c->cfg.is_viscous) {
    {
      Timer t(c, G_BC);
      if (bc_pass(c, true, 1)) return 1;
      if (bc_pass(c, false, 1)) return 1;
      c->have_wall_data = true;
    }
    Timer t(c, G_VISC);
    for (auto& blk : c->blocks)
      if (launch_visc(c, blk, cfl)) return 1;
#if AGX_NEQ != 7     // (the rans viscous kernel accumulates its Jacobians itself)
    if (c->sp.implicit && c->sp.block)
      for (auto& blk : c->blocks)
        hipLaunchKernelGGL(k_block_diag_visc, cell_grid(blk.d, CELL_BLOCK), CELL_BLOCK, 0,
                           c->stream, blk.d, c->gas, c->sp,
                           c->cfg.viscous_recon == AGX_VISC_RECON_CENTRAL_4TH ? 1 : 0);
#endif
    HIPCHK(hipGetLastError());
  }
  // the gradients of this residual's state feed the nonreflecting ghost states of
  // the ghost fills up to the next residual (CalcGrads*, procBlock.cpp:6143)
  for (auto& blk : c->blocks)
    if (blk.nr_max > 0) {
      Timer t(c, G_BC);
      hipLaunchKernelGGL(k_nr_grads, dim3((blk.nr_max + 255) / 256, blk.d.nsurf), dim3(256), 0,
                         c->stream, blk.d, c->gas);
      HIPCHK(hipGetLastError());
    }
  return 0;
}

int agx_phase_explicit_update(agx_ctx* c, int mm, double* l2, agx_linf* linf) {
  const int mode = c->cfg.time_integration == AGX_TIME_RK4 ? 1 : 0;
  return update_pass(c, mode, mm, l2, linf);
}

#if AGX_FAST
// k_lusgs_prepare of one block (write_x: a launch that writes x is a writer launch: it tags
// the values and advances the epoch)
// norms: fold the residual norms into the block's prepare slot of norm_out (AGX_RESID_NORMS).
// The lean form where the update left the block's D2 state current (AGX_D2_STATE); an
// `again` launch keeps the full one.
static int d2_prepare(agx_ctx* c, Block& blk, int write_x, int again, int norms) {
  const BlockDev& b = blk.d;
  const dim3 grid((b.d2.Pi + TT - 1) / TT, (b.d2.Pj + TT - 1) / TT, b.nk + 2 * b.ng);
  const bool lean = blk.d2_state_current && !again;
  const int ghost_s = has_connection(b) ? 1 : 0;
  const unsigned tag = write_x ? (unsigned)(++blk.kp_epoch) & 3u : 0u;
  by_bool(lean, [&](auto is_lean) {
    by_bool(norms != 0, [&](auto with_norms) {
      hipLaunchKernelGGL((k_lusgs_prepare<decltype(is_lean)::value, with_norms>), grid, dim3(256),
                         0, c->stream, b, c->gas, c->sp, write_x, tag, again, ghost_s,
                         c->partials.get());
    });
  });
  if (norms) {
    const size_t n = (size_t)(&blk - c->blocks.data());
    if (reduce_norms(c, n, (long)grid.x * grid.y * grid.z, c->norm_prepare() + n)) return 1;
    resid_norms_folded(blk);
  }
  return 0;
}
#endif
int agx_phase_implicit_begin(agx_ctx* c) { return implicit_begin(c, 1); }
// (write_x = 0: gridLevel::InvertDiagonal alone, for a coarse multigrid level)
static int implicit_begin(agx_ctx* c, int write_x) {
  x_changed(c);
  // (the group counts a launch only where a block still takes the pass)
  bool any_pass = false;
  for (auto& blk : c->blocks) any_pass = any_pass || !(write_x && blk.rhs_in_d2);
  std::unique_ptr<Timer> t;
  if (any_pass) t = std::make_unique<Timer>(c, G_PREPARE);
  c->sp.un_is_u = c->state_is_time_n ? 1 : 0;   // (read by every rhs_b of this iteration)
  for (auto& blk : c->blocks) {
    const BlockDev& b = blk.d;
#if AGX_FAST
    const bool rhs_done = write_x && blk.rhs_in_d2;
    rhs_taken(blk);
    if (rhs_done) {
      // the viscous tile kernel of this residual wrote b, 1 / a and the aInv_ plane and its
      // norms are folded (rhs_form_applies): nothing is left of the pass.  x = 0 stays
      // unwritten as the lean launch leaves it.
      x_prepared(blk, true);
      resid_norms_folded(blk);
      continue;
    }
    if (b.d2.base) {
      // diagonal terms, b and x0 straight into the D2 arrays of the sweeps (a coarse
      // multigrid level, write_x = 0: x is the restricted one)
      const int wx = write_x && (c->sp.requires_init || has_connection(b)) ? 1 : 0;
      // (the norms ride along on the finest level's launch only: a coarse multigrid level,
      // write_x = 0, keeps the update's fold; not where the viscous tile kernel of this
      // residual folded them already)
      const int norms = write_x && c->resid_norms_prepare && !blk.resid_norms_current ? 1 : 0;
      if (d2_prepare(c, blk, wx, 0, norms)) return 1;
      x_prepared(blk, write_x && !wx);
      continue;
    }
#endif
    if (!c->sp.requires_init && write_x)   // x_[bb].Zero() incl. ghosts, linearSolver.cpp:141
      hipLaunchKernelGGL(k_zero5, dim3((b.nplane + 255) / 256), dim3(256), 0,
                         c->stream, planes(b.x), b.nplane);
    hipLaunchKernelGGL(k_implicit_begin, cell_grid(b, CELL_BLOCK), CELL_BLOCK, 0,
                       c->stream, b, c->gas, c->sp, c->err_dev.get(), write_x);
    if (b.sw_geo) {
      hipLaunchKernelGGL(k_sweep_records, dim3((unsigned)((b.nplane + 255) / 256)), dim3(256), 0,
                         c->stream, b, c->sp, blk.sweep_geo_built ? 0 : 1);
      blk.sweep_geo_built = true;
    }
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// k_dplur of one block, in the solver mode's form (solver_mode_of, agx_kernels.hpp); waits:
// the faces whose cells dplur_sweep_overlapped leaves to k_dplur_shell
static void launch_dplur(agx_ctx* c, const BlockDev& b, int waits) {
  by_int<0, 1, 2>(solver_mode_of(c->sp), [&](auto mode) {
    hipLaunchKernelGGL(k_dplur<mode>, cell_grid(b, CELL_BLOCK), CELL_BLOCK, 0, c->stream, b,
                       c->gas, c->sp, waits);
  });
}

int agx_phase_relax_forward(agx_ctx* c, int sweep) {
  x_changed(c);
  x_swept(c);
  Timer t(c, G_SWEEP);
  const int full = sweep > 0 || c->sp.requires_init;
  if (is_lusgs_solver(c) && pipe_sweep_applicable(c)) return lusgs_sweep_pipe(c, true, full);
  if (is_lusgs_solver(c) && plane_sweep_all_applicable(c)) return lusgs_sweep_all(c, true, full);
  for (auto& blk : c->blocks) {
    BlockDev& b = blk.d;
    if (is_lusgs_solver(c)) {
      if (lusgs_sweep(c, blk, true, full)) return 1;
    } else {
      // dplur::DPLUR copies x to xold (linearSolver.cpp:487) and relaxes from the
      // copy; here the two sets of planes change roles instead.  Ghost cells of
      // the new x that nobody rewrites (physical boundaries) are never read
      // (ImplicitLower/Upper only cross physical or connection faces).
      for (int e = 0; e < AGX_NEQ; ++e) std::swap(b.x[e], b.xold[e]);
      launch_dplur(c, b, 0);
    }
  }
  if (!is_lusgs_solver(c)) c->halo_set[AGX_HALO_UPDATE] ^= 1;   // (x and xold changed roles)
  HIPCHK(hipGetLastError());
  return 0;
}

int agx_phase_relax_backward(agx_ctx* c, int sweep) {
  x_changed(c);
  if (!is_lusgs_solver(c)) return 0;
  Timer t(c, G_SWEEP);
  const int full = sweep > 0 || c->sp.requires_init;
  if (pipe_sweep_applicable(c)) return lusgs_sweep_pipe(c, false, full);
  if (plane_sweep_all_applicable(c)) return lusgs_sweep_all(c, false, full);
  for (auto& blk : c->blocks) {
    if (lusgs_sweep(c, blk, false, full)) return 1;
  }
  HIPCHK(hipGetLastError());
  return 0;
}

namespace {
void matrix_residual_fold(agx_ctx* c, const NormPartial* host, double* mr) {
  double sumsq = 0.0;
  long size = 0;
  for (size_t n = 0; n < c->blocks.size(); ++n) {
    const BlockDev& b = c->blocks[n].d;
    for (int e = 0; e < AGX_NEQ; ++e) sumsq += host[n].l2[e];
    // mr.Size(): ghost-inclusive (linearSolver.cpp:66-68, mgSolution.cpp:203)
    size += (long)AGX_NEQ * (b.ni + 2 * b.ng) * (b.nj + 2 * b.ng) * (b.nk + 2 * b.ng);
  }
  *mr = size > 0 ? sumsq / (double)size : 0.0;
}
}  // namespace

int agx_phase_matrix_residual(agx_ctx* c, double* mr) {
  const bool defer = c->in_iterate;      // agx_iterate reads it back with the update's norms
  NormPartial* out = defer ? c->norm_mres() : c->norm_update();
  {
    Timer t(c, G_MRESID);
    for (size_t n = 0; n < c->blocks.size(); ++n) {
      const BlockDev& b = c->blocks[n].d;
#if AGX_FAST
      if (b.d2.base && !c->mres_plane_form) {
        // (position chunk, k) pairs dealt to the XCDs band by band, see the kernels
        const long nwg = mresid_wgs(c, b);
        if (c->mresid_march) {
          const int per = mrp_per_xcd(mrp_patches(MrpPlane{b.d2.Pi, b.d2.Pj, b.ng}));
          if (MR_LDS_BYTES > 48 * 1024)
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_matrix_resid_d2m),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)MR_LDS_BYTES));
          hipLaunchKernelGGL(k_matrix_resid_d2m, dim3((unsigned)nwg), dim3(MRP_THREADS),
                             MR_LDS_BYTES, c->stream, kp_blk_of(b), KpGas{c->gas.hf, c->gas.n, c->gas.inv_n},
                             c->sp.viscous, per, MRESID_KC, c->partials.get());
        } else
          hipLaunchKernelGGL(k_matrix_resid_d2, dim3((unsigned)nwg), dim3(256), 0, c->stream, b,
                             c->gas, c->sp, c->mresid_split, c->partials.get());
        if (reduce_norms(c, n, nwg, out + n)) return 1;
        continue;
      }
#endif
      const dim3 grid = cell_grid(b, CELL_BLOCK);
      by_int<0, 1, 2>(solver_mode_of(c->sp), [&](auto mode) {
        hipLaunchKernelGGL(k_matrix_resid<mode>, grid, CELL_BLOCK, 0, c->stream, b, c->gas, c->sp,
                           c->partials.get());
      });
      if (reduce_norms(c, n, (long)grid.x * grid.y * grid.z, out + n)) return 1;
    }
  }
  if (defer) {
    c->mres_deferred = true;
    *mr = 0.0;
    return 0;
  }
  HIPCHK(hipMemcpyAsync(c->host_update(), c->norm_update(),
                        sizeof(NormPartial) * c->blocks.size(),
                        hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  matrix_residual_fold(c, c->host_update(), mr);
  return 0;
}

int agx_phase_implicit_update(agx_ctx* c, int mm, double* l2, agx_linf* linf) {
  return update_pass(c, 2, mm, l2, linf);
}

// ---- halo -----------------------------------------------------------------
int agx_halo_swap_local(agx_ctx* c, int what) {
  if (what == AGX_HALO_UPDATE) x_changed(c);
  if (c->conns.empty()) return 0;
  Timer t(c, G_BC);
  if (c->halo_batch && c->halo_batch_sides > 0) {
    // level by level: every slice of the level, then every insert (halo_batch_plan)
    if (halo_batch_tables(c, what)) return 1;
    const auto& tab = c->halo_tab_dev[what][c->halo_set[what]];
    for (const auto& L : c->halo_levels) {
      const dim3 grid((unsigned)((L.nmax + 255) / 256), (unsigned)L.sides);
      hipLaunchKernelGGL(k_halo_gather_all, grid, dim3(256), 0, c->stream, tab[0].get() + L.first);
      hipLaunchKernelGGL(k_halo_scatter_all, grid, dim3(256), 0, c->stream, tab[1].get() + L.first);
    }
    HIPCHK(hipGetLastError());
    return 0;
  }
  for (auto& k : c->conns) {
    const agx_connection& cc = k.c;
    if (!(cc.rank[0] == c->rank && cc.rank[1] == c->rank)) continue;
    const long n0 = k.side[0].n, n1 = k.side[1].n;
    if (ensure_halo_buf(c, (n0 + n1) * AGX_NEQ)) return 1;
    // both slices are taken before either insert (multiArray3d.hpp:810-821)
    const long nmax = std::max(n0, n1);
    if (nmax > 0) {
      HaloSide g[2], p[2];      // what side 0 receives, then what side 1 receives
      halo_sides(c, k, what, c->halo_buf.get(), c->halo_buf.get() + n0 * AGX_NEQ, g, p);
      const dim3 grid((nmax + 255) / 256, 2);
      hipLaunchKernelGGL(k_halo_gather2, grid, dim3(256), 0, c->stream, g[0], g[1]);
      hipLaunchKernelGGL(k_halo_scatter2, grid, dim3(256), 0, c->stream, p[0], p[1]);
    }
  }
  HIPCHK(hipGetLastError());
  return 0;
}

static int my_side(const agx_ctx* c, const Conn& k) {
  if (k.c.rank[0] == c->rank && k.c.rank[1] != c->rank) return 0;
  if (k.c.rank[1] == c->rank && k.c.rank[0] != c->rank) return 1;
  return -1;
}
int64_t agx_halo_count(agx_ctx* c, int id, int what) {
  (void)what;
  if (id < 0 || id >= (int)c->conns.size()) return -1;
  const Conn& k = c->conns[id];
  const int s = my_side(c, k);
  if (s < 0) return 0;
  return (int64_t)AGX_NEQ * std::max(k.n_send, k.side[s].n);
}
int agx_halo_pack(agx_ctx* c, int id, int what, double* dev_buf) {
  if (id < 0 || id >= (int)c->conns.size()) return fail("bad connection id");
  Conn& k = c->conns[id];
  const int s = my_side(c, k);
  if (s < 0) return fail("connection %d is not remote", id);
  Block& b = c->blocks[k.c.local_block[s]];
  const long n = k.n_send;
  if (n) hipLaunchKernelGGL(k_halo_gather, dim3((n + 255) / 256), dim3(256), 0,
                            c->stream, halo_planes(b, what),
                            k.send_src[halo_in_d2(b, what)].get(), n, dev_buf);
  HIPCHK(hipGetLastError());
  return 0;
}
int agx_halo_unpack(agx_ctx* c, int id, int what, const double* dev_buf) {
  if (what == AGX_HALO_UPDATE) x_changed(c);
  ghost_fill_gone(c);
  if (id < 0 || id >= (int)c->conns.size()) return fail("bad connection id");
  Conn& k = c->conns[id];
  const int s = my_side(c, k);
  if (s < 0) return fail("connection %d is not remote", id);
  Block& b = c->blocks[k.c.local_block[s]];
  const long n = k.side[s].n;
  if (n) hipLaunchKernelGGL(k_halo_scatter, dim3((n + 255) / 256), dim3(256), 0,
                            c->stream, halo_planes(b, what),
                            k.side[s].map[halo_in_d2(b, what)].dst.get(), n, dev_buf);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- multi-rank -------------------------------------------------------------
int agx_set_exchange(agx_ctx* c, const agx_exchange* ex) {
  if (!ex || !ex->swap || !ex->allgather || ex->nranks < 1)
    return fail("agx_set_exchange: swap, allgather and nranks are required");
  if (c->finalized) return fail("agx_set_exchange must precede agx_setup_finalize");
  c->ex = *ex;
  c->have_ex = true;
  return 0;
}

namespace {
// built-in transport: RCCL on the library's stream
int rccl_swap(void* user, int n, const agx_slab* slabs, void* stream) {
  agx_ctx* c = static_cast<agx_ctx*>(user);
  ncclResult_t r = ncclGroupStart();
  for (int q = 0; q < n && r == ncclSuccess; ++q) {
    r = ncclSend(slabs[q].send, (size_t)slabs[q].count, ncclDouble, slabs[q].peer, c->nccl,
                 (hipStream_t)stream);
    if (r == ncclSuccess)
      r = ncclRecv(slabs[q].recv, (size_t)slabs[q].count, ncclDouble, slabs[q].peer, c->nccl,
                   (hipStream_t)stream);
  }
  const ncclResult_t e = ncclGroupEnd();
  if (r == ncclSuccess) r = e;
  return r == ncclSuccess ? 0 : fail("RCCL halo exchange failed: %s", ncclGetErrorString(r));
}
int rccl_allgather(void* user, const void* send, void* recv, int64_t bytes, void* stream) {
  agx_ctx* c = static_cast<agx_ctx*>(user);
  const ncclResult_t r = ncclAllGather(send, recv, (size_t)bytes, ncclChar, c->nccl,
                                       (hipStream_t)stream);
  return r == ncclSuccess ? 0 : fail("RCCL all-gather failed: %s", ncclGetErrorString(r));
}
}  // namespace

int agx_rccl_unique_id(void* id128) {
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  const ncclResult_t r = ncclGetUniqueId(static_cast<ncclUniqueId*>(id128));
  return r == ncclSuccess ? 0 : fail("ncclGetUniqueId: %s", ncclGetErrorString(r));
}
int agx_rccl_exchange_create(agx_ctx* c, const void* id128, int nranks, int rank) {
  if (c->finalized) return fail("agx_rccl_exchange_create must precede agx_setup_finalize");
  HIPCHK(hipSetDevice(c->device));
  ncclUniqueId id;
  memcpy(&id, id128, sizeof id);
  const ncclResult_t r = ncclCommInitRank(&c->nccl, nranks, id, rank);
  if (r != ncclSuccess) return fail("ncclCommInitRank: %s", ncclGetErrorString(r));
  agx_exchange ex;
  ex.user = c; ex.swap = rccl_swap; ex.allgather = rccl_allgather;
  ex.nranks = nranks; ex.host_buffers = 0;
  c->ex = ex;
  c->have_ex = true;
  return 0;
}

// gridLevel::GetBoundaryConditions (state) / lusgs::Relax, dplur::Relax (update):
// local connections, then the slabs of connections to other ranks
int agx_halo_exchange(agx_ctx* c, int what) {
  if (what < AGX_HALO_STATE || what > AGX_HALO_TURB) return fail("bad halo selector %d", what);
  if (what == AGX_HALO_TURB && AGX_NEQ != 7) return fail("AGX_HALO_TURB: rans library only");
  if (what >= AGX_HALO_VELGRAD_A && what <= AGX_HALO_VELGRAD_B && !(c->sp.implicit && c->sp.block))
    return fail("velocity gradients are kept (and exchanged) for the block-matrix solvers only");
  if (agx_halo_swap_local(c, what)) return 1;
  return halo_exchange_remote(c, what);
}

// the slabs of connections to other ranks: pack, the transport's swap, unpack -- all on
// c->stream (dplur_sweep_overlapped points it at its second stream meanwhile)
static int halo_exchange_remote(agx_ctx* c, int what) {
  if (c->remote.empty()) return 0;
  if (!c->have_ex) return fail("connections to other ranks need an exchange (agx_set_exchange)");
  Timer t(c, G_BC);
  for (auto& r : c->remote)
    if (agx_halo_pack(c, r.cid, what, r.send.get())) return 1;
  if (c->ex.host_buffers) {
    for (auto& r : c->remote)
      HIPCHK(hipMemcpyAsync(r.hsend.get(), r.send.get(), sizeof(double) * r.count, hipMemcpyDeviceToHost,
                            c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  // (a transport that fails says why itself -- the RCCL one does -- or leaves the text empty:
  // what an earlier failure left in it is not this swap's)
  g_err[0] = '\0';
  if (c->ex.swap(c->ex.user, (int)c->slabs.size(), c->slabs.data(), c->stream)) {
    c->swap_failed = true;
    return g_err[0] ? 1 : fail("the exchange's swap operation failed");
  }
  if (c->ex.host_buffers)
    for (auto& r : c->remote)
      HIPCHK(hipMemcpyAsync(r.recv.get(), r.hrecv.get(), sizeof(double) * r.count, hipMemcpyHostToDevice,
                            c->stream));
  for (auto& r : c->remote)
    if (agx_halo_unpack(c, r.cid, what, r.recv.get())) return 1;
  return 0;
}

// One DPLUR / BDPLUR sweep of a rank with neighbours (dplur::Relax linearSolver.cpp:509-535:
// SwapUpdate, then DPLUR on every block) with the interior / boundary split: point Jacobi
// reads the previous x of a cell's six neighbours, so only the cells next to a block face with
// a connection to another rank see a ghost cell that is still travelling.  All other cells are
// relaxed on the context's stream while the slabs of the previous x are packed, swapped and
// unpacked on a second stream; the cells of those faces follow when both are done.  Bitwise
// the sequential form (the same cell function on two disjoint sets of cells).
static bool overlap_applicable(const agx_ctx* c) {
  return c->overlap && c->sp.implicit && !is_lusgs_solver(c) && c->have_ex && !c->remote.empty();
}
static int dplur_sweep_overlapped(agx_ctx* c) {
  if (!c->ov_stream) {
    HIPCHK(hipStreamCreateWithFlags(&c->ov_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->ov_ready, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ov_done, hipEventDisableTiming));
  }
  // connections inside the rank first: their ghost cells are operands of the shell as well
  if (agx_halo_swap_local(c, AGX_HALO_UPDATE)) return 1;
  HIPCHK(hipEventRecord(c->ov_ready, c->stream));
  x_changed(c);
  std::vector<int> waits(c->blocks.size(), 0);     // faces with a connection to another rank
  for (auto& r : c->remote) {
    const Conn& k = c->conns[r.cid];
    const int sd = my_side(c, k);
    waits[k.c.local_block[sd]] |= 1 << (k.c.boundary[sd] - 1);
  }
  {
    Timer t(c, G_SWEEP);
    for (size_t n = 0; n < c->blocks.size(); ++n) {
      BlockDev bs = c->blocks[n].d;      // x and xold in the roles they take in this sweep
      for (int e = 0; e < AGX_NEQ; ++e) std::swap(bs.x[e], bs.xold[e]);
      launch_dplur(c, bs, waits[n]);
    }
    HIPCHK(hipGetLastError());
  }
  {
    struct OnStream {                    // pack / swap / unpack issue on c->stream
      agx_ctx* c; hipStream_t keep;
      OnStream(agx_ctx* c_, hipStream_t s) : c(c_), keep(c_->stream) { c->stream = s; }
      ~OnStream() { c->stream = keep; }
    } on(c, c->ov_stream);
    HIPCHK(hipStreamWaitEvent(c->ov_stream, c->ov_ready, 0));
    if (halo_exchange_remote(c, AGX_HALO_UPDATE)) return 1;
    HIPCHK(hipEventRecord(c->ov_done, c->ov_stream));
  }
  HIPCHK(hipStreamWaitEvent(c->stream, c->ov_done, 0));
  {
    Timer t(c, G_SWEEP);
    for (size_t n = 0; n < c->blocks.size(); ++n) {
      BlockDev& b = c->blocks[n].d;
      for (int e = 0; e < AGX_NEQ; ++e) std::swap(b.x[e], b.xold[e]);
      if (!waits[n]) continue;
      const long nface = std::max({(long)b.ni * b.nj, (long)b.ni * b.nk, (long)b.nj * b.nk});
      by_int<0, 1, 2>(solver_mode_of(c->sp), [&](auto mode) {
        hipLaunchKernelGGL(k_dplur_shell<mode>, dim3((unsigned)((nface + 255) / 256), 6),
                           dim3(256), 0, c->stream, b, c->gas, c->sp, waits[n]);
      });
    }
    HIPCHK(hipGetLastError());
  }
  c->halo_set[AGX_HALO_UPDATE] ^= 1;     // (x and xold changed roles)
  return 0;
}

namespace {
// main.cpp:254-264 over the exchange: every rank ends up with the global norms
// `status`: this rank's local result of the iteration; a failure anywhere makes every
// rank return failure (the collectives are reached by all ranks either way)
int reduce_over_ranks(agx_ctx* c, double* l2, agx_linf* linf, double* matrix_resid,
                      const double* l2_in, const agx_linf& linf_in, int status) {
  typedef agx_ctx::NormRecord Rec;
  const int nr = c->ex.nranks;
  Rec& mine = c->rec_host.get()[0];
  memset(&mine, 0, sizeof mine);
  for (int e = 0; e < AGX_NEQ; ++e) mine.l2[e] = l2[e] - l2_in[e];   // this call's local sums
  mine.mres = *matrix_resid;
  mine.linf = linf->linf; mine.block = linf->block; mine.i = linf->i; mine.j = linf->j;
  mine.k = linf->k; mine.eqn = linf->eqn;
  mine.status = status;
  Rec* all = c->rec_host.get() + 1;
  if (!status) g_err[0] = '\0';      // (a failing all-gather names itself, see the swap)
  if (c->ex.host_buffers) {
    if (c->ex.allgather(c->ex.user, &mine, all, (int64_t)sizeof(Rec), c->stream))
      return g_err[0] ? 1 : fail("the exchange's allgather operation failed");
  } else {
    HIPCHK(hipMemcpyAsync(c->rec_dev.get(), &mine, sizeof(Rec), hipMemcpyHostToDevice, c->stream));
    if (c->ex.allgather(c->ex.user, c->rec_dev.get(), c->rec_dev.get() + 1, (int64_t)sizeof(Rec), c->stream))
      return 1;
    HIPCHK(hipMemcpyAsync(all, c->rec_dev.get() + 1, sizeof(Rec) * nr, hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  for (int r = 0; r < nr; ++r)
    if (all[r].status != 0) {
      if (status != 0) return status;      // g_err holds this rank's own message
      return fail("agx_iterate: rank %d failed (status %d); its agx_last_error has the cause",
                  r, all[r].status);
    }
  // fold in rank order from what the caller passed in: the same result on every rank, and
  // of equal maxima the lowest rank's (MaxLinf resid.cpp:55-79 keeps the lower rank's on
  // `>=`) -- starting from this rank's own record would let a rank keep its own on a tie
  double mres = 0.0;
  for (int e = 0; e < AGX_NEQ; ++e) l2[e] = l2_in[e];
  *linf = linf_in;
  for (int r = 0; r < nr; ++r) {
    for (int e = 0; e < AGX_NEQ; ++e) l2[e] += all[r].l2[e];
    mres += all[r].mres;
    if (all[r].linf > linf->linf) {
      linf->linf = all[r].linf; linf->block = all[r].block; linf->i = all[r].i;
      linf->j = all[r].j; linf->k = all[r].k; linf->eqn = all[r].eqn;
    }
  }
  *matrix_resid = mres;
  return 0;
}
}  // namespace

// ---- mgSolution::Iterate (mgSolution.cpp:246-269) ---------------------------
int agx_iterate(agx_ctx* c, int mm, double cfl, double* l2, agx_linf* linf,
                double* matrix_resid) {
  if (!c->finalized) return fail("agx_setup_finalize has not been called");
  if (!c->remote.empty() && !c->have_ex)
    return fail("agx_iterate: connections to other ranks need an exchange "
                "(agx_set_exchange / agx_rccl_exchange_create) or the phase API");
  double l2_in[AGX_NEQ];
  for (int e = 0; e < AGX_NEQ; ++e) l2_in[e] = l2[e];
  const agx_linf linf_in = *linf;
  // A local failure (a singular block, the sweep's spin limit, a refused phase) must not
  // leave the other ranks waiting in a collective: from the first failure on the compute
  // phases are skipped, the exchanges and the final all-gather are still reached, and the
  // status word of the norm record fails the call on every rank.
  // The count: a rank that fails posts exactly the exchanges a healthy rank posts in the same
  // call -- its peers are healthy ranks.  The last of them is the state exchange of the eager
  // ghost fill, which the update queues BEFORE the device's error word is read
  // (check_device_error, behind the one host synchronisation): a failure the device found
  // (spin limit, singular block, thermally perfect energy, boundary variant) surfaces with
  // that exchange already posted, a failure before the update (a refused phase) without it.
  // So the fill is made up for at the end only where this call has not queued it
  // (!ghosts_prefilled), and the ghost cells then count as filled for the next call as they do
  // on the healthy ranks.  An exchange that itself fails ends the call wherever it was posted
  // from, the update's fill included (swap_failed).
  int st = 0;
  char first_err[sizeof g_err] = "";
  const bool collective = c->have_ex && c->ex.nranks > 1;
  c->swap_failed = false;
  auto phase = [&](int r) {
    if (r && !st) { st = r; memcpy(first_err, g_err, sizeof g_err); }
  };
#define AGX_PHASE(call)                                             \
  do {                                                              \
    if (!st) {                                                      \
      phase(call);                                                  \
      if (c->swap_failed) return st;   /* (the update's eager fill) */ \
    }                                                               \
  } while (0)
  // an exchange runs even after a local failure when other ranks take part in it; a
  // failure of the exchange itself cannot be hidden from the peers and ends the call
#define AGX_XCHG(what)                                              \
  do {                                                              \
    if (!st || collective) {                                        \
      const int r_ = agx_halo_exchange(c, what);                    \
      if (r_ && st) { memcpy(g_err, first_err, sizeof g_err); return st; } \
      if (r_) return r_;                                            \
    }                                                               \
  } while (0)
  // gridLevel::GetBoundaryConditions gridLevel.cpp:287-319 (already done behind the
  // previous call's norm read-back unless something touched the state since)
  if (!c->ghosts_prefilled && fill_ghosts(c)) return 1;
  ghost_fill_gone(c);
  struct Scope { agx_ctx* c; ~Scope() { c->in_iterate = false; } } scope{c};
  c->in_iterate = true;
  // gridLevel::CalcResidual :372-400 + CalcTimeStep :240-247
  AGX_PHASE(agx_phase_residual(c, mm, cfl));
  *matrix_resid = 0.0;
  if (c->sp.implicit) {
    // gridLevel::SwapEddyViscAndGradients gridLevel.cpp:386-388 (read by the
    // off-diagonal terms of the block-matrix solvers only)
    if (c->sp.block && c->sp.viscous && !c->conns.empty()) {
      AGX_XCHG(AGX_HALO_VELGRAD_A);
      AGX_XCHG(AGX_HALO_VELGRAD_B);
    }
    // ... and of eddyViscosity_, f1_, f2_ (SwapTurbVars :389-392), rans
    if (AGX_NEQ == 7 && !c->conns.empty()) AGX_XCHG(AGX_HALO_TURB);
    // mgSolution::ImplicitUpdate :209-244; lusgs::Relax linearSolver.cpp:430-470;
    // dplur::Relax :509-535
    AGX_PHASE(agx_phase_implicit_begin(c));
    for (int s = 0; s < c->cfg.matrix_sweeps; ++s) {
      if (!st && overlap_applicable(c)) {
        // (the exchange is part of it: its failure ends the call like AGX_XCHG's)
        const int r_ = dplur_sweep_overlapped(c);
        if (r_) return r_;
        continue;
      }
      AGX_XCHG(AGX_HALO_UPDATE);
      AGX_PHASE(agx_phase_relax_forward(c, s));
      if (is_lusgs_solver(c)) {
        AGX_XCHG(AGX_HALO_UPDATE);
        AGX_PHASE(agx_phase_relax_backward(c, s));
      }
    }
    AGX_XCHG(AGX_HALO_UPDATE);
    AGX_PHASE(agx_phase_matrix_residual(c, matrix_resid));
    AGX_PHASE(agx_phase_implicit_update(c, mm, l2, linf));
    if (!st && c->mres_deferred)      // came back with the update's norms
      matrix_residual_fold(c, c->host_mres(), matrix_resid);
    c->mres_deferred = false;
  } else {
    AGX_PHASE(agx_phase_explicit_update(c, mm, l2, linf));
  }
#undef AGX_PHASE
#undef AGX_XCHG
  // the update queues the next call's ghost fill -- an exchange -- behind its norms; a call
  // that failed before its update posts it here, one that failed in it has posted it
  if (st && collective && c->eager_ghosts && !c->ghosts_prefilled) {
    if (fill_ghosts(c)) {
      if (c->swap_failed) { memcpy(g_err, first_err, sizeof g_err); return st; }
    } else {
      ghosts_filled_ahead(c);
    }
  }
  if (st) memcpy(g_err, first_err, sizeof g_err);
  if (c->have_ex) return reduce_over_ranks(c, l2, linf, matrix_resid, l2_in, linf_in, st);
  return st;
}

// ---- measurement ------------------------------------------------------------
int agx_timing_enable(agx_ctx* c, int on) {
  if (!on) resolve_timing(c);
  c->timing = on != 0;
  return 0;
}
int agx_timing_get(agx_ctx* c, int group, double* avg_ms, int64_t* launches) {
  if (group < 0 || group >= G_NGROUP) return fail("bad timing group");
  resolve_timing(c);
  *launches = c->t_n[group];
  *avg_ms = c->t_n[group] ? c->t_ms[group] / c->t_n[group] : 0.0;
  return 0;
}
int agx_timing_reset(agx_ctx* c) {
  resolve_timing(c);
  for (int g = 0; g < G_NGROUP; ++g) { c->t_ms[g] = 0.0; c->t_n[g] = 0; }
  return 0;
}
int agx_sync(agx_ctx* c) {
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
