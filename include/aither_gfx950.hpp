// aither_gfx950.hpp -- C++14 host layer over the C-ABI of aither_gfx950.h.
//
// The reference is C++ and its driver (src/main.cpp) talks to the path through
// mgSolution::{StoreOldSolution, Iterate} and the residual / resid value types.
// This header is what a C++ host links against: the same member names, the same
// argument meaning and the same error behaviour (message on std::cerr followed
// by exit(EXIT_FAILURE), main.cpp / procBlock.cpp convention), on top of
// nothing but the extern "C" entry points.  Header-only, no torch, no Python.
//
//   reference                                   here
//   ---------------------------------------------------------------------------
//   class resid (include/resid.hpp:24-75)       aither_gfx950::resid
//   class residual (include/varArray.hpp)       aither_gfx950::residual
//   mgSolution::StoreOldSolution (:103-114)     hotPath::StoreOldSolution
//   mgSolution::Iterate (:246-269)              hotPath::Iterate
//   GetFinestGridLevel pack (procBlock.cpp:4491) hotPath::Download
//   mgSolution with several levels (:128-262)   multigrid::{StoreOldSolution, Iterate,
//                                               CycleAtLevel, Restriction, Relax, Prolongation}
//
// AGX_SYMBOL_PREFIX lets the test suite build the same driver against the CPU
// oracle (prefix ora_), which exports the identical entry points.
#ifndef AITHER_GFX950_HPP
#define AITHER_GFX950_HPP
#include <algorithm>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <string>
#include <vector>
#include "aither_gfx950.h"

#ifndef AGX_SYMBOL_PREFIX
#define AGX_SYMBOL_PREFIX agx_
#endif
#define AGX_CAT2(a, b) a##b
#define AGX_CAT(a, b) AGX_CAT2(a, b)
#define AGX_SYM(name) AGX_CAT(AGX_SYMBOL_PREFIX, name)

// The start-and-resume entries are the library's alone (the CPU oracle of the test suite has
// no device to form a state on): declared here under the prefix in use, so that a driver built
// against the oracle compiles and links as long as it does not call them.
extern "C" {
int AGX_SYM(state_fill)(AGX_CAT(AGX_SYMBOL_PREFIX, ctx) *, int, const double *);
int AGX_SYM(state_from_cloud)(AGX_CAT(AGX_SYMBOL_PREFIX, ctx) *, int, int64_t, const double *,
                              const double *, double *);
int AGX_SYM(restart_unpack)(AGX_CAT(AGX_SYMBOL_PREFIX, ctx) *, int, int, const double *);
}

namespace aither_gfx950 {

// The library that serves a deck: numEqns 5 (euler / navierStokes) or 7 (rans), and
// input::ThermodynamicModel as AGX_THERMO_* (agx_config.thermodynamic_model).  All four
// export the same agx_* entry points; agx_config_set refuses the model a library is not
// built for.
inline const char *LibraryName(int numEqns, int thermodynamicModel) {
  const bool tp = thermodynamicModel == AGX_THERMO_THERMALLY_PERFECT;
  if (numEqns == 7) return tp ? "libaither_gfx950_rans_tp.so" : "libaither_gfx950_rans.so";
  return tp ? "libaither_gfx950_tp.so" : "libaither_gfx950.so";
}

// L-infinity residual with its location, resid.hpp:24-75
class resid {
  double linf_ = 0.0;
  int blk_ = 0, i_ = 0, j_ = 0, k_ = 0, eqn_ = 0;

 public:
  resid() = default;
  resid(double a, int b, int c, int d, int e, int f)
      : linf_(a), blk_(b), i_(c), j_(d), k_(e), eqn_(f) {}
  double Linf() const { return linf_; }
  int Block() const { return blk_; }
  int ILoc() const { return i_; }
  int JLoc() const { return j_; }
  int KLoc() const { return k_; }
  int Eqn() const { return eqn_; }
  void UpdateMax(double a, int b, int c, int d, int e, int f) {
    if (a > linf_) *this = resid(a, b, c, d, e, f);
  }
  void Zero() { *this = resid(); }
};

// per-equation sum of squared residuals (what procBlock.cpp:858 accumulates)
class residual {
  std::vector<double> data_;

 public:
  explicit residual(int numEqns = 5) : data_(numEqns, 0.0) {}
  int Size() const { return static_cast<int>(data_.size()); }
  double &operator[](int r) { return data_[r]; }
  const double &operator[](int r) const { return data_[r]; }
  double *data() { return data_.data(); }
  void Zero() { data_.assign(data_.size(), 0.0); }
};

// The accelerated part of one rank's gridLevel: blocks, their boundary
// conditions and connections, and the per-iteration calls.
class hotPath {
  AGX_CAT(AGX_SYMBOL_PREFIX, ctx) *ctx_ = nullptr;
  int numEqns_ = 5;
  int numBlocks_ = 0;
  std::vector<bool> seriesPlanned_;   // blocks with a time-series plan (SetSeriesPlan)
  std::vector<bool> spectraPlanned_;  // blocks with a spectra plan (SetSpectraPlan)

  static void Check(int rc, const char *what) {
    if (rc != 0) {   // reference convention: report and stop
      const char *m = AGX_SYM(last_error)();
      std::cerr << "ERROR: Error in " << what << ": " << (m ? m : "") << std::endl;
      exit(EXIT_FAILURE);
    }
  }

 public:
  hotPath(int device, int rank) {
    Check(AGX_SYM(ctx_create)(device, rank, &ctx_), "hotPath::hotPath (ctx_create)");
  }
  ~hotPath() { if (ctx_) AGX_SYM(ctx_destroy)(ctx_); }
  hotPath(const hotPath &) = delete;
  hotPath &operator=(const hotPath &) = delete;

  void Configure(const agx_config &cfg) {
    numEqns_ = cfg.n_eq;
    Check(AGX_SYM(config_set)(ctx_, &cfg), "hotPath::Configure");
  }
  // geometry of one procBlock (ghost-inclusive arrays in the reference's own
  // layout), its boundarySurfaces and the initial state; returns the block id.
  // Or geom.nodes alone (plot3dBlock's coordinates, the nine array pointers null): the
  // library forms the whole geometry on the device, complete after Finalize; an adapter
  // whose host code wants cell centres or the wall distance then fetches them with
  // agx_field_download and AGX_FIELD_CENTER / AGX_FIELD_WALL_DIST
  int AddBlock(const agx_block_geom &geom, const std::vector<agx_bc_surface> &surfs) {
    int id = -1;
    Check(AGX_SYM(block_create)(ctx_, &geom, &id), "hotPath::AddBlock");
    if (id + 1 > numBlocks_) numBlocks_ = id + 1;
    Check(AGX_SYM(block_set_bcs)(ctx_, id, static_cast<int>(surfs.size()), surfs.data()),
          "hotPath::AddBlock (boundary conditions)");
    return id;
  }
  int AddConnection(const agx_connection &conn) {
    int id = -1;
    Check(AGX_SYM(conn_create)(ctx_, &conn, &id), "hotPath::AddConnection");
    return id;
  }
  // multi-rank runs: the transport that stands where the reference has
  // MPI_Sendrecv / MPI_Reduce (multiArray3d.hpp:830-866, main.cpp:254-264).  With
  // one installed, Iterate exchanges the ghost slabs of connections to other ranks
  // itself and returns norms already reduced over the ranks.
  void SetExchange(const agx_exchange &ex) {
    Check(AGX_SYM(set_exchange)(ctx_, &ex), "hotPath::SetExchange");
  }
  // the library's own RCCL transport; id128 from RcclUniqueId() on one rank,
  // handed to the others by the host (MPI_Bcast)
  static void RcclUniqueId(void *id128) {
    Check(AGX_SYM(rccl_unique_id)(id128), "hotPath::RcclUniqueId");
  }
  void UseRccl(const void *id128, int numRanks, int rank) {
    Check(AGX_SYM(rccl_exchange_create)(ctx_, id128, numRanks, rank), "hotPath::UseRccl");
  }
  void Finalize() { Check(AGX_SYM(setup_finalize)(ctx_), "hotPath::Finalize"); }
  void UploadState(int block, const double *stateAos) {
    Check(AGX_SYM(state_upload)(ctx_, block, stateAos), "hotPath::UploadState");
  }
  void Download(int block, int field, double *aos) const {
    Check(AGX_SYM(field_download)(ctx_, block, field, aos), "hotPath::Download");
  }

  // WriteFunFile (output.cpp:209-437): the block's payload of a function file -- the
  // listed variables (AGX_OUT_*), physical cells, variable by variable, dimensional --
  // formed on the device; what comes back is what the caller writes to the file
  void OutputPack(int block, const std::vector<int32_t> &vars, double *out) const {
    Check(AGX_SYM(output_pack)(ctx_, block, static_cast<int>(vars.size()), vars.data(), out),
          "hotPath::OutputPack");
  }
  // WriteWallFun (output.cpp:472-571): the block's payload of the wall function file -- the
  // listed variables (AGX_WALL_*), variable by variable, within each the block's viscousWall
  // surfaces in the order SetBCs got them, within a surface its faces i fastest, then j, then
  // k; `out` holds vars.size() * (faces of all its wall surfaces) values
  void WallPack(int block, const std::vector<int32_t> &vars, double *out) const {
    Check(AGX_SYM(output_pack)(ctx_, block, static_cast<int>(vars.size()), vars.data(), out),
          "hotPath::WallPack");
  }
  // No counterpart in output.cpp: the integrated loads of the block's load surfaces -- its
  // viscousWall and slipWall surfaces in the order SetBCs got them -- summed on the device:
  // the listed variables (AGX_LOAD_*: area, area vector, pressure and viscous force, heat
  // load, pressure and viscous moment about the origin), variable by variable, one value per
  // surface, dimensional; `out` holds vars.size() * (load surfaces) values.  The normal points
  // into the fluid, so these are the loads ON the wall (see the header); the moment ids need a
  // block built from its nodes.  A moment about r_ref is M - r_ref x F of the same call
  void SurfaceLoads(int block, const std::vector<int32_t> &vars, double *out) const {
    Check(AGX_SYM(output_pack)(ctx_, block, static_cast<int>(vars.size()), vars.data(), out),
          "hotPath::SurfaceLoads");
  }
  // No counterpart in output.cpp: what crosses the block's flux surfaces -- every surface
  // SetBCs got, in that order, of every BC type, but the connections to other ranks -- summed
  // on the device from the face fluxes the residual pass takes: the listed variables
  // (AGX_FLUX_AREA, AGX_FLUX_INVISCID + e, AGX_FLUX_VISCOUS + e), variable by variable, one
  // value per surface, SI, positive out of the block; `out` holds vars.size() * (flux surfaces)
  // values.  A ghost-refilling read: refused between agx_phase_bc_faces and agx_phase_residual
  void SurfaceFluxes(int block, const std::vector<int32_t> &vars, double *out) const {
    Check(AGX_SYM(output_pack)(ctx_, block, static_cast<int>(vars.size()), vars.data(), out),
          "hotPath::SurfaceFluxes");
  }
  // ... and the block's balance over its physical cells (AGX_BUDGET_VOLUME, AGX_BUDGET_TOTAL +
  // e, AGX_BUDGET_RESIDUAL + e), one value per id; legal at every position.  Right after a
  // residual, BUDGET_RESIDUAL_e is the sum over the surfaces of FLUX_INVISCID_e +
  // FLUX_VISCOUS_e (e < 5); after an update the residual belongs to the state before it
  void BlockBudget(int block, const std::vector<int32_t> &vars, double *out) const {
    Check(AGX_SYM(output_pack)(ctx_, block, static_cast<int>(vars.size()), vars.data(), out),
          "hotPath::BlockBudget");
  }
  // WriteNodeFun (output.cpp:452-469): the block's payload of the nodal function file -- the
  // listed variables by their cell ids (AGX_OUT_*; AGX_NODE_BASE is added here), converted to
  // the (nk+1)(nj+1)(ni+1) nodes on the device (procBlock::CellToNode), variable by variable,
  // i fastest, dimensional; `out` holds vars.size() * nodes values.  viscosityRatio,
  // turbulentViscosity, f1, f2 are refused in the rans libraries (see the header)
  void OutputPackNodes(int block, const std::vector<int32_t> &vars, double *out) const {
    std::vector<int32_t> ids(vars);
    for (auto &v : ids) v += AGX_NODE_BASE;
    Check(AGX_SYM(output_pack)(ctx_, block, static_cast<int>(ids.size()), ids.data(), out),
          "hotPath::OutputPackNodes");
  }
  // Time statistics (no counterpart in the reference; see AGX_STAT_BASE in the C header):
  // running means and second central moments per cell and per viscousWall face, kept on the
  // device.  The time loop calls SampleStatistics after mgSolution::Iterate has converged a
  // time step; the weight is usually the step's dt.  Every block AddBlock returned is sampled,
  // one after the other: call it between time steps, where every block is legal (a block with
  // viscousWall faces refuses between agx_phase_bc_faces and agx_phase_residual, and the
  // blocks before it would have been sampled already)
  void SampleStatistics(double weight) {
    for (int b = 0; b < numBlocks_; ++b)
      Check(AGX_SYM(field_upload)(ctx_, b, AGX_FIELD_STAT_SAMPLE, &weight),
            "hotPath::SampleStatistics");
  }
  // discards the statistics of every block; the next sample starts anew
  void ResetStatistics() { SampleStatistics(0.0); }
  // the listed statistics of the block's cells (AGX_STAT_BASE + n), laid out like OutputPack's
  // payload, and of its wall faces (AGX_WSTAT_BASE + n), laid out like WallPack's; dimensional
  void Statistics(int block, const std::vector<int32_t> &ids, double *out) const {
    Check(AGX_SYM(output_pack)(ctx_, block, static_cast<int>(ids.size()), ids.data(), out),
          "hotPath::Statistics");
  }
  void WallStatistics(int block, const std::vector<int32_t> &ids, double *out) const {
    Check(AGX_SYM(output_pack)(ctx_, block, static_cast<int>(ids.size()), ids.data(), out),
          "hotPath::WallStatistics");
  }
  // the id of statistics variable n (0 ... 20 in the order of AGX_STAT_BASE, 21 the bin's
  // volume) collapsed along the index directions of mask (bit 0 = i, 1 = j, 2 = k)
  static int32_t CollapsedStatisticId(int mask, int n) { return AGX_CSTAT_BASE + 32 * mask + n; }
  // the listed statistics (n as above) of the block's cells pooled, volume weighted, over the
  // directions of mask (AGX_CSTAT_BASE): out[v * nbin + bin], the bins over the remaining
  // directions, i fastest; dimensional.  Reads the accumulators and the volumes only
  void CollapsedStatistics(int block, int mask, const std::vector<int32_t> &ids,
                           double *out) const {
    std::vector<int32_t> full(ids);
    for (auto &v : full) v = CollapsedStatisticId(mask, v);
    Check(AGX_SYM(output_pack)(ctx_, block, static_cast<int>(full.size()), full.data(), out),
          "hotPath::CollapsedStatistics");
  }
  // the block's raw accumulators (AGX_FIELD_STAT_ACCUM: 4 header values, the cell planes, the
  // wall rows; the caller sizes `payload` as the C header states) for a checkpoint, and back
  void StatisticsPayload(int block, double *payload) const {
    Check(AGX_SYM(field_download)(ctx_, block, AGX_FIELD_STAT_ACCUM, payload),
          "hotPath::StatisticsPayload");
  }
  void SetStatisticsPayload(int block, const double *payload) {
    Check(AGX_SYM(field_upload)(ctx_, block, AGX_FIELD_STAT_ACCUM, payload),
          "hotPath::SetStatisticsPayload");
  }
  // Time series (no counterpart in the reference; see AGX_FIELD_SERIES_PLAN in the C header):
  // chosen variables at chosen cells or wall faces, one row per sample, recorded on the
  // device.  SetSeriesPlan once per block ({kind, P, V, capacity, ids, points} as doubles);
  // the time loop calls SampleSeries after mgSolution::Iterate has converged a time step --
  // one kernel per planned block, no synchronisation, no copy -- and every `capacity` steps
  // at the latest SeriesRows (which synchronises) and DropSeriesRows.  Like SampleStatistics
  // it goes block by block: call it between time steps, where every plan is legal.
  void SetSeriesPlan(int block, const double *plan) {
    Check(AGX_SYM(field_upload)(ctx_, block, AGX_FIELD_SERIES_PLAN, plan),
          "hotPath::SetSeriesPlan");
    if (block >= static_cast<int>(seriesPlanned_.size())) seriesPlanned_.resize(block + 1, false);
    seriesPlanned_[block] = plan[1] != 0.0;
  }
  void SampleSeries(double t) {
    for (int b = 0; b < static_cast<int>(seriesPlanned_.size()); ++b)
      if (seriesPlanned_[b])
        Check(AGX_SYM(field_upload)(ctx_, b, AGX_FIELD_SERIES_SAMPLE, &t),
              "hotPath::SampleSeries");
  }
  // {P, V, rows, capacity}, then the rows {t, V P values} oldest first; `rows` holds
  // 4 + capacity (1 + V P) doubles
  void SeriesRows(int block, double *rows) const {
    Check(AGX_SYM(field_download)(ctx_, block, AGX_FIELD_SERIES_ROWS, rows),
          "hotPath::SeriesRows");
  }
  void DropSeriesRows(int block, int64_t n) {
    const double count = static_cast<double>(n);
    Check(AGX_SYM(field_upload)(ctx_, block, AGX_FIELD_SERIES_ROWS, &count),
          "hotPath::DropSeriesRows");
  }
  // the physical cell of the block nearest to each of numPts points (x, y, z in the units of
  // center_): where[numPts][4] = i, j, k, squared distance; the lowest linear cell index among
  // equally near ones
  void LocateCells(int block, int64_t numPts, const double *points, double *where) {
    std::vector<double> payload(1 + 3 * static_cast<size_t>(numPts));
    payload[0] = static_cast<double>(numPts);
    std::copy(points, points + 3 * numPts, payload.begin() + 1);
    Check(AGX_SYM(field_upload)(ctx_, block, AGX_FIELD_SERIES_LOCATE, payload.data()),
          "hotPath::LocateCells");
    Check(AGX_SYM(field_download)(ctx_, block, AGX_FIELD_SERIES_LOCATE, where),
          "hotPath::LocateCells");
  }
  // Spectra along a homogeneous index direction (no counterpart in the reference; see
  // AGX_FIELD_SPECTRA_PLAN in the C header).  SetSpectraPlan once per block ({along, over,
  // nvar, npair, ids, pairs} as doubles; nvar == 0 frees the block's spectra); the time loop
  // calls SampleSpectra(dt) at the place of SampleStatistics -- two kernels per planned block,
  // no synchronisation, no copy.  Spectra hands out values[spectrum][bin][mode], dimensional;
  // SpectraPayload / SetSpectraPayload carry an average into another run
  // (8 + nvar + 2 npair + (nvar + npair) bins modes doubles).
  void SetSpectraPlan(int block, const double *plan) {
    Check(AGX_SYM(field_upload)(ctx_, block, AGX_FIELD_SPECTRA_PLAN, plan),
          "hotPath::SetSpectraPlan");
    if (block >= static_cast<int>(spectraPlanned_.size()))
      spectraPlanned_.resize(block + 1, false);
    spectraPlanned_[block] = plan[2] != 0.0;
  }
  void SampleSpectra(double w) {
    for (int b = 0; b < static_cast<int>(spectraPlanned_.size()); ++b)
      if (spectraPlanned_[b])
        Check(AGX_SYM(field_upload)(ctx_, b, AGX_FIELD_SPECTRA_SAMPLE, &w),
              "hotPath::SampleSpectra");
  }
  void Spectra(int block, double *values) const {
    Check(AGX_SYM(field_download)(ctx_, block, AGX_FIELD_SPECTRA_VALUES, values),
          "hotPath::Spectra");
  }
  void SpectraPayload(int block, double *payload) const {
    Check(AGX_SYM(field_download)(ctx_, block, AGX_FIELD_SPECTRA_ACCUM, payload),
          "hotPath::SpectraPayload");
  }
  void SetSpectraPayload(int block, const double *payload) {
    Check(AGX_SYM(field_upload)(ctx_, block, AGX_FIELD_SPECTRA_ACCUM, payload),
          "hotPath::SetSpectraPayload");
  }
  void ClearSpectra() {
    const double none[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < static_cast<int>(spectraPlanned_.size()); ++b)
      if (spectraPlanned_[b]) SetSpectraPlan(b, none);
  }
  // WriteRestart (output.cpp:651-752): the block's payload, numEqns + 1 values per cell;
  // secondSolution: consVarsNm1 (multilevel time integration)
  void RestartPack(int block, bool secondSolution, double *out) const {
    Check(AGX_SYM(restart_pack)(ctx_, block, secondSolution ? 1 : 0, out),
          "hotPath::RestartPack");
  }
  // procBlock::InitializeStates (procBlock.cpp:280-355) on the device, after Finalize(): the
  // non-file branch from the nondimensional primitive of NondimensionalInitialize ...
  void FillState(int block, const double *prim) {
    Check(AGX_SYM(state_fill)(ctx_, block, prim), "hotPath::FillState");
  }
  // ... and the file branch from the cloud of CalcTreeFromCloud (points[numPts][3],
  // states[numPts][numEqns], nondimensional); returns the reference's maxDist.  Among
  // points at equal distance the lowest index wins
  double StateFromCloud(int block, int64_t numPts, const double *points, const double *states) {
    double maxDist = 0.0;
    Check(AGX_SYM(state_from_cloud)(ctx_, block, numPts, points, states, &maxDist),
          "hotPath::StateFromCloud");
    return maxDist;
  }
  // ReadSolFromRestart / ReadSolNm1FromRestart (output.cpp:1177-1305): the payload RestartPack
  // hands out, nondimensionalised on the device into the state or (secondSolution) consVarsNm1
  void RestartUnpack(int block, bool secondSolution, const double *in) {
    Check(AGX_SYM(restart_unpack)(ctx_, block, secondSolution ? 1 : 0, in),
          "hotPath::RestartUnpack");
  }

  // mgSolution::StoreOldSolution: consVarsN <- cons(state) (and N-1 on the first
  // step of a multilevel-in-time scheme)
  void StoreOldSolution(bool alsoNm1) {
    Check(AGX_SYM(store_time_n)(ctx_, alsoNm1 ? 1 : 0), "hotPath::StoreOldSolution");
  }

  // mgSolution::Iterate for one rank: boundary conditions, residual, time step,
  // explicit update or implicit solve.  residL2 is accumulated into, residLinf
  // only replaced by a larger value; returns sum(matrix residual^2) / size, which
  // the caller reduces over ranks and square-roots (main.cpp:271).
  double Iterate(int mm, double cfl, residual &residL2, resid &residLinf) {
    agx_linf linf;
    linf.linf = residLinf.Linf();
    linf.block = residLinf.Block();
    linf.i = residLinf.ILoc();
    linf.j = residLinf.JLoc();
    linf.k = residLinf.KLoc();
    linf.eqn = residLinf.Eqn();
    linf.pad_ = 0;
    double matrixResid = 0.0;
    Check(AGX_SYM(iterate)(ctx_, mm, cfl, residL2.data(), &linf, &matrixResid),
          "hotPath::Iterate");
    residLinf.UpdateMax(linf.linf, linf.block, linf.i, linf.j, linf.k, linf.eqn);
    return matrixResid;
  }

  friend class multigrid;
};

// mgSolution with more than one grid level (mgSolution.cpp:128-262) on one rank: a hotPath
// per gridLevel (finest first; every level configured, given its coarsened blocks and
// surfaces -- procBlock::GetCoarseMeshAndBCs -- and finalized by the caller) and, per level
// but the coarsest and per block, the arrays gridLevel::Coarsen builds: toCoarse_ (int32
// triples), volWeightFactor_, prolongCoeffs_ (7 doubles), all per physical fine cell in
// k-j-i order.  The cycle is the reference's; what crosses between two levels runs in the
// library (agx_mg_*).  Runs of more than one rank: every level's hotPath gets the rank's
// blocks of that level and its own SetExchange / UseRccl; the levels' connections to other
// ranks then go through agx_halo_exchange like the finest one's (restriction and prolongation
// never leave a block), and the norms Iterate returns are this rank's.
class multigrid {
  struct transfer {
    std::vector<int32_t> toCoarse;
    std::vector<double> volFac, coeffs;
  };
  std::vector<std::unique_ptr<hotPath>> solution_;
  std::vector<std::vector<transfer>> transfer_;   // [fine level][block]
  int mgCycleIndex_ = 1;                          // V: 1, W: 2
  int matrixSweeps_ = 1;
  bool lusgs_ = false;
  bool swapGradients_ = false;                    // block-matrix solver, viscous
  bool swapTurbVars_ = false;                     // rans

  static void Check(int rc, const char *what) { hotPath::Check(rc, what); }
  AGX_CAT(AGX_SYMBOL_PREFIX, ctx) *Ctx(int ll) const { return solution_[ll]->ctx_; }

  // gridLevel::GetBoundaryConditions, CalcResidual, CalcTimeStep
  void BoundaryAndResidual(int ll, int mm, double cfl) {
    Check(AGX_SYM(phase_bc_faces)(Ctx(ll)), "multigrid (phase_bc_faces)");
    Check(AGX_SYM(halo_exchange)(Ctx(ll), AGX_HALO_STATE), "multigrid (halo_exchange)");
    Check(AGX_SYM(phase_bc_edges)(Ctx(ll)), "multigrid (phase_bc_edges)");
    Check(AGX_SYM(phase_residual)(Ctx(ll), mm, cfl), "multigrid (phase_residual)");
    // CalcResidual ends with SwapEddyViscAndGradients and, for rans, SwapTurbVars
    // (gridLevel.cpp:386-392), on every level: Restriction calls it on the coarse one (:559-563)
    if (swapGradients_) {
      Check(AGX_SYM(halo_exchange)(Ctx(ll), AGX_HALO_VELGRAD_A), "multigrid (SwapEddyViscAndGradients)");
      Check(AGX_SYM(halo_exchange)(Ctx(ll), AGX_HALO_VELGRAD_B), "multigrid (SwapEddyViscAndGradients)");
    }
    if (swapTurbVars_) Check(AGX_SYM(halo_exchange)(Ctx(ll), AGX_HALO_TURB), "multigrid (SwapTurbVars)");
  }

 public:
  multigrid(int cycleIndex, const agx_config &cfg)
      : mgCycleIndex_(cycleIndex), matrixSweeps_(cfg.matrix_sweeps),
        lusgs_(cfg.matrix_solver == AGX_SOLVER_LUSGS || cfg.matrix_solver == AGX_SOLVER_BLUSGS),
        swapGradients_((cfg.matrix_solver == AGX_SOLVER_BLUSGS ||
                        cfg.matrix_solver == AGX_SOLVER_BDPLUR) && cfg.is_viscous),
        swapTurbVars_(cfg.n_eq == 7) {}
  int NumGridLevels() const { return static_cast<int>(solution_.size()); }
  hotPath &Level(int ll) { return *solution_[ll]; }
  // levels are added finest first
  void AddLevel(std::unique_ptr<hotPath> level) {
    solution_.push_back(std::move(level));
    transfer_.emplace_back();
  }
  // the transfer arrays of block `blk` of level `fl` towards level fl + 1 (blocks in order)
  void AddTransfer(int fl, std::vector<int32_t> toCoarse, std::vector<double> volFac,
                   std::vector<double> coeffs) {
    transfer_[fl].push_back(transfer{std::move(toCoarse), std::move(volFac), std::move(coeffs)});
  }

  // mgSolution::StoreOldSolution (:103-114): every level
  void StoreOldSolution(bool alsoNm1) {
    for (auto &sol : solution_) sol->StoreOldSolution(alsoNm1);
  }
  // linearSolver::Relax (linearSolver.cpp:430-470, :509-536); returns sum(r^2) / size
  double Relax(int ll, int sweeps) {
    for (int ii = 0; ii < sweeps; ++ii) {
      Check(AGX_SYM(halo_exchange)(Ctx(ll), AGX_HALO_UPDATE), "multigrid::Relax (SwapUpdate)");
      Check(AGX_SYM(phase_relax_forward)(Ctx(ll), ii), "multigrid::Relax");
      if (lusgs_) {
        Check(AGX_SYM(halo_exchange)(Ctx(ll), AGX_HALO_UPDATE), "multigrid::Relax (SwapUpdate)");
        Check(AGX_SYM(phase_relax_backward)(Ctx(ll), ii), "multigrid::Relax");
      }
    }
    Check(AGX_SYM(halo_exchange)(Ctx(ll), AGX_HALO_UPDATE), "multigrid::Relax (SwapUpdate)");
    double l2 = 0.0;
    Check(AGX_SYM(mg_matrix_residual)(Ctx(ll), &l2), "multigrid::Relax (Residual)");
    return l2;
  }
  // gridLevel::Restriction (gridLevel.cpp:538-595)
  void Restriction(int fi, int mm, double cfl) {
    const int ci = fi + 1;
    const auto &tr = transfer_[fi];
    for (size_t bb = 0; bb < tr.size(); ++bb) {
      Check(AGX_SYM(mg_restrict)(Ctx(fi), Ctx(ci), static_cast<int>(bb), AGX_MG_STATE,
                                 tr[bb].toCoarse.data(), tr[bb].volFac.data()),
            "multigrid::Restriction (state)");
      if (mm == 0) solution_[ci]->StoreOldSolution(false);
    }
    BoundaryAndResidual(ci, mm, cfl);
    Check(AGX_SYM(mg_invert_diagonal)(Ctx(ci)), "multigrid::Restriction (InvertDiagonal)");
    for (size_t bb = 0; bb < tr.size(); ++bb)
      Check(AGX_SYM(mg_restrict)(Ctx(fi), Ctx(ci), static_cast<int>(bb), AGX_MG_UPDATE,
                                 tr[bb].toCoarse.data(), tr[bb].volFac.data()),
            "multigrid::Restriction (update)");
    Check(AGX_SYM(halo_exchange)(Ctx(ci), AGX_HALO_UPDATE), "multigrid::Restriction (SwapUpdate)");
    for (size_t bb = 0; bb < tr.size(); ++bb)
      Check(AGX_SYM(mg_restrict)(Ctx(fi), Ctx(ci), static_cast<int>(bb), AGX_MG_FORCING,
                                 tr[bb].toCoarse.data(), nullptr),
            "multigrid::Restriction (forcing)");
  }
  // SubtractFromUpdate + Prolongation (mgSolution.cpp:189-192)
  void Prolongation(int ci) {
    const auto &tr = transfer_[ci - 1];
    for (size_t bb = 0; bb < tr.size(); ++bb)
      Check(AGX_SYM(mg_prolong)(Ctx(ci), Ctx(ci - 1), static_cast<int>(bb),
                                tr[bb].toCoarse.data(), tr[bb].coeffs.data()),
            "multigrid::Prolongation");
  }
  // mgSolution::CycleAtLevel (:160-205)
  double CycleAtLevel(int fl, int mm, double cfl) {
    if (fl == NumGridLevels() - 1) return Relax(fl, matrixSweeps_);   // recursive base case
    const int sweeps = std::max(matrixSweeps_ / 2, 1);
    Relax(fl, sweeps);
    const int cl = fl + 1;
    Restriction(fl, mm, cfl);
    Check(AGX_SYM(mg_save_update)(Ctx(cl)), "multigrid::CycleAtLevel (coarseDu)");
    for (int ii = 0; ii < mgCycleIndex_; ++ii) CycleAtLevel(cl, mm, cfl);
    Prolongation(cl);
    return Relax(fl, sweeps);
  }
  // mgSolution::Iterate / ImplicitUpdate (:207-262); residL2 accumulated into, residLinf only
  // replaced by a larger value, the return value as hotPath::Iterate
  double Iterate(int mm, double cfl, residual &residL2, resid &residLinf) {
    BoundaryAndResidual(0, mm, cfl);
    Check(AGX_SYM(phase_implicit_begin)(Ctx(0)), "multigrid::Iterate (InvertDiagonal)");
    const double matrixResid = CycleAtLevel(0, mm, cfl);
    agx_linf linf;
    linf.linf = residLinf.Linf();
    linf.block = residLinf.Block();
    linf.i = residLinf.ILoc();
    linf.j = residLinf.JLoc();
    linf.k = residLinf.KLoc();
    linf.eqn = residLinf.Eqn();
    linf.pad_ = 0;
    Check(AGX_SYM(phase_implicit_update)(Ctx(0), mm, residL2.data(), &linf),
          "multigrid::Iterate (UpdateBlocks)");
    residLinf.UpdateMax(linf.linf, linf.block, linf.i, linf.j, linf.k, linf.eqn);
    for (int ll = 1; ll < NumGridLevels(); ++ll)      // ResetDiagonal on every level
      Check(AGX_SYM(mg_reset_diagonal)(Ctx(ll)), "multigrid::Iterate (ResetDiagonal)");
    return matrixResid;
  }
};

}  // namespace aither_gfx950
#endif
