/* aither_gfx950.h -- C-ABI of libaither_gfx950.so (5 equations: euler,
 * navierStokes) and of libaither_gfx950_rans.so (7 equations: rans with k-omega
 * SST 2003, SST-DES or k-omega Wilcox 2006, low-Re walls or wall functions; the same sources built with -DAGX_NEQ=7, the same entry points).
 *
 * MI355X (gfx950) implementation of AITHER's per-iteration hot path:
 * ghost-cell fill, face reconstruction, inviscid/viscous fluxes, time step,
 * explicit update and the LU-SGS / DPLUR implicit sweeps.
 *
 * The library stands behind the calls that the reference's
 *   mgSolution::Iterate            (src/mgSolution.cpp:246-269)
 * makes on its finest gridLevel, plus the three data-movement points around
 * it (setup after main.cpp:163-203, StoreOldSolution main.cpp:239, and
 * GetFinestGridLevel main.cpp:282).  All arrays crossing this boundary use the
 * reference's own host layout (multiArray3d, include/multiArray3d.hpp:104-113):
 * AoS, block-size doubles per cell, i fastest, ghost-inclusive dimensions
 * (n + 2*ng).  The library owns device-resident SoA copies and never aliases
 * host memory.
 *
 * Error convention: every entry point returns 0 on success, non-zero on
 * failure; agx_last_error() returns a message (the reference prints to cerr
 * and calls exit(EXIT_FAILURE); the adapter in INTEGRATION.md keeps that).
 * Not thread-safe: one context per process per device (the reference is
 * single-threaded per MPI rank).
 */
#ifndef AITHER_GFX950_H
#define AITHER_GFX950_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The libraries are built with -fvisibility=hidden: only the agx_* entry points below are
 * exported.  libaither_gfx950.so (5 equations) and libaither_gfx950_rans.so (7 equations)
 * are the SAME sources compiled for two state layouts, so their internals must never bind
 * to each other; with the internals hidden the two can share a process (each dlopen'ed
 * RTLD_LOCAL and called through dlsym, since both export the same agx_* names). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* ---- enumerations (resolved once from the reference's std::string input
 *      options, include/input.hpp:48-291) -------------------------------- */
enum { AGX_RECON_CONSTANT = 0, AGX_RECON_MUSCL = 1, AGX_RECON_WENO = 2,
       AGX_RECON_WENOZ = 3 };                 /* input.cpp:276-303 */
enum { AGX_LIMITER_NONE = 0, AGX_LIMITER_VANALBADA = 1,
       AGX_LIMITER_MINMOD = 2 };              /* limiter.cpp:24-54 */
enum { AGX_FLUX_ROE = 0, AGX_FLUX_AUSM = 1 }; /* inviscidFlux.hpp:484-507 */
enum { AGX_TIME_EXPLICIT_EULER = 0, AGX_TIME_RK4 = 1,
       AGX_TIME_IMPLICIT_EULER = 2, AGX_TIME_CRANK_NICHOLSON = 3,
       AGX_TIME_BDF2 = 4 };                   /* input.cpp:259-275 */
enum { AGX_SOLVER_LUSGS = 0, AGX_SOLVER_DPLUR = 1,
       AGX_SOLVER_BLUSGS = 2, AGX_SOLVER_BDPLUR = 3 }; /* input.cpp:843-858 */
enum { AGX_EQN_EULER = 0, AGX_EQN_NAVIER_STOKES = 1,
       AGX_EQN_RANS = 2,
       AGX_EQN_LES = 3 /* largeEddySimulation (input.cpp:653-663, :694-709, :751): five
                          equations, IsTurbulent() true, IsRANS() false; turbulence_model wale
                          and nothing else (:965-979).  The 5-equation libraries, explicit time
                          integration (implicit LES is refused by name) */
     };                                       /* input::equationSet_, input.cpp:1033-1060 */
enum { AGX_JACOBIAN_RUSANOV = 0,
       AGX_JACOBIAN_APPROX_ROE = 1 };         /* input::InvFluxJac, fluxJacobian.cpp:196-238 */
enum { AGX_VISC_RECON_CENTRAL = 0,
       AGX_VISC_RECON_CENTRAL_4TH = 1 };      /* reconstruction.hpp:315-379 */
enum { AGX_TURB_NONE = 0, AGX_TURB_SST2003 = 1, AGX_TURB_KW_WILCOX2006 = 2,
       AGX_TURB_SST_DES = 3,
       AGX_TURB_WALE = 4 /* with AGX_EQN_LES only (input.cpp:965-979).  turbWale::EddyVisc
                            turbulence.cpp:967-996, Cw = 0.544, evaluated at every face that is
                            not a wall-law face (EddyViscAndBlending turbulence.hpp:685-695,
                            procBlock.cpp:1357-1365); enters tau and the conductivity
                            (viscousFlux.cpp:58-211, Prt = 0.9 turbulence.hpp:70), y+ at low-Re
                            walls (procBlock.cpp:1372-1376), the viscous spectral radius
                            (spectralRadius.hpp:94-123) and eddyViscosity_ (:1401-1402) */
     };                                       /* turbulence.hpp */

/* boundary condition types, ghostStates.cpp:62-689 */
enum { AGX_BC_SLIPWALL = 0, AGX_BC_VISCOUSWALL = 1, AGX_BC_CHARACTERISTIC = 2,
       AGX_BC_INLET = 3, AGX_BC_SUPERSONIC_INFLOW = 4,
       AGX_BC_SUPERSONIC_OUTFLOW = 5, AGX_BC_STAGNATION_INLET = 6,
       AGX_BC_PRESSURE_OUTLET = 7, AGX_BC_INTERBLOCK = 8,
       AGX_BC_PERIODIC = 9 };

/* fields that can be downloaded (procBlock members, include/procBlock.hpp:60-110) */
enum { AGX_FIELD_STATE = 0,      /* state_      nEq, with ghosts           */
       AGX_FIELD_RESIDUAL = 1,   /* residual_   nEq, no ghosts             */
       AGX_FIELD_DT = 2,         /* dt_         1,   no ghosts             */
       AGX_FIELD_SPEC_RADIUS = 3,/* specRadius_ 1,   no ghosts (flow part) */
       AGX_FIELD_CONS_N = 4,     /* consVarsN_  nEq, no ghosts             */
       AGX_FIELD_UPDATE = 5,     /* linearSolver x_ nEq, with ghosts       */
       AGX_FIELD_DIAGONAL = 6,   /* linearSolver a_ (scalar) 1, no ghosts;
                                  * refused by name on the diagonal-ordered LU-SGS
                                  * path, which keeps a_ only inside its sweep arrays */
       AGX_FIELD_TEMPERATURE = 7,/* temperature_ 1,  with ghosts           */
       AGX_FIELD_VISCOSITY = 8,  /* viscosity_  1,   with ghosts           */
       AGX_FIELD_CONS_NM1 = 9,   /* consVarsNm1_ nEq, no ghosts            */
       /* cell-centre gradients (velocityGrad_, temperatureGrad_, densityGrad_,
        * pressureGrad_; procBlock.cpp:1397-1449, :5950-5954): the mean of the six
        * Green-Gauss face gradients of the cell, formed ON DEMAND from the state
        * the device holds (they are not kept between iterations) with the ghost
        * cells the next residual would see: the inviscid fill of that state, then
        * the viscous-wall fill (ghost cells of connections to other ranks as last
        * exchanged); no ghosts.
        * VEL_GRAD: 9 per cell, [3 r + c] = d(velocity c)/d(x_r) (tensor.hpp) */
       AGX_FIELD_VEL_GRAD = 10, AGX_FIELD_TEMP_GRAD = 11,
       AGX_FIELD_DENS_GRAD = 12, AGX_FIELD_PRESS_GRAD = 13,
       /* the geometry the device holds, in the host layout agx_block_geom documents, ghost
        * cells included (download only; agx_field_upload refuses them): what a node-built
        * block was given by the library, or what an array-built one was created from */
       AGX_FIELD_VOLUME = 14,    /* vol_        1                               */
       AGX_FIELD_CENTER = 15,    /* center_     3                               */
       AGX_FIELD_FAREA_I = 16, AGX_FIELD_FAREA_J = 17, AGX_FIELD_FAREA_K = 18, /* 4 */
       AGX_FIELD_WIDTH_I = 19, AGX_FIELD_WIDTH_J = 20, AGX_FIELD_WIDTH_K = 21, /* 1 */
       AGX_FIELD_WALL_DIST = 22, /* wallDist_   1                               */
       /* running time statistics of the block ("time statistics" at AGX_STAT_BASE).
        * STAT_SAMPLE: upload only, ONE double w.  w > 0 and finite: the block's current state
        * enters its statistics with weight w (the accumulators are allocated on the first
        * sample).  w == 0: the block's statistics are discarded and their memory freed; the
        * next sample starts anew.  Negative or non-finite w, and a download, are refused by
        * name.  A sample writes nothing the solver reads: it is a READ of the run ("reads
        * between phases" at agx_field_download) and leaves the run bit-identical.  On a viscous
        * block with a viscousWall surface it is a ghost-refilling read like the wall
        * variables, refused between agx_phase_bc_faces and agx_phase_residual; on every other
        * block it reads physical cells only and is legal at every position.
        * STAT_ACCUM: download and upload, the block's raw (nondimensional) accumulators, for
        * checkpointing an average:
        *   4 doubles {cell planes P, wall values per face V, W (sum of weights), samples},
        *   P planes [nk][nj][ni] (i fastest, no ghost cells): the means, then the co-moments C,
        *   V rows of one value per wall face (the order of the wall payload),
        * 4 + P ni nj nk + V faces doubles in all.  P = 18 (5 equations), 19
        * (largeEddySimulation), 21 (7 equations); V = 18 on a viscous block with a viscousWall
        * surface, else 0.  Upload replaces the block's statistics (allocating if need be) and
        * is refused by name when P or V are not this library's and context's, or W or the
        * sample count is negative or non-finite; download before the first sample is refused
        * by name. */
       AGX_FIELD_STAT_SAMPLE = 23, AGX_FIELD_STAT_ACCUM = 24,
       /* time series at chosen points of the block, recorded on the device: the signals of an
        * unsteady run (spectra, two-point correlations, shedding frequencies) beside its
        * averages.  All payloads are arrays of doubles; counts, ids and indices are integral
        * doubles, and a payload with a non-integral, negative, non-finite or out-of-range entry
        * is refused by name, the message saying which entry.  After agx_setup_finalize.
        * SERIES_PLAN: upload and download, the block's plan:
        *   {kind, P, V, capacity, V variable ids, P points}
        *   kind 0, cells: ids < AGX_OUT_COUNT; a point is three values i, j, k of a physical
        *     cell (4 + V + 3 P doubles);
        *   kind 1, wall faces: ids AGX_WALL_*; a point is one index into the block's wall
        *     payload, in the order agx_output_pack hands the wall variables out
        *     (4 + V + P doubles).
        * A plan holds one kind, as an agx_output_pack call holds one range.  An upload replaces
        * the block's plan, discards its rows and allocates capacity x V x P doubles on the
        * device; P == 0 discards the plan and frees the memory (V, capacity and what follows
        * are not read).  Refused by name: unknown ids; tke, sdr, f1, f2, their gradients and
        * residuals, and the wall's tke and sdr in the 5-equation libraries; viscosity in an
        * inviscid context; wall ids without a viscous context or on a block without a
        * viscousWall surface; V < 1, V > AGX_OUT_COUNT; capacity < 1.  A refused upload leaves
        * the plan and the rows as they were.  A download returns the payload as uploaded and is
        * refused by name when the block has no plan.
        * SERIES_SAMPLE: upload only, ONE finite double t.  Appends one row to the block's
        * record: t and the V x P values, variable-major [v * P + p], dimensional -- exactly
        * what agx_output_pack with the plan's ids would deliver at those points at that moment.
        * The call enqueues one kernel on the context's stream and returns: it does not
        * synchronise the stream, copies nothing to the host and allocates nothing.  A sample
        * is a READ of the run and leaves it bit-identical; its legality is that of the
        * agx_output_pack call with the same ids ("reads between phases" at
        * agx_field_download): a cell plan without gradient ids reads physical cells only and
        * is legal at every position; a cell plan with gradient ids and every wall plan refill
        * the ghost cells and are refused between agx_phase_bc_faces and agx_phase_residual;
        * a wall plan on wall-law surfaces is refused before the first residual.  Refused by
        * name as well: a full record (rows == capacity: collect the rows first -- nothing is
        * ever overwritten); a block without a plan; a wall plan whose block's surfaces were
        * set again (agx_block_set_bcs) since the plan's upload; a non-finite t; a download.
        * SERIES_ROWS: download {P, V, rows, capacity}, then `rows` rows of 1 + V P doubles
        * {t, values}, oldest first; the caller's buffer holds 4 + capacity (1 + V P) doubles.
        * The download synchronises and leaves the record as it is.  Upload of ONE double n,
        * 0 <= n <= rows: the oldest n rows are dropped.  The record is a ring: a long run
        * samples, collects and drops for ever in the memory of the plan's upload, the rows
        * recorded after a drop wrapping around.  Both are refused by name without a plan.
        * SERIES_LOCATE: upload {P, P triples x, y, z} (P >= 1, every coordinate finite and
        * at most 1e150 in magnitude) in the units of AGX_FIELD_CENTER: the library finds on
        * the device, for each point, the PHYSICAL cell of this block whose centre is nearest.
        * Download: P x {i, j, k, d2} of the last upload, refused by name before one.  Tie rule:
        * among cells at equal squared distance the lowest linear index (k nj + j) ni + i
        * wins.  d2 is dx dx + dy dy + dz dz of centre - point; the compiler may contract the
        * sum, so cells whose distances differ by a few units of 2^-53 relative are not decided
        * the way an uncontracted sum would (as agx_state_from_cloud).  Exhaustive, points x
        * cells.  Locate touches neither the plan nor the record. */
       AGX_FIELD_SERIES_PLAN = 25, AGX_FIELD_SERIES_SAMPLE = 26, AGX_FIELD_SERIES_ROWS = 27,
       AGX_FIELD_SERIES_LOCATE = 28,
       /* wavenumber spectra along a homogeneous index direction of the block, accumulated on
        * the device: E_uu(k), the co-spectrum of uv, and with them the two-point correlations
        * of an unsteady run.  Payloads are arrays of doubles, counts and ids integral doubles,
        * checked like those of the time series.  After agx_setup_finalize.
        * A line is one run of the N physical cells of the block along `along`.  Per line and
        * variable the mean mu is taken (serially, ascending) and SUBTRACTED, then
        *   X_m = sum_n (x_n - mu) exp(-2 pi i m n / N),  m = 1 ... N / 2,
        *   P_m = c_m |X_m|^2 / N^2,  C_ab,m = c_m Re(X_a,m conj X_b,m) / N^2,
        * c_m = 2 but 1 at m = N / 2 of an even N, and entry m = 0 is mu^2 (mu_a mu_b): the
        * entries of a line sum to its mean of x_a x_b.  The lines of a bin -- one position of
        * the directions that are neither `along` nor pooled -- pool with EQUAL weights (pooled
        * directions are homogeneous; cell volumes are not used), samples by the running mean
        * S += (w / W)(s - S).  No atomics, every order of summation fixed by the extents and
        * the plan: the same calls give the same bits; identical lines or samples give one
        * line's bits; doubling every weight changes no bit; a spectrum depends on its own
        * variables only, so a plan of a subset or in another order returns the same bits.
        * SPECTRA_PLAN: upload only,
        *   {along (0 i, 1 j, 2 k), over (mask of the pooled directions, bit 0 i, 1 j, 2 k),
        *    nvar, npair, nvar variable ids, npair pairs (a, b) of indices into the variables}
        * (4 + nvar + 2 npair doubles).  Variables: AGX_OUT_DENSITY, _VEL_X, _VEL_Y, _VEL_Z,
        * _PRESSURE, _TEMPERATURE, formed as the statistics form them.  The upload replaces the
        * block's plan, discards its accumulators and allocates; nvar == 0 frees everything
        * (nothing else is read).  Refused by name, the block left as it was: another variable,
        * a repeated one, nvar > 6, a pair index out of range, a pair of a variable with
        * itself, a pair repeated or given in both orders, over containing along, N < 2,
        * N > AGX_SPECTRA_MAX_N (what the line kernel's LDS holds).
        * SPECTRA_SAMPLE: upload only, ONE double w: one sample of the state the device holds
        * now, with weight w.  Two kernels on the context's stream; no synchronisation, no copy,
        * no allocation.  It reads physical cells only: a READ of the run that leaves it
        * bit-identical and is legal at every position of the phase API, seeing the state
        * agx_output_pack would return there.  w == 0 resets W, the sample count and the
        * accumulators and keeps the plan.  Refused: w negative or not finite.
        * SPECTRA_ACCUM: download and upload, for carrying an average into another run:
        *   the plan's payload, then {W, samples, nbin, nmode}, then the raw (nondimensional)
        *   S[spectrum][bin][mode]: 8 + nvar + 2 npair + (nvar + npair) nbin nmode doubles.
        * An upload is refused by name unless its plan, nbin and nmode are the block's, and when
        * W or the sample count is negative or not finite.
        * SPECTRA_VALUES: download only, out[s][bin][m], dimensional (times the product of the
        * two variables' output factors, like the second moments of AGX_STAT_BASE): s runs over
        * the variables in plan order, then the pairs; the bins over the remaining directions,
        * the lower index direction fastest; m = 0 ... N / 2.
        * SAMPLE, ACCUM and VALUES are refused by name on a block without a plan. */
       AGX_FIELD_SPECTRA_PLAN = 29, AGX_FIELD_SPECTRA_SAMPLE = 30, AGX_FIELD_SPECTRA_ACCUM = 31,
       AGX_FIELD_SPECTRA_VALUES = 32
};
/* the longest line of a spectra plan: twiddles, one line of six variables and their means in
 * the 80 KiB of LDS the line kernel declares */
#define AGX_SPECTRA_MAX_N 1024

/* variables of a function file, WriteFunFile (output.cpp:235-407): formed and
 * re-dimensionalised ON THE DEVICE by agx_output_pack, so an output step moves what the
 * file holds instead of the whole state (GetFinestGridLevel, main.cpp:282).  Gradients:
 * d/dx, d/dy, d/dz; VELGRAD in the reference's order ux vx wx uy vy wy uz vz wz
 * (tensor XX XY XZ YX ...).  The gradients are those of the state the device holds when
 * the call is made, with the ghost cells the next residual would see (AGX_FIELD_VEL_GRAD;
 * the reference writes the ones its last residual accumulated, procBlock.cpp:1397-1449,
 * i.e. of the state before the last update); eddy viscosity, f1, f2 and the residuals
 * are the last residual's, as in the reference. */
enum { AGX_OUT_DENSITY = 0, AGX_OUT_VEL_X, AGX_OUT_VEL_Y, AGX_OUT_VEL_Z, AGX_OUT_PRESSURE,
       AGX_OUT_MACH, AGX_OUT_SOS, AGX_OUT_DT, AGX_OUT_TEMPERATURE, AGX_OUT_ENERGY,
       AGX_OUT_ENTHALPY, AGX_OUT_CP, AGX_OUT_CV, AGX_OUT_RANK, AGX_OUT_GLOBAL_POSITION,
       AGX_OUT_VISCOSITY_RATIO, AGX_OUT_TURB_VISCOSITY, AGX_OUT_VISCOSITY, AGX_OUT_TKE,
       AGX_OUT_SDR, AGX_OUT_F1, AGX_OUT_F2, AGX_OUT_WALL_DISTANCE,
       AGX_OUT_VELGRAD = 23,      /* .. 31: nine entries                          */
       AGX_OUT_TEMPGRAD = 32,     /* .. 34                                        */
       AGX_OUT_DENSGRAD = 35, AGX_OUT_PRESSGRAD = 38,
       AGX_OUT_TKEGRAD = 41, AGX_OUT_OMEGAGRAD = 44,   /* rans library             */
       AGX_OUT_RESID = 47,        /* .. 53: mass, mom_x, mom_y, mom_z, energy, tke, sdr */
       AGX_OUT_COUNT = 54 };

/* variables of the wall function file, WriteWallFun (output.cpp:472-571): the wallData_ of
 * the block's viscousWall surfaces (wallVars, wallData.hpp:33-62), dimensional with the
 * factors of output.cpp:519-553.  A range of its own in agx_output_pack: a call asks for cell
 * variables (< AGX_OUT_COUNT) or for wall variables, never both.
 *   yplus              wallVars::yplus_             procBlock.cpp:1372-1375   output.cpp:519
 *   shearStress        |shearStress_|, TauNormal    utility.cpp:426-436       :521-524
 *   viscosityRatio     turbEddyVisc_ / (viscosity_ + EPS)                     :525-527
 *   heatFlux           (k + kt) grad T . n          viscousFlux.cpp:170-178   :528-530
 *   frictionVelocity   sqrt(|tau| / rho)            viscousFlux.cpp:187       :531-533
 *   density, pressure (PressureRT, wallData.cpp:140-144), temperature, viscosity,
 *   tke, sdr           the face state of CalcWallFlux                         :534-553
 * AGX_WALL_SHEAR_X/Y/Z are an extension: the components of shearStress_ with the factor of
 * shearStress (the reference writes the magnitude only; integrated forces need the vector).
 * As in the reference the vector is TauNormal on the face's area vector, which points in the
 * direction of increasing index on both sides of a block.
 * Timing.  Low-Re faces (every wall face of the 5-equation libraries; in the rans libraries the
 * faces of low-Re surfaces and those faces of a wall-law surface whose stored y+ < 10,
 * SwitchToLowRe): evaluated from the state the device holds when the call is made, with the
 * ghost cells the next residual would see, like the gradients above (the reference writes
 * what its last residual stored, procBlock.cpp:1367-1376, i.e. of the state before the last
 * update).  Wall-law faces: the wall data the last residual's viscous ghost fill stored, as
 * they are (like eddy viscosity, f1 and f2 of the cell variables). */
enum { AGX_WALL_YPLUS = 64, AGX_WALL_SHEAR_STRESS, AGX_WALL_VISCOSITY_RATIO, AGX_WALL_HEAT_FLUX,
       AGX_WALL_FRICTION_VELOCITY, AGX_WALL_DENSITY, AGX_WALL_PRESSURE, AGX_WALL_TEMPERATURE,
       AGX_WALL_VISCOSITY, AGX_WALL_TKE, AGX_WALL_SDR,        /* the reference's eleven */
       AGX_WALL_SHEAR_X, AGX_WALL_SHEAR_Y, AGX_WALL_SHEAR_Z,  /* not in the reference's list */
       AGX_WALL_END };

/* variables of the nodal function file, WriteNodeFun (output.cpp:452-469): the cell data
 * converted to the (ni+1)(nj+1)(nk+1) nodes of the block by procBlock::AssignCornerGhostCells
 * (procBlock.cpp:2716-2753), procBlock::CellToNode (:6607-6845) and ConvertCellToNode
 * (utility.hpp:186-334), dimensional with the factors of output.cpp:235-410.  A third range of
 * agx_output_pack: node variable AGX_NODE_BASE + v exists for every cell id v < AGX_OUT_COUNT,
 * and a call holds cell ids, wall ids or node ids, never a mixture.  Node (i, j, k),
 * 0 <= i <= ni ..., lies between the cells (i-1..i, j-1..j, k-1..k); sums run over them in the
 * order k, j, i ascending.
 *   density, vel_*, pressure, tke, sdr   the node state: 1/8 of the eight cells of the state
 *       with its first ghost layer.  Face and edge ghost cells as the device holds them; the
 *       eight corner ghost cells by the rule of AssignCornerGhostCells (a third of the three
 *       edge ghost cells towards the block), formed on the fly and never stored.
 *   mach, sos, energy, enthalpy   functions of the node state (thermally perfect builds: with
 *       T = p / (rho R) of the node state, primitive::SoS / Energy).
 *   temperature, viscosity   1/8 of the eight cells' temperature_ = p / (rho R) and Sutherland
 *       viscosity_ of it (the reference averages the arrays; it does not evaluate them at the
 *       node state); cp, cv at that node temperature.
 *       Departure: UpdateAuxillaryVariables (procBlock.cpp:6176) skips the eight corner ghost
 *       cells, so the reference's temperature_ / viscosity_ there are whatever the initial
 *       condition or a restart left -- they depend on history.  Here those eight cells are
 *       evaluated from their corner-rule state.  Only the eight corner nodes of a block differ.
 *   dt, resid_*   arrays without ghost cells (ConvertCellToNode, ignoreEdge, no-ghost path):
 *       the physical cells around the node, times 1 at the block's eight corners, 1/2 on its
 *       edges, 1/8 everywhere else -- boundary-face nodes, where four cells contribute,
 *       included (the reference's factor, reproduced).
 *   wallDistance   ignoreEdge with ghost cells: physical cells and first-layer face ghost
 *       cells (edge and corner ghost cells skipped), times 1/4, 1/6, 1/8.
 *   velGrad_*, tempGrad_*, densityGrad_*, pressGrad_*, tkeGrad_*, omegaGrad_*   the Green-Gauss
 *       gradient of every physical face (CalcGradsI/J/K, boundary faces included) added to the
 *       four nodes of the face -- i-faces, j-faces, k-faces, each in the order k, j, i -- times
 *       1/3 at corners, 1/5 on edges, 1/8 on boundary faces, 1/12 inside (:6782-6785).
 *   rank, globalPosition   the block's constants.
 * Refused by name: viscosityRatio, turbulentViscosity, f1, f2 in the rans libraries.  The
 * reference averages eddyViscosity_, f1_, f2_ including their ghost cells, whose content is
 * what the residual's accumulation at boundary faces and the corner initial values left; the
 * library keeps these in physical cells and connection ghost cells only and substitutes
 * nothing.  (The 5-equation libraries write the laminar 0, as for cells.)  viscosity in an
 * inviscid context is refused as for cells.
 * Timing: every nodal call first fills the ghost cells the next residual would see, like the
 * cell gradients above, so the values are those of the state the device holds when the call
 * is made; ghost cells of connections to other ranks stay as last exchanged.  dt and the
 * residuals are the last residual's.  No atomics: two calls give the same bits.  A library
 * block is one procBlock: on a split plane the values are the above with connection ghost
 * cells (the reference converts the recombined block). */
enum { AGX_NODE_BASE = 128, AGX_NODE_END = AGX_NODE_BASE + AGX_OUT_COUNT };

/* integrated wall loads: a fourth range of agx_output_pack, with no counterpart in the
 * reference (output.cpp writes per-face wall data only).  One value per LOAD SURFACE of the
 * block -- its viscousWall and slipWall surfaces in the order agx_block_set_bcs got them --
 * dimensional (SI): out[v * nsurf + s].  Sums over the faces of the surface, with |A| the
 * face's area, n its stored unit area vector (direction of increasing index), r_f its centre:
 *   area                  sum |A|
 *   area_x/y/z            sum m |A|
 *   pressureForce_x/y/z   - sum p m |A|
 *   viscousForce_x/y/z    sum (tau . m) |A|
 *   heatLoad              sum (k + kt) grad T . m |A|: heat flowing from the fluid into the wall
 *   pressureMoment_x/y/z  sum r_f x (- p m |A|), about the origin
 *   viscousMoment_x/y/z   sum r_f x ((tau . m) |A|), about the origin
 * Orientation: m = sigma n is the wall's unit normal pointing INTO THE FLUID, sigma = +1 on
 * lower sides (surface types 1, 3, 5), -1 on upper sides (2, 4, 6); the sums are the loads
 * the fluid puts on the wall.  A box of gas at rest pushes its i-min wall towards -x;
 * u = a y with a > 0 over a j-min wall drags that wall towards +x; gas hotter than a j-min
 * wall gives it a positive heat load.
 * Face values.  viscousWall faces of a viscous context: exactly what AGX_WALL_PRESSURE,
 * AGX_WALL_SHEAR_X/Y/Z and AGX_WALL_HEAT_FLUX hand out for the face (same evaluation, same
 * timing: low-Re faces from the state now and the ghost cells the next residual would see,
 * wall-law faces the stored wall data), areas times l_ref^2, face centres times l_ref.
 * slipWall faces, and every load surface of an inviscid context: p of the wall-adjacent
 * physical cell (the ghost rule keeps the ghost pressure equal to it,
 * ghostStates.cpp:109-121), no shear, no heat flux.
 * Moments need face centres, which the device holds for node-built blocks only
 * (agx_block_geom.nodes: the centres of the load-surface faces are kept from
 * agx_setup_finalize on); a block built from arrays refuses the six moment ids by name and
 * approximates nothing.  Another reference point is the caller's M - r_ref x F.
 * Timing and legality.  A viscous context: a ghost-refilling read like the wall variables
 * ("reads between phases" at agx_field_download).  An inviscid context: physical cells only,
 * legal at every position.  Not a collective: a rank gets the loads of its own blocks.
 * No floating-point atomics and a summation shape fixed by the surfaces alone (chunks of 256
 * faces, added in ascending order): two calls, and any subset, order or repetition of ids,
 * return the same bits. */
enum { AGX_LOAD_BASE = 256, AGX_LOAD_AREA = AGX_LOAD_BASE,
       AGX_LOAD_AREA_X, AGX_LOAD_AREA_Y, AGX_LOAD_AREA_Z,
       AGX_LOAD_PRESSURE_FORCE_X, AGX_LOAD_PRESSURE_FORCE_Y, AGX_LOAD_PRESSURE_FORCE_Z,
       AGX_LOAD_VISCOUS_FORCE_X, AGX_LOAD_VISCOUS_FORCE_Y, AGX_LOAD_VISCOUS_FORCE_Z,
       AGX_LOAD_HEAT,
       AGX_LOAD_PRESSURE_MOMENT_X, AGX_LOAD_PRESSURE_MOMENT_Y, AGX_LOAD_PRESSURE_MOMENT_Z,
       AGX_LOAD_VISCOUS_MOMENT_X, AGX_LOAD_VISCOUS_MOMENT_Y, AGX_LOAD_VISCOUS_MOMENT_Z,
       AGX_LOAD_END };

/* boundary fluxes: one more range of agx_output_pack, with no counterpart in the reference.
 * What the scheme lets through the boundary of a block -- mass flow, momentum flux, energy
 * flux [, the fluxes of rho k and rho omega] per inlet, outlet, far field, wall and block
 * connection.  One value per FLUX SURFACE of the block, dimensional (SI): out[v * nsurf + s].
 * The flux surfaces are every surface agx_block_set_bcs got, in that order, of every BC type,
 * local interblock / periodic connections included; connections whose partner lies on another
 * rank are left out of the list (their ghost cells are current only between the caller's
 * exchanges).  Sums over the faces of the surface, |A| the face's area, F the flux per unit
 * area in the direction of increasing index, e the equation (mass, mom_x, mom_y, mom_z,
 * energy, tke, sdr):
 *   AGX_FLUX_AREA            sum |A|
 *   AGX_FLUX_INVISCID + e    sum sigma F_inv,e |A|
 *   AGX_FLUX_VISCOUS + e     - sum sigma F_visc,e |A|
 * Orientation: sigma = +1 on upper sides (surface types 2, 4, 6), -1 on lower sides (1, 3,
 * 5): a positive value LEAVES THE BLOCK.  The viscous flux enters the residual with the
 * opposite sign of the inviscid one (procBlock.cpp:447-463 against :1392-1430), hence the
 * minus: inviscid + viscous is the net outward flux of equation e, and summed over all
 * surfaces of a block it is the sum of the block's residual (AGX_BUDGET_RESIDUAL + e)
 * wherever the equation has no source term.  The inviscid values of the two sides of a local
 * connection cancel; the viscous values cancel except for the faces on the rim of the patch,
 * which each block evaluates with its own edge ghost cells, as its residual does.
 * Face values are exactly what the residual pass takes at the face: the configured
 * reconstruction (constant, MUSCL with the configured limiter, WENO, WENO-Z) with the ghost
 * cells as its stencil, the configured inviscid flux (Roe, AUSMPW+), the viscous flux of the
 * viscous pass (central / centralFourth face values, the face's WALE eddy viscosity in
 * largeEddySimulation contexts, the k and omega diffusion in the rans libraries, the stored
 * wall data at wall-law faces).  An inviscid context returns 0 for the viscous ids.
 * Factors: the nondimensional sum times the factor of the conserved variable (what
 * agx_restart_pack gives consVarsNm1) times a_ref l_ref^2 -- the area times l_ref^2:
 *   mass     rho_ref a_ref l_ref^2                    [kg/s]
 *   mom_x/y/z  rho_ref a_ref^2 l_ref^2                [N]
 *   energy   rho_ref a_ref^3 l_ref^2                  [W]
 *   tke      rho_ref a_ref^3 l_ref^2
 *   sdr      rho_ref^2 a_ref^3 l_ref^2 / mu_ref
 * (for e < 6 the factor of AGX_OUT_RESID + e; resid_sdr of the cell range carries the
 * reference file's a_ref^4.  The viscous energy value of a viscousWall at rest is the
 * nondimensional sum of AGX_LOAD_HEAT, which carries the wall file's mu_ref t_ref / l_ref
 * instead; the viscous momentum values are AGX_LOAD_VISCOUS_FORCE_X/Y/Z as they are.)
 * The 5-equation libraries refuse e = 5, 6 by name.
 * Timing and legality.  A ghost-refilling read in viscous and inviscid contexts alike (the
 * inviscid flux of a boundary face reads the ghost cells too): the ghost cells, edges
 * included, are those the next residual would see; refused from the caller's
 * agx_phase_bc_faces to the agx_phase_residual that follows it ("reads between phases" at
 * agx_field_download), legal elsewhere, and the run stays bit-identical.  Wall-law faces:
 * refused before the first residual, like the wall variables.  Not a collective.
 * Determinism: no floating-point atomics, a shape fixed by the surfaces alone (chunks of 256
 * faces that never span two surfaces, added in ascending order), all 15 sums formed on every
 * call: two calls, and any subset, order or repetition of ids, return the same bits.
 * Refused by name: ids of another range in the same call; more than 15 ids; a block all of
 * whose surfaces are connections to other ranks; a call before agx_setup_finalize. */
enum { AGX_FLUX_BASE = 384, AGX_FLUX_AREA = AGX_FLUX_BASE,
       AGX_FLUX_INVISCID = AGX_FLUX_BASE + 1,      /* + e, e = 0 ... 6 */
       AGX_FLUX_VISCOUS = AGX_FLUX_BASE + 8,       /* + e */
       AGX_FLUX_END = AGX_FLUX_BASE + 15 };

/* block balance: one value per id, out[v], dimensional, over the PHYSICAL cells of the block:
 *   AGX_BUDGET_VOLUME          sum V                                     times l_ref^3
 *   AGX_BUDGET_TOTAL + e       sum U_e V, the conserved variables of the state now (mass,
 *                              momentum, total energy, rho k, rho omega): the factor of the
 *                              conserved variable times l_ref^3
 *   AGX_BUDGET_RESIDUAL + e    sum residual_e, the residual planes as the last residual pass
 *                              left them, with the factor of AGX_FLUX_INVISCID + e
 * so that BUDGET_RESIDUAL_e = sum over the flux surfaces of (FLUX_INVISCID_e + FLUX_VISCOUS_e)
 * holds as delivered, to rounding, for e < 5 on a rank that holds all of the block's
 * surfaces.  In the rans libraries the k and omega residuals contain the source terms: no
 * balance is claimed for e = 5, 6.  On a coarse multigrid level the ids return what the
 * level's planes hold (the forcing term is not in the fluxes): no balance is claimed.
 * Timing.  Physical cells only: legal at every position, and the run stays bit-identical.
 * Every path keeps the residual in its planes (the fused explicit stage kernel stores it
 * beside the new state, the diagonal-ordered LU-SGS path reads it from them), so the sums are
 * never stale; but after agx_iterate, or an update phase, the residual belongs to the state
 * BEFORE the update while the fluxes and the totals belong to the state now.  The balance is
 * exact right after agx_phase_residual.
 * Determinism: the rows (j, k) of the block in chunks of 64, k outer; a row by 64 strided
 * lanes added by shuffles; the chunks added in ascending order.  A shape fixed by the extents
 * alone, no atomics, all 15 sums formed on every call.
 * Refused by name: the residual sums before the first residual (agx_phase_residual,
 * agx_iterate, or an upload of AGX_FIELD_RESIDUAL); e = 5, 6 in the 5-equation libraries;
 * ids of another range in the same call; more than 15 ids. */
enum { AGX_BUDGET_BASE = 448, AGX_BUDGET_VOLUME = AGX_BUDGET_BASE,
       AGX_BUDGET_TOTAL = AGX_BUDGET_BASE + 1,     /* + e, e = 0 ... 6 */
       AGX_BUDGET_RESIDUAL = AGX_BUDGET_BASE + 8,  /* + e */
       AGX_BUDGET_END = AGX_BUDGET_BASE + 15 };

/* time statistics: a fifth and a sixth range of agx_output_pack, with no counterpart in the
 * reference.  An unsteady run (largeEddySimulation, SST-DES, bdf2 dual time stepping) is read
 * from its time averages; the library keeps them on the device, so that a sample costs one
 * streaming pass over the block instead of a download of its state.
 * What is averaged.  Per physical cell the vector rho, u, v, w, p, T = p / (rho R), rho u,
 * rho v, rho w; in contexts with an eddy viscosity (largeEddySimulation, the rans libraries)
 * also that -- the last residual's, as AGX_OUT_TURB_VISCOSITY reads it; in the 7-equation
 * libraries also k and omega.  Second moments: the six velocity co-moments and the variances
 * of rho, p and T.  Per viscousWall face of a viscous context: the mean of each of the 14 wall
 * variables (AGX_WALL_*), and the variances of the wall pressure and of the three shear
 * components.  The Favre mean is the caller's division mean(rho u) / mean(rho); time-averaged
 * integrated loads are the integrals of the mean face values.
 * The recurrence (West 1979), per cell and per face, with the sample's weight w and the sum
 * of weights W including it:
 *   delta = x - mean;   mean += (w / W) delta;   C_ab += w (1 - w / W) delta_a delta_b
 * and the covariance is C_ab / W.  Not sums of squares: E[x^2] - E[x]^2 loses every digit at
 * the fluctuation levels an LES resolves.  Identical samples give the sample as the mean, bit
 * for bit, and second moments of exactly 0; multiplying every weight by a power of two
 * changes no bit.
 * Timing.  A sample (agx_field_upload, AGX_FIELD_STAT_SAMPLE) takes the state the device
 * holds when it is made; the wall variables are evaluated as agx_output_pack would at that
 * moment (low-Re faces from the state now with the ghost cells the next residual would see,
 * wall-law faces the stored wall data).  The time loop samples after mgSolution::Iterate has
 * converged a time step.  agx_iterate never samples.
 * Legality: see AGX_FIELD_STAT_SAMPLE.  Packing the statistics reads the accumulators only
 * and is legal at every position.
 * Determinism: no atomics, no reduction across cells; a cell's statistics are a function of
 * its own samples, and two runs give the same bits.  Not a collective: a rank averages its
 * own blocks, each block its own cells.
 * AGX_STAT_BASE + n: one value per physical cell, out[v * ni*nj*nk + cell] like the cell
 * range, dimensional (a mean with the factor of its variable, a second moment with the
 * product of the two factors), n in the order
 *   0 mean density; 1..3 mean vel_x/y/z; 4 mean pressure; 5 mean temperature;
 *   6..8 mean mom_x/y/z (rho u_i); 9 mean turbulentViscosity; 10 mean tke; 11 mean sdr;
 *   12..17 cov uu, uv, uw, vv, vw, ww; 18 var density; 19 var pressure; 20 var temperature.
 * Refused by name: mean turbulentViscosity where the context has no eddy viscosity, mean tke
 * and sdr in the 5-equation libraries.
 * AGX_WSTAT_BASE + n: one value per wall face in the layout of the wall range,
 *   n = w - AGX_WALL_YPLUS: the mean of wall variable w, for each of the 14;
 *   14 var pressure; 15..17 var shearStress_x/y/z.
 * Refused like the wall range: an inviscid context, a block without a viscousWall surface;
 * mean tke and sdr in the 5-equation libraries.
 * Both ranges refuse by name before the block's first sample; a call holds ids of one range,
 * and at most as many as the range has. */
enum { AGX_STAT_BASE = 512, AGX_STAT_END = 533 };
enum { AGX_WSTAT_BASE = 576, AGX_WSTAT_END = 594 };

/* the cell statistics collapsed along homogeneous index directions: a seventh range of
 * agx_output_pack.  A channel is read as profiles over y, a flat plate as fields over (x, y):
 * the time statistics pooled over the block's homogeneous directions, a few kilobytes where
 * the 21 planes of AGX_STAT_BASE are gigabytes.
 * id = AGX_CSTAT_BASE + 32 * mask + n.  mask: the collapsed directions, bit 0 = i, bit 1 = j,
 * bit 2 = k, 1 ... 7.  A BIN is one position of the directions that remain (lines, planes, or
 * with mask 7 the whole block).  With the volume v_c, the time means m_c, the time co-moments
 * C_c of the bin's physical cells c and the sum of weights W:
 *   V = sum v_c;   M = sum v_c m_c / V
 *   cov_ab = sum v_c [ C_c,ab / W + (m_c,a - M_a)(m_c,b - M_b) ] / V
 * cov_ab is the co-moment about the space-time mean of the bin (the law of total covariance).
 * n = 0 ... 20: the variables of AGX_STAT_BASE in its order, a mean as the pooled mean M, a
 * second moment as the pooled cov_ab; n = 21: the bin's volume V l_ref^3.
 * The recurrence.  A bin is formed by the weighted one-pass recurrence of the time statistics,
 * in space, cell by cell:
 *   V += v;  r = v / V;  cf = v (1 - r);  delta = m - M
 *   M += r delta;   T_ab += r (C_ab - T_ab);   D_ab += (cf delta_a) delta_b
 * and two partial bins join by the pairwise form, r = V2 / (V1 + V2), delta = M2 - M1:
 *   M = M1 + r delta;  T = T1 + r (T2 - T1);  D = D1 + D2 + ((V1 r) delta_a) delta_b
 * The value is cov = T / W + D / V with the dimensional factors of AGX_STAT_BASE.  No sums of
 * squares and no second pass.  Cells with bit-identical m and C give M = m and cov = C / W bit
 * for bit -- what AGX_STAT_BASE returns for a cell of the bin -- whatever their volumes.
 * Layout: out[v * nbin + bin], variable by variable in the caller's order; nbin is the product
 * of the remaining extents, the bins ordered over the remaining directions as k, then j, then
 * i, i fastest; mask 7 gives one bin.  Dimensional, like the cell range.
 * Refused by name, with nothing written: a call before the block's first sample; mask 0 or a
 * mask above 7; n above 21; ids of two masks in one call; these ids with ids of another range
 * in one call; more than AGX_CSTAT_COUNT ids (repeated ids are allowed); mean
 * turbulentViscosity, tke and sdr wherever AGX_STAT_BASE refuses them.
 * Timing and legality.  Reads the accumulators and the volume plane only: legal at every
 * position, and the run stays bit-identical.  Only the planes of the requested ids are read (a
 * second moment reads its two means).  Not a collective: a rank gets the bins of its own
 * block; blocks that share the remaining directions, and ranks, are joined by the caller with
 * the pairwise form from (V, M, cov): cov = cov1 + r (cov2 - cov1) + (V1 r / V) delta_a delta_b.
 * Determinism.  No floating-point atomics, and a shape of the recurrence and of the joins
 * fixed by the block's extents and the mask alone (the collapsed j and k positions in chunks
 * of 64, k outer; a collapsed row by 64 strided lanes joined by a butterfly; the chunks added
 * in ascending order): two calls, and any subset, order or repetition of ids, return the same
 * bits. */
enum { AGX_CSTAT_BASE = 1024, AGX_CSTAT_COUNT = 22, AGX_CSTAT_END = 2048 };

/* what a halo exchange carries (gridLevel.cpp:299-313, utility.cpp:400-423) */
enum { AGX_HALO_STATE = 0, AGX_HALO_UPDATE = 1,
       /* velocityGrad_ of the cells across connection surfaces, swapped after the
        * residual (gridLevel.cpp:343-368, :386-388) and read by the off-diagonal
        * terms of the block-matrix solvers with viscous terms; two halves of the
        * nine components, each in slabs of the usual five slots per cell */
       AGX_HALO_VELGRAD_A = 2, AGX_HALO_VELGRAD_B = 3,
       /* rans: eddyViscosity_, f1_, f2_ of the cells across connection surfaces
        * (SwapEddyViscAndGradients / SwapTurbVars, gridLevel.cpp:386-392); read by the
        * off-diagonal terms.  libaither_gfx950_rans.so (and the oracle); the 5-equation
        * library refuses it. */
       AGX_HALO_TURB = 4 };

/* ---- plain-old-data descriptors --------------------------------------- */

/* thermodynamic model (input::ThermodynamicModel, input.cpp:795-803).  A library is built for
 * one of them: libaither_gfx950[_rans].so for the calorically perfect gas,
 * libaither_gfx950[_rans]_tp.so (-DAGX_TPG=1) for the thermally perfect one (cv, cp, gamma
 * and Pr functions of T, thermodynamic.hpp:125-189); agx_config_set REFUSES the other. */
enum { AGX_THERMO_CALORICALLY_PERFECT = 0, AGX_THERMO_THERMALLY_PERFECT = 1 };
enum { AGX_MAX_VIB = 4 };     /* vibrational modes per species (fluidDatabase: 1) */

/* single-species ideal gas (calorically or thermally perfect) + Sutherland transport.
 * Values are the already-nondimensional ones the reference holds after
 * input::NondimensionalizeFluid (fluid.cpp:83-97, eos.cpp:26-36,
 * thermodynamic.cpp:27-41, transport.cpp:31-69). */
typedef struct agx_gas {
  double gas_constant;   /* idealGas::gasConst_[0] (nondimensional R)      */
  double n;              /* fluid::N(): cv = n R, cp = (n+1) R             */
  double heat_of_formation; /* caloricallyPerfect::hf_[0] (nondimensional) */
  double visc_c1, visc_s;   /* Sutherland viscosity C1 [kg/(m s K^.5)], S [K] */
  double cond_c1, cond_s;   /* Sutherland conductivity C1, S               */
  double t_ref;          /* referenceTemperature [K]                       */
  double rho_ref;        /* referenceDensity [kg/m^3]                      */
  double l_ref;          /* referenceLength [m]                            */
  double a_ref;          /* reference speed of sound [m/s] (input.cpp:608-613) */
  /* thermally perfect gas (AGX_THERMO_THERMALLY_PERFECT): the vibrational temperatures of
   * the species divided by t_ref (fluid.cpp:92); n_vib = 0 for a calorically perfect gas */
  int32_t n_vib, pad_;
  double theta_v[AGX_MAX_VIB];
} agx_gas;

/* solver configuration; one per context */
typedef struct agx_config {
  int32_t n_eq;              /* 5, or 7 = [rho, u, v, w, p, k, omega] in the rans library */
  int32_t n_ghost;           /* input::NumberGhostLayers (input.cpp:1127)  */
  int32_t recon;             /* AGX_RECON_*                                */
  int32_t limiter;           /* AGX_LIMITER_*                              */
  int32_t inviscid_flux;     /* AGX_FLUX_*                                 */
  int32_t is_viscous;        /* input::IsViscous                           */
  int32_t time_integration;  /* AGX_TIME_*                                 */
  int32_t matrix_solver;     /* AGX_SOLVER_*                               */
  int32_t matrix_sweeps;     /* input::MatrixSweeps                        */
  int32_t nonlinear_iterations; /* input::NonlinearIterations              */
  /* the rest of what the path depends on.  agx_config_set REFUSES every value
   * this build does not implement (it never substitutes another scheme): */
  int32_t equation_set;      /* AGX_EQN_*; must agree with is_viscous / n_eq */
  int32_t inv_flux_jacobian; /* AGX_JACOBIAN_* (input::InvFluxJac)          */
  int32_t viscous_recon;     /* AGX_VISC_RECON_* (input::ViscousFaceReconstruction) */
  int32_t turbulence_model;  /* AGX_TURB_* (input::TurbulenceModel)         */
  double kappa;              /* MUSCL kappa (input.cpp:277-292)            */
  double theta, zeta;        /* Beam-Warming (input.cpp:261-270)           */
  double matrix_relaxation;  /* input::MatrixRelaxation                    */
  double dual_time_cfl;      /* input::DualTimeCFL, <= 0: off              */
  double dt_nondim;          /* Dt * aRef / lRef (procBlock.cpp:808); <= 0:
                                local time stepping from CFL               */
  double viscous_cfl_coeff;  /* input::ViscousCFLCoefficient (input.cpp:1110) */
  agx_gas gas;
  int32_t thermodynamic_model; /* AGX_THERMO_* (input::ThermodynamicModel)  */
  int32_t pad_;
} agx_config;

/* geometry of one block, host AoS arrays with ghosts (procBlock.hpp:65-90).
 * Face-area arrays hold unitVec3dMag = {nx, ny, nz, |A|} per face
 * (vector3d.hpp:125-190).  Dimensions with G = 2*ng:
 *   farea_i: (ni+1+G, nj+G,   nk+G)   x 4
 *   farea_j: (ni+G,   nj+1+G, nk+G)   x 4
 *   farea_k: (ni+G,   nj+G,   nk+1+G) x 4
 *   vol, width_i/j/k, wall_dist: (ni+G, nj+G, nk+G) x 1
 *   center:  (ni+G, nj+G, nk+G) x 3                                        */
typedef struct agx_block_geom {
  int32_t ni, nj, nk;        /* physical cells                             */
  int32_t ng;                /* ghost layers                               */
  int32_t parent_block;      /* procBlock::ParentBlock (for L-inf report)  */
  int32_t global_pos;        /* procBlock::GlobalPos                       */
  const double *farea_i, *farea_j, *farea_k;
  const double *vol;
  const double *center;
  const double *width_i, *width_j, *width_k;   /* cellWidthI/J/K_          */
  const double *wall_dist;   /* may be NULL for inviscid                   */
  /* OR the node coordinates alone, [nk+1][nj+1][ni+1][3], i fastest, nondimensional (as
   * agx_plot3d_metrics takes them), with all nine pointers above NULL: the library forms the
   * whole geometry on the device.  agx_block_create computes the metrics of the physical
   * cells (and refuses a block turned inside out); agx_setup_finalize completes the ghost
   * geometry in the reference's order -- AssignGhostCellsGeom, SwapGeomSlice (which may set
   * entries of the stored connections' patch_border, the T-intersection rule),
   * AssignGhostCellsGeomEdge, CalcCellWidths and, in viscous runs, CalcWallDistance and
   * SwapWallDist.  All blocks of a context are built the same way, and all partners of its
   * connections are on this rank.  NULL: the arrays above are used.  Callers zero the
   * struct, so one compiled before this field existed passes NULL. */
  const double *nodes;
} agx_block_geom;

/* boundary-state data for one surface: the union of the fields the
 * reference's inputState subclasses hold (include/inputStates.hpp:112-420),
 * already nondimensional. */
typedef struct agx_bc_state {
  double pressure, density;
  double velocity[3];
  double stagnation_pressure, stagnation_temperature;
  double direction[3];
  double wall_temperature;   /* viscousWall isothermal                     */
  double wall_heat_flux;     /* viscousWall constant heat flux             */
  double length_scale;       /* nonreflecting inlet / outlet               */
  int32_t is_isothermal, is_heat_flux, is_nonreflecting, pad_;
  /* farfield turbulence of the state (ApplyFarfieldTurbBC, primitive.cpp:83-98):
   * turbulenceIntensity and eddyViscosityRatio; read by rans runs only */
  double turb_intensity, eddy_visc_ratio;
  /* viscousWall(wallTreatment=wallLaw): von Karman constant and wall constant
   * (inputStates.hpp:343-345); rans library; adiabatic, isothermal or heat-flux wall */
  double von_karman, wall_constant;
  int32_t is_wall_law, pad2_;
} agx_bc_state;

/* one boundarySurface (boundaryConditions.hpp:55-150): index ranges are the
 * reference's node-style ranges exactly as read from the .inp file. */
typedef struct agx_bc_surface {
  int32_t bc_type;           /* AGX_BC_*                                   */
  int32_t imin, imax, jmin, jmax, kmin, kmax;
  int32_t tag;
  agx_bc_state state;
} agx_bc_surface;

/* POD mirror of class connection (boundaryConditions.hpp:371-433) */
typedef struct agx_connection {
  int32_t rank[2];
  int32_t block[2];          /* global block ids                           */
  int32_t local_block[2];    /* ids returned by agx_block_create on that rank */
  int32_t boundary[2];       /* surface type 1..6                          */
  int32_t d1_start[2], d1_end[2], d2_start[2], d2_end[2];
  int32_t const_surf[2];
  int32_t patch_border[8];
  int32_t orientation;       /* 1..8 (boundaryConditions.cpp:653-727)      */
  int32_t is_interblock;     /* 0 for periodic                             */
} agx_connection;

/* L-infinity residual record, class resid (include/resid.hpp) */
typedef struct agx_linf {
  double linf;
  int32_t block, i, j, k, eqn;   /* eqn is 1-based (procBlock.cpp:864)     */
  int32_t pad_;
} agx_linf;

typedef struct agx_ctx agx_ctx;

/* ---- context ----------------------------------------------------------- */
const char *agx_last_error(void);
const char *agx_version(void);
/* rank: this process's rank in the job (matches agx_connection.rank[]) */
int agx_ctx_create(int device, int rank, agx_ctx **out);
void agx_ctx_destroy(agx_ctx *ctx);
/* run all library work on this hipStream_t (NULL = default stream); may be called at any
 * time: the stream used so far is drained first */
int agx_ctx_set_stream(agx_ctx *ctx, void *hip_stream);
int agx_config_set(agx_ctx *ctx, const agx_config *cfg);

/* ---- setup: after SendFinestGridLevel / AuxillaryAndWidths / SwapWallDist
 *      (main.cpp:163-203) ------------------------------------------------ */
int agx_block_create(agx_ctx *ctx, const agx_block_geom *geom, int *block_id);
int agx_block_set_bcs(agx_ctx *ctx, int block_id, int n_surfaces,
                      const agx_bc_surface *surfaces);
int agx_conn_create(agx_ctx *ctx, const agx_connection *conn, int *conn_id);
/* finish setup: complete the geometry of node-built blocks (agx_block_geom.nodes), build
 * index maps, hyperplane order, allocate work arrays */
int agx_setup_finalize(agx_ctx *ctx);

/* ---- state movement ---------------------------------------------------- */
/* replaces gridLevel ctor state init / ReadRestart (gridLevel.cpp:55,63-65) */
int agx_state_upload(agx_ctx *ctx, int block_id, const double *state_aos);
/* replaces the pack in GetFinestGridLevel (procBlock.cpp:4491-4660).
 * Reads between phases: a download, agx_output_pack and agx_restart_pack may be made at any
 * point between two calls of the library -- between the phases of an iteration, between the
 * agx_mg_* calls of a cycle, between agx_iterate calls -- and leave the run bit-identical.
 * One group is the exception, because it refills the ghost cells of the state (inviscid fill,
 * then the viscous-wall fill, which stays): the gradient fields (AGX_FIELD_VEL_GRAD ..
 * AGX_FIELD_PRESS_GRAD), and of agx_output_pack the gradient variables, every node variable
 * and every wall variable, and on a viscous context every load variable (AGX_LOAD_*; an
 * inviscid context reads physical cells only there), and in every context every flux variable
 * (AGX_FLUX_*; the budget variables AGX_BUDGET_* read physical cells only and are legal
 * everywhere).  From the caller's agx_phase_bc_faces up to the
 * agx_phase_residual that follows it the ghost cells are being filled for that residual, and
 * these calls are REFUSED with a message; they are legal from agx_phase_residual to the next
 * agx_phase_bc_faces, and between agx_iterate calls (agx_iterate's own fill does not count). */
int agx_field_download(agx_ctx *ctx, int block_id, int field, double *out_aos);
int agx_field_upload(agx_ctx *ctx, int block_id, int field, const double *in_aos);

/* ---- per time step: mgSolution::StoreOldSolution (mgSolution.cpp:103-114):
 *      consVarsN_ <- ConsVars(state_), and consVarsNm1_ <- consVarsN_ when
 *      also_nm1 != 0 (first bdf2 step) ----------------------------------- */
int agx_store_time_n(agx_ctx *ctx, int also_nm1);

/* ---- per nonlinear iteration: mgSolution::Iterate (mgSolution.cpp:246-269).
 *  mm   -- nonlinear iteration index (RK stage for rk4)
 *  cfl  -- input::CFL() after input::CalcCFL(nn) (input.cpp:637-639)
 *  l2   -- n_eq doubles, ACCUMULATED into (sum of residual^2, procBlock.cpp:858)
 *  linf -- updated only when a larger signed residual is found (:863-866)
 *  matrix_resid -- returns sum(matrixResid^2)/count (mgSolution.cpp:198-206)
 * With connections to other ranks: install an exchange first (agx_set_exchange /
 * agx_rccl_exchange_create, below), or drive the phases and exchange the slabs
 * yourself. */
int agx_iterate(agx_ctx *ctx, int mm, double cfl, double *l2, agx_linf *linf,
                double *matrix_resid);

/* ---- phases of one iteration, for multi-process runs --------------------
 * Order (explicit):  bc_faces, [halo STATE], bc_edges, residual, explicit_update
 * Order (implicit):  bc_faces, [halo STATE], bc_edges, residual, implicit_begin,
 *                    sweeps x { [halo UPDATE], relax_forward, [halo UPDATE],
 *                    relax_backward }   (LU-SGS, linearSolver.cpp:430-470)
 *                    or sweeps x { [halo UPDATE], relax_forward } (DPLUR :509-535)
 *                    [halo UPDATE], matrix_residual, implicit_update          */
int agx_phase_bc_faces(agx_ctx *ctx);          /* AssignInviscidGhostCells  procBlock.cpp:2449 */
int agx_phase_bc_edges(agx_ctx *ctx);          /* AssignInviscidGhostCellsEdge procBlock.cpp:2565 */
/* mm: nonlinear iteration (RK stage) -- explicit inviscid runs fuse the stage
 * update into the residual kernel, explicit_update then only swaps buffers */
int agx_phase_residual(agx_ctx *ctx, int mm, double cfl); /* CalcResidualNoSource :6111 + CalcBlockTimeStep :798 */
int agx_phase_explicit_update(agx_ctx *ctx, int mm, double *l2, agx_linf *linf); /* UpdateBlock :826 */
int agx_phase_implicit_begin(agx_ctx *ctx);    /* InvertDiagonal + InitializeMatrixUpdate mgSolution.cpp:225-229 */
int agx_phase_relax_forward(agx_ctx *ctx, int sweep);  /* LUSGS_Forward :341 / DPLUR :473 */
int agx_phase_relax_backward(agx_ctx *ctx, int sweep); /* LUSGS_Backward :385 */
int agx_phase_matrix_residual(agx_ctx *ctx, double *matrix_resid); /* linearSolver::Residual :92 */
int agx_phase_implicit_update(agx_ctx *ctx, int mm, double *l2, agx_linf *linf); /* UpdateBlocks gridLevel.cpp:418 */

/* ---- output: the payloads of the reference's files, packed on the device ----
 * WriteFunFile (output.cpp:209-437): `nvar` variables (AGX_OUT_*, in the caller's order --
 * the reference writes its std::set alphabetically) of one block, physical cells, i
 * fastest, variable by variable: out[v * ni*nj*nk + cell], dimensional as the reference
 * writes them (reference quantities from agx_config.gas).  Variables a build does not hold
 * (tke, sdr, eddy viscosity, f1, f2 and their gradients in the 5-equation library) come
 * out as the reference's laminar values (0), viscosity in inviscid runs is refused.
 * WriteWallFun (output.cpp:472-571): with wall variables (AGX_WALL_*) the payload of the wall
 * file of one block instead -- variable by variable in the caller's order; within a variable
 * the block's viscousWall surfaces in the order agx_block_set_bcs got them (the order of
 * wallData_, procBlock.cpp:76-85); within a surface its faces, i fastest, then j, then k over
 * the surface's index range (the loop nest of output.cpp:505-516):
 * out[v * nfaces + offset(surface) + face].  The caller sizes `out` from its own surfaces.
 * WriteNodeFun (output.cpp:452-469): with node variables (AGX_NODE_BASE + AGX_OUT_*) the
 * payload of the nodal function file of one block instead -- variable by variable in the
 * caller's order, within a variable the (nk+1)(nj+1)(ni+1) nodes, i fastest (the loop nest of
 * output.cpp:231-233 over the node block): out[v * nnodes + node].
 * Integrated wall loads (no counterpart in output.cpp): with load variables (AGX_LOAD_*) one
 * value per load surface of the block instead -- its viscousWall and slipWall surfaces in the
 * order agx_block_set_bcs got them -- variable by variable in the caller's order:
 * out[v * nsurf + surface], see the enum.
 * Boundary fluxes and the block balance (no counterpart in output.cpp): with flux variables
 * (AGX_FLUX_*) one value per flux surface of the block -- every surface agx_block_set_bcs
 * got, in that order, but the connections to other ranks -- out[v * nsurf + surface]; with
 * budget variables (AGX_BUDGET_*) one value per id, out[v]; see the enums for what they
 * refuse.
 * Time statistics (no counterpart in output.cpp): with statistics ids (AGX_STAT_BASE + n) one
 * value per physical cell in the layout of the cell variables, with wall statistics ids
 * (AGX_WSTAT_BASE + n) one value per wall face in the layout of the wall variables; with
 * collapsed statistics ids (AGX_CSTAT_BASE + 32 * mask + n) one value per bin of the
 * directions that remain, out[v * nbin + bin]; see the enums for what they refuse.
 * Refused: variables of two ranges in one call, an id in no range, a block without a
 * viscousWall surface, an inviscid context, wall-law surfaces before the first residual (the
 * three: wall variables), the four node variables named above, nvar beyond the number of ids
 * of its range (repeated ids are allowed in all four); gradient, node and wall variables
 * between agx_phase_bc_faces and the agx_phase_residual that follows it ("reads between
 * phases" at agx_field_download).  Load variables: a block without a viscousWall or slipWall
 * surface, a call before agx_setup_finalize, wall-law surfaces before the first residual, the
 * six moment ids on a block built from arrays, and -- a viscous context only -- the interval
 * between agx_phase_bc_faces and agx_phase_residual. */
int agx_output_pack(agx_ctx *ctx, int block, int nvar, const int32_t *vars, double *out);
/* WriteRestart (output.cpp:651-752), the payload of one block: cell by cell (i fastest)
 * n_eq + 1 dimensional values -- density, velocity, pressure, [tke, sdr,] mass fraction of
 * the single species (1).  which = 0: the state; which = 1: consVarsNm1 (the second
 * solution of multilevel time integration: conserved variables, :700-750). */
int agx_restart_pack(agx_ctx *ctx, int block, int which, double *out);

/* ---- start and resume: the state a run starts from, formed on the device -------------
 * After each of the three calls below the block is exactly as if the caller had made the
 * matching upload of a host array -- agx_state_upload of the ghost-padded state with those
 * physical cells and ZERO in every ghost cell, or (agx_restart_unpack, which = 1)
 * agx_field_upload(AGX_FIELD_CONS_NM1) -- the same bits in the planes and the same
 * bookkeeping.  They are legal wherever those uploads are, but only after
 * agx_setup_finalize (the cloud search reads the cell centres, which a node-built block
 * has from then on).  Refused with a message, the block untouched: a call before
 * agx_setup_finalize, a bad block id, a null pointer, and what each entry names.
 *
 * procBlock::InitializeStates, non-file branch (procBlock.cpp:325-354): every physical cell
 * takes prim[n_eq], the nondimensional primitive of primitive::NondimensionalInitialize
 * (the caller forms these n_eq scalars; rans: k, omega of ApplyFarfieldTurbBC included).
 * Refused: density <= 0, pressure <= 0 ("nonphysical density / pressure", :329-330), a
 * non-finite value. */
int agx_state_fill(agx_ctx *ctx, int block, const double *prim);
/* file branch (procBlock.cpp:287-323; CalcTreeFromCloud utility.cpp:521-605,
 * kdtree::NearestNeighbor kdtree.cpp:123-225): every physical cell takes states[id] of the
 * cloud point nearest to its centre.  points[npts][3], states[npts][n_eq], nondimensional,
 * host memory.  *max_dist (may be NULL): the largest distance from a cell centre to its
 * point, the reference's maxDist (without its floor of DBL_MIN: 0 where every centre is a
 * cloud point).
 * TIE RULE: among points at equal squared distance the LOWEST index wins (the reference's
 * k-d tree leaves ties to its build order).
 * The search is exhaustive, tiled through LDS: its work is cells x points.  128^3 cells x
 * 1e5 points is the size it is meant for (DESIGN section 8 has the measured time); a cloud
 * the size of a 256^3 grid against such a grid is over a thousand times that work and keeps the host's
 * k-d tree (case.builder, initial="host").
 * Refused: npts < 1; a cloud state with density <= 0, pressure <= 0 (:304-305) or a
 * non-finite value (a host scan of the npts rows before anything is written). */
int agx_state_from_cloud(agx_ctx *ctx, int block, int64_t npts, const double *points,
                         const double *states, double *max_dist);
/* ReadSolFromRestart (output.cpp:1177-1240) + GetStatesFromRestart, which = 0;
 * ReadSolNm1FromRestart (:1242-1305) + GetSolNm1FromRestart, which = 1: the inverse of
 * agx_restart_pack, same payload layout (cell by cell, i fastest, n_eq + 1 dimensional
 * values).  The values are divided by the reference's divisors, formed in its order, with
 * correctly rounded divisions; density is (raw / rho_ref) * mass fraction.
 * Refused: which other than 0 or 1; which = 1 where agx_field_upload refuses
 * AGX_FIELD_CONS_NM1. */
int agx_restart_unpack(agx_ctx *ctx, int block, int which, const double *in);

/* ---- set-up: the volume-sized parts of the reference's grid set-up -------
 * plot3dBlock::Volume / Centroid / FaceAreaI,J,K / FaceCenterI,J,K (plot3d.cpp:35-360) of
 * one block from its node coordinates nodes[nk+1][nj+1][ni+1][3] (i fastest, as
 * plot3dBlock holds them).  Outputs in the reference's layout, physical cells / faces only
 * (ghost geometry -- PadWithGhosts, AssignGhostCellsGeom, SwapGeomSlice: surface-sized
 * work -- stays with the caller): vol[nk][nj][ni], center[nk][nj][ni][3],
 * farea_i[nk][nj][ni+1][4] = {unit normal, |A|}, fcenter_i[nk][nj][ni+1][3], the j- and
 * k-face arrays with the extra entry in their own direction.  Any output may be NULL.
 * Host pointers; needs neither a configuration nor blocks. */
int agx_plot3d_metrics(agx_ctx *ctx, int ni, int nj, int nk, const double *nodes,
                       double *vol, double *center, double *farea_i, double *farea_j,
                       double *farea_k, double *fcenter_i, double *fcenter_j,
                       double *fcenter_k);
/* kdtree::NearestNeighbor over the viscous-wall face centres (kdtree.cpp:123-225 as
 * main.cpp:191-203 / procBlock::CalcWallDistance procBlock.cpp:6030-6042 use it): for
 * each of ncell points (x, y, z) the distance to the nearest of nwall points.  On the
 * device an exhaustive search tiled through LDS (no tree: 16.7 M cells x 65 k wall faces is
 * a fraction of a second).  The ghost-cell rule of CalcWallDistance (:6044-6107) and
 * SwapWallDist are surface-sized and stay with the caller.  Host pointers. */
int agx_nearest_wall_distance(agx_ctx *ctx, int64_t ncell, const double *cell_centres,
                              int64_t nwall, const double *wall_points, double *dist);

/* ---- geometric multigrid ---------------------------------------------
 * A grid level is a context of its own (gridLevel): same configuration, the coarsened
 * blocks and surfaces of procBlock::GetCoarseMeshAndBCs (procBlock.cpp:6471-6603; host
 * set-up, aither_amd/case/multigrid.py).  These calls move data between block `blk` of a
 * fine context and the same block of the next coarser one, and give a level what
 * mgSolution::CycleAtLevel (mgSolution.cpp:160-205) needs beyond the phases above.  Both
 * contexts live on the same device.  The forcing term is carried by all four relaxations of
 * both libraries (DPLUR, BDPLUR, BLU-SGS, scalar LU-SGS -- in the 5-equation library on its
 * diagonal-ordered production path and in its hyperplane form); the turbulence equations of
 * the 7-equation library are restricted, forced and prolonged like the flow equations, as
 * the reference's transfers on varArray do.  `to_coarse` [nk][nj][ni][3] (int32, host):
 * the coarse cell (i, j, k) of every physical cell of the fine block.
 * The device copies of `to_coarse`, `vol_fac` and `coeffs` are keyed on the HOST POINTER, per
 * fine block: an array is uploaded when its pointer differs from the one of the previous
 * call.  The arrays must therefore stay alive and unchanged for as long as the fine context
 * lives (gridLevel keeps them as members); freeing one and passing another at the same
 * address, or changing one in place, leaves the device with the old contents.
 * The caller's cycle makes the swaps that end gridLevel::CalcResidual after the
 * agx_phase_residual of EVERY level (gridLevel.cpp:386-392; Restriction :559-563 calls
 * CalcResidual on the coarse level): AGX_HALO_VELGRAD_A and _B for a viscous block-matrix
 * solver, AGX_HALO_TURB for seven equations -- the conditions of agx_iterate. */
enum { AGX_MG_STATE = 0, AGX_MG_UPDATE = 1, AGX_MG_FORCING = 2 };
/* BlockRestriction (procBlock.hpp:636-690) of
 *   AGX_MG_STATE    the primitive state, volume weighted (procBlock::Restriction :6847);
 *                   the coarse block's state is zeroed first, ghost cells included
 *   AGX_MG_UPDATE   the linear solver's x, volume weighted (linearSolver.cpp:212-222; the
 *                   caller swaps the coarse x across connections afterwards)
 *   AGX_MG_FORCING  the fine level's matrix residual (the array of its last
 *                   agx_mg_matrix_residual), summed, plus A x - b of the coarse level
 *                   (gridLevel.cpp:568-590): the coarse level's forcing term
 * vol_fac [nk][nj][ni] (host): a fine cell's volume over that of its coarse cell; NULL for
 * AGX_MG_FORCING. */
int agx_mg_restrict(agx_ctx *fine, agx_ctx *coarse, int blk, int what,
                    const int32_t *to_coarse, const double *vol_fac);
/* linearSolver::Residual (:92-109): forcing - (A x - b) of every cell, kept as an array
 * (what AGX_MG_FORCING restricts), and its mean square as mgSolution::CycleAtLevel forms
 * it (:196-204).  The caller has swapped x across connections. */
int agx_mg_matrix_residual(agx_ctx *ctx, double *mean_square);
/* gridLevel::InvertDiagonal (gridLevel.cpp:402-406) WITHOUT InitializeMatrixUpdate: a
 * coarse level's x is the restricted one */
int agx_mg_invert_diagonal(agx_ctx *ctx);
/* gridLevel::ResetDiagonal (gridLevel.cpp:408-412) of a coarse level when an iteration
 * ends (mgSolution.cpp:236-239).  The residual of a coarse level ADDS its spectral radii to
 * the diagonal, as the reference does: a level restricted to twice within a W cycle keeps
 * what its first visit left (the reference's truth contains that). */
int agx_mg_reset_diagonal(agx_ctx *ctx);
/* coarseDu = x (mgSolution.cpp:183), kept in the context for agx_mg_prolong */
int agx_mg_save_update(agx_ctx *ctx);
/* SubtractFromUpdate + Prolongation (mgSolution.cpp:189-192, gridLevel.cpp:597-611): the
 * coarse level's correction x - coarseDu at the nodes of its cells (ConvertCellToNode
 * utility.hpp:186-330, edges and corners by their own factors, no ghost cells), interpolated
 * to the fine cells with their trilinear coefficients (coeffs [nk][nj][ni][7], host;
 * TrilinearInterp utility.hpp:356-372) and added to the fine level's x.  The coarse x is
 * left as the correction. */
int agx_mg_prolong(agx_ctx *coarse, agx_ctx *fine, int blk, const int32_t *to_coarse,
                   const double *coeffs);

/* halo exchange (multiArray3d.hpp:790-873 SwapSliceLocal / SwapSliceParallel).
 * local: both sides on this rank. */
int agx_halo_swap_local(agx_ctx *ctx, int what);
/* remote: number of doubles in the packed slab of connection conn_id */
int64_t agx_halo_count(agx_ctx *ctx, int conn_id, int what);
/* pack this rank's side of the connection into dev_buf (device pointer) */
int agx_halo_pack(agx_ctx *ctx, int conn_id, int what, double *dev_buf);
/* unpack the partner's slab from dev_buf into this rank's ghost cells */
int agx_halo_unpack(agx_ctx *ctx, int conn_id, int what, const double *dev_buf);

/* ---- multi-rank runs: agx_iterate drives remote connections itself ---------
 * In the reference a rank exchanges ghost slabs with SwapSliceParallel /
 * PackSwapUnpackMPI (multiArray3d.hpp:830-866, utility.cpp:400-423: pack,
 * MPI_Sendrecv, unpack) and reduces the norms with GlobalReduceMPI / MPI_Reduce
 * (main.cpp:254-264).  Here the library packs and unpacks on the device and
 * leaves the wire to a table of two operations.  With an exchange installed
 * agx_iterate (and agx_halo_exchange) handle connections whose partner is on
 * another rank, and the norms agx_iterate returns are the GLOBAL ones on every
 * rank: l2 summed, linf the largest with its location, matrix_resid the sum of
 * the ranks' values (what MPI_SUM of main.cpp:259 forms) -- the adapter drops
 * its own reductions.
 *   host_buffers = 0: slab pointers are device memory and the operations are
 *     stream-ordered on hip_stream (the built-in RCCL transport);
 *   host_buffers = 1: the library stages the slabs through pinned host memory
 *     and calls the operations with host pointers after synchronising (an MPI,
 *     socket or shared-memory transport: MPI_Sendrecv / MPI_Allgather fit).  */
typedef struct agx_slab {
  int32_t peer;              /* rank of the partner                          */
  int32_t tag;               /* ordinal among the connections with this peer
                              * (creation order): the same on both sides     */
  int64_t count;             /* doubles to send and to receive               */
  double *send, *recv;
} agx_slab;
typedef struct agx_exchange {
  void *user;
  /* complete (or enqueue on hip_stream) send[i] -> peer[i], recv[i] <- peer[i]
   * for all n slabs of this rank; slabs come in connection-creation order */
  int (*swap)(void *user, int n, const agx_slab *slabs, void *hip_stream);
  /* every rank contributes `bytes` bytes at send; recv gets nranks * bytes,
   * in rank order */
  int (*allgather)(void *user, const void *send, void *recv, int64_t bytes,
                   void *hip_stream);
  /* Both return 0, or non-zero for an operation that did not complete (a time-out
   * included: a callback must never report an exchange it gave up on as done).
   * A failing operation ends the agx_iterate call where it is -- nothing is posted
   * after it, the peers cannot be helped -- with "the exchange's swap / allgather
   * operation failed", or, after an earlier failure of this rank's own, that one's
   * text.  A rank that fails on its own posts what a healthy rank posts, in the
   * failing call and after it, and every rank's call returns non-zero. */
  int32_t nranks;
  int32_t host_buffers;
} agx_exchange;
int agx_set_exchange(agx_ctx *ctx, const agx_exchange *ex);
/* built-in transport: RCCL over xGMI, grouped ncclSend / ncclRecv per slab and
 * one ncclAllGather for the norms, all on the library's stream (no host sync
 * between pack and unpack).  id128: 128 bytes made by agx_rccl_unique_id on one
 * rank and handed to the others by the host (MPI_Bcast in the reference's
 * driver).  Call after agx_ctx_create, before agx_setup_finalize. */
int agx_rccl_unique_id(void *id128);
int agx_rccl_exchange_create(agx_ctx *ctx, const void *id128, int nranks, int rank);
/* one ghost exchange as gridLevel::GetBoundaryConditions / lusgs::Relax place it:
 * local connections + (with an exchange installed) remote ones */
int agx_halo_exchange(agx_ctx *ctx, int what);

/* ---- measurement helpers ----------------------------------------------- */
/* average duration [ms] of the named kernel group since the last reset,
 * measured with hipEvents on the library's stream; group: 0 = inviscid residual
 * (+ fused explicit stage), 1 = update + norms, 2 = ghost cells / halo,
 * 3 = LU-SGS / DPLUR sweeps, 4 = viscous residual, 5 = implicit begin
 * (diagonal, right-hand side; no launch is counted where the viscous residual of
 * agx_iterate wrote both itself, and then group 4 carries it), 6 = matrix residual */
int agx_timing_enable(agx_ctx *ctx, int on);
int agx_timing_get(agx_ctx *ctx, int group, double *avg_ms, int64_t *launches);
int agx_timing_reset(agx_ctx *ctx);
int agx_sync(agx_ctx *ctx);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* AITHER_GFX950_H */
