// agx_series.hpp -- time series at chosen cells and wall faces, recorded on the device
// (include/aither_gfx950.h, AGX_FIELD_SERIES_PLAN / _SAMPLE / _ROWS / _LOCATE).
//
// A block's plan names V variables and P points of one kind -- physical cells or faces of the
// wall payload -- and owns a ring of `capacity` rows of V x P doubles in device memory
// (agx_series_ring.hpp has the ring's arithmetic).  A sample is one launch that gathers the
// V x P values into the next row, [v * P + p], with the evaluators of the output packs: what
// agx_output_pack with the plan's ids would deliver at those points at that moment,
// dimensional.  The launch is enqueued on the context's stream and nothing waits for it: no
// synchronisation, no copy to the host, no allocation between two time steps.  The host
// collects the rows in bulk.  No atomics: a value is a function of its point alone, so the same
// call gives the same bits.
//
// The sample kernels are gathers of a few thousand threads, a launch and a chain of dependent
// loads each; thread t = p * V + v, so the V threads of a point are neighbouring lanes whose
// loads of the point's state are the same addresses, one request of the wave.
#pragma once
#include "agx_kernels.hpp"
#include "agx_stats.hpp"

namespace agx {

// One thread per (point, variable) of a cell plan.  pts[p]: the cell's dense index
// (k nj + j) ni + i.  A thread whose variable is a gradient forms the 3 NGF gradients of its
// own cell (cell_grads18, as k_cell_grads does for every cell of the block); no other thread
// does, and no plane of gradients exists.
__global__ void __launch_bounds__(256)
k_series_cells(BlockDev b, GasDev g, OutSpec sp, const long* __restrict__ pts, long npts,
               double* __restrict__ row) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npts * sp.nvar) return;
  const long p = t / sp.nvar;
  const int v = (int)(t - p * sp.nvar);
  const long cell = pts[p];
  const int i = (int)(cell % b.ni), j = (int)((cell / b.ni) % b.nj),
            k = (int)(cell / ((long)b.ni * b.nj));
  const long q = b.idx(i, j, k);
  // (the point as k_output_pack forms it)
  OutPoint pt;
  load5(b.state, q, pt.s);
  pt.t = pt.s[4] / (pt.s[0] * g.R);
  pt.mu = out_sutherland(g, pt.t);
  out_point(g, pt);
  const int var = sp.var[v];
  double acc[3 * NGF];
  const bool grad = var >= AGX_OUT_VELGRAD && var < AGX_OUT_RESID;
  if (grad) cell_grads18(b, g, q, acc);
  const CellSource src{b, q, grad ? acc : nullptr};
  row[(long)v * npts + p] = out_value(var, pt, sp, src);
}

// Wall variable `var` of the filled wallVars of a face: the switch of k_wall_pack, factor by
// factor (output.cpp:519-553)
__device__ __forceinline__ double series_wall_value(int var, const WallVars& w, const GasDev& g,
                                                    const OutSpec& sp) {
  const double rR = sp.rho_ref, aR = sp.a_ref, lR = sp.l_ref, tR = sp.t_ref, muR = sp.mu_ref;
  const double tau_sc = (1.0 / g.scaling) * muR * aR / lR;
  switch (var) {
    case AGX_WALL_YPLUS: return w.yplus;
    case AGX_WALL_SHEAR_STRESS: return sqrt(dot3(w.shear, w.shear)) * tau_sc;
    case AGX_WALL_VISCOSITY_RATIO: return w.turb_eddy_visc / (w.viscosity + AGX_EPS);
    case AGX_WALL_HEAT_FLUX: return w.heat_flux * (muR * tR / lR);
    case AGX_WALL_FRICTION_VELOCITY: return w.friction_velocity * aR;
    case AGX_WALL_DENSITY: return w.density * rR;
    case AGX_WALL_PRESSURE: return wall_face_pressure(g, w) * (rR * aR * aR);
    case AGX_WALL_TEMPERATURE: return w.temperature * tR;
    case AGX_WALL_VISCOSITY: return w.viscosity * (muR * (1.0 / g.scaling));
    case AGX_WALL_TKE: return w.tke * (aR * aR);
    case AGX_WALL_SDR: return w.sdr * (aR * aR * rR / muR);
    case AGX_WALL_SHEAR_X: return w.shear[0] * tau_sc;
    case AGX_WALL_SHEAR_Y: return w.shear[1] * tau_sc;
    case AGX_WALL_SHEAR_Z: return w.shear[2] * tau_sc;
  }
  return 0.0;
}
// One thread per (point, variable) of a wall plan.  pts[p]: the face's index in the block's
// wall payload (k_wall_pack's order), found in the wall table as k_stats_wall finds it.
// fourth: bit 0 centralFourth, bit 1 a largeEddySimulation run (wall_face_vars).
__global__ void __launch_bounds__(256)
k_series_wall(BlockDev b, GasDev g, OutSpec sp, const WallSurfDev* __restrict__ tab, int nsurf,
              int fourth, const long* __restrict__ pts, long npts, double* __restrict__ row) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npts * sp.nvar) return;
  const long p = t / sp.nvar;
  const int v = (int)(t - p * sp.nvar);
  const StatWallFace f = stat_wall_face(b, tab, nsurf, pts[p]);
  // (through a copy, as k_wall_pack reads it: the same contraction of |tau|^2)
  WallVars wt;
  wall_face_vars(b, g, f.d, f.side, f.fi, f.fj, f.fk, f.qU, f.qL, fourth, wt);
  const WallVars w = wt;
  row[(long)v * npts + p] = series_wall_value(sp.var[v], w, g, sp);
}

// The physical cell of the block whose centre is nearest to each of npts points, exhaustive
// (points x cells).  A workgroup owns PPW points, held in registers, so that the three loads of
// a centre serve PPW distance evaluations; its 256 threads walk the cells in ascending dense
// index c = (k nj + j) ni + i with a stride of 256, (i, j, k) carried along by additions.
// TIE RULE: among cells at equal squared distance the LOWEST dense index wins.  A thread
// replaces its (d2, c) on a strictly smaller d2 only, so it keeps the lowest c of its own
// cells; the workgroup's reduction (LDS, halving) takes the smaller d2 and, on equality, the
// smaller c.  No atomics.  d2 is dx dx + dy dy + dz dz of centre - point; the compiler may
// contract it, with the caveat k_cloud_nearest states.  The caller has bounded the coordinates
// so that d2 is finite: a thread without cells (ncell is no multiple of 256) carries
// (infinity, LONG_MAX) and never wins.
// out[4 p ...]: i, j, k, d2.
constexpr int SERIES_LOCATE_PPW = 8;
template <int PPW>
__global__ void __launch_bounds__(256)
k_series_locate(BlockDev b, long npts, const double* __restrict__ pts, double* __restrict__ out) {
  __shared__ double sd[256];
  __shared__ long sc[256];
  const long nij = (long)b.ni * b.nj, ncell = nij * b.nk;
  const long p0 = (long)blockIdx.x * PPW;
  double x[PPW][3], best[PPW];
  long id[PPW];
#pragma unroll
  for (int n = 0; n < PPW; ++n) {
    const long p = min(p0 + n, npts - 1);
    x[n][0] = pts[3 * p]; x[n][1] = pts[3 * p + 1]; x[n][2] = pts[3 * p + 2];
    best[n] = __builtin_huge_val();
    id[n] = 0x7fffffffffffffffL;
  }
  // the thread's first cell, and what 256 cells further is in (i, j, k)
  long c = threadIdx.x;
  int i = (int)(c % b.ni), j = (int)((c / b.ni) % b.nj), k = (int)(c / nij);
  const int sk = (int)(256 / nij), sj = (int)((256 % nij) / b.ni), si = (int)((256 % nij) % b.ni);
  for (; c < ncell; c += 256) {
    const long q = b.idx(i, j, k);
    const double cx = b.cen[0][q], cy = b.cen[1][q], cz = b.cen[2][q];
#pragma unroll
    for (int n = 0; n < PPW; ++n) {
      const double d[3] = {cx - x[n][0], cy - x[n][1], cz - x[n][2]};
      const double d2 = dot3(d, d);
      if (d2 < best[n]) { best[n] = d2; id[n] = c; }
    }
    i += si;
    if (i >= b.ni) { i -= b.ni; ++j; }
    j += sj;
    if (j >= b.nj) { j -= b.nj; ++k; }
    k += sk;
  }
#pragma unroll
  for (int n = 0; n < PPW; ++n) {
    __syncthreads();
    sd[threadIdx.x] = best[n];
    sc[threadIdx.x] = id[n];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) {
        const double d2 = sd[threadIdx.x + w];
        const long c2 = sc[threadIdx.x + w];
        if (d2 < sd[threadIdx.x] || (d2 == sd[threadIdx.x] && c2 < sc[threadIdx.x])) {
          sd[threadIdx.x] = d2;
          sc[threadIdx.x] = c2;
        }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0 && p0 + n < npts) {
      const long cw = sc[0];
      double* o = out + 4 * (p0 + n);
      o[0] = (double)(cw % b.ni);
      o[1] = (double)((cw / b.ni) % b.nj);
      o[2] = (double)(cw / nij);
      o[3] = sd[0];
    }
  }
}

}  // namespace agx
