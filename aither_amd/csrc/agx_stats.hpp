// agx_stats.hpp -- running time statistics on the device (include/aither_gfx950.h,
// AGX_FIELD_STAT_SAMPLE / AGX_FIELD_STAT_ACCUM, AGX_STAT_*, AGX_WSTAT_*).
//
// Every physical cell, and every viscousWall face, carries running means and second central
// co-moments of a sampled vector x, advanced by the weighted one-pass recurrence of West
// (1979).  With the sample's weight w and the weights' sum W (the new sample included):
//     delta_a = x_a - mean_a                  (the mean BEFORE the sample)
//     mean_a  = mean_a + (w / W) delta_a
//     C_ab    = C_ab + (w (1 - w / W) delta_a) delta_b
// and the covariance is C_ab / W.  No sums of squares (E[x^2] - E[x]^2 has no digits left at
// the turbulence intensities an LES resolves), no atomics, no reduction across cells: a cell
// is a function of its own history, so two runs give the same bits.  W and the sample count
// are the host's; the kernels get r = w / W and cf = w (1 - w / W).  With zeroed accumulators
// and r = 1 the first sample gives mean = x, C = 0 exactly; identical samples keep both.
//
// Sampled vector of a cell (nondimensional): rho, u, v, w, p, T = p / (rho R) as the output
// pack forms it, rho u, rho v, rho w, then NX extras: the eddy viscosity of the last residual
// (largeEddySimulation runs and the 7-equation libraries), k and omega (7 equations).
// Planes: NM = 9 + NX means, then uu uv uw vv vw ww, var rho, var p, var T.
// Accumulator planes are dense over the physical cells, [plane][k][j][i], at a pitch of the
// cell count rounded up to even, so that a thread's two cells are one 16-byte access in
// every plane whatever the block's shape; the state planes are ghost-padded and are read
// with plain 8-byte loads.
#pragma once
#include "agx_kernels.hpp"

namespace agx {

constexpr int STAT_NSECOND = 9;        // second-moment planes of a cell
constexpr int STAT_NWALL_MEAN = AGX_WALL_END - AGX_WALL_YPLUS;   // 14
constexpr int STAT_NWALL = STAT_NWALL_MEAN + 4;                  // + var p, var tau_x/y/z

// One sample into the cell accumulators: a thread owns the dense cells 2 t and 2 t + 1.  The
// source places all loads of the thread -- 2 x (5 + NX) state values, 18 + NX accumulator
// pairs -- before the first use, the read-modify-write of the accumulators being the whole
// cost; the schedule is the compiler's (for NX = 1 it issues the 12 state loads and 7 of the 19
// accumulator pairs at once and the other 12 pairs in three groups behind the first uses;
// DESIGN section 8 has the measured share of the roofline that gives).
template <int NX, class Index>
__device__ __forceinline__ void stats_cells_body(const BlockDev& b, const GasDev& g, long ncell,
                                                 long pitch, double r, double cf,
                                                 double* __restrict__ acc) {
  constexpr int NM = 9 + NX, NP = NM + STAT_NSECOND;
  const long p0 = 2 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  if (p0 >= ncell) return;
  // (i, j, k) of the first cell; the second is its successor in the dense order
  const Index ni = (Index)b.ni, nj = (Index)b.nj;
  const Index row = (Index)p0 / ni;
  int i = (int)((Index)p0 - row * ni), k = (int)(row / nj);
  int j = (int)(row - (Index)k * nj);
  long q[2];
  q[0] = b.idx(i, j, k);
  if (++i == b.ni) { i = 0; if (++j == b.nj) { j = 0; ++k; } }
  // (an odd cell count: the last thread's second slot is the pad of the pitch, kept at zero)
  const bool two = p0 + 1 < ncell;
  q[1] = two ? b.idx(i, j, k) : q[0];
  double s[2][AGX_NEQ], ev[2] = {0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    load5(b.state, q[c], s[c]);
    if constexpr (NX >= 1) ev[c] = b.turb3[0][q[c]];
  }
  double2 a[NP];
#pragma unroll
  for (int n = 0; n < NP; ++n) a[n] = *reinterpret_cast<const double2*>(acc + n * pitch + p0);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    // No contraction in the recurrence: fma(rho, u, -mean) is the rounding error of the
    // product, not the 0 that identical samples must give.
#pragma clang fp contract(off)
    double x[NM];
    for (int e = 0; e < 5; ++e) x[e] = s[c][e];
    x[5] = s[c][4] / (s[c][0] * g.R);
    for (int e = 0; e < 3; ++e) x[6 + e] = s[c][0] * s[c][1 + e];
    if constexpr (NX >= 1) x[9] = ev[c];
#if AGX_NEQ == 7
    if constexpr (NX >= 3) { x[10] = s[c][5]; x[11] = s[c][6]; }
#endif
    if (c == 1 && !two)
      for (int n = 0; n < NM; ++n) x[n] = 0.0;
    double d[NM];
#pragma unroll
    for (int n = 0; n < NM; ++n) {
      double& m = c == 0 ? a[n].x : a[n].y;
      d[n] = x[n] - m;
      m = m + r * d[n];
    }
    // uu uv uw vv vw ww, rho rho, p p, T T
    constexpr int A[STAT_NSECOND] = {1, 1, 1, 2, 2, 3, 0, 4, 5};
    constexpr int B[STAT_NSECOND] = {1, 2, 3, 2, 3, 3, 0, 4, 5};
#pragma unroll
    for (int n = 0; n < STAT_NSECOND; ++n) {
      double& cm = c == 0 ? a[NM + n].x : a[NM + n].y;
      cm = cm + (cf * d[A[n]]) * d[B[n]];
    }
  }
#pragma unroll
  for (int n = 0; n < NP; ++n) *reinterpret_cast<double2*>(acc + n * pitch + p0) = a[n];
}
template <int NX>
__global__ void __launch_bounds__(256)
k_stats_cells(BlockDev b, GasDev g, long ncell, long pitch, double r, double cf,
              double* __restrict__ acc) {
  // (32-bit index arithmetic wherever the block allows it: two divisions per thread)
  if (ncell < (1L << 31)) stats_cells_body<NX, unsigned>(b, g, ncell, pitch, r, cf, acc);
  else stats_cells_body<NX, long>(b, g, ncell, pitch, r, cf, acc);
}

// the face of thread t of a launch over the viscousWall faces of a block (k_wall_pack's order)
struct StatWallFace { int d, side, fi, fj, fk; long qU, qL; };
__device__ __forceinline__ StatWallFace stat_wall_face(const BlockDev& b,
                                                       const WallSurfDev* __restrict__ tab,
                                                       int nsurf, long t) {
  int sn = 0;
  while (sn + 1 < nsurf && t >= tab[sn + 1].off) ++sn;
  const WallSurfDev ws = tab[sn];
  const long r = t - ws.off;
  StatWallFace f;
  f.fi = ws.lo[0] + (int)(r % ws.n[0]);
  f.fj = ws.lo[1] + (int)((r / ws.n[0]) % ws.n[1]);
  f.fk = ws.lo[2] + (int)(r / ((long)ws.n[0] * ws.n[1]));
  f.side = ws.side;
  f.d = (ws.side - 1) / 2;
  f.qU = b.idx(f.fi, f.fj, f.fk);
  f.qL = f.qU - b.stride(f.d);
  return f;
}
// One sample into the wall accumulators, [STAT_NWALL][total]: the 14 wall variables of
// wall_face_vars (what k_wall_pack hands out, before its dimensional factors), then the second
// central moments of the wall pressure and the three shear components.  Surface-sized.
__global__ void __launch_bounds__(256)
k_stats_wall(BlockDev b, GasDev g, const WallSurfDev* __restrict__ tab, int nsurf, long total,
             int fourth, double r, double cf, double* __restrict__ acc) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const StatWallFace f = stat_wall_face(b, tab, nsurf, t);
  // (through a copy, as k_wall_pack reads it: the same contraction of |tau|^2)
  WallVars wt;
  wall_face_vars(b, g, f.d, f.side, f.fi, f.fj, f.fk, f.qU, f.qL, fourth, wt);
  const WallVars w = wt;
  double x[STAT_NWALL_MEAN];
  x[AGX_WALL_YPLUS - AGX_WALL_YPLUS] = w.yplus;
  x[AGX_WALL_SHEAR_STRESS - AGX_WALL_YPLUS] = sqrt(dot3(w.shear, w.shear));
  x[AGX_WALL_VISCOSITY_RATIO - AGX_WALL_YPLUS] = w.turb_eddy_visc / (w.viscosity + AGX_EPS);
  x[AGX_WALL_HEAT_FLUX - AGX_WALL_YPLUS] = w.heat_flux;
  x[AGX_WALL_FRICTION_VELOCITY - AGX_WALL_YPLUS] = w.friction_velocity;
  x[AGX_WALL_DENSITY - AGX_WALL_YPLUS] = w.density;
  x[AGX_WALL_PRESSURE - AGX_WALL_YPLUS] = wall_face_pressure(g, w);
  x[AGX_WALL_TEMPERATURE - AGX_WALL_YPLUS] = w.temperature;
  x[AGX_WALL_VISCOSITY - AGX_WALL_YPLUS] = w.viscosity;
  x[AGX_WALL_TKE - AGX_WALL_YPLUS] = w.tke;
  x[AGX_WALL_SDR - AGX_WALL_YPLUS] = w.sdr;
  for (int c = 0; c < 3; ++c) x[AGX_WALL_SHEAR_X - AGX_WALL_YPLUS + c] = w.shear[c];
  {
    // (no contraction, as in the cells: rho R T - mean must be 0 for identical samples)
#pragma clang fp contract(off)
    double d[STAT_NWALL_MEAN];
#pragma unroll
    for (int n = 0; n < STAT_NWALL_MEAN; ++n) {
      const double m = acc[n * total + t];
      d[n] = x[n] - m;
      acc[n * total + t] = m + r * d[n];
    }
    constexpr int A[4] = {AGX_WALL_PRESSURE - AGX_WALL_YPLUS, AGX_WALL_SHEAR_X - AGX_WALL_YPLUS,
                          AGX_WALL_SHEAR_Y - AGX_WALL_YPLUS, AGX_WALL_SHEAR_Z - AGX_WALL_YPLUS};
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      double* cm = acc + (STAT_NWALL_MEAN + n) * total + t;
      *cm = *cm + (cf * d[A[n]]) * d[A[n]];
    }
  }
}

// The statistics of the cells, dimensional (ids relative to AGX_STAT_BASE in sp.var): a mean
// times the factor k_output_pack gives the variable, in its order of operations, so that the
// mean of identical samples is the packed variable bit for bit; a second moment C / W times
// the product of its two factors.  nm: the mean planes of this context.
__device__ __forceinline__ double stat_cell_value(int id, double a, double W, const OutSpec& sp) {
  const double rR = sp.rho_ref, aR = sp.a_ref, tR = sp.t_ref, muR = sp.mu_ref;
  switch (id) {
    case 0: return a * rR;
    case 1: case 2: case 3: return a * aR;
    case 4: return a * rR * aR * aR;
    case 5: return a * tR;
    case 6: case 7: case 8: return a * (rR * aR);
    case 9: return a * muR;
    case 10: return a * aR * aR;
    case 11: return a * aR * aR * rR / muR;
    case 18: return a / W * (rR * rR);
    case 19: return a / W * ((rR * aR * aR) * (rR * aR * aR));
    case 20: return a / W * (tR * tR);
  }
  return a / W * (aR * aR);       // 12 .. 17: the velocity co-moments
}
__global__ void __launch_bounds__(256)
k_stats_pack(long ncell, long pitch, int nm, double W, OutSpec sp, const double* __restrict__ acc,
             double* __restrict__ out) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= ncell) return;
  for (int v = 0; v < sp.nvar; ++v) {
    const int id = sp.var[v];
    const int plane = id < 12 ? id : nm + (id - 12);
    out[(long)v * ncell + p] = stat_cell_value(id, acc[plane * pitch + p], W, sp);
  }
}
// ---- the statistics collapsed along index directions (AGX_CSTAT_BASE) --------------------------
// A bin is one position of the directions that remain; its cells are pooled with their volumes
// by the same one-pass recurrence, in space:
//     V += v;  r = v / V;  cf = v (1 - r);  delta = m - M
//     M += r delta;   T_ab += r (C_ab - T_ab);   D_ab += (cf delta_a) delta_b
// and two partial bins join by the pairwise form (cstat_join).  cov_ab = T_ab / W + D_ab / V is
// the co-moment about the space-time mean.  Cells with bit-identical m and C give M = m,
// T = C and D = 0 exactly, whatever their volumes.
// Shape of the sum (fixed by the extents and the mask alone; no atomics): the collapsed j and
// k positions of a bin are its MARCH, k outer, j inner, cut into chunks of CSTAT_CHUNK steps.
// i kept: a thread per (chunk, bin) takes one cell per step, neighbouring threads neighbouring
// i.  i collapsed: a wave per (chunk, bin); per step lane l takes the row's cells l, l + 64, ...,
// and after the chunk the 64 lane partials join by a butterfly, the lower lane first.  Each
// (chunk, bin) leaves a record of CSTAT_NQ(NM) values in part[(chunk * NQ + q) * nbin + bin]:
// V, M[NM], T[9], D[9]; k_cstat_join joins a bin's records in ascending chunk order, one
// thread per (bin, requested id), and makes the value dimensional.  Every quantity is a
// function of the volumes and of its own planes, so a subset of ids returns the same bits.
constexpr int CSTAT_CHUNK = 64;
constexpr int CSTAT_VOLUME = 21;       // id of the bin's volume, after the 21 of AGX_STAT_BASE
__host__ __device__ constexpr int cstat_nq(int nm) { return 1 + nm + 2 * STAT_NSECOND; }
// the two means of a second moment (uu uv uw vv vw ww, rho rho, p p, T T)
__host__ __device__ constexpr int stat_second_a(int n) {
  constexpr int A[STAT_NSECOND] = {1, 1, 1, 2, 2, 3, 0, 4, 5};
  return A[n];
}
__host__ __device__ constexpr int stat_second_b(int n) {
  constexpr int B[STAT_NSECOND] = {1, 2, 3, 2, 3, 3, 0, 4, 5};
  return B[n];
}
struct CstatSpec {
  int mask;                // collapsed directions, bit 0 = i, 1 = j, 2 = k
  unsigned means, seconds; // the planes to pool: bit n = mean n / second moment n
  long pitch;              // of the accumulator planes
  long nbin, nchunk, steps;
};
// r of a join or a step: V2 / (V1 + V2); two empty partials (lanes beyond a short row) join
// as the identity
__device__ __forceinline__ double cstat_ratio(double v2, double vsum) {
  return vsum == 0.0 ? 0.0 : v2 / vsum;
}
template <int NM>
struct CstatPartial {
  double V, M[NM], T[STAT_NSECOND], D[STAT_NSECOND];
};
template <int NM>
__device__ __forceinline__ void cstat_join(CstatPartial<NM>& a, const CstatPartial<NM>& b,
                                           unsigned means, unsigned seconds) {
#pragma clang fp contract(off)
  const double V = a.V + b.V, r = cstat_ratio(b.V, V), cf = a.V * r;
  double d[NM];
#pragma unroll
  for (int n = 0; n < NM; ++n)
    if (means >> n & 1) {
      d[n] = b.M[n] - a.M[n];
      a.M[n] = a.M[n] + r * d[n];
    }
#pragma unroll
  for (int n = 0; n < STAT_NSECOND; ++n)
    if (seconds >> n & 1) {
      a.T[n] = a.T[n] + r * (b.T[n] - a.T[n]);
      a.D[n] = a.D[n] + b.D[n] + (cf * d[stat_second_a(n)]) * d[stat_second_b(n)];
    }
  a.V = V;
}
template <int NX>
__global__ void __launch_bounds__(256)
k_cstat_partial(BlockDev b, CstatSpec cs, const double* __restrict__ acc,
                double* __restrict__ part) {
  constexpr int NM = 9 + NX, NQ = cstat_nq(NM);
  const bool over_i = cs.mask & 1;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const long unit = over_i ? t >> 6 : t;       // (uniform over a wave where i is collapsed)
  if (unit >= cs.nbin * cs.nchunk) return;
  const long bin = unit % cs.nbin, chunk = unit / cs.nbin;
  // the bin's position in the directions that remain, 0 in the collapsed ones
  const int ni_rem = over_i ? 1 : b.ni, nj_rem = cs.mask & 2 ? 1 : b.nj;
  const int i0 = (int)(bin % ni_rem);
  const long rest = bin / ni_rem;
  const int j0 = (int)(rest % nj_rem), k0 = (int)(rest / nj_rem);
  const int cj = cs.mask & 2 ? b.nj : 1;
  const long s0 = chunk * CSTAT_CHUNK;
  const long s1 = s0 + CSTAT_CHUNK < cs.steps ? s0 + CSTAT_CHUNK : cs.steps;
  int js = (int)(s0 % cj), ks = (int)(s0 / cj);
  CstatPartial<NM> p;
  p.V = 0.0;
#pragma unroll
  for (int n = 0; n < NM; ++n) p.M[n] = 0.0;
#pragma unroll
  for (int n = 0; n < STAT_NSECOND; ++n) p.T[n] = p.D[n] = 0.0;
  const int i_first = over_i ? lane : i0, i_step = over_i ? 64 : b.ni;
  for (long s = s0; s < s1; ++s) {
    const int j = j0 + js, k = k0 + ks;
    const long row = ((long)k * b.nj + j) * b.ni;
    for (int i = i_first; i < b.ni; i += i_step) {
      const double v = b.vol[b.idx(i, j, k)];
      const double* a = acc + row + i;
      double m[NM], c[STAT_NSECOND];
#pragma unroll
      for (int n = 0; n < NM; ++n)
        if (cs.means >> n & 1) m[n] = a[n * cs.pitch];
#pragma unroll
      for (int n = 0; n < STAT_NSECOND; ++n)
        if (cs.seconds >> n & 1) c[n] = a[(NM + n) * cs.pitch];
      {
        // (no contraction, as in k_stats_cells: identical cells must leave delta = 0)
#pragma clang fp contract(off)
        p.V = p.V + v;
        const double r = cstat_ratio(v, p.V), cf = v * (1.0 - r);
        double d[NM];
#pragma unroll
        for (int n = 0; n < NM; ++n)
          if (cs.means >> n & 1) {
            d[n] = m[n] - p.M[n];
            p.M[n] = p.M[n] + r * d[n];
          }
#pragma unroll
        for (int n = 0; n < STAT_NSECOND; ++n)
          if (cs.seconds >> n & 1) {
            p.T[n] = p.T[n] + r * (c[n] - p.T[n]);
            p.D[n] = p.D[n] + (cf * d[stat_second_a(n)]) * d[stat_second_b(n)];
          }
      }
    }
    if (++js == cj) { js = 0; ++ks; }
  }
  if (over_i) {
    // the 64 lane partials of the wave: 6 steps, both lanes of a pair forming join(lower,
    // upper), so that every lane ends with the same bits
    for (int w = 1; w < 64; w <<= 1) {
      CstatPartial<NM> o;
      o.V = __shfl_xor(p.V, w);
#pragma unroll
      for (int n = 0; n < NM; ++n)
        if (cs.means >> n & 1) o.M[n] = __shfl_xor(p.M[n], w);
#pragma unroll
      for (int n = 0; n < STAT_NSECOND; ++n)
        if (cs.seconds >> n & 1) {
          o.T[n] = __shfl_xor(p.T[n], w);
          o.D[n] = __shfl_xor(p.D[n], w);
        }
      if (lane & w) {
        cstat_join<NM>(o, p, cs.means, cs.seconds);
        p = o;
      } else {
        cstat_join<NM>(p, o, cs.means, cs.seconds);
      }
    }
    if (lane != 0) return;
  }
  double* rec = part + chunk * NQ * cs.nbin + bin;
  rec[0] = p.V;
#pragma unroll
  for (int n = 0; n < NM; ++n)
    if (cs.means >> n & 1) rec[(1 + n) * cs.nbin] = p.M[n];
#pragma unroll
  for (int n = 0; n < STAT_NSECOND; ++n)
    if (cs.seconds >> n & 1) {
      rec[(1 + NM + n) * cs.nbin] = p.T[n];
      rec[(1 + NM + STAT_NSECOND + n) * cs.nbin] = p.D[n];
    }
}
// One thread per (bin, requested id): the bin's chunk records joined in ascending order,
// cov = T / W + D / V, then the factors of stat_cell_value; the volume times l_ref^3.
__global__ void __launch_bounds__(64)
k_cstat_join(CstatSpec cs, int nm, double W, OutSpec sp, const double* __restrict__ part,
             double* __restrict__ out) {
  const long bin = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (bin >= cs.nbin) return;
  const int id = sp.var[blockIdx.y], nq = cstat_nq(nm);
  const bool second = id >= 12 && id < CSTAT_VOLUME, mean = id < 12;
  const int sn = second ? id - 12 : 0;
  const int qa = 1 + (second ? stat_second_a(sn) : mean ? id : 0);
  const int qb = 1 + (second ? stat_second_b(sn) : mean ? id : 0);
  double V = 0.0, Ma = 0.0, Mb = 0.0, T = 0.0, D = 0.0;
  for (long ch = 0; ch < cs.nchunk; ++ch) {
#pragma clang fp contract(off)
    const double* rec = part + ch * nq * cs.nbin + bin;
    const double V2 = rec[0], Vs = V + V2, r = cstat_ratio(V2, Vs);
    if (id != CSTAT_VOLUME) {
      const double da = rec[qa * cs.nbin] - Ma, db = rec[qb * cs.nbin] - Mb;
      Ma = Ma + r * da;
      Mb = Mb + r * db;
      if (second) {
        T = T + r * (rec[(1 + nm + sn) * cs.nbin] - T);
        D = D + rec[(1 + nm + STAT_NSECOND + sn) * cs.nbin] + ((V * r) * da) * db;
      }
    }
    V = Vs;
  }
  double val;
  {
#pragma clang fp contract(off)
    if (id == CSTAT_VOLUME) val = V * (sp.l_ref * sp.l_ref * sp.l_ref);
    else if (mean) val = stat_cell_value(id, Ma, W, sp);
    else val = stat_cell_value(id, T / W + D / V, 1.0, sp);
  }
  out[(long)blockIdx.y * cs.nbin + bin] = val;
}

// ... and of the wall faces (ids relative to AGX_WSTAT_BASE): the factors of k_wall_pack
__device__ __forceinline__ double stat_wall_factor(int v, const GasDev& g, const OutSpec& sp) {
  const double rR = sp.rho_ref, aR = sp.a_ref, lR = sp.l_ref, tR = sp.t_ref, muR = sp.mu_ref;
  const double tau_sc = (1.0 / g.scaling) * muR * aR / lR;
  switch (v + AGX_WALL_YPLUS) {
    case AGX_WALL_SHEAR_STRESS: case AGX_WALL_SHEAR_X: case AGX_WALL_SHEAR_Y:
    case AGX_WALL_SHEAR_Z: return tau_sc;
    case AGX_WALL_HEAT_FLUX: return muR * tR / lR;
    case AGX_WALL_FRICTION_VELOCITY: return aR;
    case AGX_WALL_DENSITY: return rR;
    case AGX_WALL_PRESSURE: return rR * aR * aR;
    case AGX_WALL_TEMPERATURE: return tR;
    case AGX_WALL_VISCOSITY: return muR * (1.0 / g.scaling);
    case AGX_WALL_TKE: return aR * aR;
    case AGX_WALL_SDR: return aR * aR * rR / muR;
  }
  return 1.0;                     // yplus, viscosityRatio
}
__global__ void __launch_bounds__(256)
k_stats_wall_pack(long total, double W, GasDev g, OutSpec sp, const double* __restrict__ acc,
                  double* __restrict__ out) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  for (int v = 0; v < sp.nvar; ++v) {
    const int id = sp.var[v];
    const double a = acc[(long)id * total + t];
    double val;
    if (id < STAT_NWALL_MEAN) {
      const double fac = stat_wall_factor(id, g, sp);
      // (yplus and viscosityRatio go out as they are, like k_wall_pack's)
      val = (id == 0 || id == AGX_WALL_VISCOSITY_RATIO - AGX_WALL_YPLUS) ? a : a * fac;
    } else {
      const int of = id == STAT_NWALL_MEAN ? AGX_WALL_PRESSURE - AGX_WALL_YPLUS
                                           : AGX_WALL_SHEAR_X - AGX_WALL_YPLUS;
      const double fac = stat_wall_factor(of, g, sp);
      val = a / W * (fac * fac);
    }
    out[(long)v * total + t] = val;
  }
}

}  // namespace agx
