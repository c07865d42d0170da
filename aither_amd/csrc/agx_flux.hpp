// agx_flux.hpp -- what crosses the boundary of a block, and the block's balance
// (include/aither_gfx950.h, AGX_FLUX_*, AGX_BUDGET_*; no counterpart in the reference).
//
// The residual of a cell is -F_lo + F_up of the inviscid flux per direction (k_inv_residual,
// procBlock.cpp:447-463) and +F_lo - F_up of the viscous one (k_visc_residual,
// procBlock.cpp:1392-1430), so the residual summed over the physical cells of a block is the
// sum of the outward fluxes through its boundary faces, equation by equation, wherever there
// is no source term.  The two surface kernels evaluate exactly those boundary faces with the
// per-face helpers of the gather-form residual kernels: k_surface_flux with face_flux_1d on
// the configured reconstruction and flux, k_surface_flux_visc with visc_face (its WALE arm in
// largeEddySimulation contexts) or rans_face (the stored wall data at wall-law faces).  They
// are two launches because a residual of a viscous context takes its two fluxes from two
// ghost fills: the inviscid flux sees a viscousWall as a slip wall (AssignInviscidGhostCells),
// the viscous flux sees the viscous-wall fill that follows it.  k_block_budget sums the
// residual planes, the conserved variables and the volume of the physical cells.
//
// All are two-stage sums without floating-point atomics, of a shape fixed by the surfaces
// (the extents) alone, and form all 15 sums on every call: any subset, order or repetition of
// ids returns the bits of the full call.
#pragma once
#include "agx_kernels.hpp"

namespace agx {

enum { FLUX_NQ = AGX_FLUX_END - AGX_FLUX_BASE, FLUX_CHUNK = 256, FLUX_NE = 7 };
static_assert(FLUX_NQ == 1 + 2 * FLUX_NE && AGX_BUDGET_END - AGX_BUDGET_BASE == FLUX_NQ,
              "area | inviscid[7] | viscous[7] and volume | total[7] | residual[7]");
// A flux surface: any surface agx_block_set_bcs received whose ghost cells this rank fills
// (every BC type, local connections included), cut into chunks of FLUX_CHUNK faces of its own.
struct FluxSurfDev {
  int lo[3], n[3];     // first face / cell index and count per direction (1 across the surface)
  int side;            // surface type 1..6
  long chunk0;         // its first chunk
};
// The dimensional factor of conserved variable e (what k_restart_pack gives consVarsNm1):
// rho_ref | rho_ref a_ref (x3) | rho_ref a_ref^2 (energy, rho k) | rho_ref^2 a_ref^2 / mu_ref.
// A flux or a residual sum carries a_ref l_ref^2 more, a total l_ref^3.
__device__ __forceinline__ double cons_scale(const OutSpec& sp, int e) {
  const double rR = sp.rho_ref, aR = sp.a_ref;
  return e == 0 ? rR : e < 4 ? rR * aR : e < 6 ? rR * aR * aR : rR * rR * aR * aR / sp.mu_ref;
}

// The face of a thread: one thread per face of a chunk, a workgroup per chunk (blockIdx.x).
// The faces of an i-surface lie a row pitch apart (one value per 128-byte line): surface-sized
// work, read as it lies.  false: a padding thread of the surface's last chunk.
struct FluxFace {
  int d, fi, fj, fk;
  long qU;            // the face is the lower d-face of this cell: a physical cell on a lower
                      // side, the first ghost cell on an upper one
  double sg;          // +1 on upper sides, -1 on lower ones: out of the block
};
__device__ __forceinline__ bool flux_face(const BlockDev& b, const FluxSurfDev* __restrict__ tab,
                                          int nsurf, FluxFace& f) {
  const long ch = blockIdx.x;
  int sn = 0;
  while (sn + 1 < nsurf && ch >= tab[sn + 1].chunk0) ++sn;
  const FluxSurfDev fs = tab[sn];
  const long r = (ch - fs.chunk0) * FLUX_CHUNK + threadIdx.x;
  if (r >= (long)fs.n[0] * fs.n[1] * fs.n[2]) return false;
  f.fi = fs.lo[0] + (int)(r % fs.n[0]);
  f.fj = fs.lo[1] + (int)((r / fs.n[0]) % fs.n[1]);
  f.fk = fs.lo[2] + (int)(r / ((long)fs.n[0] * fs.n[1]));
  f.d = (fs.side - 1) / 2;
  f.qU = b.idx(f.fi, f.fj, f.fk);
  f.sg = fs.side % 2 == 0 ? 1.0 : -1.0;
  return true;
}
// The N sums of a chunk from its threads' terms, into rec[0 .. N): inside a wave by shuffles
// over the distances 32, 16 .. 1, the four waves through LDS in wave order
template <int N>
__device__ __forceinline__ void flux_chunk_sum(const double* s, double* __restrict__ rec) {
  __shared__ double red[FLUX_CHUNK / 64][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < N; ++v) {
    double x = s[v];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if (lane == 0) red[wave][v] = x;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double x = red[0][threadIdx.x];
    for (int wv = 1; wv < FLUX_CHUNK / 64; ++wv) x += red[wv][threadIdx.x];
    rec[threadIdx.x] = x;
  }
}
// Area and inviscid sums of every chunk, with the ghost cells of the inviscid fill;
// partial: [chunk][FLUX_NQ], nondimensional, entries 0 .. FLUX_NE
template <int RECON, int LIM, int FLUX>
__global__ void __launch_bounds__(FLUX_CHUNK)
k_surface_flux(BlockDev b, GasDev g, double kappa, const FluxSurfDev* __restrict__ tab, int nsurf,
               double* __restrict__ partial) {
  constexpr int H = RECON == AGX_RECON_CONSTANT ? 1 : (RECON == AGX_RECON_MUSCL ? 2 : 3);
  double s[1 + FLUX_NE];
#pragma unroll
  for (int v = 0; v < 1 + FLUX_NE; ++v) s[v] = 0.0;
  FluxFace ff;
  if (flux_face(b, tab, nsurf, ff)) {
    const long sd = b.stride(ff.d);
    double area[4], f[AGX_NEQ];
    load_area(b, ff.d, ff.qU, area);
    // the 2 H cells about the face, the face between entries H - 1 and H
    double st[2 * H][AGX_NEQ], w[2 * H];
#pragma unroll
    for (int m = 0; m < 2 * H; ++m) {
      const long qq = ff.qU + (m - H) * sd;
      load5(b.state, qq, st[m]);
      w[m] = b.wid[ff.d][qq];
    }
    face_flux_1d<RECON, LIM, FLUX>(g, kappa, st, w, H, area, f);
    s[0] = area[3];
#pragma unroll
    for (int e = 0; e < AGX_NEQ; ++e) s[1 + e] = ff.sg * (f[e] * area[3]);
  }
  flux_chunk_sum<1 + FLUX_NE>(s, partial + (long)blockIdx.x * FLUX_NQ);
}
// The viscous sums of every chunk, with the ghost cells of the viscous-wall fill, entries
// 1 + FLUX_NE .. FLUX_NQ of the records.  fourth: bit 0 centralFourth, bit 1 a
// largeEddySimulation run (5 equations).  The residual adds the flux to the cell above the
// face, hence the sign.
__global__ void __launch_bounds__(FLUX_CHUNK)
k_surface_flux_visc(BlockDev b, GasDev g, const FluxSurfDev* __restrict__ tab, int nsurf,
                    int fourth, double* __restrict__ partial) {
  double s[FLUX_NE];
#pragma unroll
  for (int v = 0; v < FLUX_NE; ++v) s[v] = 0.0;
  FluxFace ff;
  if (flux_face(b, tab, nsurf, ff)) {
    double f[AGX_NEQ];     // (already times |A|)
#if AGX_NEQ == 7
    RansFace o;
    double sf[AGX_NEQ], muf, n[4];
    rans_face(b, g, ff.d, ff.fi, ff.fj, ff.fk, (fourth & 1) != 0, o, sf, muf, n);
    for (int e = 0; e < AGX_NEQ; ++e) f[e] = o.f[e];
#else
    if (fourth & 2) visc_face<false, true>(b, g, ff.d, ff.qU, f, (fourth & 1) != 0);
    else visc_face(b, g, ff.d, ff.qU, f, (fourth & 1) != 0);
#endif
#pragma unroll
    for (int e = 0; e < AGX_NEQ; ++e) s[e] = -(ff.sg * f[e]);
  }
  flux_chunk_sum<FLUX_NE>(s, partial + (long)blockIdx.x * FLUX_NQ + 1 + FLUX_NE);
}
// One thread per (variable of the call, surface): the surface's chunk records in ascending
// order, then the factor.  viscous = 0 (an inviscid context): the viscous ids give 0.
// out[v * nsurf + s]
__global__ void __launch_bounds__(64)
k_surface_flux_sum(OutSpec sp, const FluxSurfDev* __restrict__ tab, int nsurf, long nchunk,
                   int viscous, const double* __restrict__ partial, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= sp.nvar * nsurf) return;
  const int v = t / nsurf, sn = t % nsurf;
  const int q = sp.var[v] - AGX_FLUX_BASE;
  const long c0 = tab[sn].chunk0, c1 = sn + 1 < nsurf ? tab[sn + 1].chunk0 : nchunk;
  double x = 0.0;
  if (viscous || q <= FLUX_NE)
    for (long ch = c0; ch < c1; ++ch) x += partial[ch * FLUX_NQ + q];
  const double a2 = sp.l_ref * sp.l_ref;
  out[t] = x * (q == 0 ? a2 : cons_scale(sp, (q - 1) % FLUX_NE) * (sp.a_ref * a2));
}

// The block balance.  The rows (j, k) of the block are the march, k outer, cut into chunks of
// BUDGET_CHUNK rows (the chunking of k_cstat_partial with i collapsed): a wave per chunk, lane l
// takes the cells l, l + 64, ... of each row, the 64 lane sums are added by shuffles over the
// distances 32, 16 .. 1, and the chunk leaves one record of FLUX_NQ sums.  with_resid = 0: the
// residual planes are not read (no residual has been formed yet) and their sums come out 0.
constexpr int BUDGET_CHUNK = 64;
__global__ void __launch_bounds__(256)
k_block_budget(BlockDev b, GasDev g, long nchunk, int with_resid, double* __restrict__ partial) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const long chunk = t >> 6;                  // (uniform over a wave)
  if (chunk >= nchunk) return;
  const long rows = (long)b.nj * b.nk;
  const long r0 = chunk * BUDGET_CHUNK;
  const long r1 = r0 + BUDGET_CHUNK < rows ? r0 + BUDGET_CHUNK : rows;
  double s[FLUX_NQ];
#pragma unroll
  for (int v = 0; v < FLUX_NQ; ++v) s[v] = 0.0;
  for (long row = r0; row < r1; ++row) {
    const int j = (int)(row % b.nj), k = (int)(row / b.nj);
    for (int i = lane; i < b.ni; i += 64) {
      const long q = b.idx(i, j, k);
      const double vol = b.vol[q];
      double p[AGX_NEQ], u[AGX_NEQ];
      load5(b.state, q, p);
      prim_to_cons(g, p, u);
      s[0] += vol;
#pragma unroll
      for (int e = 0; e < AGX_NEQ; ++e) s[1 + e] += u[e] * vol;
      if (with_resid) {
#pragma unroll
        for (int e = 0; e < AGX_NEQ; ++e) s[1 + FLUX_NE + e] += b.resid[e][q];
      }
    }
  }
#pragma unroll
  for (int v = 0; v < FLUX_NQ; ++v) {
    double x = s[v];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if (lane == 0) partial[chunk * FLUX_NQ + v] = x;
  }
}
// One thread per variable of the call: the chunk records in ascending order, then the factor
__global__ void __launch_bounds__(64)
k_block_budget_sum(OutSpec sp, long nchunk, const double* __restrict__ partial,
                   double* __restrict__ out) {
  const int v = threadIdx.x;
  if (v >= sp.nvar) return;
  const int q = sp.var[v] - AGX_BUDGET_BASE;
  double x = 0.0;
  for (long ch = 0; ch < nchunk; ++ch) x += partial[ch * FLUX_NQ + q];
  const double lR = sp.l_ref, a2 = lR * lR;
  out[v] = x * (q == 0 ? a2 * lR
                : q <= FLUX_NE ? cons_scale(sp, q - 1) * (a2 * lR)
                               : cons_scale(sp, q - 1 - FLUX_NE) * (sp.a_ref * a2));
}

}  // namespace agx
