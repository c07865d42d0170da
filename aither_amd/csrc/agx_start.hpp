// agx_start.hpp -- the state a run starts or resumes from, formed on the device
// (agx_state_fill, agx_state_from_cloud, agx_restart_unpack; include/aither_gfx950.h).
//
// The three entry points leave a block exactly as the matching upload of a host array would:
// agx_state_upload of the ghost-padded state with zero in every ghost cell, or, for the second
// solution of a restart, agx_field_upload(AGX_FIELD_CONS_NM1).  An upload writes the positions
// of the padded box and nothing else of a plane (the alignment padding of a row keeps what it
// held); so do these kernels.
#pragma once
#include "agx_kernels.hpp"

namespace agx {

struct StartPrim { double v[AGX_NEQ]; };

// procBlock::InitializeStates, non-file branch (procBlock.cpp:325-354), and the ghost cells of
// the other two entries.  One thread per position of a padded row (sx of them, so a wave's
// stores of a plane are one contiguous run); positions outside the padded box are left alone.
//   physical = 1: physical cells take prim, ghost cells 0
//   physical = 0: ghost cells take 0, physical cells are left to the kernel that follows
__global__ void __launch_bounds__(256) k_state_fill(BlockDev b, StartPrim prim, int physical) {
  const int cj = b.nj + 2 * b.ng, ck = b.nk + 2 * b.ng;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)ck * cj * b.sx) return;
  const int x = (int)(t % b.sx);
  const long row = t / b.sx;
  const int i = x - b.ioff, j = (int)(row % cj) - b.ng, k = (int)(row / cj) - b.ng;
  if (i < -b.ng || i >= b.ni + b.ng) return;
  const bool phys = i >= 0 && i < b.ni && j >= 0 && j < b.nj && k >= 0 && k < b.nk;
  if (phys && !physical) return;
  const long q = b.idx(i, j, k);
#pragma unroll
  for (int e = 0; e < AGX_NEQ; ++e) b.state[e][q] = phys ? prim.v[e] : 0.0;
}

// ReadSolFromRestart (output.cpp:1177-1240; which = 0, into the state planes) and
// ReadSolNm1FromRestart (:1242-1305; which = 1, into consVarsNm1): the inverse of
// k_restart_pack.  The payload is cell-major, n_eq + 1 values per cell, so a lane per cell
// would gather with a stride of 48 (64) bytes: a workgroup takes its run of 256 cells --
// 256 (n_eq + 1) contiguous doubles -- through LDS instead, coalesced on the payload side, a
// row per cell with an odd stride on the LDS side (k_sweep_records' staging, the other way
// round), and each lane then stores its cell's values plane by plane.
// The reference divides (value /= divisor), and so does this kernel: div[e] holds the divisors
// as the reference's expressions form them, made on the host in that order
// (restart_divisors), and every quotient is a correctly rounded fp64 division (the build has
// no fast-math flag; no reciprocal is formed).  Density: (raw / rho_ref) * mf (:1197, :1228).
struct RestartDiv { double rho, v[AGX_NEQ]; };
constexpr int RST_NV = AGX_NEQ + 1;       // values of a cell in the payload
constexpr int RST_ROW = RST_NV | 1;       // LDS row stride: odd (7 or 9 doubles)
__global__ void __launch_bounds__(256)
k_restart_unpack(BlockDev b, RestartDiv dv, int which, const double* __restrict__ in) {
  __shared__ double row[256 * RST_ROW];
  const long ncell = (long)b.ni * b.nj * b.nk;
  const long p0 = (long)blockIdx.x * 256;
  const long nval = (min(p0 + 256, ncell) - p0) * RST_NV;     // this workgroup's doubles
  const double* src = in + p0 * RST_NV;
#pragma unroll
  for (int m = 0; m < RST_NV; ++m) {
    const int n = m * 256 + (int)threadIdx.x;
    if (n < nval) row[(n / RST_NV) * RST_ROW + n % RST_NV] = src[n];
  }
  __syncthreads();
  const long p = p0 + threadIdx.x;
  if (p >= ncell) return;
  const int i = (int)(p % b.ni), j = (int)((p / b.ni) % b.nj), k = (int)(p / ((long)b.ni * b.nj));
  const long q = b.idx(i, j, k);
  const double* r = row + threadIdx.x * RST_ROW;
  double* const* dst = which == 0 ? b.state : b.consnm1;
  dst[0][q] = (r[0] / dv.rho) * r[AGX_NEQ];
#pragma unroll
  for (int e = 1; e < AGX_NEQ; ++e) dst[e][q] = r[e] / dv.v[e];
}

// procBlock::InitializeStates, file branch (procBlock.cpp:287-323): every physical cell takes
// the state of the cloud point nearest to its centre.  kdtree::NearestNeighbor
// (kdtree.cpp:123-225) as the exhaustive search of k_nearest_wall_planes -- 256 points per LDS
// tile, the cells in registers -- that carries the index of the minimum beside it.
// TIE RULE: among points at equal squared distance the LOWEST point index wins (the points are
// visited in ascending order and only a strictly smaller distance replaces the minimum).  The
// reference's k-d tree leaves ties to the order its build left the points in.
// The squared distance is dx dx + dy dy + dz dz of the differences centre - point; the compiler
// may contract it, so winners closer than a few units of 2^-53 relative are not decided the way
// an uncontracted sum would.
// A thread holds CPT cells, 256 apart, so that the three LDS broadcast reads of a point serve
// CPT distance evaluations.  The cell's state planes are written here (states[id], a gather of
// n_eq doubles from the staged cloud), and the workgroup's largest distance goes to
// part[blockIdx.x]: the caller folds the partial maxima (no floating-point atomics).
// The work is cells x points: see agx_state_from_cloud for the sizes it is meant for.
// AGX_CLOUD_CPT: the CPT the library is built with (DESIGN section 8 has the timing of 1, 2, 4).
#ifndef AGX_CLOUD_CPT
#define AGX_CLOUD_CPT 2
#endif
template <int CPT>
__global__ void __launch_bounds__(256)
k_cloud_nearest(BlockDev b, long npts, const double* __restrict__ pts,
                const double* __restrict__ states, double* __restrict__ part) {
  __shared__ double sp[256][3];
  __shared__ double smax[256];
  const long ncell = (long)b.ni * b.nj * b.nk;
  long q[CPT];
  double c[CPT][3], best[CPT];
  long id[CPT];
#pragma unroll
  for (int n = 0; n < CPT; ++n) {
    const long t = ((long)blockIdx.x * CPT + n) * 256 + threadIdx.x;
    const long tc = min(t, ncell - 1);
    const int i = (int)(tc % b.ni), j = (int)((tc / b.ni) % b.nj),
              k = (int)(tc / ((long)b.ni * b.nj));
    q[n] = b.idx(i, j, k);
    c[n][0] = b.cen[0][q[n]]; c[n][1] = b.cen[1][q[n]]; c[n][2] = b.cen[2][q[n]];
    best[n] = 1.7976931348623157e308;
    id[n] = 0;
  }
  for (long p0 = 0; p0 < npts; p0 += 256) {
    const long p = min(p0 + threadIdx.x, npts - 1);
    const int mlim = (int)min(256L, npts - p0);
    __syncthreads();
    sp[threadIdx.x][0] = pts[3 * p]; sp[threadIdx.x][1] = pts[3 * p + 1];
    sp[threadIdx.x][2] = pts[3 * p + 2];
    __syncthreads();
#pragma unroll 4
    for (int m = 0; m < mlim; ++m) {
      const double x = sp[m][0], y = sp[m][1], z = sp[m][2];
#pragma unroll
      for (int n = 0; n < CPT; ++n) {
        const double d[3] = {c[n][0] - x, c[n][1] - y, c[n][2] - z};
        const double d2 = dot3(d, d);
        if (d2 < best[n]) { best[n] = d2; id[n] = p0 + m; }
      }
    }
  }
  double far = 0.0;
#pragma unroll
  for (int n = 0; n < CPT; ++n) {
    const long t = ((long)blockIdx.x * CPT + n) * 256 + threadIdx.x;
    if (t >= ncell) continue;
    far = fmax(far, sqrt(best[n]));
    const double* s = states + AGX_NEQ * id[n];
#pragma unroll
    for (int e = 0; e < AGX_NEQ; ++e) b.state[e][q[n]] = s[e];
  }
  smax[threadIdx.x] = far;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = smax[0];
}

}  // namespace agx
