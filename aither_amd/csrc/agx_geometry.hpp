// agx_geometry.hpp -- a block's whole geometry formed on the device from its node
// coordinates (agx_block_geom.nodes): the kernels behind agx_block_create /
// agx_setup_finalize for node-built blocks.  They restate, on the block's SoA planes and in
// the reference's order,
//   * PadWithGhosts + procBlock::AssignGhostCellsGeom      procBlock.cpp:2160-2268
//   * SwapGeomSlice / procBlock::PutGeomSlice              utility.cpp:212-255, procBlock.cpp:3165-3600
//   * procBlock::AssignGhostCellsGeomEdge                  procBlock.cpp:2270-2425
//   * procBlock::CalcCellWidths                            procBlock.cpp:6397-6412
//   * the ghost rule of procBlock::CalcWallDistance        procBlock.cpp:6044-6107
// After the metrics every step is a copy, a sign flip or one add / subtract, so the result
// equals the host pipeline's (aither_amd/case/geometry.py) bit for bit; widths and wall
// distance hold a sqrt of a dot product.  Everything but the metrics, the widths and the
// wall search is surface-sized: one launch per surface and layer, lanes along i where the
// surface has an i extent.
#pragma once
#include "agx_kernels.hpp"

namespace agx {

// the planes the geometry pass works on: the block's own and the face centres, which live
// for the pass only (fCenterI/J/K_, procBlock.hpp:77-79)
struct GeoPlanes {
  double* vol;
  double* cen[3];
  double* fa[3][4];
  double* fc[3][3];
  double* wdist;
};

// ---- metrics of the physical cells and faces straight into the planes: the arithmetic of
// k_plot3d_metrics (m_pyramid, m_face), one thread per node.  what: 1 = volume, centre and
// face areas (agx_block_create), 2 = face centres (the pass of agx_setup_finalize).
// err: 4 negative volume, 5 + d negative d-face area.
__global__ void __launch_bounds__(256)
k_metrics_planes(BlockDev b, const double* __restrict__ x, GeoPlanes g, int what, int* err) {
  const int ni = b.ni, nj = b.nj, nk = b.nk;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nn = (long)(ni + 1) * (nj + 1) * (nk + 1);
  if (t >= nn) return;
  const int i = (int)(t % (ni + 1)), j = (int)((t / (ni + 1)) % (nj + 1)),
            k = (int)(t / ((long)(ni + 1) * (nj + 1)));
  auto nd = [&](int a, int bb, int c, double* v) {
    const double* p = x + 3 * (((long)c * (nj + 1) + bb) * (ni + 1) + a);
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
  };
  const long q = b.idx(i, j, k);
  if (what == 1 && i < ni && j < nj && k < nk) {
    double c000[3], c100[3], c010[3], c110[3], c001[3], c101[3], c011[3], c111[3], cen[3];
    nd(i, j, k, c000); nd(i + 1, j, k, c100); nd(i, j + 1, k, c010); nd(i + 1, j + 1, k, c110);
    nd(i, j, k + 1, c001); nd(i + 1, j, k + 1, c101); nd(i, j + 1, k + 1, c011);
    nd(i + 1, j + 1, k + 1, c111);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      cen[c] = 0.125 * (((((((c000[c] + c100[c]) + c010[c]) + c110[c]) + c001[c]) + c101[c]) +
                         c011[c]) + c111[c]);
    g.cen[0][q] = cen[0]; g.cen[1][q] = cen[1]; g.cen[2][q] = cen[2];
    double v = m_pyramid(cen, c000, c001, c011, c010);
    v = v + m_pyramid(cen, c100, c110, c111, c101);
    v = v + m_pyramid(cen, c000, c100, c101, c001);
    v = v + m_pyramid(cen, c010, c011, c111, c110);
    v = v + m_pyramid(cen, c000, c010, c110, c100);
    v = v + m_pyramid(cen, c001, c101, c111, c011);
    if (!(v > 0.0)) *err = 4;
    g.vol[q] = v;
  }
  double n00[3], n10[3], n01[3], n11[3], xac[3], xbd[3], fa[4], fc[3];
  auto put = [&](int d) {
    if (what == 1) {
      if (!(fa[3] > 0.0)) *err = 5 + d;
#pragma unroll
      for (int c = 0; c < 4; ++c) g.fa[d][c][q] = fa[c];
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) g.fc[d][c][q] = fc[c];
    }
  };
  if (j < nj && k < nk) {          // i-face, plot3d.cpp:150-181
    nd(i, j, k, n00); nd(i, j + 1, k, n10); nd(i, j, k + 1, n01); nd(i, j + 1, k + 1, n11);
    m_sub(n11, n00, xac); m_sub(n10, n01, xbd);
    m_face(n00, n10, n01, n11, xac, xbd, what == 1 ? fa : nullptr, what == 1 ? nullptr : fc);
    put(0);
  }
  if (i < ni && k < nk) {          // j-face, plot3d.cpp:224-255
    nd(i, j, k, n00); nd(i + 1, j, k, n10); nd(i, j, k + 1, n01); nd(i + 1, j, k + 1, n11);
    m_sub(n01, n10, xac); m_sub(n00, n11, xbd);
    m_face(n00, n10, n01, n11, xac, xbd, what == 1 ? fa : nullptr, what == 1 ? nullptr : fc);
    put(1);
  }
  if (i < ni && j < nj) {          // k-face, plot3d.cpp:300-331
    nd(i, j, k, n00); nd(i + 1, j, k, n10); nd(i, j + 1, k, n01); nd(i + 1, j + 1, k, n11);
    m_sub(n01, n10, xac); m_sub(n11, n00, xbd);
    m_face(n00, n10, n01, n11, xac, xbd, what == 1 ? fa : nullptr, what == 1 ? nullptr : fc);
    put(2);
  }
}

// wallDist_ starts at DEFAULT_WALL_DIST (macros.hpp.in) everywhere
__global__ void __launch_bounds__(256) k_geo_fill(double* p, long n, double v) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) p[t] = v;
}

// ---- procBlock::AssignGhostCellsGeom, one surface and one layer.  Index ranges as
// multiArray3d::Slice(dir, ind, r1, r2, id, type) gives them (multiArray3d.hpp:529-573):
// the plane of cells `ind` normal to d3, d-faces one longer along d, and the d3-faces of an
// upper surface one further out.  A thread is one position (ta, tb) of the surface,
// extended by one in both in-plane directions for the faces that close the lines.
struct GhostGeomOp {
  int d3, upper, layer;
  int lo[3], hi[3];         // cell range of the surface (lo[d3] = its constant index)
  int n3;                   // physical cells along d3
};
__global__ void __launch_bounds__(256) k_ghost_geom(BlockDev b, GeoPlanes g, GhostGeomOp o) {
  const int d3 = o.d3;
  // lanes along i where the surface has an i extent
  const int da = d3 == 0 ? 1 : 0, db = d3 == 2 ? 1 : 2;      // in-plane directions, da faster
  const int la = o.hi[da] - o.lo[da], lb = o.hi[db] - o.lo[db];
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)(la + 1) * (lb + 1)) return;
  const int ta = (int)(t % (la + 1)), tb = (int)(t / (la + 1));
  const int r3 = o.lo[d3], layer = o.layer;
  int g_cell, i_cell, p_cell, pi_cell, i_face, pi_face;
  if (o.upper) {
    g_cell = r3 + layer - 1; i_cell = max(r3 - layer, 0);
    p_cell = g_cell - 1; pi_cell = i_cell + 1;
    i_face = max(r3 - layer, 0); pi_face = i_face + 1;
  } else {
    g_cell = r3 - layer; i_cell = min(r3 + layer - 1, o.n3 - 1);
    p_cell = g_cell + 1; pi_cell = i_cell - 1;
    i_face = min(r3 + layer, o.n3); pi_face = i_face - 1;
  }
  // position (sa, sb) of the surface in plane `ind` of cells / lower faces
  auto at = [&](int ind, int sa, int sb) {
    int c[3];
    c[d3] = ind; c[da] = o.lo[da] + sa; c[db] = o.lo[db] + sb;
    return b.idx(c[0], c[1], c[2]);
  };
  const bool in_a = ta < la, in_b = tb < lb;
  const int ca = min(ta, la - 1), cb = min(tb, lb - 1);     // GrowI/J/K: the last entry again
  // face to face across the boundary cell; cell to cell from the second layer on
  auto dist_c2c = [&](int sa, int sb, double* out) {
    if (layer > 1) {
      const long ch = at(pi_cell, sa, sb), cl = at(i_cell, sa, sb);
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c] = g.cen[c][ch] - g.cen[c][cl];
    } else {
      const long qh = at(pi_face, sa, sb), ql = at(i_face, sa, sb);
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c] = g.fc[d3][c][qh] - g.fc[d3][c][ql];
    }
  };
  if (in_a && in_b) {
    const long qg = at(g_cell, ta, tb), qi = at(i_cell, ta, tb), qp = at(p_cell, ta, tb);
    double f2f[3], c2c[3];
    {
      const long qh = at(pi_face, ta, tb), ql = at(i_face, ta, tb);
#pragma unroll
      for (int c = 0; c < 3; ++c) f2f[c] = g.fc[d3][c][qh] - g.fc[d3][c][ql];
    }
    dist_c2c(ta, tb, c2c);
    g.vol[qg] = g.vol[qi];
    // d3-faces: those of an upper surface sit one further out
    const int s = o.upper ? 1 : 0;
    const long fg = at(g_cell + s, ta, tb), fi = at(i_cell + s, ta, tb), fp = at(p_cell + s, ta, tb);
#pragma unroll
    for (int c = 0; c < 4; ++c) g.fa[d3][c][fg] = g.fa[d3][c][fi];
#pragma unroll
    for (int c = 0; c < 3; ++c) g.fc[d3][c][fg] = f2f[c] + g.fc[d3][c][fp];
#pragma unroll
    for (int c = 0; c < 3; ++c) g.cen[c][qg] = g.cen[c][qp] + c2c[c];
  }
  // in-plane faces: one more along their own direction
  if (in_b) {
    const long qg = at(g_cell, ta, tb), qi = at(i_cell, ta, tb), qp = at(p_cell, ta, tb);
#pragma unroll
    for (int c = 0; c < 4; ++c) g.fa[da][c][qg] = g.fa[da][c][qi];
    double cc[3];
    dist_c2c(ca, tb, cc);
#pragma unroll
    for (int c = 0; c < 3; ++c) g.fc[da][c][qg] = cc[c] + g.fc[da][c][qp];
  }
  if (in_a) {
    const long qg = at(g_cell, ta, tb), qi = at(i_cell, ta, tb), qp = at(p_cell, ta, tb);
#pragma unroll
    for (int c = 0; c < 4; ++c) g.fa[db][c][qg] = g.fa[db][c][qi];
    double cc[3];
    dist_c2c(ta, cb, cc);
#pragma unroll
    for (int c = 0; c < 3; ++c) g.fc[db][c][qg] = cc[c] + g.fc[db][c][qp];
  }
}

// ---- SwapGeomSlice: copy records built on the host (agx_api.hip, geo_swap).  A record
// moves one cell's volume (kind 0), its centre (1), or the area and centre of one face
// (2: dr-face of the receiver <- ds-face of the sender, the unit normal flipped where the
// reference multiplies unitVec3dMag by -1).  All records of both sides are gathered into a
// buffer before any is scattered (both slices are taken before either insert).
struct GeoCopy { long dst, src; int kind, dr, ds, flip; };
__global__ void __launch_bounds__(256)
k_geo_gather(GeoPlanes s, const GeoCopy* __restrict__ rec, long n, double* __restrict__ buf) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const GeoCopy r = rec[t];
  double* o = buf + 7 * t;
  if (r.kind == 0) {
    o[0] = s.vol[r.src];
  } else if (r.kind == 1) {
    for (int c = 0; c < 3; ++c) o[c] = s.cen[c][r.src];
  } else {
    for (int c = 0; c < 4; ++c) {
      const double v = s.fa[r.ds][c][r.src];
      o[c] = (r.flip && c < 3) ? -v : v;
    }
    for (int c = 0; c < 3; ++c) o[4 + c] = s.fc[r.ds][c][r.src];
  }
}
__global__ void __launch_bounds__(256)
k_geo_scatter(GeoPlanes d, const GeoCopy* __restrict__ rec, long n, const double* __restrict__ buf) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const GeoCopy r = rec[t];
  const double* o = buf + 7 * t;
  if (r.kind == 0) {
    d.vol[r.dst] = o[0];
  } else if (r.kind == 1) {
    for (int c = 0; c < 3; ++c) d.cen[c][r.dst] = o[c];
  } else {
    for (int c = 0; c < 4; ++c) d.fa[r.dr][c][r.dst] = o[c];
    for (int c = 0; c < 3; ++c) d.fc[r.dr][c][r.dst] = o[4 + c];
  }
}
// one plane through an index list (sender volumes for the T-intersection test, SwapWallDist)
__global__ void __launch_bounds__(256)
k_geo_gather1(const double* __restrict__ p, const long* __restrict__ idx, long n,
              double* __restrict__ buf) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) buf[t] = p[idx[t]];
}
__global__ void __launch_bounds__(256)
k_geo_scatter1(double* __restrict__ p, const long* __restrict__ idx, long n,
               const double* __restrict__ buf) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) p[idx[t]] = buf[t];
}

// ---- procBlock::AssignGhostCellsGeomEdge, one edge line (direction d, corner cc, layers
// layer2 / layer3): index ranges as multiArray3d::Slice(dir, d2Ind, d3Ind, physOnly = true,
// id, upper2, upper3) gives them (multiArray3d.hpp:473-523).  A thread is one position
// along the line, one more than the cells for the d-faces.
struct EdgeGeomOp {
  int d, two, three;        // line direction and the two it is an edge of
  int nd;                   // physical cells along d
  int g2, p2, i2, g3, p3;   // ghost / previous / interior index in `two`, ghost / previous in `three`
  int u2, u3;
};
__global__ void __launch_bounds__(256) k_edge_geom(BlockDev b, GeoPlanes g, EdgeGeomOp o) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t > o.nd) return;
  // line (a2, a3) of array `fid` (-1: a cell array) at position s along d
  auto at = [&](int a2, int a3, int fid, int s) {
    if (o.u2 && fid == o.two) a2 += 1;
    else if (o.u3 && fid == o.three) a3 += 1;
    int c[3];
    c[o.d] = s; c[o.two] = a2; c[o.three] = a3;
    return b.idx(c[0], c[1], c[2]);
  };
  const bool cell = t < o.nd;
  const int tc = min(t, o.nd - 1);                 // GrowI/J/K
  double c2c[3], f2f[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 3; ++c)
    c2c[c] = g.cen[c][at(o.g2, o.p3, -1, tc)] - g.cen[c][at(o.p2, o.p3, -1, tc)];
  if (cell) {
    g.vol[at(o.g2, o.g3, -1, t)] = g.vol[at(o.i2, o.g3, -1, t)];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      f2f[c] = g.fc[o.two][c][at(o.g2, o.p3, o.two, t)] - g.fc[o.two][c][at(o.p2, o.p3, o.two, t)];
  }
  for (int f = 0; f < 3; ++f) {
    if (!cell && f != o.d) continue;
    const long qg = at(o.g2, o.g3, f, t), qi = at(o.i2, o.g3, f, t);
    for (int c = 0; c < 4; ++c) g.fa[f][c][qg] = g.fa[f][c][qi];
  }
  if (cell) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      g.cen[c][at(o.g2, o.g3, -1, t)] = c2c[c] + g.cen[c][at(o.p2, o.g3, -1, t)];
  }
  for (int f = 0; f < 3; ++f) {
    if (!cell && f != o.d) continue;
    const long qg = at(o.g2, o.g3, f, t), qp = at(o.p2, o.g3, f, t);
    for (int c = 0; c < 3; ++c) {
      const double dist = f == o.two ? f2f[c] : c2c[c];
      g.fc[f][c][qg] = dist + g.fc[f][c][qp];
    }
  }
}

// ---- procBlock::CalcCellWidths over the whole ghost-padded array: the distance between
// the lower and the upper d-face centre of every cell
__global__ void __launch_bounds__(256) k_cell_widths(BlockDev b, GeoPlanes g, double* w0,
                                                     double* w1, double* w2) {
  const int ci = b.ni + 2 * b.ng, cj = b.nj + 2 * b.ng, ck = b.nk + 2 * b.ng;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)ci * cj * ck) return;
  const int i = (int)(t % ci) - b.ng, j = (int)((t / ci) % cj) - b.ng,
            k = (int)(t / ((long)ci * cj)) - b.ng;
  const long q = b.idx(i, j, k);
  double* w[3] = {w0, w1, w2};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const long qu = q + b.stride(d);
    const double df[3] = {g.fc[d][0][q] - g.fc[d][0][qu], g.fc[d][1][q] - g.fc[d][1][qu],
                          g.fc[d][2][q] - g.fc[d][2][qu]};
    w[d][q] = sqrt(dot3(df, df));
  }
}

// ---- wall distance.  Face centres of one viscousWall surface, packed (x, y, z) per face;
// the nearest-wall search of the physical cells of a block (k_nearest_wall's search, the
// cells read from and the distance written to the planes); the ghost rule of
// procBlock::CalcWallDistance for one surface, all layers.
__global__ void __launch_bounds__(256)
k_wall_points(BlockDev b, GeoPlanes g, int d3, int lo0, int lo1, int lo2, int hi0, int hi1,
              int hi2, double* __restrict__ out) {
  const int lo[3] = {lo0, lo1, lo2}, n[3] = {hi0 - lo0, hi1 - lo1, hi2 - lo2};
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n[0] * n[1] * n[2]) return;
  const int i = lo[0] + (int)(t % n[0]), j = lo[1] + (int)((t / n[0]) % n[1]),
            k = lo[2] + (int)(t / ((long)n[0] * n[1]));
  const long q = b.idx(i, j, k);
  for (int c = 0; c < 3; ++c) out[3 * t + c] = g.fc[d3][c][q];
}
__global__ void __launch_bounds__(256)
k_nearest_wall_planes(BlockDev b, GeoPlanes g, long nwall, const double* __restrict__ wall) {
  __shared__ double sw[256][3];
  const long ncell = (long)b.ni * b.nj * b.nk;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long tc = min(t, ncell - 1);
  const int i = (int)(tc % b.ni), j = (int)((tc / b.ni) % b.nj), k = (int)(tc / ((long)b.ni * b.nj));
  const long q = b.idx(i, j, k);
  const double c[3] = {g.cen[0][q], g.cen[1][q], g.cen[2][q]};
  double best = 1.7976931348623157e308;
  for (long p0 = 0; p0 < nwall; p0 += 256) {
    const long p = min(p0 + threadIdx.x, nwall - 1);
    __syncthreads();
    sw[threadIdx.x][0] = wall[3 * p]; sw[threadIdx.x][1] = wall[3 * p + 1];
    sw[threadIdx.x][2] = wall[3 * p + 2];
    __syncthreads();
#pragma unroll 8
    for (int m = 0; m < 256; ++m) {
      const double d[3] = {c[0] - sw[m][0], c[1] - sw[m][1], c[2] - sw[m][2]};
      best = fmin(best, dot3(d, d));
    }
  }
  if (t < ncell) g.wdist[q] = sqrt(best);
}
__global__ void __launch_bounds__(256)
k_wall_dist_ghosts(BlockDev b, double* wd, int d3, int upper, int is_wall, int lo0, int lo1,
                   int lo2, int hi0, int hi1, int hi2) {
  const int lo[3] = {lo0, lo1, lo2}, n[3] = {hi0 - lo0, hi1 - lo1, hi2 - lo2};
  const int nd = d3 == 0 ? b.ni : (d3 == 1 ? b.nj : b.nk);
  const long cells = (long)n[0] * n[1] * n[2];
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cells * b.ng) return;
  const int layer = 1 + (int)(t / cells);
  const long s = t % cells;
  int cg[3] = {lo[0] + (int)(s % n[0]), lo[1] + (int)((s / n[0]) % n[1]),
               lo[2] + (int)(s / ((long)n[0] * n[1]))};
  int cs[3] = {cg[0], cg[1], cg[2]};
  if (upper) { cg[d3] = nd + layer - 1; cs[d3] = is_wall ? nd - layer : nd - 1; }
  else       { cg[d3] = -layer;         cs[d3] = is_wall ? layer - 1 : 0; }
  const double v = wd[b.idx(cs[0], cs[1], cs[2])];
  wd[b.idx(cg[0], cg[1], cg[2])] = is_wall ? -1.0 * v : 1.0 * v;
}

}  // namespace agx
