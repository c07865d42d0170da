// agx_mresid_plan.hpp -- which workgroup of k_matrix_resid_d2m owns which plane positions,
// and where each of its threads finds its four in-plane neighbours.
//
// A plane of Pi x Pj padded cells is stored diagonal by diagonal (agx_lusgs.hpp):
// position(ie, je) = dstart(de) - jlo(de) + je with de = ie + je.  In (de, je) space the plane
// is a parallelogram, jlo(de) <= je <= jhi(de).  The kernel cuts it into PATCHES: rectangles
// of MRP_W consecutive diagonals (rows) by MRP_L consecutive je (columns), a thread per cell,
//
//     thread t = row * MRP_L + col of patch (d0, j0)  <->  cell (de, je) = (d0 + row, j0 + col).
//
// Because the runs of a patch are aligned on je, the in-plane neighbours of a cell are
//     (ie - 1, je)  the same column of the row below     (ie, je - 1)  column - 1 of the row below
//     (ie + 1, je)  the same column of the row above     (ie, je + 1)  column + 1 of the row above
// in both triangles of the plane, and a row's own positions are consecutive (coalesced).
// Each thread publishes its cell in LDS slot (row, column); the rows -1 and MRP_W and the
// columns -1 and MRP_L of the slot array are the RIM, filled from the arrays by "extra"
// loads that the first threads of the patch perform (mrp_extra).  Every neighbour is then
// read from a slot; mrp_neighbour names it.
//
// 8 x 32 (half a wave per diagonal) against 4 x 64 (a wave per diagonal): a padded plane of
// 262 x 262 takes 306 patches instead of 335 (88 % of the threads own a position instead of
// 80 %), the rim is 80 loads per patch instead of 136 and the slot array 340 instead of 396
// slots; measured equal at 256^3, taken for the LDS.
//
// A band is the MRP_W diagonals [MRP_W b, MRP_W b + MRP_W); its patches start at the band's
// smallest je and follow each other along je.  Patches are numbered band by band; the XCDs
// get contiguous ranges of that sequence (workgroup n runs on XCD n % 8), so the patches
// that share a rim share an L2.  Each patch is marched along k in chunks of kc planes.
//
// Plain C++ for host and device: the kernel decodes with it, the host sizes the launch with
// it and tests/cpp/mresid_plan.cpp checks it without a GPU.
#pragma once

#if defined(__HIPCC__)
#define AGX_MP_HD __host__ __device__
#else
#define AGX_MP_HD
#endif

namespace agx {

#ifndef AGX_MRP_W
#define AGX_MRP_W 8
#endif
#ifndef AGX_MRP_L
#define AGX_MRP_L 32
#endif
constexpr int MRP_W = AGX_MRP_W;      // diagonals of a patch
constexpr int MRP_L = AGX_MRP_L;      // je of a patch: a row of MRP_L consecutive threads
constexpr int MRP_THREADS = MRP_W * MRP_L;
constexpr int MRP_ROWS = MRP_W + 2;   // slot rows -1 .. MRP_W
constexpr int MRP_COLS = MRP_L + 2;   // slot columns -1 .. MRP_L
constexpr int MRP_SLOTS = MRP_ROWS * MRP_COLS;
// face statics are read of the upper neighbours only: rows 1 .. MRP_W
constexpr int MRP_FACE_SLOTS = MRP_W * MRP_COLS;
// the rim: rows -1 and MRP_W (MRP_L + 1 slots each), column -1 of the rows 0 .. MRP_W - 2,
// column MRP_L of the rows 1 .. MRP_W - 1
constexpr int MRP_EXTRAS = 2 * (MRP_L + 1) + 2 * (MRP_W - 1);
static_assert(MRP_EXTRAS <= MRP_THREADS, "one extra load per thread");

struct MrpPlane { int Pi, Pj, ng; };
struct MrpPatch { int d0, j0; };

AGX_MP_HD inline int mrp_min(int a, int b) { return a < b ? a : b; }
AGX_MP_HD inline int mrp_max(int a, int b) { return a > b ? a : b; }
AGX_MP_HD inline int mrp_ndiag(const MrpPlane& p) { return p.Pi + p.Pj - 1; }
AGX_MP_HD inline int mrp_jlo(const MrpPlane& p, int de) { return mrp_max(0, de - (p.Pi - 1)); }
AGX_MP_HD inline int mrp_jhi(const MrpPlane& p, int de) { return mrp_min(de, p.Pj - 1); }
// start of diagonal de (the dstart table of the D2 layout in closed form)
AGX_MP_HD inline int mrp_dstart(const MrpPlane& p, int de) {
  const int a = mrp_min(p.Pi, p.Pj), bm = mrp_max(p.Pi, p.Pj);
  if (de <= a) return de * (de + 1) / 2;
  if (de <= bm) return a * (a + 1) / 2 + (de - a) * a;
  const int r = p.Pi + p.Pj - 1 - de;
  return p.Pi * p.Pj - r * (r + 1) / 2;
}
AGX_MP_HD inline bool mrp_in_plane(const MrpPlane& p, int de, int je) {
  return de >= 0 && de < mrp_ndiag(p) && je >= mrp_jlo(p, de) && je <= mrp_jhi(p, de);
}
// plane position of (de, je); mrp_in_plane(p, de, je) must hold
AGX_MP_HD inline int mrp_pos(const MrpPlane& p, int de, int je) {
  return mrp_dstart(p, de) - mrp_jlo(p, de) + je;
}

// What a plane position is to the pass: MRP_NONE (outside the plane, a corner or a ghost
// cell of the second layer and beyond: never a neighbour of a physical cell), MRP_CELL (a
// physical cell) or the side 1 .. 4 (i-lower, i-upper, j-lower, j-upper, the surface numbers
// of bc_is_connection) whose first ghost layer it belongs to.  A ghost position is a
// neighbour only across a connection surface: the kernel publishes it like a cell where its
// side has one and leaves it out otherwise.
enum { MRP_NONE = -1, MRP_CELL = 0 };
AGX_MP_HD inline int mrp_kind(const MrpPlane& p, int de, int je) {
  if (!mrp_in_plane(p, de, je)) return MRP_NONE;
  const int ie = de - je;
  const bool in_i = ie >= p.ng && ie < p.Pi - p.ng, in_j = je >= p.ng && je < p.Pj - p.ng;
  if (in_i && in_j) return MRP_CELL;
  if (in_j) return ie == p.ng - 1 ? 1 : (ie == p.Pi - p.ng ? 2 : MRP_NONE);
  if (in_i) return je == p.ng - 1 ? 3 : (je == p.Pj - p.ng ? 4 : MRP_NONE);
  return MRP_NONE;
}

// ---- patches ----
AGX_MP_HD inline int mrp_bands(const MrpPlane& p) { return (mrp_ndiag(p) + MRP_W - 1) / MRP_W; }
AGX_MP_HD inline int mrp_band_j0(const MrpPlane& p, int band) { return mrp_jlo(p, MRP_W * band); }
AGX_MP_HD inline int mrp_band_runs(const MrpPlane& p, int band) {
  const int dl = mrp_min(MRP_W * band + MRP_W - 1, mrp_ndiag(p) - 1);
  const int len = mrp_jhi(p, dl) - mrp_band_j0(p, band) + 1;    // >= 1: jlo and jhi only grow
  return (len + MRP_L - 1) / MRP_L;
}
inline int mrp_patches(const MrpPlane& p) {
  int n = 0;
  for (int b = 0; b < mrp_bands(p); ++b) n += mrp_band_runs(p, b);
  return n;
}
// patch n of the band-by-band sequence; false past its end
AGX_MP_HD inline bool mrp_patch(const MrpPlane& p, int n, MrpPatch& pt) {
  const int nb = mrp_bands(p);
  for (int b = 0; b < nb; ++b) {
    const int r = mrp_band_runs(p, b);
    if (n < r) {
      pt.d0 = MRP_W * b;
      pt.j0 = mrp_band_j0(p, b) + MRP_L * n;
      return true;
    }
    n -= r;
  }
  pt.d0 = pt.j0 = 0;
  return false;
}

// ---- XCD dealing and k-chunks ----
// workgroup n runs on XCD n % 8; XCD x marches the patches [x per, x per + per) chunk by chunk
struct MrpWg { int patch, kch; };
AGX_MP_HD inline int mrp_per_xcd(int npatch) { return (npatch + 7) / 8; }
AGX_MP_HD inline int mrp_kchunks(int nk, int kc) { return (nk + kc - 1) / kc; }
AGX_MP_HD inline long mrp_wgs(int npatch, int nk, int kc) {
  return 8L * mrp_per_xcd(npatch) * mrp_kchunks(nk, kc);
}
// (patch >= npatch: a workgroup without work, it posts a zero partial)
AGX_MP_HD inline MrpWg mrp_deal(int wg, int per) {
  const int xcd = wg % 8, m = wg / 8;
  return MrpWg{xcd * per + m % per, m / per};
}
AGX_MP_HD inline void mrp_kchunk(int nk, int kc, int kch, int& k0, int& k1) {
  k0 = kch * kc;
  k1 = mrp_min(k0 + kc, nk);
}

// ---- threads, slots, neighbours ----
AGX_MP_HD inline int mrp_slot(int row, int col) { return (row + 1) * MRP_COLS + col + 1; }
// the face statics of row 1 .. MRP_W
AGX_MP_HD inline int mrp_face_slot(int row, int col) { return (row - 1) * MRP_COLS + col + 1; }

// what thread t of a patch loads and publishes: `kind` says whether there is anything
// (mrp_kind), de / je which cell, slot where its column goes, fslot where its lower i- and
// j-face statics go (-1: nobody reads them)
struct MrpLoad { int kind, de, je, slot, fslot; };
AGX_MP_HD inline MrpLoad mrp_load_at(const MrpPlane& p, const MrpPatch& pt, int row, int col,
                                     bool faces) {
  MrpLoad o;
  o.de = pt.d0 + row; o.je = pt.j0 + col;
  o.kind = mrp_kind(p, o.de, o.je);
  o.slot = mrp_slot(row, col);
  o.fslot = faces ? mrp_face_slot(row, col) : -1;
  return o;
}
// its own cell
AGX_MP_HD inline MrpLoad mrp_own(const MrpPlane& p, const MrpPatch& pt, int t) {
  const int w = t / MRP_L, l = t % MRP_L;
  return mrp_load_at(p, pt, w, l, w >= 1);
}
// its share of the rim (kind MRP_NONE for t >= MRP_EXTRAS): consecutive threads take
// consecutive positions of the rows -1 and MRP_W
AGX_MP_HD inline MrpLoad mrp_extra(const MrpPlane& p, const MrpPatch& pt, int t) {
  if (t < MRP_L + 1) return mrp_load_at(p, pt, -1, t - 1, false);
  t -= MRP_L + 1;
  if (t < MRP_L + 1) return mrp_load_at(p, pt, MRP_W, t, true);
  t -= MRP_L + 1;
  if (t < MRP_W - 1) return mrp_load_at(p, pt, t, -1, false);
  t -= MRP_W - 1;
  if (t < MRP_W - 1) return mrp_load_at(p, pt, t + 1, MRP_L, true);
  MrpLoad o;
  o.kind = MRP_NONE; o.de = o.je = 0; o.slot = 0; o.fslot = -1;
  return o;
}
// neighbour q of the cell of (row w, column l): 0 (ie - 1, je), 1 (ie, je - 1), 2 (ie + 1, je),
// 3 (ie, je + 1).  Its column is in `slot`; for the upper two the statics of the face
// between them (its lower i- / j-face) are in `fslot`.
struct MrpNb { int de, je, slot, fslot; };
AGX_MP_HD inline MrpNb mrp_neighbour(const MrpPatch& pt, int w, int l, int q) {
  const int row = q < 2 ? w - 1 : w + 1;
  const int col = q == 1 ? l - 1 : (q == 3 ? l + 1 : l);
  return MrpNb{pt.d0 + row, pt.j0 + col, mrp_slot(row, col),
               q < 2 ? -1 : mrp_face_slot(row, col)};
}

}  // namespace agx
