// The patch plan of the matrix residual (aither_amd/csrc/agx_mresid_plan.hpp) under the
// address and undefined-behaviour sanitizers: one k-step of k_matrix_resid_d2m is replayed
// on the host, patch by patch and thread by thread, over padded planes of many shapes and
// with every set of sides that carry a connection surface.  Every plane position is owned
// exactly once; the slot each of a physical cell's four neighbours is read from was written
// in the same step, by the owner or by a rim load, with the position pos2(ie -+ 1, je) /
// pos2(ie, je -+ 1) -- and so were the face statics of the upper two; the XCD dealing visits
// every patch once per k-chunk; the k-chunks cover [0, nk) once.
#include <cstdio>
#include <vector>

#include "../../aither_amd/csrc/agx_mresid_plan.hpp"

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("mresid_plan: %s failed at line %d\n", #cond, __LINE__);   \
      return 1;                                                              \
    }                                                                        \
  } while (0)

using namespace agx;

// the D2 layout's own statement of a position (agx_lusgs.hpp: a table of diagonal starts)
struct Table {
  int Pi, Pj;
  std::vector<int> dstart;
  Table(int pi, int pj) : Pi(pi), Pj(pj), dstart((size_t)(pi + pj), 0) {
    int n = 0;
    for (int de = 0; de < pi + pj - 1; ++de) {
      dstart[(size_t)de] = n;
      for (int je = 0; je < pj; ++je)
        if (de - je >= 0 && de - je < pi) ++n;
    }
    dstart[(size_t)(pi + pj - 1)] = n;
  }
  int pos2(int ie, int je) const {
    const int de = ie + je, jlo = de - (Pi - 1) > 0 ? de - (Pi - 1) : 0;
    return dstart[(size_t)de] + je - jlo;
  }
};

static bool wanted(int kind, int conn) {
  return kind == MRP_CELL || (kind > 0 && (conn >> (kind - 1) & 1));
}

static int walk_plane(int Pi, int Pj, int ng, long& patches_seen) {
  const MrpPlane p{Pi, Pj, ng};
  const Table tab(Pi, Pj);
  const int ni = Pi - 2 * ng, nj = Pj - 2 * ng;
  REQUIRE(ni >= 1 && nj >= 1);
  const int npatch = mrp_patches(p);
  REQUIRE(npatch >= 1);
  for (int de = 0; de < mrp_ndiag(p); ++de) REQUIRE(mrp_dstart(p, de) == tab.dstart[(size_t)de]);
  std::vector<int> owned((size_t)(Pi * Pj), 0);
  MrpPatch pt;
  REQUIRE(!mrp_patch(p, npatch, pt) && !mrp_patch(p, npatch + 7, pt));
  // (without a ghost layer no side can carry a connection)
  for (int conn = 0; conn < (ng > 0 ? 16 : 1); ++conn) {
    for (int n = 0; n < npatch; ++n) {
      REQUIRE(mrp_patch(p, n, pt));
      REQUIRE(pt.d0 % MRP_W == 0 && pt.d0 < mrp_ndiag(p) && pt.j0 >= 0);
      // the step's stores: position per column slot and per face slot (-1: not written)
      std::vector<int> col((size_t)MRP_SLOTS, -1), face((size_t)MRP_FACE_SLOTS, -1);
      for (int t = 0; t < MRP_THREADS; ++t) {
        const MrpLoad ld[2] = {mrp_own(p, pt, t), mrp_extra(p, pt, t)};
        for (int m = 0; m < 2; ++m) {
          const MrpLoad& o = ld[m];
          if (m == 0 && conn == 0 && mrp_in_plane(p, o.de, o.je))
            ++owned[(size_t)tab.pos2(o.de - o.je, o.je)];
          if (m == 1 && t >= MRP_EXTRAS) REQUIRE(o.kind == MRP_NONE);
          if (!wanted(o.kind, conn)) continue;
          REQUIRE(mrp_in_plane(p, o.de, o.je));
          const int pos = mrp_pos(p, o.de, o.je);
          REQUIRE(pos == tab.pos2(o.de - o.je, o.je) && pos >= 0 && pos < Pi * Pj);
          REQUIRE(o.slot >= 0 && o.slot < MRP_SLOTS && o.fslot >= -1 && o.fslot < MRP_FACE_SLOTS);
          REQUIRE(col[(size_t)o.slot] == -1);        // one writer per slot
          col[(size_t)o.slot] = pos;
          if (o.fslot >= 0) {
            REQUIRE(face[(size_t)o.fslot] == -1);
            face[(size_t)o.fslot] = pos;
          }
        }
      }
      // the step's reads: the neighbours the kernel takes of a physical cell
      for (int t = 0; t < MRP_THREADS; ++t) {
        const MrpLoad me = mrp_own(p, pt, t);
        if (me.kind != MRP_CELL) continue;
        const int w = t / MRP_L, l = t % MRP_L;      // row, column
        const int ie = me.de - me.je, je = me.je, i = ie - ng, j = je - ng;
        REQUIRE(i >= 0 && i < ni && j >= 0 && j < nj);
        const bool use[4] = {i > 0 || (conn & 1), j > 0 || (conn & 4), i < ni - 1 || (conn & 2),
                             j < nj - 1 || (conn & 8)};
        const int nie[4] = {ie - 1, ie, ie + 1, ie}, nje[4] = {je, je - 1, je, je + 1};
        for (int q = 0; q < 4; ++q) {
          const MrpNb nb = mrp_neighbour(pt, w, l, q);
          REQUIRE(nb.de == nie[q] + nje[q] && nb.je == nje[q]);
          REQUIRE(nb.slot >= 0 && nb.slot < MRP_SLOTS);
          REQUIRE((q < 2) == (nb.fslot < 0) && nb.fslot < MRP_FACE_SLOTS);
          if (!use[q]) continue;
          // (with ng = 0 a rim cell has no neighbour beyond the plane; the kernel has ng >= 1)
          REQUIRE(nie[q] >= 0 && nie[q] < Pi && nje[q] >= 0 && nje[q] < Pj);
          REQUIRE(col[(size_t)nb.slot] == tab.pos2(nie[q], nje[q]));
          if (q >= 2) REQUIRE(face[(size_t)nb.fslot] == tab.pos2(nie[q], nje[q]));
        }
      }
    }
  }
  for (int pos = 0; pos < Pi * Pj; ++pos) REQUIRE(owned[(size_t)pos] == 1);
  // the XCD dealing and the k-chunks
  const int per = mrp_per_xcd(npatch);
  const int kcs[3] = {1, 5, 32};
  for (int kc : kcs) {
    const int nks[6] = {1, kc - 1, kc, kc + 1, 2 * kc + 1, 3 * kc - 1};
    for (int nk : nks) {
      if (nk < 1) continue;
      const int nch = mrp_kchunks(nk, kc);
      std::vector<int> planes((size_t)nk, 0);
      for (int c = 0; c < nch; ++c) {
        int k0, k1;
        mrp_kchunk(nk, kc, c, k0, k1);
        REQUIRE(k0 >= 0 && k0 < k1 && k1 <= nk && k1 - k0 <= kc);
        for (int k = k0; k < k1; ++k) ++planes[(size_t)k];
      }
      for (int k = 0; k < nk; ++k) REQUIRE(planes[(size_t)k] == 1);
      const long nwg = mrp_wgs(npatch, nk, kc);
      REQUIRE(nwg == 8L * per * nch && nwg < 0x7fffffffL);
      std::vector<int> seen((size_t)npatch * nch, 0);
      for (int wg = 0; wg < (int)nwg; ++wg) {
        const MrpWg d = mrp_deal(wg, per);
        REQUIRE(d.kch >= 0 && d.kch < nch && d.patch >= 0 && d.patch < 8 * per);
        // an XCD (wg % 8) holds a contiguous range of the patch sequence
        REQUIRE(d.patch / per == wg % 8);
        if (d.patch < npatch) ++seen[(size_t)d.kch * npatch + d.patch];
      }
      for (int v : seen) REQUIRE(v == 1);
    }
  }
  patches_seen += npatch;
  return 0;
}

int main() {
  // (Pi, Pj, ng): diagonals shorter than a wave, longer than one run, Pi >> Pj and Pj >> Pi,
  // 1 x n and n x 1, the planes of the device tests and the padded plane of the benchmark
  // (256 + 2 * 3)
  const int shapes[][3] = {{5, 5, 1},   {9, 7, 1},    {11, 13, 3},  {76, 9, 3},   {9, 76, 3},
                           {74, 72, 3}, {300, 4, 1},  {4, 300, 1},  {1, 9, 0},    {9, 1, 0},
                           {1, 200, 0}, {3, 130, 1},  {130, 3, 1},  {64, 64, 2},  {65, 66, 2},
                           {128, 67, 2}, {1, 1, 0},   {262, 262, 3}, {260, 260, 2}};
  long patches = 0;
  int planes = 0;
  for (const auto& s : shapes) {
    if (walk_plane(s[0], s[1], s[2], patches)) {
      std::printf("mresid_plan: plane %d x %d, ng %d\n", s[0], s[1], s[2]);
      return 1;
    }
    ++planes;
  }
  std::printf("mresid_plan: %d planes, %ld patches walked\n", planes, patches);
  return 0;
}
