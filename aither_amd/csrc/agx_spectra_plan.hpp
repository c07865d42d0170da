// agx_spectra_plan.hpp -- the line, bin, chunk and twiddle-index arithmetic of the spectra
// (agx_spectra.hpp), in plain C++ for host and device: the kernels, the host path and
// tests/cpp/spectra_plan.cpp (an exhaustive walk under the host sanitizers) share it.
//
// Directions: `along` is transformed; of the other two, d1 is the lower index direction and d2
// the higher (along i: j, k; along j: i, k; along k: i, j).  A line is a position (p1, p2) of
// (d1, d2).  Each of d1, d2 is pooled (a bit of `over`) or remains; a bin is a position of the
// remaining ones, the lower direction fastest.
// A workgroup loads a TILE: `tl` consecutive positions of d1 at one p2 (the last tile of a row
// may hold fewer).  A thread takes a mode and a GROUP of SPECTRA_LB consecutive lines of the
// tile.  The tiles a workgroup marches through are its STEPS: step st of a row of pooled
// directions is tile st % nt1 (where d1 is pooled, else the workgroup's own tile) at
// p2 = st / nt1 (where d2 is pooled, else the workgroup's own), cut into chunks of
// SPECTRA_CHUNK steps.  One RECORD per (chunk, group) where d1 is pooled -- the lines of a
// group lie in one bin --, one per chunk where it is not -- every line of the tile is a bin of
// its own.  A bin's records are joined in ascending record order.
#pragma once

#if defined(__HIPCC__)
#define AGX_SPECTRA_HD __host__ __device__
#else
#define AGX_SPECTRA_HD
#endif

namespace agx {

constexpr int SPECTRA_MAX_N = 1024;        // longest line (AGX_SPECTRA_MAX_N of the header)
constexpr int SPECTRA_MAX_VAR = 6;
constexpr int SPECTRA_MAX_PAIR = 15;
constexpr int SPECTRA_LDS_DOUBLES = 10240; // 80 KiB of a CU's 160: two workgroups per CU
constexpr int SPECTRA_LDS_SMALL = 4096;    // the kernel form for plans that need no more: 32 KiB
constexpr int SPECTRA_TILE = 64;           // widest tile: a 512-byte row of i
constexpr int SPECTRA_LB = 4;              // lines of a thread
constexpr int SPECTRA_CHUNK = 8;           // steps of a record

struct SpectraShape {
  int along, over;       // 0 i, 1 j, 2 k; mask bit 0 i, 1 j, 2 k
  int nvar, npair;
  int n;                 // N, the line's cells
  int nmode;             // N / 2 + 1
  int d1, d2;            // the other directions, d1 < d2
  int n1, n2;            // their extents
  int pool1, pool2;      // 1: pooled
  int tl, nt1, ng;       // lines of a full tile, tiles of a row of d1, groups of a tile
  long steps, nchunk;    // of a workgroup's march; its chunks
  long nfix;             // the workgroups of one chunk index: (tile, p2) that are not marched
  long nbin, nrec;       // bins; records of a bin
  long lines;            // lines of a bin
};

// the index of the canonical pair (a < b) of nvar <= 6 variables in the enumeration
// (0,1) (0,2) ... (0,5) (1,2) ...: what the kernels' unrolled loops count
AGX_SPECTRA_HD constexpr int spectra_pair_index(int a, int b) {
  return a * (2 * SPECTRA_MAX_VAR - a - 1) / 2 + (b - a - 1);
}

// LDS of the line kernel, in doubles: the twiddles (cos, sin) of N, then the tile
// [n][var][line], then the line means [var][line]
AGX_SPECTRA_HD constexpr long spectra_lds_doubles(int n, int nvar, int tl) {
  return 2L * n + (long)nvar * tl * n + (long)nvar * tl;
}

// the shape of a plan on a block of ext[3] = {ni, nj, nk} cells; false: N is out of range
// (2 ... SPECTRA_MAX_N).  along in 0..2, over a mask without the bit of along, nvar in 1..6.
AGX_SPECTRA_HD inline bool spectra_shape(const int ext[3], int along, int over, int nvar,
                                         int npair, SpectraShape* s) {
  s->along = along; s->over = over; s->nvar = nvar; s->npair = npair;
  s->n = ext[along];
  if (s->n < 2 || s->n > SPECTRA_MAX_N) return false;
  s->nmode = s->n / 2 + 1;
  s->d1 = along == 0 ? 1 : 0;
  s->d2 = along == 2 ? 1 : 2;
  s->n1 = ext[s->d1]; s->n2 = ext[s->d2];
  s->pool1 = over >> s->d1 & 1; s->pool2 = over >> s->d2 & 1;
  // the widest tile the LDS holds, a multiple of the thread's lines where it can be.  The
  // tile is that of a plan of SPECTRA_MAX_VAR variables whatever nvar is: tiles, groups,
  // records and with them every order of pooling are functions of the extents, along and over
  // alone, so a plan of a subset of the variables returns the same bits for what it shares (a
  // plan of fewer variables uses less of the LDS, and the launch asks for less)
  long cap = (SPECTRA_LDS_DOUBLES - 2L * s->n) / ((long)SPECTRA_MAX_VAR * (s->n + 1));
  int tl = cap < SPECTRA_TILE ? (int)cap : SPECTRA_TILE;
  if (tl > s->n1) tl = s->n1;
  if (tl > SPECTRA_LB) {
    // whole groups, and of those widths the one with the most lines per pass of the 256
    // threads over the (mode, group) units; the wider of equals
    tl -= tl % SPECTRA_LB;
    int best = tl;
    long best_num = 0, best_den = 1;
    for (int t = SPECTRA_LB; t <= tl; t += SPECTRA_LB) {
      const long passes = ((long)(s->n / 2) * (t / SPECTRA_LB) + 255) / 256;
      if (t * best_den >= best_num * passes) { best = t; best_num = t; best_den = passes; }
    }
    tl = best;
  }
  s->tl = tl;
  s->nt1 = (s->n1 + tl - 1) / tl;
  s->ng = (tl + SPECTRA_LB - 1) / SPECTRA_LB;
  s->steps = (long)(s->pool1 ? s->nt1 : 1) * (s->pool2 ? s->n2 : 1);
  s->nchunk = (s->steps + SPECTRA_CHUNK - 1) / SPECTRA_CHUNK;
  s->nfix = (long)(s->pool1 ? 1 : s->nt1) * (s->pool2 ? 1 : s->n2);
  s->nbin = (long)(s->pool1 ? 1 : s->n1) * (s->pool2 ? 1 : s->n2);
  s->nrec = s->nchunk * (s->pool1 ? s->ng : 1);
  s->lines = (long)(s->pool1 ? s->n1 : 1) * (s->pool2 ? s->n2 : 1);
  return true;
}

// workgroup wg of the line kernel: its chunk and the tile / p2 it does not march through
struct SpectraGroup { long chunk; int tile, p2; };
AGX_SPECTRA_HD inline SpectraGroup spectra_workgroup(const SpectraShape& s, long wg) {
  SpectraGroup g;
  const long fix = wg % s.nfix;
  g.chunk = wg / s.nfix;
  g.tile = s.pool1 ? 0 : (int)(fix % s.nt1);
  g.p2 = s.pool2 ? 0 : (int)(s.pool1 ? fix : fix / s.nt1);
  return g;
}
// step st of a workgroup's march: the tile and p2 it loads
AGX_SPECTRA_HD inline void spectra_step(const SpectraShape& s, const SpectraGroup& g, long st,
                                        int* tile, int* p2) {
  *tile = s.pool1 ? (int)(st % s.nt1) : g.tile;
  *p2 = s.pool2 ? (int)(s.pool1 ? st / s.nt1 : st) : g.p2;
}
// valid lines of a tile, and of group gr of it
AGX_SPECTRA_HD inline int spectra_tile_lines(const SpectraShape& s, int tile) {
  const int left = s.n1 - tile * s.tl;
  return left < s.tl ? left : s.tl;
}
AGX_SPECTRA_HD inline int spectra_group_lines(const SpectraShape& s, int tile, int gr) {
  const int left = spectra_tile_lines(s, tile) - gr * SPECTRA_LB;
  return left < 0 ? 0 : left < SPECTRA_LB ? left : SPECTRA_LB;
}
// the bin of line p1 (position in d1) at p2
AGX_SPECTRA_HD inline long spectra_bin(const SpectraShape& s, int p1, int p2) {
  if (s.pool1) return s.pool2 ? 0 : p2;
  return s.pool2 ? p1 : (long)p2 * s.n1 + p1;
}
// the record of (chunk, group): where d1 remains every group writes the chunk's one record
AGX_SPECTRA_HD inline long spectra_record(const SpectraShape& s, long chunk, int gr) {
  return s.pool1 ? chunk * s.ng + gr : chunk;
}
// lines a record of a bin holds: those of its group over the steps of its chunk (where d1
// remains: one line per step)
AGX_SPECTRA_HD inline long spectra_record_lines(const SpectraShape& s, long rec) {
  const long chunk = s.pool1 ? rec / s.ng : rec;
  const int gr = s.pool1 ? (int)(rec % s.ng) : 0;
  const long s0 = chunk * SPECTRA_CHUNK;
  const long s1 = s0 + SPECTRA_CHUNK < s.steps ? s0 + SPECTRA_CHUNK : s.steps;
  if (!s.pool1) return s1 - s0;
  long count = 0;
  for (long st = s0; st < s1; ++st) count += spectra_group_lines(s, (int)(st % s.nt1), gr);
  return count;
}
// cell (i, j, k) of entry n of the line at (p1, p2)
AGX_SPECTRA_HD inline void spectra_cell(const SpectraShape& s, int n, int p1, int p2, int ijk[3]) {
  ijk[s.along] = n; ijk[s.d1] = p1; ijk[s.d2] = p2;
}
// the twiddle index of the next cell of mode m: q = m n mod N without a product
AGX_SPECTRA_HD inline int spectra_next_q(int q, int m, int n) {
  q += m;
  return q >= n ? q - n : q;
}
// doubles of the record buffer and of the accumulators
AGX_SPECTRA_HD inline long spectra_values(const SpectraShape& s) {
  return (long)(s.nvar + s.npair) * s.nbin * s.nmode;
}

}  // namespace agx
