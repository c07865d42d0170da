// The line, bin, chunk and twiddle-index arithmetic of the spectra
// (aither_amd/csrc/agx_spectra_plan.hpp) under the address and undefined-behaviour sanitizers:
// the walk of k_spectra_lines is replayed on the host, workgroup by workgroup, step by step,
// unit by unit, over plans of many block shapes.  Every cell of the block is loaded exactly
// once into an LDS slot inside the tile; every record slot is pooled with the line numbers 1,
// 2, 3 ... by one owner; a bin's records hold the lines spectra_record_lines says, and all the
// lines of the bin together; the stepped twiddle index is m n mod N.
// With arguments `shape ni nj nk along over nvar` it prints the plan's shape instead (the host
// test holds the Python restatement's copy of the arithmetic against it).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../aither_amd/csrc/agx_spectra_plan.hpp"

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("spectra_plan: %s failed at line %d\n", #cond, __LINE__);  \
      return 1;                                                              \
    }                                                                        \
  } while (0)

using namespace agx;

static int walk(const int ext[3], int along, int over, int nvar) {
  SpectraShape s;
  const bool ok = spectra_shape(ext, along, over, nvar, 0, &s);
  REQUIRE(ok == (ext[along] >= 2 && ext[along] <= SPECTRA_MAX_N));
  if (!ok) return 0;
  REQUIRE(s.tl >= 1 && s.tl <= SPECTRA_TILE && s.tl <= s.n1);
  REQUIRE(s.tl <= SPECTRA_LB || s.tl % SPECTRA_LB == 0);
  REQUIRE(spectra_lds_doubles(s.n, nvar, s.tl) <= SPECTRA_LDS_DOUBLES);
  REQUIRE(s.nmode == s.n / 2 + 1);
  const long ncell = (long)ext[0] * ext[1] * ext[2];
  REQUIRE(s.nbin * s.lines * s.n == ncell);
  std::vector<char> lds((size_t)SPECTRA_LDS_DOUBLES, 0);
  std::vector<int> seen((size_t)ncell, 0);
  // per (record, bin): the lines pooled so far (the count the owner pooled last)
  std::vector<long> pooled((size_t)(s.nrec * s.nbin), 0);
  const int nm1 = s.nmode - 1;
  for (long wgi = 0; wgi < s.nchunk * s.nfix; ++wgi) {
    const SpectraGroup wg = spectra_workgroup(s, wgi);
    REQUIRE(wg.chunk >= 0 && wg.chunk < s.nchunk);
    const long s0 = wg.chunk * SPECTRA_CHUNK;
    const long s1 = s0 + SPECTRA_CHUNK < s.steps ? s0 + SPECTRA_CHUNK : s.steps;
    REQUIRE(s0 < s1);
    for (long st = s0; st < s1; ++st) {
      int tile, p2;
      spectra_step(s, wg, st, &tile, &p2);
      REQUIRE(tile >= 0 && tile < s.nt1 && p2 >= 0 && p2 < s.n2);
      const int tlv = spectra_tile_lines(s, tile), l0 = tile * s.tl;
      REQUIRE(tlv >= 1 && tlv <= s.tl);
      // the loader's units
      std::fill(lds.begin(), lds.end(), 0);
      for (int u = 0; u < s.n * s.tl; ++u) {
        const int n = along == 0 ? u % s.n : u / s.tl, l = along == 0 ? u / s.n : u % s.tl;
        REQUIRE(n < s.n && l < s.tl);
        if (l < tlv) {
          int c[3];
          spectra_cell(s, n, l0 + l, p2, c);
          for (int d = 0; d < 3; ++d) REQUIRE(c[d] >= 0 && c[d] < ext[d]);
          ++seen[((size_t)c[2] * ext[1] + c[1]) * ext[0] + c[0]];
        }
        for (int v = 0; v < nvar; ++v) {
          const long at = 2L * s.n + ((long)n * nvar + v) * s.tl + l;
          REQUIRE(at < 2L * s.n + (long)nvar * s.tl * s.n);
          REQUIRE(lds[(size_t)at] == 0);
          lds[(size_t)at] = 1;
        }
      }
      for (int u = 0; u < nvar * s.tl; ++u) {
        const long at = 2L * s.n + (long)nvar * s.tl * s.n + u;
        REQUIRE(at < SPECTRA_LDS_DOUBLES);
        lds[(size_t)at] = 1;
      }
      // the units of the transform: the slots one (mode, group) owner pools, mode 1 standing
      // for all; every group of the tile is met once
      int lines_met = 0;
      for (int u = 0; u < (nm1 + 1) * s.ng; ++u) {
        const bool zero = u >= nm1 * s.ng;
        const int m = zero ? 0 : 1 + u % nm1, gr = zero ? u - nm1 * s.ng : u / nm1;
        REQUIRE(m <= nm1 && gr < s.ng);
        const int gl = spectra_group_lines(s, tile, gr);
        REQUIRE(gl >= 0 && gl <= SPECTRA_LB && (gl == 0 || gr * SPECTRA_LB + gl <= tlv));
        if (m != 1) continue;
        long before = 0;
        if (s.pool1)
          for (long sp = s0; sp < st; ++sp)
            before += spectra_group_lines(s, (int)(sp % s.nt1), gr);
        else
          before = st - s0;
        const long rec = spectra_record(s, wg.chunk, gr);
        REQUIRE(rec >= 0 && rec < s.nrec);
        for (int j = 0; j < gl; ++j) {
          const long bin = spectra_bin(s, l0 + gr * SPECTRA_LB + j, p2);
          REQUIRE(bin >= 0 && bin < s.nbin);
          const long cnt = s.pool1 ? before + j + 1 : before + 1;
          long& slot = pooled[(size_t)(rec * s.nbin + bin)];
          REQUIRE(slot + 1 == cnt);
          slot = cnt;
          ++lines_met;
        }
      }
      REQUIRE(lines_met == tlv);
    }
  }
  for (long c = 0; c < ncell; ++c) REQUIRE(seen[(size_t)c] == 1);
  for (long bin = 0; bin < s.nbin; ++bin) {
    long total = 0;
    for (long rec = 0; rec < s.nrec; ++rec) {
      REQUIRE(pooled[(size_t)(rec * s.nbin + bin)] == spectra_record_lines(s, rec));
      total += spectra_record_lines(s, rec);
    }
    REQUIRE(total == s.lines);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 8 && !std::strcmp(argv[1], "shape")) {
    const int ext[3] = {std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])};
    SpectraShape s;
    if (!spectra_shape(ext, std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7]), 0, &s)) {
      std::printf("refused\n");
      return 0;
    }
    std::printf("%d %d %d %ld %ld %ld %ld %ld %ld", s.tl, s.nt1, s.ng, s.steps, s.nchunk, s.nfix,
                s.nbin, s.nrec, s.lines);
    for (long r = 0; r < s.nrec; ++r) std::printf(" %ld", spectra_record_lines(s, r));
    std::printf("\n");
    return 0;
  }
  // the stepped twiddle index
  for (int n = 2; n <= 1024; n = n < 40 ? n + 1 : n * 2 + 1)
    for (int m = 0; m <= n / 2; ++m) {
      int q = 0;
      for (int k = 0; k < n; ++k) {
        REQUIRE(q == (int)((long)m * k % n));
        q = spectra_next_q(q, m, n);
        REQUIRE(q >= 0 && q < n);
      }
    }
  // the canonical pairs: a bijection onto 0 ... 14
  int hit[SPECTRA_MAX_PAIR] = {};
  for (int a = 0; a < SPECTRA_MAX_VAR; ++a)
    for (int b = a + 1; b < SPECTRA_MAX_VAR; ++b) {
      const int p = spectra_pair_index(a, b);
      REQUIRE(p >= 0 && p < SPECTRA_MAX_PAIR);
      ++hit[p];
    }
  for (int p = 0; p < SPECTRA_MAX_PAIR; ++p) REQUIRE(hit[p] == 1);
  // plans: every small shape, then long lines, wide rows and many steps
  long plans = 0;
  const int big[][3] = {{67, 3, 2},  {2, 3, 130},  {130, 70, 3}, {256, 20, 9},  {9, 256, 20},
                        {20, 9, 256}, {1024, 5, 2}, {3, 1024, 2}, {70, 2, 1024}, {1025, 2, 2},
                        {66, 9, 6},  {200, 1, 37},  {1, 100, 19}, {13, 37, 1}};
  for (int pass = 0; pass < 2; ++pass) {
    const int count = pass == 0 ? 9 * 9 * 9 : (int)(sizeof big / sizeof big[0]);
    for (int e = 0; e < count; ++e) {
      int ext[3];
      if (pass == 0) { ext[0] = 1 + e % 9; ext[1] = 1 + e / 9 % 9; ext[2] = 1 + e / 81; }
      else std::memcpy(ext, big[e], sizeof ext);
      for (int along = 0; along < 3; ++along)
        for (int over = 0; over < 8; ++over) {
          if (over >> along & 1) continue;
          for (int nvar = 1; nvar <= SPECTRA_MAX_VAR; nvar += pass == 0 ? 5 : 1) {
            if (walk(ext, along, over, nvar)) {
              std::printf("spectra_plan: block %d x %d x %d along %d over %d nvar %d\n", ext[0],
                          ext[1], ext[2], along, over, nvar);
              return 1;
            }
            ++plans;
          }
        }
    }
  }
  std::printf("spectra_plan: %ld plans walked\n", plans);
  return 0;
}
