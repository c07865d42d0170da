// agx_spectra.hpp -- wavenumber spectra and co-spectra along a homogeneous index direction,
// accumulated on the device (include/aither_gfx950.h, AGX_FIELD_SPECTRA_PLAN / _SAMPLE /
// _ACCUM / _VALUES).
//
// A line is one run of N physical cells along the plan's direction.  Per line and variable a:
//     mu_a  = (sum_n x_n) / N                        (serial, ascending n)
//     y_n   = x_n - mu_a
//     X_a,m = sum_n y_n (cos - i sin)(2 pi q / N),   q = m n mod N,   m = 1 ... N / 2
//     P_a,m = c_m |X_a,m|^2 / N^2,   C_ab,m = c_m Re(X_a,m conj X_b,m) / N^2
// with c_m = 2, and 1 at m = N / 2 of an even N; entry m = 0 is mu_a^2 (mu_a mu_b).  The sum
// over m is the line mean of x_a x_b (Parseval).  The mean goes before the transform: on
// pressure-like data, 1 + 1e-8 noise, the raw transform loses every digit of the spectrum.
// The twiddles are a table of N (cos, sin) pairs rounded from extended precision on the host;
// q is stepped (agx_spectra_plan.hpp), never an angle that grows.
//
// The lines of a bin pool with EQUAL weights (pooled directions are homogeneous; the volume
// weights of the collapsed statistics are deliberately not used):
//     M += (p - M) / l                      line l = 1, 2, ... of a record
//     M += (c2 / (c1 + c2)) (M2 - M)        records of c1, c2 lines, ascending record order
// and samples join by the weighted running mean S += (w / W) (M - S).  All three are compiled
// without contraction: identical lines, records or samples leave the difference 0 and the bits
// of one line.  No atomics; the order of every sum is a function of the block's extents and
// the plan (agx_spectra_plan.hpp), so two runs give the same bits; a spectrum is a function of
// its own one or two variables, the inner product is written with explicit fma and the
// spectrum's own arithmetic without contraction, so a plan of a subset, or in another order,
// returns the same bits for what it shares.
//
// k_spectra_lines: a workgroup marches through the tiles of one chunk (the tile is sized for a
// plan of six variables whatever the plan holds, agx_spectra_plan.hpp: the grouping of lines
// into records, and so the bits, do not depend on the number of variables).  Per tile: the planned
// variables of tl lines go to LDS as [n][var][line] (along j or k the tile is a row of i, a
// coalesced load per n; along i a line is contiguous), a thread per (var, line) sums the
// line, subtracts the mean in place and keeps it; then a thread per (mode, group of 4 lines)
// -- lanes take consecutive modes, so a data read is an LDS broadcast and the twiddle read is
// strided -- forms re / im of all variables of its 4 lines in ascending n by vector fma (the
// twiddle pair is read once per n for 8 NV fma) and pools the spectra into its record, which
// the thread owns for the whole chunk (a read-modify-write of global memory no other thread
// touches).  k_spectra_join: a thread per (spectrum, bin, mode) joins the bin's records in
// ascending order and applies the recurrence in time.
#pragma once
#include "agx_kernels.hpp"
#include "agx_spectra_plan.hpp"

namespace agx {

struct SpectraDev {
  SpectraShape s;
  int var[SPECTRA_MAX_VAR];          // 0 rho, 1 u, 2 v, 3 w, 4 p, 5 T
  int pair_spec[SPECTRA_MAX_PAIR];   // spectrum of the canonical pair (a < b), or -1
};

// variable `code` of the cell at q, nondimensional, as k_stats_cells forms it
__device__ __forceinline__ double spectra_var(const BlockDev& b, const GasDev& g, int code,
                                              long q) {
  if (code == 5) return b.state[4][q] / (b.state[0][q] * g.R);
  const double* pl = code == 0 ? b.state[0] : code == 1 ? b.state[1] : code == 2 ? b.state[2]
                     : code == 3 ? b.state[3] : b.state[4];
  return pl[q];
}

// one line's spectrum p into the running mean of its record: line number cnt (1: the first)
__device__ __forceinline__ void spectra_pool(double* slot, double p, long cnt) {
#pragma clang fp contract(off)
  const double m = cnt == 1 ? 0.0 : *slot;
  *slot = m + (p - m) / (double)cnt;
}

// one entry of a line's (co-)spectrum from the transforms of its two variables (the same one
// twice: the auto-spectrum); at m = 0 re holds the line means
__device__ __forceinline__ double spectra_entry(bool zero, double cm, double n2, double re_a,
                                                double im_a, double re_b, double im_b) {
#pragma clang fp contract(off)
  return zero ? re_a * re_b : cm * (re_a * re_b + im_a * im_b) / n2;
}

// LDSD: the doubles of LDS this form declares, SPECTRA_LDS_DOUBLES or SPECTRA_LDS_SMALL (the
// tile does not depend on the number of variables, so a plan of few variables or short lines
// needs a fraction of the LDS and more workgroups fit a CU); the host picks the form that
// holds spectra_lds_doubles(N, NV, tl).
template <int NV, int LDSD>
__global__ void __launch_bounds__(256)
k_spectra_lines(BlockDev b, GasDev g, SpectraDev pd, const double* __restrict__ tw_g,
                double* part) {
  __shared__ double lds[LDSD];
  const SpectraShape& s = pd.s;
  constexpr int LB = SPECTRA_LB;
  const int N = s.n, TL = s.tl, tid = threadIdx.x;
  double* tw = lds;
  double* D = lds + 2 * N;
  double* MU = D + (long)NV * TL * N;
  for (int t = tid; t < 2 * N; t += 256) tw[t] = tw_g[t];
  const SpectraGroup wg = spectra_workgroup(s, blockIdx.x);
  const long s0 = wg.chunk * SPECTRA_CHUNK;
  const long s1 = s0 + SPECTRA_CHUNK < s.steps ? s0 + SPECTRA_CHUNK : s.steps;
  const int nspec = s.nvar + s.npair, NM1 = s.nmode - 1;
  const long rec_pitch = (long)nspec * s.nbin * s.nmode;
  const double n2 = (double)N * (double)N;
  for (long st = s0; st < s1; ++st) {
    int tile, p2;
    spectra_step(s, wg, st, &tile, &p2);
    const int tlv = spectra_tile_lines(s, tile), l0 = tile * TL;
    __syncthreads();       // (the twiddles are in; the last step's readers are through)
    for (int u = tid; u < N * TL; u += 256) {
      const int n = s.along == 0 ? u % N : u / TL, l = s.along == 0 ? u / N : u % TL;
      double x[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) x[v] = 0.0;
      if (l < tlv) {
        int c[3];
        spectra_cell(s, n, l0 + l, p2, c);
        const long q = b.idx(c[0], c[1], c[2]);
#pragma unroll
        for (int v = 0; v < NV; ++v) x[v] = spectra_var(b, g, pd.var[v], q);
      }
#pragma unroll
      for (int v = 0; v < NV; ++v) D[((long)n * NV + v) * TL + l] = x[v];
    }
    __syncthreads();
    for (int u = tid; u < NV * TL; u += 256) {
      // (u = v TL + l: the line of variable v at [n][v][l])
      double* line = D + (long)(u / TL) * TL + u % TL;
      const long pitch = (long)NV * TL;
      double sum = 0.0;
      for (int n = 0; n < N; ++n) sum += line[n * pitch];
      const double mu = sum / (double)N;
      for (int n = 0; n < N; ++n) line[n * pitch] -= mu;
      MU[u] = mu;
    }
    __syncthreads();
    // units: (mode 1 ... N/2, group), lanes along the modes; then the groups' entries m = 0
    for (int u = tid; u < (NM1 + 1) * s.ng; u += 256) {
      const bool zero = u >= NM1 * s.ng;
      const int m = zero ? 0 : 1 + u % NM1, gr = zero ? u - NM1 * s.ng : u / NM1;
      const int gl = spectra_group_lines(s, tile, gr);
      if (gl == 0) continue;
      double re[NV][LB], im[NV][LB];
      if (zero) {
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
          for (int j = 0; j < LB; ++j) {
            // (a short last group: the slot of a line that is not there is not read)
            re[v][j] = j < gl ? MU[v * TL + gr * LB + j] : 0.0;
            im[v][j] = 0.0;
          }
      } else {
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
          for (int j = 0; j < LB; ++j) re[v][j] = im[v][j] = 0.0;
        const bool full = gl == LB;
        const double* d = D + gr * LB;
        int q = 0;
        for (int n = 0; n < N; ++n) {
          const double cs = tw[2 * q], sn = tw[2 * q + 1];
#pragma unroll
          for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int j = 0; j < LB; ++j) {
              // (a tile narrower than a group: TL < LB, the lines beyond it are not in LDS)
              const double y = full || j < gl ? d[v * TL + j] : 0.0;
              re[v][j] = fma(y, cs, re[v][j]);
              im[v][j] = fma(y, sn, im[v][j]);
            }
          d += (long)NV * TL;
          q = spectra_next_q(q, m, N);
        }
      }
      // where d1 is pooled the group's lines follow one another in one record of one bin;
      // where it remains each line is a bin and the record counts the steps
      long before = 0;
      if (s.pool1)
        for (long sp = s0; sp < st; ++sp)
          before += spectra_group_lines(s, (int)(sp % s.nt1), gr);
      else
        before = st - s0;
      const long rec = spectra_record(s, wg.chunk, gr);
      const double cm = (!zero && 2 * m == N) ? 1.0 : 2.0;
#pragma unroll
      for (int j = 0; j < LB; ++j) {
        if (j >= gl) continue;
        const long bin = spectra_bin(s, l0 + gr * LB + j, p2);
        const long cnt = s.pool1 ? before + j + 1 : before + 1;
        double* slot = part + rec * rec_pitch + bin * s.nmode + m;
        const long sp_pitch = s.nbin * s.nmode;
#pragma unroll
        for (int a = 0; a < NV; ++a)
          spectra_pool(slot + a * sp_pitch,
                       spectra_entry(zero, cm, n2, re[a][j], im[a][j], re[a][j], im[a][j]), cnt);
#pragma unroll
        for (int a = 0; a < NV; ++a)
#pragma unroll
          for (int c = a + 1; c < NV; ++c) {
            const int sx = pd.pair_spec[spectra_pair_index(a, c)];
            if (sx < 0) continue;
            spectra_pool(slot + sx * sp_pitch,
                         spectra_entry(zero, cm, n2, re[a][j], im[a][j], re[c][j], im[c][j]),
                         cnt);
          }
      }
    }
  }
}

// One thread per (spectrum, bin, mode), t = (spectrum nbin + bin) nmode + m: the bin's records
// in ascending order (lines[rec]: the lines a record holds; an empty one is skipped), then
// S += r (M - S) with r = w / W of the sample.
__global__ void __launch_bounds__(256)
k_spectra_join(long total, long nrec, const double* __restrict__ lines,
               const double* __restrict__ part, double r, double* __restrict__ S) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  {
#pragma clang fp contract(off)
    double M = 0.0, cnt = 0.0;
    for (long rec = 0; rec < nrec; ++rec) {
      const double c2 = lines[rec];
      if (c2 == 0.0) continue;
      cnt = cnt + c2;
      M = M + (c2 / cnt) * (part[rec * total + t] - M);
    }
    const double old = S[t];
    S[t] = old + r * (M - old);
  }
}

}  // namespace agx
