// Ensemble summary of a forecast (no model): per (window, day, region) group of the S Monte-Carlo
// samples of y_hat (T, S*B, R) -- the predictive mean, the population standard deviation, quantiles
// and, against targets, the per-day scores of lib/Metrics.py (nll, log mass of [y - 0.5, y + 0.6],
// mae) -- what lib/utils.py:21-26 / :53-54 of the reference form in NumPy / SciPy over a host copy
// of the whole (B, S, T, R) prediction.
//
// One read of y_hat: for a fixed (t, s) the B*R group values are contiguous, so a workgroup takes
// G neighbouring groups of one t and loads its [S][G] tile row by row (coalesced) into LDS as
// scaled doubles; mean and std (two passes) come from the tile, the quantiles from the tile sorted
// in place along S by a bitonic compare-exchange network (all threads, padded to a power of two with
// +inf).  Every workgroup writes one fp64 partial per score; a second launch sums the partials of
// each t in a fixed order (no atomics: the same bits run to run).  grid.y is t, so no workgroup
// straddles two time indices.  Everything after the load is fp64: the difference of two normal CDFs
// and its == 0 floor agree with SciPy's only there, and the work is one group per (t, b, r).
//
// The VERIFY variant (ude_forecast_verify) scores the ensemble itself from the same, always sorted,
// tile: CRPS, the weighted interval score, interval coverage, the PIT bin of the target's mid-rank
// and the empirical mass of the multibin window.  Per-day values go through per-workgroup partials
// as above; per-region values through a per-group terms scratch that a second kernel sums over b.
// The body is one template: the instantiation behind ude_forecast_summary has no VERIFY code, and
// the VERIFY one runs the shared code first, so the six shared outputs have the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace ude {

constexpr int FC_THREADS = 256;
constexpr int FC_TILE_ELEMS = 4096;      // [S][G] doubles: 32 KiB, four workgroups per CU by LDS
constexpr int FC_MAX_G = 64;
constexpr int FC_MAX_SQ = 1024;          // largest S with quantiles (the sorted tile)
constexpr int FC_MAX_ALPHA = 16;         // interval levels of the weighted interval score
constexpr int FC_MAX_PIT = 64;           // PIT histogram bins
constexpr int FC_TERMS = 7;              // per-group terms: nll, log mass, |y - mean|, crps, wis, log
                                         // empirical mass, coverage bits (bit k: interval k holds y)
constexpr int FC_DEAD_BIN = 255;         // PIT bin of a column past B R
constexpr double FC_MASS_FLOOR = 4.5399929762484854e-05;   // lib/Metrics.py mb_log: an exactly zero mass -> e^-10

struct FcGeom {
  int rows;      // tile rows: S, or its power-of-two padding when sorting; 0 = no tile (S too large)
  int G;         // groups per workgroup (power of two)
  int nbx;       // workgroups per time index
};

__host__ __device__ inline int fc_pow2_ceil(int x) { int p = 1; while (p < x) p <<= 1; return p; }
__host__ __device__ inline int fc_pow2_floor(int x) { int p = 1; while (2 * p <= x) p <<= 1; return p; }

__host__ __device__ inline FcGeom fc_geom(int S, int BR, int n_q) {
  FcGeom g;
  g.rows = n_q > 0 ? fc_pow2_ceil(S) : S;
  if (g.rows > FC_TILE_ELEMS) g.rows = 0;                 // n_q == 0 only: y_hat is read from L2 twice
  int G = g.rows ? fc_pow2_floor(FC_TILE_ELEMS / g.rows) : FC_MAX_G;
  if (G > FC_MAX_G) G = FC_MAX_G;
  const int need = fc_pow2_ceil(BR);
  if (G > need) G = need;
  g.G = G;
  g.nbx = (BR + G - 1) / G;
  return g;
}

struct FcArgs {
  const float* yhat;
  const double* scale;
  const float* y_true;
  const double* q;
  double* mean;
  double* std;
  double* quant;
  double* part;        // [T][nbx][3]
  int T, S, B, R, n_q;
};

struct FcVerifyArgs {
  const double* alpha; // [K] interval levels in (0, 1)
  double* vpart;       // [T][nbx][3 + K + J]: crps, wis, log empirical mass, K coverage and J PIT counts
  double* terms;       // [T][FC_TERMS][B R]
  int K, J;
};

// scipy.special.ndtr's branches (cephes ndtr.c) on the fp64 erf / erfc
__device__ __forceinline__ double fc_ndtr(double a) {
  const double x = a * 0.70710678118654752440, z = fabs(x);
  if (z < 0.70710678118654752440) return 0.5 + 0.5 * erf(x);
  const double y = 0.5 * erfc(z);
  return x > 0 ? 1.0 - y : y;
}

// fixed-order tree sum over the row slices of each column: red[rr * G + c], result in red[c]
__device__ __forceinline__ double fc_col_sum(double* red, double v, int rr, int c, int G, int RP) {
  __syncthreads();                               // the previous result has been read
  red[rr * G + c] = v;
  __syncthreads();
  for (int off = RP >> 1; off > 0; off >>= 1) {
    if (rr < off) red[rr * G + c] += red[(rr + off) * G + c];
    __syncthreads();
  }
  return red[c];
}

// numpy.quantile, method 'linear' (numpy/lib/function_base.py _lerp), of the S sorted rows of column c
__device__ __forceinline__ double fc_quantile(const double* tile, int c, int G, int S, double q) {
  const double h = (double)(S - 1) * q;
  int lo = (int)floor(h);
  if (lo < 0) lo = 0;
  if (lo > S - 1) lo = S - 1;
  const int hi = lo + 1 < S ? lo + 1 : S - 1;
  const double gm = h - (double)lo, x = tile[lo * G + c], y = tile[hi * G + c], d = y - x;
  return gm >= 0.5 ? y - d * (1.0 - gm) : x + d * gm;
}

// how many of the S sorted rows of column c are < x (LE: <= x); the +inf padding rows are never read
template <bool LE>
__device__ __forceinline__ int fc_count_below(const double* tile, int c, int G, int S, double x) {
  int lo = 0, hi = S;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const double v = tile[mid * G + c];
    if (LE ? v <= x : v < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// bitonic network along the rows (a power of two) of every column of tile [rows][G], ascending: rows / 2
// compare-exchanges per column and stage over all threads.  Moves values only, so what it sorts keeps its bits.
__device__ __forceinline__ void fc_bitonic_sort(double* tile, int rows, int rr, int c, int G, int RP) {
  const int half = rows >> 1;
  for (int k = 2; k <= rows; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int p = rr; p < half; p += RP) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
        const double x = tile[i * G + c], y = tile[l * G + c];
        const bool up = (i & k) == 0;
        if ((x > y) == up) {
          tile[i * G + c] = y;
          tile[l * G + c] = x;
        }
      }
    }
  }
  __syncthreads();
}

// The ensemble statistics of one column, stated once for the summary / verify kernel and the season
// kernel (ude_season.h).  All threads of the workgroup call them (they go through fc_col_sum); thread
// row rr takes the samples rr, rr + RP, ..

struct FcMoments { double mean, sd; };

// mean and population std (two passes) of val(0) .. val(S - 1)
template <class Val>
__device__ __forceinline__ FcMoments fc_col_moments(double* red, Val val, int S, int rr, int c, int G, int RP) {
  FcMoments m;
  double acc = 0.0;
  for (int s = rr; s < S; s += RP) acc += val(s);
  m.mean = fc_col_sum(red, acc, rr, c, G, RP) / (double)S;
  acc = 0.0;
  for (int s = rr; s < S; s += RP) {
    const double d = val(s) - m.mean;
    acc += d * d;
  }
  m.sd = sqrt(fc_col_sum(red, acc, rr, c, G, RP) / (double)S);
  return m;
}

// CRPS of the S sorted rows x_0 <= .. of column c against y: mean |x_i - y| - sum (2 i - S + 1) x_i / S^2
__device__ __forceinline__ double fc_col_crps(double* red, const double* tile, double y, int S, int rr, int c, int G,
                                              int RP) {
  double w = 0.0, ad = 0.0;
  for (int i = rr; i < S; i += RP) {
    const double x = tile[i * G + c];
    w += (double)(2 * i - S + 1) * x;
    ad += fabs(x - y);
  }
  const double wsum = fc_col_sum(red, w, rr, c, G, RP);
  const double asum = fc_col_sum(red, ad, rr, c, G, RP);
  const double dS = (double)S;
  return asum / dS - wsum / (dS * dS);
}

// log of the mass the S sorted rows of column c give the multibin window [cb - 0.5, cb + 0.6),
// cb = floor(10 y) / 10 (lib/Metrics.py mb_log(bins=True)); an empty window counts as FC_MASS_FLOOR.
// One thread's work: no fc_col_sum.
__device__ __forceinline__ double fc_window_log_mass(const double* tile, int c, int G, int S, double y) {
  const double cb = floor(y * 10.0) / 10.0;
  const int n = fc_count_below<false>(tile, c, G, S, cb + 0.6) - fc_count_below<false>(tile, c, G, S, cb - 0.5);
  return log(n == 0 ? FC_MASS_FLOOR : (double)n / (double)S);
}

// The two fixed-order sums of the reduce kernels (no atomics: the same bits run to run).
// One wave: entry k of the partials first .. first + n - 1 of part [..][width], lane-strided then a fixed
// butterfly; every lane has the sum
__device__ __forceinline__ double fc_wave_sum(const double* part, size_t first, int n, int width, int k, int ln) {
  double s = 0.0;
  for (int i = ln; i < n; i += 64) s += part[(first + i) * width + k];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

// One thread: (p[0] + p[R] + .. + p[(B - 1) R], in that order) / B
__device__ __forceinline__ double fc_group_mean(const double* p, int B, int R) {
  double acc = 0.0;
#pragma unroll 8
  for (int b = 0; b < B; ++b) acc += p[(size_t)b * R];
  return acc / (double)B;
}

template <bool VERIFY>
__device__ __forceinline__ void fc_summary_body(const FcArgs& a, const FcVerifyArgs& v) {
  extern __shared__ __attribute__((aligned(16))) double fc_lds[];
  const int BR = a.B * a.R;
  const FcGeom ge = fc_geom(a.S, BR, VERIFY ? 1 : a.n_q);   // VERIFY always sorts
  const int G = ge.G, RP = FC_THREADS / G, rows = ge.rows;
  double* red = fc_lds;                          // [RP][G] = 256 doubles
  double* tile = fc_lds + FC_THREADS;            // [rows][G]
  const int tid = threadIdx.x, c = tid & (G - 1), rr = tid / G;
  const int t = blockIdx.y, g = blockIdx.x * G + c;
  const bool live = g < BR;
  const int b = live ? g / a.R : 0, r = live ? g - b * a.R : 0;
  const double sc = (live && a.scale) ? a.scale[r] : 1.0;
  const float* src = a.yhat + (size_t)t * a.S * BR + g;
  const bool tiled = rows > 0;

  if (tiled) {
    for (int s = rr; s < rows; s += RP)
      tile[s * G + c] = s < a.S ? (live ? (double)src[(size_t)s * BR] * sc : 0.0) : (double)INFINITY;
  }
  auto val = [&](int s) -> double {
    if (tiled) return tile[s * G + c];
    return live ? (double)src[(size_t)s * BR] * sc : 0.0;
  };
  if (tiled) __syncthreads();
  const FcMoments mo = fc_col_moments(red, val, a.S, rr, c, G, RP);
  const double mean = mo.mean, sd = mo.sd;
  const size_t o = ((size_t)b * a.T + t) * a.R + r;
  if (live && rr == 0) {
    a.mean[o] = mean;
    a.std[o] = sd;
  }

  if (VERIFY || a.n_q > 0) {
    fc_bitonic_sort(tile, rows, rr, c, G, RP);
    if (live) {
      for (int k = rr; k < a.n_q; k += RP)
        a.quant[(((size_t)k * a.B + b) * a.T + t) * a.R + r] = fc_quantile(tile, c, G, a.S, a.q[k]);
    }
  }

  if (a.y_true) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    if (live && rr == 0) {
      const double y = (double)a.y_true[o] * sc, z = (y - mean) / sd;
      t0 = 0.5 * z * z + log(sd) + 0.91893853320467274178;
      double mass = fc_ndtr((y + 0.6 - mean) / sd) - fc_ndtr((y - 0.5 - mean) / sd);
      if (mass == 0.0) mass = FC_MASS_FLOOR;
      t1 = log(mass);
      t2 = fabs(y - mean);
    }
    __syncthreads();
    if (rr == 0) {
      red[c] = t0;
      red[G + c] = t1;
      red[2 * G + c] = t2;
    }
    __syncthreads();
    if (tid < 3) {
      double s = 0.0;
      for (int i = 0; i < G; ++i) s += red[tid * G + i];
      a.part[((size_t)t * gridDim.x + blockIdx.x) * 3 + tid] = s;
    }
    if constexpr (VERIFY) {
      if (live && rr == 0) {
        double* tg = v.terms + (size_t)t * FC_TERMS * BR + g;
        tg[0] = t0;
        tg[(size_t)BR] = t1;
        tg[(size_t)2 * BR] = t2;
      }
    }
  }

  if constexpr (VERIFY) {
    // the ensemble's own scores from the sorted tile (targets are given: checked by the host)
    const double y = live ? (double)a.y_true[o] * sc : 0.0;
    const double crps = fc_col_crps(red, tile, y, a.S, rr, c, G, RP);
    double iv = 0.0, bits = 0.0;                   // interval k of thread row k mod RP
    for (int k = rr; k < v.K; k += RP) {
      const double al = v.alpha[k];
      const double l = fc_quantile(tile, c, G, a.S, 0.5 * al), u = fc_quantile(tile, c, G, a.S, 1.0 - 0.5 * al);
      iv += 0.5 * al * ((u - l) + (2.0 / al) * fmax(l - y, 0.0) + (2.0 / al) * fmax(y - u, 0.0));
      if (l <= y && y <= u) bits += (double)(1 << k);
    }
    const double ivsum = fc_col_sum(red, iv, rr, c, G, RP);
    const double cover = fc_col_sum(red, bits, rr, c, G, RP);   // distinct bits: the sum is their union
    double t3 = 0.0, t4 = 0.0, t5 = 0.0, packed = (double)(FC_DEAD_BIN << 16);
    if (live && rr == 0) {
      t3 = crps;
      t4 = (0.5 * fabs(y - fc_quantile(tile, c, G, a.S, 0.5)) + ivsum) / ((double)v.K + 0.5);
      const int n_lt = fc_count_below<false>(tile, c, G, a.S, y), n_le = fc_count_below<true>(tile, c, G, a.S, y);
      int bin = (v.J * (n_lt + n_le)) / (2 * a.S);
      if (bin > v.J - 1) bin = v.J - 1;
      t5 = fc_window_log_mass(tile, c, G, a.S, y);
      packed = cover + (double)(bin << 16);
      double* tg = v.terms + ((size_t)t * FC_TERMS + 3) * BR + g;
      tg[0] = t3;
      tg[(size_t)BR] = t4;
      tg[(size_t)2 * BR] = t5;
      tg[(size_t)3 * BR] = cover;
    }
    __syncthreads();
    if (rr == 0) {
      red[c] = t3;
      red[G + c] = t4;
      red[2 * G + c] = t5;
      red[3 * G + c] = packed;
    }
    __syncthreads();
    const int NP = 3 + v.K + v.J;
    if (tid < NP) {
      double s = 0.0;
      if (tid < 3) {
        for (int i = 0; i < G; ++i) s += red[tid * G + i];
      } else {
        int n = 0;
        for (int i = 0; i < G; ++i) {
          const unsigned pk = (unsigned)red[3 * G + i];
          n += tid < 3 + v.K ? (pk >> (tid - 3)) & 1u : (pk >> 16) == (unsigned)(tid - 3 - v.K);
        }
        s = (double)n;
      }
      v.vpart[((size_t)t * gridDim.x + blockIdx.x) * NP + tid] = s;
    }
  }
}

__global__ __launch_bounds__(FC_THREADS) void ude_forecast_summary_kernel(FcArgs a) {
  fc_summary_body<false>(a, FcVerifyArgs{});
}

__global__ __launch_bounds__(FC_THREADS) void ude_forecast_verify_kernel(FcArgs a, FcVerifyArgs v) {
  fc_summary_body<true>(a, v);
}

// scores[k][t] = (fc_wave_sum over the workgroups of t) / (B R)
__global__ __launch_bounds__(64) void ude_forecast_scores_kernel(const double* __restrict__ part, int nbx, int T,
                                                                 double inv_n, double* __restrict__ scores) {
  const int t = blockIdx.x, ln = threadIdx.x;
  for (int k = 0; k < 3; ++k) {
    const double s = fc_wave_sum(part, (size_t)t * nbx, nbx, 3, k, ln);
    if (ln == 0) scores[(size_t)k * T + t] = s * inv_n;
  }
}

// The VERIFY outputs, one workgroup of FC_TERMS waves per (64 regions, t); wave f takes term f.
// vreg[f][t][r] = fc_group_mean of the group terms over b: f < 6 the six scores, 6 + k the coverage of
// interval k (an integer count, divided once).  The first workgroup of each t also forms vday[k][t] =
// (fc_wave_sum over the workgroup partials of t) / (B R), k < 3 + K + J, wave f those with k = f mod FC_TERMS.
__global__ __launch_bounds__(64 * FC_TERMS) void ude_forecast_verify_reduce_kernel(
    const double* __restrict__ vpart, const double* __restrict__ terms, int nbx, int T, int B, int R, int K, int J,
    double* __restrict__ vday, double* __restrict__ vreg) {
  const int t = blockIdx.y, ln = threadIdx.x, f = threadIdx.y;
  const size_t BR = (size_t)B * R;
  if (blockIdx.x == 0) {
    const int NP = 3 + K + J;
    for (int k = f; k < NP; k += FC_TERMS) {
      const double s = fc_wave_sum(vpart, (size_t)t * nbx, nbx, NP, k, ln);
      if (ln == 0) vday[(size_t)k * T + t] = s / (double)BR;
    }
  }
  const int r = blockIdx.x * 64 + ln;
  if (r >= R) return;
  const double* p = terms + ((size_t)t * FC_TERMS + f) * BR + r;
  if (f < 6) {
    vreg[((size_t)f * T + t) * R + r] = fc_group_mean(p, B, R);
  } else {
    int cnt[FC_MAX_ALPHA] = {};
#pragma unroll 8
    for (int b = 0; b < B; ++b) {
      const unsigned bits = (unsigned)p[(size_t)b * R];
#pragma unroll
      for (int k = 0; k < FC_MAX_ALPHA; ++k) cnt[k] += (bits >> k) & 1u;
    }
#pragma unroll
    for (int k = 0; k < FC_MAX_ALPHA; ++k)
      if (k < K) vreg[((size_t)(6 + k) * T + t) * R + r] = (double)cnt[k] / (double)B;
  }
}

inline bool fc_shape_ok(int T, int S, int B, int R, int n_q) {
  if (T < 1 || T > 65535 || S < 1 || B < 1 || R < 1 || n_q < 0) return false;
  if ((int64_t)B * R > (int64_t)1 << 30 || (int64_t)S * B * R > (int64_t)1 << 40) return false;
  return n_q == 0 || S <= FC_MAX_SQ;
}

inline int forecast_summary_workspace(int T, int S, int B, int R, int n_q, int64_t* ws_bytes) {
  if (!ws_bytes || !fc_shape_ok(T, S, B, R, n_q)) return -2;
  *ws_bytes = (int64_t)T * fc_geom(S, B * R, n_q).nbx * 3 * 8;
  return 0;
}

// What forecast_summary and forecast_verify (sorted: it always sorts its tile) share: the checks of the
// shape and of the pointers both take, the kernel's arguments, its geometry and its dynamic LDS bytes.
inline bool fc_launch_args(int T, int S, int B, int R, const float* yhat, const double* scale, const float* y_true,
                           const double* q, int n_q, void* ws, double* mean, double* std, double* quant, bool sorted,
                           FcArgs* a, FcGeom* ge, size_t* lds) {
  if (!fc_shape_ok(T, S, B, R, n_q) || !yhat || !mean || !std) return false;
  if (n_q > 0 && (!q || !quant)) return false;
  *a = FcArgs{yhat, scale, y_true, q, mean, std, quant, (double*)ws, T, S, B, R, n_q};
  *ge = fc_geom(S, B * R, sorted ? 1 : n_q);
  *lds = ((size_t)FC_THREADS + (size_t)ge->rows * ge->G) * 8;
  return true;
}

inline int forecast_summary(int T, int S, int B, int R, const float* yhat, const double* scale, const float* y_true,
                            const double* q, int n_q, void* ws, double* mean, double* std, double* quant,
                            double* scores, hipStream_t s) {
  FcArgs a;
  FcGeom ge;
  size_t lds;
  if (!fc_launch_args(T, S, B, R, yhat, scale, y_true, q, n_q, ws, mean, std, quant, false, &a, &ge, &lds)) return -2;
  if (y_true && (!ws || !scores)) return -2;
  hipLaunchKernelGGL(ude_forecast_summary_kernel, dim3(ge.nbx, T), dim3(FC_THREADS), lds, s, a);
  if (hipGetLastError() != hipSuccess) return -3;
  if (y_true) {
    hipLaunchKernelGGL(ude_forecast_scores_kernel, dim3(T), dim3(64), 0, s, (const double*)ws, ge.nbx, T,
                       1.0 / ((double)B * (double)R), scores);
    if (hipGetLastError() != hipSuccess) return -3;
  }
  return 0;
}

inline bool fc_verify_ok(int T, int S, int B, int R, int n_q, int K, int J) {
  return fc_shape_ok(T, S, B, R, n_q) && S <= FC_MAX_SQ && K >= 1 && K <= FC_MAX_ALPHA && J >= 1 && J <= FC_MAX_PIT;
}

// workspace: part [T][nbx][3] | vpart [T][nbx][3 + K + J] | terms [T][FC_TERMS][B R], doubles
inline int forecast_verify_workspace(int T, int S, int B, int R, int n_q, int K, int J, int64_t* ws_bytes) {
  if (!ws_bytes || !fc_verify_ok(T, S, B, R, n_q, K, J)) return -2;
  const int64_t nbx = fc_geom(S, B * R, 1).nbx;
  *ws_bytes = ((int64_t)T * nbx * (6 + K + J) + (int64_t)T * FC_TERMS * B * R) * 8;
  return 0;
}

inline int forecast_verify(int T, int S, int B, int R, const float* yhat, const double* scale, const float* y_true,
                           const double* q, int n_q, const double* alpha, int K, int J, void* ws, double* mean,
                           double* std, double* quant, double* scores, double* vday, double* vreg, hipStream_t s) {
  FcArgs a;
  FcGeom ge;
  size_t lds;
  if (!fc_verify_ok(T, S, B, R, n_q, K, J)) return -2;
  if (!fc_launch_args(T, S, B, R, yhat, scale, y_true, q, n_q, ws, mean, std, quant, true, &a, &ge, &lds)) return -2;
  if (!y_true || !alpha || !ws || !scores || !vday || !vreg) return -2;
  FcVerifyArgs v;
  v.alpha = alpha; v.K = K; v.J = J;
  v.vpart = a.part + (size_t)T * ge.nbx * 3;
  v.terms = v.vpart + (size_t)T * ge.nbx * (3 + K + J);
  hipLaunchKernelGGL(ude_forecast_verify_kernel, dim3(ge.nbx, T), dim3(FC_THREADS), lds, s, a, v);
  if (hipGetLastError() != hipSuccess) return -3;
  hipLaunchKernelGGL(ude_forecast_scores_kernel, dim3(T), dim3(64), 0, s, (const double*)ws, ge.nbx, T,
                     1.0 / ((double)B * (double)R), scores);
  if (hipGetLastError() != hipSuccess) return -3;
  hipLaunchKernelGGL(ude_forecast_verify_reduce_kernel, dim3((R + 63) / 64, T), dim3(64, FC_TERMS), 0, s,
                     (const double*)v.vpart, (const double*)v.terms, ge.nbx, T, B, R, K, J, vday, vreg);
  if (hipGetLastError() != hipSuccess) return -3;
  return 0;
}

}  // namespace ude
