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
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace ude {

constexpr int FC_THREADS = 256;
constexpr int FC_TILE_ELEMS = 4096;      // [S][G] doubles: 32 KiB, four workgroups per CU by LDS
constexpr int FC_MAX_G = 64;
constexpr int FC_MAX_SQ = 1024;          // largest S with quantiles (the sorted tile)

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

__global__ __launch_bounds__(FC_THREADS) void ude_forecast_summary_kernel(FcArgs a) {
  extern __shared__ __attribute__((aligned(16))) double fc_lds[];
  const int BR = a.B * a.R;
  const FcGeom ge = fc_geom(a.S, BR, a.n_q);
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
  double acc = 0.0;
  for (int s = rr; s < a.S; s += RP) acc += val(s);
  const double mean = fc_col_sum(red, acc, rr, c, G, RP) / (double)a.S;
  acc = 0.0;
  for (int s = rr; s < a.S; s += RP) {
    const double d = val(s) - mean;
    acc += d * d;
  }
  const double sd = sqrt(fc_col_sum(red, acc, rr, c, G, RP) / (double)a.S);
  const size_t o = ((size_t)b * a.T + t) * a.R + r;
  if (live && rr == 0) {
    a.mean[o] = mean;
    a.std[o] = sd;
  }

  if (a.n_q > 0) {
    // bitonic network along S: rows / 2 compare-exchanges per column and stage over all threads
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
    if (live) {
      for (int k = rr; k < a.n_q; k += RP) {
        // numpy.quantile, method 'linear' (numpy/lib/function_base.py _lerp)
        const double h = (double)(a.S - 1) * a.q[k];
        int lo = (int)floor(h);
        if (lo < 0) lo = 0;
        if (lo > a.S - 1) lo = a.S - 1;
        const int hi = lo + 1 < a.S ? lo + 1 : a.S - 1;
        const double gm = h - (double)lo, x = tile[lo * G + c], y = tile[hi * G + c], d = y - x;
        a.quant[(((size_t)k * a.B + b) * a.T + t) * a.R + r] = gm >= 0.5 ? y - d * (1.0 - gm) : x + d * gm;
      }
    }
  }

  if (a.y_true) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    if (live && rr == 0) {
      const double y = (double)a.y_true[o] * sc, z = (y - mean) / sd;
      t0 = 0.5 * z * z + log(sd) + 0.91893853320467274178;
      double mass = fc_ndtr((y + 0.6 - mean) / sd) - fc_ndtr((y - 0.5 - mean) / sd);
      if (mass == 0.0) mass = 4.5399929762484854e-05;
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
  }
}

// scores[k][t] = (sum over the workgroups of t, lane-strided then a fixed butterfly) / (B R)
__global__ __launch_bounds__(64) void ude_forecast_scores_kernel(const double* __restrict__ part, int nbx, int T,
                                                                 double inv_n, double* __restrict__ scores) {
  const int t = blockIdx.x, ln = threadIdx.x;
  for (int k = 0; k < 3; ++k) {
    double s = 0.0;
    for (int i = ln; i < nbx; i += 64) s += part[((size_t)t * nbx + i) * 3 + k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (ln == 0) scores[(size_t)k * T + t] = s * inv_n;
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

inline int forecast_summary(int T, int S, int B, int R, const float* yhat, const double* scale, const float* y_true,
                            const double* q, int n_q, void* ws, double* mean, double* std, double* quant,
                            double* scores, hipStream_t s) {
  if (!fc_shape_ok(T, S, B, R, n_q) || !yhat || !mean || !std) return -2;
  if (n_q > 0 && (!q || !quant)) return -2;
  if (y_true && (!ws || !scores)) return -2;
  const FcGeom ge = fc_geom(S, B * R, n_q);
  FcArgs a;
  a.yhat = yhat; a.scale = scale; a.y_true = y_true; a.q = q;
  a.mean = mean; a.std = std; a.quant = quant; a.part = (double*)ws;
  a.T = T; a.S = S; a.B = B; a.R = R; a.n_q = n_q;
  const size_t lds = ((size_t)FC_THREADS + (size_t)ge.rows * ge.G) * 8;
  hipLaunchKernelGGL(ude_forecast_summary_kernel, dim3(ge.nbx, T), dim3(FC_THREADS), lds, s, a);
  if (hipGetLastError() != hipSuccess) return -3;
  if (y_true) {
    hipLaunchKernelGGL(ude_forecast_scores_kernel, dim3(T), dim3(64), 0, s, (const double*)ws, ge.nbx, T,
                       1.0 / ((double)B * (double)R), scores);
    if (hipGetLastError() != hipSuccess) return -3;
  }
  return 0;
}

}  // namespace ude
