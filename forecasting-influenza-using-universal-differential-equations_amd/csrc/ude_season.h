// Seasonal targets of an ensemble forecast (no model): what depends on how a trajectory's output times hang
// together -- per sample the peak over the considered times t_m = start + m every, the first m that attains
// it, the total, and with a baseline the onset (the first m that starts `run` consecutive values at or
// above it) -- summarised per (window, region) group over the S samples of y_hat (T, S*B, R), and scored
// against the observed season when targets are given.  The formulas are at ude_forecast_season in
// include/ude_rk4.h.
//
// One read of y_hat.  A workgroup takes G neighbouring columns of the contiguous B*R axis with all S samples
// and all M considered times.  Pass 1, thread (c, rr): for each of its samples s = rr, rr + RP, .. the M
// values of column c (for a fixed (t, s) the G values are contiguous, so the rows coalesce as in the summary
// kernel; FS_BATCH loads of a sample are in flight at once), with peak / when / total / run counter / onset
// in registers; the results go to LDS: V[s][c] = peak, V[s][G + c] = total, and the two index tiles.  Pass 2
// treats V as one [rows][2 G] tile of the summary's helpers, thread (c2, rr2): columns c2 < G are the peaks,
// the others the totals, so one pass gives mean / std (two passes over the unsorted tile), one bitonic
// network sorts both, and quantiles and CRPS come from the same code for both.  The histograms are counts
// of the index tiles (integers, divided once); the window counts of the log scores are integers summed by
// fc_col_sum (exact in fp64).  Per-workgroup partials and per-group terms, summed in a fixed order by a
// second kernel: no atomics, the same bits run to run.
//
// LDS: V (2 rows G doubles) + the index tiles (2 rows G ints) + the reduction row and a few per-column
// arrays.  With the summary's G (rows G <= 4096) that is about 100 KiB: one workgroup per CU and a
// dynamic-LDS attribute.  The kernel is bound by the latency of pass 1's loads, so what pays is workgroups
// in flight, not width: measured on the MI355X at the forecast's shape (T 57, S 128, B R 3136; weekly M = 8 /
// daily M = 57, min of 30 alternating runs, ms) rows G <= 4096 (98 workgroups, with the attribute) 0.131 /
// 0.457, <= 2048 (196) 0.081 / 0.261, <= 1024 (392) 0.056 / 0.160, <= 512 (784) 0.055 / 0.164, <= 256 (1568)
// 0.072 / 0.192; sixteen loads in flight instead of eight changed none of them by more than 4 %.  So
// rows G <= 1024, a quarter of the summary's tile: at most 30 KiB of LDS, no attribute.
#pragma once
#include "ude_forecast.h"

namespace ude {

constexpr int FS_BATCH = 8;              // loads of one sample in flight
constexpr int FS_TERMS = 5;              // log P(peak time), log P(onset), log P(peak value), crps peak, crps total

constexpr int UDE_FS_CELLS = FC_TILE_ELEMS / 4;   // rows G of a workgroup (the measurement above)

__host__ __device__ inline FcGeom fs_geom(int S, int BR) {
  FcGeom g = fc_geom(S, BR, 1);
  while (g.G > 1 && g.G * g.rows > UDE_FS_CELLS) g.G >>= 1;
  g.nbx = (BR + g.G - 1) / g.G;
  return g;
}

struct FsArgs {
  const float* yhat;
  const double* scale;
  const double* base;  // [R] scaled units, or null: no onset
  const float* y_true;
  const double* q;
  double* stats;       // [4][B R]: peak mean, peak std, total mean, total std
  double* quant;       // [2][n_q][B R]: peak, total
  double* peak_time;   // [B][M][R]
  double* onset;       // [B][M + 1][R]
  double* part;        // [nbx][FS_TERMS]
  double* terms;       // [FS_TERMS][B R]
  int T, S, B, R, n_q, start, every, run, window, M;
};

// the state of one trajectory's walk over m = 0 .. M-1 (samples and the observed season alike)
struct FsWalk {
  double peak, total;
  int when, cnt, onset;
  __device__ __forceinline__ void init(int M) { peak = 0.0; total = 0.0; when = 0; cnt = 0; onset = M; }
  __device__ __forceinline__ void step(int m, double v, bool has_base, double base, int run, int M) {
    if (m == 0 || v > peak) { peak = v; when = m; }        // strict: the first index of the peak
    total += v;
    if (has_base) {
      cnt = v >= base ? cnt + 1 : 0;
      if (cnt >= run && onset == M) onset = m - run + 1;
    }
  }
};

__global__ __launch_bounds__(FC_THREADS) void ude_forecast_season_kernel(FsArgs a) {
  extern __shared__ __attribute__((aligned(16))) double fc_lds[];
  __shared__ double obs_peak[FC_MAX_G], obs_total[FC_MAX_G];
  __shared__ int obs_when[FC_MAX_G], obs_onset[FC_MAX_G];
  __shared__ double grp[FS_TERMS][FC_MAX_G];     // the group terms of this workgroup's columns
  const int BR = a.B * a.R, M = a.M;
  const FcGeom ge = fs_geom(a.S, BR);
  const int G = ge.G, rows = ge.rows, G2 = 2 * G;
  double* red = fc_lds;                          // [256 / G2][G2] = 256 doubles
  double* V = fc_lds + FC_THREADS;               // [rows][G2]
  int* wh = (int*)(V + (size_t)rows * G2);       // [rows][G]
  int* on = wh + (size_t)rows * G;               // [rows][G]
  const int tid = threadIdx.x;
  const bool has_base = a.base != nullptr;
  const size_t tstride = (size_t)a.every * a.S * BR;

  {  // pass 1
    const int c = tid & (G - 1), rr = tid / G, RP = FC_THREADS / G;
    const int g = blockIdx.x * G + c;
    const bool live = g < BR;
    const int r = live ? g % a.R : 0;
    const double sc = (live && a.scale) ? a.scale[r] : 1.0;
    const double base = has_base ? a.base[r] : 0.0;
    const float* src = a.yhat + (size_t)a.start * a.S * BR + g;
    for (int s = rr; s < rows; s += RP) {
      if (s >= a.S) {                             // padding rows sort to the end
        V[s * G2 + c] = (double)INFINITY;
        V[s * G2 + G + c] = (double)INFINITY;
        continue;
      }
      FsWalk w;
      w.init(M);
      if (live) {
        const float* ps = src + (size_t)s * BR;
        for (int m0 = 0; m0 < M; m0 += FS_BATCH) {
          float x[FS_BATCH];
#pragma unroll
          for (int j = 0; j < FS_BATCH; ++j) x[j] = m0 + j < M ? ps[(size_t)(m0 + j) * tstride] : 0.0f;
#pragma unroll
          for (int j = 0; j < FS_BATCH; ++j)
            if (m0 + j < M) w.step(m0 + j, (double)x[j] * sc, has_base, base, a.run, M);
        }
      }
      V[s * G2 + c] = w.peak;
      V[s * G2 + G + c] = w.total;
      wh[s * G + c] = w.when;
      on[s * G + c] = w.onset;
    }
    if (a.y_true && rr == 0) {                    // the observed season of group c, by the same rules
      FsWalk w;
      w.init(M);
      if (live) {
        const int b = g / a.R;
        const float* py = a.y_true + ((size_t)b * a.T + a.start) * a.R + r;
        for (int m = 0; m < M; ++m)
          w.step(m, (double)py[(size_t)m * a.every * a.R] * sc, has_base, base, a.run, M);
      }
      obs_peak[c] = w.peak;
      obs_total[c] = w.total;
      obs_when[c] = w.when;
      obs_onset[c] = w.onset;
    }
  }
  __syncthreads();

  // pass 2: V as [rows][G2]; column c2 is the peaks (which = 0) or the totals (which = 1) of group c
  const int c2 = tid & (G2 - 1), rr = tid / G2, RP = FC_THREADS / G2;
  const int which = c2 / G, c = c2 & (G - 1);
  const int g = blockIdx.x * G + c;
  const bool live = g < BR;
  const int b = live ? g / a.R : 0, r = live ? g - b * a.R : 0;
  const double dS = (double)a.S;

  const FcMoments mo = fc_col_moments(red, [&](int s) { return V[s * G2 + c2]; }, a.S, rr, c2, G2, RP);
  if (live && rr == 0) {
    a.stats[(size_t)(2 * which) * BR + g] = mo.mean;
    a.stats[(size_t)(2 * which + 1) * BR + g] = mo.sd;
  }

  fc_bitonic_sort(V, rows, rr, c2, G2, RP);
  if (live) {
    for (int k = rr; k < a.n_q; k += RP)
      a.quant[((size_t)which * a.n_q + k) * BR + g] = fc_quantile(V, c2, G2, a.S, a.q[k]);
  }

  // histograms: which = 0 the peak times (M bins), which = 1 the onsets (M + 1 bins, the last "none")
  {
    const int* idx = which ? on : wh;
    const int bins = which ? (has_base ? M + 1 : 0) : M;
    double* out = which ? a.onset : a.peak_time;
    if (live) {
      for (int m = rr; m < bins; m += RP) {
        int n = 0;
        for (int s = 0; s < a.S; ++s) n += idx[s * G + c] == m;
        out[((size_t)b * bins + m) * a.R + r] = (double)n / dS;
      }
    }
  }

  if (!a.y_true) return;                          // uniform: a kernel argument

  // the window counts of the two time scores and the sorted-sample CRPS sums of the two value columns
  const int ostar = which ? obs_onset[c] : obs_when[c];
  const double y = which ? obs_total[c] : obs_peak[c];
  double cnt = 0.0;
  {
    const int* idx = which ? on : wh;
    const bool none = which && ostar == M;        // observed: no onset within the horizon
    for (int s = rr; s < a.S; s += RP) {
      const int i = idx[s * G + c];
      const int d = i > ostar ? i - ostar : ostar - i;
      cnt += none ? (double)(i == M) : (double)(i < M && d <= a.window);
    }
  }
  const double nwin = fc_col_sum(red, cnt, rr, c2, G2, RP);
  const double col_crps = fc_col_crps(red, V, y, a.S, rr, c2, G2, RP);
  if (rr == 0) {
    double lt = 0.0, lv = 0.0, crps = 0.0;        // dead columns add zero to the partials
    if (live) {
      lt = (which && !has_base) ? 0.0 : log(nwin == 0.0 ? FC_MASS_FLOOR : nwin / dS);
      crps = col_crps;
      if (!which) lv = fc_window_log_mass(V, c2, G2, a.S, y);
      a.terms[(size_t)which * BR + g] = lt;                       // 0: peak time, 1: onset
      a.terms[(size_t)(3 + which) * BR + g] = crps;               // 3: peak, 4: total
      if (!which) a.terms[(size_t)2 * BR + g] = lv;
    }
    grp[which][c] = lt;
    grp[3 + which][c] = crps;
    if (!which) grp[2][c] = lv;
  }
  __syncthreads();
  if (tid < FS_TERMS) {
    double s = 0.0;
    for (int i = 0; i < G; ++i) s += grp[tid][i];
    a.part[(size_t)blockIdx.x * FS_TERMS + tid] = s;
  }
}

// One workgroup of FS_TERMS waves per 64 regions; wave f takes term f.  region[f][r] = fc_group_mean of
// the group terms over b.  The first workgroup also forms overall[f] = (fc_wave_sum over the workgroup
// partials) / (B R).
__global__ __launch_bounds__(64 * FS_TERMS) void ude_forecast_season_reduce_kernel(
    const double* __restrict__ part, const double* __restrict__ terms, int nbx, int B, int R,
    double* __restrict__ overall, double* __restrict__ region) {
  const int ln = threadIdx.x, f = threadIdx.y;
  const size_t BR = (size_t)B * R;
  if (blockIdx.x == 0) {
    const double s = fc_wave_sum(part, 0, nbx, FS_TERMS, f, ln);
    if (ln == 0) overall[f] = s / (double)BR;
  }
  const int r = blockIdx.x * 64 + ln;
  if (r >= R) return;
  region[(size_t)f * R + r] = fc_group_mean(terms + (size_t)f * BR + r, B, R);
}

// M, the number of considered times, or 0 when the arguments are out of range
inline int fs_times(int T, int S, int B, int R, int n_q, int start, int every, int run, int window) {
  if (!fc_shape_ok(T, S, B, R, n_q) || S > FC_MAX_SQ) return 0;
  if (start < 0 || start >= T || every < 1 || run < 1 || window < 0) return 0;
  return (int)(((int64_t)T - start + every - 1) / every);
}

// workspace: part [nbx][FS_TERMS] | terms [FS_TERMS][B R], doubles
inline int forecast_season_workspace(int T, int S, int B, int R, int n_q, int start, int every, int run, int window,
                                     int64_t* ws_bytes) {
  if (!ws_bytes || !fs_times(T, S, B, R, n_q, start, every, run, window)) return -2;
  *ws_bytes = ((int64_t)fs_geom(S, B * R).nbx + (int64_t)B * R) * FS_TERMS * 8;
  return 0;
}

inline int forecast_season(int T, int S, int B, int R, int start, int every, int run, int window, const float* yhat,
                           const double* scale, const double* base, const float* y_true, const double* q, int n_q,
                           void* ws, double* stats, double* quant, double* peak_time, double* onset, double* overall,
                           double* region, hipStream_t s) {
  const int M = fs_times(T, S, B, R, n_q, start, every, run, window);
  if (!M || !yhat || !stats || !peak_time) return -2;
  if (n_q > 0 && (!q || !quant)) return -2;
  if (base && !onset) return -2;
  if (y_true && (!ws || !overall || !region)) return -2;
  const FcGeom ge = fs_geom(S, B * R);
  FsArgs a;
  a.yhat = yhat; a.scale = scale; a.base = base; a.y_true = y_true; a.q = q;
  a.stats = stats; a.quant = quant; a.peak_time = peak_time; a.onset = onset;
  a.part = (double*)ws;
  a.terms = a.part ? a.part + (size_t)ge.nbx * FS_TERMS : nullptr;
  a.T = T; a.S = S; a.B = B; a.R = R; a.n_q = n_q;
  a.start = start; a.every = every; a.run = run; a.window = window; a.M = M;
  const size_t cells = (size_t)ge.rows * ge.G;
  const size_t lds = ((size_t)FC_THREADS + 2 * cells) * 8 + 2 * cells * 4;
  hipLaunchKernelGGL(ude_forecast_season_kernel, dim3(ge.nbx), dim3(FC_THREADS), lds, s, a);
  if (hipGetLastError() != hipSuccess) return -3;
  if (y_true) {
    hipLaunchKernelGGL(ude_forecast_season_reduce_kernel, dim3((R + 63) / 64), dim3(64, FS_TERMS), 0, s,
                       (const double*)a.part, (const double*)a.terms, ge.nbx, B, R, overall, region);
    if (hipGetLastError() != hipSuccess) return -3;
  }
  return 0;
}

}  // namespace ude
