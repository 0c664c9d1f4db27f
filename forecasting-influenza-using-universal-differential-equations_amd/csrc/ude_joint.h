// Joint scores of an ensemble forecast (no model): the energy score and the variogram score of the S
// trajectories of y_hat (T, S*B, R) against the observed one -- what depends on how the ensemble's days and
// regions move together.  Over the considered times t_m = start + m every a window b is scored on three
// coordinate blocks: series (b, r): region r's M times; field (b, m): the R regions at time m; joint (b): all
// M R coordinates (energy only).  The formulas are at ude_forecast_joint in include/ude_rk4.h.
//
// Energy, ude_forecast_joint_energy_kernel.  A workgroup owns (b, i-tile, j-tile) with j-tile >= i-tile of the
// S x S sample pairs, 16 x 16; thread tid owns the pair (i, j) = (16 ti + tid / 16, 16 tj + tid % 16).  One
// sweep with m outer and r inner reads y_hat once: for every m the rows of the 16 + 16 samples and of the
// target (for a fixed (t, s, b) the R values are contiguous: coalesced) go to LDS as scaled doubles, and the
// thread forms d = x_i - x_j coordinate by coordinate (fp64, direct differences: never |x_i|^2 + |x_j|^2 -
// 2 x_i . x_j, which cancels what the scores are made of).  d d is added, r ascending, to the field sum of this m
// and to the series sum of region r, which the thread keeps in registers for JS_RC regions (128 VGPRs); at the
// end of an m the field distance is the root of the field sum, and the field sum goes to the joint sum before
// the root; after the last m the series distances are the roots of the series sums and the joint distance
// that of the joint sum.  With R > JS_RC the same sweep runs once more per further chunk of JS_RC regions,
// reading only that chunk, for its series sums.  The first term |x_i - y| is the same code: on a diagonal tile
// the thread of the pair (i, i), whose distance is zero, takes the target's row as its partner instead, and its
// distances go to the first-term sums.  Every distance is summed over the workgroup's pairs by a fixed
// butterfly in each wave and w0 + w1 + w2 + w3 over the four waves (rows past S count zero), and written as
// one partial per (workgroup, block); the reduce kernel sums the partials of a window over its tile pairs
// ((ti, tj), tj >= ti, row by row: lane l takes the pairs l, l + 64, .. in order, then the same butterfly),
// the off-diagonal tiles twice, and forms ES = first / S - pairs / (2 S^2).
// The tile of the next step (thread tid: column tid % 64 of the rows tid / 64 + 4 j; a wave reads 64
// neighbouring regions of one row) is loaded into registers while this step's is summed, and stored to the
// other of two LDS buffers behind it: one barrier per step.
//
// Variogram, ude_forecast_joint_variogram_kernel.  One workgroup per block: B R series blocks (C = M
// coordinates) then B M field blocks (C = R).  The block's S x C values sit in LDS as scaled doubles, JV_TILE
// at a time (all C coordinates of as many samples as fit, s ascending).  Thread tid owns the coordinate pairs
// p = 256 k + tid (k < JV_NPT, then the next 256 JV_NPT pairs), p counting (c, c') with c < c' row by row of
// c'; per pair a sequential sum over s = 0 .. S-1 of |x_sc - x_sc'|^p (p = 0.5: one sqrt; p = 1: fabs; no
// pow), then (|y_c - y_c'|^p - sum / S)^2, added over the thread's pairs in order and over the 256 threads by a
// fixed tree.  A block of one coordinate has no pair: exactly 0.
//
// The means over the B windows are fc_group_mean (p[0] + p[1] + .., divided once) in a last launch.  No
// atomics; nothing in the geometry depends on values: the same bits run to run.
//
// LDS: energy two tiles of 33 rows of JS_LD doubles (34 KiB) and 4 KiB of sums, static (the row stride is odd
// so that the 16 partner rows of a half-wave fall on different banks); variogram JV_TILE + 256 doubles (62 KiB,
// dynamic: under 64 KiB, no attribute).  The energy kernel takes 221 VGPRs and no scratch: two workgroups per
// CU.
//
// Measured on the MI355X at the forecast's shape (T 57, S 128, B 64, R 49: 36 tile pairs x 64 windows = 2304
// energy workgroups, 6784 variogram workgroups daily), kernel times from a kernel trace, min of 6 calls, us,
// weekly (6, 7) M = 8 / daily (0, 1) M = 57:
//   energy, as it is                                                        279 / 1049
//   energy, the tile loaded, a barrier, summed, a barrier (no prefetch)     308 / 1327
//   energy, the loads issued two steps ahead (two register sets)            285 / 1107
//   energy, the row index made wave-uniform so that addresses are scalar    306 / 1279
//   energy, fma(d, d, sum) in place of d d then +                           275 / 1055  (no gain: kept plain)
//   variogram (p = 0.5), as it is                                           204 / 1262
//   variogram, series blocks renumbered so that one XCD takes the regions
//   of one window (a block reads one float of each 128-byte line)           208 / 1263  (no gain: left out)
//   reduce 5 / 6, means 10 / 8
// The 16 x 16 tile with one pair per thread is what lets a thread hold the 64 series sums (a 2 x 2 block of
// pairs would need 256 of them); wider tiles were not built.  The whole call and the torch routes: DESIGN.md.
#pragma once
#include "ude_forecast.h"

namespace ude {

constexpr int JS_TILE = 16;              // samples per side of a pair tile
constexpr int JS_RC = 64;                // regions a thread keeps series sums for, per sweep
constexpr int JS_LD = JS_RC + 1;         // LDS row stride (doubles)
constexpr int JS_ROWS = 2 * JS_TILE + 1; // i rows, j rows, the target
constexpr int JS_PF = (JS_ROWS + 3) / 4; // rows a thread carries from global memory to LDS per step
constexpr int JS_MAX_C = 4096;           // largest M and R (a variogram block's coordinates fit the tile)
constexpr int JV_TILE = 7680;            // doubles of a variogram tile (the forecast's 128 x 57 block in one piece)
constexpr int JV_NPT = 8;                // coordinate pairs of a thread per pass over the samples

struct JsArgs {
  const float* yhat;
  const double* scale;
  const float* y_true;
  double* part;        // [B][ntp][2][1 + R + M]: pair sums then first-term sums of joint, series r, field m
  double* e_joint;     // [B]
  double* e_series;    // [B][R]
  double* e_field;     // [B][M]
  double* v_series;    // [B][R]
  double* v_field;     // [B][M]
  int T, S, B, R, start, every, M, nt;
};

__host__ __device__ inline int js_tiles(int S) { return (S + JS_TILE - 1) / JS_TILE; }
__host__ __device__ inline int js_tile_pairs(int S) { const int nt = js_tiles(S); return nt * (nt + 1) / 2; }

// fixed butterfly over the 64 lanes of a wave: every lane has the sum
__device__ __forceinline__ double js_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(256) void ude_forecast_joint_energy_kernel(JsArgs a) {
  __shared__ double rows[2][JS_ROWS * JS_LD];    // the tile of a step, double-buffered
  __shared__ double wred[2][2][4];               // field, by the parity of m: [pairs | first][wave]
  __shared__ double sred[2][JS_RC][4];           // series and joint
  const int tid = threadIdx.x, li = tid >> 4, lj = tid & 15, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.y, R = a.R, M = a.M, S = a.S;
  // tile pair blockIdx.x -> (ti, tj), tj >= ti, row by row
  int ti = 0, rest = blockIdx.x;
  while (rest >= a.nt - ti) { rest -= a.nt - ti; ++ti; }
  const int tj = ti + rest;
  const bool diag = ti == tj;
  const int si = ti * JS_TILE + li, sj = tj * JS_TILE + lj;
  const bool first = diag && li == lj;           // this thread's partner is the target
  const double w_pair = (!first && si < S && sj < S) ? 1.0 : 0.0;
  const double w_first = (first && si < S) ? 1.0 : 0.0;
  const int oi = li * JS_LD, oj = (first ? 2 * JS_TILE : JS_TILE + lj) * JS_LD;
  const size_t BR = (size_t)a.B * R, K = (size_t)1 + R + M;
  double* part = a.part + ((size_t)b * gridDim.x + blockIdx.x) * 2 * K;

  // The tile of a step (m, chunk c): thread tid carries column k = tid % 64 of the rows tid / 64 + 4 j from
  // global memory to LDS, the next step's while this step's is summed (a wave reads 64 neighbouring regions
  // of one row; one scale per thread and step).
  const int lk = tid & 63;
  float pre[JS_PF];
  double psc;
  auto fetch = [&](int m, int c) {
    const int t = a.start + m * a.every, r = c * JS_RC + lk;
    const bool live = r < R;
    psc = (live && a.scale) ? a.scale[r] : 1.0;
#pragma unroll
    for (int j = 0; j < JS_PF; ++j) {
      const int row = wave + 4 * j;
      float v = 0.0f;                            // columns past R and rows past S: d = 0
      if (live && row < 2 * JS_TILE) {
        const int s = row < JS_TILE ? ti * JS_TILE + row : tj * JS_TILE + row - JS_TILE;
        if (s < S) v = a.yhat[((size_t)t * S + s) * BR + (size_t)b * R + r];
      } else if (live && row == 2 * JS_TILE) {
        v = a.y_true[((size_t)b * a.T + t) * R + r];
      }
      pre[j] = v;
    }
  };
  auto store = [&](double* buf) {
#pragma unroll
    for (int j = 0; j < JS_PF; ++j) {
      const int row = wave + 4 * j;
      if (row < JS_ROWS) buf[row * JS_LD + lk] = (double)pre[j] * psc;
    }
  };

  const int n_chunks = (R + JS_RC - 1) / JS_RC;
  for (int q = 0; q < n_chunks; ++q) {           // sweep q: the series sums of chunk q; sweep 0 also field and joint
    double sacc[JS_RC];
#pragma unroll
    for (int k = 0; k < JS_RC; ++k) sacc[k] = 0.0;
    double jacc = 0.0, facc = 0.0;
    // the steps of a sweep: sweep 0 takes every chunk of every m (c inner), sweep q > 0 chunk q of every m
    const int per_m = q == 0 ? n_chunks : 1, n_steps = M * per_m;
    __syncthreads();                             // the previous sweep's tiles and sums have been read
    fetch(0, q);
    store(rows[0]);
    __syncthreads();
    for (int u = 0; u < n_steps; ++u) {
      const int m = u / per_m, c = q == 0 ? u - m * per_m : q;
      const bool more = u + 1 < n_steps;
      if (more) fetch((u + 1) / per_m, q == 0 ? (u + 1) % per_m : q);
      const int rcp = (min(JS_RC, R - c * JS_RC) + 7) & ~7;
      const double* xi = rows[u & 1] + oi;
      const double* xj = rows[u & 1] + oj;
      const bool ser = c == q;
#pragma unroll
      for (int k0 = 0; k0 < JS_RC; k0 += 8) {
        if (k0 < rcp) {
#pragma unroll
          for (int k = k0; k < k0 + 8; ++k) {
            const double d = xi[k] - xj[k];
            const double d2 = d * d;
            if (q == 0) facc += d2;
            if (ser) sacc[k] += d2;
          }
        }
      }
      const bool m_done = q == 0 && c == n_chunks - 1;
      if (m_done) {
        jacc += facc;
        const double dist = sqrt(facc);
        facc = 0.0;
        const double wp = js_wave_sum(w_pair * dist);
        const double wf = diag ? js_wave_sum(w_first * dist) : 0.0;
        if (lane == 0) {
          wred[m & 1][0][wave] = wp;
          wred[m & 1][1][wave] = wf;
        }
      }
      if (more) store(rows[(u + 1) & 1]);        // last read in step u - 1, behind that step's barrier
      __syncthreads();
      // wred[m & 1] is next written in step m + 2, behind the barrier of step m + 1
      if (m_done && tid < 2) {
        const double* w = wred[m & 1][tid];
        part[(size_t)tid * K + 1 + R + m] = ((w[0] + w[1]) + w[2]) + w[3];
      }
    }
    // the series distances of chunk q, and with q = 0 the joint distance
    const int r0 = q * JS_RC, rc = min(JS_RC, R - r0);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < JS_RC; ++k) {
      if (k < rc) {
        const double dist = sqrt(sacc[k]);
        const double wp = js_wave_sum(w_pair * dist);
        const double wf = diag ? js_wave_sum(w_first * dist) : 0.0;
        if (lane == 0) {
          sred[0][k][wave] = wp;
          sred[1][k][wave] = wf;
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < 2 * rc; e += 256) {
      const int w = e / rc, k = e - w * rc;
      part[(size_t)w * K + 1 + r0 + k] = ((sred[w][k][0] + sred[w][k][1]) + sred[w][k][2]) + sred[w][k][3];
    }
    if (q == 0) {
      const double dist = sqrt(jacc);
      const double wp = js_wave_sum(w_pair * dist);
      const double wf = diag ? js_wave_sum(w_first * dist) : 0.0;
      __syncthreads();                           // sred has been read
      if (lane == 0) {
        sred[0][0][wave] = wp;
        sred[1][0][wave] = wf;
      }
      __syncthreads();
      if (tid < 2) part[(size_t)tid * K] = ((sred[tid][0][0] + sred[tid][0][1]) + sred[tid][0][2]) + sred[tid][0][3];
    }
  }
}

// One wave per (b, block k): ES = first / S - pairs / (2 S^2), the partials of the window's tile pairs summed
// by fc_wave_sum in tile order; an off-diagonal tile stands for (i, j) and (j, i).
__global__ __launch_bounds__(256) void ude_forecast_joint_reduce_kernel(JsArgs a) {
  const int ln = threadIdx.x, b = blockIdx.y, R = a.R, M = a.M;
  const int K = 1 + R + M, k = blockIdx.x * 4 + threadIdx.y;
  if (k >= K) return;                            // whole waves
  const int nt = a.nt, ntp = nt * (nt + 1) / 2;
  // pairs: diagonal tiles once, the others twice.  Lane-strided over the tile pairs, then the fixed butterfly
  double pairs = 0.0, first = 0.0;
  const double* p = a.part + (size_t)b * ntp * 2 * K;
  for (int i = ln; i < ntp; i += 64) {
    int ti = 0, rest = i;
    while (rest >= nt - ti) { rest -= nt - ti; ++ti; }
    const double v = p[(size_t)i * 2 * K + k];
    pairs += rest == 0 ? v : v + v;
    first += p[((size_t)i * 2 + 1) * K + k];
  }
  pairs = js_wave_sum(pairs);
  first = js_wave_sum(first);
  if (ln != 0) return;
  const double dS = (double)a.S;
  const double es = first / dS - pairs / (2.0 * dS * dS);
  if (k == 0) a.e_joint[b] = es;
  else if (k <= R) a.e_series[(size_t)b * R + k - 1] = es;
  else a.e_field[(size_t)b * M + k - 1 - R] = es;
}

// coordinate pair p -> (c, c2), c < c2, counting row by row of c2: p = c2 (c2 - 1) / 2 + c
__device__ __forceinline__ void jv_pair(long long p, int* c, int* c2) {
  long long hi = (long long)((1.0 + sqrt(1.0 + 8.0 * (double)p)) * 0.5);
  while (hi * (hi - 1) / 2 > p) --hi;
  while ((hi + 1) * hi / 2 <= p) ++hi;
  *c2 = (int)hi;
  *c = (int)(p - hi * (hi - 1) / 2);
}

template <bool ROOT>
__device__ __forceinline__ double jv_pow(double d) { return ROOT ? sqrt(fabs(d)) : fabs(d); }

template <bool ROOT>
__global__ __launch_bounds__(256) void ude_forecast_joint_variogram_kernel(JsArgs a) {
  extern __shared__ __attribute__((aligned(16))) double jv_lds[];
  double* red = jv_lds;                          // [256]
  double* tile = jv_lds + 256;                   // [rows][C]
  const int tid = threadIdx.x, R = a.R, M = a.M, S = a.S;
  const size_t BR = (size_t)a.B * R;
  // the block: its C coordinates are (t0 + c dt, r0 + c dr)
  const bool series = blockIdx.x < (unsigned)(a.B * R);
  const int g = series ? blockIdx.x : blockIdx.x - a.B * R;
  const int b = series ? g / R : g / M;
  const int C = series ? M : R;
  const int t0 = series ? a.start : a.start + (g - b * M) * a.every, dt = series ? a.every : 0;
  const int r0 = series ? g - b * R : 0, dr = series ? 0 : 1;
  double* out = series ? a.v_series + g : a.v_field + g;
  const long long n_pairs = (long long)C * (C - 1) / 2;
  const int rows = min(S, JV_TILE / C);
  const double dS = (double)S;

  double total = 0.0;
  for (long long p0 = 0; p0 < n_pairs; p0 += 256 * JV_NPT) {
    int c1[JV_NPT], c2[JV_NPT];
    double acc[JV_NPT];
#pragma unroll
    for (int k = 0; k < JV_NPT; ++k) {
      const long long p = p0 + (long long)k * 256 + tid;
      acc[k] = 0.0;
      c1[k] = c2[k] = -1;
      if (p < n_pairs) jv_pair(p, &c1[k], &c2[k]);
    }
    for (int s0 = 0; s0 < S; s0 += rows) {
      const int n = min(rows, S - s0);
      __syncthreads();                           // the previous tile has been read
      for (int e = tid; e < n * C; e += 256) {
        const int s = e / C, c = e - s * C, r = r0 + c * dr;
        const double sc = a.scale ? a.scale[r] : 1.0;
        tile[e] = (double)a.yhat[((size_t)(t0 + c * dt) * S + s0 + s) * BR + (size_t)b * R + r] * sc;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < JV_NPT; ++k) {
        if (c1[k] >= 0) {
          const double* x1 = tile + c1[k];
          const double* x2 = tile + c2[k];
          double s_acc = acc[k];
          for (int s = 0; s < n; ++s) s_acc += jv_pow<ROOT>(x1[(size_t)s * C] - x2[(size_t)s * C]);
          acc[k] = s_acc;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < JV_NPT; ++k) {
      if (c1[k] >= 0) {
        const int ra = r0 + c1[k] * dr, rb = r0 + c2[k] * dr;
        const double ya = (double)a.y_true[((size_t)b * a.T + t0 + c1[k] * dt) * R + ra] * (a.scale ? a.scale[ra] : 1.0);
        const double yb = (double)a.y_true[((size_t)b * a.T + t0 + c2[k] * dt) * R + rb] * (a.scale ? a.scale[rb] : 1.0);
        const double e = jv_pow<ROOT>(ya - yb) - acc[k] / dS;
        total += e * e;
      }
    }
  }
  __syncthreads();
  red[tid] = total;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) *out = red[0];
}

// means [1 + 2 R + 2 M]: fc_group_mean over the B windows of e_joint | e_series | e_field | v_series | v_field
__global__ __launch_bounds__(256) void ude_forecast_joint_means_kernel(JsArgs a, double* __restrict__ means) {
  const int R = a.R, M = a.M, B = a.B;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= 1 + 2 * R + 2 * M) return;
  double v;
  if (k == 0) v = fc_group_mean(a.e_joint, B, 1);
  else if (k < 1 + R) v = fc_group_mean(a.e_series + (k - 1), B, R);
  else if (k < 1 + R + M) v = fc_group_mean(a.e_field + (k - 1 - R), B, M);
  else if (k < 1 + 2 * R + M) v = fc_group_mean(a.v_series + (k - 1 - R - M), B, R);
  else v = fc_group_mean(a.v_field + (k - 1 - 2 * R - M), B, M);
  means[k] = v;
}

// M, the number of considered times, or 0 when the arguments are out of range.  p_code = 2 p: 1 or 2
inline int js_times(int T, int S, int B, int R, int start, int every, int p_code) {
  if (!fc_shape_ok(T, S, B, R, 0) || S > FC_MAX_SQ || R > JS_MAX_C || B > 65535) return 0;
  if (start < 0 || start >= T || every < 1 || (p_code != 1 && p_code != 2)) return 0;
  const int64_t M = ((int64_t)T - start + every - 1) / every;
  return M > JS_MAX_C ? 0 : (int)M;
}

// workspace: part [B][tile pairs][2][1 + R + M], doubles
inline int forecast_joint_workspace(int T, int S, int B, int R, int start, int every, int p_code, int64_t* ws_bytes) {
  const int M = js_times(T, S, B, R, start, every, p_code);
  if (!ws_bytes || !M) return -2;
  *ws_bytes = (int64_t)B * js_tile_pairs(S) * 2 * (1 + R + M) * 8;
  return 0;
}

inline int forecast_joint(int T, int S, int B, int R, int start, int every, int p_code, const float* yhat,
                          const double* scale, const float* y_true, void* ws, double* e_joint, double* e_series,
                          double* e_field, double* v_series, double* v_field, double* means, hipStream_t s) {
  const int M = js_times(T, S, B, R, start, every, p_code);
  if (!M || !yhat || !y_true || !ws || !e_joint || !e_series || !e_field || !v_series || !v_field || !means) return -2;
  JsArgs a;
  a.yhat = yhat; a.scale = scale; a.y_true = y_true; a.part = (double*)ws;
  a.e_joint = e_joint; a.e_series = e_series; a.e_field = e_field; a.v_series = v_series; a.v_field = v_field;
  a.T = T; a.S = S; a.B = B; a.R = R; a.start = start; a.every = every; a.M = M; a.nt = js_tiles(S);
  const int ntp = js_tile_pairs(S), K = 1 + R + M;
  hipLaunchKernelGGL(ude_forecast_joint_energy_kernel, dim3(ntp, B), dim3(256), 0, s, a);
  if (hipGetLastError() != hipSuccess) return -3;
  const size_t lds = (size_t)(JV_TILE + 256) * 8;
  if (p_code == 1)
    hipLaunchKernelGGL(ude_forecast_joint_variogram_kernel<true>, dim3(B * (R + M)), dim3(256), lds, s, a);
  else
    hipLaunchKernelGGL(ude_forecast_joint_variogram_kernel<false>, dim3(B * (R + M)), dim3(256), lds, s, a);
  if (hipGetLastError() != hipSuccess) return -3;
  hipLaunchKernelGGL(ude_forecast_joint_reduce_kernel, dim3((K + 3) / 4, B), dim3(64, 4), 0, s, a);
  if (hipGetLastError() != hipSuccess) return -3;
  hipLaunchKernelGGL(ude_forecast_joint_means_kernel, dim3((2 * K - 1 + 255) / 256), dim3(256), 0, s, a, means);
  if (hipGetLastError() != hipSuccess) return -3;
  return 0;
}

}  // namespace ude
