// CRPS training head (no model): the sample-based CRPS of y_hat (T, S*B, R) against targets y (B, T, R) as a
// differentiable loss -- the definition at ude_crps_forward in include/ude_rk4.h.  Per group (t, b, r), with
// x_(0) <= .. <= x_(S-1) the sorted samples x_s = y_hat[t, s*B+b, r] and D = S (fair: S - 1),
//   c     = sum_s |x_s - y| / S - sum_i (2 i - S + 1) x_(i) / (S D)
//   num_s = D sgn(x_s - y) - (#{x_j < x_s} + #{x_j <= x_s} - S)        (an integer; 0 where y == -1)
//   loss  = sum of c over the groups with y != -1, / (B T R);   d loss / d x_s = g / (B T R) * num_s / (S D)
//
// The forward is the summary kernel's geometry (ude_forecast.h: fc_geom, one coalesced read of y_hat into the
// [S'][G] fp64 LDS tile, fc_bitonic_sort).  The sort moves values only, so a sample's ranks come from two binary
// searches of its own value in its sorted column (fc_count_below: sorted values only, every bound S -- the +inf
// padding rows are never read); the value is the fp32 element read again (the workgroup read it a sort ago, so
// it should still be in L2: supposed, no counter run).  What the backward needs is the int16 numerator per element (|num| <= 2 S <= 2048): 2 bytes per
// element of y_hat, so the backward is one streaming pass and never sorts.  Per workgroup one fp64 partial (its
// columns' c summed serially), a second launch sums the partials in a fixed order: no atomics, the same bits
// run to run.  Everything after the fp32 load is fp64; out[0] and d y_hat are rounded once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ude_forecast.h"

namespace ude {

struct CrpsArgs {
  const float* yhat;   // (T, S*B, R)
  const float* y;      // (B, T, R), -1 = missing
  double* part;        // [T][nbx]
  int16_t* num;        // (T, S*B, R): the gradient numerators
  int T, S, B, R, fair;
};

// fc_col_crps with the pair term over S D instead of S^2 (D = S - 1: the fair score); same sums, same order
__device__ __forceinline__ double crps_col_fair(double* red, const double* tile, double y, int S, int D, int rr, int c,
                                                int G, int RP) {
  double w = 0.0, ad = 0.0;
  for (int i = rr; i < S; i += RP) {
    const double x = tile[i * G + c];
    w += (double)(2 * i - S + 1) * x;
    ad += fabs(x - y);
  }
  const double wsum = fc_col_sum(red, w, rr, c, G, RP);
  const double asum = fc_col_sum(red, ad, rr, c, G, RP);
  const double dS = (double)S;
  return asum / dS - wsum / (dS * (double)D);
}

__global__ __launch_bounds__(FC_THREADS) void ude_crps_fwd_kernel(CrpsArgs a) {
  extern __shared__ __attribute__((aligned(16))) double fc_lds[];
  const int BR = a.B * a.R, S = a.S;
  const FcGeom ge = fc_geom(S, BR, 1);
  const int G = ge.G, RP = FC_THREADS / G, rows = ge.rows;
  double* red = fc_lds;                          // [RP][G] = 256 doubles
  double* tile = fc_lds + FC_THREADS;            // [rows][G]
  const int tid = threadIdx.x, c = tid & (G - 1), rr = tid / G;
  const int t = blockIdx.y, g = blockIdx.x * G + c;
  const bool live = g < BR;
  const int b = live ? g / a.R : 0, r = live ? g - b * a.R : 0;
  const size_t col = (size_t)t * S * BR + g;     // element (t, s = 0, g); s advances by BR
  const float* src = a.yhat + col;

  for (int s = rr; s < rows; s += RP)
    tile[s * G + c] = s < S ? (live ? (double)src[(size_t)s * BR] : 0.0) : (double)INFINITY;
  const float yf = live ? a.y[((size_t)b * a.T + t) * a.R + r] : -1.f;
  const bool scored = live && yf != -1.f;        // a masked group counts in the divisor only
  const double y = (double)yf;
  fc_bitonic_sort(tile, rows, rr, c, G, RP);

  const int D = a.fair ? S - 1 : S;
  const double crps = a.fair ? crps_col_fair(red, tile, y, S, D, rr, c, G, RP)
                             : fc_col_crps(red, tile, y, S, rr, c, G, RP);
  if (live) {
    int16_t* dst = a.num + col;
    for (int s = rr; s < S; s += RP) {
      int num = 0;
      if (scored) {
        const double x = (double)src[(size_t)s * BR];
        const int n_lt = fc_count_below<false>(tile, c, G, S, x), n_le = fc_count_below<true>(tile, c, G, S, x);
        num = D * ((x > y) - (x < y)) - (n_lt + n_le - S);
      }
      dst[(size_t)s * BR] = (int16_t)num;
    }
  }
  __syncthreads();                               // red[c] (the column's wsum / asum) has been read
  if (rr == 0) red[c] = scored ? crps : 0.0;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < G; ++i) s += red[i];
    a.part[(size_t)t * gridDim.x + blockIdx.x] = s;
  }
}

// out[0] = (float)((the n partials, lane-strided then a fixed butterfly) / M)
__global__ __launch_bounds__(64) void ude_crps_finalize_kernel(const double* __restrict__ part, int n, double M,
                                                               float* __restrict__ out) {
  const int ln = threadIdx.x;
  const double s = fc_wave_sum(part, 0, n, 1, 0, ln);
  if (ln == 0) out[0] = (float)(s / M);
}

// d y_hat[e] = (float)(grad[0] / M * num[e] / (S D)): thread i < n8 takes the 8 elements from 8 i (one 16-byte
// read, two 16-byte writes), the threads behind them one element each of the tail from 8 n8
__global__ __launch_bounds__(256) void ude_crps_bwd_kernel(const int16_t* __restrict__ num,
                                                           const float* __restrict__ grad, double M, double SD,
                                                           size_t n8, size_t n, float* __restrict__ dyhat) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const double sc = (double)grad[0] / M;
  if (i < n8) {
    union { uint4 q; int16_t h[8]; } v;
    v.q = *reinterpret_cast<const uint4*>(num + 8 * i);
    float4 lo, hi;
    lo.x = (float)(sc * (double)v.h[0] / SD);
    lo.y = (float)(sc * (double)v.h[1] / SD);
    lo.z = (float)(sc * (double)v.h[2] / SD);
    lo.w = (float)(sc * (double)v.h[3] / SD);
    hi.x = (float)(sc * (double)v.h[4] / SD);
    hi.y = (float)(sc * (double)v.h[5] / SD);
    hi.z = (float)(sc * (double)v.h[6] / SD);
    hi.w = (float)(sc * (double)v.h[7] / SD);
    float4* dst = reinterpret_cast<float4*>(dyhat + 8 * i);
    dst[0] = lo;
    dst[1] = hi;
  } else {
    const size_t e = 8 * n8 + (i - n8);
    if (e < n) dyhat[e] = (float)(sc * (double)num[e] / SD);
  }
}

inline bool crps_shape_ok(int T, int S, int B, int R, int fair) {
  return fc_shape_ok(T, S, B, R, 1) && !(fair && S < 2);
}

// ws holds fp64 partials at its start: 8-byte aligned (the int16 numerators follow at a multiple of 256)
inline bool crps_ws_ok(const void* ws) { return ws && ((uintptr_t)ws & 7) == 0; }

// workspace: part [T][nbx] doubles | num (T, S*B, R) int16 from the next multiple of 256 bytes
inline int64_t crps_num_off(int T, int S, int B, int R) {
  const int64_t part = (int64_t)T * fc_geom(S, B * R, 1).nbx * 8;
  return (part + 255) / 256 * 256;
}

inline int crps_workspace(int T, int S, int B, int R, int64_t* ws_bytes) {
  if (!ws_bytes || !crps_shape_ok(T, S, B, R, 0)) return -2;
  *ws_bytes = crps_num_off(T, S, B, R) + (int64_t)T * S * B * R * 2;
  return 0;
}

inline int crps_forward(int T, int S, int B, int R, int fair, const float* yhat, const float* y, void* ws, float* out,
                        hipStream_t s) {
  if (!crps_shape_ok(T, S, B, R, fair) || !yhat || !y || !crps_ws_ok(ws) || !out) return -2;
  const FcGeom ge = fc_geom(S, B * R, 1);
  if ((int64_t)T * ge.nbx > (int64_t)1 << 30) return -2;
  CrpsArgs a{yhat, y, (double*)ws, (int16_t*)((unsigned char*)ws + crps_num_off(T, S, B, R)), T, S, B, R, fair != 0};
  const size_t lds = ((size_t)FC_THREADS + (size_t)ge.rows * ge.G) * 8;
  hipLaunchKernelGGL(ude_crps_fwd_kernel, dim3(ge.nbx, T), dim3(FC_THREADS), lds, s, a);
  if (hipGetLastError() != hipSuccess) return -3;
  hipLaunchKernelGGL(ude_crps_finalize_kernel, dim3(1), dim3(64), 0, s, (const double*)a.part, T * ge.nbx,
                     (double)B * (double)T * (double)R, out);
  if (hipGetLastError() != hipSuccess) return -3;
  return 0;
}

inline int crps_backward(int T, int S, int B, int R, int fair, const float* grad, const void* ws, float* dyhat,
                         hipStream_t s) {
  if (!crps_shape_ok(T, S, B, R, fair) || !grad || !crps_ws_ok(ws) || !dyhat) return -2;
  const int16_t* num = (const int16_t*)((const unsigned char*)ws + crps_num_off(T, S, B, R));
  const size_t n = (size_t)T * S * B * R;
  // 16-byte accesses need both pointers 16-byte aligned (num follows ws's alignment: its offset is a multiple of 256)
  const bool vec = (((uintptr_t)num | (uintptr_t)dyhat) & 15) == 0;
  const size_t n8 = vec ? n / 8 : 0, threads = n8 + (n - 8 * n8), blocks = (threads + 255) / 256;
  if (blocks > (size_t)0x7fffffff) return -2;
  hipLaunchKernelGGL(ude_crps_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, num, grad,
                     (double)B * (double)T * (double)R, (double)S * (double)(fair ? S - 1 : S), n8, n, dyhat);
  if (hipGetLastError() != hipSuccess) return -3;
  return 0;
}

}  // namespace ude
