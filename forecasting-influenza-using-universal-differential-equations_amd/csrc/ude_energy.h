// Energy-score training head (no model): the energy score of the S trajectories of y_hat (T, S*B, R) against
// targets y (B, T, R) as a differentiable loss -- the definition at ude_energy_forward in include/ude_rk4.h.
// A block is a set of coordinates (t, r) of one window b: joint (all T R, K = 1), series (region r's T times,
// K = R) or field (the R regions at time t, K = T); a coordinate with y == -1 is dropped from its blocks.
//
// Geometry, forward and backward alike: a workgroup owns (b, block, i-tile): 16 samples i against all S samples
// j and the target (row S).  The block's coordinates are swept t ascending, r ascending within t, EN_CC at a
// time: the S + 1 rows of a chunk go to LDS as doubles (thread tid: column tid % 32 of the rows tid / 32 + 8 m;
// for joint and field blocks a wave reads two rows of
// 32 neighbouring regions; a series block reads one float per row and time), a dropped coordinate as 0 in every
// row, so that it adds nothing to any distance and gets the gradient 0.  Thread tid owns the pairs (i, j) =
// (16 ti + tid / 16, tid % 16 + 16 u), u < NJT, the kernel's template parameter: 3, 5 or 9, the smallest that
// covers ceil((S + 1) / 16) (a partner past the target repeats the target's row and is not used).  It adds d d
// with d = x_i - x_j formed directly in fp64 (never |x_i|^2 + |x_j|^2 - 2 x_i . x_j) to the pair's sum of
// squares, four columns at a time; the root is taken once per pair and block.  The row stride is odd, so the 16
// partner rows of a half-wave fall on different banks and the four i rows of a wave are broadcasts.
// A block of more than one chunk (C > 32) has one workgroup per i-tile; a block of one chunk has one workgroup,
// which takes the i-tiles in turn on the tile staged once (a series block at T <= 32, a field block at R <= 32).
//
// Forward: the roots are summed over the workgroup's pairs -- u ascending in the thread, a fixed butterfly in
// each wave, w0 + w1 + w2 + w3 over the waves -- into one partial each for the pair term (all S x S ordered
// pairs: nothing is halved by symmetry, the flops are trivial) and the first term.  A second launch forms
// ES = first / S - pairs / (2 S D) per (b, block), the tiles in order, and sums 256 blocks by a fixed tree; a
// third sums those partials (lane-strided, then the butterfly) and divides by B K.
// Backward: nothing is kept between the calls; the pair distances are formed again by the same sweep, their
// inverses (0 for a distance of exactly 0) times the term's coefficient, 1 / S for the target and -1 / (S D) for
// a sample, go to LDS as w[16][S + 1], and a second sweep over the chunks (staged again only when the block has
// more than one) gives thread (tid / 32 + 8 h, tid % 32) the coordinate's sum_j w_ij (x_ic - x_jc), j ascending,
// direct differences again.  Every element of d y_hat belongs to exactly one (b, block, i-tile) and is written
// once, rounded once from fp64.  No atomics; nothing in the geometry depends on values: the same bits run to
// run.
//
// LDS, dynamic: (S + 1) rows of EN_LD doubles + 8 sums (forward: 34.1 KiB at S = 128, 17.2 KiB at S = 64), the
// backward 16 (S + 1) inverse norms more (50.2 / 25.3 KiB).  Registers and timings: DESIGN.md.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ude {

constexpr int EN_TILE = 16;                            // samples i of a workgroup
constexpr int EN_CC = 32;                              // coordinates of a staged chunk
constexpr int EN_LD = EN_CC + 1;                       // LDS row stride (doubles), odd
constexpr int EN_MAX_S = 128;                          // largest S
constexpr int EN_MAX_C = 1024;                         // largest T and R
enum { EN_JOINT = 0, EN_SERIES = 1, EN_FIELD = 2 };

struct EnArgs {
  const float* yhat;   // (T, S*B, R)
  const float* y;      // (B, T, R), -1 = missing
  const float* grad;   // backward: d loss / d energy, one float
  double* part;        // forward: [B][K][nt][2] pair sums, first-term sums
  float* dyhat;        // backward: (T, S*B, R)
  int T, S, B, R, kind, D, K, nt, ntg;   // ntg: workgroups per block (nt, or 1: en_tile_groups)
};

__host__ __device__ inline int en_blocks(int kind, int T, int R) { return kind == EN_JOINT ? 1 : kind == EN_SERIES ? R : T; }
__host__ __device__ inline int en_tiles(int S) { return (S + EN_TILE - 1) / EN_TILE; }

// the coordinates of block blk: (t0 + q / nR, r0 + q % nR), q < C
struct EnBlock { int t0, r0, nR, C; };
__device__ __forceinline__ EnBlock en_block(const EnArgs& a, int blk) {
  if (a.kind == EN_SERIES) return {0, blk, 1, a.T};
  if (a.kind == EN_FIELD) return {blk, 0, a.R, a.R};
  return {0, 0, a.R, a.T * a.R};
}

// fixed butterfly over the 64 lanes of a wave: every lane has the sum
__device__ __forceinline__ double en_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// chunk ch of the block's coordinates -> tile[S + 1][EN_LD]; columns past the block and dropped coordinates 0
__device__ __forceinline__ void en_stage(const EnArgs& a, double* tile, int b, const EnBlock& k, int ch, int tid) {
  const int c = tid & (EN_CC - 1), q = ch * EN_CC + c;
  const bool in = q < k.C;
  const int dt = in ? q / k.nR : 0;
  const int t = k.t0 + dt, r = k.r0 + (in ? q - dt * k.nR : 0);
  const float yv = in ? a.y[((size_t)b * a.T + t) * a.R + r] : -1.f;
  const bool live = in && yv != -1.f;
  const size_t BR = (size_t)a.B * a.R;
  const float* src = a.yhat + (size_t)t * a.S * BR + (size_t)b * a.R + r;   // sample s at + s BR
  for (int row = tid >> 5; row <= a.S; row += 256 / EN_CC) {
    double v = 0.0;
    if (live) v = row < a.S ? (double)src[(size_t)row * BR] : (double)yv;
    tile[row * EN_LD + c] = v;
  }
}

// acc[u] = sum over the block's live coordinates of (x_i - x_j)^2, i = row irow, j = min(lj + 16 u, S), u < NJT
// (NJT >= ceil((S + 1) / 16): a partner past the target repeats the target's row and is not used).  Four
// columns at a time with every partner's read issued before the first is used; the columns of the last four
// past the block are 0 in every row and add an exact 0.  staged: chunk 0 of a one-chunk block is in the tile.
template <int NJT>
__device__ __forceinline__ void en_sum_squares(const EnArgs& a, double* tile, int b, const EnBlock& k, int irow, int lj,
                                               int tid, bool staged, double (&acc)[NJT]) {
  const int S = a.S, n_ch = (k.C + EN_CC - 1) / EN_CC;
  const double* xj[NJT];
#pragma unroll
  for (int u = 0; u < NJT; ++u) {
    acc[u] = 0.0;
    xj[u] = tile + min(lj + 16 * u, S) * EN_LD;
  }
  const double* xi = tile + irow * EN_LD;
  for (int ch = 0; ch < n_ch; ++ch) {
    if (!staged) {
      __syncthreads();                           // the previous chunk has been read
      en_stage(a, tile, b, k, ch, tid);
      __syncthreads();
    }
    const int cw4 = (min(EN_CC, k.C - ch * EN_CC) + 3) & ~3;
    for (int c0 = 0; c0 < cw4; c0 += 4) {
      double xv[4], xp[4][NJT];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        xv[c] = xi[c0 + c];
#pragma unroll
        for (int u = 0; u < NJT; ++u) xp[c][u] = xj[u][c0 + c];
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int u = 0; u < NJT; ++u) {
          const double d = xv[c] - xp[c][u];
          acc[u] += d * d;
        }
      }
    }
  }
}

// grid.x = (block, tile group): nt tile groups of one i-tile each, or, for a block of one chunk, one group that
// takes the nt i-tiles in turn on the tile staged once
template <int NJT>
__global__ __launch_bounds__(256) void ude_energy_fwd_kernel(EnArgs a) {
  extern __shared__ __attribute__((aligned(16))) double en_lds[];
  const int S = a.S;
  double* tile = en_lds;                         // [S + 1][EN_LD]
  double* red = en_lds + (S + 1) * EN_LD;        // [pairs | first][wave]
  const int tid = threadIdx.x, li = tid >> 4, lj = tid & 15, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.y, blk = blockIdx.x / a.ntg, tg = blockIdx.x - blk * a.ntg;
  const EnBlock k = en_block(a, blk);
  for (int ti = tg; ti < a.nt; ti += a.ntg) {
    const int i = ti * EN_TILE + li;
    double acc[NJT];
    en_sum_squares<NJT>(a, tile, b, k, min(i, S - 1), lj, tid, ti != tg, acc);
    double pairs = 0.0, first = 0.0;
#pragma unroll
    for (int u = 0; u < NJT; ++u) {
      const int j = lj + 16 * u;
      if (i < S && j <= S) {
        const double dist = sqrt(acc[u]);
        if (j < S) pairs += dist;
        else first += dist;
      }
    }
    pairs = en_wave_sum(pairs);
    first = en_wave_sum(first);
    if (lane == 0) {
      red[wave] = pairs;
      red[4 + wave] = first;
    }
    __syncthreads();
    if (tid < 2) {
      const double* w = red + 4 * tid;
      a.part[(((size_t)b * a.K + blk) * a.nt + ti) * 2 + tid] = ((w[0] + w[1]) + w[2]) + w[3];
    }
    __syncthreads();                             // red has been read
  }
}

// part2[workgroup] = sum over its 256 blocks q = (b, block) of ES_q = first / S - pairs / (2 S D), the tiles of a
// block in order, the blocks by a fixed tree
__global__ __launch_bounds__(256) void ude_energy_reduce_kernel(const double* __restrict__ part, int n, int nt, double dS,
                                                                double dD, double* __restrict__ part2) {
  __shared__ double red[256];
  const int tid = threadIdx.x, q = blockIdx.x * 256 + tid;
  double es = 0.0;
  if (q < n) {
    const double* p = part + (size_t)q * nt * 2;
    double pairs = 0.0, first = 0.0;
    for (int t = 0; t < nt; ++t) {
      pairs += p[2 * t];
      first += p[2 * t + 1];
    }
    es = first / dS - pairs / (2.0 * dS * dD);
  }
  red[tid] = es;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) part2[blockIdx.x] = red[0];
}

// out[0] = (float)((the n2 partials, lane-strided then the butterfly) / (B K))
__global__ __launch_bounds__(64) void ude_energy_finalize_kernel(const double* __restrict__ part2, int n2, double BK,
                                                                 float* __restrict__ out) {
  const int ln = threadIdx.x;
  double s = 0.0;
  for (int i = ln; i < n2; i += 64) s += part2[i];
  s = en_wave_sum(s);
  if (ln == 0) out[0] = (float)(s / BK);
}

template <int NJT>
__global__ __launch_bounds__(256) void ude_energy_bwd_kernel(EnArgs a) {
  extern __shared__ __attribute__((aligned(16))) double en_lds[];
  const int S = a.S, W = S + 1;
  double* tile = en_lds;                         // [S + 1][EN_LD]
  double* w = en_lds + W * EN_LD;                // [16][S + 1]: coefficient / distance
  const int tid = threadIdx.x, li = tid >> 4, lj = tid & 15;
  const int b = blockIdx.y, blk = blockIdx.x / a.ntg, tg = blockIdx.x - blk * a.ntg;
  const EnBlock k = en_block(a, blk);
  const double c_pair = -1.0 / ((double)S * (double)a.D), c_first = 1.0 / (double)S;
  const double gs = (double)a.grad[0] / ((double)a.B * (double)a.K);
  const size_t BR = (size_t)a.B * a.R;
  const int n_ch = (k.C + EN_CC - 1) / EN_CC, c = tid & (EN_CC - 1);
  for (int ti = tg; ti < a.nt; ti += a.ntg) {
    const int i0 = ti * EN_TILE;
    double acc[NJT];
    en_sum_squares<NJT>(a, tile, b, k, min(i0 + li, S - 1), lj, tid, ti != tg, acc);
#pragma unroll
    for (int u = 0; u < NJT; ++u) {
      const int j = lj + 16 * u;
      if (j <= S) {
        const double inv = acc[u] > 0.0 ? 1.0 / sqrt(acc[u]) : 0.0;
        w[li * W + j] = inv * (j == S ? c_first : c_pair);
      }
    }
    __syncthreads();
    for (int ch = 0; ch < n_ch; ++ch) {
      if (n_ch > 1) {                            // a block of one chunk is still in the tile
        __syncthreads();
        en_stage(a, tile, b, k, ch, tid);
        __syncthreads();
      }
      const int q = ch * EN_CC + c;
      if (q < k.C) {
        const int dt = q / k.nR, t = k.t0 + dt, r = k.r0 + q - dt * k.nR;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int l = (tid >> 5) + 8 * h, i = i0 + l;
          if (i < S) {
            const double xv = tile[i * EN_LD + c];
            const double* wl = w + l * W;
            const double* xc = tile + c;
            double sum = 0.0;
#pragma unroll 8
            for (int j = 0; j <= S; ++j) sum += wl[j] * (xv - xc[j * EN_LD]);
            a.dyhat[((size_t)t * S + i) * BR + (size_t)b * a.R + r] = (float)(gs * sum);
          }
        }
      }
    }
    __syncthreads();                             // w (and a one-chunk tile's reads) are done before the next i-tile
  }
}

// the partners a thread holds: the smallest of 3, 5, 9 that covers ceil((S + 1) / 16)
inline int en_partners(int S) { return S + 1 <= 48 ? 3 : S + 1 <= 80 ? 5 : 9; }
// tile groups of a block: one (the i-tiles in turn) when the block is one chunk, else one per i-tile
inline int en_tile_groups(int kind, int T, int S, int R) {
  const int C = kind == EN_JOINT ? T * R : kind == EN_SERIES ? T : R;
  return C <= EN_CC ? 1 : en_tiles(S);
}

inline bool en_shape_ok(int T, int S, int B, int R, int kind, int fair) {
  return T >= 1 && T <= EN_MAX_C && R >= 1 && R <= EN_MAX_C && S >= 1 && S <= EN_MAX_S && B >= 1 && B <= 65535 &&
         kind >= EN_JOINT && kind <= EN_FIELD && !(fair && S < 2);
}

// the partials are doubles: 8-byte aligned
inline bool en_ws_ok(const void* ws) { return ws && ((uintptr_t)ws & 7) == 0; }

// workspace: part [B][K][nt][2] doubles | part2 [ceil(B K / 256)] doubles
inline int energy_workspace(int T, int S, int B, int R, int kind, int64_t* ws_bytes) {
  if (!ws_bytes || !en_shape_ok(T, S, B, R, kind, 0)) return -2;
  const int64_t n = (int64_t)B * en_blocks(kind, T, R);
  *ws_bytes = (n * en_tiles(S) * 2 + (n + 255) / 256) * 8;
  return 0;
}

inline int energy_forward(int T, int S, int B, int R, int kind, int fair, const float* yhat, const float* y, void* ws,
                          float* out, hipStream_t s) {
  if (!en_shape_ok(T, S, B, R, kind, fair) || !yhat || !y || !en_ws_ok(ws) || !out) return -2;
  const int K = en_blocks(kind, T, R), nt = en_tiles(S), n = B * K, n2 = (n + 255) / 256;
  EnArgs a{yhat, y, nullptr, (double*)ws, nullptr, T, S, B, R, kind, fair ? S - 1 : S, K, nt,
           en_tile_groups(kind, T, S, R)};
  double* part2 = a.part + (size_t)n * nt * 2;
  const size_t lds = ((size_t)(S + 1) * EN_LD + 8) * 8;
  const dim3 grid(K * a.ntg, B);
  switch (en_partners(S)) {
    case 3: hipLaunchKernelGGL(ude_energy_fwd_kernel<3>, grid, dim3(256), lds, s, a); break;
    case 5: hipLaunchKernelGGL(ude_energy_fwd_kernel<5>, grid, dim3(256), lds, s, a); break;
    default: hipLaunchKernelGGL(ude_energy_fwd_kernel<9>, grid, dim3(256), lds, s, a);
  }
  if (hipGetLastError() != hipSuccess) return -3;
  hipLaunchKernelGGL(ude_energy_reduce_kernel, dim3(n2), dim3(256), 0, s, (const double*)a.part, n, nt, (double)S,
                     (double)a.D, part2);
  if (hipGetLastError() != hipSuccess) return -3;
  hipLaunchKernelGGL(ude_energy_finalize_kernel, dim3(1), dim3(64), 0, s, (const double*)part2, n2,
                     (double)B * (double)K, out);
  if (hipGetLastError() != hipSuccess) return -3;
  return 0;
}

inline int energy_backward(int T, int S, int B, int R, int kind, int fair, const float* yhat, const float* y,
                           const float* grad, float* dyhat, hipStream_t s) {
  if (!en_shape_ok(T, S, B, R, kind, fair) || !yhat || !y || !grad || !dyhat) return -2;
  const int K = en_blocks(kind, T, R), nt = en_tiles(S);
  EnArgs a{yhat, y, grad, nullptr, dyhat, T, S, B, R, kind, fair ? S - 1 : S, K, nt, en_tile_groups(kind, T, S, R)};
  const size_t lds = ((size_t)(S + 1) * EN_LD + (size_t)EN_TILE * (S + 1)) * 8;
  const dim3 grid(K * a.ntg, B);
  switch (en_partners(S)) {
    case 3: hipLaunchKernelGGL(ude_energy_bwd_kernel<3>, grid, dim3(256), lds, s, a); break;
    case 5: hipLaunchKernelGGL(ude_energy_bwd_kernel<5>, grid, dim3(256), lds, s, a); break;
    default: hipLaunchKernelGGL(ude_energy_bwd_kernel<9>, grid, dim3(256), lds, s, a);
  }
  if (hipGetLastError() != hipSuccess) return -3;
  return 0;
}

}  // namespace ude
