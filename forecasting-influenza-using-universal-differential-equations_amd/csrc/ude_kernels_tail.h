// Behind the backward: the deterministic reductions over the per-workgroup partials (slab -> parameter order,
// gradient finalize, the BAYES eps slab), the static-feature gradients, ude_bwd_tail_kernel and
// ude_stats_finalize_kernel.
#pragma once
#include "ude_kernels_core.h"
#include "ude_kernels_pack.h"   // static_col

namespace ude {

// ============================================================================
// Deterministic reductions over the per-workgroup partials
// ============================================================================
// Slab offset -> index into the torch-ordered parameter vector (-1: padding).
// Inverse of the dW tile layout: tile T = dyn_tiles_before(d, k) + ct holds rows
// frt(d, k) * 16 + [0, 16) of layer d of net fnet(d, k) and input columns ct * 16 +
// [0, 16) in MFMA C order (lane = (row >> 2) * 16 + col, reg = row & 3).
template <class M>
__device__ __forceinline__ int slab_to_param(int off) {
  int e = -1;
  if (off >= M::SLAB_DB) {
    const int idx = off - M::SLAB_DB, T = idx >> 4, row = idx & 15;
    sfor<M::D>([&](auto ii) {
      constexpr int i = decltype(ii)::value;
      if (T >= M::FTbase(i) && T < M::FTbase(i) + M::FT(i)) {
        const int k = T - M::FTbase(i);
        sfor<2>([&](auto nn) {
          constexpr int net = decltype(nn)::value;
          if constexpr (M::has(net, i)) {
            constexpr int kb = net == 0 ? 0 : M::rto(0, i);
            constexpr int in_full = i == 0 ? M::R * M::L : M::in_dim(net, i);
            if (k >= kb && k < kb + M::rto(net, i)) {
              const int o = (k - kb) * 16 + row;
              if (o < M::out_dim(net, i)) e = M::param_w_off(net, i) + M::out_dim(net, i) * in_full + o;
            }
          }
        });
      }
    });
    return e;
  }
  const int T = off >> 8, wq = off & 255, ln = wq >> 2;
  const int row = (ln >> 4) * 4 + (wq & 3), fc = ln & 15;
  sfor<M::D>([&](auto ii) {
    constexpr int i = decltype(ii)::value;
    sfor<M::FT(i)>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      constexpr int net = M::fnet(i, k);
      constexpr int t0 = M::dyn_tiles_before(i, k);
      if (T >= t0 && T < t0 + M::rti(net, i)) {
        const int f = (T - t0) * 16 + fc;
        const int o = M::frt(i, k) * 16 + row;
        constexpr int in_full = i == 0 ? M::R * M::L : M::in_dim(net, i);
        const int col = i == 0 ? M::col0(f) : (f < M::in_dim(net, i) ? f : -1);
        if (o < M::out_dim(net, i) && col >= 0) e = M::param_w_off(net, i) + o * in_full + col;
      }
    });
  });
  return e;
}

// Deterministic cross-workgroup reduction of the gradient slabs: a block owns 64
// consecutive slab offsets (coalesced reads) x 4 groups of slabs, each summed in
// slab order, then combined in a fixed order; the result is scattered to torch order.
template <class M>
__device__ __forceinline__ void grad_finalize_body(const float* __restrict__ slab, int ngrid, float* __restrict__ dparams,
                                                   int blk, float (*part)[64]) {
  const int lo = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int off = blk * 64 + lo;
  float v = 0.f;
  if (off < M::SLAB_TOTAL) {
    const int per = (ngrid + 3) / 4, g0 = grp * per, g1 = min(ngrid, g0 + per);
    const float* p = slab + off;
#pragma unroll 8
    for (int gi = g0; gi < g1; ++gi) v += p[(size_t)gi * M::SLAB_STRIDE];
  }
  part[grp][lo] = v;
  __syncthreads();
  if (grp == 0 && off < M::SLAB_TOTAL) {
    const int e = slab_to_param<M>(off);
    if (e >= 0) dparams[e] = (part[0][lo] + part[1][lo]) + (part[2][lo] + part[3][lo]);
  }
}

// BAYES: the eps stream ([eval][N_PARAMS], torch order) re-laid out per evaluation in
// slab order (dW tiles in MFMA C order, bias rows), the layout the backward weights
// each evaluation's dW / bias sums with.  Padding slots get 0.
template <class M>
__global__ __launch_bounds__(256) void ude_eps_slab_kernel(const float* __restrict__ eps,
                                                           float* __restrict__ eslab) {
  const int off = blockIdx.x * 256 + threadIdx.x;
  const size_t ev = blockIdx.y;
  if (off >= M::SLAB_TOTAL) return;
  const int p = slab_to_param<M>(off);
  eslab[ev * M::SLAB_TOTAL + off] = p >= 0 ? eps[ev * M::N_PARAMS + p] : 0.f;
}

// ============================================================================
// Static-feature gradients (latent dims >= 3 are per-trajectory constants):
//   dW0[o][static s] = sum_n G0[n][o] * y0[n][static s]
//   dy0[n][static s] = sum_o W0[o][static s] * G0[n][o] + sum_j dlatent[j][n][static s]
// with G0[n][o] = sum over every evaluation of the layer-0 output gradient.
// ============================================================================
// One trajectory tile of the dW0[:, static] GEMM for the lane's static column (region r, static dim
// cc; s_ok: not a pad column): acc[o] += G0[tile] (row tile o: K0 x 16 trajectories) x x_static[tile]
// (16 x the column); MFMA q covers trajectories 4g + q.  The callers own the tile walk; acc goes by value.
template <class M>
struct StaticAcc { f4 v[M::K0 / 16]; };
template <class M>
__device__ __forceinline__ StaticAcc<M> static_tile_mac(const float* g0buf, const float* y0, int n_traj, int tile, int t,
                                                        int g, int r, int cc, bool s_ok, StaticAcc<M> acc) {
  constexpr int NOT = M::K0 / 16;
  f4 a[NOT];
#pragma unroll
  for (int o = 0; o < NOT; ++o)
    a[o] = *reinterpret_cast<const f4*>(g0buf + ((size_t)tile * M::K0 + o * 16 + t) * TT + 4 * g);
  float b[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = tile * TT + 4 * g + q;
    b[q] = (s_ok && n < n_traj) ? y0[((size_t)n * M::R + r) * M::L + 3 + cc] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int o = 0; o < NOT; ++o) acc.v[o] = mfma4(a[o][q], b[q], acc.v[o]);
  return acc;
}

// dparams index (torch order) of dW0[row om of the nets' stacked layer-0 outputs][static column s];
// -1 for a pad row
template <class M>
__device__ __forceinline__ int64_t static_dparam_index(int om, int s) {
  constexpr int P0 = M::HAS_P ? M::kout(0, 0) : 0;   // rows [0, P0): the rate net; behind them: the augmentation net
  const int net = om >= P0 ? 1 : 0, o = om - (net ? P0 : 0);
  if (o >= (net ? M::out_dim(1, 0) : M::out_dim(0, 0))) return -1;
  return (net ? M::param_w_off(1, 0) : M::param_w_off(0, 0)) + (int64_t)o * M::R * M::L + static_col<M>(s);
}

// d y0[:, static] = G0[tile]^T (16 x K0) x W0SP (K0 x S16) on MFMA, plus the direct
// cotangents of every output time (static latent dims are carried unchanged).
// One workgroup per trajectory tile; wave w owns static column tiles w, w + 4, ...
// The time sums read the tile's contiguous (16, R, L) block of every output time
// (coalesced, all dims) into LDS first: the static dims alone are a 5-of-8 stride.
template <class M>
__device__ __forceinline__ void dy0_static_body(const float* __restrict__ g0buf, const float* __restrict__ pack,
                                                const float* __restrict__ dlatent, int n_traj, int n_times,
                                                float* __restrict__ dy0, int tile, float* tsum) {
  // tsum: [TT][R][L] time sums of d latent (LDS)
  constexpr int NST = M::S16 / 16, SPW = (NST + 3) / 4, BLK = TT * M::R * M::L;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, t = lane & 15, g = lane >> 4;
  const size_t NRL = (size_t)n_traj * M::R * M::L;
  if (!dlatent) {                                    // static cotangents all zero
    #pragma unroll 1
    for (int i = threadIdx.x; i < BLK; i += 256) tsum[i] = 0.f;
  } else {
    const int nvalid = min(TT, n_traj - tile * TT) * M::R * M::L;
    const float* blk = dlatent + (size_t)tile * BLK;
    if constexpr ((M::R * M::L) % 4 == 0) {
      // 16-B loads, 8 output times in flight per lane (the sums stay in time order)
      #pragma unroll 1
      for (int i = 4 * threadIdx.x; i < BLK; i += 4 * 256) {
        f4 v = f4zero();
        if (i < nvalid) {
#pragma unroll 8
          for (int jt = 0; jt < n_times; ++jt) v += *reinterpret_cast<const f4*>(blk + (size_t)jt * NRL + i);
        }
        *reinterpret_cast<f4*>(tsum + i) = v;
      }
    } else {
      #pragma unroll 1
      for (int i = threadIdx.x; i < BLK; i += 256) {
        float v = 0.f;
        if (i < nvalid) {
#pragma unroll 8
          for (int jt = 0; jt < n_times; ++jt) v += blk[(size_t)jt * NRL + i];
        }
        tsum[i] = v;
      }
    }
  }
  __syncthreads();
  const float* gb = g0buf + (size_t)tile * M::K0 * TT;
  const float* wp = pack + M::W0SP_OFF;
  // operands in batches of QB k-steps, loaded unconditionally (column tiles past NST clamp
  // to the last one; their results are never stored) so a batch's loads are all in flight
  // before its MFMAs -- a guarded load per MFMA serialises on its latency
  constexpr int KQ = M::K0 / 4, QB = 8;
  int col[SPW];
#pragma unroll
  for (int j = 0; j < SPW; ++j) col[j] = min(w + 4 * j, NST - 1) * 16 + t;
  f4 acc[SPW];
#pragma unroll
  for (int j = 0; j < SPW; ++j) acc[j] = f4zero();
#pragma unroll
  for (int q0 = 0; q0 < KQ; q0 += QB) {
    float a[QB], b[QB][SPW];
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
      if (q0 + qq < KQ) {
        const int k = 4 * (q0 + qq) + g;
        a[qq] = gb[k * TT + t];                        // A[traj t][o = k]
#pragma unroll
        for (int j = 0; j < SPW; ++j) b[qq][j] = wp[k * M::S16 + col[j]];
      }
    }
#pragma unroll
    for (int qq = 0; qq < QB; ++qq)
      if (q0 + qq < KQ)
#pragma unroll
        for (int j = 0; j < SPW; ++j) acc[j] = mfma4(a[qq], b[qq][j], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < SPW; ++j) {
    const int s = (w + 4 * j) * 16 + t;
    if (w + 4 * j >= NST || s >= M::S) continue;
    const int r = s / (M::L - 3), cc = s - r * (M::L - 3);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = tile * TT + 4 * g + e;
      if (n < n_traj)
        dy0[((size_t)n * M::R + r) * M::L + 3 + cc] = acc[j][e] + tsum[((4 * g + e) * M::R + r) * M::L + 3 + cc];
    }
  }
}

// ---- the backward's tail in ONE launch ----------------------------------------
// Three independent jobs, one block role each, run side by side instead of four launches in series:
//   [0, TCH * NST)              static weight gradient dW0[:, static] = sum_n G0[n] x_static[n]^T:
//                               block (chunk c, static column tile st), 4 waves over the chunk's tiles,
//                               summed in LDS in wave order, the chunk partial written; the last chunk
//                               block of column tile st to arrive (ticket on ctl[1 + st], agent-scope
//                               release / acquire) sums the TCH partials in chunk order and scatters
//                               them to torch order -- no separate reduce launch, deterministic
//   [.., + ngf)                 the gradient slabs' fixed-order sum (grad_finalize_body; BAYES: both
//                               halves)
//   [.., + n_tiles)             dy0 static of one trajectory tile (dy0_static_body: HBM-bound time sums
//                               of d latent + G0^T W0SP on MFMA)
// The latency-bound chunk blocks are dispatched first (blocks start in index order), the bandwidth-bound
// dy0 blocks fill the chip behind them.  ctl[1 ..] are zero on entry and left zero.
// static-gradient chunks: fewer, longer chunks win -- the last block's fixed-order sum of the chunk
// partials (device-coherent loads) is the tail's long pole (state49 bwd + tail 1.719 / 1.686 / 1.692 ms
// at 32 / 16 / 8 chunks, 1.737 / 1.810 at 64 / 128: profiles/r05/ab_tch_*.txt)
constexpr int TCH = 16;
template <class M>
struct Tail {
  static constexpr int NST = M::S16 / 16, NOT = M::K0 / 16;
  static constexpr int N_SP = M::HOIST ? TCH * NST : 0;
  static constexpr int NGF = (M::SLAB_TOTAL + 63) / 64;
  static constexpr int N_GF = NGF * (M::BAYES ? 2 : 1);
  // dynamic LDS: the dy0 tile's time sums, or 3 waves' static-gradient partial tiles
  static constexpr int LDS = cmax(M::HOIST ? TT * M::R * M::L * 4 : 0, 3 * NOT * 256 * 4 + 16);
  static int blocks(int n_tiles) { return (M::HOIST ? n_tiles : 0) + N_SP + N_GF; }
  // chunk partials [NST][TCH][NOT][64 lanes][4] (MFMA C order) behind the G0 sums
  static constexpr int64_t part_floats() { return M::HOIST ? (int64_t)NST * TCH * NOT * 256 : 0; }
};

template <class M>
__device__ void static_grad_chunk(const float* __restrict__ g0buf, const float* __restrict__ y0, int n_traj,
                                  int n_tiles, float* __restrict__ part, unsigned int* ctl,
                                  float* __restrict__ dparams, int c, int st, float* lds) {
  constexpr int NOT = Tail<M>::NOT, NST = Tail<M>::NST;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, t = lane & 15, g = lane >> 4;
  const int per = (n_tiles + TCH - 1) / TCH;
  const int tb = c * per, te = min(n_tiles, tb + per);
  const int s = st * 16 + t;
  const int r = s / (M::L - 3), cc = s - r * (M::L - 3);
  const bool s_ok = s < M::S;
  StaticAcc<M> acc;
#pragma unroll
  for (int o = 0; o < NOT; ++o) acc.v[o] = f4zero();
  #pragma unroll 4
  for (int tile = tb + w; tile < te; tile += WAVES) {
    acc = static_tile_mac<M>(g0buf, y0, n_traj, tile, t, g, r, cc, s_ok, acc);
  }
  // the 4 waves' partial tiles summed in wave order (LDS), written as this chunk's partial
  f4* red = reinterpret_cast<f4*>(lds);
  if (w > 0) {
#pragma unroll
    for (int o = 0; o < NOT; ++o) red[((w - 1) * NOT + o) * 64 + lane] = acc.v[o];
  }
  __syncthreads();
  unsigned int* flag = reinterpret_cast<unsigned int*>(lds) + 3 * NOT * 256;   // behind the partial tiles
  if (w == 0) {
    // device-coherent (sc1) stores, acknowledged before the ticket (publish_fence; the ordering
    // argument and why no agent-scope fence: see finalize_stats_last)
    double* dst = reinterpret_cast<double*>(part + ((size_t)st * TCH + c) * NOT * 256);
#pragma unroll
    for (int o = 0; o < NOT; ++o) {
      const f4 v = ((acc.v[o] + red[o * 64 + lane]) + red[(NOT + o) * 64 + lane]) + red[(2 * NOT + o) * 64 + lane];
      __hip_atomic_store(dst + (o * 64 + lane) * 2, __builtin_bit_cast(double, __builtin_shufflevector(v, v, 0, 1)),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(dst + (o * 64 + lane) * 2 + 1, __builtin_bit_cast(double, __builtin_shufflevector(v, v, 2, 3)),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    publish_fence();
    unsigned int ticket = 0;
    if (lane == 0) ticket = __hip_atomic_fetch_add(ctl + 1 + st, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0) *flag = ticket;
  }
  __syncthreads();
  if (*flag != TCH - 1) return;                      // block-uniform
  __asm__ __volatile__("" ::: "memory");             // the partial loads stay behind the ticket
  // last chunk of column tile st: the TCH partials in chunk order (device-coherent loads); element
  // (o, lane, e) is row o * 16 + 4 (lane / 16) + e, static column st * 16 + lane % 16
  const double* src = reinterpret_cast<const double*>(part + (size_t)st * TCH * NOT * 256);
  for (int i = threadIdx.x; i < NOT * 64; i += 256) {
    f4 v = f4zero();
    #pragma unroll 8
    for (int ch = 0; ch < TCH; ++ch) {
      const double* q = src + ((size_t)ch * NOT * 64 + i) * 2;
      typedef float f2 __attribute__((ext_vector_type(2)));
      const f2 lo = __builtin_bit_cast(f2, __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      const f2 hi = __builtin_bit_cast(f2, __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      const f4 u = {lo[0], lo[1], hi[0], hi[1]};
      v += u;
    }
    const int o = i >> 6, ln = i & 63;
    const int sc = st * 16 + (ln & 15);
    if (sc >= M::S) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t idx = static_dparam_index<M>(o * 16 + 4 * (ln >> 4) + e, sc);
      if (idx >= 0) dparams[idx] = v[e];
    }
  }
  if (threadIdx.x == 0) ctl[1 + st] = 0u;
  (void)NST;
}

template <class M>
__global__ __launch_bounds__(256) void ude_bwd_tail_kernel(const float* __restrict__ slab, int ngrid,
                                                           const float* __restrict__ g0buf,
                                                           const float* __restrict__ pack,
                                                           const float* __restrict__ y0,
                                                           const float* __restrict__ dlatent, int n_traj,
                                                           int n_tiles, int n_times, float* __restrict__ part,
                                                           unsigned int* ctl, float* __restrict__ dy0,
                                                           float* __restrict__ dparams) {
  extern __shared__ __attribute__((aligned(16))) float tl[];
  int b = blockIdx.x;
  if constexpr (M::HOIST) {
    if (b < Tail<M>::N_SP) {
      static_grad_chunk<M>(g0buf, y0, n_traj, n_tiles, part, ctl, dparams, b % TCH, b / TCH, tl);
      return;
    }
    b -= Tail<M>::N_SP;
  }
  if (b < Tail<M>::N_GF) {
    float (*pp)[64] = reinterpret_cast<float (*)[64]>(tl);
    if (M::BAYES && b >= Tail<M>::NGF)
      grad_finalize_body<M>(slab + M::SLAB_TOTAL, ngrid, dparams + M::N_PARAMS, b - Tail<M>::NGF, pp);
    else
      grad_finalize_body<M>(slab, ngrid, dparams, b, pp);
    return;
  }
  if constexpr (M::HOIST) dy0_static_body<M>(g0buf, pack, dlatent, n_traj, n_times, dy0, b - Tail<M>::N_GF, tl);
}

template <int V_ = 0>
__global__ void ude_stats_finalize_kernel(double* __restrict__ slab, int ngrid, double n_eval,
                                          float* __restrict__ o_mean, float* __restrict__ o_std,
                                          float* __restrict__ o_norm) {
  // ... and the fp64 totals back into slab[0..4] (read by the data-parallel statistics exchange)
  // wave c sums statistic c: lane-strided partials, then a fixed butterfly (deterministic)
  __shared__ double tot[5];
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  if (wv < 5) {
    double s = 0.0;
    for (int gi = ln; gi < ngrid; gi += 64) s += slab[(size_t)gi * 5 + wv];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (ln == 0) tot[wv] = s;
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < 2) {
    const double m = tot[c] / n_eval;
    const double var = (tot[2 + c] - n_eval * m * m) / (n_eval - 1.0);
    if (o_mean) o_mean[c] = (float)m;
    if (o_std) o_std[c] = (float)sqrt(var > 0.0 ? var : 0.0);
  }
  if (c == 4 && o_norm) o_norm[0] = (float)sqrt(tot[4]);
  if (c < 5) slab[c] = tot[c];
}

}  // namespace ude
