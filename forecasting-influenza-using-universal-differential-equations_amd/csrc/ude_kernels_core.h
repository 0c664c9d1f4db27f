// What every RK4 kernel file builds on: static loops, the MFMA and barrier wrappers, the launch arguments,
// profiling stamps, DPP row sums, the schedule and packed-weight readers, checkpoint / stored-activation
// indexing, and the side statistics' publication (wave sums, publish_fence, finalize_stats_last).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include <type_traits>
#include "ude_model.h"
#include "ude_sir.h"

namespace ude {

typedef float f4 __attribute__((ext_vector_type(4)));

template <class Fn, int... I>
__device__ __forceinline__ void sfor_i(Fn&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class Fn>
__device__ __forceinline__ void sfor(Fn&& f) {
  sfor_i(f, std::make_integer_sequence<int, N>{});
}

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f4 f4zero() { f4 z = {0.f, 0.f, 0.f, 0.f}; return z; }

// Workgroup barrier for LDS hand-offs.  __syncthreads()'s workgroup-scope fence waits for every
// outstanding memory operation of the wave (s_waitcnt vmcnt(0)), so each barrier of the stage
// loop drained the prefetch loads issued a stage ahead (backward) and the checkpoint /
// activation-row stores (forward), exposing their HBM latency at every phase.  The RK4 kernels
// hand data between waves only through LDS (global results are read by later launches), so their
// barriers fence the LDS address space only: in-flight global loads and stores cross them.
__device__ __forceinline__ void lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

struct KArgs {
  const float* pack;
  const float* y0;
  const unsigned char* sched;
  float* latent;
  float* ckpt;
  double* stats_slab;
  const float* dlatent;
  // side statistics of the solve (backward: read) and their cotangents (nullable: zero)
  const float* st_mean;       // 2 floats: mean beta, mean gamma (posterior loc, lib/models.py:152-156)
  const float* st_std;        // 2 floats: unbiased std (posterior scale)
  const float* st_norm;       // 1 float: |Fa| (torch.norm(torch.stack(tracker)), lib/VAE.py:180)
  const float* d_mean;
  const float* d_std;
  const float* d_norm;
  float* dy0;
  float* slab;
  int n_traj, n_steps, n_out, n_tiles;
  float fa_w;
  unsigned long long* prof;   // diagnostic builds only (-DUDE_PROFILE): per-segment cycle sums
  float* g0buf;               // backward: per-trajectory layer-0 gradient sums [tile][K0][16]
  const float* eslab;         // BAYES backward: the eps stream in slab order, [eval][SLAB_TOTAL]
  const float* dlat_sir;      // backward: the compact S, I, R cotangent (T, N, R, 3) when dlatent is
                              // null (its dims >= 3 all zero); exactly one of the two is set
  const float* dec_pack;      // DEC forward: decoder fragments + bias (Model::DEC_PACK floats)
  float* yhat;                // DEC forward: (T, N, R) decoder outputs, written instead of the latent
  double* reg_slab;           // DEC forward: per-workgroup latent_init_loss partial sums
  float* ckpt_final;          // DEC training forward: the final-state block (ckpt + ckpt_final_off)
  float* gst;                 // GST backward: layer-output gradient rows [tile][step][stage][16][ACT_A4]
  // forward: the statistics finalised in the kernel by its last workgroup (finalize_stats_last)
  unsigned int* ctl;          // arrival counter, zero on entry, left zero; the host never passes null
                              // (Ops::launch_forward), fwd_body still tests it (see there)
  float* o_mean;              // 2 floats
  float* o_std;               // 2 floats
  float* o_norm;              // 1 float
  double* o_sums;             // 5 doubles: sum beta, sum gamma, sum beta^2, sum gamma^2, sum Fa^2 (nullable)
  float* o_reg;               // DEC: latent_init_loss (1 float)
  double n_eval;              // 4 n_steps N R: the number of recorded rates per statistic
  float* dyn;                 // DYN forward: (C, T, N, R) dynamics channels (dyn_channels<M>() of them)
  const float* scn;           // SCN forward: (n_steps, R, 2) multipliers of (beta, gamma) per step and region
};

// The channels of the DYN forward, in order: s, i, r; beta, gamma, r_eff (rate net); fa_s, fa_i, fa_r
// (augmentation net).  Channel c of output time j is the (N, R) block at ((c * T + j) * N) * R.
template <class M>
constexpr int dyn_channels() { return 3 + (M::HAS_P ? 3 : 0) + (M::HAS_A ? 3 : 0); }

// latent_init_loss summand (lib/train_functions.py:116-126): |x| where x < 0, |1 - x| where x > 1
__device__ __forceinline__ float reg_term(float v) {
  return (v < 0.f ? fabsf(v) : 0.f) + (v > 1.f ? fabsf(1.f - v) : 0.f);
}

// Timing ablations for a diagnostic build (-DUDE_ABL=n, tools/ablate.py): component n of the
// small-record backward is skipped (results are wrong; only the kernel time is read).
#ifndef UDE_ABL
#define UDE_ABL 0
#endif
// Measured-off A/B variants of rounds 3-5 (two interleaved accumulation chains, early activation-row
// stores, row-mapped latent outputs, raised critical-path priority; round 5: input-gradient fragments
// a phase earlier, interleaved static hoist, tail time sums with fewer round trips, forward copy-wave
// priority, more static-gradient chunks) were removed from the tree: profiles/r04/ab_*.log and
// profiles/r05/ab_*.txt hold their measurements.

// In-kernel cycle stamps for a diagnostic build (-DUDE_PROFILE): wave-uniform
// s_memtime deltas accumulated per segment; compiled out otherwise.
constexpr int NPROF = 28;
constexpr int PROF_FWD_SLOT = 4096;          // the training forward's rows start at workgroup slot 4096
struct Prof {
  unsigned long long acc[NPROF];
  unsigned long long last;
};
#ifdef UDE_PROFILE
#define UDE_STAMP(pf, seg)                                                    \
  do {                                                                        \
    if (pf) {                                                                 \
      __builtin_amdgcn_sched_barrier(0);                                      \
      const unsigned long long t_ = __builtin_amdgcn_s_memtime();             \
      __builtin_amdgcn_sched_barrier(0);                                      \
      (pf)->acc[seg] += t_ - (pf)->last;                                      \
      (pf)->last = t_;                                                        \
    }                                                                         \
  } while (0)
#else
#define UDE_STAMP(pf, seg) do { } while (0)
#endif

// Sum over the 16 lanes of a DPP row -- the 16 trajectories t = lane & 15 of a tile row -- by four
// DPP adds (quad_perm lane ^ 1, lane ^ 2, row_half_mirror, row_mirror): the association of the xor
// butterfly, so bitwise the same sums, without the LDS-crossbar ds_bpermute round trips of
// __shfl_xor (4 dependent LDS latencies per reduction).  Every lane of the row holds the sum.
// (state49 bwd 1.83 -> 1.72 ms, gradients bit-identical: profiles/r05/ab_dpp.txt)
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_mov<0xB1>(v);      // quad_perm [1, 0, 3, 2]
  v += dpp_mov<0x4E>(v);      // quad_perm [2, 3, 0, 1]
  v += dpp_mov<0x141>(v);     // row_half_mirror
  v += dpp_mov<0x140>(v);     // row_mirror
  return v;
}

// The step / output schedule (dt, the output CSR) is read every stage.  It is wave-uniform and
// read-only, so it is read through the constant address space: scalar loads (s_load, scalar
// cache) that count only in lgkmcnt.  A generic pointer compiled to FLAT loads, which count in
// vmcnt as well, so every schedule read waited for all of the wave's in-flight global stores
// (the forward's checkpoint and activation rows) and prefetch loads.
typedef const __attribute__((address_space(4))) float* SchedF;
typedef const __attribute__((address_space(4))) int* SchedI;
struct Sched {
  SchedF dt;
  SchedI out_start;
  SchedI out_j;
  SchedI out_mode;
  SchedF out_slope;
  __device__ Sched(const unsigned char* base, int n_steps, int n_out) {
    dt = (SchedF)base;
    out_start = (SchedI)(dt + n_steps);
    out_j = out_start + n_steps + 1;
    out_mode = out_j + n_out;
    out_slope = (SchedF)(out_mode + n_out);
  }
};

// Packed weights are read through a buffer resource (SGPR descriptor): every
// fragment load is `voffset = lane*16` + a compile-time scalar offset, so no
// per-tile 64-bit lane addresses are materialised (they were hoisted out of the
// step loop and spilled).
typedef __amdgpu_buffer_rsrc_t Rsrc;
__device__ __forceinline__ Rsrc make_rsrc(const float* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ f4 ldw(Rsrc rs, int voff_bytes, int soff_bytes) {
  return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff_bytes, soff_bytes, 0));
}

// SCN: the scenario's multipliers (m_beta, m_gamma) of region r in the step whose row starts row_bytes into
// the (n_steps, R, 2) table: one 8-byte load through a buffer resource (no 64-bit lane address).  The row
// offset is wave-uniform; the callers keep r < R and the row below n_steps (the table is 8-byte aligned:
// the host entry checks).
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 ld_scn(Rsrc rs, int r, int row_bytes) {
  return __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(rs, r * 8, row_bytes, 0));
}

__device__ __forceinline__ size_t ckpt_index(int tile, int n_steps, int step, int stage, int F, int f, int t) {
  return ((((size_t)tile * n_steps + step) * 4 + stage) * F + f) * TT + t;
}

// GST training forward: the tiles' static features ([tile][16][S16]) behind the stage checkpoints and
// stored rows (the weight-gradient GEMM's layer-0 input beside each stage's stored input).
template <class M>
__host__ __device__ __forceinline__ size_t gst_static_off(int n_tiles, int n_steps) {
  return (size_t)n_tiles * n_steps * 4 * (M::F * TT + (M::ACT_STORED ? TT * M::XST_W : 0));
}
// DEC training forward: the solve's final state y_{n_steps} ([tile][F][16]) behind the stage
// checkpoints, stored activations and (GST) static features, i.e. at ude_query's ckpt_bytes (the
// decoder backward reads every output state from there).
template <class M>
__host__ __device__ __forceinline__ size_t ckpt_final_off(int n_tiles, int n_steps) {
  return gst_static_off<M>(n_tiles, n_steps) + (M::GST ? (size_t)n_tiles * TT * M::S16 : 0);
}

// Stored activations (Model::ACT_STORED) of one tile-stage: [16][XST_W] behind the checkpoint.
template <class M>
__host__ __device__ __forceinline__ float* act_block(float* ckpt, int n_tiles, int n_steps, int tile, int step,
                                                     int stage) {
  const size_t ck = (size_t)n_tiles * n_steps * 4 * M::F * TT;
  return ckpt + ck + (((size_t)tile * n_steps + step) * 4 + stage) * TT * M::XST_W;
}
template <class M>
constexpr int act_q_per_thread() { return (TT * M::ACT_A4 / 4 + NTHREADS - 1) / NTHREADS; }
// Quad i of a tile-stage's activation rows ([16][ACT_A4] in record order, i = t * ACT_A4 / 4 + q)
// -> its quad index in the stored block ([16][XST_W], activation rows at column ACT_IN).
template <class M>
__host__ __device__ __forceinline__ int act_src_q(int i) {
  constexpr int QR = M::ACT_A4 / 4;
  if constexpr (M::XST_W == M::ACT_A4) return i;
  else return (i / QR) * (M::XST_W / 4) + M::ACT_IN / 4 + (i - (i / QR) * QR);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Fixed-order sum of one statistic's per-workgroup partials by one wave (lane-strided, then a fixed
// butterfly): the order of ude_stats_finalize_kernel (the dopri5 forward's finalize).  The partials are
// read with device-coherent loads (written by other workgroups, possibly on other XCDs, with
// device-coherent stores).
__device__ __forceinline__ double wave_sum_partials(const double* part, int n, int stride, int off, int ln) {
  double s = 0.0;
  for (int gi = ln; gi < n; gi += 64)
    s += __hip_atomic_load(part + (size_t)gi * stride + off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

// Statistics from the per-workgroup partials, by wave 0 of the last workgroup to arrive (ticket on
// A.ctl):
//   mean_c = S_c / n, std_c = sqrt((S2_c - n mean_c^2) / (n - 1)) (torch's unbiased std,
//   lib/models.py:152-156), |Fa| = sqrt(S_Fa) (lib/VAE.py:180); DEC: latent_init_loss.
// Publication without agent-scope fences: on gfx950 those write back / invalidate the whole L2 of the
// XCD (buffer_wbl2 / buffer_inv sc1), which at the end of a forward that has just written GBs of
// checkpoints cost 52 us per launch (measured).  Instead the partials go out as device-scope (sc1)
// stores, complete (s_waitcnt vmcnt(0)) before the ticket is taken, and the last workgroup reads them
// with device-scope loads: the device-coherent path, no cache maintenance.  The counter is reset for
// the next launch (stream ordered).
//
// Ordering argument (the atomics are relaxed: under the HIP/C++ memory model alone this pattern would
// be a data race, so it rests on gfx950's hardware ordering, made explicit here):
//  1. the partials are agent-scope (sc1) stores: written through to the device-coherent level, not
//     left in a non-coherent cache;
//  2. publish_fence(): s_waitcnt vmcnt(0) -- every store of the wave has been acknowledged (is visible
//     device-wide) -- plus a compiler barrier, so no memory operation is moved across it;
//  3. only then the ticket's agent-scope fetch_add (performed at the device-coherent level, after
//     step 2 in program order);
//  4. the last arrival, after its ticket came back and another compiler barrier, reads the partials
//     with agent-scope (sc1) loads, which are served from the device-coherent level.
// An acquire / release pair at agent scope would add an L2 write-back / invalidate of the XCD
// (buffer_wbl2 / buffer_inv sc1): 52 us at the end of a forward that has just written GBs.
__device__ __forceinline__ void publish_fence() {
  __builtin_amdgcn_s_waitcnt(0x0F70);              // vmcnt(0): this wave's stores are acknowledged
  __asm__ __volatile__("" ::: "memory");           // and the compiler keeps every access on its side
}

// OPT (the inference DEC forward): the latent_init_loss buffers are optional, null skips the term
template <bool DEC, bool OPT = false>
__device__ __forceinline__ void finalize_stats_last(const KArgs& A, int ln) {
  publish_fence();
  unsigned int ticket = 0;
  if (ln == 0) ticket = __hip_atomic_fetch_add(A.ctl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  ticket = __builtin_amdgcn_readfirstlane(ticket);
  if (ticket != gridDim.x - 1) return;
  __asm__ __volatile__("" ::: "memory");           // the partial loads stay behind the ticket
  const int ng = gridDim.x;
  double tot[5];
#pragma unroll
  for (int c = 0; c < 5; ++c) tot[c] = wave_sum_partials(A.stats_slab, ng, 5, c, ln);
  double reg = 0.0;
  const bool has_reg = DEC && (!OPT || (A.reg_slab && A.o_reg));
  if constexpr (DEC) {
    if (has_reg) reg = wave_sum_partials(A.reg_slab, ng, 1, 0, ln);
  }
  if (ln < 2) {
    const double n = A.n_eval, t0 = ln == 0 ? tot[0] : tot[1], t2 = ln == 0 ? tot[2] : tot[3];
    const double m = t0 / n;
    const double var = (t2 - n * m * m) / (n - 1.0);
    if (A.o_mean) A.o_mean[ln] = (float)m;
    if (A.o_std) A.o_std[ln] = (float)sqrt(var > 0.0 ? var : 0.0);
  }
  if (ln == 2 && A.o_norm) A.o_norm[0] = (float)sqrt(tot[4]);
  if (ln == 3 && has_reg) A.o_reg[0] = (float)reg;
  // o_sums may alias stats_slab[0..4], workgroup 0's partials (ude_rk4_forward / ude_rk4_forward_dec hand
  // the totals back there).  That is safe, and rests on this function's shape: one wave does all of it,
  // every other workgroup has stored its partials and left (its ticket is taken), and the value lane c
  // stores to o_sums[c] is tot[c], whose butterfly has consumed every lane's loads of statistic c --
  // stats_slab[c] among them, the only partial that store overwrites.  A finalize spread over several
  // waves, or one that re-read a partial after this store, would break it.
  if (A.o_sums && ln < 5) {
    double v = tot[0];
#pragma unroll
    for (int c = 1; c < 5; ++c) v = ln == c ? tot[c] : v;
    A.o_sums[ln] = v;
  }
  if (ln == 0) *A.ctl = 0u;
}

// The nets' final-layer outputs in a trajectory's record behind mlp_forward: the rate net's q at
// Q_OUT + 2 r (HAS_P) and the augmentation net's raw Fa at FA_OUT + 3 r (HAS_A), region r
template <class M> constexpr int Q_OUT = M::HAS_P ? M::act_off(0, M::nl(0) - 1) : 0;
template <class M> constexpr int FA_OUT = M::HAS_A ? M::act_off(1, M::nl(1) - 1) : 0;

}  // namespace ude
