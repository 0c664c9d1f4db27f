// The forward solve: tile starts, fwd_body (all four RK4 stages of every step, the training stores, the DEC
// and DYN epilogues, the SCN rate multipliers), fwd_sbody (the split forward's store waves) and ude_fwd_kernel.
#pragma once
#include "ude_kernels_mlp.h"

namespace ude {

// Forward tile start (L = 8), before the stage input: the record's static features from y0, CS loads in
// flight at a time, ahead of any global store of the tile (loads and stores count together in vmcnt, so a
// load issued behind pending stores waits for them to complete).
template <class M, int SR, int XOFF>
__device__ __forceinline__ void fwd_tile_static(const KArgs& A, float* lds, int n0) {
  // every load of the thread in flight at once (state49: 16; 4 at a time measured fwd 0.921 -> 0.909 ms
  // against this, profiles/r05/ab_tile_static.txt)
  constexpr int PS = (TT * M::S16 + NTHREADS - 1) / NTHREADS, CS = PS < 16 ? PS : 16;
  int tid = threadIdx.x;
  // thread-derived offsets formed here each tile, not hoisted into registers the stage loop needs
  asm volatile("" : "+v"(tid));
#pragma unroll
  for (int u0 = 0; u0 < PS; u0 += CS) {
    float sv[CS];
#pragma unroll
    for (int uu = 0; uu < CS; ++uu) {
      const int i = tid + (u0 + uu) * NTHREADS;
      const int t = i / M::S16, s = i - t * M::S16;
      const int n = n0 + t;
      float v = 0.f;
      if (u0 + uu < PS && i < TT * M::S16 && s < M::S && n < A.n_traj) {
        const int r = s / (M::L - 3), c = 3 + s - r * (M::L - 3);
        v = A.y0[((size_t)n * M::R + r) * M::L + c];
      }
      sv[uu] = v;
    }
#pragma unroll
    for (int uu = 0; uu < CS; ++uu) {
      const int i = tid + (u0 + uu) * NTHREADS;
      const int t = i / M::S16, s = i - t * M::S16;
      if (u0 + uu < PS && i < TT * M::S16) lds[t * SR + XOFF + s] = sv[uu];
    }
  }
}

// latent[0] and the static latent dims of every output time (zero derivative, carried unchanged:
// lib/models.py:144), from the record (stage input in the Y slot, static features at XOFF) after the
// tile-start barrier: stores only, row-mapped (consecutive lanes, consecutive 32-B (n, r) rows of the
// tile's contiguous (16, R, 8) latent block).  The per-output copy loop this replaces read y0 once per
// iteration behind its own pending stores (18% of the state49 training forward, tools/stage_profile.py).
template <class M, int SR, int XOFF>
__device__ __forceinline__ void fwd_tile_latent(const KArgs& A, const Sched& sc, const float* lds, int n0) {
  constexpr int NROW = TT * M::R, PR = (NROW + NTHREADS - 1) / NTHREADS;
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int nvalid = min(TT, A.n_traj - n0) * M::R;
  const size_t NRL = (size_t)A.n_traj * M::R * M::L;
  #pragma unroll 1
  for (int u = 0; u < PR; ++u) {
    const int i = tid + u * NTHREADS;
    if (i < nvalid) {
      const int t = i / M::R, r = i - t * M::R;
      const float* rec = lds + t * SR;
      const f4 lo = {rec[M::Y_OFF + 3 * r], rec[M::Y_OFF + 3 * r + 1], rec[M::Y_OFF + 3 * r + 2], rec[XOFF + 5 * r]};
      const f4 hi = {rec[XOFF + 5 * r + 1], rec[XOFF + 5 * r + 2], rec[XOFF + 5 * r + 3], rec[XOFF + 5 * r + 4]};
      const size_t row = ((size_t)n0 * M::R + i) * M::L;
      f4* d0 = reinterpret_cast<f4*>(A.latent + row);
      d0[0] = lo;
      d0[1] = hi;
      #pragma unroll 1
      for (int o = 0; o < A.n_out; ++o) {
        float* d = A.latent + (size_t)sc.out_j[o] * NRL + row;
        d[3] = lo[3];
        *reinterpret_cast<f4*>(d + 4) = hi;
      }
    }
  }
}

// The stage input in the record's Y slot ([16][F] at Y_OFF) -> its checkpoint block ([F][16]): lane
// (f, q) gathers trajectories 4q .. 4q + 3 of feature f (conflict-free LDS reads: consecutive lanes,
// consecutive banks) and writes them as one 16-B store; 64 lanes cover 1 KB of the block.
template <class M, int SR>
__device__ __forceinline__ void store_ckpt_rows(float* blk, const float* lds, int tid) {
  constexpr int NQ = M::F * (TT / 4), PER = (NQ + NTHREADS - 1) / NTHREADS;
  asm volatile("" : "+v"(tid));
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int i = tid + u * NTHREADS;
    if (i < NQ) {
      const int f = i >> 2, t0 = (i & 3) * 4;
      const f4 v = {lds[t0 * SR + M::Y_OFF + f], lds[(t0 + 1) * SR + M::Y_OFF + f],
                    lds[(t0 + 2) * SR + M::Y_OFF + f], lds[(t0 + 3) * SR + M::Y_OFF + f]};
      reinterpret_cast<f4*>(blk)[i] = v;
    }
  }
}

// How a forward variant's mlp_forward gets its streamed fragments (ude_kernels_mlp.h FS_*): resident weights
// (WREG, RES, PFB) and the models outside Model::PF_F stream as before; of the others every variant issues its
// loads in consumption order, and carries them a phase ahead where that compiles without scratch at two
// workgroups per CU (256 VGPRs).
template <class M, bool TRAIN, bool DEC, bool DYN, bool SCN, bool RESIDENT>
constexpr int fwd_stream_mode() {
  if (RESIDENT || !M::PF_F) return FS_PHASE;
  if (UDE_ABL == 17) return FS_ABL;
  // the training DEC forward with stored activations is at the limit already (state49: 249 VGPRs; 36 B of
  // scratch with the carry): consumption-order loads only
  if (TRAIN && DEC && M::ACT_STORED) return FS_ORDER;
  // phase 0 of the first owned net across the flux pass, the other net's at phase 0's head: all of phase 0
  // (FS_CARRY) spilled in every variant but the inference DEC ones (state49: 72 - 116 B of scratch)
  return FS_CARRY1;
}

// ============================================================================
// Forward solve
// ============================================================================
// DEC (decoder epilogue): instead of the (T, N, R, L) latent, every output time
// emits y_hat = W_dec . y[:3R] + b_dec ((T, N, R), the Decoder of lib/models.py:27-51 as
// lib/VAE.py:138 applies it) and the latent_init_loss sum over y[..., :3] (:189); the training
// forward also stores the final state for the decoder backward.  Outputs must be grid hits
// (schedule mode 1; the host checks).
// RES (deterministic weights too large for two workgroups' registers, launched when the tiles do not
// outnumber the CUs): one workgroup per CU with every forward fragment resident in VGPRs for the whole
// launch -- no phase waits on the L2 latency of its weights (the few-tile / strong-scaling shard case,
// where no second workgroup on the CU hides it).
// DYN (the inference DEC forward, deterministic weights): beside y_hat, every output time emits the
// dynamics channels of dyn_channels<M>() into A.dyn (C, T, N, R): the state S, I, R and the nets' outputs
// evaluated at that state -- beta, gamma (unmasked, as the reference appends them to `params`),
// r_eff = beta S / gamma, and the raw Fa (before Fa_w and the mask, as appended to `tracker`).  An output
// time that starts a step takes them from that step's stage 0, ahead of its flux pass (dyn_pass); the
// last output time ends the last step and has no evaluation of the solve, so one more mlp_forward runs
// on the final state and the same pass follows it: no RK update, no store but A.dyn, nothing added to
// the side statistics.
// SCN (the inference DEC forward of a deterministic model with a rate net): a scenario.  A.scn is a table
// (n_steps, R, 2) of multipliers; all four stage evaluations of step k scale the rate net's outputs of
// region r by row k -- beta' = |m[k][r][0] q0|, gamma' = |m[k][r][1] q1|, which for m >= 0 is fl(m |q|), so
// a table of ones gives the plain solve's bits -- before sir_flux; Fa, the mask and the RK update are
// unchanged, and the side statistics sum the scaled rates.  Per step, not per time: stage 4 of step k is
// evaluated at the start time of step k + 1 and still takes row k.  With DYN the channels report the scaled
// rates: an output that starts a step takes that step's row, the last output the last step's.
// Each thread's pairs keep their region from step to step: their multipliers (2 SLOTS registers) are loaded
// once per step ahead of stage 0's layers and held for its four flux passes, or at the head of every flux
// pass where the registers are not there (SCN_AHEAD below).
template <class M, bool TRAIN, int W, bool SPLIT = false, bool DEC = false, bool RES = false, bool DYN = false,
          bool SCN = false>
__device__ void fwd_body(const KArgs& A, float* lds) {
  static_assert(!DYN || (DEC && !TRAIN && !SPLIT && !M::BAYES), "DYN: the deterministic inference DEC forward only");
  static_assert(!SCN || (DEC && !TRAIN && !SPLIT && !M::BAYES && M::HAS_P),
                "SCN: the deterministic inference DEC forward of a model with a rate net only");
  constexpr int SR = M::SR_F;
  constexpr int SL = M::SLOTS;
  int tid = threadIdx.x;
  const int lane = tid & 63;
  const Sched sc(A.sched, A.n_steps, A.n_out);
  const size_t NRL = (size_t)A.n_traj * M::R * M::L;
  const Rsrc rs = make_rsrc(A.pack, M::PACK_TOTAL * 4);
  const Rsrc rsd = DEC ? make_rsrc(A.dec_pack, M::DEC_PACK * 4) : rs;
  constexpr int SCN_ROW = M::R * 8;              // bytes of one step's row of the scenario table
  // where the plain kernel streams its weights (!WREG) there is room to hold a step's multipliers of the
  // thread's pairs from ahead of stage 0's layers (state49 FaFp: 213 -> 221 VGPRs, no scratch; forecast_scn
  // 2.116 ms against 2.162 ms with the loads in the flux pass, forecast_dec 2.113 - 2.133); a model whose
  // fragments live in registers is at its limit (state49 Fp: 256 VGPRs and 32 B of scratch without SCN):
  // its loads go at the head of every flux pass (24 B of scratch; held across the step: 40 B)
  constexpr bool SCN_AHEAD = !M::WREG;
  const Rsrc rsm = SCN ? make_rsrc(A.scn, A.n_steps * SCN_ROW) : rs;
  double st_b = 0, st_g = 0, st_bb = 0, st_gg = 0, st_fa = 0;
  // DEC: this thread's latent_init_loss partial lives in LDS behind the record (the large models'
  // forward is at its 256-VGPR limit: two more live registers spilled)
  double* st_reg = reinterpret_cast<double*>(lds + M::REG_LDS_F) + tid;
  if constexpr (DEC) *st_reg = 0.0;

  // BAYES at small sizes (PFB): each evaluation's weight sample lives in registers, loaded while the
  // previous evaluation's flux pass runs (its L2 latency off the layer phases; at one tile per CU
  // nothing else on the CU hides it)
  constexpr bool PFB = M::FWD_PFB;
  WRegs<M, W, false, true, RES || PFB> wr;
  if constexpr (!PFB) wr.load(rs, lane);
  // Streamed fragments (Model::PF_F, weights not resident): issued in the MFMAs' consumption order and, in the
  // variants with the registers for it, carried a phase ahead (FS_CARRY / FS_CARRY1): phase 0's (state49: 20
  // quads a wave, or the first net's 10) are issued after each stage's last layer barrier, ahead of the
  // activation-row copy and the flux pass, whose stores are all younger in vmcnt, so the next stage's first
  // MFMA waits for neither an L2 round trip nor those stores; phases 1.. are issued by the phase before
  // (mlp_forward).  The loads issued at a tile's last stage serve the next tile's first (the weights are the
  // launch's; a workgroup's last issue is never read).  No explicit wait count is needed: the loads and their
  // first use share the stage loop's body, and the compiler's count at phase 0's first MFMA allows for the
  // stores and loads issued since (state49 training forward: vmcnt(24); tools/spill_check.py's assembly).
  // Which variant carries how much is fwd_stream_mode's (registers: profiles/r07/spill_check_r49.txt).
  constexpr int FSM = fwd_stream_mode<M, TRAIN, DEC, DYN, SCN, decltype(wr)::ON>();
  constexpr bool CARRY = FSM == FS_CARRY || FSM == FS_CARRY1;
  f4 fsf[(CARRY && M::WF_Q(W) > 0) ? M::WF_Q(W) : 1], fsb[(CARRY && M::WB_Q(W) > 0) ? M::WB_Q(W) : 1];
  auto issue_d0 = [&]() {
    if constexpr (CARRY) {
      load_phase_frags<M, W, 0, carry0_nets<M, W, FSM>()>(rs, lane, fsf, fsb);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  if constexpr (FSM == FS_ABL) {
    fsf[0] = ldw(rs, lane * 16, 0);
    __builtin_amdgcn_s_waitcnt(0x0F70);
  }
  Prof prof_, *pf = nullptr;
#ifdef UDE_PROFILE
  if (TRAIN && A.prof && tid == 0) {
    pf = &prof_;
    for (int i = 0; i < NPROF; ++i) prof_.acc[i] = 0;
    prof_.last = __builtin_amdgcn_s_memtime();
  }
#endif

  #pragma unroll 1
  for (int i = tid; i < TT * SR; i += NTHREADS) lds[i] = 0.f;
  lds_sync();
  issue_d0();                                     // the first tile's first stage

  for (int tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    const int n0 = tile * TT;
    // The RK4 state and the 3/8-rule combinations are carried in fp64 (the stage evaluations stay fp32:
    // every stage input is rounded to fp32 for the MLPs, the checkpoint and the masks).  The reference's
    // torchdiffeq combination runs in fp32; on trajectories that pass next to the mask boundary of
    // lib/models.py:130 its rounding is amplified ~1e5-fold (whole-batch weight
    // gradients of the M1 FaFp batch 5x outside the fp32 oracle's spread); an fp64 state brings those
    // trajectories 2-50x closer to fp64 (tools/ns_traj.py, "fp32 rhs / fp64 state") at 3 extra VGPRs per
    // state slot and a few fp64 VALU operations per stage.
    double ys[SL][3];
    float k1[SL][3], k2[SL][3], k3[SL][3];
    // DEC: y_hat of output jo from the state in the record's Y slot (decoder row tiles over the
    // waves; no barrier: the next write of the Y slot is behind the next stage's layer barriers)
    auto dec_emit = [&](int jo) {
      if constexpr (DEC) {
        const int t = lane & 15, g = lane >> 4;
        sfor<M::RTD>([&](auto kk) {
          constexpr int k = decltype(kk)::value;
          if constexpr (k % WAVES == W) {
            f4 acc = ldw(rsd, g * 16, (M::DEC_WF + k * 16) * 4);
            acc = gemm_tile_lean<M::F16, k * (M::F16 / 16) * 256, 2>(rsd, lds + t * SR + M::Y_OFF, lane, acc);
            const int n = n0 + t;
            if (n < A.n_traj) {
              float* dst = A.yhat + ((size_t)jo * A.n_traj + n) * M::R + k * 16 + 4 * g;
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (k * 16 + 4 * g + e < M::R) dst[e] = acc[e];
            }
          }
        });
      }
    };

    // DYN: the channels of output jo, from the record of a finished mlp_forward whose Y slot still holds
    // the evaluated state.  A pass of its own over the thread's (trajectory, region) pairs, run between the
    // layers' last barrier and the flux pass, when nothing of the flux pass is live: each thread reads and
    // the flux pass then rewrites only its own pairs' Y slots, so no barrier separates the two.  Not a hot
    // path (one stage in four, nine stores per pair): a rolled loop whose thread-derived addresses are
    // formed here per use, not hoisted into registers the stage loop needs (at R = 49 the plain kernel is
    // close to its 256 VGPRs).  4-B stores at stride R across the tile's trajectories, as the latent
    // stores of the models without 16-B rows.
    auto dyn_pass = [&](int jo, [[maybe_unused]] int row) {
      if constexpr (DYN) {
        int td = threadIdx.x;
        asm volatile("" : "+v"(td));
        const size_t NR = (size_t)A.n_traj * M::R, CS = (size_t)(A.n_out + 1) * NR;
        #pragma unroll 1
        for (int p = td; p < M::PAIRS; p += NTHREADS) {
          const int r = p / TT, t = p - r * TT;
          const int n = n0 + t;
          if (n < A.n_traj) {
            const float* rec = lds + t * SR;
            float* dst = A.dyn + (size_t)jo * NR + (size_t)n * M::R + r;
            const float s = rec[M::Y_OFF + 3 * r];
            dst[0] = s;
            dst[CS] = rec[M::Y_OFF + 3 * r + 1];
            dst[2 * CS] = rec[M::Y_OFF + 3 * r + 2];
            if constexpr (M::HAS_P) {
              float b, gm;
              if constexpr (SCN) {
                const f2 m = ld_scn(rsm, r, row * SCN_ROW);
                sir_rates(m[0] * rec[Q_OUT<M> + 2 * r], m[1] * rec[Q_OUT<M> + 2 * r + 1], b, gm);
              } else {
                sir_rates(rec[Q_OUT<M> + 2 * r], rec[Q_OUT<M> + 2 * r + 1], b, gm);
              }
              dst[3 * CS] = b;
              dst[4 * CS] = gm;
              dst[5 * CS] = sir_r_eff(b, s, gm);
            }
            if constexpr (M::HAS_A) {
              constexpr int c0 = M::HAS_P ? 6 : 3;
#pragma unroll
              for (int c = 0; c < 3; ++c) dst[(c0 + c) * CS] = rec[FA_OUT<M> + 3 * r + c];
            }
          }
        }
      }
    };

    // the row-mapped tile start (fwd_tile_static / fwd_tile_latent; L = 8: 16-B latent rows, checked by
    // the host entry)
    constexpr bool rows16 = M::L == 8;
    // large records: each stage's checkpointed input written as 16-B rows from the Y slot behind phase 0's
    // weight loads (state49 fwd 0.945 -> 0.925 ms); small records keep three 4-B stores per (trajectory,
    // region) in the flux pass (rows cost M1 2%; profiles/r04/ab_ck_*.log)
    constexpr bool CKR = SL > 1;
    if constexpr (rows16) fwd_tile_static<M, SR, M::XSF_OFF>(A, lds, n0);
    // y0 -> registers, LDS Y slot, latent[0], ckpt(step 0, stage 0)
    sfor<SL>([&](auto ss) {
      constexpr int sl = decltype(ss)::value;
      const int p = tid + sl * NTHREADS;
      if (p < M::PAIRS) {
        const int r = p / TT, t = p - r * TT;
        const int n = n0 + t;
        const bool valid = n < A.n_traj;
        const float* src = A.y0 + ((size_t)n * M::R + r) * M::L;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float y = valid ? src[c] : 0.f;
          ys[sl][c] = (double)y;
          lds[t * SR + M::Y_OFF + 3 * r + c] = y;
          if (TRAIN && !CKR && A.n_steps > 0) A.ckpt[ckpt_index(tile, A.n_steps, 0, 0, M::F, 3 * r + c, t)] = y;
          if (DEC && valid) *st_reg += (double)reg_term(y);
        }
        if (valid && !DEC && !rows16) {
          float* dst = A.latent + ((size_t)n * M::R + r) * M::L;
          for (int c = 0; c < M::L; ++c) dst[c] = src[c];
        }
      }
    });
    // static latent dims (zero derivative, carried unchanged: lib/models.py:144) of every output
    // time, once per tile (not in the step loop, where each copy waited on a global load)
    if constexpr (M::L > 3 && !DEC && !rows16) {
      #pragma unroll 1
      for (int i = tid; i < A.n_out * M::PAIRS; i += NTHREADS) {
        const int o = i / M::PAIRS, p = i - o * M::PAIRS;
        const int r = p / TT, t = p - r * TT, n = n0 + t;
        if (n < A.n_traj) {
          const float* src = A.y0 + ((size_t)n * M::R + r) * M::L;
          float* dst = A.latent + (size_t)sc.out_j[o] * NRL + ((size_t)n * M::R + r) * M::L;
#pragma unroll
          for (int c = 3; c < M::L; ++c) dst[c] = src[c];
        }
      }
    }
    if constexpr (!rows16) load_static<M, SR, M::XSF_OFF>(A.y0, lds, n0, A.n_traj);
    lds_sync();
    if constexpr (TRAIN && M::GST) {
      // the tile's static features once ([tile][16][S16] behind the stored rows): the weight-gradient
      // GEMM's layer-0 input beside each stage's stored input
      f4* dst = reinterpret_cast<f4*>(A.ckpt + gst_static_off<M>(A.n_tiles, A.n_steps) + (size_t)tile * TT * M::S16);
      constexpr int QS = M::S16 / 4;
      #pragma unroll 1
      for (int i = tid; i < TT * QS; i += NTHREADS) {
        const int t = i / QS, q = i - t * QS;
        dst[i] = *reinterpret_cast<const f4*>(lds + t * SR + M::XSF_OFF + 4 * q);
      }
    }
    f4 c1[M::NZ(W) > 0 ? M::NZ(W) : 1];
    static_hoist<M, W, SR, M::XSF_OFF>(rs, lds, c1, lane);
    if constexpr (rows16 && !DEC) fwd_tile_latent<M, SR, M::XSF_OFF>(A, sc, lds, n0);
    lds_sync();                                   // the static features (aliased by the activations) are dead
    if constexpr (DEC) dec_emit(0);               // output 0 = y0
    UDE_STAMP(pf, 15);

    for (int step = 0; step < A.n_steps; ++step) {
      // DEC (R=49, at the 256-VGPR limit): the thread-derived 64-bit store addresses are recomputed
      // each step rather than hoisted out of the loop and spilled (each reload waited on every
      // checkpoint / activation store in flight)
      if constexpr (DEC) asm volatile("" : "+v"(tid));
      const float dt = sc.dt[step];
      // DYN: the output time this step starts on (0 = y0, or the grid-hit output that ended the previous
      // step), -1 when it starts between outputs
      int dyn_jo = -1;
      if constexpr (DYN) {
        if (step == 0) dyn_jo = 0;
        else if (sc.out_start[step - 1] < sc.out_start[step]) dyn_jo = sc.out_j[sc.out_start[step - 1]];
      }
      // SCN: this step's multipliers of the thread's pairs, in flight under stage 0's layers ...
      [[maybe_unused]] f2 mq[SL];
      if constexpr (SCN && SCN_AHEAD) {
        sfor<SL>([&](auto ss) {
          constexpr int sl = decltype(ss)::value;
          const int p = tid + sl * NTHREADS;
          mq[sl] = ld_scn(rsm, min(p / TT, M::R - 1), step * SCN_ROW);      // p >= PAIRS: a valid row entry, unused
        });
      }
      for (int j = 0; j < 4; ++j) {
        // BAYES: evaluation 4 step + j has its own weight sample
        Rsrc rse = rs;
        if constexpr (M::BAYES) rse = make_rsrc(A.pack + (size_t)(4 * step + j) * M::PACK_TOTAL, M::PACK_TOTAL * 4);
        if constexpr (PFB) {
          if (step == 0 && j == 0) wr.load(rse, lane, false);        // the tile's first evaluation
        }
        // this stage's input (the record's Y slot, layer 0's input) -> its checkpoint, issued behind
        // phase 0's weight loads (their waits then do not wait for these stores) and read before
        // the phase's barrier (the flux pass overwrites the slot after the last phase)
        mlp_forward<M, W, SR>(rse, lds, c1, lane, wr, pf, [&](auto dd) {
          if constexpr (decltype(dd)::value == 0) {
            if constexpr (TRAIN && CKR)
              store_ckpt_rows<M, SR>(A.ckpt + ckpt_index(tile, A.n_steps, step, j, M::F, 0, 0), lds, tid);
          }
        }, std::integral_constant<int, FSM>{}, fsf, fsb);
        issue_d0();                                // the next stage's phase 0 (FS_CARRY), ahead of every store below
        if constexpr (PFB) {
          const int en = 4 * step + j + 1;
          if (en < 4 * A.n_steps) wr.load(make_rsrc(A.pack + (size_t)en * M::PACK_TOTAL, M::PACK_TOTAL * 4), lane, false);
        }
        if constexpr (TRAIN && M::ACT_STORED && !SPLIT && UDE_ABL != 11) {
          // this stage's activation rows -> HBM for the backward (read before the flux barrier;
          // the stores drain behind the rest of the stage)
          f4* dst = reinterpret_cast<f4*>(act_block<M>(A.ckpt, A.n_tiles, A.n_steps, tile, step, j));
          constexpr int QR = M::ACT_A4 / 4, NQ = act_q_per_thread<M>();
          // all of a thread's LDS reads, then all its 16-B stores (state49 fwd 0.936 -> 0.892 ms against
          // batches of 3 quads, profiles/r04/ab_uc_*.log: the phases' registers are free by then)
          constexpr int UC = NQ <= 5 ? NQ : cmin(NQ, 16);
          #pragma unroll 1
          for (int u0 = 0; u0 < NQ; u0 += UC) {
#pragma unroll
            for (int uu = 0; uu < UC; ++uu) {
              const int i = tid + (u0 + uu) * NTHREADS;
              if (u0 + uu < NQ && i < TT * QR) {
                const int t = i / QR, q = i - t * QR;
                dst[act_src_q<M>(i)] = *reinterpret_cast<const f4*>(lds + t * SR + M::ACT0 + 4 * q);
              }
            }
          }
        }
        UDE_STAMP(pf, 0);
        if constexpr (DYN) {
          if (j == 0 && dyn_jo >= 0) dyn_pass(dyn_jo, step);
        }
        if constexpr (SCN && !SCN_AHEAD) {                   // ... or loaded here, every stage
          sfor<SL>([&](auto ss) {
            constexpr int sl = decltype(ss)::value;
            const int p = tid + sl * NTHREADS;
            mq[sl] = ld_scn(rsm, min(p / TT, M::R - 1), step * SCN_ROW);
          });
        }
        if constexpr (UDE_ABL != 12) sfor<SL>([&](auto ss) {
          constexpr int sl = decltype(ss)::value;
          const int p = tid + sl * NTHREADS;
          if (p < M::PAIRS) {
            const int r = p / TT, t = p - r * TT;
            const int n = n0 + t;
            const bool valid = n < A.n_traj;
            float* rec = lds + t * SR;
            float Y[3], f[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) Y[c] = rec[M::Y_OFF + 3 * r + c];
            if constexpr (TRAIN && M::GST) {
              // the stage input in front of the stored activation rows (the layer-0 input of the
              // weight-gradient GEMM); its pad columns [F, F16) zeroed by the last region's threads
              float* xrow = act_block<M>(A.ckpt, A.n_tiles, A.n_steps, tile, step, j) + t * M::XST_W;
#pragma unroll
              for (int c = 0; c < 3; ++c) xrow[3 * r + c] = Y[c];
              if (r == M::R - 1)
                for (int c = M::F; c < M::F16; ++c) xrow[c] = 0.f;
            }
            if constexpr (M::HAS_P) {
              float b, gm;
              if constexpr (SCN)
                sir_flux(Y[0], Y[1], mq[sl][0] * rec[Q_OUT<M> + 2 * r], mq[sl][1] * rec[Q_OUT<M> + 2 * r + 1], f, b, gm);
              else
                sir_flux(Y[0], Y[1], rec[Q_OUT<M> + 2 * r], rec[Q_OUT<M> + 2 * r + 1], f, b, gm);
              if (valid && UDE_ABL != 14) {
                st_b += (double)b; st_g += (double)gm;
                st_bb += (double)b * (double)b; st_gg += (double)gm * (double)gm;
              }
            }
            if constexpr (M::HAS_A) {
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                const float fa = rec[FA_OUT<M> + 3 * r + c];
                sir_add_fa<M::HAS_P>(f[c], A.fa_w, fa);
                if (valid && UDE_ABL != 14) st_fa += (double)fa * (double)fa;
              }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = sir_masked(Y[c]) ? 0.f : f[c];
            float Yn[3];
            const double dd = (double)dt;
            if (j == 0) {
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                k1[sl][c] = f[c];
                Yn[c] = (float)(ys[sl][c] + (dd * (double)f[c]) * (1.0 / 3.0));
              }
            } else if (j == 1) {
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                k2[sl][c] = f[c];
                Yn[c] = (float)(ys[sl][c] + dd * ((double)f[c] - (double)k1[sl][c] * (1.0 / 3.0)));
              }
            } else if (j == 2) {
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                k3[sl][c] = f[c];
                Yn[c] = (float)(ys[sl][c] + dd * (((double)k1[sl][c] - (double)k2[sl][c]) + (double)f[c]));
              }
            } else {
              float yold[3];
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                yold[c] = (float)ys[sl][c];
                const double dy =
                    ((((double)k1[sl][c] + 3.0 * ((double)k2[sl][c] + (double)k3[sl][c])) + (double)f[c]) * dd) * 0.125;
                ys[sl][c] = ys[sl][c] + dy;
                Yn[c] = (float)ys[sl][c];
              }
              if constexpr (DEC) {
                // every output is a grid hit (mode 1): latent_init_loss of the new state; y_hat
                // follows from the record after the barrier (dec_emit)
                if (valid && sc.out_start[step] < sc.out_start[step + 1]) {
#pragma unroll
                  for (int c = 0; c < 3; ++c) *st_reg += (double)reg_term(Yn[c]);
                }
                if (TRAIN && step == A.n_steps - 1) {
#pragma unroll
                  for (int c = 0; c < 3; ++c) A.ckpt_final[((size_t)tile * M::F + 3 * r + c) * TT + t] = Yn[c];
                }
              } else if (valid && UDE_ABL != 16) {
                const int o_end = sc.out_start[step + 1];
                #pragma unroll 1
                for (int o = sc.out_start[step]; o < o_end; ++o) {
                  const int jo = sc.out_j[o], mode = sc.out_mode[o];
                  const float slope = sc.out_slope[o];
                  float* dst = A.latent + (size_t)jo * NRL + ((size_t)n * M::R + r) * M::L;
                  float v[3];
#pragma unroll
                  for (int c = 0; c < 3; ++c) {
                    if (mode == 0) v[c] = yold[c];
                    else if (mode == 1) v[c] = Yn[c];
                    else v[c] = yold[c] + slope * (Yn[c] - yold[c]);
                  }
                  if constexpr (rows16) {
                    // 16-B aligned 32-B rows (host entry check): one 12-byte store per (trajectory,
                    // region) instead of three (the stores' issue was 4.6% of the state49 forward)
                    __builtin_memcpy(__builtin_assume_aligned(dst, 16), v, 12);
                  } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) dst[c] = v[c];
                  }
                }
              }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) rec[M::Y_OFF + 3 * r + c] = Yn[c];
            if (TRAIN) {
              const int ns = j == 3 ? step + 1 : step;
              const int nj = j == 3 ? 0 : j + 1;
              if (!CKR && ns < A.n_steps && UDE_ABL != 15) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                  A.ckpt[ckpt_index(tile, A.n_steps, ns, nj, M::F, 3 * r + c, t)] = Yn[c];
              }
            }
          }
        });
        UDE_STAMP(pf, 16);
        lds_sync();
        UDE_STAMP(pf, 1);
      }
      if constexpr (DEC) {
        if (sc.out_start[step] < sc.out_start[step + 1]) dec_emit(sc.out_j[sc.out_start[step]]);
      }
    }
    if constexpr (DYN) {
      // the last output time: the nets at the final state.  The Y slot is only read (dec_emit of that
      // output may still be reading it); the barrier at the end keeps the next tile's start (static
      // features over the activation rows, the Y slot) behind this pass's reads.  The condition is the
      // schedule's: uniform over the workgroup.
      const int last = A.n_steps - 1;
      if (sc.out_start[last] < sc.out_start[last + 1]) {
        const int jo = sc.out_j[sc.out_start[last]];
        mlp_forward<M, W, SR>(rs, lds, c1, lane, wr, pf, NoHook{}, std::integral_constant<int, FSM>{}, fsf, fsb);
        issue_d0();                              // FS_CARRY: this call consumed the next tile's
        dyn_pass(jo, last);                      // SCN: the last step's row
        lds_sync();
      }
    }
  }

  // deterministic per-workgroup partial sums
  constexpr int NS = DEC ? 6 : 5;
  double* red = reinterpret_cast<double*>(lds);
  double v[6] = {wave_sum(st_b), wave_sum(st_g), wave_sum(st_bb), wave_sum(st_gg), wave_sum(st_fa),
                 DEC ? wave_sum(*st_reg) : 0.0};
  lds_sync();
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < NS; ++c) red[(tid >> 6) * NS + c] = v[c];
  }
  lds_sync();
  // the inference DEC forward (!TRAIN): latent_init_loss is optional (null reg_slab: skipped)
  if (tid < NS && (TRAIN || tid < 5 || A.reg_slab)) {
    double s = 0;
    for (int w = 0; w < WAVES; ++w) s += red[w * NS + tid];
    double* dst = tid < 5 ? A.stats_slab + (size_t)blockIdx.x * 5 + tid : A.reg_slab + blockIdx.x;
    // device-coherent store, read back by the last workgroup (see finalize_stats_last)
    // A.ctl is never null; the two tests of it here only keep the kernel's register allocation as measured
    if (A.ctl) __hip_atomic_store(dst, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *dst = s;
  }
  // the last workgroup to finish turns every workgroup's partials into the statistics (no separate
  // finalize launch; wave 0 only, so the split forward's partner waves keep their barrier sequence)
  if (A.ctl && tid < 64) finalize_stats_last<DEC, DEC && !TRAIN>(A, tid);
#ifdef UDE_PROFILE
  if (pf) for (int i = 0; i < NPROF; ++i) A.prof[(size_t)blockIdx.x * NPROF + i] = prof_.acc[i];
#endif
}

// Training forward of small records (Model::split_fwd): waves 4-7 store each stage's activation
// rows (the backward's input) from the record to HBM while waves 0-3 run the flux pass; the same
// barrier sequence as fwd_body.
template <class M, bool DEC>
__device__ void fwd_sbody(const KArgs& A, float* lds) {
  constexpr int SR = M::SR_F;
  constexpr int QR = M::ACT_A4 / 4, NQ = act_q_per_thread<M>();
  const int wt = threadIdx.x - NTHREADS;
  lds_sync();                                  // record zeroed
  for (int tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    lds_sync();                                // tile inputs in the record
    lds_sync();                                // static hoist
    for (int step = 0; step < A.n_steps; ++step) {
      #pragma unroll 1
      for (int j = 0; j < 4; ++j) {
        sfor<M::D>([&](auto) { lds_sync(); }); // the MLP phases
        f4* dst = reinterpret_cast<f4*>(act_block<M>(A.ckpt, A.n_tiles, A.n_steps, tile, step, j));
        f4 v[NQ];
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          const int i = wt + u * NTHREADS;
          if (i < TT * QR) {
            const int t = i / QR, q = i - t * QR;
            v[u] = *reinterpret_cast<const f4*>(lds + t * SR + M::ACT0 + 4 * q);
          }
        }
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          const int i = wt + u * NTHREADS;
          if (i < TT * QR) dst[act_src_q<M>(i)] = v[u];
        }
        lds_sync();                            // flux pass (the next stage rewrites the rows)
      }
    }
  }
  lds_sync();                                  // side-statistic reduction
  lds_sync();
}

// SPLIT (training, Model::split_fwd, launched when every tile has a CU of its own): 8 waves.
// DEC: the decoder epilogue (y_hat and latent_init_loss, no latent).
// DYN: the dynamics channels beside y_hat (the deterministic inference DEC forward only; see fwd_body).
// SCN: a scenario table scales the rates per step and region (the same forward only; see fwd_body).
template <class M, bool TRAIN, bool SPLIT = false, bool DEC = false, bool RES = false, bool DYN = false,
          bool SCN = false>
__global__ __launch_bounds__(SPLIT ? 2 * NTHREADS : NTHREADS, (SPLIT || RES) ? 1 : 2) void ude_fwd_kernel(KArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if constexpr (SPLIT) {
    if (w >= WAVES) { fwd_sbody<M, DEC>(a, lds); return; }
  }
  if (w == 0) fwd_body<M, TRAIN, 0, SPLIT, DEC, RES, DYN, SCN>(a, lds);
  else if (w == 1) fwd_body<M, TRAIN, 1, SPLIT, DEC, RES, DYN, SCN>(a, lds);
  else if (w == 2) fwd_body<M, TRAIN, 2, SPLIT, DEC, RES, DYN, SCN>(a, lds);
  else fwd_body<M, TRAIN, 3, SPLIT, DEC, RES, DYN, SCN>(a, lds);
}

}  // namespace ude
