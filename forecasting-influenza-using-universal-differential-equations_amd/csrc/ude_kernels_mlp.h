// The MLP layer machinery on v_mfma_f32_16x16x4_f32: GEMM tiles, register-resident weights (WRegs),
// mlp_forward, the static-feature hoist, mlp_backward, and the partner waves' weight-gradient phases
// (mlp_backward_dw, mlp_backward_dw_l with its LDS-DMA helpers).
#pragma once
#include "ude_kernels_core.h"

namespace ude {

// One 16-row tile of  C[o][t] += sum_k A[o][k] * B[t][k]  with K = KP (multiple of 16).
// A: packed fragments at float offset WOFF of the pack ([KP/16][64][4] for this tile);
// B: the per-trajectory LDS record, lane group g reading features [g*KP/4, (g+1)*KP/4).
template <int KP, int WOFF>
__device__ __forceinline__ f4 gemm_tile(Rsrc rs, const float* bp, int lane, f4 acc) {
  constexpr int KQ = KP / 4;
  constexpr int NQ = KP / 16;
  const float* b = bp + (lane >> 4) * KQ;
  // every A fragment of the tile is issued before the first MFMA (the scheduler
  // otherwise serialises load -> wait -> 4 MFMAs, paying the L2 latency per quad)
  f4 a[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) a[q] = ldw(rs, lane * 16, (WOFF + q * 256) * 4);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const f4 x = *reinterpret_cast<const f4*>(b + 4 * q);
    acc = mfma4(a[q][0], x[0], acc);
    acc = mfma4(a[q][1], x[1], acc);
    acc = mfma4(a[q][2], x[2], acc);
    acc = mfma4(a[q][3], x[3], acc);
  }
  return acc;
}

// As gemm_tile with the A fragments in flight QC quads at a time (4 QC VGPRs): for a GEMM outside
// the stage loop's critical path in a kernel at its register limit (the DEC forward's decoder).
template <int KP, int WOFF, int QC>
__device__ __forceinline__ f4 gemm_tile_lean(Rsrc rs, const float* bp, int lane, f4 acc) {
  constexpr int KQ = KP / 4, NQ = KP / 16;
  const float* b = bp + (lane >> 4) * KQ;
#pragma unroll
  for (int q0 = 0; q0 < NQ; q0 += QC) {
    f4 a[QC];
#pragma unroll
    for (int q = 0; q < QC; ++q)
      if (q0 + q < NQ) a[q] = ldw(rs, lane * 16, (WOFF + (q0 + q) * 256) * 4);
#pragma unroll
    for (int q = 0; q < QC; ++q) {
      if (q0 + q < NQ) {
        const f4 x = *reinterpret_cast<const f4*>(b + 4 * (q0 + q));
        acc = mfma4(a[q][0], x[0], acc);
        acc = mfma4(a[q][1], x[1], acc);
        acc = mfma4(a[q][2], x[2], acc);
        acc = mfma4(a[q][3], x[3], acc);
      }
    }
  }
  return acc;
}

// Split form: issue a tile's fragments into a caller array (so several tiles, or a
// whole phase, can be in flight before the first MFMA), then run the MFMA chain.
template <int KP, int WOFF>
__device__ __forceinline__ void load_frags(Rsrc rs, int lane, f4* fr) {
#pragma unroll
  for (int q = 0; q < KP / 16; ++q) fr[q] = ldw(rs, lane * 16, (WOFF + q * 256) * 4);
}
template <int KP>
__device__ __forceinline__ f4 mma_frags(const f4* fr, const float* bp, int lane, f4 acc) {
  constexpr int KQ = KP / 4;
  const float* b = bp + (lane >> 4) * KQ;
#pragma unroll
  for (int q = 0; q < KP / 16; ++q) {
    const f4 x = *reinterpret_cast<const f4*>(b + 4 * q);
    acc = mfma4(fr[q][0], x[0], acc);
    acc = mfma4(fr[q][1], x[1], acc);
    acc = mfma4(fr[q][2], x[2], acc);
    acc = mfma4(fr[q][3], x[3], acc);
  }
  return acc;
}

// ELU (alpha 1).  expm1 is evaluated unconditionally on min(x, 0) and selected,
// so the compiler emits straight-line code instead of a divergent branch per value.
// (libm expm1f: torch's expm1-grade accuracy; the adaptive dopri5 step control is
// sensitive to the last bits of the RHS, measured: a 1-ulp-of-1 exp2 variant moves its
// evaluation points enough to shift the side statistics by 2e-3.)
__device__ __forceinline__ float elu1(float x) {
  const float e = expm1f(fminf(x, 0.f));
  return x > 0.f ? x : e;
}

template <class M, int NZ_>
using C1Arr = f4[NZ_ > 0 ? NZ_ : 1];

// Input-gradient (dX) fragments of wave W at depth d: [XQ(W, d)] quads in tile order.
template <class M, int W, int d>
__device__ __forceinline__ void load_x_frags(Rsrc rs, int lane, f4* fx) {
  if constexpr (d == 0 && M::SPLITX0) {
    // wave W's K quads qq = W (mod WAVES) of every layer-0 input tile m (merged nets, P first)
    constexpr int PQ = M::HAS_P ? M::kout(0, 0) / 16 : 0;
    sfor<M::XT(0)>([&](auto mm) {
      constexpr int m = decltype(mm)::value;
      sfor<M::x0q_w(W)>([&](auto jj) {
        constexpr int j = decltype(jj)::value, qq = W + j * WAVES;
        constexpr int net = qq < PQ ? 0 : 1, q = qq < PQ ? qq : qq - PQ;
        fx[m * M::x0q_w(W) + j] =
            ldw(rs, lane * 16, (M::wt_off(net, 0) + m * (M::kout(net, 0) / 16) * 256 + q * 256) * 4);
      });
    });
    return;
  }
  sfor<M::XT(d)>([&](auto mm) {
    constexpr int m = decltype(mm)::value;
    if constexpr (M::xowner(d, m) == W) {
      constexpr int q0 = M::xq_before(W, d, m);
      if constexpr (d == 0) {
        if constexpr (M::HAS_P)
          load_frags<M::kout(0, 0), M::wt_off(0, 0) + m * (M::kout(0, 0) / 16) * 256>(rs, lane, fx + q0);
        if constexpr (M::HAS_A)
          load_frags<M::kout(1, 0), M::wt_off(1, 0) + m * (M::kout(1, 0) / 16) * 256>(
              rs, lane, fx + q0 + (M::HAS_P ? M::kout(0, 0) / 16 : 0));
      } else {
        constexpr int net = M::xnet(d, m), rt = M::xrt(d, m);
        load_frags<M::kout(net, d), M::wt_off(net, d) + rt * (M::kout(net, d) / 16) * 256>(rs, lane, fx + q0);
      }
    }
  });
}

// Layer 0 of a record with at most 4 dynamic features (R = 1: S, I, R) and the static ones hoisted: every
// K step but the first multiplies padding, so the phase runs ONE MFMA per output tile with lane (o, g)
// holding W[o][g] and feature g instead of KP / 4 -- the same non-zero products added in the same order
// (the padded steps add exact zeros), so bitwise the same layer output.  With packo below: M1 FaFp step
// 7.50 -> 7.34 ms, gradients bitwise equal (profiles/r06/ab_pack_r1/).
template <class M>
constexpr bool pack0() { return M::HOIST && M::F <= 4 && M::F16 == 16; }
// ... for the waves that own at least two layer-0 tiles: with one tile per wave (Fp [32, 32]) the packed
// phase measured 1% slower (fwd 1.507 -> 1.522 ms, profiles/r06/ab_pack_r1/ab_fp32_4way.txt)
template <class M, int W>
constexpr bool pack0_w() { return pack0<M>() && M::NZ(W) >= 2; }
// The same for the input gradient of an output layer with at most 4 outputs (R = 1: the 2 rates, the 3
// Fa components): K = the 16-padded outputs, one MFMA per input tile with lane (h, g) holding W[g][h]
// and dZ[g] (register-resident weights only: the packed values are formed once per launch).
template <class M>
constexpr bool packo(int net, int d) {
  return M::has(net, d) && d > 0 && d == M::nl(net) - 1 && M::kout(net, d) == 16 && M::out_dim(net, d) <= 4;
}

// Register-resident weights (Model::WREG): every fragment / bias quad wave W reads in the
// forward (and, BWD, the input-gradient fragments), loaded once per launch.
struct NoWRegs {
  static constexpr bool ON = false;
  f4 wf[1], wb[1], wx[1];
};
template <class M, int W, bool BWD, bool NEED_F_ = !BWD || !M::ACT_STORED, bool FORCE = false>
struct WRegs {
  static constexpr bool ON = M::WREG || FORCE;
  static constexpr bool NEED_F = NEED_F_;   // a stored-activation RK4 backward never runs the forward
  static constexpr int NF = (ON && NEED_F) ? M::WF_Q(W) : 0, NB = (ON && NEED_F) ? M::WB_Q(W) : 0;
  static constexpr int NX = (ON && BWD) ? M::WX_Q(W) : 0;
  static constexpr int NP0 = (ON && NEED_F && pack0_w<M, W>()) ? M::NZ(W) : 0;
  // packo: the wave's output-layer input-gradient tiles in (d, m) order
  static constexpr int po_index(int d, int m) {
    int c = 0;
    for (int e = 0; e < M::D; ++e)
      for (int j = 0; j < M::XT(e); ++j) {
        if (e == d && j == m) return c;
        if (M::xowner(e, j) == W && packo<M>(M::xnet(e, j), e)) ++c;
      }
    return c;
  }
  static constexpr int NPO = (ON && BWD) ? po_index(M::D, 0) : 0;
  f4 wf[NF > 0 ? NF : 1], wb[NB > 0 ? NB : 1], wx[NX > 0 ? NX : 1];
  float w0[NP0 > 0 ? NP0 : 1];              // pack0: lane (o, g)'s layer-0 weight W[o][g]
  float wo[NPO > 0 ? NPO : 1];              // packo: lane (h, g)'s output-layer weight W[g][h]
  __device__ __forceinline__ void load(Rsrc rs, int lane, bool wait = true) {
    if constexpr (ON) {
      const int g = lane >> 4;
      sfor<M::D>([&](auto dd) {
        constexpr int d = decltype(dd)::value;
        if constexpr (NEED_F) sfor<M::FT(d)>([&](auto kk) {
          constexpr int k = decltype(kk)::value;
          if constexpr (M::fowner(d, k) == W) {
            constexpr int net = M::fnet(d, k), rt = M::frt(d, k), KP = M::kin(net, d);
            load_frags<KP, M::wf_off(net, d) + rt * (KP / 16) * 256>(rs, lane,
                                                                     wf + M::fq_base(W, d) + M::fq_before(W, d, k));
            if constexpr (M::has_bias(d))
              wb[M::nb_base(W, d) + M::nb_before(W, d, k)] = ldw(rs, g * 16, (M::b_off(net, d) + rt * 16) * 4);
          }
        });
        if constexpr (BWD) load_x_frags<M, W, d>(rs, lane, wx + M::xq_base(W, d));
      });
      // wait for the fragments here, once: the loop-carried wait analysis otherwise keeps them
      // "pending" at the step loop's head and puts a vmcnt(0) before the first MFMA of every
      // stage, which also drains the loads prefetched a stage ahead (s_waitcnt vmcnt(0))
      if (wait) __builtin_amdgcn_s_waitcnt(0x0F70);
      if constexpr (NP0 > 0) {
        // lane (o, g) takes element g of lane (o, 0)'s fragment quad (W[o][0..3]), once per launch
        sfor<M::FT(0)>([&](auto kk) {
          constexpr int k = decltype(kk)::value;
          if constexpr (M::fowner(0, k) == W) {
            const f4 q = wf[M::fq_base(W, 0) + M::fq_before(W, 0, k)];
            const int src = lane & 15;
            const float v0 = __shfl(q[0], src, 64), v1 = __shfl(q[1], src, 64);
            const float v2 = __shfl(q[2], src, 64), v3 = __shfl(q[3], src, 64);
            w0[M::nz_before(W, k)] = g == 0 ? v0 : (g == 1 ? v1 : (g == 2 ? v2 : v3));
          }
        });
      }
      if constexpr (NPO > 0) {
        sfor<M::D>([&](auto dd) {
          constexpr int d = decltype(dd)::value;
          if constexpr (d > 0) sfor<M::XT(d)>([&](auto mm) {
            constexpr int m = decltype(mm)::value;
            if constexpr (M::xowner(d, m) == W && packo<M>(M::xnet(d, m), d)) {
              // K = 16 outputs: one quad per tile, lane (h, g) holds W[4 g + e][h]
              const f4 q = wx[M::xq_base(W, d) + M::xq_before(W, d, m)];
              const int src = lane & 15;
              const float v0 = __shfl(q[0], src, 64), v1 = __shfl(q[1], src, 64);
              const float v2 = __shfl(q[2], src, 64), v3 = __shfl(q[3], src, 64);
              wo[po_index(d, m)] = g == 0 ? v0 : (g == 1 ? v1 : (g == 2 ? v2 : v3));
            }
          });
        });
      }
    }
  }
};

// Forward pass of both MLPs for the stage input held in the record's Y slot.
// Leaves post-activation outputs of every layer in the record (the final
// layers' raw outputs: P-net pre-|.| rates q, A-net Fa).  Ends on a barrier.
struct NoHook {
  template <class D>
  __device__ __forceinline__ void operator()(D) const {}
};

// Phase d's streamed forward fragments and bias quads of wave W, issued in the order the phase's MFMAs
// consume them (per net: the owned tiles' bias quads, then K quad by K quad across the tiles that share
// the B operand), so the first MFMA of the phase waits for the first load only.  fr: [FQ(W, d)] at
// fq_before(W, d, k) + q; bs: [nb_phase(W, d)] at nb_before(W, d, k).  NETS: bit n set = net n's tiles.
template <class M, int W, int d, int NETS = 3>
__device__ __forceinline__ void load_phase_frags(Rsrc rs, int lane, f4* fr, f4* bs) {
  const int g = lane >> 4;
  sfor<2>([&](auto nn) {
    constexpr int net = decltype(nn)::value;
    if constexpr (M::owns_f(W, d, net) && ((NETS >> net) & 1)) {
      constexpr int NQ = M::kin(net, d) / 16;
      if constexpr (M::has_bias(d))
        sfor<M::FT(d)>([&](auto kk) {
          constexpr int k = decltype(kk)::value;
          if constexpr (M::fowner(d, k) == W && M::fnet(d, k) == net)
            bs[M::nb_before(W, d, k)] = ldw(rs, g * 16, (M::b_off(net, d) + M::frt(d, k) * 16) * 4);
        });
      sfor<NQ>([&](auto qq) {
        constexpr int q = decltype(qq)::value;
        sfor<M::FT(d)>([&](auto kk) {
          constexpr int k = decltype(kk)::value;
          if constexpr (M::fowner(d, k) == W && M::fnet(d, k) == net)
            fr[M::fq_before(W, d, k) + q] =
                ldw(rs, lane * 16, (M::wf_off(net, d) + M::frt(d, k) * NQ * 256 + q * 256) * 4);
        });
      });
    }
  });
}

// How mlp_forward gets the fragments it streams from L2 (weights not register-resident):
//   FS_PHASE  each phase issues its own at its head, tile by tile, and its MFMAs wait for them;
//   FS_ORDER  the same, issued in the MFMAs' consumption order (load_phase_frags);
//   FS_CARRY  (Model::PF_F) every phase finds its fragments in flight: they live in the caller's arrays
//             (`fsf` [WF_Q(W)], `fsb` [WB_Q(W)], WRegs' layout), the caller issues phase 0's ahead of the call
//             and phase d issues phase d + 1's;
//   FS_CARRY1 as FS_CARRY, but of phase 0 the caller issues only the tiles of the first net the wave owns
//             (carry0_nets) and phase 0 the other net's at its head: half the registers across the caller's
//             code, and the second net's MFMAs start a whole net's chain after their loads;
//   FS_ABL    timing ablation (UDE_ABL 17): every fragment and bias quad is fsf[0], nothing is loaded.
enum : int { FS_PHASE = 0, FS_ORDER = 1, FS_CARRY = 2, FS_ABL = 3, FS_CARRY1 = 4 };
// the nets (bit mask) whose phase-0 tiles of wave W the caller issues ahead of mlp_forward
template <class M, int W, int FSM>
constexpr int carry0_nets() {
  if (FSM == FS_CARRY) return 3;
  if (FSM == FS_CARRY1) return M::owns_f(W, 0, 0) ? 1 : 2;
  return 0;
}

// One phase of mlp_forward in the FS_ORDER / FS_CARRY / FS_ABL modes (see there), up to its barrier.
template <class M, int W, int SR, int d, int FSM, class Hook>
__device__ __forceinline__ void mlp_forward_phase_fs(Rsrc rs, float* rec, const f4* c1, int lane, const Hook& hook,
                                                     f4* fsf, f4* fsb) {
  constexpr int NF = M::FQ(W, d), NB = M::nb_phase(W, d);
  static_assert(NF <= 24 && !(d == 0 && pack0_w<M, W>()), "Model::PF_F: no chunked and no packed layer 0");
  const int g = lane >> 4;
  constexpr bool CARRY = FSM == FS_CARRY || FSM == FS_CARRY1, OWN = FSM == FS_ORDER;
  f4 frl[(OWN && NF > 0) ? NF : 1], bsl[(OWN && NB > 0) ? NB : 1];
  const f4* fr = CARRY ? fsf + M::fq_base(W, d) : frl;
  const f4* bs = CARRY ? fsb + M::nb_base(W, d) : bsl;
  if constexpr (OWN) load_phase_frags<M, W, d>(rs, lane, frl, bsl);
  // FS_CARRY: the next phase's fragments go out at this phase's head, next to this phase's own (in flight
  // since the phase before).  Phase 0 carries the most (state49: 20 quads), so phase 1's are issued
  // inside it, once the first net's MFMAs have freed that net's fragments -- where a wave owns tiles of both
  // nets; else behind the phase's MFMAs.
  constexpr bool NEXT = CARRY && d + 1 < M::D;
  constexpr bool MID0 = d == 0 && M::owns_f(W, 0, 0) && M::owns_f(W, 0, 1);
  auto issue_next = [&]() {
    if constexpr (NEXT) load_phase_frags<M, W, (NEXT ? d + 1 : d)>(rs, lane, fsf + M::fq_base(W, d + 1),
                                                                  fsb + M::nb_base(W, d + 1));
  };
  if constexpr (d > 0) issue_next();
  if constexpr (d == 0 && CARRY) load_phase_frags<M, W, 0, 3 & ~carry0_nets<M, W, FSM>()>(rs, lane, fsf, fsb);
  if constexpr (!(CARRY && MID0)) hook(std::integral_constant<int, d>{});
  __builtin_amdgcn_sched_barrier(0);
  auto FR = [&](int i) -> f4 {
    if constexpr (FSM == FS_ABL) return fsf[0];
    else return fr[i];
  };
  f4 acc[M::FT(d) > 0 ? M::FT(d) : 1];
  sfor<M::FT(d)>([&](auto kk) {
    constexpr int k = decltype(kk)::value;
    if constexpr (M::fowner(d, k) == W) {
      if constexpr (d == 0 && M::HOIST) acc[k] = c1[M::nz_before(W, k)];
      else if constexpr (FSM == FS_ABL) acc[k] = fsf[0];
      else acc[k] = bs[M::nb_before(W, d, k)];
    }
  });
  // as mlp_forward: the wave's tiles of one net share the B operand, read QB quads ahead of their MFMAs
  sfor<2>([&](auto nn) {
    constexpr int net = decltype(nn)::value;
    if constexpr (M::owns_f(W, d, net)) {
      constexpr int KP = M::kin(net, d);
      constexpr int inoff = d == 0 ? M::Y_OFF : M::act_off(net, d - 1);
      const float* b = rec + inoff + g * (KP / 4);
      constexpr int NQ = KP / 16, QB = 5;
#pragma unroll
      for (int q0 = 0; q0 < NQ; q0 += QB) {
        f4 xb[QB];
#pragma unroll
        for (int q = q0; q < q0 + QB && q < NQ; ++q) xb[q - q0] = *reinterpret_cast<const f4*>(b + 4 * q);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = q0; q < q0 + QB && q < NQ; ++q) {
          const f4 x = xb[q - q0];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            sfor<M::FT(d)>([&](auto kk) {
              constexpr int k = decltype(kk)::value;
              if constexpr (M::fowner(d, k) == W && M::fnet(d, k) == net) {
                const f4 wq = FR(M::fq_before(W, d, k) + q);
                if constexpr (UDE_ABL == 13) acc[k][e] += x[e];
                else acc[k] = mfma4(wq[e], x[e], acc[k]);
              }
            });
        }
      }
      if constexpr (CARRY && MID0 && net == 0) {
        // the stage-input checkpoint rows still go out behind the loads (see fwd_body)
        __builtin_amdgcn_sched_barrier(0);
        issue_next();
        hook(std::integral_constant<int, d>{});
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  });
  if constexpr (d == 0 && !MID0) {
    __builtin_amdgcn_sched_barrier(0);
    issue_next();
    __builtin_amdgcn_sched_barrier(0);
  }
  sfor<M::FT(d)>([&](auto kk) {
    constexpr int k = decltype(kk)::value;
    if constexpr (M::fowner(d, k) == W) {
      constexpr int net = M::fnet(d, k), rt = M::frt(d, k);
      f4 a = acc[k];
      if constexpr (M::act(net, d)) {
        a[0] = elu1(a[0]); a[1] = elu1(a[1]);
        a[2] = elu1(a[2]); a[3] = elu1(a[3]);
      }
      *reinterpret_cast<f4*>(rec + M::act_off(net, d) + rt * 16 + g * 4) = a;
    }
  });
}

// `hook(integral_constant<d>)` runs right after phase d's weight loads are issued
// (used by the backward to start HBM loads early without holding registers long).
template <class M, int W, int SR, class WR = NoWRegs, class Hook = NoHook, int FSM = FS_PHASE>
__device__ __forceinline__ void mlp_forward(Rsrc rs, float* lds, const f4* c1, int lane, const WR& wr = WR{},
                                            Prof* pf = nullptr, const Hook& hook = Hook{},
                                            std::integral_constant<int, FSM> = {}, f4* fsf = nullptr,
                                            f4* fsb = nullptr) {
  constexpr bool RW = WR::ON;
  static_assert(FSM == FS_PHASE || !RW, "resident fragments are not streamed");
  const int t = lane & 15, g = lane >> 4;
  float* rec = lds + t * SR;
  sfor<M::D>([&](auto dd) {
    constexpr int d = decltype(dd)::value;
    constexpr int NF = M::FQ(W, d);
    if constexpr (FSM != FS_PHASE) {
      mlp_forward_phase_fs<M, W, SR, d, FSM>(rs, rec, c1, lane, hook, fsf, fsb);
      lds_sync();
      UDE_STAMP(pf, 2 + d);
      return;
    }
    // all of this wave's weight fragments (and biases) for the phase are in flight
    // before its first MFMA -- unless they would not fit next to the working set (the Bayesian
    // state model's layer 0, K = 416: 208 VGPRs, spilled at the forward's 256): then chunk by chunk
    constexpr bool CHUNK_A = !RW && NF > 24;
    constexpr bool P0 = d == 0 && pack0_w<M, W>();
    f4 fr[(NF > 0 && !RW && !CHUNK_A) ? NF : 1], bias[(M::FT(d) > 0 && !RW) ? M::FT(d) : 1];
    float w0s[(P0 && !RW && M::NZ(W) > 0) ? M::NZ(W) : 1];
    if constexpr (!RW) {
      sfor<M::FT(d)>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        if constexpr (M::fowner(d, k) == W) {
          constexpr int net = M::fnet(d, k), rt = M::frt(d, k), KP = M::kin(net, d);
          if constexpr (P0) {
            // W[o][g]: element g of lane (o, 0)'s fragment quad
            w0s[M::nz_before(W, k)] = __builtin_bit_cast(
                float, __builtin_amdgcn_raw_buffer_load_b32(rs, ((lane & 15) * 4 + g) * 4,
                                                            (M::wf_off(net, d) + rt * (KP / 16) * 256) * 4, 0));
          } else if constexpr (!CHUNK_A) {
            load_frags<KP, M::wf_off(net, d) + rt * (KP / 16) * 256>(rs, lane, fr + M::fq_before(W, d, k));
          }
          if constexpr (M::has_bias(d)) bias[k] = ldw(rs, g * 16, (M::b_off(net, d) + rt * 16) * 4);
        }
      });
    }
    auto FR = [&](int i) -> f4 {
      if constexpr (RW) return wr.wf[M::fq_base(W, d) + i];
      else return fr[i];
    };
    hook(dd);
    __builtin_amdgcn_sched_barrier(0);
    f4 acc[M::FT(d) > 0 ? M::FT(d) : 1];
    sfor<M::FT(d)>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      if constexpr (M::fowner(d, k) == W) {
        if constexpr (d == 0 && M::HOIST) acc[k] = c1[M::nz_before(W, k)];
        else if constexpr (RW) acc[k] = wr.wb[M::nb_base(W, d) + M::nb_before(W, d, k)];
        else acc[k] = bias[k];
      }
    });
    if constexpr (P0) {
      // pack0: one MFMA per owned tile, lane (t, g) supplies feature g of trajectory t
      const float xg = g < M::F ? rec[M::Y_OFF + g] : 0.f;
      sfor<M::FT(d)>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        if constexpr (M::fowner(d, k) == W) {
          float wv;
          if constexpr (RW) wv = wr.w0[M::nz_before(W, k)];
          else wv = w0s[M::nz_before(W, k)];
          acc[k] = mfma4(wv, xg, acc[k]);
        }
      });
    }
    // the wave's tiles of one net share the B operand (the layer input): one LDS
    // read feeds every tile, and consecutive MFMAs go to different accumulators
    if constexpr (!P0) sfor<2>([&](auto nn) {
      constexpr int net = decltype(nn)::value;
      if constexpr (M::owns_f(W, d, net)) {
        constexpr int KP = M::kin(net, d);
        constexpr int inoff = d == 0 ? M::Y_OFF : M::act_off(net, d - 1);
        const float* b = rec + inoff + g * (KP / 4);
        // B quads are read in chunks of QB ahead of their MFMAs (one LDS wait per chunk)
        constexpr int NQ = KP / 16, QB = CHUNK_A ? 4 : 5;
        // CHUNK_A: the chunks' weight fragments double-buffered, chunk c + 1's loads in flight
        // during chunk c's MFMAs (fully unrolled: the buffer index is a constant)
        f4 fa[2][CHUNK_A ? M::FT(d) : 1][CHUNK_A ? QB : 1];
        auto load_chunk = [&](int bsel, int c0) {
          if constexpr (CHUNK_A)
            sfor<M::FT(d)>([&](auto kk) {
              constexpr int k = decltype(kk)::value;
              if constexpr (M::fowner(d, k) == W && M::fnet(d, k) == net) {
                constexpr int rt = M::frt(d, k);
#pragma unroll
                for (int q = c0; q < c0 + QB && q < NQ; ++q)
                  fa[bsel][k][q - c0] = ldw(rs, lane * 16, (M::wf_off(net, d) + rt * NQ * 256 + q * 256) * 4);
              }
            });
        };
        load_chunk(0, 0);
#pragma unroll
        for (int q0 = 0; q0 < NQ; q0 += QB) {
          f4 xb[QB];
          const int cb = (q0 / QB) & 1;
          if (q0 + QB < NQ) load_chunk(cb ^ 1, q0 + QB);
#pragma unroll
          for (int q = q0; q < q0 + QB && q < NQ; ++q) xb[q - q0] = *reinterpret_cast<const f4*>(b + 4 * q);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int q = q0; q < q0 + QB && q < NQ; ++q) {
            const f4 x = xb[q - q0];
#pragma unroll
            for (int e = 0; e < 4; ++e)
              sfor<M::FT(d)>([&](auto kk) {
                constexpr int k = decltype(kk)::value;
                if constexpr (M::fowner(d, k) == W && M::fnet(d, k) == net) {
                  f4 wq;
                  if constexpr (CHUNK_A) wq = fa[cb][CHUNK_A ? k : 0][CHUNK_A ? q - q0 : 0];
                  else wq = FR(M::fq_before(W, d, k) + q);
                  if constexpr (UDE_ABL == 13) acc[k][e] += x[e];
                  else acc[k] = mfma4(wq[e], x[e], acc[k]);
                }
              });
          }
        }
      }
    });
    sfor<M::FT(d)>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      if constexpr (M::fowner(d, k) == W) {
        constexpr int net = M::fnet(d, k), rt = M::frt(d, k);
        f4 a = acc[k];
        if constexpr (M::act(net, d)) {
          a[0] = elu1(a[0]); a[1] = elu1(a[1]);
          a[2] = elu1(a[2]); a[3] = elu1(a[3]);
        }
        *reinterpret_cast<f4*>(rec + M::act_off(net, d) + rt * 16 + g * 4) = a;
      }
    });
    lds_sync();
    UDE_STAMP(pf, 2 + d);
  });
}

// Static-feature hoist: c1[o][t] = b0[o] + sum_s W0[o][static s] * x_static[t][s].
template <class M, int W, int SR, int XOFF>
__device__ __forceinline__ void static_hoist(Rsrc rs, const float* lds, f4* c1, int lane) {
  if constexpr (M::HOIST) {
    const int t = lane & 15, g = lane >> 4;
    sfor<M::FT(0)>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      if constexpr (M::fowner(0, k) == W) {
        constexpr int net = M::fnet(0, k);
        constexpr int rt = M::frt(0, k);
        f4 acc = ldw(rs, g * 16, (M::b_off(net, 0) + rt * 16) * 4);
        acc = gemm_tile<M::S16, M::wsf_off(net) + rt * (M::S16 / 16) * 256>(rs, lds + t * SR + XOFF, lane, acc);
        c1[M::nz_before(W, k)] = acc;
      }
    });
    __builtin_amdgcn_s_waitcnt(0x0F70);   // once per tile (see WRegs::load)
  }
}

// Load the tile's static features (latent dims >= 3 of y0) into the record.
template <class M, int SR, int XOFF>
__device__ __forceinline__ void load_static(const float* __restrict__ y0, float* lds, int n0, int n_traj) {
  if constexpr (M::S > 0) {
    #pragma unroll 1
    for (int i = threadIdx.x; i < TT * M::S16; i += NTHREADS) {
      const int t = i / M::S16, s = i - t * M::S16;
      const int n = n0 + t;
      float v = 0.f;
      if (s < M::S && n < n_traj) {
        const int r = s / (M::L - 3), c = 3 + s - r * (M::L - 3);
        v = y0[((size_t)n * M::R + r) * M::L + c];
      }
      lds[t * SR + XOFF + s] = v;
    }
  }
}

// BAYES: `es` addresses this evaluation's eps in slab order; every tile's dW
// contribution of the evaluation is also accumulated eps-weighted into `dws` (and the
// bias row sums into DBS): d|std| = sum_eval eps_eval * dW_eval (models_bayes.py:45-46).
// DX_ONLY (SPLIT_BWD critical-path waves): only the input gradients; the weight gradients of
// the phase are the partner waves' (mlp_backward_dw).
// GST: the wave's owned rows of every layer-output gradient also go to `gblk` (this tile-stage's
// [16][ACT_A4] block, record column order) for ude_gst_dw_kernel.
// GST (no weight-gradient work, registers to spare): the input-gradient fragments come from `fxp`
// ([WX_Q(W)] quads, phase d at xq_base(W, d)), each phase's loaded while the previous phase runs
// (the caller issues the first phase's before the flux pass), so no phase waits on the L2 latency.
template <class M, int W, int SR, bool DX_ONLY = false, bool PFX = false, class DW, class DS, class G0, class EP0,
          class WR>
__device__ __forceinline__ void mlp_backward(Rsrc rs, Rsrc es, float* lds, DW& dw, DS& dws, G0& g0t, int lane,
                                             Prof* pf, const EP0& ep0, const WR& wr, float* gblk = nullptr,
                                             f4* fxp = nullptr) {
  constexpr bool RW = WR::ON;
  constexpr bool PF = PFX && !RW;     // only the RK4 backward (bwd_body) hands over the fxp array
  const int t = lane & 15, g = lane >> 4;
  float* rec = lds + t * SR;
  sfor<M::D>([&](auto ee) {
    constexpr int d = M::D - 1 - decltype(ee)::value;
    UDE_STAMP(pf, 24 + d);
    // input-gradient fragments go out first; the LDS-only dW GEMMs below hide them
    constexpr int NX = M::XQ(W, d);
    f4 fx[(NX > 0 && !RW && !PF) ? NX : 1];
    if constexpr (!RW && !PF) load_x_frags<M, W, d>(rs, lane, fx);
    auto FX = [&](int i) -> f4 {
      if constexpr (RW) return wr.wx[M::xq_base(W, d) + i];
      else if constexpr (PF) return fxp[M::xq_base(W, d) + i];
      else return fx[i];
    };
    // BAYES: this evaluation's eps for the wave's dW tiles (C layout) and bias rows
    constexpr int NE = (M::BAYES && !DX_ONLY) ? M::ndw_phase(W, d) : 0;
    f4 ef[NE > 0 ? NE : 1], eb[M::FT(d) > 0 ? M::FT(d) : 1];
    if constexpr (M::BAYES && !DX_ONLY) {
      sfor<M::FT(d)>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        if constexpr (M::fowner(d, k) == W) {
          constexpr int e0 = M::ndw_before(W, d, k) - M::ndw_before(W, d, 0);
          sfor<M::rti(M::fnet(d, k), d)>([&](auto cc) {
            constexpr int ct = decltype(cc)::value;
            ef[e0 + ct] = ldw(es, lane * 16, (M::dyn_tiles_before(d, k) + ct) * 1024);
          });
          eb[k] = ldw(es, g * 16, (M::SLAB_DB + (M::FTbase(d) + k) * 16) * 4);
        }
      });
    }
    __builtin_amdgcn_sched_barrier(0);
    // (1) rows owned by this wave: bias/G sums and the dW GEMM (K = trajectories).
    // When they fit, every owned tile's LDS operands are read before the first MFMA
    // (one LDS latency per phase instead of one per tile).
    constexpr int NOWN = M::own_phase(W, d);
    constexpr int NDP = M::ndw_phase(W, d);
    constexpr bool BATCH = !DX_ONLY && !M::BAYES && NOWN > 0 && 4 * NOWN * 2 + 4 * NDP <= 96;
    if constexpr (BATCH) {
      f4 gvv[NOWN];
      float gaa[NOWN][4], bva[NDP][4];
      sfor<M::FT(d)>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        if constexpr (M::fowner(d, k) == W) {
          constexpr int net = M::fnet(d, k), rt = M::frt(d, k), goff = M::gbuf(net, d);
          constexpr int inoff = d == 0 ? M::Y_OFF : M::act_off(net, d - 1);
          constexpr int o = M::ng_before(W, d, k) - M::ng_before(W, d, 0);
          constexpr int e0 = M::ndw_before(W, d, k) - M::ndw_before(W, d, 0);
          gvv[o] = *reinterpret_cast<const f4*>(rec + goff + rt * 16 + g * 4);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            gaa[o][s] = lds[(4 * g + s) * SR + goff + rt * 16 + t];
            sfor<M::rti(net, d)>([&](auto cc) {
              constexpr int ct = decltype(cc)::value;
              bva[e0 + ct][s] = lds[(4 * g + s) * SR + inoff + ct * 16 + t];
            });
          }
        }
      });
      __builtin_amdgcn_sched_barrier(0);
      sfor<M::FT(d)>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        if constexpr (M::fowner(d, k) == W) {
          constexpr int net = M::fnet(d, k);
          constexpr int o = M::ng_before(W, d, k) - M::ng_before(W, d, 0);
          constexpr int e0 = M::ndw_before(W, d, k) - M::ndw_before(W, d, 0);
#pragma unroll
          for (int s = 0; s < 4; ++s)
            sfor<M::rti(net, d)>([&](auto cc) {
              constexpr int ct = decltype(cc)::value;
              constexpr int idx = M::ndw_before(W, d, k) + ct;
              dw[idx] = mfma4(gaa[o][s], bva[e0 + ct][s], dw[idx]);
            });
          if constexpr (d == 0) {
            g0t[M::nz_before(W, k)] += gvv[o];
          } else {
            f4 r = gvv[o];
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = row16_sum(r[e]);
            if (t == 0) {
              float* db = lds + M::DB_LDS + (M::FTbase(d) + k) * 16 + g * 4;
              db[0] += r[0]; db[1] += r[1]; db[2] += r[2]; db[3] += r[3];
            }
          }
        }
      });
      __builtin_amdgcn_sched_barrier(0);
    } else if constexpr (!DX_ONLY)
    sfor<M::FT(d)>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      if constexpr (M::fowner(d, k) == W) {
        constexpr int net = M::fnet(d, k);
        constexpr int rt = M::frt(d, k);
        constexpr int goff = M::gbuf(net, d);
        constexpr int inoff = d == 0 ? M::Y_OFF : M::act_off(net, d - 1);
        const f4 gv = *reinterpret_cast<const f4*>(rec + goff + rt * 16 + g * 4);
        if constexpr (d == 0 && !M::BAYES) {
          g0t[M::nz_before(W, k)] += gv;          // per-trajectory sums: static-feature gradients
        } else {
          // bias gradient: sum over the tile's 16 trajectories, then into this
          // wave's rows of the workgroup's LDS row sums (fixed order: deterministic)
          f4 r = gv;
#pragma unroll
          for (int e = 0; e < 4; ++e) r[e] = row16_sum(r[e]);
          if (t == 0) {
            float* db = lds + M::DB_LDS + (M::FTbase(d) + k) * 16 + g * 4;
            db[0] += r[0]; db[1] += r[1]; db[2] += r[2]; db[3] += r[3];
            if constexpr (M::BAYES) {
              float* dbs = lds + M::DBS_LDS + (M::FTbase(d) + k) * 16 + g * 4;
              const f4 e = eb[k];
              dbs[0] += r[0] * e[0]; dbs[1] += r[1] * e[1]; dbs[2] += r[2] * e[2]; dbs[3] += r[3] * e[3];
            }
          }
        }
        // all of the tile's LDS operands are read before its first MFMA: one LDS
        // latency per tile instead of one per MFMA pair
        constexpr int NC = M::rti(net, d);
        float ga[4], bv[4][NC];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          ga[s] = lds[(4 * g + s) * SR + goff + rt * 16 + t];
#pragma unroll
          for (int ct = 0; ct < NC; ++ct) bv[s][ct] = lds[(4 * g + s) * SR + inoff + ct * 16 + t];
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (M::BAYES) {
          // this evaluation's tile contribution on its own, then into both sums
          f4 tmp[NC];
          sfor<NC>([&](auto cc) { tmp[decltype(cc)::value] = f4zero(); });
#pragma unroll
          for (int s = 0; s < 4; ++s)
            sfor<NC>([&](auto cc) {
              constexpr int ct = decltype(cc)::value;
              tmp[ct] = mfma4(ga[s], bv[s][ct], tmp[ct]);
            });
          sfor<NC>([&](auto cc) {
            constexpr int ct = decltype(cc)::value;
            constexpr int idx = M::ndw_before(W, d, k) + ct;
            constexpr int e0 = M::ndw_before(W, d, k) - M::ndw_before(W, d, 0);
            dw[idx] += tmp[ct];
            dws[idx] += tmp[ct] * ef[e0 + ct];
          });
        } else {
          // s outer: consecutive MFMAs update different dW tiles (no accumulator chain)
#pragma unroll
          for (int s = 0; s < 4; ++s)
            sfor<NC>([&](auto cc) {
              constexpr int ct = decltype(cc)::value;
              constexpr int idx = M::ndw_before(W, d, k) + ct;
              dw[idx] = mfma4(ga[s], bv[s][ct], dw[idx]);
            });
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    });
    if constexpr (M::GST) {
      sfor<M::FT(d)>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        if constexpr (M::fowner(d, k) == W) {
          constexpr int net = M::fnet(d, k), rt = M::frt(d, k);
          const f4 gv = *reinterpret_cast<const f4*>(rec + M::gbuf(net, d) + rt * 16 + g * 4);
          *reinterpret_cast<f4*>(gblk + t * M::ACT_A4 + (M::act_off(net, d) - M::ACT0) + rt * 16 + g * 4) = gv;
        }
      });
    }
    // (2) gradient w.r.t. the layer input (rows = input features); tiles sharing a
    // B operand (the same net's output gradient) are interleaved
    f4 xa[M::XT(d) > 0 ? M::XT(d) : 1];
    if constexpr (d == 0 && M::SPLITX0) {
      // partial input gradient of every layer-0 tile over this wave's K quads, to LDS;
      // summed (fixed wave order) and fed to the RK adjoint by bwd_body after the barrier
      constexpr int PQ = M::HAS_P ? M::kout(0, 0) / 16 : 0;
      // two accumulation chains per tile (even / odd K steps): half the dependent-MFMA latency
      f4 xo[M::XT(0)];
      sfor<M::XT(0)>([&](auto mm) { xa[decltype(mm)::value] = f4zero(); xo[decltype(mm)::value] = f4zero(); });
      f4 xq[M::x0q_w(W) > 0 ? M::x0q_w(W) : 1];
      sfor<M::x0q_w(W)>([&](auto jj) {
        constexpr int j = decltype(jj)::value, qq = W + j * WAVES;
        constexpr int net = qq < PQ ? 0 : 1, q = qq < PQ ? qq : qq - PQ;
        constexpr int KP = M::kout(net, 0);
        xq[j] = *reinterpret_cast<const f4*>(rec + M::gbuf(net, 0) + g * (KP / 4) + 4 * q);
      });
      sfor<M::x0q_w(W)>([&](auto jj) {
        constexpr int j = decltype(jj)::value;
        const f4 x = xq[j];
#pragma unroll
        for (int e = 0; e < 4; e += 2)
          sfor<M::XT(0)>([&](auto mm) {
            constexpr int m = decltype(mm)::value;
            xa[m] = mfma4(FX(m * M::x0q_w(W) + j)[e], x[e], xa[m]);
            xo[m] = mfma4(FX(m * M::x0q_w(W) + j)[e + 1], x[e + 1], xo[m]);
          });
      });
      sfor<M::XT(0)>([&](auto mm) {
        constexpr int m = decltype(mm)::value;
        *reinterpret_cast<f4*>(lds + M::X0P_LDS + ((W * M::XT(0) + m) * 64 + lane) * 4) = xa[m] + xo[m];
      });
      lds_sync();
      UDE_STAMP(pf, 7 + d);
      return;
    }
    f4 avv[M::XT(d) > 0 ? M::XT(d) : 1];
    sfor<M::XT(d)>([&](auto mm) {
      constexpr int m = decltype(mm)::value;
      if constexpr (M::xowner(d, m) == W) {
        xa[m] = f4zero();
        if constexpr (d > 0) {
          // the ELU-derivative operand of the epilogue, read ahead of the MFMAs
          constexpr int net = M::xnet(d, m), rt = M::xrt(d, m);
          if constexpr (M::act(net, d - 1))
            avv[m] = *reinterpret_cast<const f4*>(rec + M::act_off(net, d - 1) + rt * 16 + g * 4);
        }
      }
    });
    sfor<2>([&](auto nn) {
      constexpr int net = decltype(nn)::value;
      if constexpr (RW && packo<M>(net, d) && M::owns_x(W, d, net)) {
        // packo: one MFMA per tile, lane (t, g) supplies output g's gradient (padded rows are zero)
        const float xg = rec[M::gbuf(net, d) + g];
        sfor<M::XT(d)>([&](auto mm) {
          constexpr int m = decltype(mm)::value;
          if constexpr (M::xowner(d, m) == W && M::xnet(d, m) == net)
            xa[m] = mfma4(wr.wo[WR::po_index(d, m)], xg, xa[m]);
        });
      } else if constexpr (M::has(net, d) && M::owns_x(W, d, net)) {
        constexpr int KP = M::kout(net, d);
        // d == 0: both nets' fragments of a tile sit back to back (P first)
        constexpr int qoff = (d == 0 && net == 1 && M::HAS_P) ? M::kout(0, 0) / 16 : 0;
        const float* b = rec + M::gbuf(net, d) + g * (KP / 4);
        f4 xb[KP / 16];
#pragma unroll
        for (int q = 0; q < KP / 16; ++q) xb[q] = *reinterpret_cast<const f4*>(b + 4 * q);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < KP / 16; ++q) {
          const f4 x = xb[q];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            sfor<M::XT(d)>([&](auto mm) {
              constexpr int m = decltype(mm)::value;
              if constexpr (M::xowner(d, m) == W && (d == 0 || M::xnet(d, m) == net)) {
                if constexpr (UDE_ABL == 3) xa[m][e] += x[e];
                else xa[m] = mfma4(FX(M::xq_before(W, d, m) + qoff + q)[e], x[e], xa[m]);
              }
            });
        }
      }
    });
    if constexpr (PF && d > 0) load_x_frags<M, W, d - 1>(rs, lane, fxp + M::xq_base(W, d - 1));
    sfor<M::XT(d)>([&](auto mm) {
      constexpr int m = decltype(mm)::value;
      if constexpr (M::xowner(d, m) == W) {
        f4 acc = xa[m];
        if constexpr (d == 0) {
          ep0(m * 16 + g * 4, acc);
        } else {
          constexpr int net = M::xnet(d, m);
          constexpr int rt = M::xrt(d, m);
          if constexpr (M::act(net, d - 1)) {
            const f4 av = avv[m];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = av[e] <= 0.f ? acc[e] * (av[e] + 1.f) : acc[e];
          }
          *reinterpret_cast<f4*>(rec + M::gbuf(net, d - 1) + rt * 16 + g * 4) = acc;
        }
      }
    });
    UDE_STAMP(pf, 20 + d);
    lds_sync();
    UDE_STAMP(pf, 7 + d);
  });
}

// Weight gradients of one backward stage on the SPLIT_BWD partner waves (W = the index of the
// critical-path wave sharing the SIMD): the same barrier sequence as mlp_backward, and in phase
// d the rows the wave owns: dW += g . in^T (MFMA, K = the tile's 16 trajectories) from the
// phase's LDS operands, and per-trajectory bias sums in registers (reduced over the trajectories
// once, at the launch end, instead of a cross-lane reduction every phase).
template <class M, int W, int SR>
__device__ __forceinline__ void mlp_backward_dw(const float* lds, f4* dw, f4* g0t, f4* gacc, int lane) {
  const int t = lane & 15, g = lane >> 4;
  const float* rec = lds + t * SR;
  sfor<M::D>([&](auto ee) {
    constexpr int d = M::D - 1 - decltype(ee)::value;
    sfor<M::FT(d)>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      if constexpr (M::fowner(d, k) == W && !(UDE_ABL == 6 && d == 1)) {
        constexpr int net = M::fnet(d, k), rt = M::frt(d, k), goff = M::gbuf(net, d);
        constexpr int inoff = d == 0 ? M::Y_OFF : M::act_off(net, d - 1);
        constexpr int NC = M::rti(net, d);
        const f4 gv = *reinterpret_cast<const f4*>(rec + goff + rt * 16 + g * 4);
        float ga[4], bv[4][NC];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          ga[s] = lds[(4 * g + s) * SR + goff + rt * 16 + t];
#pragma unroll
          for (int ct = 0; ct < NC; ++ct) bv[s][ct] = lds[(4 * g + s) * SR + inoff + ct * 16 + t];
        }
        if constexpr (d == 0) g0t[M::nz_before(W, k)] += gv;
        else gacc[M::ng_before(W, d, k)] += gv;
#pragma unroll
        for (int s = 0; s < 4; ++s)
          sfor<NC>([&](auto cc) {
            constexpr int ct = decltype(cc)::value;
            constexpr int idx = M::ndw_before(W, d, k) + ct;
            dw[idx] = mfma4(ga[s], bv[s][ct], dw[idx]);
          });
      }
    });
    lds_sync();
  });
}

// ---- SPLIT_BWD_L: the partner waves of large records ------------------------------------
// Barrier for waves with LDS-DMA loads in flight: their LDS writes are retired by lgkmcnt, the
// DMA (which counts on vmcnt) stays in flight across it (lds_sync's release fence would drain it,
// holding the critical-path waves at this barrier for the HBM latency).
__device__ __forceinline__ void lds_sync_dma() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0) only
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void wait_dma() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0)
  __builtin_amdgcn_sched_barrier(0);
}
typedef __attribute__((address_space(3))) void* LdsPtr;

// LDS-DMA of one layer's activation rows (net, i) of tile-stage (step, jj) into the record:
// partner wave W moves trajectories 4W .. 4W+3, one 16-B-per-lane instruction each (kout / 4
// lanes; the record row's layer slice is contiguous, so the lane-linear destination fits).  The
// source goes through a buffer resource: SGPR base of the tile-stage block, one shared per-lane
// offset (16 lane) and the slice's constant offset in the scalar soffset.  Per-instruction
// per-lane addresses held in VGPRs spilled, and every spill reload (a vmcnt wait) drained all
// DMAs in flight.
template <class M, int W, int net, int i>
__device__ __forceinline__ void dma_layer(Rsrc src, float* lds, int lane) {
  if constexpr (UDE_ABL == 22) return;
  constexpr int SR = M::SR_B, KO = M::kout(net, i), OFF = M::act_off(net, i);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int t = 4 * W + u;
#if defined(__HIP_DEVICE_COMPILE__)
    if (lane < KO / 4)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(src, (LdsPtr)(lds + t * SR + OFF), 16, 16 * lane,
                                               (t * M::XST_W + M::ACT_IN + (OFF - M::ACT0)) * 4, 0, 0);
#endif
  }
}
template <class M>
__device__ __forceinline__ Rsrc act_rsrc(const KArgs& A, int tile, int step, int jj) {
  return make_rsrc(act_block<M>(A.ckpt, A.n_tiles, A.n_steps, tile, step, jj), TT * M::XST_W * 4);
}
// the layers whose last reader of the current stage is phase d (d = D: the flux pass)
template <class M, int W, int d>
__device__ __forceinline__ void dma_freed(Rsrc src, float* lds, int lane) {
  sfor<2>([&](auto nn) {
    constexpr int net = decltype(nn)::value;
    if constexpr (d == M::D) {
      if constexpr (M::has(net, 0)) dma_layer<M, W, net, M::nl(net) - 1>(src, lds, lane);
    } else if constexpr (d >= 1 && M::has(net, d) && d - 1 < M::nl(net) - 1) {
      dma_layer<M, W, net, d - 1>(src, lds, lane);
    }
  });
}
// LDS-DMA of the checkpointed stage input ([F][16], contiguous) into the staging slot
template <class M, int W>
__device__ __forceinline__ void dma_ckpt(const KArgs& A, float* lds, int tile, int step, int jj, int lane) {
  constexpr int NF = M::F * TT, NC = (NF + 255) / 256;
  const Rsrc src = make_rsrc(A.ckpt + ckpt_index(tile, A.n_steps, step, jj, M::F, 0, 0), NF * 4);
#pragma unroll
  for (int c = W; c < NC; c += WAVES) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (c * 256 + 4 * lane < NF)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(src, (LdsPtr)(lds + M::STG_LDS + c * 256), 16, 16 * lane, c * 1024,
                                               0, 0);
#endif
  }
}

// Weight gradients of one stage (large records): as mlp_backward_dw, with each owned tile's input
// operands read in chunks of XC column tiles (registers: the dW accumulators fill this wave) and the
// bias sums reduced across the tile's trajectories into the LDS row sums every phase.
template <class M, int W, int SR, class After>
__device__ __forceinline__ void mlp_backward_dw_l(float* lds, f4* dw, f4* g0t, int lane, const After& after,
                                                  Prof* pf = nullptr) {
  const int t = lane & 15, g = lane >> 4;
  const float* rec = lds + t * SR;
  constexpr int XC = 4;
  sfor<M::D>([&](auto ee) {
    constexpr int d = M::D - 1 - decltype(ee)::value;
    sfor<M::FT(d)>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      if constexpr (M::fowner(d, k) == W) {
        constexpr int net = M::fnet(d, k), rt = M::frt(d, k), goff = M::gbuf(net, d);
        constexpr int inoff = d == 0 ? M::Y_OFF : M::act_off(net, d - 1);
        constexpr int NC = M::rti(net, d);
        const f4 gv = *reinterpret_cast<const f4*>(rec + goff + rt * 16 + g * 4);
        float ga[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) ga[s] = lds[(4 * g + s) * SR + goff + rt * 16 + t];
        if constexpr (UDE_ABL != 21) sfor<(NC + XC - 1) / XC>([&](auto cc0) {
          constexpr int c0 = decltype(cc0)::value * XC;
          constexpr int NCC = cmin(XC, NC - c0);
          float bv[4][NCC];
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int ct = 0; ct < NCC; ++ct) bv[s][ct] = lds[(4 * g + s) * SR + inoff + (c0 + ct) * 16 + t];
#pragma unroll
          for (int s = 0; s < 4; ++s)
            sfor<NCC>([&](auto cc) {
              constexpr int ct = decltype(cc)::value;
              constexpr int idx = M::ndw_before(W, d, k) + c0 + ct;
              dw[idx] = mfma4(ga[s], bv[s][ct], dw[idx]);
            });
        });
        if constexpr (d == 0) {
          g0t[M::nz_before(W, k)] += gv;
        } else {
          f4 r = gv;
#pragma unroll
          for (int e = 0; e < 4; ++e) r[e] = row16_sum(r[e]);
          if (t == 0) {
            float* db = lds + M::DB_LDS + (M::FTbase(d) + k) * 16 + g * 4;
            db[0] += r[0]; db[1] += r[1]; db[2] += r[2]; db[3] += r[3];
          }
        }
      }
    });
    // the next stage's rows freed by phase d + 1 (D: the flux pass) are fetched behind this phase's
    // MFMAs instead of ahead of them, except layer 0's (needed soonest: issued as phase 0 starts)
    if constexpr (d + 1 >= 2) after(std::integral_constant<int, d + 1>{});
    UDE_STAMP(pf, 20 + d);
    lds_sync_dma();
    UDE_STAMP(pf, 7 + d);
    if constexpr (d == 1) after(std::integral_constant<int, 1>{});
    UDE_STAMP(pf, 24 + d);
  });
}

}  // namespace ude
