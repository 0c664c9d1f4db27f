// The backward solve (VJP): the RK4 adjoint epilogue, output cotangents, checkpoint loads, the flux backward,
// tile / kernel ends, bwd_body, the partner waves (bwd_wbody, bwd_wbody_l), ude_bwd_kernel and the static
// time-sum kernels.
#pragma once
#include "ude_kernels_mlp.h"

namespace ude {

// ============================================================================
// Backward (VJP)
// ============================================================================
// RK4 (3/8 rule) adjoint of the stage input, MLP part: consumes the layer-0 input
// gradient dY (4 features x 1 trajectory per lane) straight from the dX tile's
// registers (see the flux section of bwd_body for the direct part).
template <class M, int SR>
struct RkAdjointEp {
  float* rec;      // this lane's trajectory record
  float dt;
  int jj;          // RK stage (3..0)
  __device__ __forceinline__ void operator()(int f0, f4 dY) const {
    if constexpr (M::FULL0) {
      // static features (rows F16..): no RK adjoint, their input gradient is summed
      // over every evaluation of the solve (DYS, written to dy0 at tile end)
      if (f0 >= M::F16) {
        *reinterpret_cast<f4*>(rec + M::DYS_OFF + f0 - M::F16) += dY;
        return;
      }
    }
    if (f0 >= M::F4) return;                       // padded feature rows
    // DYF: the stage's flux part (parked by the flux pass) joins the MLP part first, one update
    if constexpr (M::DYF) dY += *reinterpret_cast<const f4*>(rec + M::DYF_OFF + f0);
    f4* accy = reinterpret_cast<f4*>(rec + M::RK_ACCY + f0);
    f4* dk1 = reinterpret_cast<f4*>(rec + M::RK_DK1 + f0);
    f4* dk2 = reinterpret_cast<f4*>(rec + M::RK_DK2 + f0);
    f4* dk3 = reinterpret_cast<f4*>(rec + M::RK_DK3 + f0);
    // every read before the first write: one LDS round trip, not one per accumulator
    const f4 a = *accy, k1 = *dk1, k2 = *dk2, k3 = *dk3;
    rk_adjoint_update(dY, dt, jj, a, k1, k2, k3, accy, dk1, dk2, dk3);
  }
  // 3/8-rule stage-input adjoint: accy += dY and the stage cotangents of the stages before jj
  //   Y2 = y + (dt k1)/3, Y3 = y + dt (k2 - k1/3), Y4 = y + dt (k1 - k2 + k3)
  static __device__ __forceinline__ void rk_adjoint_update(f4 dY, float dt, int jj, f4 a, f4 k1, f4 k2, f4 k3,
                                                           f4* accy, f4* dk1, f4* dk2, f4* dk3) {
    *accy = a + dY;
    if (jj == 3) {
      const f4 u = dt * dY;
      *dk1 = k1 + u; *dk2 = k2 - u; *dk3 = k3 + u;
    } else if (jj == 2) {
      const f4 u = dt * dY;
      *dk2 = k2 + u; *dk1 = k1 - u * (1.0f / 3.0f);
    } else if (jj == 1) {
      *dk1 = k1 + (dY * (1.0f / 3.0f)) * dt;
    }
  }
};

// Cotangents of the outputs written after RK step `step` (torchdiffeq's
// _linear_interp between y_step and y_step+1): sg = the y_{step+1}-side share,
// pg = the y_step-side share, per pair slot (p = tid + sl * NTHREADS) and S/I/R.
// out_issue starts the loads of the step's first output (if any); out_finish turns
// them into shares and handles any further outputs of the step synchronously.
template <class M>
__device__ __forceinline__ void out_load(const KArgs& A, const Sched& sc, int o, int n0,
                                         float (&gv)[M::SLOTS][3], int tid = threadIdx.x) {
  // one source: the full (T, N, R, L) cotangent, or the compact S, I, R one (exactly one of
  // them is set, see ude_rk4_backward_sir)
  const int ld = A.dlatent ? M::L : 3;
  const float* gl = (A.dlatent ? A.dlatent : A.dlat_sir) + (size_t)sc.out_j[o] * A.n_traj * M::R * ld;
  sfor<M::SLOTS>([&](auto ss) {
    constexpr int sl = decltype(ss)::value;
    const int p = tid + sl * NTHREADS;
    const int r = p / TT, t = p - r * TT, n = n0 + t;
    const bool valid = p < M::PAIRS && n < A.n_traj;
    const size_t base = valid ? ((size_t)n * M::R + r) * ld : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) gv[sl][c] = valid ? gl[base + c] : 0.f;
  });
}
template <class M>
__device__ __forceinline__ void out_issue(const KArgs& A, const Sched& sc, int step, int n0,
                                          float (&gv)[M::SLOTS][3], int tid = threadIdx.x) {
  if (sc.out_start[step] < sc.out_start[step + 1]) out_load<M>(A, sc, sc.out_start[step], n0, gv, tid);
}
template <class M>
__device__ __forceinline__ void out_finish(const KArgs& A, const Sched& sc, int step, int n0,
                                           float (&gv)[M::SLOTS][3], float (&sg)[M::SLOTS][3],
                                           float (&pg)[M::SLOTS][3], int tid = threadIdx.x) {
#pragma unroll
  for (int sl = 0; sl < M::SLOTS; ++sl)
#pragma unroll
    for (int c = 0; c < 3; ++c) { sg[sl][c] = 0.f; pg[sl][c] = 0.f; }
  const int o_beg = sc.out_start[step], o_end = sc.out_start[step + 1];
  #pragma unroll 1
  for (int o = o_beg; o < o_end; ++o) {
    if (o > o_beg) out_load<M>(A, sc, o, n0, gv, tid);
    const int mode = sc.out_mode[o];
    const float slope = sc.out_slope[o];
#pragma unroll
    for (int sl = 0; sl < M::SLOTS; ++sl)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float a = mode == 2 ? slope * gv[sl][c] : (mode == 1 ? gv[sl][c] : 0.f);
        const float b = mode == 2 ? gv[sl][c] - a : (mode == 0 ? gv[sl][c] : 0.f);
        sg[sl][c] += a;
        pg[sl][c] += b;
      }
  }
}

// Issue the loads of one checkpointed stage input ([f][t] per tile-stage in HBM)
// into registers, slot sl of thread tid holding pair p = tid + sl * NTHREADS.
template <class M>
__device__ __forceinline__ void ckpt_issue(const KArgs& A, int tile, int step, int jj, float (&ck)[M::SLOTS][3],
                                           int tid = threadIdx.x) {
  const Rsrc rck = make_rsrc(A.ckpt + ckpt_index(tile, A.n_steps, step, jj, M::F, 0, 0), M::F * TT * 4);
  sfor<M::SLOTS>([&](auto ss) {
    constexpr int sl = decltype(ss)::value;
    const int p = tid + sl * NTHREADS;
    const int r = p / TT, t = p - r * TT;
    const int v = (p < M::PAIRS) ? (3 * r * TT + t) * 4 : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      ck[sl][c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rck, v, c * TT * 4, 0));
  });
}

// Flux backward for one RK stage (reference RHS, lib/models.py:130-150):
//   dS = -beta S I, dI = beta S I - gamma I, dR = gamma I  (+ fa_w * Fa for FaFp),
// masked where a state leaves (-1, 2); beta = |q0|, gamma = |q1|.  Writes the
// final-layer gradients (d q, d Fa incl. the |Fa| and posterior side-statistic
// terms) and applies the direct (d flux / d S, I) part of the RK adjoint.
template <class M, int SR>
__device__ __forceinline__ void flux_backward(float* lds, const KArgs& A, int n0, int jj, float dt,
                                              const float* ca, const float* cb, const float* mu, float cn) {
  constexpr int RG = (M::R + 3) / 4, ITEMS = TT * RG;
  constexpr int QO = Q_OUT<M>, QG = M::HAS_P ? M::gbuf(0, M::nl(0) - 1) : 0;
  constexpr int FO = FA_OUT<M>, FG = M::HAS_A ? M::gbuf(1, M::nl(1) - 1) : 0;
  constexpr bool VEC_Q = !M::HAS_P || M::QW <= M::kout(0, M::nl(0) - 1);
  constexpr bool VEC_F = !M::HAS_A || M::F4 <= M::kout(1, M::nl(1) - 1);
  // G regions per item: 4 (12 features, 8 rates: 16-B LDS ops), or all of them when R < 4 (one
  // item per trajectory with only its live features: at R = 1 a quarter of the VALU and LDS
  // work of a 4-region group, on the single wave that runs the pass)
  constexpr int G = M::R < 4 ? M::R : 4;
  constexpr int NQF = (3 * G + 3) / 4, NQR = (2 * G + 3) / 4;   // feature / rate quads per item
  constexpr int NF = 4 * NQF, NR = 4 * NQR;
  #pragma unroll 1
  for (int it = threadIdx.x; it < ITEMS; it += NTHREADS) {
    const int t = it & (TT - 1), rg = it >> 4;
    const bool valid = n0 + t < A.n_traj;
    float* rec = lds + t * SR;
    float Y[NF], dk[NF], dres[NF];
    const int f0 = 12 * rg;
    const int dko = jj == 3 ? M::RK_A : jj == 2 ? M::RK_DK3 : jj == 1 ? M::RK_DK2 : M::RK_DK1;
#pragma unroll
    for (int v = 0; v < NQF; ++v) {
      const f4 y = *reinterpret_cast<const f4*>(rec + M::Y_OFF + f0 + 4 * v);
      const f4 k = *reinterpret_cast<const f4*>(rec + dko + f0 + 4 * v);
#pragma unroll
      for (int e = 0; e < 4; ++e) { Y[4 * v + e] = y[e]; dk[4 * v + e] = k[e]; }
    }
    // the RK adjoint accumulators this stage updates, read with the other operands (every LDS
    // read of the item before its first write: one round trip)
    f4 ra[NQF], r1[NQF], r2[NQF], r3[NQF];
    if constexpr (M::HAS_P && !M::DYF) {
#pragma unroll
      for (int v = 0; v < NQF; ++v) {
        ra[v] = *reinterpret_cast<const f4*>(rec + M::RK_ACCY + f0 + 4 * v);
        r1[v] = *reinterpret_cast<const f4*>(rec + M::RK_DK1 + f0 + 4 * v);
        r2[v] = *reinterpret_cast<const f4*>(rec + M::RK_DK2 + f0 + 4 * v);
        r3[v] = *reinterpret_cast<const f4*>(rec + M::RK_DK3 + f0 + 4 * v);
      }
    }
    float qv[NR], fav[NF];
    if constexpr (M::HAS_P) {
#pragma unroll
      for (int v = 0; v < NQR; ++v) {
        const f4 x = *reinterpret_cast<const f4*>(rec + QO + 8 * rg + 4 * v);
#pragma unroll
        for (int e = 0; e < 4; ++e) qv[4 * v + e] = x[e];
      }
    }
    if constexpr (M::HAS_A) {
#pragma unroll
      for (int v = 0; v < NQF; ++v) {
        const f4 fa = *reinterpret_cast<const f4*>(rec + FO + f0 + 4 * v);
#pragma unroll
        for (int e = 0; e < 4; ++e) fav[4 * v + e] = fa[e];
      }
    }
    if (jj == 3) {
#pragma unroll
      for (int i = 0; i < NF; ++i) dk[i] = (dk[i] * 0.125f) * dt;
    }
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const bool live = valid && i < 3 * G && (4 * rg + i / 3) < M::R;
      dres[i] = (!live || sir_masked(Y[i])) ? 0.f : dk[i];
    }
    if constexpr (M::HAS_A) {
      float dfa[NF];
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        const bool live = valid && i < 3 * G && (4 * rg + i / 3) < M::R;
        dfa[i] = sir_fa_cot<M::HAS_P>(live, A.fa_w, dres[i], cn * fav[i]);
      }
      if constexpr (VEC_F) {
#pragma unroll
        for (int v = 0; v < NQF; ++v) {
          f4 o = {dfa[4 * v], dfa[4 * v + 1], dfa[4 * v + 2], dfa[4 * v + 3]};
          *reinterpret_cast<f4*>(rec + FG + f0 + 4 * v) = o;
        }
      } else {
#pragma unroll
        for (int i = 0; i < NF; ++i)
          if (f0 + i < M::kout(1, M::nl(1) - 1)) rec[FG + f0 + i] = dfa[i];
      }
    }
    float dyf[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) dyf[i] = 0.f;
    if constexpr (M::HAS_P) {
      float dq[NR];
#pragma unroll
      for (int i = 0; i < NR; ++i) dq[i] = 0.f;
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const bool live = valid && (4 * rg + j) < M::R;
        const float dr[3] = {dres[3 * j], dres[3 * j + 1], dres[3 * j + 2]};
        float b, gm, dbeta, dgam;
        sir_rates(qv[2 * j], qv[2 * j + 1], b, gm);
        sir_flux_vjp(Y[3 * j], Y[3 * j + 1], b, gm, dr, dbeta, dgam, dyf[3 * j], dyf[3 * j + 1]);
        // the side statistics' cotangents reach beta / gamma directly
        dbeta = live ? dbeta + (ca[0] + cb[0] * (b - mu[0])) : 0.f;
        dgam = live ? dgam + (ca[1] + cb[1] * (gm - mu[1])) : 0.f;
        dq[2 * j] = sir_abs_cot(qv[2 * j], dbeta);
        dq[2 * j + 1] = sir_abs_cot(qv[2 * j + 1], dgam);
      }
      if constexpr (VEC_Q) {
#pragma unroll
        for (int v = 0; v < NQR; ++v) {
          f4 o = {dq[4 * v], dq[4 * v + 1], dq[4 * v + 2], dq[4 * v + 3]};
          *reinterpret_cast<f4*>(rec + QG + 8 * rg + 4 * v) = o;
        }
      } else {
#pragma unroll
        for (int i = 0; i < NR; ++i)
          if (8 * rg + i < M::kout(0, M::nl(0) - 1)) rec[QG + 8 * rg + i] = dq[i];
      }
      // RK4 (3/8 rule) adjoint of the stage input, direct (flux) part; the MLP part
      // is added by mlp_backward's layer-0 epilogue (RkAdjointEp)
      //   Y2 = y + (dt k1)/3, Y3 = y + dt (k2 - k1/3), Y4 = y + dt (k1 - k2 + k3)
#pragma unroll
      for (int v = 0; v < NQF; ++v) {
        const f4 dY = {dyf[4 * v], dyf[4 * v + 1], dyf[4 * v + 2], dyf[4 * v + 3]};
        const int f = f0 + 4 * v;
        if constexpr (M::DYF) {
          // parked for the stage's one adjoint update (RkAdjointEp, with the MLP part)
          *reinterpret_cast<f4*>(rec + M::DYF_OFF + f) = dY;
          continue;
        }
        RkAdjointEp<M, SR>::rk_adjoint_update(dY, dt, jj, ra[v], r1[v], r2[v], r3[v],
                                              reinterpret_cast<f4*>(rec + M::RK_ACCY + f),
                                              reinterpret_cast<f4*>(rec + M::RK_DK1 + f),
                                              reinterpret_cast<f4*>(rec + M::RK_DK2 + f),
                                              reinterpret_cast<f4*>(rec + M::RK_DK3 + f));
      }
    }
    // the padded rows of the final-layer gradient slots (the slots alias wider layers'
    // gradients, so they are re-zeroed every stage), by the item of the last region group
    if (rg == RG - 1) {
      if constexpr (M::HAS_P) {
        constexpr int lo = cmin(8 * (RG - 1) + 4 * NQR, M::kout(0, M::nl(0) - 1)), hi = M::kout(0, M::nl(0) - 1);
#pragma unroll
        for (int o = lo; o < hi; o += 4) *reinterpret_cast<f4*>(rec + QG + o) = f4zero();
      }
      if constexpr (M::HAS_A) {
        constexpr int lo = cmin(12 * (RG - 1) + 4 * NQF, M::kout(1, M::nl(1) - 1)), hi = M::kout(1, M::nl(1) - 1);
#pragma unroll
        for (int o = lo; o < hi; o += 4) *reinterpret_cast<f4*>(rec + FG + o) = f4zero();
      }
    }
  }
}

// Tile end (deterministic RHS): per-trajectory layer-0 gradient sums -> global (the
// static-feature gradients are computed from them by ude_static_*_kernel); their trajectory
// sums -> the workgroup's bias row sums in LDS.
template <class M, int W, class AT>
__device__ __forceinline__ void g0_tile_end(const AT& A, float* lds, const f4* g0t, int tile, int lane) {
  const int t16 = lane & 15, g = lane >> 4;
  sfor<M::FT(0)>([&](auto kk) {
    constexpr int k = decltype(kk)::value;
    if constexpr (M::fowner(0, k) == W) {
      const f4 gv = g0t[M::nz_before(W, k)];
      if constexpr (M::HOIST) {
        float* dst = A.g0buf + ((size_t)tile * M::K0 + k * 16 + g * 4) * TT + t16;
        dst[0] = gv[0]; dst[TT] = gv[1]; dst[2 * TT] = gv[2]; dst[3 * TT] = gv[3];
      }
      f4 r = gv;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = row16_sum(r[e]);
      if (t16 == 0) {
        float* db = lds + M::DB_LDS + k * 16 + g * 4;
        db[0] += r[0]; db[1] += r[1]; db[2] += r[2]; db[3] += r[3];
      }
    }
  });
}

// Kernel end: wave W's dW register tiles (and BAYES eps-weighted ones) -> the workgroup slab.
template <class M, int W, class DW, class DS>
__device__ __forceinline__ void dw_to_slab(const DW& dw, const DS& dws, float* myslab, int lane) {
  sfor<M::D>([&](auto dd) {
    constexpr int d = decltype(dd)::value;
    sfor<M::FT(d)>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      if constexpr (M::fowner(d, k) == W) {
        constexpr int net = M::fnet(d, k);
        sfor<M::rti(net, d)>([&](auto cc) {
          constexpr int ct = decltype(cc)::value;
          reinterpret_cast<f4*>(myslab + (M::dyn_tiles_before(d, k) + ct) * 256)[lane] = dw[M::ndw_before(W, d, k) + ct];
          if constexpr (M::BAYES)
            reinterpret_cast<f4*>(myslab + M::SLAB_TOTAL + (M::dyn_tiles_before(d, k) + ct) * 256)[lane] =
                dws[M::ndw_before(W, d, k) + ct];
        });
      }
    });
  });
}

template <class M, int W>
__device__ void bwd_body(const KArgs& A, float* lds) {
  constexpr int SR = M::SR_B;
  constexpr int SL = M::SLOTS;
  constexpr int NDWn = M::NDW(W) > 0 ? M::NDW(W) : 1;
  constexpr int NZn = M::NZ(W) > 0 ? M::NZ(W) : 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int t16 = lane & 15, g = lane >> 4;
  const Sched sc(A.sched, A.n_steps, A.n_out);
  const size_t NRL = (size_t)A.n_traj * M::R * M::L;
  float* myslab = A.slab + (size_t)blockIdx.x * M::SLAB_STRIDE;
  const Rsrc rs = make_rsrc(A.pack, M::PACK_TOTAL * 4);

  // side-statistic cotangents -> per-eval gradient coefficients
  //   d mean_c / d p = 1/n ;  d std_c / d p = (p - mean_c) / ((n - 1) std_c)   (torch std backward)
  //   d |Fa| / d Fa = Fa / |Fa|  (0 when |Fa| == 0, torch norm backward)
  const double nev = 4.0 * (double)A.n_steps * (double)A.n_traj * (double)M::R;
  float ca[2] = {0.f, 0.f}, cb[2] = {0.f, 0.f}, mu[2] = {0.f, 0.f}, cn = 0.f;
  if constexpr (M::HAS_P) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      mu[c] = A.st_mean[c];
      ca[c] = A.d_mean ? (float)((double)A.d_mean[c] / nev) : 0.f;
      const double sd = (double)A.st_std[c];
      cb[c] = A.d_std ? (float)((double)A.d_std[c] / ((nev - 1.0) * sd)) : 0.f;
    }
  }
  if constexpr (M::HAS_A) {
    const float nrm = A.st_norm[0];
    cn = (nrm > 0.f && A.d_norm) ? A.d_norm[0] / nrm : 0.f;
  }

  // SPLITB: the weight-gradient accumulators live on the partner waves (bwd_wbody / bwd_wbody_l)
  // GST: no weight-gradient accumulators (ude_gst_dw_kernel forms them from the stored rows)
  constexpr bool NO_DW = M::SPLITB || M::GST;
  f4 dw[NO_DW ? 1 : NDWn], dws[(M::BAYES && !M::GST) ? NDWn : 1], g0t[NZn], c1[NZn];
#pragma unroll
  for (int i = 0; i < (NO_DW ? 1 : NDWn); ++i) dw[i] = f4zero();
  if constexpr (M::BAYES && !M::GST) {
#pragma unroll
    for (int i = 0; i < NDWn; ++i) dws[i] = f4zero();
  }
  Prof prof_, *pf = nullptr;
#ifdef UDE_PROFILE
  if (A.prof && tid == 0) {
    pf = &prof_;
    for (int i = 0; i < NPROF; ++i) prof_.acc[i] = 0;
    prof_.last = __builtin_amdgcn_s_memtime();
  }
#endif

  WRegs<M, W, true> wr;
  wr.load(rs, lane);

  #pragma unroll 1
  for (int i = tid; i < M::LDS_B / 4; i += NTHREADS) lds[i] = 0.f;
  lds_sync();

  for (int tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    const int n0 = tile * TT;
    // the record's static features feed only the static hoist of a recomputed forward (and FULL0's
    // layer 0); with stored activations their alias of the activation region must stay untouched
    // (the SPLIT_BWD_L partner waves fill it by LDS-DMA meanwhile)
    if constexpr (!M::ACT_STORED || (M::FULL0 && !M::GST)) load_static<M, SR, M::XSB_OFF>(A.y0, lds, n0, A.n_traj);
    if constexpr (M::FULL0) {
      #pragma unroll 1
      for (int i = tid; i < TT * M::S16; i += NTHREADS) {
        const int t = i / M::S16, s = i - t * M::S16;
        lds[t * SR + M::DYS_OFF + s] = 0.f;
      }
    }
    // output cotangents of the last step: y_{n+1} share -> RK_A, y_n share staged in
    // DK3 (picked up by the step start).  Later steps get theirs under the flux pass
    // of the previous step's last stage.  (These pair-mapped stores are the only
    // writes of RK_A here: every (t, f < F) is covered, zeros without a step.)
    {
      float gv[SL][3], sg[SL][3], pg[SL][3];
      if (A.n_steps > 0) {
        out_issue<M>(A, sc, A.n_steps - 1, n0, gv);
        out_finish<M>(A, sc, A.n_steps - 1, n0, gv, sg, pg);
      } else {
#pragma unroll
        for (int sl = 0; sl < SL; ++sl)
#pragma unroll
          for (int c = 0; c < 3; ++c) { sg[sl][c] = 0.f; pg[sl][c] = 0.f; }
      }
      sfor<SL>([&](auto ss) {
        constexpr int sl = decltype(ss)::value;
        const int p = tid + sl * NTHREADS;
        if (p < M::PAIRS) {
          const int r = p / TT, t = p - r * TT;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            lds[t * SR + M::RK_A + 3 * r + c] = sg[sl][c];
            lds[t * SR + M::RK_DK3 + 3 * r + c] = pg[sl][c];
          }
        }
      });
    }
    lds_sync();
    if constexpr (!M::ACT_STORED) static_hoist<M, W, SR, M::XSB_OFF>(rs, lds, c1, lane);
#pragma unroll
    for (int i = 0; i < NZn; ++i) g0t[i] = f4zero();
    lds_sync();
    UDE_STAMP(pf, 15);

    bool have_next = false;
    // small records with stored activations (CARRY): the next stage's activation rows and
    // checkpointed input are loaded into registers one whole stage ahead and written
    // straight into the record at that stage's start (no LDS staging slot, and the HBM
    // latency is covered by a full stage of work instead of one flux pass)
    constexpr bool CARRY = M::STORE_ACT && SL == 1;
    f4 actr[CARRY ? act_q_per_thread<M>() : 1];
    float ckr[SL][3];
    // CARRY: the next step's output cotangents are loaded at stage 1 of the step (a whole stage
    // ahead of the flux pass of stage 0 that consumes them)
    float gvc[SL][3];
    // GST: the next stage's checkpointed input and activation rows are carried in registers (no LDS
    // staging slot; the rows' HBM latency runs under the stage's four layer phases), and every phase's
    // input-gradient fragments are prefetched one phase ahead (mlp_backward PF)
    float ckg[M::GST ? SL : 1][3];
    constexpr bool GST_A = M::GST && M::STORE_ACT_D;
    f4 actg[GST_A ? act_q_per_thread<M>() : 1];
    float gvg[GST_A ? SL : 1][3];          // GST: the next step's output cotangents, loaded a stage ahead
    f4 fxp[(M::PF_X && M::WX_Q(W) > 0) ? M::WX_Q(W) : 1];
    for (int step = A.n_steps - 1; step >= 0; --step) {
      const float dt = sc.dt[step];
      // step start: RK_A already holds the adjoint of y_{n+1} including this step's
      // output cotangents (y_n-side share staged in DK3); set up the accumulators and
      // the stage cotangents of the 3/8 combination dy = (k1 + 3 (k2 + k3) + k4) dt / 8.
      {
        constexpr int NV = M::NVL;
        #pragma unroll 1
        for (int i = tid; i < TT * NV; i += NTHREADS) {
          const int t = i / NV, v = i - t * NV;
          float* rec = lds + t * SR + 4 * v;
          const f4 a = *reinterpret_cast<const f4*>(rec + M::RK_A);
          const f4 pend = *reinterpret_cast<const f4*>(rec + M::RK_DK3);
          const f4 sdk = (a * 0.125f) * dt;
          *reinterpret_cast<f4*>(rec + M::RK_PEND) = pend;
          *reinterpret_cast<f4*>(rec + M::RK_ACCY) = a;
          *reinterpret_cast<f4*>(rec + M::RK_DK1) = sdk;
          *reinterpret_cast<f4*>(rec + M::RK_DK2) = 3.0f * sdk;
          *reinterpret_cast<f4*>(rec + M::RK_DK3) = 3.0f * sdk;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      UDE_STAMP(pf, 14);

      for (int jj = 3; jj >= 0; --jj) {
        // stage input: from the staging slot the previous stage's flux pass filled,
        // or (first stage of the tile) straight from the forward's checkpoint
        // large records: the step's output cotangents are loaded at its last stage's start, with
        // the activation rows (their latency is paid there anyway), not right before the flux pass
        float gvs[M::STORE_ACT_D ? SL : 1][3];
        if constexpr (M::STORE_ACT_D && !GST_A) {
          if (jj == 0 && step > 0) out_issue<M>(A, sc, step - 1, n0, gvs);
        }
        if (GST_A && have_next) {
          constexpr int QR = M::ACT_A4 / 4;
#pragma unroll
          for (int u = 0; u < act_q_per_thread<M>(); ++u) {
            const int i = tid + u * NTHREADS;
            if (i < TT * QR) {
              const int t = i / QR, q = i - t * QR;
              *reinterpret_cast<f4*>(lds + t * SR + M::ACT0 + 4 * q) = actg[GST_A ? u : 0];
            }
          }
        } else if constexpr (M::STORE_ACT_D && !M::SPLIT_BWD_L && UDE_ABL != 8) {
          // this stage's activation rows straight from the forward's store (issued first: the
          // stage-input copy below runs under their latency)
          constexpr int QR = M::ACT_A4 / 4;
          const f4* src = reinterpret_cast<const f4*>(act_block<M>(A.ckpt, A.n_tiles, A.n_steps, tile, step, jj));
          f4 av[act_q_per_thread<M>()];
#pragma unroll
          for (int u = 0; u < act_q_per_thread<M>(); ++u) {
            const int i = tid + u * NTHREADS;
            if (i < TT * QR) av[u] = src[act_src_q<M>(i)];
          }
#pragma unroll
          for (int u = 0; u < act_q_per_thread<M>(); ++u) {
            const int i = tid + u * NTHREADS;
            if (i < TT * QR) {
              const int t = i / QR, q = i - t * QR;
              *reinterpret_cast<f4*>(lds + t * SR + M::ACT0 + 4 * q) = av[u];
            }
          }
        }
        if constexpr (M::SPLIT_BWD) {
          // stage input, activation rows and output cotangents: the partner waves' (bwd_wbody)
        } else if constexpr (M::SPLIT_BWD_L) {
          // stage input and activation rows: the partner waves' (bwd_wbody_l)
        } else if (CARRY && have_next && UDE_ABL != 4) {
          constexpr int QR = M::ACT_A4 / 4;
#pragma unroll
          for (int u = 0; u < act_q_per_thread<M>(); ++u) {
            const int i = tid + u * NTHREADS;
            if (i < TT * QR) {
              const int t = i / QR, q = i - t * QR;
              *reinterpret_cast<f4*>(lds + t * SR + M::ACT0 + 4 * q) = actr[u];
            }
          }
          if (tid < M::PAIRS) {
            const int r = tid / TT, t = tid - r * TT;
#pragma unroll
            for (int c = 0; c < 3; ++c) lds[t * SR + M::Y_OFF + 3 * r + c] = ckr[0][c];
          }
        } else if (M::GST && have_next) {
          sfor<SL>([&](auto ss) {
            constexpr int sl = decltype(ss)::value;
            const int p = tid + sl * NTHREADS;
            if (p < M::PAIRS) {
              const int r = p / TT, t = p - r * TT;
#pragma unroll
              for (int c = 0; c < 3; ++c) lds[t * SR + M::Y_OFF + 3 * r + c] = ckg[M::GST ? sl : 0][c];
            }
          });
        } else if (have_next) {
          // the 3R stage-input features (quads of the F4-wide staging row, clipped to the
          // record's F16-wide Y slot: beyond it starts the activation region)
          constexpr int QY = cmin(M::F4, M::F16) / 4, NV = TT * QY;
          #pragma unroll 1
          for (int i = tid; i < NV; i += NTHREADS) {
            const int t = i / QY, v = i - t * QY;
            *reinterpret_cast<f4*>(lds + t * SR + M::Y_OFF + 4 * v) =
                *reinterpret_cast<const f4*>(lds + M::STG_LDS + t * M::F4 + 4 * v);
          }
          if constexpr (M::STORE_ACT) {
            constexpr int QR = M::ACT_A4 / 4;
            #pragma unroll
            for (int u = 0; u < act_q_per_thread<M>(); ++u) {
              const int i = tid + u * NTHREADS;
              if (i < TT * QR) {
                const int t = i / QR, q = i - t * QR;
                *reinterpret_cast<f4*>(lds + t * SR + M::ACT0 + 4 * q) =
                    *reinterpret_cast<const f4*>(lds + M::ACT_STG + 4 * i);
              }
            }
          }
        } else {
          if constexpr (M::STORE_ACT) {
            // first stage of the tile: its activations straight from the forward's store
            constexpr int QR = M::ACT_A4 / 4;
            const f4* src = reinterpret_cast<const f4*>(act_block<M>(A.ckpt, A.n_tiles, A.n_steps, tile, step, jj));
            #pragma unroll
            for (int u = 0; u < act_q_per_thread<M>(); ++u) {
              const int i = tid + u * NTHREADS;
              if (i < TT * QR) {
                const int t = i / QR, q = i - t * QR;
                *reinterpret_cast<f4*>(lds + t * SR + M::ACT0 + 4 * q) = src[act_src_q<M>(i)];
              }
            }
          }
          float ck[SL][3];
          ckpt_issue<M>(A, tile, step, jj, ck);
          sfor<SL>([&](auto ss) {
            constexpr int sl = decltype(ss)::value;
            const int p = tid + sl * NTHREADS;
            if (p < M::PAIRS) {
              const int r = p / TT, t = p - r * TT;
#pragma unroll
              for (int c = 0; c < 3; ++c) lds[t * SR + M::Y_OFF + 3 * r + c] = ck[sl][c];
            }
          });
        }
        UDE_STAMP(pf, 0);
        lds_sync();
        UDE_STAMP(pf, 1);
        // at the step's last stage the next step's output cotangents are loaded from
        // fwd phase 1 on (consumed after the flux pass)
        const int nstep = jj > 0 ? step : step - 1, njj = jj > 0 ? jj - 1 : 3;
        have_next = nstep >= 0;
        const bool next_out = jj == 0 && have_next;
        float gvn[SL][3];
        // BAYES: evaluation 4 step + jj's weight sample and eps
        Rsrc rse = rs, es = rs;
        if constexpr (M::BAYES) {
          const size_t ev = (size_t)(4 * step + jj);
          rse = make_rsrc(A.pack + ev * M::PACK_TOTAL, M::PACK_TOTAL * 4);
          es = make_rsrc(A.eslab + ev * M::SLAB_TOTAL, M::SLAB_TOTAL * 4);
        }
        if constexpr (M::PF_X) load_x_frags<M, W, M::D - 1>(rse, lane, fxp + M::xq_base(W, M::D - 1));
        // the next stage's checkpointed input: small records (one pair slot per thread)
        // fetch it before the recomputed forward, whose phases then hide the HBM latency;
        // wide ones under the flux pass (registers only live across that pass)
        float ckn[SL][3], sgn[SL][3], pgn[SL][3];
        constexpr bool EARLY_CK = SL == 1;
        if constexpr (M::SPLIT_BWD) {
          flux_backward<M, SR>(lds, A, n0, jj, dt, ca, cb, mu, cn);
        } else if constexpr (CARRY) {
          // the step's output cotangents (loaded a stage ago) are consumed before the next stage's
          // loads are issued: their wait sits in out_finish's runtime loop, where the compiler can
          // only emit vmcnt(0), which would also drain the fresh prefetch (HBM latency per step)
          if (next_out) out_finish<M>(A, sc, nstep, n0, gvc, sgn, pgn);
          if (jj == 1 && step > 0) out_issue<M>(A, sc, step - 1, n0, gvc);
          if (have_next) {
            ckpt_issue<M>(A, tile, nstep, njj, ckr);
            constexpr int QR = M::ACT_A4 / 4;
            const f4* src = reinterpret_cast<const f4*>(act_block<M>(A.ckpt, A.n_tiles, A.n_steps, tile, nstep, njj));
#pragma unroll
            for (int u = 0; u < act_q_per_thread<M>(); ++u) {
              const int i = tid + u * NTHREADS;
              if (i < TT * QR) actr[u] = src[act_src_q<M>(i)];
            }
          }
          if constexpr (UDE_ABL != 2) flux_backward<M, SR>(lds, A, n0, jj, dt, ca, cb, mu, cn);
        } else if (EARLY_CK && have_next) {
          ckpt_issue<M>(A, tile, nstep, njj, ckn);
        }
        if constexpr (CARRY) {
        } else if constexpr (M::STORE_ACT_D) {
          flux_backward<M, SR>(lds, A, n0, jj, dt, ca, cb, mu, cn);
        } else if constexpr (M::STORE_ACT) {
          // the stage's activations are the forward's (staged above); the next stage's are
          // fetched now and land in ACT_STG after the flux pass
          f4 actn[act_q_per_thread<M>()];
          if (have_next) {
            constexpr int QR = M::ACT_A4 / 4;
            const f4* src = reinterpret_cast<const f4*>(act_block<M>(A.ckpt, A.n_tiles, A.n_steps, tile, nstep, njj));
            #pragma unroll
            for (int u = 0; u < act_q_per_thread<M>(); ++u) {
              const int i = tid + u * NTHREADS;
              if (i < TT * QR) actn[u] = src[act_src_q<M>(i)];
            }
          }
          if (next_out) out_issue<M>(A, sc, nstep, n0, gvn);
          flux_backward<M, SR>(lds, A, n0, jj, dt, ca, cb, mu, cn);
          if (have_next) {
            constexpr int QR = M::ACT_A4 / 4;
            #pragma unroll
            for (int u = 0; u < act_q_per_thread<M>(); ++u) {
              const int i = tid + u * NTHREADS;
              if (i < TT * QR) *reinterpret_cast<f4*>(lds + M::ACT_STG + 4 * i) = actn[u];
            }
          }
        } else {
          mlp_forward<M, W, SR>(rse, lds, c1, lane, wr, pf, [&](auto dd) {
            if constexpr (decltype(dd)::value == (M::D > 2 ? 1 : 0))
              if (next_out) out_issue<M>(A, sc, nstep, n0, gvn);
          });
        }

        // flux backward: d k_j -> d q (pre-|.| rates), d Fa, and the direct d Y.
        // One item = one trajectory x a group of 4 regions (12 features, 8 rates):
        // every record access is a 16-B LDS op.
        if (!M::SPLIT_BWD_L && !GST_A && !EARLY_CK && have_next) ckpt_issue<M>(A, tile, nstep, njj, ckn);
        if constexpr (!M::ACT_STORED) flux_backward<M, SR>(lds, A, n0, jj, dt, ca, cb, mu, cn);
        UDE_STAMP(pf, 16);
        if (!M::SPLIT_BWD && next_out) {
          if constexpr (GST_A) out_finish<M>(A, sc, nstep, n0, gvg, sgn, pgn);
          else if constexpr (M::STORE_ACT_D) out_finish<M>(A, sc, nstep, n0, gvs, sgn, pgn);
          else if constexpr (!CARRY) out_finish<M>(A, sc, nstep, n0, gvn, sgn, pgn);
          // step nstep's output cotangents: the y_{n+1} share joins PEND (RK_A of the
          // next step = ACCY + PEND), the y_n share is staged in DK3 (dead at jj == 0)
          sfor<SL>([&](auto ss) {
            constexpr int sl = decltype(ss)::value;
            const int p = tid + sl * NTHREADS;
            if (p < M::PAIRS) {
              const int r = p / TT, t = p - r * TT;
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                lds[t * SR + M::RK_PEND + 3 * r + c] += sgn[sl][c];
                lds[t * SR + M::RK_DK3 + 3 * r + c] = pgn[sl][c];
              }
            }
          });
        }
        UDE_STAMP(pf, 17);
        if constexpr (GST_A) {
          if (have_next) {
            // the next stage's input, activation rows and (a stage ahead of their consumer) output
            // cotangents, issued only after this stage's waits: no wait until the next stage start
            ckpt_issue<M>(A, tile, nstep, njj, ckg);
            const f4* src = reinterpret_cast<const f4*>(act_block<M>(A.ckpt, A.n_tiles, A.n_steps, tile, nstep, njj));
#pragma unroll
            for (int u = 0; u < act_q_per_thread<M>(); ++u) {
              const int i = tid + u * NTHREADS;
              if (i < TT * (M::ACT_A4 / 4)) actg[u] = src[act_src_q<M>(i)];
            }
            if (jj == 1 && step > 0) out_issue<M>(A, sc, step - 1, n0, gvg);
          }
        } else if (M::GST && !CARRY && have_next) {
#pragma unroll
          for (int sl = 0; sl < (M::GST ? SL : 1); ++sl)
#pragma unroll
            for (int c = 0; c < 3; ++c) ckg[sl][c] = ckn[sl][c];
        } else if (!CARRY && !M::SPLIT_BWD_L && have_next) {
          sfor<SL>([&](auto ss) {
            constexpr int sl = decltype(ss)::value;
            const int p = tid + sl * NTHREADS;
            if (p < M::PAIRS) {
              const int r = p / TT, t = p - r * TT;
#pragma unroll
              for (int c = 0; c < 3; ++c) lds[M::STG_LDS + t * M::F4 + 3 * r + c] = ckn[sl][c];
            }
          });
        }
        UDE_STAMP(pf, 18);
        UDE_STAMP(pf, 6);
        lds_sync();
        UDE_STAMP(pf, 11);
        if constexpr (UDE_ABL == 7) sfor<M::D>([&](auto) { lds_sync(); });
        else mlp_backward<M, W, SR, NO_DW, M::PF_X>(rse, es, lds, dw, dws, g0t, lane, pf,
                                           RkAdjointEp<M, SR>{lds + t16 * SR, dt, jj}, wr,
                                           M::GST ? A.gst + (((size_t)tile * A.n_steps + step) * 4 + jj) * TT * M::ACT_A4
                                                  : nullptr, fxp);
        if constexpr (M::SPLITX0) {
          // sum the waves' partial layer-0 input gradients -> RK adjoint (MLP part).  The RK rows
          // use the step-end thread <-> (t, quad) mapping, so the step end needs no barrier.
          auto x0sum = [&](int t, int f0) {
            const int m = f0 >> 4, li = ((f0 >> 2) & 3) * 16 + t;
            f4 v = f4zero();
#pragma unroll
            for (int w = 0; w < WAVES; ++w)
              v += *reinterpret_cast<const f4*>(lds + M::X0P_LDS + ((w * M::XT(0) + m) * 64 + li) * 4);
            return v;
          };
          constexpr int NV = M::NVL, NVX = cmin(M::F4, M::F16) / 4;
          #pragma unroll 1
          for (int i = tid; i < TT * NV; i += NTHREADS) {
            const int t = i / NV, v = i - t * NV;
            if (UDE_ABL != 5 && v < NVX) RkAdjointEp<M, SR>{lds + t * SR, dt, jj}(4 * v, x0sum(t, 4 * v));
          }
          if constexpr (M::FULL0) {
            constexpr int NS = M::S16 / 4;
            #pragma unroll 1
            for (int i = tid; i < TT * NS; i += NTHREADS) {
              const int t = i / NS, v = i - t * NS;
              RkAdjointEp<M, SR>{lds + t * SR, dt, jj}(M::F16 + 4 * v, x0sum(t, M::F16 + 4 * v));
            }
          }
        }

        UDE_STAMP(pf, 12);
      }
      // step end (same thread <-> element mapping as the step start: no barrier)
      {
        constexpr int NV = M::NVL;
        #pragma unroll 1
        for (int i = tid; i < TT * NV; i += NTHREADS) {
          const int t = i / NV, v = i - t * NV;
          float* rec = lds + t * SR + 4 * v;
          *reinterpret_cast<f4*>(rec + M::RK_A) =
              *reinterpret_cast<const f4*>(rec + M::RK_ACCY) + *reinterpret_cast<const f4*>(rec + M::RK_PEND);
        }
      }
      UDE_STAMP(pf, 13);
    }

    // ---- tile end: dy0 (dynamic), static-feature gradients, layer-0 bias sums ----
    lds_sync();
    #pragma unroll 1
    for (int p = tid; p < M::PAIRS; p += NTHREADS) {
      const int r = p / TT, t = p - r * TT;
      const int n = n0 + t;
      if (n < A.n_traj) {
        const size_t base = ((size_t)n * M::R + r) * M::L;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          A.dy0[base + c] = lds[t * SR + M::RK_A + 3 * r + c] +
                            (A.dlatent ? A.dlatent[base + c] : A.dlat_sir[((size_t)n * M::R + r) * 3 + c]);
      }
    }
    if constexpr (M::FULL0) {
      // static latent dims: the summed input gradient of every evaluation (the direct cotangent of
      // every output time -- they are carried unchanged -- is added by ude_static_tsum_kernel, a
      // coalesced pass over d latent outside this latency-bound loop)
      #pragma unroll 1
      for (int i = tid; i < TT * M::S; i += NTHREADS) {
        const int t = i / M::S, s = i - t * M::S;
        const int n = n0 + t;
        if (n < A.n_traj) {
          const int r = s / (M::L - 3), c = 3 + s - r * (M::L - 3);
          A.dy0[((size_t)n * M::R + r) * M::L + c] = lds[t * SR + M::DYS_OFF + s];
        }
      }
    }
    lds_sync();
    // per-trajectory layer-0 gradient sums -> global (static-feature gradients are
    // computed from them by ude_static_*_kernel); their trajectory sums -> bias row sums
    // (BAYES: layer-0 bias and static columns were accumulated per evaluation instead)
    if constexpr (!M::BAYES && !M::SPLITB) g0_tile_end<M, W>(A, lds, g0t, tile, lane);
    lds_sync();
  }

  // ---- kernel end: register tiles + LDS row sums -> this workgroup's slab ----
  if constexpr (!NO_DW) dw_to_slab<M, W>(dw, dws, myslab, lane);
  // SPLITB: the partner waves' last bias row sums land before this barrier
  if constexpr (M::SPLITB) lds_sync();
  #pragma unroll 1
  for (int i = tid; i < (M::GST ? 0 : M::NDB); i += NTHREADS) {
    myslab[M::SLAB_DB + i] = lds[M::DB_LDS + i];
    if constexpr (M::BAYES) myslab[M::SLAB_TOTAL + M::SLAB_DB + i] = lds[M::DBS_LDS + i];
  }
#ifdef UDE_PROFILE
  if (pf) for (int i = 0; i < NPROF; ++i) A.prof[(size_t)blockIdx.x * NPROF + i] = prof_.acc[i];
#endif
}
// L = 8, 16-B aligned rows: one thread per (n, r) row, whole 32-B rows loaded (both 16-B halves of every
// output time in flight at once, coalesced), the same additions in the same order as the scalar kernel
// below (dy0 first, then output times ascending): bitwise the same dy0.
template <class M>
__global__ __launch_bounds__(256) void ude_static_tsum_rows_kernel(const float* __restrict__ dlatent, int n_traj,
                                                                   int n_times, float* __restrict__ dy0) {
  static_assert(M::L == 8, "row kernel: L = 8");
  const size_t NR = (size_t)n_traj * M::R, NRL = NR * M::L;
  for (size_t nr = (size_t)blockIdx.x * 256 + threadIdx.x; nr < NR; nr += (size_t)gridDim.x * 256) {
    f4* d = reinterpret_cast<f4*>(dy0 + nr * M::L);
    f4 lo = d[0], hi = d[1];
    float v3 = lo[3];
    #pragma unroll 3
    for (int jt = 0; jt < n_times; ++jt) {
      const f4* g = reinterpret_cast<const f4*>(dlatent + (size_t)jt * NRL + nr * M::L);
      v3 += g[0][3];
      hi += g[1];
    }
    lo[3] = v3;
    d[0] = lo;
    d[1] = hi;
  }
}

// FULL0 (Bayesian RHS, static dims in the solve's layer 0): dy0[n, r, c >= 3] += sum_j dlatent[j, n, r, c]
// in output order j (the same additions as one loop after the input-gradient sum).
template <class M>
__global__ __launch_bounds__(256) void ude_static_tsum_kernel(const float* __restrict__ dlatent, int n_traj,
                                                              int n_times, float* __restrict__ dy0) {
  constexpr int SPR = M::L - 3;
  const size_t NRL = (size_t)n_traj * M::R * M::L, total = (size_t)n_traj * M::R * SPR;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t nr = i / SPR;
    const size_t base = nr * M::L + 3 + (i - nr * SPR);
    float v = dy0[base];
    #pragma unroll 4
    for (int jt = 0; jt < n_times; ++jt) v += dlatent[(size_t)jt * NRL + base];
    dy0[base] = v;
  }
}

// SPLIT_BWD partner wave W + 4: the weight gradients of every stage (mlp_backward_dw), on the
// exact barrier sequence of bwd_body's critical-path waves (every lds_sync there has its
// counterpart here, in the same order).
template <class M, int W>
__device__ void bwd_wbody(const KArgs& A, float* lds) {
  constexpr int SR = M::SR_B;
  constexpr int NDWn = M::NDW(W) > 0 ? M::NDW(W) : 1;
  constexpr int NZn = M::NZ(W) > 0 ? M::NZ(W) : 1;
  constexpr int NGn = M::NG(W) > 0 ? M::NG(W) : 1;
  const int lane = threadIdx.x & 63, t16 = lane & 15, g = lane >> 4;
  float* myslab = A.slab + (size_t)blockIdx.x * M::SLAB_STRIDE;
  f4 dw[NDWn], g0t[NZn], gacc[NGn];
#pragma unroll
  for (int i = 0; i < NDWn; ++i) dw[i] = f4zero();
#pragma unroll
  for (int i = 0; i < NGn; ++i) gacc[i] = f4zero();
  __builtin_amdgcn_s_setprio(1);         // as bwd_wbody_l (M1 bwd 4.44 -> 4.38 ms, profiles/r05/ab_partner_prio_m1.txt)
  lds_sync();                            // record zeroed
  // These waves also move the stage data (the critical-path waves issue no global load in the
  // stage loop): each stage's checkpointed input and activation rows, loaded one stage ahead into
  // registers and written into the record at the stage start, and the output cotangents of each
  // step, loaded a stage ahead and folded into the RK adjoint rows.  Their waits are this wave's
  // own, so no wait of the critical path can drain the prefetch.
  const Sched sc(A.sched, A.n_steps, A.n_out);
  const int wt = threadIdx.x - NTHREADS;                // 0..255: the pair / quad index
  constexpr int QR = M::ACT_A4 / 4, NQ = act_q_per_thread<M>();
  f4 actr[NQ];
  float ckr[1][3], gvc[1][3];
  auto put_stage = [&](int tile_) {                     // carried rows -> the record
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      const int i = wt + u * NTHREADS;
      if (i < TT * QR) {
        const int t = i / QR, q = i - t * QR;
        *reinterpret_cast<f4*>(lds + t * SR + M::ACT0 + 4 * q) = actr[u];
      }
    }
    if (wt < M::PAIRS) {
      const int r = wt / TT, t = wt - r * TT;
#pragma unroll
      for (int c = 0; c < 3; ++c) lds[t * SR + M::Y_OFF + 3 * r + c] = ckr[0][c];
    }
  };
  auto get_stage = [&](int tile_, int step_, int jj_) {  // issue one stage's loads
    ckpt_issue<M>(A, tile_, step_, jj_, ckr, wt);
    const f4* src = reinterpret_cast<const f4*>(act_block<M>(A.ckpt, A.n_tiles, A.n_steps, tile_, step_, jj_));
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      const int i = wt + u * NTHREADS;
      if (i < TT * QR) actr[u] = src[act_src_q<M>(i)];
    }
  };
  for (int tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    const int n0 = tile * TT;
    lds_sync();                          // last step's output cotangents staged
#pragma unroll
    for (int i = 0; i < NZn; ++i) g0t[i] = f4zero();
    lds_sync();
    bool have = false;
    for (int step = A.n_steps - 1; step >= 0; --step) {
      #pragma unroll 1
      for (int jj = 3; jj >= 0; --jj) {
        const int nstep = jj > 0 ? step : step - 1, njj = jj > 0 ? jj - 1 : 3;
        if (!have) get_stage(tile, step, jj);           // the tile's first stage
        put_stage(tile);
        lds_sync();                      // stage input + activation rows in the record
        // the rest runs in the flux interval (these waves' MFMA-free wait), not ahead of the
        // stage-input barrier, where its dependent scalar schedule loads delayed the critical path
        if (jj == 0 && nstep >= 0) {
          // step nstep's output cotangents: the y_{n+1} share joins PEND (RK_A of the next step
          // = ACCY + PEND), the y_n share is staged in DK3 (dead at jj == 0; read at the step start)
          float sg[1][3], pg[1][3];
          out_finish<M>(A, sc, nstep, n0, gvc, sg, pg, wt);
          if (wt < M::PAIRS) {
            const int r = wt / TT, t = wt - r * TT;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              lds[t * SR + M::RK_PEND + 3 * r + c] += sg[0][c];
              lds[t * SR + M::RK_DK3 + 3 * r + c] = pg[0][c];
            }
          }
        }
        if (jj == 1 && step > 0) out_issue<M>(A, sc, step - 1, n0, gvc, wt);
        have = nstep >= 0;
        if (have) get_stage(tile, nstep, njj);
        lds_sync();                      // flux pass: final-layer gradients written
        if constexpr (UDE_ABL == 1) { sfor<M::D>([&](auto) { lds_sync(); }); }
        else mlp_backward_dw<M, W, SR>(lds, dw, g0t, gacc, lane);
      }
    }
    lds_sync();                          // tile end: dy0
    lds_sync();
    g0_tile_end<M, W>(A, lds, g0t, tile, lane);
    lds_sync();
  }
  // kernel end: dW tiles -> slab; bias row sums of layers >= 1 from the per-trajectory sums
  f4 none[1];
  dw_to_slab<M, W>(dw, none, myslab, lane);
  sfor<M::D>([&](auto dd) {
    constexpr int d = decltype(dd)::value;
    if constexpr (d > 0) sfor<M::FT(d)>([&](auto kk) {
      constexpr int k = decltype(kk)::value;
      if constexpr (M::fowner(d, k) == W) {
        f4 r = gacc[M::ng_before(W, d, k)];
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = row16_sum(r[e]);
        if (t16 == 0) {
          float* db = lds + M::DB_LDS + (M::FTbase(d) + k) * 16 + g * 4;
          db[0] += r[0]; db[1] += r[1]; db[2] += r[2]; db[3] += r[3];
        }
      }
    });
  });
  lds_sync();                            // bias row sums complete -> bwd_body copies them
}

// SPLIT_BWD_L partner wave W + 4: weight gradients of every stage and the next stage's data
// (LDS-DMA), on the exact barrier sequence of bwd_body's critical-path waves.
template <class M, int W>
__device__ void bwd_wbody_l(const KArgs& A, float* lds) {
  constexpr int SR = M::SR_B;
  constexpr int NDWn = M::NDW(W) > 0 ? M::NDW(W) : 1;
  constexpr int NZn = M::NZ(W) > 0 ? M::NZ(W) : 1;
  int lane = threadIdx.x & 63;
  float* myslab = A.slab + (size_t)blockIdx.x * M::SLAB_STRIDE;
  f4 dw[NDWn], g0t[NZn];
#pragma unroll
  for (int i = 0; i < NDWn; ++i) dw[i] = f4zero();
  // the second-dispatched half of the workgroup at static priority 1 for the whole launch (the
  // arbitration loser otherwise; MI355X_MICROARCH "Two waves per SIMD" item 4): state49 bwd
  // 1.744 -> 1.724 ms (profiles/r05/ab_partner_prio.txt)
  __builtin_amdgcn_s_setprio(1);
  Prof prof_, *pf = nullptr;
#if defined(UDE_PROFILE) && defined(UDE_PROFILE_PARTNER)
  // diagnostic (-DUDE_PROFILE_PARTNER on top of -DUDE_PROFILE): partner wave 4 (W = 0) stamps its own
  // segments into row 2 * PROF_FWD_SLOT + block.  Its stamps perturb the stage far more than the
  // critical path's (s_memtime waits on the partner's LDS traffic): a separate build, for its shares.
  if (W == 0 && A.prof && lane == 0) {
    pf = &prof_;
    for (int i = 0; i < NPROF; ++i) prof_.acc[i] = 0;
    prof_.last = __builtin_amdgcn_s_memtime();
  }
#endif
  lds_sync();                                           // record zeroed
  // staged stage input [f][t] -> Y slot [t][f]: each wave moves exactly the 256-float chunks its own
  // dma_ckpt wrote (its vmcnt wait covers only its own DMAs; the other waves' may still be landing)
  auto put_stage = [&]() {
    constexpr int NF = M::F * TT, NC = (NF + 255) / 256;
#pragma unroll
    for (int c = W; c < NC; c += WAVES)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = c * 256 + e * 64 + lane;
        if (i < NF) lds[(i & 15) * SR + M::Y_OFF + (i >> 4)] = lds[M::STG_LDS + i];
      }
  };
  auto dma_all = [&](int tile_, int step_, int jj_) {
    const Rsrc src = act_rsrc<M>(A, tile_, step_, jj_);
    sfor<2>([&](auto nn) {
      constexpr int net = decltype(nn)::value;
      sfor<M::nl(net)>([&](auto ii) { dma_layer<M, W, net, decltype(ii)::value>(src, lds, lane); });
    });
    dma_ckpt<M, W>(A, lds, tile_, step_, jj_, lane);
  };
  for (int tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    // the tile's first stage: everything at once (nothing of it is in the record yet)
    if (A.n_steps > 0) dma_all(tile, A.n_steps - 1, 3);
    lds_sync_dma();                                     // last step's output cotangents staged
#pragma unroll
    for (int i = 0; i < NZn; ++i) g0t[i] = f4zero();
    lds_sync_dma();
    for (int step = A.n_steps - 1; step >= 0; --step) {
      #pragma unroll 1
      for (int jj = 3; jj >= 0; --jj) {
        const int nstep = jj > 0 ? step : step - 1, njj = jj > 0 ? jj - 1 : 3;
        const bool have = nstep >= 0;
        // lane is opaque per stage: the ~40 lane-derived LDS addresses of the stage (staging copy,
        // operand reads) are recomputed here instead of hoisted out of the loop, where they spilled
        // next to the 176 dW VGPRs and every scratch reload (a vmcnt wait) drained the DMAs in flight
        asm volatile("" : "+v"(lane));
        UDE_STAMP(pf, 13);
        wait_dma();                                     // this stage's rows and input have landed
        UDE_STAMP(pf, 0);
        put_stage();
        UDE_STAMP(pf, 2);
        lds_sync_dma();                                 // stage input + activation rows in the record
        UDE_STAMP(pf, 1);
        if (have) dma_ckpt<M, W>(A, lds, tile, nstep, njj, lane);   // staging slot free again
        UDE_STAMP(pf, 3);
        lds_sync_dma();                                 // flux pass: final-layer gradients written
        UDE_STAMP(pf, 16);
        UDE_STAMP(pf, 17);
        mlp_backward_dw_l<M, W, SR>(lds, dw, g0t, lane, [&](auto dd) {
          constexpr int d = decltype(dd)::value;
          if constexpr (d >= 1)
            if (have) dma_freed<M, W, d>(act_rsrc<M>(A, tile, nstep, njj), lds, lane);
        }, pf);
      }
    }
    lds_sync_dma();                                     // tile end: dy0
    lds_sync_dma();
    g0_tile_end<M, W>(A, lds, g0t, tile, lane);
    lds_sync_dma();
    UDE_STAMP(pf, 15);
  }
  wait_dma();
  f4 none[1];
  dw_to_slab<M, W>(dw, none, myslab, lane);
  lds_sync();                                           // bias row sums complete -> bwd_body copies them
#ifdef UDE_PROFILE
  if (pf) for (int i = 0; i < NPROF; ++i) A.prof[(size_t)(2 * PROF_FWD_SLOT + blockIdx.x) * NPROF + i] = prof_.acc[i];
#endif
}

template <class M>
__global__ __launch_bounds__(M::BWD_THREADS) void ude_bwd_kernel(KArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if constexpr (M::SPLIT_BWD) {
    if (w >= WAVES) {
      if (w == 4) bwd_wbody<M, 0>(a, lds);
      else if (w == 5) bwd_wbody<M, 1>(a, lds);
      else if (w == 6) bwd_wbody<M, 2>(a, lds);
      else bwd_wbody<M, 3>(a, lds);
      return;
    }
  }
  if constexpr (M::SPLIT_BWD_L) {
    if (w >= WAVES) {
      if (w == 4) bwd_wbody_l<M, 0>(a, lds);
      else if (w == 5) bwd_wbody_l<M, 1>(a, lds);
      else if (w == 6) bwd_wbody_l<M, 2>(a, lds);
      else bwd_wbody_l<M, 3>(a, lds);
      return;
    }
  }
  if (w == 0) bwd_body<M, 0>(a, lds);
  else if (w == 1) bwd_body<M, 1>(a, lds);
  else if (w == 2) bwd_body<M, 2>(a, lds);
  else bwd_body<M, 3>(a, lds);
}

}  // namespace ude
