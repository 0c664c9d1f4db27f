// Weight packing: the nets' parameters -> the kernels' MFMA fragment order (ude_pack_kernel), and the decoder's
// (ude_dec_pack_kernel).
#pragma once
#include "ude_kernels_core.h"

namespace ude {

// ============================================================================
// Weight packing (one launch, blockIdx.y = segment)
// ============================================================================
struct PackPtrs {
  const float* W[2][5];
  const float* b[2][5];
  const float* Ws[2][5];   // BAYES: w_std / b_std (|.| is taken here, models_bayes.py:45-46)
  const float* bs[2][5];
  const float* eps;        // BAYES: [eval][N_PARAMS] in torch parameter order
};

template <class M>
__device__ __forceinline__ int static_col(int s) {
  const int r = s / (M::L - 3);
  return r * M::L + 3 + (s - r * (M::L - 3));
}

// One launch packs every segment (blockIdx.y) of one weight set; BAYES: blockIdx.z =
// evaluation, whose sample w = mu + eps * |std| (the reference's fp32 op order) is
// packed PACK_TOTAL floats after the previous one's.
template <class M>
__global__ __launch_bounds__(256) void ude_pack_kernel(PackPtrs P, float* __restrict__ pack) {
  const int seg = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const size_t ev = M::BAYES ? blockIdx.z : 0;
  pack += ev * M::PACK_TOTAL;
  sfor<2>([&](auto nn) {
    constexpr int net = decltype(nn)::value;
    sfor<5>([&](auto ii) {
      constexpr int i = decltype(ii)::value;
      if constexpr (M::has(net, i)) {
        constexpr int base = (net * 5 + i) * 3;
        constexpr int in = M::in_dim(net, i), out = M::out_dim(net, i);
        constexpr int in_full = i == 0 ? M::R * M::L : in;
        const float* Wp = P.W[net][i];
        auto wval = [&](int o, int f) -> float {
          const int col = i == 0 ? M::col0(f) : (f < in ? f : -1);
          if (o >= out || col < 0) return 0.f;
          const size_t w = (size_t)o * in_full + col;
          float v = Wp[w];
          if constexpr (M::BAYES) v = v + P.eps[ev * M::N_PARAMS + M::param_w_off(net, i) + w] * fabsf(P.Ws[net][i][w]);
          return v;
        };
        if (seg == base + 0 && idx < M::wf_size(net, i)) {
          constexpr int KQ = M::kin(net, i) / 4, NQ = M::kin(net, i) / 16;
          const int e = idx & 3, ln = (idx >> 2) & 63, q = (idx >> 8) % NQ, rt = (idx >> 8) / NQ;
          pack[M::wf_off(net, i) + idx] = wval(rt * 16 + (ln & 15), (ln >> 4) * KQ + 4 * q + e);
        } else if (seg == base + 1 && idx < M::wt_size(net, i)) {
          constexpr int KQ = M::kout(net, i) / 4, NQ = M::kout(net, i) / 16;
          const int e = idx & 3, ln = (idx >> 2) & 63, q = (idx >> 8) % NQ, rt = (idx >> 8) / NQ;
          pack[M::wt_off(net, i) + idx] = wval((ln >> 4) * KQ + 4 * q + e, rt * 16 + (ln & 15));
        } else if (seg == base + 2 && idx < M::b_size(net, i)) {
          float v = 0.f;
          if (idx < out) {
            v = P.b[net][i][idx];
            if constexpr (M::BAYES)
              v = v + P.eps[ev * M::N_PARAMS + M::param_w_off(net, i) + out * in_full + idx] * fabsf(P.bs[net][i][idx]);
          }
          pack[M::b_off(net, i) + idx] = v;
        }
      }
    });
    if constexpr (M::HOIST && M::has(net, 0)) {
      if (seg == 30 + net && idx < M::wsf_size(net)) {
        constexpr int KQ = M::S16 / 4, NQ = M::S16 / 16;
        constexpr int out = M::out_dim(net, 0);
        const int e = idx & 3, ln = (idx >> 2) & 63, q = (idx >> 8) % NQ, rt = (idx >> 8) / NQ;
        const int o = rt * 16 + (ln & 15), s = (ln >> 4) * KQ + 4 * q + e;
        pack[M::wsf_off(net) + idx] =
            (o < out && s < M::S) ? P.W[net][0][(size_t)o * M::R * M::L + static_col<M>(s)] : 0.f;
      }
    }
  });
  if constexpr (M::HOIST) {
    if (seg == 32 && idx < M::W0SP_SIZE) {
      // plain [merged layer-0 row][static feature] copy (dy0 static kernel)
      int om = idx / M::S16;
      const int s = idx - om * M::S16;
      int net = 0;
      if (!M::HAS_P || om >= (M::HAS_P ? M::kout(0, 0) : 0)) {
        net = 1;
        om -= M::HAS_P ? M::kout(0, 0) : 0;
      }
      const int out = M::out_dim(net, 0);
      float v = 0.f;
      if (s < M::S && om < out && (net == 0 ? M::HAS_P : M::HAS_A))
        v = P.W[net][0][(size_t)om * M::R * M::L + static_col<M>(s)];
      pack[M::W0SP_OFF + idx] = v;
    }
  }
}

// Decoder Linear(3R -> R) (lib/models.py:39) -> the DEC epilogue's fragment layout (Model::DEC_PACK).
template <class M>
__global__ __launch_bounds__(256) void ude_dec_pack_kernel(const float* __restrict__ Wd, const float* __restrict__ bd,
                                                           float* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < M::DEC_WF) {
    constexpr int KQ = M::F16 / 4, NQ = M::F16 / 16;
    const int e = idx & 3, ln = (idx >> 2) & 63, q = (idx >> 8) % NQ, rt = (idx >> 8) / NQ;
    const int o = rt * 16 + (ln & 15), f = (ln >> 4) * KQ + 4 * q + e;
    out[idx] = (o < M::R && f < M::F) ? Wd[(size_t)o * M::F + f] : 0.f;
  } else if (idx < M::DEC_PACK) {
    const int o = idx - M::DEC_WF;
    out[idx] = o < M::R ? bd[o] : 0.f;
  }
}

}  // namespace ude
