// The model's equations, once: the SIR right-hand side the nets drive (lib/models.py:130-150) and
// its VJP, as the fused RK4, dopri5 and single-evaluation kernels all evaluate them.
//   beta = |q0|, gamma = |q1|                      (q: the rate net's final-layer outputs)
//   plus = (beta S) I, minus = gamma I,  f = (-plus, plus - minus, minus)
//   f += fa_w Fa  (FaFp)  /  f = Fa  (Fa only)    (Fa: the augmentation net's outputs)
//   f[c] = 0 where Y[c] lies outside [-1, 2]
//   r_eff = (beta S) / gamma
// Plain fp32 on values (scalars and float[3]); no intrinsics, no LDS, no Model<>.  The functions are
// per step and per component, so each kernel keeps its own loads, stores, vector widths and statistic
// sums between them, and adds its own direct cotangents of beta / gamma for the pairs that exist.
// The sequence flux -> + fa_w Fa -> mask is therefore composed by each forward caller (fwd_body,
// dopri_body, eval_f_pairs, eval_fwd_body, tests/native/ude_sir_host.cpp): a change to the order of
// those steps or to the number of components is still made at each of them.
// The operation order of every expression is fixed: the kernels are built with -ffp-contract=off,
// so a host compile of this header gives the device's bits (tests/test_sir_host.py), and the RK4
// forward is pinned bit for bit against an independent restatement (oracle/ude_korder.c, which
// must not include this file).
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define UDE_SIR_FN __host__ __device__ __forceinline__
#else
#define UDE_SIR_FN inline
#endif

namespace ude {

// the state component y is outside the model's domain: its derivative (and cotangent) is cut
UDE_SIR_FN bool sir_masked(float y) { return y > 2.f || y < -1.f; }
// beta, gamma from the rate net's outputs
UDE_SIR_FN void sir_rates(float q0, float q1, float& b, float& gm) { b = fabsf(q0); gm = fabsf(q1); }
UDE_SIR_FN float sir_r_eff(float b, float s, float gm) { return (b * s) / gm; }

// the flux of one (trajectory, region) pair at (S, I) = (y0, y1); b / gm: its rates, unmasked
UDE_SIR_FN void sir_flux(float y0, float y1, float q0, float q1, float (&f)[3], float& b, float& gm) {
  sir_rates(q0, q1, b, gm);
  const float plus = (b * y0) * y1;
  const float minus = gm * y1;
  f[0] = -plus; f[1] = plus - minus; f[2] = minus;
}

// the raw Fa[c] enters the flux's f[c] with weight fa_w (FaFp, HAS_P) or is the right-hand side (Fa only)
template <bool HAS_P>
UDE_SIR_FN void sir_add_fa(float& f, float fa_w, float fa) { f = HAS_P ? f + fa_w * fa : fa; }

// cotangent of Fa[c] from the masked cotangent dres of f[c], plus the caller's direct cotangent of Fa
template <bool HAS_P>
UDE_SIR_FN float sir_fa_cot(bool live, float fa_w, float dres, float extra) {
  const float d = HAS_P ? fa_w * dres : dres;
  return live ? d + extra : 0.f;
}

// VJP of the flux: from the masked cotangents dres of f to those of beta, gamma and the direct part of (S, I)'s
UDE_SIR_FN void sir_flux_vjp(float y0, float y1, float b, float gm, const float (&dres)[3], float& dbeta, float& dgam,
                             float& dyf0, float& dyf1) {
  const float dplus = dres[1] - dres[0];
  const float dminus = dres[2] - dres[1];
  const float dpi = dplus * y1;                     // d(beta*S)
  dbeta = dpi * y0;
  dyf0 = dpi * b;
  dyf1 = dplus * (b * y0) + dminus * gm;
  dgam = dminus * y1;
}
// cotangent of q from the cotangent d of |q|: zero at zero
UDE_SIR_FN float sir_abs_cot(float q, float d) { return q > 0.f ? d : (q < 0.f ? -d : 0.f); }

}  // namespace ude
