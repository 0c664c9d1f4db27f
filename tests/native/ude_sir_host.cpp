// Host compile of csrc/ude_sir.h for tests/test_sir_host.py: the header's functions looped over
// arrays, for the three model kinds (1 Fp, 2 Fa, 3 FaFp; configs.KIND_CODE).  Built with
//   g++ -O2 -ffp-contract=off -fno-fast-math -fPIC -shared -I <csrc>
// so every expression rounds as the kernels' (-ffp-contract=off) do.
#include "ude_sir.h"

namespace {

template <bool HAS_P, bool HAS_A>
void rhs_rows(int n, const float* Y, const float* q, const float* fa, float fa_w, float* f, float* rates,
              float* r_eff, int* masked) {
  for (int i = 0; i < n; ++i) {
    const float y[3] = {Y[3 * i], Y[3 * i + 1], Y[3 * i + 2]};
    // the kernels' forward: rates, flux, + Fa per component, mask
    float o[3] = {0.f, 0.f, 0.f};
    if (HAS_P) {
      float b, gm;
      ude::sir_flux(y[0], y[1], q[2 * i], q[2 * i + 1], o, b, gm);
      rates[2 * i] = b;
      rates[2 * i + 1] = gm;
      r_eff[i] = ude::sir_r_eff(b, y[0], gm);
    }
    for (int c = 0; c < 3; ++c) {
      if (HAS_A) ude::sir_add_fa<HAS_P>(o[c], fa_w, fa[3 * i + c]);
      masked[3 * i + c] = ude::sir_masked(y[c]) ? 1 : 0;
      f[3 * i + c] = ude::sir_masked(y[c]) ? 0.f : o[c];
    }
  }
}

template <bool HAS_P, bool HAS_A>
void vjp_rows(int n, const float* Y, const float* q, const float* cot_f, const int* live, const float* extra_rates,
              const float* extra_fa, float fa_w, float* dres, float* dq, float* dyf, float* dfa) {
  for (int i = 0; i < n; ++i) {
    const bool lv = live[i] != 0;
    float dr[3];
    for (int c = 0; c < 3; ++c) {
      dr[c] = (!lv || ude::sir_masked(Y[3 * i + c])) ? 0.f : cot_f[3 * i + c];
      dres[3 * i + c] = dr[c];
      if (HAS_A) dfa[3 * i + c] = ude::sir_fa_cot<HAS_P>(lv, fa_w, dr[c], extra_fa[3 * i + c]);
    }
    if (HAS_P) {
      float b, gm, dbeta, dgam;
      ude::sir_rates(q[2 * i], q[2 * i + 1], b, gm);
      ude::sir_flux_vjp(Y[3 * i], Y[3 * i + 1], b, gm, dr, dbeta, dgam, dyf[2 * i], dyf[2 * i + 1]);
      // the callers' direct cotangents of beta / gamma, for the pairs that exist
      dq[2 * i] = ude::sir_abs_cot(q[2 * i], lv ? dbeta + extra_rates[2 * i] : 0.f);
      dq[2 * i + 1] = ude::sir_abs_cot(q[2 * i + 1], lv ? dgam + extra_rates[2 * i + 1] : 0.f);
    }
  }
}

}  // namespace

extern "C" {

// f (n, 3), rates (n, 2), r_eff (n), masked (n, 3) of n rows (Y (n, 3), q (n, 2), fa (n, 3))
int ude_sir_host_rhs(int kind, int n, const float* Y, const float* q, const float* fa, float fa_w, float* f,
                     float* rates, float* r_eff, int* masked) {
  if (kind == 1) rhs_rows<true, false>(n, Y, q, fa, fa_w, f, rates, r_eff, masked);
  else if (kind == 2) rhs_rows<false, true>(n, Y, q, fa, fa_w, f, rates, r_eff, masked);
  else if (kind == 3) rhs_rows<true, true>(n, Y, q, fa, fa_w, f, rates, r_eff, masked);
  else return -1;
  return 0;
}

// the masked cotangent dres (n, 3), dq (n, 2), the direct (dS, dI) part dyf (n, 2) and dfa (n, 3) from the
// cotangent cot_f (n, 3) of f, live (n) and the callers' direct cotangents of the rates (n, 2) and of Fa (n, 3)
int ude_sir_host_vjp(int kind, int n, const float* Y, const float* q, const float* cot_f, const int* live,
                     const float* extra_rates, const float* extra_fa, float fa_w, float* dres, float* dq, float* dyf,
                     float* dfa) {
  if (kind == 1) vjp_rows<true, false>(n, Y, q, cot_f, live, extra_rates, extra_fa, fa_w, dres, dq, dyf, dfa);
  else if (kind == 2) vjp_rows<false, true>(n, Y, q, cot_f, live, extra_rates, extra_fa, fa_w, dres, dq, dyf, dfa);
  else if (kind == 3) vjp_rows<true, true>(n, Y, q, cot_f, live, extra_rates, extra_fa, fa_w, dres, dq, dyf, dfa);
  else return -1;
  return 0;
}

}  // extern "C"
