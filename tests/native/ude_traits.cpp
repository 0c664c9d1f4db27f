// Host print of the compile-time traits csrc/ude_model.h derives for one model configuration
// (tests/lattice_helpers.py, tests/test_config_lattice.py).  Includes only ude_model.h:
//   g++ -std=c++17 -I <csrc> -DUDE_ONE_CONFIG=R,L,KIND,NPH,P0,P1,P2,P3,NAH,A0,A1,A2,A3 ude_traits.cpp
// One "NAME value" line per trait.  A configuration whose record does not fit fails the header's
// static_assert here exactly as it does in the gfx950 build.
#include <cstdio>

#include "ude_model.h"

#define UDE_MODEL_X(...) ude::Model<__VA_ARGS__>
using M = UDE_MODEL_X(UDE_ONE_CONFIG);
using MR = ude::Recompute<M>;

#define P(name) std::printf(#name " %d\n", int(M::name))

int main() {
  P(R); P(L); P(KIND); P(D); P(F); P(F16); P(S16); P(K0);
  P(SLOTS); P(HOIST); P(FULL0); P(BAYES); P(GST);
  P(STORE_ACT); P(STORE_ACT_D); P(SPLIT_FWD); P(SPLIT_BWD); P(SPLIT_BWD_L);
  P(SPLITX0); P(DYF); P(WREG); P(FWD_RES); P(FWD_PFB);
  P(ACT_A4); P(LDS_F); P(LDS_B); P(N_PARAMS);
  std::printf("MAX_WREG_Q %d\n", M::max_wreg_q());
  std::printf("MAX_NDW %d\n", M::max_ndw());
  std::printf("RECOMPUTE_LDS_B %d\n", int(MR::LDS_B));
  return 0;
}
