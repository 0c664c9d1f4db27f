// Aggregates of an ensemble forecast (no model): weighted sums over the regions, trajectory by trajectory, for
// every level of a hierarchy at once -- the HHS regions and the nation of the state model.  A level is a weight
// matrix (G_l, R); the levels' rows are stacked into w (G_tot, R), g_off[l] the first row of level l.  For a row
// rho of R consecutive fp32 values (a (t, n) of y_hat, a (b, t) of y_true, a (t, n) of a dynamics plane) and a
// stacked row g: acc = 0, then acc = acc + w[g, r] * v_r for r ascending in fp64, every product and every sum
// rounded on its own (no fused multiply-add), stored as (float)acc.  The formulas are at ude_forecast_aggregate
// and ude_forecast_aggregate_dyn in include/ude_rk4.h.
//
// Thread-to-work mapping, ude_forecast_aggregate_kernel<F, NACC>.  A 256-thread workgroup owns tiles of AG_ROWS
// = 64 consecutive rows (tile t = blockIdx.x, then + gridDim.x).  Lane l of every wave owns row l of the tile;
// wave v owns per = ceil(gp / 4) consecutive stacked rows g = gb + v per + j, j < per <= NACC, of the pass's gp =
// min(G_tot - gb, 4 NACC) stacked rows: a thread holds NACC x F::NP fp64 accumulators in registers (NACC = 4, 16
// or 64 by G_tot, chosen at launch; indices are static after unrolling).  The regions are walked in chunks of CW
// = 63 / NP (an odd number) with the accumulators carried, so the order stays r ascending: the chunk of the
// tile -- nr rows x cw regions, for cw = R one contiguous span of the input -- is loaded coalesced by all 256
// threads into LDS as the functor's fp64 values with a row stride of CW doubles (odd: the 32 lanes of a
// ds_read_b64 group, which own consecutive rows, hit distinct bank pairs), then every thread reads its row's
// v_r once per r and adds w[g, r] v_r to its accumulators; w[g, r] is wave-uniform (the wave index comes through
// readfirstlane), a scalar load.  After the last chunk the outputs go through the same LDS as floats, [row][g of
// the pass] (AG_STAGE_G stacked rows at a time, odd row stride), and are written level by level: a level's
// (rows, G_l) block of the tile is one contiguous run of nr G_l floats when the level lies inside the pass.
// With G_tot <= 4 NACC there is one pass and every input element is read exactly once, for all levels together;
// that holds for the prediction kernel always (NACC = 64 covers G_tot = 256).
//
// The functor F gives the fp64 values of a region: AgPlain v = (double)x * scale (NP = 1, one output; without
// a scale another instantiation);
// AgRates s, i, (beta s) i, gamma i from four planes of dyn (NP = 4) and at the end the outputs s, i, beta =
// inc / (s i), gamma = rec / i, r_eff = inc / rec from the four fp64 sums, each rounded once to fp32.  The other
// planes of dyn (r, fa_*) are plain sums: ude_forecast_aggregate_dyn launches AgRates for the rate planes and
// AgPlain over the others taken as further rows (a level's (C, rows, G_l) block is (C rows, G_l)), so every
// plane but the unused r_eff is read exactly once.  AgRates keeps 4 NACC accumulators, NACC <= 16: a hierarchy
// of more than 64 stacked rows takes ceil(G_tot / 64) passes over its four planes.
//
// No workspace, no atomics, nothing in the geometry depends on values: the same bits run to run.  LDS 31.5 KiB
// static (five workgroups per CU).
#pragma once
#include "ude_forecast.h"

namespace ude {

constexpr int AG_ROWS = 64;                    // rows of a tile: one per lane
constexpr int AG_WAVES = 4;
constexpr int AG_LD = 63;                      // doubles of LDS per tile row, over the functor's planes
constexpr int AG_TILE = AG_ROWS * AG_LD;       // doubles of the tile
constexpr int AG_STAGE_G = 124;                // stacked rows staged per round: 64 x 125 floats fit the tile
constexpr int AG_MAX_R = 4096;
constexpr int AG_MAX_G = 256;
constexpr int AG_MAX_LEVELS = 16;
constexpr int AG_MAX_GRID = 65536;             // workgroups of a launch; further tiles by stride
#ifndef AG_LOADS
#define AG_LOADS 4                             // elements a thread has in flight while it loads the tile
#endif
#ifndef AG_K_UNROLL
#define AG_K_UNROLL 4                          // regions per round of LDS and scalar loads
#endif

typedef __attribute__((address_space(4))) double AgConstDouble;

struct AgArgs {
  const float* x;        // (rows, R); AgRates: plane 0 of dyn (C, rows, R)
  const double* scale;   // (R,) or null (AgPlain)
  const double* w;       // (G_tot, R)
  float* out;
  long long rows;        // rows of x
  long long lvl_stride;  // floats of out per stacked row: level l's block starts at lvl_stride * g_off[l]
  long long row0;        // row of a level's block that input row 0 goes to
  int R, n_levels, G_tot;
  int g_off[AG_MAX_LEVELS + 1];
};

template <bool SCALED>
struct AgPlain {
  static constexpr int NP = 1, NOUT = 1;
  __device__ static __forceinline__ void load(const AgArgs& a, size_t idx, int r, double* v) {
    v[0] = (double)a.x[idx];
    if constexpr (SCALED) v[0] = v[0] * a.scale[r];
  }
  __device__ static __forceinline__ float out(const double* s, int) { return (float)s[0]; }
  __device__ static __forceinline__ int chan(int) { return 0; }
};

// planes s (0), i (1), beta (3), gamma (4) of dyn -> sums of s, i, inc = (beta s) i, rec = gamma i
struct AgRates {
  static constexpr int NP = 4, NOUT = 5;
  __device__ static __forceinline__ void load(const AgArgs& a, size_t idx, int, double* v) {
    const size_t plane = (size_t)a.rows * a.R;
    const double s = (double)a.x[idx], i = (double)a.x[idx + plane];
    const double beta = (double)a.x[idx + 3 * plane], gamma = (double)a.x[idx + 4 * plane];
    v[0] = s;
    v[1] = i;
    v[2] = (beta * s) * i;
    v[3] = gamma * i;
  }
  __device__ static __forceinline__ float out(const double* s, int o) {
    switch (o) {
      case 0: return (float)s[0];
      case 1: return (float)s[1];
      case 2: return (float)(s[2] / (s[0] * s[1]));
      case 3: return (float)(s[3] / s[1]);
      default: return (float)(s[2] / s[3]);
    }
  }
  __device__ static __forceinline__ int chan(int o) { return o < 2 ? o : o + 1; }   // s, i, beta, gamma, r_eff
};

template <class F, int NACC>
__global__ __launch_bounds__(256) void ude_forecast_aggregate_kernel(AgArgs a) {
  constexpr int NP = F::NP;
  constexpr int CW = (AG_LD / NP) % 2 ? AG_LD / NP : AG_LD / NP - 1;   // regions of a chunk = LDS row stride: odd
  constexpr int PLANE = AG_ROWS * CW;
  static_assert(NP * PLANE <= AG_TILE && AG_ROWS * (AG_STAGE_G | 1) <= 2 * AG_TILE, "the tile holds both");
  __shared__ double tile[AG_TILE];
  __shared__ int goff[AG_MAX_LEVELS + 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int R = a.R;
  if (tid == 0) {
#pragma unroll
    for (int l = 0; l <= AG_MAX_LEVELS; ++l) goff[l] = a.g_off[l];
  }
  const long long n_tiles = (a.rows + AG_ROWS - 1) / AG_ROWS;
  for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const long long rho0 = t * AG_ROWS;
    const int nr = (int)min((long long)AG_ROWS, a.rows - rho0);
    for (int gb = 0; gb < a.G_tot; gb += AG_WAVES * NACC) {
      const int gp = min(a.G_tot - gb, AG_WAVES * NACC);
      const int per = (gp + AG_WAVES - 1) / AG_WAVES;
      const int ng = max(0, min(per, gp - wv * per));   // this wave's stacked rows: gb + wv per + j, j < ng
      double acc[NACC][NP];
#pragma unroll
      for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[j][p] = 0.0;

      for (int c0 = 0; c0 < R; c0 += CW) {
        const int cw = min(CW, R - c0);
        __syncthreads();                         // the previous chunk, or the staged outputs, have been read
        {
          // element e = row cw + k of the chunk, e = tid, tid + 256, ..: (row, k) advance without a division
          const int n = nr * cw, dq = 256 / cw, dr = 256 - dq * cw;
          int row = tid / cw, k = tid - row * cw;
          for (int e = tid; e < n; e += 256 * AG_LOADS) {   // AG_LOADS elements in flight per thread
            double v[AG_LOADS][NP];
            int at[AG_LOADS];
#pragma unroll
            for (int u = 0; u < AG_LOADS; ++u) {
              // past the chunk: the tile's first element once more (no branch around a load), not stored
              const bool live = e + 256 * u < n;
              const int lr = live ? row : 0, lk = live ? k : 0;
              at[u] = row * CW + k;
              F::load(a, (size_t)(rho0 + lr) * R + c0 + lk, c0 + lk, v[u]);
              row += dq;
              k += dr;
              if (k >= cw) { k -= cw; ++row; }
            }
#pragma unroll
            for (int u = 0; u < AG_LOADS; ++u) {
              if (e + 256 * u < n) {
#pragma unroll
                for (int p = 0; p < NP; ++p) tile[p * PLANE + at[u]] = v[u][p];
              }
            }
          }
        }
        __syncthreads();
        if (ng > 0) {                            // rows past nr sum what the tile holds; they are not written
          const double* tp = tile + lane * CW;
          // through the constant address space: the wave-uniform address then takes the scalar path
          const AgConstDouble* wr = (const AgConstDouble*)(uintptr_t)(a.w + (size_t)(gb + wv * per) * R + c0);
#pragma unroll AG_K_UNROLL
          for (int k = 0; k < cw; ++k) {
            double v[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) v[p] = tp[p * PLANE + k];
#pragma unroll
            for (int j0 = 0; j0 < NACC; j0 += 4) {
              if (j0 < ng) {
#pragma unroll
                for (int j = j0; j < j0 + 4; ++j) {
                  const double wg = wr[(size_t)min(j, ng - 1) * R + k];   // j >= ng: a sum nobody reads
#pragma unroll
                  for (int p = 0; p < NP; ++p) acc[j][p] = acc[j][p] + wg * v[p];
                }
              }
            }
          }
        }
      }

      float* st = reinterpret_cast<float*>(tile);
#pragma unroll
      for (int o = 0; o < F::NOUT; ++o) {
        for (int s0 = 0; s0 < gp; s0 += AG_STAGE_G) {
          const int sw = min(AG_STAGE_G, gp - s0), sld = sw | 1;
          __syncthreads();                       // the tile, or the previous round, has been read
#pragma unroll
          for (int j = 0; j < NACC; ++j) {
            const int gi = wv * per + j - s0;
            if (j < ng && gi >= 0 && gi < sw) st[lane * sld + gi] = F::out(acc[j], o);
          }
          __syncthreads();
          const int ga = gb + s0, gz = ga + sw;  // the stacked rows of this round
          for (int l = 0; l < a.n_levels; ++l) {
            const int la = goff[l], G = goff[l + 1] - la;
            const int ca = max(la, ga), wd = min(la + G, gz) - ca;
            if (wd <= 0) continue;
            float* dst = a.out + a.lvl_stride * la + (a.row0 + F::chan(o) * a.rows + rho0) * G + (ca - la);
            const float* src = st + (ca - ga);
            const int n = nr * wd;
            for (int e = tid; e < n; e += 256) {
              const int row = e / wd, c = e - row * wd;
              dst[(size_t)row * G + c] = src[row * sld + c];
            }
          }
        }
      }
    }
  }
}

// G_tot, or 0 when the shape is out of range
inline int ag_total(int64_t rows, int R, int n_levels, const int32_t* g_off) {
  if (rows < 0 || R < 1 || R > AG_MAX_R || n_levels < 1 || n_levels > AG_MAX_LEVELS || !g_off || g_off[0] != 0)
    return 0;
  for (int l = 0; l < n_levels; ++l)
    if (g_off[l + 1] <= g_off[l]) return 0;
  return g_off[n_levels] > AG_MAX_G ? 0 : g_off[n_levels];
}

template <class F>
inline int ag_launch(const AgArgs& a, hipStream_t s) {
  const long long n_tiles = (a.rows + AG_ROWS - 1) / AG_ROWS;
  const dim3 grid((unsigned)(n_tiles < AG_MAX_GRID ? n_tiles : AG_MAX_GRID));
  const int per = (a.G_tot + AG_WAVES - 1) / AG_WAVES;
  if (per <= 4) {
    hipLaunchKernelGGL((ude_forecast_aggregate_kernel<F, 4>), grid, dim3(256), 0, s, a);
  } else if (per <= 16 || F::NP > 1) {
    hipLaunchKernelGGL((ude_forecast_aggregate_kernel<F, 16>), grid, dim3(256), 0, s, a);
  } else {
    if constexpr (F::NP == 1) hipLaunchKernelGGL((ude_forecast_aggregate_kernel<F, 64>), grid, dim3(256), 0, s, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

inline AgArgs ag_args(int64_t rows, int R, int n_levels, const int32_t* g_off, int G_tot, const double* w, float* out) {
  AgArgs a = {};
  a.w = w; a.out = out; a.rows = rows; a.lvl_stride = rows; a.R = R; a.n_levels = n_levels; a.G_tot = G_tot;
  for (int l = 0; l <= AG_MAX_LEVELS; ++l) a.g_off[l] = g_off[l < n_levels ? l : n_levels];
  return a;
}

inline int forecast_aggregate(int64_t rows, int R, int n_levels, const int32_t* g_off, const float* x,
                              const double* scale, const double* w, float* out, hipStream_t s) {
  const int G_tot = ag_total(rows, R, n_levels, g_off);
  if (!G_tot || !x || !w || !out) return -2;
  if (rows == 0) return 0;
  AgArgs a = ag_args(rows, R, n_levels, g_off, G_tot, w, out);
  a.x = x;
  a.scale = scale;
  return scale ? ag_launch<AgPlain<true>>(a, s) : ag_launch<AgPlain<false>>(a, s);
}

// kind: UDE_KIND_FP / _FA / _FAFP, the Bayes bit (4) ignored.  C = 3 + 3 [rate net] + 3 [augmentation net]
inline int forecast_aggregate_dyn(int kind, int64_t rows, int R, int n_levels, const int32_t* g_off, const float* dyn,
                                  const double* w, float* out, hipStream_t s) {
  const int G_tot = ag_total(rows, R, n_levels, g_off);
  const int k = kind & ~4;
  if (!G_tot || k < 1 || k > 3 || !dyn || !w || !out) return -2;
  if (rows == 0) return 0;
  const bool rates = k & 1, flux = k & 2;
  const int C = 3 + (rates ? 3 : 0) + (flux ? 3 : 0);
  const size_t plane = (size_t)rows * R;
  AgArgs a = ag_args(rows, R, n_levels, g_off, G_tot, w, out);
  a.lvl_stride = (long long)C * rows;
  // planes c0 .. c0 + n - 1 as n rows more rows of a plain sum
  auto plain = [&](int c0, int n) {
    AgArgs b = a;
    b.x = dyn + (size_t)c0 * plane;
    b.rows = (long long)n * rows;
    b.row0 = (long long)c0 * rows;
    return ag_launch<AgPlain<false>>(b, s);
  };
  if (!rates) return plain(0, 6);                // s, i, r, fa_s, fa_i, fa_r
  a.x = dyn;
  int rc = ag_launch<AgRates>(a, s);             // s, i, beta, gamma, r_eff
  if (rc == 0) rc = plain(2, 1);                 // r
  if (rc == 0 && flux) rc = plain(6, 3);         // fa_s, fa_i, fa_r
  return rc;
}

}  // namespace ude
