/*
 * ude_rk4.h -- C-ABI of the MI355X (gfx950) UDE RK4 solver library.
 *
 * Drop-in boundary for the reference's hot path:
 *   torchdiffeq.odeint(ode, z, t, method='rk4', options=dict(step_size=h))
 *   called at lib/VAE.py:137 (and tuning/tune_encoders.py:221,
 *   tuning/tune_node.py:204, tuning/tune_Fp.py:93), with `ode` one of the
 *   right-hand sides Fp / Fa / FaFp of lib/models.py:109-265, plus the
 *   autograd backward through that solve that lib/VAE.py:203
 *   (`loss.backward()`) triggers, and the side statistics the loss reads:
 *   ode.posterior() (lib/models.py:152-156, lib/VAE.py:173) and
 *   torch.norm(torch.stack(ode.tracker)) (lib/VAE.py:180).
 *
 * Conventions
 *   - every pointer is a device pointer (HBM) unless stated; the caller owns
 *     every buffer, sized by ude_query(); the library never allocates and
 *     keeps no state between calls (re-entrant, stream ordered);
 *   - y0 / latent / dlatent / dy0 are row-major (..., N, R, L) fp32 exactly as
 *     a contiguous torch tensor; weights are nn.Linear layout (out, in);
 *   - return value 0 = ok, < 0 = error (UDE_E_*); the Python layer raises.
 */
#ifndef UDE_RK4_H
#define UDE_RK4_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* ude_stream_t; /* == hipStream_t */

enum {
  UDE_OK = 0,
  UDE_E_UNSUPPORTED = -1, /* no compiled kernel for this model description */
  UDE_E_INVALID = -2,     /* bad argument (sizes, null pointers)            */
  UDE_E_HIP = -3,         /* a HIP runtime call failed                      */
  UDE_E_SOLVER = -4       /* adaptive solve failed (see UdeDopriInfo.status) */
};

/* kind: Fp / Fa / FaFp, optionally | UDE_KIND_BAYES for the Bayesian right-hand
 * sides Bayes_Fp / Bayes_Fa / Bayes_FaFp of lib/in_development/models_bayes.py
 * (:69-265), whose Dense_Variational layers (:12-48) draw a fresh weight sample
 * w = w_mean + eps * |w_std| at every evaluation. */
enum { UDE_KIND_FP = 1, UDE_KIND_FA = 2, UDE_KIND_FAFP = 3, UDE_KIND_BAYES = 4 };

/* The RHS module: lib/models.py FaFp(n_regions, latent_dim, net_sizes,
 * aug_net_sizes) etc.  Hidden-size lists of up to 4 entries. */
typedef struct UdeModelDesc {
  int32_t kind;          /* UDE_KIND_*                                   */
  int32_t n_regions;     /* R                                            */
  int32_t latent_dim;    /* L (>= 3)                                     */
  int32_t n_p_hidden;    /* len(net_sizes), 0 if no P-net                */
  int32_t p_hidden[4];
  int32_t n_a_hidden;    /* len(aug_net_sizes), 0 if no A-net            */
  int32_t a_hidden[4];
} UdeModelDesc;

/* One solve: N trajectories, `n_steps` RK4 grid steps, `n_out` output times. */
typedef struct UdeProblem {
  int32_t n_traj;
  int32_t n_steps;
  int32_t n_out;
  float fa_w;            /* FaFp.Fa_w (lib/models.py:225)                */
  int32_t recompute;     /* 0: the training forward stores every stage's activation rows
                            (UdeSizes.act_bytes of the checkpoint) and the backward reads
                            them; 1: memory fallback -- only the 3R stage inputs are stored
                            and the backward re-runs each stage's layers from them (same
                            results, bit for bit).  Forward and backward must agree. */
} UdeProblem;

/* Buffer sizes in bytes for one (model, problem). */
typedef struct UdeSizes {
  int64_t pack_bytes;       /* packed weights                                  */
  int64_t sched_bytes;      /* step/output schedule (layout below)              */
  int64_t ckpt_bytes;       /* stage states saved by a training forward          */
  int64_t stats_slab_bytes; /* per-workgroup fp64 partial sums                   */
  int64_t grad_slab_bytes;  /* per-workgroup gradient partials                   */
  int64_t n_params;         /* floats in the flat parameter-gradient output      */
  int32_t grid_fwd;         /* workgroups launched by the forward                */
  int32_t grid_bwd;         /* workgroups launched by the backward               */
  int32_t lds_fwd;          /* bytes of LDS per workgroup                        */
  int32_t lds_bwd;
  int64_t dec_pack_bytes;   /* packed decoder (ude_pack_decoder)                  */
  int64_t ckpt_final_bytes; /* final-state block a decoder-epilogue training forward
                               stores behind ckpt_bytes                          */
  int64_t dec_ws_bytes;     /* ude_decoder_backward workspace                     */
  int64_t act_bytes;        /* part of ckpt_bytes holding stored activation rows
                               (0 with UdeProblem.recompute = 1)                 */
  int64_t ctl_bytes;        /* control words of the *_ex calls (see below); stats_slab and, where the
                               backward has a tail kernel, grad_slab end in as many spare ones: a
                               call handed none zeroes and uses those                              */
} UdeSizes;

/*
 * Schedule buffer (host-built, copied to the device), little-endian, packed:
 *   float   dt[n_steps]            grid[n+1]-grid[n] in fp32 (torchdiffeq)
 *   int32   out_start[n_steps+1]   CSR: outputs written after step n
 *   int32   out_j[n_out]           output index (1..T-1; output 0 is y0)
 *   int32   out_mode[n_out]        0: y(t0)  1: y(t1)  2: linear interpolation
 *   float   out_slope[n_out]       (t_j - t0)/(t1 - t0) in fp32
 * n_out here counts outputs 1..T-1 (T-1 entries).
 */

/* 1 if a kernel for this model is compiled into this library. */
int ude_supported(const UdeModelDesc* m);

/* Fill *out.  `device` is the HIP device ordinal used to size the grid. */
int ude_query(const UdeModelDesc* m, const UdeProblem* p, int device, UdeSizes* out);

/* Pack nn.Linear weights into the fragment layouts the kernels read.
 * W[i] / b[i]: P-net layers first (i = 0..n_p_hidden), then A-net layers. */
int ude_pack_weights(const UdeModelDesc* m, const float* const* W, const float* const* b,
                     float* pack, ude_stream_t stream);

/* Bayesian models (kind & UDE_KIND_BAYES): the per-evaluation weight samples of
 * one solve.  Replaces Dense_Variational.make_z + forward (models_bayes.py:30-48),
 * called 4 * n_steps times per solve by the reference: eps (device) is that draw
 * stream, [4 * n_steps][n_params / 2] floats, row e feeding evaluation e (stage
 * e % 4 of step e / 4), each row in torch parameter order (per layer: weight
 * (out, in) then bias; rate net first) -- the order the reference's layers call
 * make_z within one evaluation.  W_* / b_*: the layers' w_mean / b_mean /
 * w_std / b_std (|std| is taken here).  pack is sized by ude_query
 * (pack_bytes) and holds every sample plus the eps stream the backward needs.
 * For Bayesian models ude_query's n_params is 2 x the parameter count and
 * ude_rk4_backward's dparams = [d mean (torch order) | d |std| (torch order)]. */
int ude_pack_weights_bayes(const UdeModelDesc* m, const UdeProblem* p, const float* const* W_mean,
                           const float* const* b_mean, const float* const* W_std, const float* const* b_std,
                           const float* eps, float* pack, ude_stream_t stream);

/* Forward solve.  latent: (T, N, R, L) with T = n_out + 1.  If ckpt != NULL
 * the stage states are saved for ude_rk4_backward.  stats_out (device, 5
 * floats) receives {mean_beta, mean_gamma, std_beta, std_gamma, |Fa|}
 * (entries of an absent net are 0); on return stats_slab[0..4] holds the fp64
 * totals {sum beta, sum gamma, sum beta^2, sum gamma^2, sum Fa^2} those are
 * formed from (the data-parallel statistics exchange all-reduces them; the
 * same holds for ude_rk4_forward_dec and ude_dopri5_forward's workspace).
 * With L = 8, latent must be 16-byte aligned (the tile start writes its 32-B
 * (n, r) rows with 16-B stores): UDE_E_INVALID otherwise. */
int ude_rk4_forward(const UdeModelDesc* m, const UdeProblem* p, const float* pack,
                    const void* sched, const float* y0, float* latent, float* ckpt,
                    double* stats_slab, float* stats_out, ude_stream_t stream);

/* Backward (VJP) through the same solve.
 *   dlatent: (T, N, R, L) cotangent of latent
 *   dstats (device, 5 floats): d/dmean[2], d/dstd[2], d/d|Fa|
 *   dy0: (N, R, L) written;  dparams: n_params floats, torch parameter order
 *   (for each net: weight (out,in) then bias, layer by layer; P-net first). */
int ude_rk4_backward(const UdeModelDesc* m, const UdeProblem* p, const float* pack,
                     const void* sched, const float* y0, const float* ckpt,
                     const float* dlatent, const float* stats_out, const float* dstats,
                     float* dy0, float* grad_slab, float* dparams, ude_stream_t stream);

/* Backward with the S, I, R output cotangents handed over compactly: the
 * training loss terms read only latent[..., :3] (lib/VAE.py:138, :189 -- Decoder and
 * latent_init_loss), so their cotangent has zeros in every dim >= 3.  Exactly one of dlatent
 * (T, N, R, L) and dlatent_sir (T, N, R, 3) is given (the other NULL); with dlatent_sir the
 * dims >= 3 are zero.  With the fused loss head (ude_loss_head_backward_sir) neither the zero
 * dims nor a full-size cotangent are written or read.  Replaces the same autograd backward as
 * ude_rk4_backward (lib/VAE.py:203). */
int ude_rk4_backward_sir(const UdeModelDesc* m, const UdeProblem* p, const float* pack,
                         const void* sched, const float* y0, const float* ckpt,
                         const float* dlatent, const float* dlatent_sir, const float* stats_out,
                         const float* dstats, float* dy0, float* grad_slab, float* dparams,
                         ude_stream_t stream);

/* ---- side statistics as separate buffers, statistics and gradients finalised in-kernel --------
 * The reference reads a solve's statistics as three tensors: posterior() = Normal(mean, std) of every
 * recorded rate (lib/models.py:152-156, lib/VAE.py:173) and torch.norm(torch.stack(tracker)) = |Fa|
 * (lib/VAE.py:180).  The *_ex calls take them as separate device buffers (what the autograd layer
 * hands over as three outputs / three cotangents: no split, concatenation or zero-fill between the
 * solve and the loss), and finalise in the solve's own launches:
 *   ude_rk4_forward_ex / ude_rk4_forward_dec_ex: the last workgroup of the forward kernel turns the
 *     per-workgroup fp64 partials (stats_slab) into mean / std / |Fa| (and reg_out), in a fixed order;
 *   ude_rk4_backward_ex: the per-workgroup gradient slabs, the static-feature weight gradient and
 *     dy0's static dims are formed by ONE trailing kernel.
 * ctl: ude_query's ctl_bytes of device memory, zeroed by the caller ONCE (e.g. at allocation) and
 * left zero by every call; calls that share a ctl buffer must be stream ordered (one ctl per stream
 * that runs solves concurrently).  Any UdeSideStats pointer of an absent net may be NULL; every
 * UdeSideStatsGrad pointer is nullable (zero cotangent).  ude_rk4_forward / _forward_dec / _backward /
 * _backward_sir are these launches behind a memset of spare control words: the same bits in every result. */
typedef struct UdeSideStats {
  float* mean;      /* 2 floats: mean beta, mean gamma        (posterior().loc)   */
  float* std;       /* 2 floats: unbiased std of beta, gamma  (posterior().scale) */
  float* fa_norm;   /* 1 float: |Fa| over every evaluation                         */
  double* sums;     /* 5 doubles, nullable: sum beta, sum gamma, sum beta^2, sum gamma^2, sum Fa^2 */
} UdeSideStats;

typedef struct UdeSideStatsGrad {
  const float* d_mean;     /* 2 floats, nullable */
  const float* d_std;      /* 2 floats, nullable */
  const float* d_fa_norm;  /* 1 float, nullable  */
} UdeSideStatsGrad;

int ude_rk4_forward_ex(const UdeModelDesc* m, const UdeProblem* p, const float* pack, const void* sched,
                       const float* y0, float* latent, float* ckpt, double* stats_slab, uint32_t* ctl,
                       const UdeSideStats* stats, ude_stream_t stream);

int ude_rk4_forward_dec_ex(const UdeModelDesc* m, const UdeProblem* p, const float* pack, const void* sched,
                           const float* y0, const float* dec_pack, float* yhat, float* ckpt, double* stats_slab,
                           double* reg_slab, uint32_t* ctl, const UdeSideStats* stats, float* reg_out,
                           ude_stream_t stream);

/* stats: the forward's mean / std / fa_norm (read; sums unused). */
int ude_rk4_backward_ex(const UdeModelDesc* m, const UdeProblem* p, const float* pack, const void* sched,
                        const float* y0, const float* ckpt, const float* dlatent, const float* dlatent_sir,
                        const UdeSideStats* stats, const UdeSideStatsGrad* dstats, float* dy0, float* grad_slab,
                        uint32_t* ctl, float* dparams, ude_stream_t stream);

/* ---- adaptive Dormand-Prince solve (forward) ---------------------------------
 * Replaces torchdiffeq.odeint(func, y0, t, rtol, atol, method='dopri5',
 * options={'first_step': h?}) -- the default method of the solver API the
 * reference imports (lib/VAE.py:5, run_ode.py:24) -- for the UDE right-hand
 * sides (deterministic kinds only).  torchdiffeq semantics: one step size for
 * the whole batch from the RMS error norm over all N*R*L state elements, accept
 * iff error_ratio <= 1, torchdiffeq's initial-step heuristic, dense output (DPS
 * interpolant of the last accepted step) at every t_out, float64 time
 * arithmetic.  Stats are taken over every RHS evaluation (rejected steps and the
 * start-up evaluations included), as the reference's params / tracker lists.
 *   p->n_out = T - 1 (p->n_steps is ignored); t_out: T increasing float64 times
 *   (device); latent: (T, N, R, L); ws: ude_dopri5_workspace() bytes; info
 *   (host, may be NULL): step / evaluation counts and the failure reason
 *   (status 1: dt underflow, 2: max_steps reached, 3: non-finite state).
 * first_step <= 0 selects the initial step automatically.  This call waits for
 * the device (the number of steps is data dependent): it checks the device's
 * "done" flag every 8 step attempts. */
typedef struct UdeDopriInfo {
  int32_t n_steps, n_accepted, n_evals, status;
} UdeDopriInfo;

int ude_dopri5_workspace(const UdeModelDesc* m, const UdeProblem* p, int device, int64_t* ws_bytes);

int ude_dopri5_forward(const UdeModelDesc* m, const UdeProblem* p, const float* pack, const double* t_out,
                       double rtol, double atol, double first_step, int32_t max_steps, const float* y0,
                       float* latent, void* ws, float* stats_out, UdeDopriInfo* info, ude_stream_t stream);

/* ---- fused loss head ----------------------------------------------------------
 * The training loss terms that read the solve's latent, forward and backward in one
 * pass each over it (replaces, for one model's R and L):
 *   y_pred = Decoder(latent[..., :3])  (lib/models.py:27-51, Linear(3R -> R); lib/VAE.py:138)
 *            reshaped (T, S, B, R) -> permuted (B, S, T, R), sample n = s * B + b
 *   out[0] = nll_loss(y_pred, y)       (lib/train_functions.py:81-90: mean / unbiased std
 *            over the S samples, -Normal.log_prob(y), zero where y == -1, mean over B*T*R)
 *   out[1] = latent_init_loss(latent[..., :3])  (lib/train_functions.py:116-126, a sum)
 * latent (T, S*B, R, L), W (R, 3R), b (R), y (B, T, R); S >= 2.  ws: workspace bytes
 * from ude_loss_head_workspace, kept from forward to backward (per-group mean / std).
 * backward: grad (device, 2 floats) = d loss / d out; writes dlatent (T, S*B, R, L)
 * (dims >= 3: zero), dW (R, 3R), db (R). */
int ude_loss_head_workspace(const UdeModelDesc* m, int32_t T, int32_t S, int32_t B, int device, int64_t* ws_bytes);

int ude_loss_head_forward(const UdeModelDesc* m, int32_t T, int32_t S, int32_t B, const float* latent,
                          const float* W, const float* b, const float* y, void* ws, float* out, ude_stream_t stream);

int ude_loss_head_backward(const UdeModelDesc* m, int32_t T, int32_t S, int32_t B, const float* latent,
                           const float* W, const float* b, const float* y, const float* grad, void* ws,
                           float* dlatent, float* dW, float* db, ude_stream_t stream);

/* As ude_loss_head_backward, but d latent is written compactly: dlatent_sir (T, S*B, R, 3) =
 * the S, I, R cotangents (the loss terms do not read dims >= 3), to be handed to
 * ude_rk4_backward_sir. */
int ude_loss_head_backward_sir(const UdeModelDesc* m, int32_t T, int32_t S, int32_t B, const float* latent,
                               const float* W, const float* b, const float* y, const float* grad, void* ws,
                               float* dlatent_sir, float* dW, float* db, ude_stream_t stream);

/* ---- one evaluation of the right-hand side and its VJP ---------------------------------
 * Fp / Fa / FaFp.forward(t, x) (lib/models.py:129-146, :177-188, :230-254) for every trajectory
 * of a batch: f (N, R, L) = the returned derivative (dims >= 3 zero, masked outside [-1, 2]),
 * rates (N, R, 2) = |net(x)| (what params.append records, :137 / :238; nullable) and
 * fa (N, R, 3) = aug_net(x) (tracker.append, :187 / :252; nullable).  ude_rhs_vjp: given the
 * cotangents of f (dims >= 3 ignored), rates and fa (both nullable: zero) writes dx (N, R, L)
 * and dparams (torch parameter order, ude_query's n_params) -- what autograd computes through
 * one forward() call.  These serve the solves that are not the fused RK4 kernel (adaptive
 * solves with autograd, odeint_adjoint, euler / midpoint) and, with each evaluation's sampled
 * weights packed by ude_pack_weights as a deterministic model, the Bayesian RHS
 * (models_bayes.py:43-48).  Deterministic kinds only; p->n_traj = N, p->fa_w = FaFp.Fa_w;
 * ws: ude_rhs_workspace() bytes. */
int ude_rhs_workspace(const UdeModelDesc* m, const UdeProblem* p, int device, int64_t* ws_bytes);

int ude_rhs_forward(const UdeModelDesc* m, const UdeProblem* p, const float* pack, const float* x, float* f,
                    float* rates, float* fa, ude_stream_t stream);

int ude_rhs_vjp(const UdeModelDesc* m, const UdeProblem* p, const float* pack, const float* x, const float* cot_f,
                const float* cot_rates, const float* cot_fa, float* dx, void* ws, float* dparams,
                ude_stream_t stream);

/* ---- decoder epilogue: the training solve without a latent ----------
 * The VAE's training loss reads the latent only through y_pred = Decoder(latent[..., :3])
 * (lib/models.py:27-51 Linear(3R -> R); lib/VAE.py:138) and latent_init_loss(latent[..., :3])
 * (lib/train_functions.py:116-126, lib/VAE.py:186).  ude_rk4_forward_dec runs the training forward
 * of ude_rk4_forward but emits, at every output time, y_hat (T, N, R) = W_dec . y[:3R] + b_dec
 * (y_pred = y_hat.reshape(T, S, B, R).permute(2, 1, 0, 3)) and reg_out (device float) =
 * latent_init_loss over every output's S, I, R, and writes no (T, N, R, L) latent.  Every output
 * time must be a grid point (torchdiffeq exact hit: schedule mode 1), n_steps >= 1 and
 * T <= 2048 (ude_decoder_backward returns UDE_E_INVALID otherwise).
 *   dec_pack: ude_query's dec_pack_bytes, filled by ude_pack_decoder(W_dec (R, 3R), b_dec (R));
 *   ckpt: ckpt_bytes + ckpt_final_bytes (the final state is stored behind the checkpoints);
 *   stats_slab: stats_slab_bytes; reg_slab: grid_fwd doubles.
 * ude_decoder_backward: given d y_hat (T, N, R) and grad_reg (device float, d loss / d reg_out)
 * writes the compact S, I, R cotangent dl3 (T, N, R, 3) for ude_rk4_backward_sir (every output
 * state read back from ckpt), d W_dec (R, 3R) and d b_dec (R); ws: dec_ws_bytes.
 * ude_nll_*: nll_loss(y_pred, y) (lib/train_functions.py:81-90) over y_hat (T, S*B, R) with targets
 * y (B, T, R), -1 = missing: out[0] = the mean nll; ws (ude_nll_workspace) keeps the per-group
 * sample mean / std (T, B, R, 2) for the backward, which writes d y_hat given grad (device float,
 * d loss / d nll). */
int ude_pack_decoder(const UdeModelDesc* m, const float* W_dec, const float* b_dec, float* dec_pack,
                     ude_stream_t stream);

int ude_rk4_forward_dec(const UdeModelDesc* m, const UdeProblem* p, const float* pack, const void* sched,
                        const float* y0, const float* dec_pack, float* yhat, float* ckpt, double* stats_slab,
                        double* reg_slab, float* stats_out, float* reg_out, ude_stream_t stream);

int ude_decoder_backward(const UdeModelDesc* m, const UdeProblem* p, const void* sched, const float* ckpt,
                         const float* dyhat, const float* W_dec, const float* grad_reg, void* ws, float* dl3,
                         float* dW_dec, float* db_dec, ude_stream_t stream);

int ude_nll_workspace(const UdeModelDesc* m, int32_t T, int32_t S, int32_t B, int64_t* ws_bytes);

int ude_nll_forward(const UdeModelDesc* m, int32_t T, int32_t S, int32_t B, const float* yhat, const float* y,
                    void* ws, float* out, ude_stream_t stream);

int ude_nll_backward(const UdeModelDesc* m, int32_t T, int32_t S, int32_t B, const float* yhat, const float* y,
                     const float* grad, const void* ws, float* dyhat, ude_stream_t stream);

/* ude_crps_*: the CRPS training head -- the sample-based continuous ranked probability score of the ensemble
 * y_hat (T, S*B, R) fp32 (sample n = s*B + b; no model, any y_hat: the decoder epilogue's or another) against
 * targets y (B, T, R) fp32, as a differentiable loss.  y == -1 means missing, as in nll_loss.  This is the one
 * definition the kernels (csrc/ude_crps.h), lib/train_functions.py crps_loss and the tests share.
 *   Per group (t, b, r): the samples x_s = y_hat[t, s*B+b, r], sorted x_(0) <= .. <= x_(S-1), the target
 *   y = y[b, t, r], D = S, or D = S - 1 with fair (the unbiased "fair" score of a small ensemble),
 *     c = (1 / S) sum_s |x_s - y| - (1 / (S D)) sum_i (2 i - S + 1) x_(i)
 *       = E|X - y| - sum_i sum_j |x_i - x_j| / (2 S D); with D = S exactly ude_forecast_verify's crps.
 *   loss = (1 / (B T R)) sum over the groups of c [y != -1]: nll_loss's mask and divisor (a masked group
 *   counts in the divisor).
 *   Gradient, the symmetric (mid-rank) subgradient -- what autograd gives on the pairwise form, ties included:
 *     d loss / d x_s = (g / (B T R)) num_s / (S D),   num_s = D sgn(x_s - y) - (n_lt + n_le - S),
 *     n_lt = #{j: x_j < x_s}, n_le = #{j: x_j <= x_s} (counts x_s itself), sgn(0) = 0, num_s = 0 for a masked
 *     group.  num_s is formed as an integer, so an exact zero stays exact.
 *   Arithmetic: everything after the fp32 load is fp64; out[0] and d y_hat are fp32, each rounded once from
 *   fp64: d y_hat[e] = (float)((double)grad[0] / (B T R) * num[e] / (S D)).  No scaler: training targets are in
 *   model units.  Fixed-order sums, no atomics: the same bits run to run.
 * ude_crps_forward writes out[0] = loss and keeps in ws (ude_crps_workspace() bytes: the per-workgroup fp64
 * partials and the int16 numerators, 2 bytes per element of y_hat) what ude_crps_backward needs: given grad
 * (device float, d loss / d crps) it writes d y_hat in one streaming pass (it reads neither y_hat nor y and does
 * not sort).  Stream-ordered, caller-owned buffers, no host read.  ws must be 8-byte aligned (the fp64 partials
 * are at its start) and hold all ude_crps_workspace() bytes, which need not be a multiple of 4; the backward
 * uses 16-byte accesses when ws and dyhat are both 16-byte aligned and scalar ones otherwise.  1 <= S <= 1024,
 * S >= 2 with fair, T <= 65535, no null pointer; UDE_E_INVALID otherwise, before any launch.  S = 1 without fair is the masked MAE.  The
 * reference has no counterpart: it trains on nll_loss of the sample mean / std alone. */
int ude_crps_workspace(int32_t T, int32_t S, int32_t B, int32_t R, int64_t* ws_bytes);

int ude_crps_forward(int32_t T, int32_t S, int32_t B, int32_t R, int32_t fair, const float* yhat, const float* y,
                     void* ws, float* out, ude_stream_t stream);

int ude_crps_backward(int32_t T, int32_t S, int32_t B, int32_t R, int32_t fair, const float* grad, const void* ws,
                      float* dyhat, ude_stream_t stream);

/* ude_energy_*: the energy-score training head -- the energy score of the ensemble's trajectories against the
 * observed one, as a differentiable loss: the joint score ude_forecast_joint reports, where ude_crps_* is the
 * marginal one.  This is the one definition the kernels (csrc/ude_energy.h), lib/train_functions.py energy_loss
 * and the tests share.
 *   y_hat (T, S*B, R) fp32, sample n = s*B + b (no model, any y_hat: the decoder epilogue's or another); targets
 *   y (B, T, R) fp32 in model units (no scaler); y[b,t,r] == -1 means missing, as in nll_loss and crps_loss.
 *   A block C is a set of coordinates (t, r) of one window b, chosen by `block`; K blocks per window:
 *     UDE_ENERGY_JOINT  (0): all T R coordinates, K = 1;
 *     UDE_ENERGY_SERIES (1): region r's T times, K = R;
 *     UDE_ENERGY_FIELD  (2): the R regions at time t, K = T.
 *   A coordinate whose target is missing is dropped from its window's blocks, in both terms of the score.
 *   |.|_C is the Euclidean norm over the live coordinates of C, x_i the row of sample i (x_ic = y_hat[t, i*B+b,
 *   r]), D = S, or D = S - 1 with fair (S >= 2):
 *     ES_C          = (1 / S) sum_i |x_i - y|_C - (1 / (2 S D)) sum_i sum_j |x_i - x_j|_C
 *     loss          = (1 / (B K)) sum_b sum_C ES_C
 *     d loss / d x_ic = (g / (B K)) [ (x_ic - y_c) / (S |x_i - y|_C) - (1 / (S D)) sum_j (x_ic - x_jc) / |x_i - x_j|_C ]
 *                     for c live in C.
 *   A block with no live coordinate contributes 0 and still counts in the divisor B K (nll_loss's convention).  A
 *   term whose norm is exactly 0 contributes 0 (j = i, tied samples, a sample on the target): the symmetric
 *   subgradient.  The gradient at a dropped coordinate is exactly 0.  With S = 1 the pair term is exactly 0.
 *   With D = S and nothing missing the joint / series / field loss is the mean over the windows of
 *   ude_forecast_joint's energy_joint / energy_series / energy_field; with R = 1 field, and with T = 1 series,
 *   is ude_crps_forward's loss.
 *   Arithmetic: differences are formed directly in fp64 after the fp32 load -- never |x_i|^2 + |x_j|^2 - 2 x_i .
 *   x_j, nor x_ic sum_j w_ij - sum_j w_ij x_jc, which cancel the digits that close members leave; squares are
 *   summed r ascending within t ascending, one root per pair and block; out[0] and d y_hat are fp32, each
 *   rounded once from fp64.  Fixed-order sums, no atomics: the same bits run to run.
 * ude_energy_forward writes out[0] = loss; ws (ude_energy_workspace() bytes, 8-byte aligned: fp64 partials)
 * is scratch of that call alone.  ude_energy_backward keeps nothing from the forward: given y_hat, y and grad
 * (device float, d loss / d energy) it forms the pair distances again and writes every element of d y_hat
 * (T, S*B, R) once.  Stream-ordered, caller-owned buffers, no host read.  1 <= S <= 128, S >= 2 with fair,
 * T <= 1024, R <= 1024, B <= 65535, block 0..2, no null pointer; UDE_E_INVALID otherwise, before any launch.
 * The reference has no counterpart: it trains on nll_loss alone. */
#define UDE_ENERGY_JOINT 0
#define UDE_ENERGY_SERIES 1
#define UDE_ENERGY_FIELD 2

int ude_energy_workspace(int32_t T, int32_t S, int32_t B, int32_t R, int32_t block, int64_t* ws_bytes);

int ude_energy_forward(int32_t T, int32_t S, int32_t B, int32_t R, int32_t block, int32_t fair, const float* yhat,
                       const float* y, void* ws, float* out, ude_stream_t stream);

int ude_energy_backward(int32_t T, int32_t S, int32_t B, int32_t R, int32_t block, int32_t fair, const float* yhat,
                        const float* y, const float* grad, float* dyhat, ude_stream_t stream);

/* ---- odeint_adjoint's augmented dynamics (torchdiffeq adjoint; the solver API lib/VAE.py:5 imports) --
 * One evaluation of the right-hand side and its VJP in ONE launch: f_out = f_scale * f(x) (N, R, L),
 * dx = cot_f^T df/dx (N, R, L) and dparams = cot_f^T df/dtheta (torch parameter order).  The reversed
 * augmented dynamics of odeint_adjoint's backward, (-f, a^T df/dy, a^T df/dtheta), are f_scale = -1,
 * cot_f = a; replaces the module call + torch.autograd.grad per augmented evaluation.  Deterministic
 * kinds; ws: ude_rhs_workspace() bytes. */
int ude_rhs_eval_vjp(const UdeModelDesc* m, const UdeProblem* p, const float* pack, const float* x,
                     const float* cot_f, float* f_out, float f_scale, float* dx, void* ws, float* dparams,
                     ude_stream_t stream);

/* Dense passes of the adaptive step controllers (torchdiffeq's Dormand-Prince step; no model).
 * ude_lincomb: out[i] = base[i] + sum_j coef[j] * k[j][i] over n floats (base nullable: 0; coef a
 * DEVICE array of nk <= 8 floats; k a host array of nk device pointers), one pass.
 * ude_scaled_sumsq: out[0] (device fp64) = sum_i (err_i / (atol + rtol * max(|y0_i|, |y1_i|)))^2
 * (the error ratio's numerator, tolerance formed in fp32); out must hold UDE_SUMSQ_WS doubles. */
#define UDE_SUMSQ_WS 1025
int ude_lincomb(int64_t n, const float* base, const float* const* k, int32_t nk, const float* coef, float* out,
                ude_stream_t stream);
int ude_scaled_sumsq(int64_t n, const float* err, const float* y0, const float* y1, double atol, double rtol,
                     double* out, ude_stream_t stream);
/* ude_lincomb_hc: ude_lincomb with the nk coefficients in a HOST array, copied into the launch (the
 * controller forms them from its exact host mirror of dt: no device scalar arithmetic per stage).
 * ude_dopri_ratio: one attempt's error ratio and next step size on the device, status[0..2] (device fp64)
 * = [ratio, next dt, *flag (nullable: 0)]: ratio = max(|err[0] / (atol + rtol max(|y0[0]|, |y1[0]|))| (fp32
 * tolerance), sqrt(ssq[i * UDE_SUMSQ_WS] / n[i]) for the n_pieces <= 4 sums of ude_scaled_sumsq, extra[0 ..
 * n_extra)) (NaN-propagating), next dt = dt * 10 at ratio 0, else dt * clamp(0.9 / ratio^0.2, ratio < 1 ? 1 :
 * 0.2, 10) -- torchdiffeq's mixed norm and _optimal_step_size (torchdiffeq/_impl/rk_common.py), in
 * PyTorch's operation order; one host read per attempt.  Replace the per-attempt operator chains of the
 * adaptive controller (odeint_adjoint's fused backward). */
int ude_lincomb_hc(int64_t n, const float* base, const float* const* k, int32_t nk, const float* coef_host,
                   float* out, ude_stream_t stream);
int ude_dopri_ratio(const float* err, const float* y0, const float* y1, double atol, double rtol, const double* ssq,
                    const int64_t* n, int32_t n_pieces, const double* extra, int32_t n_extra, double dt,
                    const unsigned char* flag, double* status, ude_stream_t stream);

/* ---- the forecast (lib/utils.py:20-56 test, lib/VAE.py evaluate / validate) ---------------------
 * ude_rk4_forecast_dec: the forward-only solve with the decoder epilogue.  Writes y_hat (T, N, R) =
 * Decoder(latent[..., :3]) at every output time and the side statistics; no latent, no checkpoint, no
 * stored activations, no final-state block and no latent_init_loss.  Preconditions of
 * ude_rk4_forward_dec_ex (every output time a grid point, n_steps >= 1; UDE_E_INVALID otherwise);
 * pack / dec_pack / sched / stats_slab / ctl / stats as there (ctl nullable: stats_slab's spare words).
 * Bayesian kinds take the pack of ude_pack_weights_bayes.  y_hat equals ude_rk4_forward_dec's bit for
 * bit.  Replaces model(x, t, n_samples, training=False)'s odeint + Decoder (lib/utils.py:21). */
int ude_rk4_forecast_dec(const UdeModelDesc* m, const UdeProblem* p, const float* pack, const void* sched,
                         const float* y0, const float* dec_pack, float* yhat, double* stats_slab, uint32_t* ctl,
                         const UdeSideStats* stats, ude_stream_t stream);

/* ude_rk4_forecast_dyn: ude_rk4_forecast_dec (same arguments, the same bits in y_hat and the side
 * statistics) that also writes the dynamics of every output time, dyn (C, T, N, R) fp32, channel order
 *   s, i, r                 latent[..., :3] at that time (the fp32 rounding of the solve's state)
 *   beta, gamma, r_eff      kinds with a rate net (Fp, FaFp): the rates the RHS appends to `params`
 *                           evaluated at that state (lib/models.py:120-127, unmasked), and
 *                           r_eff = (beta * s) / gamma in fp32, one IEEE division, no clamp
 *   fa_s, fa_i, fa_r        kinds with an augmentation net (Fa, FaFp): what the RHS appends to
 *                           `tracker` (before Fa_w and the mask)
 * so C = UDE_DYN_CHANNELS(kind): 6 for Fp, 6 for Fa, 9 for FaFp; there is no query, C follows from the
 * kind.  (C*T, N, R) is directly what ude_forecast_summary reads.  The last output time ends the last
 * step, so its nets are evaluated once more on the final state; that evaluation is not part of the side
 * statistics, which stay those of the solve (4 * n_steps evaluations).  Deterministic kinds only
 * (UDE_E_UNSUPPORTED with UDE_KIND_BAYES: no weight sample of the solve belongs to that evaluation) and,
 * as for ude_rk4_forecast_dec, not with UdeProblem.recompute.  Rows n >= n_traj do not exist: exactly
 * C * T * n_traj * R floats are written.  Replaces the (T, N, R, L) latent of the inference odeint plus
 * one RHS module call per output time (each of which appends to `params` / `tracker`). */
#define UDE_DYN_CHANNELS(kind) (3 + (((kind) & UDE_KIND_FP) ? 3 : 0) + (((kind) & UDE_KIND_FA) ? 3 : 0))
int ude_rk4_forecast_dyn(const UdeModelDesc* m, const UdeProblem* p, const float* pack, const void* sched,
                         const float* y0, const float* dec_pack, float* yhat, float* dyn, double* stats_slab,
                         uint32_t* ctl, const UdeSideStats* stats, ude_stream_t stream);

/* ude_rk4_forecast_scn: ude_rk4_forecast_dec under a scenario -- "transmission falls 30 % in these regions
 * from day 10".  scn is a table (n_steps, R, 2) of fp32 multipliers, 8-byte aligned, every entry finite and
 * >= 0: scn[k][r][0] scales beta and scn[k][r][1] scales gamma of region r in RK4 step k.
 *   per step, not per time   all four stage evaluations of step k use row k -- also the stage at the
 *                            step's end time, which the next step's first stage shares: a right-hand
 *                            side that jumps at a grid point is integrated piece by piece
 *   what is scaled           beta' = fl(m_beta |q0|), gamma' = fl(m_gamma |q1|) in fp32 (q: the rate net's
 *                            outputs); then plus = (beta' S) I, minus = gamma' I, + Fa_w Fa and the mask as
 *                            ever.  Fa is not scaled.  A table of ones gives ude_rk4_forecast_dec's bits
 *   dyn (nullable)           the channels of ude_rk4_forecast_dyn with beta = beta', gamma = gamma',
 *                            r_eff = (beta' s) / gamma' (one fp32 division of the emitted channels); an
 *                            output that starts a step uses that step's row, the last output the last
 *                            step's row (n_steps - 1)
 *   stats                    the side statistics of the scaled rates (they belong to the scenario)
 * Other arguments and preconditions as ude_rk4_forecast_dyn.  Kinds with a rate net only (UDE_E_UNSUPPORTED
 * for Fa, for UDE_KIND_BAYES and with UdeProblem.recompute); UDE_E_INVALID for a null or misaligned scn or
 * n_steps < 1.  A host expands per-output-interval multipliers to steps with the schedule's out_start. */
int ude_rk4_forecast_scn(const UdeModelDesc* m, const UdeProblem* p, const float* pack, const void* sched,
                         const float* y0, const float* dec_pack, const float* scn, float* yhat, float* dyn,
                         double* stats_slab, uint32_t* ctl, const UdeSideStats* stats, ude_stream_t stream);

/* Ensemble summary of y_hat (T, S*B, R) (sample n = s*B + b; no model): for every group (t, b, r) the S
 * values v_s = (double)y_hat[t, s*B+b, r] * scale[r] give mean, population std (ddof 0, two passes) and
 * quant[k] = numpy.quantile(v, q[k]) ('linear'; S <= 1024 when n_q > 0, NaN inputs undefined); with
 * targets y = (double)y_true[b, t, r] * scale[r], scores (3, T) = per time index the mean over its B*R
 * groups of [-log N(y; mean, std), log(Phi((y+0.6-mean)/std) - Phi((y-0.5-mean)/std)) with an exactly
 * zero mass replaced by 4.5399929762484854e-05, |y - mean|] = lib/Metrics.py nll / mb_log / mae (skill =
 * exp of the second).  -1 targets are not masked (as lib/utils.py).  fp64 after the load; fixed-order
 * sums, no atomics.  ws: ude_forecast_summary_workspace() bytes (only read with y_true).  Replaces the
 * host copy + NumPy / SciPy of lib/utils.py:22-26 and :53-54. */
int ude_forecast_summary_workspace(int32_t T, int32_t S, int32_t B, int32_t R, int32_t n_q, int64_t* ws_bytes);
int ude_forecast_summary(int32_t T, int32_t S, int32_t B, int32_t R, const float* yhat, const double* scale,
                         const float* y_true, const double* q, int32_t n_q, void* ws, double* mean, double* std,
                         double* quant, double* scores, ude_stream_t stream);

/* ude_forecast_verify: ude_forecast_summary (same arguments, the same bits in mean / std / quant / scores;
 * y_true required, S <= 1024 always: the tile is always sorted) plus scores of the ensemble itself.  With
 * x_(0) <= .. <= x_(S-1) the sorted v of a group, K = n_alpha levels alpha[k] in (0, 1) (1 <= K <= 16,
 * not checked: device memory), l_k / u_k / m the 'linear' quantiles at alpha_k / 2, 1 - alpha_k / 2, 0.5 and
 * J = n_pit bins (1 <= J <= 64), per group
 *   crps  = sum_i |v_i - y| / S - sum_i (2 i - S + 1) x_(i) / S^2
 *   wis   = (|y - m| / 2 + sum_k alpha_k / 2 [(u_k - l_k) + 2 / alpha_k ((l_k - y)+ + (y - u_k)+)]) / (K + 1/2)
 *   cov_k = [l_k <= y <= u_k],   pit bin = min(J - 1, J (#{v < y} + #{v <= y}) div 2 S)
 *   mass  = #{c - 0.5 <= v < c + 0.6} / S with c = floor(10 y) / 10, an empty window -> 4.5399929762484854e-05
 * (lib/Metrics.py mb_log(bins=True)'s window on the samples).  day (3 + K + J, T): per time index the mean
 * over its B*R groups of [crps, wis, log mass, cov_0 .. cov_{K-1}] and the fraction of groups in each PIT
 * bin.  region (6 + K, T, R): the mean over the B windows of a (t, r) of [the three terms of scores, crps, wis,
 * log mass, cov_k].  Counts are summed exactly and divided once.  Fixed-order sums, no atomics: the same
 * bits run to run.  ws: ude_forecast_verify_workspace() bytes. */
int ude_forecast_verify_workspace(int32_t T, int32_t S, int32_t B, int32_t R, int32_t n_q, int32_t n_alpha,
                                  int32_t n_pit, int64_t* ws_bytes);
int ude_forecast_verify(int32_t T, int32_t S, int32_t B, int32_t R, const float* yhat, const double* scale,
                        const float* y_true, const double* q, int32_t n_q, const double* alpha, int32_t n_alpha,
                        int32_t n_pit, void* ws, double* mean, double* std, double* quant, double* scores,
                        double* day, double* region, ude_stream_t stream);

/* ude_forecast_season: the seasonal targets of y_hat (T, S*B, R) (sample n = s*B + b; no model) -- what
 * depends on how a trajectory's output times hang together.  The considered output indices are t_m = start +
 * m * every, m = 0 .. M-1, M = ceil((T - start) / every) (weekly points of a daily grid: start 6, every 7);
 * the others are never read.  For a group (b, r) and sample s, fp64 after the fp32 load:
 *   v[m]   = (double)y_hat[t_m, s*B+b, r] * scale[r]
 *   peak_s = max_m v[m],   when_s = the smallest m that attains it (numpy.argmax),
 *   total_s = sum_m v[m] (m ascending),
 *   onset_s = the smallest m <= M - run with v[m+k] >= base[r] for all k < run, else M ("no onset within the
 *             horizon"; equality counts as at or above; base (R,) in scaled units, nullable: no onset)
 * Per group over the S samples (S <= 1024; NaN inputs undefined):
 *   stats (4, B, R)        mean and population std (ddof 0, two passes) of peak_s, then of total_s
 *   quant (2, n_q, B, R)   numpy.quantile ('linear') at q[k] of peak_s, then of total_s
 *   peak_time (B, M, R)    #{when_s = m} / S
 *   onset (B, M + 1, R)    #{onset_s = m} / S (only with base; bin M is "none")
 * Counts are integers, divided once.  With targets, y[m] = (double)y_true[b, t_m, r] * scale[r] gives the
 * observed y* = max, m* = its first index, o* and sum y by the same rules (-1 targets are not masked), and per
 * group, with an exactly zero P or an empty window replaced by 4.5399929762484854e-05,
 *   0  log P, P = sum over |m - m*| <= window, 0 <= m <= M-1, of peak_time[m]
 *   1  log P, P = onset[M] if o* = M, else the sum over |m - o*| <= window, m < M, of onset[m] (0 without base)
 *   2  log(#{c - 0.5 <= peak_s < c + 0.6} / S), c = floor(10 y*) / 10 (ude_forecast_verify's mass, on the peaks)
 *   3  crps of peak_s against y*,   4  crps of total_s against sum y   (ude_forecast_verify's sorted-sample
 *      formula: sum_i |x_i - y| / S - sum_i (2 i - S + 1) x_(i) / S^2)
 * overall (5,): the mean over the B*R groups; region (5, R): the mean over the B windows (skills are exp of
 * terms 0 - 2).  Fixed-order sums, no atomics: the same bits run to run.  start in [0, T), every >= 1,
 * run >= 1 (run > M is legal: no sample has an onset), window >= 0; UDE_E_INVALID otherwise.  quant nullable
 * with n_q = 0; onset only read with base; ws (ude_forecast_season_workspace() bytes), overall and region only
 * with y_true.  Every considered element of y_hat is read exactly once.  The reference has no counterpart:
 * it replaces a host copy of the whole (B, S, T, R) prediction and NumPy over its trajectories. */
int ude_forecast_season_workspace(int32_t T, int32_t S, int32_t B, int32_t R, int32_t n_q, int32_t start,
                                  int32_t every, int32_t run, int32_t window, int64_t* ws_bytes);
int ude_forecast_season(int32_t T, int32_t S, int32_t B, int32_t R, int32_t start, int32_t every, int32_t run,
                        int32_t window, const float* yhat, const double* scale, const double* base,
                        const float* y_true, const double* q, int32_t n_q, void* ws, double* stats, double* quant,
                        double* peak_time, double* onset, double* overall, double* region, ude_stream_t stream);

/* ude_forecast_joint: the joint scores of y_hat (T, S*B, R) (sample n = s*B + b; no model) against y_true
 * (B, T, R) -- the proper scores that see how the ensemble's days and regions move together.  Considered
 * output indices t_m = start + m * every, m = 0 .. M-1, M = ceil((T - start) / every), as ude_forecast_season;
 * the others are never read.  fp64 after the fp32 load: x_s[m, r] = (double)y_hat[t_m, s*B+b, r] * scale[r],
 * y[m, r] = (double)y_true[b, t_m, r] * scale[r].  For a window b and a block C of coordinates (m, r), with
 * |a|_C = sqrt(sum over C of a[m, r]^2) (formed from the differences themselves, never from an expansion of
 * the square) and p = p_code / 2 (p_code 1: p = 0.5, one sqrt; p_code 2: p = 1, the absolute value),
 *   ES_C = (1 / S) sum_i |x_i - y|_C - (1 / (2 S^2)) sum_i sum_j |x_i - x_j|_C          (energy score)
 *   VS_C = sum over c < c' in C of (|y_c - y_c'|^p - (1 / S) sum_s |x_sc - x_sc'|^p)^2   (variogram score,
 *          unweighted; s ascending; a block of one coordinate: exactly 0)
 * on the blocks
 *   series (b, r): the M times of region r     e_series, v_series (B, R)
 *   field (b, m):  the R regions at time m     e_field, v_field (B, M)
 *   joint (b):     all M R coordinates         e_joint (B,)   (no variogram: O((M R)^2 S))
 * means (1 + 2 R + 2 M): the mean over the B windows (b ascending, divided once) of e_joint | e_series (R) |
 * e_field (M) | v_series (R) | v_field (M).  In one dimension ES is the CRPS; with S = 1 the pair term is
 * exactly 0.  Fixed-order sums, no atomics: the same bits run to run.  S <= 1024, R <= 4096, M <= 4096,
 * B <= 65535, start in [0, T), every >= 1, p_code 1 or 2, no null pointer but scale; UDE_E_INVALID otherwise,
 * before any launch.  ws: ude_forecast_joint_workspace() bytes.  The reference has no counterpart: it replaces
 * a host copy of the whole (B, S, T, R) prediction and an (S, S, M R) temporary per window. */
int ude_forecast_joint_workspace(int32_t T, int32_t S, int32_t B, int32_t R, int32_t start, int32_t every,
                                 int32_t p_code, int64_t* ws_bytes);
int ude_forecast_joint(int32_t T, int32_t S, int32_t B, int32_t R, int32_t start, int32_t every, int32_t p_code,
                       const float* yhat, const double* scale, const float* y_true, void* ws, double* e_joint,
                       double* e_series, double* e_field, double* v_series, double* v_field, double* means,
                       ude_stream_t stream);

/* ude_forecast_aggregate: weighted sums over the regions of an ensemble forecast, row by row (no model) -- the
 * HHS regions and the nation of the state model as coherent ensembles, S whole trajectories per window.  A level
 * is a weight matrix (G_l, R), fp64, any sign, rows need not sum to 1; a hierarchy is an ordered list of levels
 * whose rows are stacked in that order into w (G_tot, R); g_off[l] is level l's first stacked row, g_off[0] = 0
 * and g_off[n_levels] = G_tot (g_off is a HOST array of n_levels + 1 entries, read before the call returns).
 * For a row rho of R consecutive fp32 values x[rho, :] and a stacked row g, in fp64:
 *   v_r = (double)x[rho, r] * scale[r]             (scale null: v_r = (double)x[rho, r])
 *   acc = 0;  for r = 0 .. R-1 ascending:  acc = acc + w[g, r] * v_r
 * Every product and every sum is rounded on its own: no fused multiply-add (the library is built with
 * -ffp-contract=off, which this relies on), r ascending, no reassociation.  The sum is stored as (float)acc, one
 * round-to-nearest.  A row is a (t, n) of y_hat (T, N, R) (rows = T N) or a (b, t) of y_true (B, T, R) (rows =
 * B T).  Level l's output is the contiguous block (rows, G_l) at float offset rows * g_off[l] of out (rows *
 * G_tot floats in all): each block is by itself a (T, N, G_l) array (targets: (B, T, G_l)) that
 * ude_forecast_summary / _verify / _season / _joint read unchanged, with scale = NULL (it is applied here).  The
 * aggregated ensemble is thus DEFINED as that fp32 array; everything downstream is the existing definitions on it.
 * Each element of x is read exactly once, for all levels together.  No workspace, no atomics: the same bits run
 * to run.  1 <= R <= 4096, 1 <= G_tot <= 256, 1 <= n_levels <= 16, g_off strictly increasing from 0, rows >= 0
 * (rows = 0: success without a launch), element offsets are 64-bit, no null pointer but scale; UDE_E_INVALID
 * otherwise, before any launch.  The reference has no counterpart (it trains one model per level): this replaces
 * a host copy of the whole prediction, or torch glue that rounds and sums in an order nobody has stated. */
int ude_forecast_aggregate(int64_t rows, int32_t R, int32_t n_levels, const int32_t* g_off, const float* x,
                           const double* scale, const double* w, float* out, ude_stream_t stream);

/* ude_forecast_aggregate_dyn: the same levels on the dynamics dyn (C, rows, R) fp32 of ude_rk4_forecast_dyn, C =
 * UDE_DYN_CHANNELS(kind) in its channel order (s, i, r; beta, gamma, r_eff with a rate net; fa_s, fa_i, fa_r with
 * an augmentation net); UDE_KIND_BAYES in kind is accepted and ignored (the latent fallback emits the same
 * channels).  No scale.  Per row and stacked row g, with ude_forecast_aggregate's summation rule (fp64, r
 * ascending, every operation rounded on its own; x_r the fp32 inputs converted to fp64):
 *   s_g = sum w s_r      i_g = sum w i_r      r_g = sum w r_r      fa_*_g = sum w fa_*_r
 *   inc_g = sum w[g, r] * ((beta_r * s_r) * i_r)        rec_g = sum w[g, r] * (gamma_r * i_r)
 *   beta_g = inc_g / (s_g * i_g)      gamma_g = rec_g / i_g      r_eff_g = inc_g / rec_g
 * from the fp64 sums; each output channel is rounded once to fp32.  inc and rec are the aggregate's new
 * infections and recoveries per unit time, r_eff_g their ratio, and beta_g / gamma_g the rates a single SIR
 * population with the aggregate's S and I would need to reproduce them, so r_eff_g = beta_g s_g / gamma_g by
 * construction (the mean of the regional r_eff is not the aggregate's reproduction number).  Under a scenario
 * the emitted beta and gamma are already the scaled ones.  Divisions are plain IEEE: i_g = 0 gives inf or NaN, as
 * the regional r_eff has no clamp either.  The input r_eff channel is not read; every other element is read
 * once when G_tot <= 64 (the rate planes ceil(G_tot / 64) times beyond).  Level l's output is the block (C,
 * rows, G_l) at float offset C * rows * g_off[l] of out, same channel order: (C*T, N, G_l) is what
 * ude_forecast_summary reads.  Limits and errors as ude_forecast_aggregate, and kind without the Bayes bit must
 * be UDE_KIND_FP, _FA or _FAFP.  Replaces a host copy of the (C, T, N, R) dynamics. */
int ude_forecast_aggregate_dyn(int32_t kind, int64_t rows, int32_t R, int32_t n_levels, const int32_t* g_off,
                               const float* dyn, const double* w, float* out, ude_stream_t stream);

/* Library build tag (for logs / tests). */
const char* ude_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* UDE_RK4_H */
