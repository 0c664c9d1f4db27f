// gfx950 kernels for the batched UDE RK4 solve (forward + VJP).
//
// Hot path replaced: torchdiffeq.odeint(ode, z, t, method='rk4',
// options=dict(step_size=h)) at lib/VAE.py:137 with ode in {Fp, Fa, FaFp}
// (lib/models.py:109-265), and the autograd backward of lib/VAE.py:203.
//
// Execution model (one workgroup = 4 waves = one tile of TT=16 trajectories):
//  * every MLP layer is a small GEMM  out[o][t] = W[o][:] . in[t][:]  on
//    v_mfma_f32_16x16x4_f32 (exact fp32); the 16 trajectories are the MFMA N
//    dimension, output rows are split across the 4 waves (row tiles of 16);
//  * activations live in LDS as one [t][feature] record per trajectory; weights
//    stream from L2 in a pre-packed fragment order (one 16-B load per lane feeds
//    4 MFMAs);
//  * all 4 RK4 stages of every step run inside the launch; the training forward saves
//    the 4 stage inputs per step (3R floats each) and each stage's activation rows
//    (Model::ACT_STORED) for the backward, which reads them back instead of re-running
//    the forward and back-propagates through the 3/8-rule;
//  * the parameter gradient dW[o][i] = sum_{t,eval} g[t][o] in[t][i] is another
//    MFMA GEMM (K = trajectories) whose accumulators stay in each wave's registers
//    for the whole launch (the wave owns the rows it computed in the forward);
//    per-workgroup partials are summed by a separate deterministic pass;
//  * latent dims >= 3 have zero derivative (lib/models.py:144, :249), so they are
//    per-trajectory constants: their layer-0 contribution W0[:,static].x + b0 is
//    hoisted once per tile, and their weight gradient uses the per-trajectory sum
//    of layer-0 output gradients (one GEMM per tile).
//
// This file is the umbrella: the kernels live in the parts below, included in dependency order.
//   ude_kernels_core.h  static loops, MFMA / barrier wrappers, KArgs, Sched, Rsrc, indexing, statistics
//   ude_kernels_mlp.h   GEMM tiles, WRegs, mlp_forward, static hoist, mlp_backward(_dw, _dw_l), LDS-DMA
//   ude_kernels_fwd.h   tile starts, fwd_body, fwd_sbody, ude_fwd_kernel
//   ude_kernels_bwd.h   RK adjoint, flux_backward, bwd_body, bwd_wbody(_l), ude_bwd_kernel, static_tsum
//   ude_kernels_pack.h  ude_pack_kernel, ude_dec_pack_kernel
//   ude_kernels_tail.h  slab reductions, static gradients, ude_bwd_tail_kernel, ude_stats_finalize_kernel
#pragma once
#include "ude_kernels_core.h"
#include "ude_kernels_mlp.h"
#include "ude_kernels_fwd.h"
#include "ude_kernels_bwd.h"
#include "ude_kernels_pack.h"
#include "ude_kernels_tail.h"
