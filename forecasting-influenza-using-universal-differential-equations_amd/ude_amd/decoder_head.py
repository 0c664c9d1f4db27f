"""Decoder epilogue of the training solve and the nll over its output.

The reference's training step reads the latent of ``odeint`` only through

* ``y_pred = self.dec(self.latent[..., :3])`` (lib/VAE.py:138; Decoder = Flatten + Linear(3R -> R),
  lib/models.py:27-51) reshaped ``(T, S, B, R)`` and permuted ``(B, S, T, R)``, and
* ``reg_loss = 0.1 * latent_init_loss(self.latent[..., :3])`` (lib/VAE.py:186,
  lib/train_functions.py:116-126).

``solve_decode`` runs the training solve with both computed in the forward kernel's output
path (``FusedRK4Dec``, ude_rk4_forward_dec): ``y_hat (T, N, R)`` and the reg sum, and no
``(T, N, R, L)`` latent is written; the latent is rebuilt from the training store only if
something reads it (``LazyLatent``).  ``nll_head`` is ``nll_loss(y_pred, y)``
(lib/train_functions.py:81-90) over ``y_hat`` on the gfx950 nll kernels (per (t, b, r)
sample mean / unbiased std, -log N(y), masked y == -1, mean), forward and backward one pass each.
``crps_head`` is ``crps_loss(y_pred, y)`` (lib/train_functions.py; not in the reference: the sample-based
CRPS of the ensemble as a training loss) over the same ``y_hat`` on the gfx950 CRPS kernels
(csrc/ude_crps.h: the summary kernel's sorted tile, the mid-rank gradient's integer numerators kept for a
one-pass backward).
``energy_head`` is ``energy_loss(y_pred, y)`` (likewise not in the reference: the energy score of the
ensemble's trajectories, the joint score) over the same ``y_hat`` on the gfx950 energy kernels
(csrc/ude_energy.h: direct fp64 pair differences per block; the backward forms them again).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _native
from . import fused as _fused


MAX_TIMES = 2048          # output times the decoder backward's grid-point table holds (DecBwdDims::MAX_T)


def decoder_linear(dec) -> Optional[torch.nn.Linear]:
    """The Linear(3R -> R) of a reference Decoder (lib/models.py:37-40), else None."""
    seq = getattr(dec, "decoder", None)
    if not isinstance(seq, torch.nn.Sequential) or len(seq) != 2:
        return None
    if not isinstance(seq[0], torch.nn.Flatten) or not isinstance(seq[1], torch.nn.Linear):
        return None
    if getattr(dec, "latent_dim", None) != 3:
        return None
    return seq[1]


def eligible(ode, y0: torch.Tensor, linear: Optional[torch.nn.Linear]) -> bool:
    from .solvers import fusable
    R = getattr(ode, "n_regions", None)
    return (linear is not None and fusable(ode, y0) and ode.uncertainty in ("none", "bayes")
            and not ode.materialize_tracking and tuple(linear.weight.shape) == (R, 3 * R)
            and linear.bias is not None and linear.weight.dtype == torch.float32
            and linear.weight.device == y0.device)


class LazyLatent:
    """``VAE.latent`` of a decoder-epilogue solve: materialised (differentiably) on first read."""

    def __init__(self, token, ckpt, y0, plan):
        self._args = (token, ckpt, y0, plan)
        self._value = None

    def get(self) -> torch.Tensor:
        if self._value is None:
            self._value = _fused.materialize_latent(*self._args)
            self._args = None
        return self._value

    @property
    def materialized(self) -> bool:
        return self._value is not None


def solve_decode(ode, y0: torch.Tensor, t: torch.Tensor, step_size, linear: torch.nn.Linear):
    """(y_hat (T, N, R), reg (scalar), LazyLatent, plan) -- or None when the schedule has an output
    time that is not a grid point (the epilogue needs exact hits: torchdiffeq mode y(t1))."""
    from . import solvers
    plan = solvers.plan_for(ode, y0, t, step_size)
    if plan.out_k is None or plan.n_times > MAX_TIMES:
        return None
    if ode.uncertainty == "bayes":
        # every evaluation's weight sample (models_bayes.py:43-48) from the solve's eps stream
        mus, sds = ode.ude_mean_std()
        eps = ode.take_eps(4 * plan.prob.n_steps, sum(int(p.numel()) for p in mus), y0.device)
        yhat, reg, mean, std, fa_norm, token, ckpt, sums = _fused.FusedBayesRK4Dec.apply(
            plan, y0.contiguous(), eps, linear.weight, linear.bias, *(mus + sds))
    else:
        params = []
        for lin in ode.ude_linears():
            params += [lin.weight, lin.bias]
        yhat, reg, mean, std, fa_norm, token, ckpt, sums = _fused.FusedRK4Dec.apply(
            plan, y0.contiguous(), linear.weight, linear.bias, *params)
    ode._record_fused((mean, std, fa_norm), plan.n_eval, sums=sums)
    return yhat, reg, LazyLatent(token, ckpt, y0, plan), plan


class _NllHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lib, desc, T, S, B, yhat, y):
        dev = yhat.device
        stream = _fused._stream(dev)
        ws = torch.empty(max(lib.nll_workspace(desc, T, S, B) // 4, 1), dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        yhat, y = yhat.contiguous(), y.contiguous()
        with _fused._timed("nll_fwd"):
            lib.nll_forward(desc, T, S, B, yhat.data_ptr(), y.data_ptr(), ws.data_ptr(), out.data_ptr(), stream)
        ctx.meta = (lib, desc, T, S, B)
        ctx.save_for_backward(yhat, y, ws)
        ctx.mark_non_differentiable(ws)
        return out[0], ws

    @staticmethod
    def backward(ctx, g, _gws=None):
        lib, desc, T, S, B = ctx.meta
        yhat, y, ws = ctx.saved_tensors
        dev = yhat.device
        grad = torch.zeros(1, dtype=torch.float32, device=dev) if g is None else g.reshape(1).float()
        dyhat = torch.empty_like(yhat)
        with _fused._timed("nll_bwd"):
            lib.nll_backward(desc, T, S, B, yhat.data_ptr(), y.data_ptr(), grad.data_ptr(), ws.data_ptr(),
                             dyhat.data_ptr(), _fused._stream(dev))
        return None, None, None, None, None, dyhat, None


MAX_CRPS_SAMPLES = 1024   # FC_MAX_SQ of csrc/ude_forecast.h: the largest S the kernel's sorted tile holds


class _CrpsHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lib, T, S, B, R, fair, yhat, y):
        dev = yhat.device
        # every byte of it: 2 bytes per element of y_hat behind the partials, not always a multiple of 4
        ws = torch.empty(lib.crps_workspace(T, S, B, R), dtype=torch.uint8, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        yhat, y = yhat.contiguous(), y.contiguous()
        with _fused._timed("crps_fwd"):
            lib.crps_forward(T, S, B, R, fair, yhat.data_ptr(), y.data_ptr(), ws.data_ptr(), out.data_ptr(),
                             _fused._stream(dev))
        ctx.meta = (lib, T, S, B, R, fair)
        ctx.save_for_backward(ws)                 # the backward reads the workspace's numerators only
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lib, T, S, B, R, fair = ctx.meta
        ws, = ctx.saved_tensors
        dev = ws.device
        grad = g.reshape(1).float().contiguous()
        dyhat = torch.empty((T, S * B, R), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), _fused._timed("crps_bwd"):
            lib.crps_backward(T, S, B, R, fair, grad.data_ptr(), ws.data_ptr(), dyhat.data_ptr(), _fused._stream(dev))
        return None, None, None, None, None, None, dyhat, None


def crps_head(yhat: torch.Tensor, y: torch.Tensor, n_samples: int, batch: int, fair: bool = False):
    """``train_functions.crps_loss`` (the definition at ude_crps_forward in include/ude_rk4.h) of y_pred =
    y_hat (T, S*B, R) as lib/VAE.py:138 reshapes it, against targets y (B, T, R): a scalar that carries
    autograd to ``yhat`` -- the decoder epilogue's output or any other fp32 HIP tensor of that shape.  On
    the gfx950 CRPS kernels (no model: any library); more than 1024 samples take the torch definition on
    the device."""
    from . import forecast as _forecast
    import lib.train_functions as train_functions
    if yhat.dim() != 3:
        raise ValueError(f"crps_head: y_hat {tuple(yhat.shape)} is not (T, S*B, R)")
    T, N, R = (int(v) for v in yhat.shape)
    S, B = int(n_samples), int(batch)
    if N != S * B or tuple(y.shape) != (B, T, R) or S < 1:
        raise ValueError(f"crps_head: y_hat {tuple(yhat.shape)} / targets {tuple(y.shape)} do not match "
                         f"S={n_samples}, B={batch}")
    if fair and S < 2:
        raise ValueError("crps_head: the fair score needs at least 2 samples")
    if not yhat.is_cuda or yhat.dtype != torch.float32:
        raise ValueError("crps_head: y_hat is an fp32 tensor on a HIP device (train_functions.crps_loss "
                         "is the definition for any other)")
    if S > MAX_CRPS_SAMPLES:
        return train_functions.crps_loss(yhat.reshape(T, S, B, R).permute(2, 1, 0, 3), y.to(torch.float32), fair=fair)
    lib = _forecast._library()
    if lib is None:
        raise _native.UdeError("crps_head: no gfx950 library is built (run __graft_entry__.build())")
    with torch.cuda.device(yhat.device):
        return _CrpsHead.apply(lib, T, S, B, R, int(bool(fair)), yhat, y.to(device=yhat.device, dtype=torch.float32))


# The block kinds are named once, in lib.train_functions.ENERGY_BLOCKS; the C-ABI's integer is the index there and
# the header's UDE_ENERGY_JOINT / _SERIES / _FIELD (0 / 1 / 2) -- checked against the header by the tests.


class _EnergyHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lib, T, S, B, R, kind, fair, yhat, y):
        dev = yhat.device
        ws = torch.empty(lib.energy_workspace(T, S, B, R, kind) // 8, dtype=torch.float64, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        yhat, y = yhat.contiguous(), y.contiguous()
        with _fused._timed("energy_fwd"):
            lib.energy_forward(T, S, B, R, kind, fair, yhat.data_ptr(), y.data_ptr(), ws.data_ptr(), out.data_ptr(),
                               _fused._stream(dev))
        ctx.meta = (lib, T, S, B, R, kind, fair)
        ctx.save_for_backward(yhat, y)            # the backward forms the pair distances again: no workspace kept
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lib, T, S, B, R, kind, fair = ctx.meta
        yhat, y = ctx.saved_tensors
        dev = yhat.device
        grad = g.reshape(1).float().contiguous()
        dyhat = torch.empty((T, S * B, R), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), _fused._timed("energy_bwd"):
            lib.energy_backward(T, S, B, R, kind, fair, yhat.data_ptr(), y.data_ptr(), grad.data_ptr(),
                                dyhat.data_ptr(), _fused._stream(dev))
        return None, None, None, None, None, None, None, dyhat, None


def energy_head(yhat: torch.Tensor, y: torch.Tensor, n_samples: int, batch: int, block: str = "joint",
                fair: bool = False):
    """``train_functions.energy_loss`` (the definition at ude_energy_forward in include/ude_rk4.h) of y_pred =
    y_hat (T, S*B, R) as lib/VAE.py:138 reshapes it, against targets y (B, T, R): a scalar that carries autograd
    to ``yhat`` -- the decoder epilogue's output or any other fp32 HIP tensor of that shape.  On the gfx950
    energy kernels (no model: any library); more than 128 samples, or more than 1024 times or regions, take
    the torch definition on the device."""
    from . import forecast as _forecast
    import lib.train_functions as train_functions
    if yhat.dim() != 3:
        raise ValueError(f"energy_head: y_hat {tuple(yhat.shape)} is not (T, S*B, R)")
    blocks = train_functions.ENERGY_BLOCKS
    if block not in blocks:
        raise ValueError(f"energy_head: block {block!r} is not one of {blocks}")
    T, N, R = (int(v) for v in yhat.shape)
    S, B = int(n_samples), int(batch)
    if N != S * B or tuple(y.shape) != (B, T, R) or S < 1:
        raise ValueError(f"energy_head: y_hat {tuple(yhat.shape)} / targets {tuple(y.shape)} do not match "
                         f"S={n_samples}, B={batch}")
    if fair and S < 2:
        raise ValueError("energy_head: the fair score needs at least 2 samples")
    if not yhat.is_cuda or yhat.dtype != torch.float32:
        raise ValueError("energy_head: y_hat is an fp32 tensor on a HIP device (train_functions.energy_loss "
                         "is the definition for any other)")
    lib = _forecast._library()
    if lib is None:
        raise _native.UdeError("energy_head: no gfx950 library is built (run __graft_entry__.build())")
    kind = blocks.index(block)
    if not lib.energy_supported(T, S, B, R, kind):
        # beyond the kernels' sizes (the library says which: ude_energy_workspace returns UDE_E_INVALID)
        return train_functions.energy_loss(yhat.reshape(T, S, B, R).permute(2, 1, 0, 3), y.to(torch.float32),
                                           block=block, fair=fair)
    with torch.cuda.device(yhat.device):
        return _EnergyHead.apply(lib, T, S, B, R, kind, int(bool(fair)), yhat,
                                 y.to(device=yhat.device, dtype=torch.float32))


def nll_head(ode, yhat: torch.Tensor, y: torch.Tensor, n_samples: int, batch: int):
    """(nll, group_stats (T, B, R, 2) = per-group sample mean / std) of y_pred = y_hat as lib/VAE.py
    :138 reshapes it, against targets y (B, T, R)."""
    cfg = ode.ude_config()
    lib = _native.library_for(cfg)
    desc = _native.make_desc(cfg)
    T, N, R = yhat.shape
    if N != n_samples * batch or tuple(y.shape) != (batch, T, R) or n_samples < 2:
        raise ValueError(f"nll_head: y_hat {tuple(yhat.shape)} / targets {tuple(y.shape)} do not match "
                         f"S={n_samples}, B={batch}")
    with torch.cuda.device(yhat.device):
        nll, ws = _NllHead.apply(lib, desc, T, int(n_samples), int(batch), yhat, y.to(torch.float32))
    return nll, ws[: T * batch * R * 2].view(T, batch, R, 2)
