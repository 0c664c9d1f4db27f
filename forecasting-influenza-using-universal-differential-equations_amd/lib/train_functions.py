"""Drop-in for lib/train_functions.py: the loss helpers lib/VAE.py composes around
the ODE solve (KL_annealing :17-44, get_kl_params :77-80, nll_loss :81-90,
make_prior / reparam :92-102, latent_init_loss :116-126, history :142-176,
kl_div :178-179, make_file :12-15) with the reference's signatures.  ``crps_loss`` is not in the reference:
the sample-based CRPS of the MC samples as a training loss, next to ``nll_loss``; nor is ``energy_loss``, the
energy score of the MC trajectories (the joint score, where the CRPS is the marginal one)."""
import os
import subprocess

import numpy as np
import torch
from torch.distributions import Normal, kl_divergence  # noqa: F401  (re-exported, lib/VAE.py:167)
from torch.utils.checkpoint import checkpoint

from lib.models import make_prior, reparam  # noqa: F401


def make_file(prefix):
    folder = "/".join(prefix.split("/")[:-1])
    if folder and not os.path.exists(folder):
        os.makedirs(folder)


def KL_annealing(step, anneal_params):
    """KL weight schedule: linear / sigmoid / cosine ramp over reset_pos*split steps, then flat."""
    if not anneal_params.get("anneal", True):
        return 1
    period = anneal_params.get("reset_pos", 10000)
    split = anneal_params.get("split", 0.5)
    lo, hi = anneal_params.get("lower", 0.0), anneal_params.get("upper", 1.0)
    kind = anneal_params.get("type", "linear")
    while step > period:
        step -= period
    ramp = int(period * split)
    if step >= ramp:
        return hi
    frac = step / ramp
    if kind == "linear":
        return lo + frac * (hi - lo)
    if kind == "sigmoid":
        return lo + (hi - lo) / (1 + np.exp(-10 * (frac - 0.5)))
    if kind == "cosine":
        return lo + 0.5 * (1 - np.cos(np.pi * frac)) * (hi - lo)
    return None


def get_kl_params(epoch, Q, means=[0.8, 0.55], stds=[0.2, 0.2], device="cpu", limit=1e10):
    """KL(N(means, stds) || Q).mean() -- Q is ode.posterior() (lib/VAE.py:173)."""
    if epoch >= limit:
        return torch.tensor(0)
    prior = Normal(torch.tensor(means, device=device), torch.tensor(stds, device=device))
    return kl_divergence(prior, Q).mean()


def nll_loss(y_pred, y, mean=True):
    """Gaussian NLL of y under the MC-sample mean/std (dim 1); entries with y == -1 are masked."""
    dist = Normal(torch.mean(y_pred, 1), torch.std(y_pred, 1))
    out = -dist.log_prob(y) * (y != -1).float()
    return out.mean() if mean else out


class _SortedCrps(torch.autograd.Function):
    """Per-group CRPS of the samples along dim 1 (the definition at ude_crps_forward in include/ude_rk4.h):
    forward from the sorted samples, backward the mid-rank subgradient num_s / (S D) from two searches of
    every sample in its sorted group.  Plain autograd through ``sort`` would break ties by index."""

    @staticmethod
    def forward(ctx, y_pred, y, D):
        S = y_pred.shape[1]
        xs = y_pred.sort(dim=1).values
        rank = (torch.arange(S, dtype=y_pred.dtype, device=y_pred.device) * 2 - (S - 1)).view(1, S, 1, 1)
        live = y != -1
        c = (y_pred - y.unsqueeze(1)).abs().sum(1) / S - (rank * xs).sum(1) / (S * D)
        ctx.save_for_backward(y_pred, xs, y, live)
        ctx.D = D
        return c * live.to(c.dtype)

    @staticmethod
    def backward(ctx, g):
        y_pred, xs, y, live = ctx.saved_tensors
        S, D = y_pred.shape[1], ctx.D
        cols = xs.movedim(1, -1).contiguous()                   # (B, T, R, S): searchsorted's innermost dim
        v = y_pred.movedim(1, -1).contiguous()
        n_lt = torch.searchsorted(cols, v, right=False)
        n_le = torch.searchsorted(cols, v, right=True)
        num = D * torch.sign(v - y.unsqueeze(-1)).to(torch.int64) - (n_lt + n_le - S)
        num = num * live.unsqueeze(-1)
        return (g.unsqueeze(-1) * num.to(g.dtype) / (S * D)).movedim(-1, 1), None, None


def crps_loss(y_pred, y, fair=False, mean=True):
    """Sample-based CRPS of the MC samples (dim 1 of y_pred (B, S, T, R)) against y (B, T, R): per group
    E|X - y| - sum_ij |x_i - x_j| / (2 S D), D = S, or S - 1 with ``fair``; entries with y == -1 are
    masked and count in the mean's divisor, as in ``nll_loss``.  With D = S it is the ``crps`` that
    ``forecast(verify=True)`` reports.  O(S log S) per group; the gradient is the symmetric (mid-rank) one."""
    S = y_pred.shape[1]
    if fair and S < 2:
        raise ValueError("crps_loss: the fair score needs at least 2 samples")
    out = _SortedCrps.apply(y_pred, y.to(y_pred.dtype), S - 1 if fair else S)
    return out.mean() if mean else out


ENERGY_BLOCKS = ("joint", "series", "field")
ENERGY_CHUNK_BYTES = 256 << 20      # the largest temporary energy_loss forms, with or without autograd


def _guarded_root(s):
    """sqrt(s) with the value and the gradient 0 at s == 0 (plain sqrt's gradient there is inf, times 0: NaN)."""
    pos = s > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))


def energy_loss(y_pred, y, block="joint", fair=False):
    """Energy score of the MC trajectories (dim 1 of y_pred (B, S, T, R)) against y (B, T, R), the definition
    at ude_energy_forward in include/ude_rk4.h: per window and block C of coordinates -- ``"joint"`` all T R,
    ``"series"`` region r's T times, ``"field"`` the R regions at time t -- ES_C = sum_i |x_i - y|_C / S -
    sum_ij |x_i - x_j|_C / (2 S D), D = S, or S - 1 with ``fair``; a coordinate with y == -1 is dropped from its
    blocks, a block without a live coordinate counts 0 in the mean over the B K blocks.  With D = S it is the
    mean over the windows of the ``energy_joint`` / ``energy_series`` / ``energy_field`` that
    ``forecast(joint=True)`` reports.  Pairwise differences are formed directly, windows (and, where one window
    is too large, samples i) a chunk at a time, so that no temporary exceeds about 256 MB; under autograd each
    chunk keeps only its inputs and forms its differences again in the backward (``torch.utils.checkpoint``),
    so that bound holds on the gradient path too.  The guarded root gives a norm of exactly 0 the gradient 0."""
    if block not in ENERGY_BLOCKS:
        raise ValueError(f"energy_loss: block {block!r} is not one of {ENERGY_BLOCKS}")
    B, S, T, R = y_pred.shape
    if fair and S < 2:
        raise ValueError("energy_loss: the fair score needs at least 2 samples")
    D = S - 1 if fair else S
    K = {"joint": 1, "series": R, "field": T}[block]
    over = {"joint": (-2, -1), "series": (-2,), "field": (-1,)}[block]    # the dims a block's norm sums over
    y = y.to(y_pred.dtype)
    live = (y != -1).to(y_pred.dtype)

    def pair_sum(xi, x, m):
        """sum over the chunk's pairs and blocks of |x_i - x_j|_C: the (n, ni, S, T, R) temporaries live here"""
        d2 = torch.square(xi.unsqueeze(2) - x.unsqueeze(1)) * m.unsqueeze(1)
        return _guarded_root(d2.sum(over)).sum()

    recompute = torch.is_grad_enabled() and y_pred.requires_grad
    per_window = S * S * T * R * y_pred.element_size()
    nb = max(1, min(B, ENERGY_CHUNK_BYTES // per_window))
    total = y_pred.new_zeros(())
    for b0 in range(0, B, nb):
        x, yy, m = y_pred[b0:b0 + nb], y[b0:b0 + nb].unsqueeze(1), live[b0:b0 + nb].unsqueeze(1)
        n = x.shape[0]
        first = _guarded_root((torch.square(x - yy) * m).sum(over)).sum()
        ni = max(1, min(S, ENERGY_CHUNK_BYTES // (n * S * T * R * y_pred.element_size())))
        pairs = y_pred.new_zeros(())
        for i0 in range(0, S, ni):
            xi = x[:, i0:i0 + ni]
            pairs = pairs + (checkpoint(pair_sum, xi, x, m, use_reentrant=False) if recompute
                             else pair_sum(xi, x, m))
        total = total + (first / S - pairs / (2.0 * S * D))
    return total / (B * K)


def latent_init_loss(x):
    """sum over entries of (|x| where x < 0) + (|1 - x| where x > 1)."""
    zero = torch.zeros_like(x)
    return (torch.where(x < 0, abs(x), zero) + torch.where(x > 1, abs(1 - x), zero)).sum()


def kl_div(Q_mu, Q_std, P_mu, P_std):
    return torch.sum(kl_divergence(Normal(Q_mu, Q_std), Normal(P_mu, P_std)), -1)


def get_free_gpu():
    """Index of the GPU with the most free memory (rocm-smi on ROCm)."""
    try:
        import torch.cuda as tc
        free = [tc.mem_get_info(i)[0] for i in range(tc.device_count())]
        return int(np.argmax(free)) if free else 0
    except Exception:
        out = subprocess.run(["rocm-smi", "--showmeminfo", "vram", "--csv"], capture_output=True, text=True).stdout
        rows = [r.split(",") for r in out.strip().splitlines()[1:]]
        free = [int(r[1]) - int(r[2]) for r in rows if len(r) >= 3]
        return int(np.argmax(free)) if free else 0


class history:
    """Per-batch loss records -> per-epoch means (lib/train_functions.py:142-176)."""

    def __init__(self):
        self.batches = []
        self.batch_history = []
        self.epoch_history = []

    def batch(self, data=None, names=None, batch=None):
        if batch is None:
            batch = dict(zip(names, data))
        for k, v in list(batch.items()):
            if torch.is_tensor(v):
                batch[k] = v.detach().cpu().numpy()
        self.batches.append(batch)

    def epoch(self):
        return {k: np.asarray([b[k] for b in self.batches]).mean() for k in self.batches[0]}

    def reset(self):
        self.batch_history.append(self.batches)
        self.epoch_history.append(self.epoch())
        self.batches = []
