"""CPU side of tests/test_decoder_epilogue.py: the inputs and the fp64 reference chain of the
decoder-epilogue training path (ude_amd/decoder_head.py: solve_decode -> nll_head -> autograd).

Nothing here touches a device: the chain is the CPU oracle's solve (oracle/ude_oracle.py,
oracle/ude_oracle_bayes.py), the decoder, ``nll_loss`` and ``latent_init_loss`` of
lib/train_functions.py in plain torch, autograd for d x / d W_dec / d b_dec, and the oracle's VJP of
the solve for d y0 and the ODE weights.  ``dtype=torch.float32`` runs the same chain in fp32 (the
distance a bar may be derived from, ``helpers.tol``'s rule).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, Optional

import torch

from oracle.ude_oracle import OracleRHS, odeint_rk4, solve_and_grad
from oracle.ude_oracle_bayes import OracleBayesRHS, solve_and_grad_bayes

G_NLL, G_REG = 0.8, 0.1
DMEAN, DSTD, DNORM = (0.3, -0.2), (0.5, 0.1), 0.1
P_OUT = 0.25                     # share of (n, r) rows that start outside [0, 1]

# kind, R, L, net, aug, S, B, T, grid steps per output, seed (the first of 0, 1, 2, ... whose fp64
# reference meets ``check_conditions``)
CHAIN_CASES = {
    "FaFp_R1_two_steps": ("FaFp", 1, 8, [64, 64, 32], [64, 64], 9, 5, 6, 2, 0),
    "Fp_R1": ("Fp", 1, 8, [32, 32], None, 2, 40, 4, 1, 15),
    "FaFp_R10": ("FaFp", 10, 8, [64, 64, 32], [64, 64], 7, 5, 5, 1, 1),
    "FaFp_R49_split": ("FaFp", 49, 8, [64, 64, 32], [64, 64], 5, 7, 4, 1, 0),
    "FaFp_R3_L5": ("FaFp", 3, 5, [40, 24], [36], 17, 3, 6, 1, 0),
    "Fa_R1_three_steps": ("Fa", 1, 8, None, [64, 64], 4, 4, 4, 3, 0),
    "BFaFp_R1": ("BFaFp", 1, 8, [64, 64, 32], [64, 64], 6, 4, 4, 1, 0),
    "BFaFp_R10_gst": ("BFaFp", 10, 8, [64, 64, 32], [64, 64], 3, 6, 3, 1, 0),
    # the configuration lattice (tests/lattice_helpers.py c1, c5, c7, c12): no static dims; the large-record
    # kernels with resident weights, with the small-R paths, and with no weight residency at all
    "lattice_c1_L3": ("Fp", 1, 3, [32, 32], None, 5, 7, 4, 1, 0),
    "lattice_c5_R17": ("FaFp", 17, 8, [64, 64, 32], [64, 64], 5, 7, 4, 1, 0),
    "lattice_c7_wide": ("FaFp", 1, 8, [128, 128, 128], [128, 128], 5, 7, 5, 1, 0),
    "lattice_c12_R40": ("FaFp", 40, 8, [128, 128, 64], [128, 128], 5, 7, 3, 1, 0),
}
MIN_GROUP_STD = 0.015


@dataclass
class Case:
    kind: str
    mod: torch.nn.Module          # on the host, fp32
    y0: torch.Tensor              # (N, R, L) fp32
    t: torch.Tensor
    h: torch.Tensor
    W: torch.Tensor               # (R, 3R) fp32
    b: torch.Tensor               # (R,) fp32
    y: torch.Tensor               # (B, T, R) fp32 targets
    S: int
    B: int
    eps: Optional[torch.Tensor]   # Bayesian: the solve's (4 n_steps, n_params) draws
    c_yhat: torch.Tensor          # (T, N, R) fp64
    dl_full: torch.Tensor         # (T, N, R, L) fp64, non-zero in every latent dim
    latent64: torch.Tensor        # the fp64 oracle's latent
    mask_margin: float            # closest approach of any stage input's S, I, R to the RHS mask
    _refs: Dict = field(default_factory=dict)

    @property
    def bayes(self) -> bool:
        return self.kind.startswith("B")


def time_grid(T: int, div: int):
    """``t = arange(T) / 7`` and ``h = (t[1] - t[0]) / div`` when every output is then a point of
    torchdiffeq's grid ``t[0] + k h`` (the epilogue's condition, decoder_head.solve_decode); fl(3 / 7)
    is not 3 fl(1 / 7), so from T = 5 on the output times are formed as ``k * fl(1 / 7)`` instead."""
    from ude_amd.schedule import build_schedule
    for t in (torch.arange(T, dtype=torch.float32) / 7, torch.arange(T, dtype=torch.float32) * (torch.tensor(1.0) / 7)):
        h = (t[1] - t[0]) / div
        if all(int(m) == 1 for m in build_schedule(t, h).out_mode):
            return t, h
    raise AssertionError("no grid with every output on a grid point")


def _oracle(case_or_mod, bayes: bool, dtype):
    return (OracleBayesRHS if bayes else OracleRHS).from_module(case_or_mod, dtype)


def _forward(mod, bayes, y0, t, h, eps, dtype):
    """(latent, closest approach to the mask at -1 / 2 over every stage input) of the oracle's solve --
    ``solve_and_grad(...).latent`` with the stage inputs watched."""
    rhs = _oracle(mod, bayes, dtype)
    margins = []

    def watched(tt, x):
        xs = x[..., :3]
        margins.append(float(torch.minimum((xs - 2).abs(), (xs + 1).abs()).min()))
        return rhs(tt, x)

    rhs.clear_tracking()
    if bayes:
        rhs.eps = eps.to(dtype)
    with torch.no_grad():
        lat = odeint_rk4(watched, y0.to(dtype), t, h)
    rhs.clear_tracking()
    return lat, min(margins)


def decode(x, W, b):
    """Decoder = Flatten + Linear(3R -> R) on the S, I, R dims (lib/models.py:27-51): (T, N, R)."""
    T, N, R, _ = x.shape
    return x.reshape(T, N, 3 * R) @ W.T + b


def group_view(yhat, S, B):
    """y_pred of lib/VAE.py:138: (B, S, T, R), trajectory n = s * B + b."""
    T, N, R = yhat.shape
    return yhat.reshape(T, S, B, R).permute(2, 1, 0, 3)


def group_stats(yhat, S, B):
    """(T, B, R, 2): every group's sample mean and unbiased std."""
    yp = group_view(yhat, S, B)
    return torch.stack([yp.mean(1), yp.std(1)], -1).permute(1, 0, 2, 3)


def make_case(pkg, kind, R, L, net, aug, S, B, T, div, seed) -> Case:
    import ude_amd.bayes as bayes_mod
    torch.manual_seed(seed)
    bayes = kind.startswith("B")
    base = kind[1:] if bayes else kind
    cls = getattr(bayes_mod, "Bayes_" + base) if bayes else getattr(pkg, base)
    kw = {}
    if net is not None:
        kw["net_sizes"] = net
    if aug is not None:
        kw["aug_net_sizes"] = aug
    mod = cls(R, latent_dim=L, **kw)
    if base == "FaFp":
        mod.Fa_w = 0.7
    gen = torch.Generator().manual_seed(seed + 1)
    eps = None
    t, h = time_grid(T, div)
    if bayes:
        mus, sds = mod.ude_mean_std()
        with torch.no_grad():
            for p in sds:
                p.copy_(0.05 * torch.randn(p.shape, generator=gen))
        from ude_amd.schedule import build_schedule
        eps = torch.randn(4 * build_schedule(t, h).n_steps, sum(int(p.numel()) for p in mus), generator=gen)
    N = S * B

    def u(lo, hi):
        return lo + (hi - lo) * torch.rand(N, R, generator=gen)

    out = torch.rand(N, R, generator=gen) < P_OUT
    s_in, i_in = u(0.50, 0.75), u(0.08, 0.15)
    sir_in = torch.stack([s_in, i_in, 1 - s_in - i_in], -1)
    sir_out = torch.stack([u(1.10, 1.20), u(-0.15, -0.08), u(-0.15, -0.08)], -1)
    sir = torch.where(out[..., None], sir_out, sir_in)
    y0 = torch.cat([sir, torch.randn(N, R, L - 3, generator=gen)], -1)
    W = torch.randn(R, 3 * R, generator=gen) / math.sqrt(3 * R)
    b = 0.1 * torch.randn(R, generator=gen)
    lat, margin = _forward(mod, bayes, y0, t, h, eps, torch.float64)
    st = group_stats(decode(lat[..., :3], W.double(), b.double()), S, B)           # (T, B, R, 2)
    y = (st[..., 0] + 0.7 * st[..., 1] * torch.randn(T, B, R, generator=gen, dtype=torch.float64)).permute(1, 0, 2)
    c_yhat = torch.randn(T, N, R, generator=gen, dtype=torch.float64)
    dl_full = torch.randn(T, N, R, L, generator=gen, dtype=torch.float64)
    return Case(kind, mod, y0, t, h, W, b, y.float().contiguous(), S, B, eps, c_yhat, dl_full, lat, margin)


def conditions(case: Case) -> dict:
    """What the fp64 reference must satisfy before a kernel is compared with it."""
    x = case.latent64[..., :3]
    sd = group_stats(decode(x, case.W.double(), case.b.double()), case.S, case.B)[..., 1]
    return {"kink": float(torch.minimum(x.abs(), (x - 1).abs()).min()),
            "outside": float(((x < 0) | (x > 1)).double().mean()),
            "mask": case.mask_margin,
            "min_group_std": float(sd.min())}


def check_conditions(case: Case) -> dict:
    c = conditions(case)
    assert c["kink"] >= 1e-4, c            # 10 x the 1e-5 state bar: no fp32 state on the other branch
    assert c["outside"] >= 0.05, c         # reg and its derivative are exercised
    assert c["mask"] >= 0.2, c             # no stage near the RHS mask at -1 / 2
    # nll's gradient grows like sd^-3, so an error d of y_hat moves a group's gradient by about 3 d / sd
    # of itself, and the group with the smallest sd carries most of the gradient's norm.  A correct fp32
    # y_hat is off by some 5e-8 here (|y_hat| < 1, a few roundings); 3 * 5e-8 / sd stays under half of
    # the 2e-5 gradient bar from sd = 0.015 on.  (S = 2, B = 40: seeds 0..14 have a group below that;
    # their own fp32 chains are up to 3e-2 from fp64 in d y0.)
    assert c["min_group_std"] >= MIN_GROUP_STD, c
    return c


def reference_chain(case: Case, terms, stats_cot: bool = True, dtype=torch.float64) -> dict:
    """The chain for  loss = [nll] g_nll nll + [reg] g_reg reg + [yhat] <y_hat, c> + [latent] <latent, dl>
    (+ the side-statistics cotangents when ``stats_cot``).  Returns y_hat, reg, nll, stats (T, B, R, 2),
    mean / std / fa_norm, latent, d_y0, d_ode (list, C-ABI order; Bayesian: means then raw stds), dW, db."""
    terms = frozenset(terms)
    key = (terms, stats_cot, dtype)
    if key in case._refs:
        return case._refs[key]
    import lib.train_functions as tf
    lat = case.latent64 if dtype == torch.float64 else \
        _forward(case.mod, case.bayes, case.y0, case.t, case.h, case.eps, dtype)[0]
    x = lat[..., :3].detach().clone().requires_grad_(True)
    W = case.W.to(dtype).clone().requires_grad_(True)
    b = case.b.to(dtype).clone().requires_grad_(True)
    yhat = decode(x, W, b)
    nll = tf.nll_loss(group_view(yhat, case.S, case.B), case.y.to(dtype))
    reg = tf.latent_init_loss(x)
    loss = x.sum() * 0.0
    if "nll" in terms:
        loss = loss + G_NLL * nll
    if "reg" in terms:
        loss = loss + G_REG * reg
    if "yhat" in terms:
        loss = loss + (yhat * case.c_yhat.to(dtype)).sum()
    dx, dW, db = torch.autograd.grad(loss, [x, W, b], allow_unused=True)
    cot = torch.zeros_like(lat)
    if dx is not None:
        cot[..., :3] = dx
    if "latent" in terms:
        cot = cot + case.dl_full.to(dtype)
    dm = torch.tensor(DMEAN, dtype=dtype) if stats_cot else None
    ds = torch.tensor(DSTD, dtype=dtype) if stats_cot else None
    dn = DNORM if stats_cot else None
    rhs = _oracle(case.mod, case.bayes, dtype)
    if case.bayes:
        r = solve_and_grad_bayes(rhs, case.eps.to(dtype), case.y0.to(dtype), case.t, case.h, cot, dm, ds, dn)
        side = {k: r.get(k) for k in ("mean", "std", "fa_norm")}
        d_y0, d_ode = r["grads"]["y0"], r["grads"]["mu"] + r["grads"]["sd"]
    else:
        r = solve_and_grad(rhs, case.y0.to(dtype), case.t, case.h, cot, dm, ds, dn)
        side = {"mean": r.mean, "std": r.std, "fa_norm": r.fa_norm}
        d_y0, d_ode = r.grads["y0"], [g for n, g in r.grads.items() if n != "y0"]
    out = {"yhat": yhat.detach(), "reg": reg.detach(), "nll": nll.detach(),
           "stats": group_stats(yhat.detach(), case.S, case.B), "latent": lat, **side,
           "d_y0": d_y0, "d_ode": d_ode,
           "dW": torch.zeros_like(W) if dW is None else dW, "db": torch.zeros_like(b) if db is None else db}
    case._refs[key] = out
    return out


def chain_distance(a: dict, b: dict) -> dict:
    """Normwise distance of every quantity of chain result a from b (d_ode: the worst tensor)."""
    from helpers import normwise_rel
    out = {}
    for k in ("yhat", "reg", "nll", "stats", "mean", "std", "fa_norm", "d_y0", "dW", "db"):
        if b.get(k) is not None:
            out[k] = normwise_rel(a[k], b[k])
    out["d_ode"] = max(normwise_rel(x, y) for x, y in zip(a["d_ode"], b["d_ode"]))
    return out


# ---- the nll kernels alone --------------------------------------------------------------------------

def nll_inputs(R, T, S, B, seed, rel_sigma=(0.05, 0.4), offset=(-1.5, 1.5), mask=0.2):
    """Synthetic y_hat (T, S*B, R) fp32 ~ N(mu_g, sigma_g) per group, mu in [1, 3], sigma / mu in
    ``rel_sigma``; targets (B, T, R) fp32 ``offset`` group-sds off the group mean, about ``mask`` of them
    -1 (first and last element and one whole time index among them); a random upstream gradient."""
    gen = torch.Generator().manual_seed(seed)

    def u(lo, hi, shape):
        return lo + (hi - lo) * torch.rand(shape, generator=gen, dtype=torch.float64)

    mu = u(1.0, 3.0, (T, 1, B, R))
    sg = mu * u(rel_sigma[0], rel_sigma[1], (T, 1, B, R))
    yhat = (mu + sg * torch.randn(T, S, B, R, generator=gen, dtype=torch.float64)).reshape(T, S * B, R).float()
    st = group_stats(yhat.double(), S, B)
    y = (st[..., 0] + u(offset[0], offset[1], (T, B, R)) * st[..., 1]).permute(1, 0, 2).float().contiguous()
    if mask:
        m = torch.rand(B, T, R, generator=gen) < mask
        m[0, 0, 0] = m[-1, -1, -1] = True
        m[:, T // 2, :] = True
        y[m] = -1.0
    g = float(u(0.2, 2.0, (1,)))
    return yhat, y, g


def nll_reference(yhat, y, S, B, g, dtype=torch.float64) -> dict:
    """lib.train_functions.nll_loss on the host in ``dtype``: nll, stats (T, B, R, 2), d y_hat of g * nll."""
    import lib.train_functions as tf
    yh = yhat.detach().to(dtype).clone().requires_grad_(True)
    nll = tf.nll_loss(group_view(yh, S, B), y.to(dtype))
    (d,) = torch.autograd.grad(g * nll, [yh])
    return {"nll": nll.detach(), "stats": group_stats(yh.detach(), S, B), "dyhat": d}
