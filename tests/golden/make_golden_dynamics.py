"""Generate the dynamics fixtures tests/golden/e2e_dyn_*.npz (run in the build container).

The reference's own RHS classes (lib/models.py Fp / Fa / FaFp of the reference checkout, as
make_golden.py imports them) are integrated by the oracle RK4 (oracle/ude_oracle.py, as torchdiffeq) in
fp32 (the reference's dtype) and in fp64 (the parity target).  At every output time the module is then
called once on that output state, and what that call appends is taken as the reference appends it:
``params[-1]`` (beta, gamma: lib/models.py:137 / :238, before the mask) and ``tracker[-1]`` (the raw Fa:
:187 / :252, before Fa_w and the mask); ``r_eff = beta * s / gamma`` in the run's dtype.

Stored: the weights, y0, t, and ``ref64_dyn`` / ``ref32_dyn`` (C, T, N, R) in the channel order of
``ude_amd.forecast.dynamics_names`` (s, i, r[, beta, gamma, r_eff][, fa_s, fa_i, fa_r]); meta_json holds
the per-channel normwise fp32-vs-fp64 distances over all times (``ref32_vs_ref64``) and over the last
time index alone (``ref32_vs_ref64_last``).

The rate net's final layer is set to small weights (x 0.1) around a bias at the prior means (beta 0.8,
gamma 0.55), and the generator asserts min gamma >= 0.1 over the fp64 result: below that r_eff's
relative error is gamma's absolute error divided by gamma and a comparison of r_eff would say nothing.

The files are named e2e_dyn_*: tests/conftest.py takes every other *.npz under tests/golden/ whose name
does not start with rhs_ / e2e_ / bayes_ / loss_ as a solver case.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dynamics.py
"""
from __future__ import annotations

import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ.get("UDE_REFERENCE", "/root/reference"))   # as make_golden.py
sys.dont_write_bytecode = True

import lib.models as ref_models  # noqa: E402  (reference, read-only)
from oracle.ude_oracle import odeint_rk4, normwise_rel  # noqa: E402
from make_golden import build_module, make_y0  # noqa: E402

N_TRAJ = 20                       # one full 16-trajectory tile and one ragged tile
N_TIMES = 4                       # 3 weekly steps
GAMMA_MIN = 0.1
PRIOR_MEANS = (0.8, 0.55)         # beta, gamma

CASES = [
    # name, kind, R, L, net_sizes, aug_net_sizes, fa_w
    ("e2e_dyn_fafp_r1", "FaFp", 1, 8, [64, 64, 32], [64, 64], 1.0),
    ("e2e_dyn_fafp_r3_l5", "FaFp", 3, 5, [40, 24], [36], 0.5),
    ("e2e_dyn_fp_r10", "Fp", 10, 8, [64, 64, 32], None, 1.0),
    ("e2e_dyn_fa_r1", "Fa", 1, 8, None, [64, 64], 1.0),
    ("e2e_dyn_fafp_r49", "FaFp", 49, 8, [64, 64, 32], [64, 64], 1.0),
]


def channel_names(kind):
    return (("s", "i", "r") + (("beta", "gamma", "r_eff") if kind in ("Fp", "FaFp") else ())
            + (("fa_s", "fa_i", "fa_r") if kind in ("Fa", "FaFp") else ()))


def tame_rate_net(mod, R):
    """Final layer of the rate net: small weights, bias at the prior means of (beta, gamma)."""
    last = (mod.Fp_net if mod.ode_type == "Fp" else mod.net)[-1]
    with torch.no_grad():
        last.weight.mul_(0.1)
        last.bias.copy_(torch.tensor(PRIOR_MEANS).repeat(R))


def run(mod, y0, t, dtype):
    """dyn (C, T, N, R) in ``dtype``: the reference module on the oracle RK4, then one module call per
    output state."""
    mod = copy.deepcopy(mod).to(dtype)
    kind = mod.ode_type
    with torch.no_grad():
        mod.clear_tracking()
        latent = odeint_rk4(mod, y0.to(dtype), t.to(dtype), (t[1] - t[0]).to(dtype))
        chans = [[] for _ in channel_names(kind)]
        for j in range(latent.shape[0]):
            x = latent[j].clone()
            mod.clear_tracking()
            mod(t[j].to(dtype), x)
            row = [x[..., 0], x[..., 1], x[..., 2]]
            if kind in ("Fp", "FaFp"):
                p = mod.params[-1]
                row += [p[..., 0], p[..., 1], p[..., 0] * x[..., 0] / p[..., 1]]
            if kind in ("Fa", "FaFp"):
                fa = mod.tracker[-1]
                row += [fa[..., 0], fa[..., 1], fa[..., 2]]
            for c, v in zip(chans, row):
                c.append(v.clone())
        mod.clear_tracking()
    return torch.stack([torch.stack(c) for c in chans])


def main():
    torch.set_num_threads(1)
    for ci, (name, kind, R, L, net, aug, fa_w) in enumerate(CASES):
        torch.manual_seed(3000 + ci)
        gen = torch.Generator().manual_seed(4000 + ci)
        mod = build_module(kind, R, L, net, aug)
        if kind == "FaFp":
            mod.Fa_w = fa_w
        if kind != "Fa":
            tame_rate_net(mod, R)
        t = torch.arange(N_TIMES, dtype=torch.float32)
        y0 = make_y0(gen, N_TRAJ, R, L, False)
        sd32 = {k: v.detach().clone() for k, v in mod.state_dict().items()}
        d32, d64 = run(mod, y0, t, torch.float32), run(mod, y0, t, torch.float64)
        names = channel_names(kind)
        assert d64.shape == (len(names), N_TIMES, N_TRAJ, R)
        if "gamma" in names:
            gmin = float(d64[names.index("gamma")].min())
            assert gmin >= GAMMA_MIN, (name, gmin)
        dist = {n: normwise_rel(d32[c], d64[c]) for c, n in enumerate(names)}
        dist_last = {n: normwise_rel(d32[c, -1], d64[c, -1]) for c, n in enumerate(names)}
        assert max(dist.values()) <= 1e-4, dist
        arrs = {"y0": y0.numpy(), "t": t.numpy(), "ref32_dyn": d32.float().numpy(), "ref64_dyn": d64.double().numpy()}
        for k, v in sd32.items():
            arrs["w_" + k] = v.numpy()
        meta = {"name": name, "kind": kind, "n_regions": R, "latent_dim": L, "net_sizes": net,
                "aug_net_sizes": aug, "n_traj": N_TRAJ, "step": "t1-t0", "fa_w": fa_w,
                "state_dict_keys": list(sd32.keys()), "channels": list(names),
                "ref32_vs_ref64": dist, "ref32_vs_ref64_last": dist_last,
                "generator": "tests/golden/make_golden_dynamics.py (reference lib/models.py + oracle RK4, one "
                             "module call per output state)"}
        arrs["meta_json"] = np.array(json.dumps(meta))
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **arrs)
        print(f"{name:20s} {os.path.getsize(path):7d} B  worst ref32-vs-ref64 {max(dist.values()):.2e} "
              f"(last time {max(dist_last.values()):.2e})"
              + (f"  min gamma {gmin:.3f}" if "gamma" in names else ""))


if __name__ == "__main__":
    main()
