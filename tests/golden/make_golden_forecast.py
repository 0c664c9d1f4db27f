"""Generate the forecast fixtures tests/golden/e2e_forecast_*.npz (run in the build container).

The reference VAE (lib/VAE.py + lib/models.py of the reference checkout, as make_golden.py imports it;
the oracle RK4 as torchdiffeq)
forecasts the test windows as lib/utils.py:21 does -- ``model(x, t, n_samples, training=False)`` --
in fp32 (the reference's dtype) and in fp64 (the parity target), with the eps draw of
``VAE.__call__`` pinned by replacing ``torch.randn`` for the call.  The reference's own scoring
arithmetic follows (lib/utils.py:22-26, :53-54): ``* scaler``, ``.mean(1)``, ``.std(1)``, and
lib/Metrics.py ``nll`` / ``skill`` / ``mae`` at every time index; plus ``numpy.quantile`` of the
scaled prediction at QUANTILES.

Stored (no latent, no full prediction): inputs, weights, eps, the scaler, y_test, the fp64 results
and the per-quantity normwise fp32-vs-fp64 distances (meta_json).  The Bayesian case's per-evaluation
weight draws ``ode_eps`` (4 * 36 evaluations x 11.8k parameters) are stored as their generator seed
(``meta["ode_eps_seed"]``, ``torch.randn(shape, generator=torch.Generator().manual_seed(seed))``) with
their first row (``ode_eps_head``) to detect a change of the generator: the draws themselves would
be 6.8 MB.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_forecast.py
"""
from __future__ import annotations

import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ.get("UDE_REFERENCE", "/root/reference"))   # as make_golden.py
sys.dont_write_bytecode = True

import lib.models as ref_models  # noqa: E402  (reference, read-only)
import lib.Metrics as ref_metrics  # noqa: E402
from oracle.ude_oracle import odeint_rk4, normwise_rel  # noqa: E402

QUANTILES = [0.025, 0.25, 0.5, 0.75, 0.975]
ENC = {"q_sizes": [32, 16], "ff_sizes": [16, 16], "SIR_scaler": [0.1, 0.05, 1.0]}
ODE = {"net_sizes": [64, 64, 32], "aug_net_sizes": [64, 64]}


def ode_eps_from_seed(seed, n_eval, n_par):
    return torch.randn(n_eval, n_par, generator=torch.Generator().manual_seed(seed))


def make_case(name, R, n_qs, B, S_, window, gamma, seed, bayes=False):
    td = types.ModuleType("torchdiffeq")

    def _odeint(func, y0, t, rtol=1e-7, atol=1e-9, method=None, options=None, event_fn=None):
        assert method == "rk4"
        return odeint_rk4(func, y0, t, (options or {}).get("step_size"))
    td.odeint = _odeint
    sys.modules["torchdiffeq"] = td
    import lib.VAE as ref_vae
    torch.manual_seed(seed)
    ode_cls = ref_models.FaFp
    if bayes:
        import lib.in_development.models_bayes as ref_bayes
        ode_cls = ref_bayes.Bayes_FaFp
    model = ref_vae.VAE(ref_models.Encoder_Back_GRU, ode_cls, ref_models.Decoder, n_qs, 8, R,
                        ode_params=dict(ODE, prior_std=0.05), enc_params=ENC, uncertainty=True, ode_kl_w=1 / 153)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(B, window, R * (n_qs + 1), generator=gen)
    t = torch.arange(window + gamma + 1, dtype=torch.float32) / 7     # daily outputs, step 1/7
    T = len(t)
    eps = torch.randn(S_, B, R, model.ld_enc, generator=gen)
    sd = {part: {k: v.clone() for k, v in getattr(model, part).state_dict().items()}
          for part in ("enc", "ode", "dec")}
    ode_eps, ode_seed = None, None
    if bayes:
        n_par = sum(p.numel() for p in model.ode.parameters()) // 2
        ode_seed = seed + 2
        ode_eps = ode_eps_from_seed(ode_seed, 4 * (T - 1), n_par)

    def predict(dtype):
        m = copy.deepcopy(model)
        for part in ("enc", "ode", "dec"):
            getattr(m, part).to(dtype)
        m.dtype = dtype
        m.enc.scaler = m.enc.scaler.to(dtype)
        if bayes:
            from make_golden_bayes import inject
            inject(m.ode, ode_eps.to(dtype))
        real_randn = torch.randn
        torch.randn = lambda *a, **k: eps.to(dtype).clone()
        try:
            y_pred = m(x.to(dtype), t.to(dtype), n_samples=S_, training=False)
        finally:
            torch.randn = real_randn
        return y_pred.detach().numpy()                                 # (B, S, T, R)

    p32, p64 = predict(torch.float32), predict(torch.float64)
    # the scaler: the ensemble spread of the scaled prediction around the width of Metrics.mb_log's
    # window ([y - 0.5, y + 0.6]), spread 1 : 2.5 over the regions, so the skill is neither 0 nor 1
    sd_raw = np.median(p64.std(1))
    scaler = (np.linspace(0.8, 2.0, R) if R > 1 else np.array([1.2])) / sd_raw
    rng = np.random.default_rng(seed + 3)
    mean64 = (p64 * scaler).mean(1)
    std64 = (p64 * scaler).std(1)
    y_test = ((mean64 + 0.7 * std64 * rng.standard_normal(mean64.shape)) / scaler).astype(np.float32)

    def score(pred):
        # lib/utils.py:22-26, :53-54 at every time index
        y_pr = pred * scaler[np.newaxis, np.newaxis, np.newaxis, :]
        y_te = y_test * scaler[np.newaxis, np.newaxis, :]
        mu, sg = y_pr.mean(1), y_pr.std(1)
        out = {"mean": mu, "std": sg, "quantiles": np.quantile(y_pr, QUANTILES, axis=1)}
        out["nll"] = np.array([ref_metrics.nll(y_te[:, g, :], mu[:, g, :], sg[:, g, :]) for g in range(T)])
        out["skill"] = np.array([ref_metrics.skill(y_te[:, g, :], mu[:, g, :], sg[:, g, :]) for g in range(T)])
        out["mae"] = np.array([ref_metrics.mae(y_te[:, g, :], mu[:, g, :], sg[:, g, :]) for g in range(T)])
        from scipy.stats import norm
        d = norm(loc=mu, scale=sg)
        out["_mass"] = d.cdf(y_te + 0.6) - d.cdf(y_te - 0.5)
        return out

    r32, r64 = score(p32), score(p64)
    mass = r64.pop("_mass")
    r32.pop("_mass")
    dist = {k: float(normwise_rel(torch.from_numpy(np.asarray(r32[k], dtype=np.float64)),
                                  torch.from_numpy(np.asarray(r64[k], dtype=np.float64)))) for k in r64}
    # conditions on the fixture
    z = (y_test * scaler - r64["mean"]) / r64["std"]
    assert np.abs(z).max() < 6, np.abs(z).max()
    mid = np.mean((r64["skill"] >= 0.05) & (r64["skill"] <= 0.95))
    assert mid >= 0.5, (mid, r64["skill"])
    assert mass.min() >= 1e-6, mass.min()
    assert max(dist.values()) <= 1e-3, dist

    arrs = {"x": x.numpy(), "t": t.numpy(), "eps": eps.numpy(), "scaler": scaler.astype(np.float64),
            "y_test": y_test}
    if bayes:
        arrs["ode_eps_head"] = ode_eps[0].numpy()
    for part in ("enc", "ode", "dec"):
        for k, v in sd[part].items():
            arrs[f"w_{part}.{k}"] = v.numpy()
    for k, v in r64.items():
        arrs["ref64_" + k] = np.asarray(v, dtype=np.float64)
    meta = {"B": B, "window": window, "gamma": gamma, "n_qs": n_qs, "n_regions": R, "n_samples": S_, "bayes": bayes,
            "quantiles": QUANTILES, "ode_params": ODE, "enc_params": ENC, "ref32_vs_ref64": dist,
            "ode_eps_seed": ode_seed, "ode_eps_shape": None if ode_eps is None else list(ode_eps.shape),
            "generator": "tests/golden/make_golden_forecast.py (reference lib/VAE.py + lib/models.py + lib/Metrics.py, "
                         "oracle RK4 as torchdiffeq), fp32 and fp64 runs of the reference forecast"}
    arrs["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **arrs)
    print(f"{name}: {os.path.getsize(path)} bytes, skill {r64['skill'].min():.3f}..{r64['skill'].max():.3f} "
          f"(in [0.05, 0.95] at {mid:.0%}), min mass {mass.min():.2e}, worst ref32-vs-ref64 {max(dist.values()):.2e}")


def main():
    make_case("e2e_forecast_us", R=1, n_qs=90, B=6, S_=32, window=8, gamma=28, seed=2101)
    make_case("e2e_forecast_state49", R=49, n_qs=8, B=2, S_=16, window=8, gamma=28, seed=2149)
    make_case("e2e_forecast_us_bayes", R=1, n_qs=90, B=6, S_=32, window=8, gamma=28, seed=2177, bayes=True)


if __name__ == "__main__":
    main()
