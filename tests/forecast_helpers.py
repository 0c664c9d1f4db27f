"""Shared pieces of the forecast tests (test_forecast*.py; forecast_verify_helpers.py and
forecast_season_helpers.py build on them)."""
import numpy as np
import torch

from helpers import normwise_rel

FORECAST_CASES = ["e2e_forecast_us", "e2e_forecast_state49", "e2e_forecast_us_bayes"]
QUANTITIES = ("mean", "std", "quantiles", "nll", "skill", "mae")
MASS_FLOOR = 4.5399929762484854e-05      # e^-10, written out: the references do not import the implementation's
LEVELS = [0.0, 0.025, 0.5, 0.9, 1.0]


def build_vae(g, device):
    import lib.VAE as vae_mod
    import lib.models as models
    m = g["meta"]
    ode_cls = models.FaFp
    if m.get("bayes"):
        from lib.in_development.models_bayes import Bayes_FaFp as ode_cls
    model = vae_mod.VAE(models.Encoder_Back_GRU, ode_cls, models.Decoder, m["n_qs"], 8, m["n_regions"],
                        ode_params=dict(m["ode_params"], prior_std=0.05), enc_params=m["enc_params"],
                        uncertainty=True, ode_kl_w=1 / 153)
    for part in ("enc", "ode", "dec"):
        sd = {k[len(part) + 3:]: torch.from_numpy(g[k]) for k in g if k.startswith(f"w_{part}.")}
        getattr(model, part).load_state_dict(sd, strict=True)
    return model.to(device)


def ode_eps_of(g):
    """The Bayesian case's weight draws: regenerated from the fixture's seed, checked against the
    stored first row (a changed generator would otherwise only show as a parity failure)."""
    m = g["meta"]
    if not m.get("bayes"):
        return None
    eps = torch.randn(*m["ode_eps_shape"], generator=torch.Generator().manual_seed(m["ode_eps_seed"]))
    assert torch.equal(eps[0], torch.from_numpy(g["ode_eps_head"])), "torch's CPU normal generator changed"
    return eps


def run_forecast(g, device, monkeypatch, **kw):
    model = build_vae(g, device)
    eps = torch.from_numpy(g["eps"]).to(device)
    ode_eps = ode_eps_of(g)
    monkeypatch.setattr(torch, "randn", lambda *a, **k: eps.clone())
    try:
        if ode_eps is not None:
            model.ode.set_eps_stream(ode_eps.to(device))
        fc = model.forecast(torch.from_numpy(g["x"]).to(device), torch.from_numpy(g["t"]),
                            n_samples=g["meta"]["n_samples"], y_true=torch.from_numpy(g["y_test"]).to(device),
                            scaler=g["scaler"], quantiles=g["meta"]["quantiles"], **kw)
    finally:
        monkeypatch.undo()
    return model, fc


def passthrough(g, device, monkeypatch, **forecast_kw):
    """VAE.forecast(..., **forecast_kw): (what it hands to ensemble_summary -- ``yhat``, ``S``, ``B`` and the
    keywords under their names --, the Forecast)."""
    from ude_amd import forecast as fmod
    seen = {}
    inner = fmod.ensemble_summary

    def spy(yhat, n_samples, batch, **kw):
        seen.update(kw, yhat=yhat.detach().float().cpu().numpy(), S=n_samples, B=batch)
        return inner(yhat, n_samples, batch, **kw)

    monkeypatch.setattr(fmod, "ensemble_summary", spy)
    _, fc = run_forecast(g, device, monkeypatch, **forecast_kw)
    return seen, fc


def same_bits(a, b):
    """torch.equal on the bit patterns (a NaN, as the Gaussian scores of an S = 1 group, equals itself);
    None only equals None."""
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype == torch.float64 and a.shape == b.shape and \
        torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def check_against_fixture(g, fc):
    """Each quantity within max(2e-5, 2 x the reference's own fp32-vs-fp64 distance), normwise."""
    errs = {}
    for k in QUANTITIES:
        errs[k] = normwise_rel(getattr(fc, k), g["ref64_" + k])
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, e in errs.items():
        bar = max(2e-5, 2.0 * g["meta"]["ref32_vs_ref64"][k])
        assert e <= bar, (k, e, bar)


def numpy_summary(yhat, S, B, scale, y_true, q):
    """The host arithmetic of lib/utils.py:22-26, :53-54 with the drop-in lib/Metrics.py, fp64."""
    import lib.Metrics as Metrics
    T, N, R = yhat.shape
    scale = np.ones(R) if scale is None else np.asarray(scale, dtype=np.float64)
    v = yhat.astype(np.float64).reshape(T, S, B, R) * scale[None, None, None, :]
    mu, sd = v.mean(1), v.std(1)                                   # (T, B, R)
    out = {"mean": mu.transpose(1, 0, 2), "std": sd.transpose(1, 0, 2)}
    if q is not None:
        out["quantiles"] = np.quantile(v, q, axis=1).transpose(0, 2, 1, 3)
    if y_true is not None:
        y = y_true.astype(np.float64).transpose(1, 0, 2) * scale[None, None, :]
        out["nll"] = np.array([Metrics.nll(y[g], mu[g], sd[g]) for g in range(T)])
        out["mb_log"] = np.array([Metrics.mb_log(y[g], mu[g], sd[g]).mean() for g in range(T)])
        out["mae"] = np.array([Metrics.mae(y[g], mu[g], sd[g]) for g in range(T)])
    return out


def synth(T, S, B, R, seed, targets=True, ties=False, far=None):
    """Synthetic y_hat (T, S*B, R) ~ N(mu_g, sigma_g) per group with sigma_g / mu_g >= 1e-2, a scale
    vector, and targets within 1.5 sigma of the group mean (every mass >= 1e-6 at these widths;
    far: targets that many sigma away instead).  ties: repeated values inside every group."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(1.0, 3.0, size=(T, 1, B, R))
    sg = mu * rng.uniform(0.05, 0.4, size=(T, 1, B, R))
    v = mu + sg * rng.standard_normal((T, S, B, R))
    if ties and S >= 4:
        v[:, 1] = v[:, 0]
        v[:, S - 1] = v[:, S // 2]
    yhat = v.reshape(T, S * B, R).astype(np.float32)
    scale = rng.uniform(0.5, 4.0, size=R)
    y = None
    if targets:
        v32 = yhat.astype(np.float64).reshape(T, S, B, R)
        m, s = v32.mean(1), v32.std(1)
        off = rng.uniform(-1.5, 1.5, size=m.shape) if far is None else np.full(m.shape, float(far))
        y = (m + off * s).transpose(1, 0, 2).astype(np.float32)          # (B, T, R)
    return yhat, scale, y
