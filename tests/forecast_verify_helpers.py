"""Shared pieces of the ``verify`` tests (test_forecast_verify.py, test_forecast_verify_gpu.py): the
cases, a brute-force NumPy reference written independently of the implementation (CRPS over all
pairs, WIS as a sum of pinball losses with numpy.quantile, counts by direct comparison) and the
comparison with its bars."""
import functools

import numpy as np
import torch
from scipy.stats import norm

from helpers import normwise_rel
import forecast_helpers
from forecast_helpers import LEVELS, MASS_FLOOR, same_bits, synth  # noqa: F401 (same_bits: the tests import it here)

FLUSIGHT_ALPHAS = (0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)
CONTINUOUS = ("crps", "wis", "crps_r", "wis_r", "nll_r", "mae_r")
LOGS = ("ens_skill", "ens_skill_r", "skill_r")
EXACT = ("coverage", "coverage_r", "pit")
NEW_FIELDS = CONTINUOUS + LOGS + EXACT
OLD_FIELDS = ("mean", "std", "quantiles", "nll", "skill", "mae")

# name -> ((T, S, B, R), synth keywords, scaled); seed 100 + S as in the summary tests
CASES = {
    "odd_S_12_groups": ((3, 5, 4, 1), {}, True),          # padding rows, fewer groups than a wave, one zero mass
    "tile_width_BR147": ((2, 128, 3, 49), {}, True),      # dead columns in the last workgroup
    "ties": ((2, 64, 7, 10), {"ties": True}, True),       # repeated samples, a target on one of them
    "S1024": ((1, 1024, 2, 3), {}, True),                 # the largest S, G = 4
    "S1": ((2, 1, 5, 2), {}, True),                       # CRPS = |v - y|, mid-rank 1/2
    "nbx69": ((2, 2, 90, 49), {}, True),                  # more than 64 workgroups per time index
    "far_above": ((2, 16, 3, 2), {"far": 6.0}, True),     # coverage 0, last PIT bin, floored masses
    "far_below": ((2, 7, 3, 2), {"far": -6.0}, True),     # first PIT bin
    "no_scale": ((2, 9, 3, 10), {}, False),
}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    (T, S, B, R), kw, scaled = CASES[name]
    yhat, scale, y = synth(T, S, B, R, seed=100 + S, **kw)
    if name == "ties":
        y[0, 0, 0] = yhat[0, 0, 0]              # sample 0 of group (t 0, b 0, r 0), which sample 1 repeats
    if name == "S1":
        y[:, 1, :] += np.float32(0.25)          # synth puts an S = 1 target on its sample: move those of t = 1
    return yhat, (scale if scaled else None), y, S, B


def reference(yhat, S, B, scale, y_true, alphas=FLUSIGHT_ALPHAS, J=10):
    T, N, R = yhat.shape
    sc = np.ones(R) if scale is None else np.asarray(scale, dtype=np.float64)
    v = yhat.astype(np.float64).reshape(T, S, B, R) * sc
    y = y_true.astype(np.float64).transpose(1, 0, 2) * sc                       # (T, B, R)
    n = B * R
    first = np.abs(v - y[:, None]).mean(1)
    pairs = np.stack([np.abs(v[t][:, None] - v[t][None, :]).mean((0, 1)) for t in range(T)])
    crps = first - 0.5 * pairs
    assert (crps >= 0.2 * first).all()                                          # no bad cancellation
    al = np.asarray(alphas, dtype=np.float64)
    K = len(al)
    lo, up = np.quantile(v, al / 2, axis=1), np.quantile(v, 1 - al / 2, axis=1)  # (K, T, B, R)
    # the exact counts below are only meaningful when no target sits within rounding of an interval end
    for e in (lo, up):
        d = np.abs(y - e)
        assert ((d == 0) | (d > 1e-9 * np.abs(y))).all(), "a target within rounding of an interval end: other seed"
    wis = np.zeros_like(y)
    for tau in np.concatenate([[0.5], al / 2, 1 - al / 2]):
        qt = np.quantile(v, tau, axis=1)
        wis += ((y < qt) - tau) * (qt - y)
    wis /= K + 0.5
    cover = (lo <= y) & (y <= up)
    n_lt, n_le = (v < y[:, None]).sum(1), (v <= y[:, None]).sum(1)
    pit_bin = np.minimum(J - 1, (J * (n_lt + n_le)) // (2 * S))
    cb = np.floor(y * 10) / 10
    n_win = ((v >= cb[:, None] - 0.5) & (v < cb[:, None] + 0.6)).sum(1)
    log_emp = np.log(np.where(n_win == 0, MASS_FLOOR, n_win / S))
    mu, sd = v.mean(1), v.std(1)
    out = {
        "crps": crps.mean((1, 2)), "wis": wis.mean((1, 2)), "ens_skill": log_emp.mean((1, 2)),
        "coverage": cover.sum((2, 3)) / n,
        "pit": np.stack([np.bincount(pit_bin[t].ravel(), minlength=J) for t in range(T)]) / n,
        "crps_r": crps.mean(1), "wis_r": wis.mean(1), "ens_skill_r": log_emp.mean(1), "coverage_r": cover.sum(2) / B,
        "mae_r": np.abs(y - mu).mean(1),
        "zero_masses": int((n_win == 0).sum()), "groups": int(n_win.size), "tied_targets": int((n_lt != n_le).sum()),
        "max_tie": int((n_le - n_lt).max()),
    }
    if S > 1:                                      # at S = 1 the std is 0 and the Gaussian scores are NaN
        import lib.Metrics as Metrics
        out["nll_r"] = -norm.logpdf(y, loc=mu, scale=sd).mean(1)
        out["skill_r"] = Metrics.mb_log(y, mu, sd).mean(1)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(name):
    yhat, scale, y, S, B = case_inputs(name)
    return reference(yhat, S, B, scale, y)


def check(fc, ref, label=""):
    """Continuous quantities (skills by their logs) within 1e-10 normwise, counts exactly."""
    got = fc.numpy()
    errs = {}
    for k in CONTINUOUS + LOGS:
        if k not in ref:
            continue                                                            # Gaussian scores at S = 1
        errs[k] = normwise_rel(np.log(got[k]) if k in LOGS else got[k], ref[k])
    same = {k: bool(np.array_equal(got[k], ref[k])) for k in EXACT}
    print(label, {k: f"{e:.2e}" for k, e in errs.items()}, same)
    for k in NEW_FIELDS:
        assert got[k].dtype == np.float64 and got[k].shape == ref.get(k, got[k]).shape, k
    for k, e in errs.items():
        assert e <= 1e-10, (k, e)
    for k, ok in same.items():
        assert ok, (k, got[k], ref[k])


def summary(name, device="cpu", **kw):
    from ude_amd.forecast import ensemble_summary
    yhat, scale, y, S, B = case_inputs(name)
    return ensemble_summary(torch.from_numpy(yhat).to(device), S, B, y_true=torch.from_numpy(y).to(device), scale=scale,
                            quantiles=LEVELS, **kw)


def passthrough(g, device, monkeypatch):
    """VAE.forecast(..., verify=True): (the y_hat it hands to ensemble_summary, the Forecast)."""
    seen, fc = forecast_helpers.passthrough(g, device, monkeypatch, verify=True)
    assert seen["verify"] is True
    return seen, fc
