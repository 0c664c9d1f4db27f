"""The ensemble forecast on the CPU (ude_amd/forecast.py's torch fp64 definitions, VAE.forecast's
``__call__`` path): the summary against NumPy / SciPy through the drop-in lib/Metrics.py, the
forecast against the reference's own (tests/golden/e2e_forecast_*.npz, make_golden_forecast.py), and
the identity of the draw with ``__call__``."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import normwise_rel
from forecast_helpers import (FORECAST_CASES, build_vae, check_against_fixture, numpy_summary, run_forecast,
                              synth)


@pytest.mark.parametrize("shape", [(3, 5, 4, 1), (2, 16, 3, 49), (1, 7, 2, 3)])
def test_summary_matches_numpy_and_metrics(pkg, shape):
    from ude_amd.forecast import ensemble_summary
    T, S, B, R = shape
    yhat, scale, y = synth(T, S, B, R, seed=11 + R)
    q = [0.0, 0.025, 0.5, 0.9, 1.0]
    fc = ensemble_summary(torch.from_numpy(yhat), S, B, y_true=torch.from_numpy(y), scale=scale, quantiles=q)
    ref = numpy_summary(yhat, S, B, scale, y, q)
    assert fc.mean.dtype == torch.float64 and tuple(fc.mean.shape) == (B, T, R)
    assert tuple(fc.quantiles.shape) == (len(q), B, T, R) and tuple(fc.nll.shape) == (T,)
    for k in ("mean", "std", "quantiles", "nll", "mae"):
        assert normwise_rel(getattr(fc, k), ref[k]) <= 1e-10, k
    assert normwise_rel(fc.skill.log(), ref["mb_log"]) <= 1e-10
    host = fc.numpy()
    assert isinstance(host["mean"], np.ndarray) and host["quantiles"].shape == (len(q), B, T, R)
    bare = ensemble_summary(torch.from_numpy(yhat), S, B)
    assert bare.quantiles is None and bare.nll is None
    assert normwise_rel(bare.mean, numpy_summary(yhat, S, B, None, None, None)["mean"]) <= 1e-10


@pytest.mark.parametrize("case", FORECAST_CASES)
def test_forecast_cpu_matches_reference(pkg, monkeypatch, case):
    g = load_golden(case)
    model, fc = run_forecast(g, "cpu", monkeypatch)
    check_against_fixture(g, fc)


def test_forecast_draw_is_calls_draw(pkg):
    g = load_golden("e2e_forecast_us")
    model = build_vae(g, "cpu")
    x, t = torch.from_numpy(g["x"]), torch.from_numpy(g["t"])
    S = 8
    torch.manual_seed(5)
    fc = model.forecast(x, t, n_samples=S, scaler=g["scaler"])
    torch.manual_seed(5)
    y_pred = model(x, t, n_samples=S, training=False)                 # (B, S, T, R)
    ref = (y_pred.detach().double() * torch.from_numpy(g["scaler"])).mean(1)
    assert torch.allclose(fc.mean, ref, rtol=1e-12, atol=0.0)
    assert fc.nll is None and fc.quantiles is None
