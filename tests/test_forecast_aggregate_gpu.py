"""``aggregate=`` on the MI355X (ude_forecast_aggregate, ude_forecast_aggregate_dyn, csrc/ude_aggregate.h): bit
for bit against the brute-force NumPy reference of forecast_aggregate_helpers.py at the smallest shapes where
the kernels take another path; run-to-run bits; the limits; VAE.forecast end to end on the device."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from forecast_helpers import run_forecast
from forecast_aggregate_helpers import (CASES, DYN_CASES, FORECAST_CASES, KINDS, aggregate, aggregate_dyn, case, check,
                                        dyn_case, expected_level, forecast_levels, forecast_options, same_container,
                                        spied_forecast)

pytestmark = pytest.mark.gpu


def recorded(fn):
    """(fn(), the kinds of the native calls it made)"""
    from ude_amd import fused
    events = []
    fused.EVENTS = events
    try:
        out = fn()
    finally:
        fused.EVENTS = None
    torch.cuda.synchronize()
    return out, [e[0] for e in events]


@pytest.mark.parametrize("name", list(CASES))
def test_aggregate_kernel_matches_brute_force(pkg, name):
    got, kinds = recorded(lambda: aggregate(name, "cuda"))
    assert kinds == ["forecast_aggregate"]                                  # one native call for all levels
    assert all(v.is_cuda for v in got)
    check(got, case(name)[3], name)
    for a, b in zip(got, aggregate(name, "cuda")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))       # the same bits on a second call


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", list(DYN_CASES))
def test_aggregate_dyn_kernels_match_brute_force(pkg, name, kind):
    got, kinds = recorded(lambda: aggregate_dyn(name, kind, "cuda"))
    assert kinds == ["forecast_aggregate_dyn"]
    assert all(v.is_cuda for v in got)
    check(got, dyn_case(name, kind)[3], f"{name} {kind}")
    for a, b in zip(got, aggregate_dyn(name, kind, "cuda")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_aggregate_reads_a_view(pkg):
    """A non-contiguous input and fp64 values are read as the contiguous fp32 array they stand for."""
    from ude_amd.forecast import Aggregate, ensemble_aggregate
    x, ws, scale, ref = case("offsets")
    wide = torch.zeros(x.shape[:-1] + (2 * x.shape[-1],), dtype=torch.float64, device="cuda")
    wide[..., ::2] = torch.tensor(x, device="cuda")
    out = ensemble_aggregate(wide[..., ::2], {f"level{l}": Aggregate(w) for l, w in enumerate(ws)}, scale=scale)
    check(list(out.values()), ref, "view")


def test_aggregate_limits_on_the_device(pkg):
    from ude_amd.forecast import Aggregate, aggregate_dynamics, ensemble_aggregate
    x = torch.zeros(2, 3, device="cuda")
    with pytest.raises(ValueError):
        ensemble_aggregate(x, {"a": Aggregate(np.ones((257, 3)))})
    with pytest.raises(ValueError):
        ensemble_aggregate(x, {"a": Aggregate(np.ones((200, 3))), "b": Aggregate(np.ones((57, 3)))})
    with pytest.raises(ValueError):
        ensemble_aggregate(x, {f"l{k}": Aggregate(np.ones((1, 3))) for k in range(17)})
    with pytest.raises(ValueError):
        ensemble_aggregate(torch.zeros(1, 4097, device="cuda"), {"a": Aggregate(np.ones((1, 4097)))})
    with pytest.raises(ValueError):
        aggregate_dynamics(torch.zeros(6, 1, 2, 3, device="cuda"), KINDS["Fp"], {"a": Aggregate(np.ones((257, 3)))})
    empty = ensemble_aggregate(torch.zeros(0, 3, device="cuda"), {"a": Aggregate(np.ones((2, 3)))})
    assert tuple(empty["a"].shape) == (0, 2)                                # rows = 0: no launch


@pytest.mark.parametrize("gname", FORECAST_CASES)
def test_forecast_fills_aggregates_on_the_device(pkg, monkeypatch, gname):
    from ude_amd.forecast import Aggregate
    g = load_golden(gname)
    spec = forecast_levels(g["meta"]["n_regions"])
    opts = forecast_options()
    levels = {k: Aggregate(w, baseline=b) for k, (w, b) in spec.items()}
    (seen, fc), kinds = recorded(lambda: spied_forecast(g, "cuda", monkeypatch, aggregate=levels, **opts))
    baseline = ["forecast_dyn", "forecast_verify", "forecast_summary", "forecast_season", "forecast_joint"]
    per_level = ["forecast_verify", "forecast_summary", "forecast_season", "forecast_joint"]
    assert kinds == baseline + ["forecast_aggregate", "forecast_aggregate", "forecast_aggregate_dyn"] + \
        per_level * len(spec), kinds
    assert all(v.is_cuda for _, v in fc._tensors())
    for name, (w, base) in spec.items():
        same_container(fc.aggregates[name], expected_level(g, seen, w, base, "cuda", opts), f"{gname} {name}")
    host = fc.cpu()
    for (ka, a), (kb, b) in zip(host._tensors(), fc._tensors()):
        assert ka == kb and not a.is_cuda and torch.equal(a, b.cpu()), ka
    assert list(host.aggregates) == list(spec)


def test_plain_forecast_with_aggregates_on_the_device(pkg, monkeypatch):
    """Without options: the prediction and the targets are aggregated, one summary per level."""
    from ude_amd.forecast import Aggregate
    g = load_golden("e2e_forecast_state49")
    spec = forecast_levels(49)
    levels = {k: Aggregate(w) for k, (w, _) in spec.items()}
    (_, fc), kinds = recorded(lambda: run_forecast(g, "cuda", monkeypatch, aggregate=levels))
    assert kinds == ["forecast_dec", "forecast_summary", "forecast_aggregate", "forecast_aggregate",
                     "forecast_summary", "forecast_summary"]
    assert fc.aggregates["nation"].nll is not None and fc.aggregates["nation"].dynamics is None


def test_aggregate_none_launches_nothing(pkg, monkeypatch):
    g = load_golden("e2e_forecast_us")
    (_, fc), kinds = recorded(lambda: run_forecast(g, "cuda", monkeypatch, aggregate=None))
    assert fc.aggregates is None and kinds == ["forecast_dec", "forecast_summary"]
