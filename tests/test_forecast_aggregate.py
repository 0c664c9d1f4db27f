"""``aggregate=`` on the CPU (ude_amd/forecast.py's torch fp64 loops): ``ensemble_aggregate`` and
``aggregate_dynamics`` bit for bit against the brute-force NumPy reference of forecast_aggregate_helpers.py; the
argument checks of ``Aggregate``, ``from_groups`` and ``VAE.forecast``; the checks of ude_forecast_aggregate and
ude_forecast_aggregate_dyn (host code of the library); ``VAE.forecast(aggregate=...)`` end to end against the
existing ``ensemble_*`` functions on the reference's aggregated arrays; the identity level; scenarios; and that
``aggregate=None`` changes nothing."""
import ctypes
from dataclasses import fields

import numpy as np
import pytest
import torch

from conftest import load_golden
from forecast_helpers import run_forecast, same_bits
from forecast_aggregate_helpers import (CASES, DYN_CASES, FORECAST_CASES, KINDS, aggregate, aggregate_dyn, case, check,
                                        dyn_case, expected_level, forecast_levels, forecast_options, same_container,
                                        spied_forecast, state_levels)


@pytest.mark.parametrize("name", list(CASES))
def test_aggregate_matches_brute_force(pkg, name):
    check(aggregate(name), case(name)[3], name)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", list(DYN_CASES))
def test_aggregate_dynamics_matches_brute_force(pkg, name, kind):
    check(aggregate_dyn(name, kind), dyn_case(name, kind)[3], f"{name} {kind}")


def test_aggregate_of_the_rates_is_consistent(pkg):
    """r_eff = beta s / gamma holds for the aggregate up to the roundings of its three divisions, and it is not the
    weighted mean of the regional r_eff."""
    dyn, names, ws, ref = dyn_case("R70", "FaFp")
    a = ref[0].astype(np.float64)
    s, beta, gamma, r_eff = a[0], a[3], a[4], a[5]
    assert np.allclose(r_eff, beta * s / gamma, rtol=1e-6)
    mean_of_regional = (dyn[5].astype(np.float64) @ ws[0].T)
    assert not np.allclose(r_eff, mean_of_regional, rtol=1e-3)


def test_aggregate_validation(pkg):
    from ude_amd.forecast import Aggregate, aggregate_dynamics, ensemble_aggregate
    a = Aggregate([[0.25, 0.75, 0.0], [0.0, 0.0, -1.0]], names=("ab", "c"), baseline=[1.0, 2.0])
    assert a.weights.dtype == np.float64 and a.weights.shape == (2, 3) and (a.n_groups, a.n_regions) == (2, 3)
    assert a.names == ("ab", "c") and a.baseline == (1.0, 2.0) and Aggregate(np.eye(2), baseline=3).baseline == 3.0
    assert not a.weights.flags.writeable
    with pytest.raises(Exception):
        a.names = None                                                      # frozen
    for bad in ([1.0, 2.0], [[1.0, np.nan]], [[np.inf]], np.zeros((0, 3)), np.zeros((2, 0)), "ab", np.zeros((1, 2, 3))):
        with pytest.raises(ValueError):
            Aggregate(bad)
    with pytest.raises(ValueError):
        Aggregate(np.eye(2), names=("a",))
    for bad in ([1.0, 2.0, 3.0], [[1.0, 2.0]], np.nan, "high"):
        with pytest.raises(ValueError):
            Aggregate(np.eye(2), baseline=bad)
    x = torch.zeros(4, 3)
    with pytest.raises(TypeError):
        ensemble_aggregate(x, [a])                                          # a mapping
    with pytest.raises(TypeError):
        ensemble_aggregate(x, {"a": a.weights})                             # of Aggregate
    with pytest.raises(ValueError):
        ensemble_aggregate(x, {})
    with pytest.raises(ValueError):
        ensemble_aggregate(x, {"a": Aggregate(np.eye(2))})                  # another R
    with pytest.raises(ValueError):
        ensemble_aggregate(x, {"a": a}, scale=[1.0, 2.0])                   # one per region
    with pytest.raises(ValueError):
        aggregate_dynamics(torch.zeros(6, 2, 2, 3), ("s", "i", "r", "beta", "gamma"), {"a": a})
    with pytest.raises(ValueError):
        aggregate_dynamics(torch.zeros(6, 2, 3), KINDS["Fp"], {"a": a})
    # the CPU path has no limits
    big = ensemble_aggregate(torch.ones(2, 3), {f"l{k}": Aggregate(np.ones((20, 3))) for k in range(17)})
    assert len(big) == 17 and all(bool((v == 3).all()) for v in big.values())


def test_from_groups(pkg):
    from ude_amd.forecast import Aggregate
    share = [2.0, 6.0, 0.0, 1.0, 3.0]
    a = Aggregate.from_groups(5, [[0, 1], [2, 3], [4]], share, names=("x", "y", "z"), baseline=0.5)
    want = np.array([[0.25, 0.75, 0, 0, 0], [0, 0, 0.0, 1.0, 0], [0, 0, 0, 0, 1.0]])
    assert np.array_equal(a.weights, want) and a.names == ("x", "y", "z") and a.baseline == 0.5
    nation = Aggregate.from_groups(5, [range(5)], share)
    assert np.array_equal(nation.weights, (np.array(share) / 12.0)[None])
    hhs, whole = state_levels(49, 3)                                        # the helpers' own construction
    assert np.allclose(hhs.sum(1), 1.0) and np.isclose(whole.sum(), 1.0)
    for bad in (dict(groups=[[0, 5]]), dict(groups=[[0, 0]]), dict(groups=[[]]), dict(groups=[]), dict(groups=[[2]]),
                dict(groups=[[-1]]), dict(groups=[[0.5]]), dict(share=[1.0] * 4), dict(share=[1, 1, -1, 1, 1]),
                dict(share=[1, 1, np.nan, 1, 1]), dict(R=0), dict(R=True)):
        kw = dict(dict(R=5, groups=[[0, 1]], share=share), **bad)
        with pytest.raises(ValueError):
            Aggregate.from_groups(kw["R"], kw["groups"], kw["share"])


def test_aggregate_entries_reject_bad_arguments(pkg):
    from ude_amd import _native
    lib = _native.prebuilt()
    f, g = lib.lib.ude_forecast_aggregate, lib.lib.ude_forecast_aggregate_dyn
    one = ctypes.c_void_p(8)                                                # never dereferenced: a check fails first
    off = lambda *v: (ctypes.c_int32 * len(v))(*v)
    ok = (4, 3, 2, off(0, 2, 3))
    # rows = 0 with everything else in order: success, nothing launched
    assert f(0, 3, 2, off(0, 2, 3), one, None, one, one, None) == 0
    assert g(3, 0, 3, 2, off(0, 2, 3), one, one, one, None) == 0
    assert g(3 | 4, 0, 3, 2, off(0, 2, 3), one, one, one, None) == 0        # the Bayes bit is ignored
    assert f(0, 4096, 16, off(*range(16), 256), one, one, one, one, None) == 0   # the limits themselves
    for rows, R, n, o in [(-1, 3, 2, off(0, 2, 3)), (4, 0, 2, off(0, 2, 3)), (4, 4097, 2, off(0, 2, 3)),
                          (4, 3, 0, off(0)), (4, 3, 17, off(*range(18))), (4, 3, 2, off(1, 2, 3)),
                          (4, 3, 2, off(0, 2, 2)), (4, 3, 2, off(0, 3, 2)), (4, 3, 1, off(0, 257)),
                          (4, 3, 2, off(0, 0, 3)), (4, 3, 2, None)]:
        assert f(rows, R, n, o, one, one, one, one, None) == -2, (rows, R, n)
        assert g(3, rows, R, n, o, one, one, one, None) == -2, (rows, R, n)
    for k in (0, 2, 3):                                                     # each required pointer (scale may be null)
        args = [one] * 4
        args[k] = None
        assert f(*ok, *args, None) == -2, k
    for k in range(3):
        args = [one] * 3
        args[k] = None
        assert g(3, *ok, *args, None) == -2, k
    for kind in (0, 4, 8, 11, -1):
        assert g(kind, *ok, one, one, one, None) == -2, kind
    with pytest.raises(_native.UdeError):
        lib.forecast_aggregate(4, 0, 2, off(0, 2, 3), 8, None, 8, 8, None)


@pytest.mark.parametrize("gname", FORECAST_CASES)
def test_forecast_fills_aggregates(pkg, monkeypatch, gname):
    from ude_amd.forecast import Aggregate, Forecast
    g = load_golden(gname)
    spec = forecast_levels(g["meta"]["n_regions"])
    opts = forecast_options()
    seen, fc = spied_forecast(g, "cpu", monkeypatch, aggregate={k: Aggregate(w, baseline=b) for k, (w, b) in spec.items()},
                              **opts)
    assert list(fc.aggregates) == list(spec)
    for name, (w, base) in spec.items():
        level = fc.aggregates[name]
        assert isinstance(level, Forecast) and tuple(level.mean.shape) == (seen["B"], len(g["t"]), w.shape[0])
        assert level.season is not None and (level.season.onset is None) == (base is None)
        same_container(level, expected_level(g, seen, w, base, "cpu", opts), f"{gname} {name}")
    # the baseline is the call's without aggregate
    _, plain = run_forecast(g, "cpu", monkeypatch, **opts)
    assert plain.aggregates is None
    fc.aggregates = None
    same_container(fc, plain, "baseline")


@pytest.mark.parametrize("gname", FORECAST_CASES)
def test_identity_level_is_the_baseline(pkg, monkeypatch, gname):
    """(float)(1.0 * (double)y) = y: without a scaler the identity level has the baseline's bits in every field;
    with it, what is rounded to fp32 is the scaled value: within 2^-23 max|v|, one fp32 rounding of a value."""
    from ude_amd.forecast import Aggregate
    g = load_golden(gname)
    R = g["meta"]["n_regions"]
    opts = forecast_options()
    levels = {"same": Aggregate(np.eye(R), baseline=opts["season"].baseline)}
    raw = dict(g, scaler=None)
    _, fc = run_forecast(raw, "cpu", monkeypatch, aggregate=levels, **opts)
    same, fc.aggregates = fc.aggregates["same"], None
    # The dynamics: every channel but r_eff keeps its bits (beta_g = ((beta s) i) / (s i) in fp64 is beta within
    # 3 roundings of fp64, so its fp32 rounding is beta).  The regional r_eff is fl32(fl32(beta s) / gamma), two
    # fp32 roundings of the exact ratio; the aggregate's is the fp64 ratio rounded once: each value within
    # (2 + 1) 2^-24 of the other, relatively, hence mean and quantiles within 2^-22 max|r_eff|.
    d_same, d_base, same.dynamics, fc.dynamics = same.dynamics, fc.dynamics, None, None
    same_container(same, fc, "same")
    assert d_same.names == d_base.names
    for c, n in enumerate(d_base.names):
        if n != "r_eff":
            assert same_bits(d_same.mean[c].contiguous(), d_base.mean[c].contiguous()), n
            assert same_bits(d_same.std[c].contiguous(), d_base.std[c].contiguous()), n
            assert same_bits(d_same.quantiles[:, c].contiguous(), d_base.quantiles[:, c].contiguous()), n
        else:
            bound = 2.0 ** -22 * float(d_base.quantiles[:, c].abs().amax())
            for k in ("mean", "quantiles"):
                a, b = (getattr(d, k)[c] if k == "mean" else getattr(d, k)[:, c] for d in (d_same, d_base))
                assert float((a - b).abs().max()) <= bound, (k, float((a - b).abs().max()), bound)
    seen, fc = spied_forecast(g, "cpu", monkeypatch, aggregate=levels)
    same = fc.aggregates["same"]
    bound = 2.0 ** -23 * float(np.abs(seen["yhat"].astype(np.float64) * g["scaler"]).max())
    for k in ("mean", "quantiles"):
        err = float((getattr(same, k) - getattr(fc, k)).abs().max())
        print(gname, k, err, bound)
        assert err <= bound, (k, err, bound)


def test_forecast_aggregate_arguments(pkg, monkeypatch):
    from ude_amd.forecast import Aggregate
    g = load_golden("e2e_forecast_us")
    for bad in ([Aggregate([[1.0]])], {"a": np.eye(1)}, "nation", {"a": None}):
        with pytest.raises(TypeError):
            run_forecast(g, "cpu", monkeypatch, aggregate=bad)
    with pytest.raises(ValueError):
        run_forecast(g, "cpu", monkeypatch, aggregate={"a": Aggregate(np.eye(2))})      # another R
    with pytest.raises(ValueError):
        run_forecast(g, "cpu", monkeypatch, aggregate={})


def test_scenarios_get_aggregates(pkg, monkeypatch):
    """The summary of the aggregated scenario prediction and of the aggregated paired difference; an identity
    scenario's aggregated effect is exactly zero."""
    from ude_amd.forecast import Aggregate, Scenario
    g = load_golden("e2e_forecast_state49")
    spec = forecast_levels(49)
    levels = {k: Aggregate(w, baseline=b) for k, (w, b) in spec.items()}
    _, fc = run_forecast(g, "cpu", monkeypatch, aggregate=levels,
                         scenarios={"same": Scenario(), "less": Scenario(beta=0.7)})
    for name, sf in fc.scenarios.items():
        assert list(sf.forecast.aggregates) == list(sf.effect.aggregates) == list(spec)
        for k, (w, _) in spec.items():
            a, e = sf.forecast.aggregates[k], sf.effect.aggregates[k]
            assert tuple(a.mean.shape) == tuple(e.mean.shape) == (2, len(g["t"]), w.shape[0])
            assert a.quantiles is not None and a.nll is None and a.season is None and a.aggregates is None
    for k in spec:
        e = fc.scenarios["same"].effect.aggregates[k]
        assert not e.mean.any() and not e.std.any() and not e.quantiles.any()
        assert same_bits(fc.scenarios["same"].forecast.aggregates[k].mean, fc.aggregates[k].mean)
        assert bool(fc.scenarios["less"].effect.aggregates[k].mean.any())


def test_aggregate_none_changes_nothing(pkg, monkeypatch):
    g = load_golden("e2e_forecast_us")
    _, plain = run_forecast(g, "cpu", monkeypatch)
    _, none = run_forecast(g, "cpu", monkeypatch, aggregate=None)
    assert plain.aggregates is None and none.aggregates is None
    same_container(plain, none, "aggregate=None")


def test_cpu_and_numpy_carry_the_aggregates(pkg):
    from ude_amd.forecast import Forecast
    level = Forecast(torch.ones(2, 3, 1, dtype=torch.float64), torch.zeros(2, 3, 1, dtype=torch.float64))
    fc = Forecast(torch.ones(2, 3, 4, dtype=torch.float64), torch.zeros(2, 3, 4, dtype=torch.float64),
                  aggregates={"nation": level})
    assert [f.name for f in fields(Forecast)][-2:] == ["aggregates", "joint"]
    assert len(fc._tensors()) == 4 and fc.cpu() is fc
    arrays = fc.numpy()
    assert isinstance(arrays["aggregates"]["nation"], dict) and arrays["aggregates"]["nation"]["mean"].shape == (2, 3, 1)
    half = fc._map(lambda t: t * 0.5)
    assert torch.equal(half.aggregates["nation"].mean, level.mean * 0.5)
