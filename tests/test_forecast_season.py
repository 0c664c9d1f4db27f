"""``season=`` on the CPU (ude_amd/forecast.py's torch fp64 definitions): the distribution over the
ensemble of each trajectory's peak value, peak time, total and onset, and their scores against the
observed season, against a brute-force NumPy reference (forecast_season_helpers.py); the argument
checks; ude_forecast_season_workspace's checks (host code of the library); VAE.forecast's
pass-through; and that ``season=None`` changes nothing."""
import ctypes
from dataclasses import fields

import numpy as np
import pytest
import torch

from conftest import load_golden
from forecast_helpers import run_forecast, synth
from forecast_season_helpers import (CASES, FIELDS, SCORES, case_inputs, case_reference, check, golden_baseline,
                                     passthrough, reference, same_bits, targets)


def test_reference_covers_the_branches(pkg):
    """On the reference alone: each case does what its comment says."""
    refs = {name: case_reference(name) for name in CASES}
    assert refs["M1"]["M"] == refs["M1_run2"]["M"] == 1 and refs["weekly"]["M"] == 4
    assert (refs["M1_run2"]["onset"][:, 1] == 1).all() and 0 < refs["M1"]["no_onset"] < 1
    assert refs["weekly"]["peak_mean"].max() < 100                         # no skipped 1e30 shows
    S1 = refs["S1"]
    assert set(np.unique(S1["peak_time"])) == {0.0, 1.0} and (S1["peak_std"] == 0).all()
    yhat, scale, y, S, B, base, opts = case_inputs("S1")
    peak = (yhat.astype(np.float64).reshape(4, 1, 5, 2) * scale).max(0)[0]
    y_peak = (y.astype(np.float64).transpose(1, 0, 2) * scale).max(0)
    assert np.allclose(S1["peak_crps"], np.abs(peak - y_peak).mean(), rtol=1e-13)
    ties = refs["ties"]
    assert ties["peak_time"][:, -1].sum() == 0                             # the last time only ever ties
    yhat, scale, y, S, B, base, opts = case_inputs("ties")
    v = yhat.astype(np.float64).reshape(4, S, B, -1) * scale
    assert int((v == base).sum()) >= 2 * len(base) and (y[0, 1, 0].astype(np.float64) * scale[0]) == base[0]
    edges = refs["edges"]
    assert edges["y_when"][0, 0] == 0 and edges["y_when"][1, 0] == edges["M"] - 1
    assert edges["empty_value_windows"] >= 2
    assert refs["far"]["no_onset"] == 1 and (refs["far"]["y_onset"] == refs["far"]["M"]).all()
    assert refs["far"]["onset_skill"] == 0                                 # P = onset[M] = 1 everywhere
    assert refs["plain"]["onset"] is None and "peak_crps" not in refs["plain"]
    assert 0 < refs["BR147"]["no_onset"] < 1 and refs["BR147"]["distinct_when"] > 2


@pytest.mark.parametrize("name", list(CASES))
def test_season_matches_brute_force(pkg, name):
    (T, S, B, R), _ = CASES[name]
    st = targets(name)
    ref = case_reference(name)
    M = ref["M"]
    assert tuple(st.peak_mean.shape) == tuple(st.total_std.shape) == (B, R)
    assert tuple(st.peak_quantiles.shape) == tuple(st.total_quantiles.shape) == (5, B, R)
    assert tuple(st.peak_time.shape) == (B, M, R)
    assert torch.equal(st.peak_time.sum(1) * S, torch.full((B, R), float(S), dtype=torch.float64))
    if name != "plain":
        assert tuple(st.onset.shape) == (B, M + 1, R)
        assert tuple(st.peak_crps.shape) == () and tuple(st.onset_skill_r.shape) == (R,)
    check(st, ref, name)


def test_baseline_forms_and_no_baseline_with_targets(pkg):
    """A scalar baseline is one per region; without a baseline the other scores are still formed."""
    from ude_amd.forecast import Season, ensemble_season
    yhat, scale, y, S, B, _, opts = case_inputs("odd_S")
    args = (torch.from_numpy(yhat), S, B)
    kw = dict(y_true=torch.from_numpy(y), scale=scale, quantiles=[0.5])
    a = ensemble_season(*args, Season(baseline=3.0, run=2), **kw)
    b = ensemble_season(*args, Season(baseline=[3.0], run=2), **kw)
    for f in fields(a):
        assert same_bits(getattr(a, f.name), getattr(b, f.name)), f.name
    check(a, reference(yhat, S, B, (0, 1, 2, 1), scale, y, np.full(1, 3.0), q=[0.5]), "scalar baseline")
    c = ensemble_season(*args, Season(run=2), **kw)
    assert c.onset is None and c.onset_skill is None and c.onset_skill_r is None
    check(c, reference(yhat, S, B, (0, 1, 2, 1), scale, y, None, q=[0.5]), "no baseline")
    d = ensemble_season(*args, Season(run=2), scale=scale)
    assert d.peak_quantiles is None and d.peak_crps is None


def test_season_validation(pkg):
    from ude_amd.forecast import Season, ensemble_season
    s = Season()
    assert (s.baseline, s.start, s.every, s.run, s.window) == (None, 0, 1, 3, 1)
    for bad in (dict(start=-1), dict(every=0), dict(run=0), dict(window=-1), dict(every=1.5), dict(run=True),
                dict(baseline=float("nan")), dict(baseline=[[1.0, 2.0]]), dict(baseline=[])):
        with pytest.raises(ValueError):
            Season(**bad)
    with pytest.raises(Exception):
        s.start = 3                                                         # frozen
    yhat, scale, y = synth(4, 4, 3, 2, seed=1)
    yh, yt = torch.from_numpy(yhat), torch.from_numpy(y)
    with pytest.raises(ValueError):
        ensemble_season(yh, 4, 3, Season(start=4))                          # start < T
    ensemble_season(yh, 4, 3, Season(start=3, run=7))                       # run > M is legal
    with pytest.raises(ValueError):
        ensemble_season(yh, 4, 3, Season(baseline=[1.0, 2.0, 3.0]))         # one per region
    with pytest.raises(ValueError):
        ensemble_season(yh, 3, 4, Season(), y_true=yt)                      # targets are (B, T, R)
    with pytest.raises(ValueError):
        ensemble_season(yh, 5, 3, Season())
    with pytest.raises(ValueError):
        ensemble_season(yh, 4, 3, Season(), quantiles=[1.5])
    with pytest.raises(TypeError):
        ensemble_season(yh, 4, 3, True)
    # the CPU path has no S limit
    big, _, yb = synth(2, 1025, 1, 2, seed=2)
    st = ensemble_season(torch.from_numpy(big), 1025, 1, Season(baseline=2.0, run=1), y_true=torch.from_numpy(yb))
    assert bool(torch.isfinite(st.peak_crps))


def test_season_workspace_rejects_bad_arguments(pkg):
    from ude_amd import _native
    lib = _native.prebuilt()
    # S = 128: G = 8, a quarter of the summary's, so 392 workgroups; 5 partials each + 5 terms per group, doubles
    assert lib.forecast_season_workspace(57, 128, 64, 49, 5, 6, 7, 3, 1) == (392 + 64 * 49) * 5 * 8
    out = ctypes.c_int64(0)
    f = lib.lib.ude_forecast_season_workspace
    assert f(2, 1024, 3, 4, 0, 1, 1, 9, 0, ctypes.byref(out)) == 0          # run > M is legal
    for T, S, B, R, n_q, start, every, run, window in [
            (2, 1025, 3, 4, 0, 0, 1, 1, 0), (0, 8, 3, 4, 0, 0, 1, 1, 0), (2, 0, 3, 4, 0, 0, 1, 1, 0),
            (2, 8, 0, 4, 0, 0, 1, 1, 0), (2, 8, 3, 0, 0, 0, 1, 1, 0), (2, 8, 3, 4, -1, 0, 1, 1, 0),
            (2, 8, 3, 4, 0, -1, 1, 1, 0), (2, 8, 3, 4, 0, 2, 1, 1, 0), (2, 8, 3, 4, 0, 0, 0, 1, 0),
            (2, 8, 3, 4, 0, 0, 1, 0, 0), (2, 8, 3, 4, 0, 0, 1, 1, -1), (65536, 8, 3, 4, 0, 0, 1, 1, 0)]:
        assert f(T, S, B, R, n_q, start, every, run, window, ctypes.byref(out)) == -2, (T, S, B, R, start, every, run)
    assert f(2, 8, 3, 4, 0, 0, 1, 1, 0, None) == -2
    g = lib.lib.ude_forecast_season                                         # checked before any launch
    assert g(2, 8, 3, 4, 2, 1, 1, 0, *([None] * 5), 0, *([None] * 8)) == -2
    assert g(2, 8, 3, 4, 0, 1, 1, 0, *([None] * 5), 0, *([None] * 8)) == -2  # no y_hat


@pytest.mark.parametrize("case", ["e2e_forecast_us", "e2e_forecast_state49"])
@pytest.mark.parametrize("grid", ["weekly", "daily"])
def test_forecast_fills_season(pkg, monkeypatch, case, grid):
    from ude_amd.forecast import Season
    g = load_golden(case)
    base = golden_baseline(g)
    start, every = (6, 7) if grid == "weekly" else (0, 1)
    season = Season(baseline=base, start=start, every=every)
    seen, fc = passthrough(g, "cpu", monkeypatch, season)
    ref = reference(seen["yhat"], seen["S"], seen["B"], (start, every, 3, 1), g["scaler"], g["y_test"], base,
                    q=g["meta"]["quantiles"])
    check(fc.season, ref, f"{case} {grid}")
    # the fixtures are not degenerate: several peak times and onset bins per group, some samples without onset
    assert ref["distinct_when"] > 1.5 and ref["distinct_onset"] >= 2.5 and 0.09 <= ref["no_onset"] <= 0.57, \
        (ref["distinct_when"], ref["distinct_onset"], ref["no_onset"])


def test_season_none_changes_nothing(pkg, monkeypatch):
    from ude_amd.forecast import Season
    g = load_golden("e2e_forecast_us")
    _, plain = run_forecast(g, "cpu", monkeypatch)
    _, none = run_forecast(g, "cpu", monkeypatch, season=None)
    _, on = run_forecast(g, "cpu", monkeypatch, season=Season(baseline=golden_baseline(g), start=6, every=7))
    assert plain.season is None and none.season is None and on.season is not None
    for f in fields(plain):
        if f.name in ("dynamics", "season"):
            continue
        assert same_bits(getattr(plain, f.name), getattr(none, f.name)), f.name
        assert same_bits(getattr(plain, f.name), getattr(on, f.name)), f.name


def test_cpu_and_numpy_carry_the_season(pkg):
    from ude_amd.forecast import Forecast, SeasonTargets
    st = targets("odd_S")
    fc = Forecast(st.peak_mean, st.peak_std, season=st)
    host = fc.cpu()
    assert isinstance(host.season, SeasonTargets) and same_bits(host.season.onset, st.onset)
    arrays = fc.numpy()
    assert isinstance(arrays["season"], dict) and set(arrays["season"]) == {f.name for f in fields(st)}
    assert all(isinstance(arrays["season"][k], np.ndarray) for k in FIELDS)
    assert np.array_equal(arrays["season"]["peak_time"], st.peak_time.numpy())
    half = fc._map(lambda t: t * 0.5)
    assert torch.equal(half.season.peak_time, st.peak_time * 0.5) and half.season.onset is not None
    assert set(SCORES) <= set(arrays["season"])
