"""``season=`` on the MI355X (ude_forecast_season, csrc/ude_season.h): the seasonal targets against the
brute-force NumPy reference of forecast_season_helpers.py at the shapes where the kernel takes another
path; run-to-run bits; the one-time case against the summary kernel; the S limit; VAE.forecast end to
end on the device."""
from dataclasses import fields

import pytest
import torch

from conftest import load_golden
from forecast_season_helpers import (CASES, LEVELS, case_inputs, case_reference, check, golden_baseline, passthrough,
                                     reference, same_bits, targets)
from helpers import normwise_rel

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_season_kernel_matches_brute_force(pkg, name):
    from ude_amd import fused
    ref = case_reference(name)
    events = []
    fused.EVENTS = events
    try:
        st = targets(name, "cuda")
    finally:
        fused.EVENTS = None
    torch.cuda.synchronize()
    assert [e[0] for e in events] == ["forecast_season"]                  # the native path ran
    assert st.peak_mean.is_cuda and st.peak_time.is_cuda
    check(st, ref, name)
    again = targets(name, "cuda")
    for f in fields(st):
        assert same_bits(getattr(st, f.name), getattr(again, f.name)), f.name


@pytest.mark.parametrize("name", ["M1", "M1_run2"])
def test_one_considered_time_is_the_summary_of_that_day(pkg, name):
    """M = 1: every trajectory's peak and total are its value at that time index."""
    from ude_amd.forecast import ensemble_summary
    yhat, scale, y, S, B, _, (start, _, _, _) = case_inputs(name)
    st = targets(name, "cuda")
    fc = ensemble_summary(torch.from_numpy(yhat).cuda(), S, B, scale=scale, quantiles=LEVELS)
    for k in ("peak", "total"):
        for stat in ("mean", "std"):
            e = normwise_rel(getattr(st, f"{k}_{stat}"), getattr(fc, stat)[:, start])
            assert e <= 1e-10, (k, stat, e)
        assert torch.equal(getattr(st, f"{k}_quantiles"), fc.quantiles[:, :, start]), k
    assert torch.equal(st.peak_time, torch.ones_like(st.peak_time))


def test_season_sample_limit_on_the_device(pkg):
    from ude_amd.forecast import Season, ensemble_season
    with pytest.raises(ValueError):
        ensemble_season(torch.zeros(2, 1025, 2, device="cuda"), 1025, 1, Season())


@pytest.mark.parametrize("case", ["e2e_forecast_us", "e2e_forecast_state49"])
@pytest.mark.parametrize("start,every", [(6, 7), (0, 1)])
def test_forecast_fills_season_on_the_device(pkg, monkeypatch, case, start, every):
    from ude_amd import fused
    from ude_amd.forecast import Season
    g = load_golden(case)
    base = golden_baseline(g)
    events = []
    fused.EVENTS = events
    try:
        seen, fc = passthrough(g, "cuda", monkeypatch, Season(baseline=base, start=start, every=every))
    finally:
        fused.EVENTS = None
    torch.cuda.synchronize()
    assert [e[0] for e in events] == ["forecast_dec", "forecast_summary", "forecast_season"]
    assert fc.season.peak_time.is_cuda
    check(fc.season, reference(seen["yhat"], seen["S"], seen["B"], (start, every, 3, 1), g["scaler"], g["y_test"], base,
                               q=g["meta"]["quantiles"]), case)
    host = fc.cpu()
    assert not host.season.onset.is_cuda and torch.equal(host.season.onset, fc.season.onset.cpu())
