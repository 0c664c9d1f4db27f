"""``verify=`` on the MI355X (ude_forecast_verify, csrc/ude_forecast.h): the ensemble's own scores
against the brute-force NumPy reference of forecast_verify_helpers.py at the shapes where the kernel
takes another path; the shared outputs bit for bit against ude_forecast_summary; run-to-run bits; the
S limit; VAE.forecast's pass-through on the device."""
import pytest
import torch

from conftest import load_golden
from forecast_verify_helpers import (CASES, NEW_FIELDS, OLD_FIELDS, case_inputs, case_reference, check, passthrough,
                                     reference, same_bits, summary)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_verify_kernel_matches_brute_force(pkg, name):
    from ude_amd import fused
    ref = case_reference(name)
    plain = summary(name, "cuda")
    events = []
    fused.EVENTS = events
    try:
        fc = summary(name, "cuda", verify=True)
    finally:
        fused.EVENTS = None
    torch.cuda.synchronize()
    assert [e[0] for e in events] == ["forecast_verify"]                  # the native path ran
    assert fc.crps.is_cuda
    check(fc, ref, name)
    for k in NEW_FIELDS:
        assert getattr(plain, k) is None, k
    for k in OLD_FIELDS:                                                  # the same bits as ude_forecast_summary
        assert same_bits(getattr(plain, k), getattr(fc, k)), k
    again = summary(name, "cuda", verify=True)
    for k in OLD_FIELDS + NEW_FIELDS:
        assert same_bits(getattr(fc, k), getattr(again, k)), k


def test_verify_without_quantiles_keeps_the_bits(pkg):
    """No quantiles asked for: the verify kernel still sorts, the summary kernel does not."""
    from ude_amd.forecast import ensemble_summary
    yhat, scale, y, S, B = case_inputs("tile_width_BR147")
    args = (torch.from_numpy(yhat).cuda(), S, B)
    kw = dict(y_true=torch.from_numpy(y).cuda(), scale=scale)
    plain, fc = ensemble_summary(*args, **kw), ensemble_summary(*args, verify=True, **kw)
    assert fc.quantiles is None
    for k in ("mean", "std", "nll", "skill", "mae"):
        assert same_bits(getattr(plain, k), getattr(fc, k)), k
    check(fc, case_reference("tile_width_BR147"), "no quantiles")


def test_custom_verify_on_the_device(pkg):
    from ude_amd.forecast import Verify
    yhat, scale, y, S, B = case_inputs("ties")
    fc = summary("ties", "cuda", verify=Verify(alphas=(0.5,), pit_bins=4))
    check(fc, reference(yhat, S, B, scale, y, alphas=(0.5,), J=4), "custom")
    fc = summary("ties", "cuda", verify=Verify(alphas=tuple(i / 17 for i in range(1, 17)), pit_bins=64))
    check(fc, reference(yhat, S, B, scale, y, alphas=tuple(i / 17 for i in range(1, 17)), J=64), "16 alphas, 64 bins")


def test_verify_sample_limit_on_the_device(pkg):
    from ude_amd.forecast import ensemble_summary
    yhat = torch.zeros(1, 1025, 2, device="cuda")
    with pytest.raises(ValueError):
        ensemble_summary(yhat, 1025, 1, y_true=torch.zeros(1, 1, 2, device="cuda"), verify=True)


@pytest.mark.parametrize("case", ["e2e_forecast_us", "e2e_forecast_state49"])
def test_forecast_passes_verify_through_on_the_device(pkg, monkeypatch, case):
    g = load_golden(case)
    seen, fc = passthrough(g, "cuda", monkeypatch)
    assert fc.crps.is_cuda
    check(fc, reference(seen["yhat"], seen["S"], seen["B"], g["scaler"], g["y_test"]), case)
