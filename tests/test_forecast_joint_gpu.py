"""``joint=`` on the MI355X (ude_forecast_joint, csrc/ude_joint.h): the energy and variogram scores against the
brute-force NumPy reference of forecast_joint_helpers.py at the shapes where the kernels take another path;
run-to-run bits; the identities; the S limit; VAE.forecast end to end on the device."""
from dataclasses import fields

import pytest
import torch

from conftest import load_golden
from forecast_helpers import run_forecast
from forecast_joint_helpers import (CASES, case_inputs, case_reference, check, identities, one_sample, passthrough,
                                    reference, same_bits, scores)
from helpers import normwise_rel

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
def test_joint_kernels_match_brute_force(pkg, name):
    ref = case_reference(name)
    js, kinds = recorded(lambda: scores(name, "cuda"))
    assert kinds == ["forecast_joint"]                                      # the native path ran
    assert all(getattr(js, f.name).is_cuda for f in fields(js))
    check(js, ref, name)
    again = scores(name, "cuda")
    for f in fields(js):
        assert same_bits(getattr(js, f.name), getattr(again, f.name)), f.name


def test_one_sample_has_no_pair_term_on_the_device(pkg):
    one_sample(scores("S1", "cuda"))


def test_one_dimension_is_the_crps_on_the_device(pkg):
    from ude_amd.forecast import ensemble_summary
    yhat, scale, y, S, B, _, _ = case_inputs("R1")
    fc = ensemble_summary(torch.from_numpy(yhat).cuda(), S, B, y_true=torch.from_numpy(y).cuda(), scale=scale,
                          verify=True)
    e = normwise_rel(scores("R1", "cuda").energy_field_t, fc.crps)
    assert e <= 1e-10, e
    yhat, scale, y, S, B, (start, _), _ = case_inputs("M1")
    fc = ensemble_summary(torch.from_numpy(yhat).cuda(), S, B, y_true=torch.from_numpy(y).cuda(), scale=scale,
                          verify=True)
    e = normwise_rel(scores("M1", "cuda").energy_series_r, fc.crps_r[start])
    assert e <= 1e-10, e


def test_identities_on_the_device(pkg):
    from ude_amd.forecast import Joint, ensemble_joint
    identities(ensemble_joint, Joint, "cuda")


def test_joint_sample_limit_on_the_device(pkg):
    from ude_amd.forecast import ensemble_joint
    with pytest.raises(ValueError):
        ensemble_joint(torch.zeros(2, 1025, 2, device="cuda"), 1025, 1, torch.zeros(1, 2, 2, device="cuda"))


@pytest.mark.parametrize("case", ["e2e_forecast_us", "e2e_forecast_state49"])
def test_forecast_fills_joint_on_the_device(pkg, monkeypatch, case):
    g = load_golden(case)
    (seen, fc), kinds = recorded(lambda: passthrough(g, "cuda", monkeypatch, True))
    assert kinds == ["forecast_dec", "forecast_summary", "forecast_joint"]
    assert all(v.is_cuda for _, v in fc.joint._tensors())
    check(fc.joint, reference(seen["yhat"], seen["S"], seen["B"], (0, 1), 0.5, g["scaler"], g["y_test"]), case)
    host = fc.cpu()
    for f in fields(host.joint):
        a, b = getattr(host.joint, f.name), getattr(fc.joint, f.name)
        assert not a.is_cuda and torch.equal(a, b.cpu()), f.name


def test_joint_none_launches_nothing(pkg, monkeypatch):
    g = load_golden("e2e_forecast_us")
    (_, fc), kinds = recorded(lambda: run_forecast(g, "cuda", monkeypatch, joint=None))
    assert fc.joint is None and "forecast_joint" not in kinds
    assert kinds == ["forecast_dec", "forecast_summary"]
