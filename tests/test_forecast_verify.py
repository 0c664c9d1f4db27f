"""``verify=`` on the CPU (ude_amd/forecast.py's torch fp64 definitions): CRPS, weighted interval score,
coverage, PIT and the empirical multibin skill, per day and per region, against a brute-force NumPy
reference (forecast_verify_helpers.py); the argument checks; ude_forecast_verify_workspace's shape
checks (host code of the library); and VAE.forecast's pass-through."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from forecast_helpers import synth
from forecast_verify_helpers import (CASES, NEW_FIELDS, OLD_FIELDS, case_inputs, case_reference, check, passthrough,
                                     reference, same_bits, summary)


def test_reference_covers_the_branches(pkg):
    """On the reference alone: the floor path and the ordinary one both run, a target sits on a repeated
    sample, and the PIT histogram is spread."""
    refs = {name: case_reference(name) for name in CASES}
    assert refs["odd_S_12_groups"]["zero_masses"] == 1
    assert refs["far_above"]["zero_masses"] == 10 and refs["far_below"]["zero_masses"] == 12   # of 12: mostly the floor
    assert any(0 < r["zero_masses"] for r in refs.values()) and any(r["zero_masses"] < r["groups"] for r in refs.values())
    assert refs["ties"]["tied_targets"] >= 1 and refs["ties"]["max_tie"] >= 2
    assert refs["S1"]["tied_targets"] == 10                               # t = 0: every target on its sample
    pit = sum(r["pit"].sum(0) for r in refs.values())
    assert int((pit > 0).sum()) >= 3
    assert refs["far_above"]["coverage"].max() == 0 and refs["far_above"]["pit"][:, -1].min() == 1
    assert refs["far_below"]["pit"][:, 0].min() == 1


@pytest.mark.parametrize("name", list(CASES))
def test_verify_matches_brute_force(pkg, name):
    (T, S, B, R), _, _ = CASES[name]
    fc = summary(name, verify=True)
    K, J = 11, 10
    assert tuple(fc.crps.shape) == tuple(fc.wis.shape) == tuple(fc.ens_skill.shape) == (T,)
    assert tuple(fc.coverage.shape) == (K, T) and tuple(fc.pit.shape) == (T, J)
    assert tuple(fc.coverage_r.shape) == (K, T, R)
    for k in ("nll_r", "skill_r", "mae_r", "crps_r", "wis_r", "ens_skill_r"):
        assert tuple(getattr(fc, k).shape) == (T, R), k
    assert torch.allclose(fc.pit.sum(1), torch.ones(T, dtype=torch.float64), rtol=0, atol=1e-14)
    check(fc, case_reference(name), name)


def test_verify_none_changes_nothing(pkg):
    plain, on = summary("no_scale"), summary("no_scale", verify=True)
    for k in NEW_FIELDS:
        assert getattr(plain, k) is None, k
    for k in OLD_FIELDS:
        assert same_bits(getattr(plain, k), getattr(on, k)), k
    again = summary("no_scale", verify=True)
    for k in OLD_FIELDS + NEW_FIELDS:
        assert same_bits(getattr(on, k), getattr(again, k)), k
    host = on.cpu().numpy()
    assert all(isinstance(host[k], np.ndarray) for k in NEW_FIELDS)


def test_custom_verify(pkg):
    from ude_amd.forecast import Verify
    yhat, scale, y, S, B = case_inputs("ties")
    fc = summary("ties", verify=Verify(alphas=(0.5,), pit_bins=4))
    assert tuple(fc.coverage.shape) == (1, 2) and tuple(fc.pit.shape) == (2, 4)
    check(fc, reference(yhat, S, B, scale, y, alphas=(0.5,), J=4), "custom")


def test_verify_argument_errors(pkg):
    from ude_amd.forecast import FLUSIGHT_ALPHAS, Verify, ensemble_summary
    assert Verify().alphas == FLUSIGHT_ALPHAS == (0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)
    assert Verify().pit_bins == 10
    yhat, scale, y = synth(2, 4, 3, 2, seed=1)
    with pytest.raises(ValueError):
        ensemble_summary(torch.from_numpy(yhat), 4, 3, scale=scale, verify=True)          # no targets
    for bad in ((0.0,), (1.0,), (0.2, 1.5), (-0.1,)):
        with pytest.raises(ValueError):
            Verify(alphas=bad)
    with pytest.raises(ValueError):
        Verify(alphas=tuple(np.linspace(0.01, 0.99, 17)))
    Verify(alphas=tuple(np.linspace(0.01, 0.99, 16)), pit_bins=64)
    with pytest.raises(ValueError):
        Verify(pit_bins=65)
    # the CPU path has no S limit
    big, _, yb = synth(1, 1025, 1, 2, seed=2)
    fc = ensemble_summary(torch.from_numpy(big), 1025, 1, y_true=torch.from_numpy(yb), verify=True)
    assert bool(torch.isfinite(fc.crps).all())


def test_verify_workspace_rejects_bad_shapes(pkg):
    from ude_amd import _native
    lib = _native.prebuilt()
    assert lib.forecast_verify_workspace(57, 128, 64, 49, 5, 11, 10) == \
        (57 * 98 * (6 + 11 + 10) + 57 * 7 * 64 * 49) * 8                  # partials + group terms, doubles
    out = ctypes.c_int64(0)
    f = lib.lib.ude_forecast_verify_workspace
    assert f(2, 1024, 3, 4, 0, 16, 64, ctypes.byref(out)) == 0
    for T, S, B, R, n_q, K, J in [(2, 1025, 3, 4, 0, 11, 10), (0, 8, 3, 4, 0, 11, 10), (2, 0, 3, 4, 0, 11, 10),
                                  (2, 8, 0, 4, 0, 11, 10), (2, 8, 3, 0, 0, 11, 10), (2, 8, 3, 4, -1, 11, 10),
                                  (2, 8, 3, 4, 0, 0, 10), (2, 8, 3, 4, 0, 17, 10), (2, 8, 3, 4, 0, 11, 0),
                                  (2, 8, 3, 4, 0, 11, 65), (65536, 8, 3, 4, 0, 11, 10)]:
        assert f(T, S, B, R, n_q, K, J, ctypes.byref(out)) == -2, (T, S, B, R, n_q, K, J)
    assert f(2, 8, 3, 4, 0, 11, 10, None) == -2


def test_forecast_passes_verify_through(pkg, monkeypatch):
    g = load_golden("e2e_forecast_us")
    seen, fc = passthrough(g, "cpu", monkeypatch)
    check(fc, reference(seen["yhat"], seen["S"], seen["B"], g["scaler"], g["y_test"]), "e2e_forecast_us")
