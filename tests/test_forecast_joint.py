"""``joint=`` on the CPU (ude_amd/forecast.py's torch fp64 definitions): the energy and variogram scores of
the ensemble's trajectories on the series, field and joint blocks against a brute-force NumPy reference
(forecast_joint_helpers.py); the identities with the CRPS; the argument checks; ude_forecast_joint's checks
(host code of the library); VAE.forecast's pass-through; and that ``joint=None`` changes nothing."""
import ctypes
from dataclasses import fields

import numpy as np
import pytest
import torch

from conftest import load_golden
from forecast_helpers import run_forecast, synth
from forecast_joint_helpers import (CASES, FIELDS, case_inputs, case_reference, check, identities, one_sample,
                                    passthrough, reference, same_bits, scores)
from helpers import normwise_rel


def test_reference_covers_the_branches(pkg):
    """On the reference alone: each case does what its comment says."""
    refs = {name: case_reference(name) for name in ("S1", "M1", "weekly", "R1", "ties", "S17")}
    yhat, scale, y, S, B, _, p = case_inputs("S1")
    x = yhat.astype(np.float64).reshape(4, 5, 2) * scale                       # S = 1: (T, B, R)
    t = y.astype(np.float64).transpose(1, 0, 2) * scale
    assert np.allclose(refs["S1"]["energy_joint"], np.sqrt(((x - t) ** 2).sum((0, 2))), rtol=1e-14)
    vs = (np.abs(t[0] - t[1]) ** p - np.abs(x[0] - x[1]) ** p) ** 2            # the pair of times 0 and 1
    assert (vs > 0).all() and (refs["S1"]["variogram_series"] >= vs).all()
    assert refs["M1"]["M"] == 1 and not refs["M1"]["variogram_series"].any() and refs["M1"]["variogram_field"].all()
    assert refs["weekly"]["M"] == 4 and refs["weekly"]["energy_joint"].max() < 100   # no skipped 1e30 shows
    assert not refs["R1"]["variogram_field"].any() and refs["R1"]["variogram_series"].all()
    yhat, scale, y, S, B, _, _ = case_inputs("ties")
    v = yhat.reshape(4, S, B, 10)
    assert np.array_equal(v[:, 0], v[:, 1]) and np.array_equal(v[:, S - 1], v[:, S // 2])
    assert np.array_equal(y[0], v[:, 3, 0])
    # the score is no small difference of its two terms: the subtraction costs under one digit
    assert min(case_reference(name)["joint_over_first"] for name in CASES) >= 0.1


@pytest.mark.parametrize("name", list(CASES))
def test_joint_matches_brute_force(pkg, name):
    (T, S, B, R), _, _ = CASES[name]
    js = scores(name)
    ref = case_reference(name)
    M = ref["M"]
    assert tuple(js.energy_joint.shape) == (B,) and tuple(js.energy_joint_mean.shape) == ()
    assert tuple(js.energy_series.shape) == tuple(js.variogram_series.shape) == (B, R)
    assert tuple(js.energy_field.shape) == tuple(js.variogram_field.shape) == (B, M)
    assert tuple(js.energy_series_r.shape) == tuple(js.variogram_series_r.shape) == (R,)
    assert tuple(js.energy_field_t.shape) == tuple(js.variogram_field_t.shape) == (M,)
    check(js, ref, name)


def test_one_sample_has_no_pair_term(pkg):
    """S = 1: ES = |x - y| with nothing subtracted."""
    one_sample(scores("S1"))


def test_one_dimension_is_the_crps(pkg):
    """R = 1: the field block is one number and its energy score the CRPS of ``verify=``; M = 1: the series
    block is that day's value."""
    from ude_amd.forecast import ensemble_summary
    yhat, scale, y, S, B, _, _ = case_inputs("R1")
    fc = ensemble_summary(torch.from_numpy(yhat), S, B, y_true=torch.from_numpy(y), scale=scale, verify=True)
    js = scores("R1")
    e = normwise_rel(js.energy_field_t, fc.crps)
    assert e <= 1e-10, e
    yhat, scale, y, S, B, (start, _), _ = case_inputs("M1")
    fc = ensemble_summary(torch.from_numpy(yhat), S, B, y_true=torch.from_numpy(y), scale=scale, verify=True)
    e = normwise_rel(scores("M1").energy_series_r, fc.crps_r[start])
    assert e <= 1e-10, e


def test_identities(pkg):
    from ude_amd.forecast import Joint, ensemble_joint
    identities(ensemble_joint, Joint, "cpu")


def test_joint_validation(pkg):
    from ude_amd.forecast import Joint, ensemble_joint
    j = Joint()
    assert (j.start, j.every, j.p) == (0, 1, 0.5) and j.times(57) == 57 and Joint(6, 7).times(57) == 8
    for bad in (dict(start=-1), dict(every=0), dict(every=1.5), dict(start=True), dict(p=2.0), dict(p=0), dict(p=True),
                dict(p="half")):
        with pytest.raises(ValueError):
            Joint(**bad)
    with pytest.raises(Exception):
        j.start = 3                                                         # frozen
    yhat, scale, y = synth(4, 4, 3, 2, seed=1)
    yh, yt = torch.from_numpy(yhat), torch.from_numpy(y)
    with pytest.raises(ValueError):
        ensemble_joint(yh, 4, 3, None)                                      # the targets are required
    with pytest.raises(ValueError):
        ensemble_joint(yh, 4, 3, yt, Joint(start=4))                        # start < T
    with pytest.raises(ValueError):
        ensemble_joint(yh, 3, 4, yt)                                        # targets are (B, T, R)
    with pytest.raises(ValueError):
        ensemble_joint(yh, 5, 3, yt)
    with pytest.raises(ValueError):
        ensemble_joint(yh, 4, 3, yt, scale=[1.0, 2.0, 3.0])                 # one per region
    with pytest.raises(TypeError):
        ensemble_joint(yh, 4, 3, yt, True)
    # the CPU path has no S limit
    big, _, yb = synth(2, 1025, 1, 2, seed=2)
    js = ensemble_joint(torch.from_numpy(big), 1025, 1, torch.from_numpy(yb))
    assert bool(torch.isfinite(js.energy_joint_mean))


def test_joint_entry_rejects_bad_arguments(pkg):
    from ude_amd import _native
    lib = _native.prebuilt()
    # S = 128: 8 tiles of 16 per side, 36 tile pairs; per window and pair two rows of 1 + R + M doubles
    assert lib.forecast_joint_workspace(57, 128, 64, 49, 0, 1, 1) == 64 * 36 * 2 * (1 + 49 + 57) * 8
    assert lib.forecast_joint_workspace(57, 17, 2, 3, 6, 7, 2) == 2 * 3 * 2 * (1 + 3 + 8) * 8
    out = ctypes.c_int64(0)
    f = lib.lib.ude_forecast_joint_workspace
    assert f(2, 1024, 3, 4, 1, 9, 2, ctypes.byref(out)) == 0
    for T, S, B, R, start, every, p_code in [
            (2, 1025, 3, 4, 0, 1, 1), (0, 8, 3, 4, 0, 1, 1), (2, 0, 3, 4, 0, 1, 1), (2, 8, 0, 4, 0, 1, 1),
            (2, 8, 3, 0, 0, 1, 1), (2, 8, 3, 4, -1, 1, 1), (2, 8, 3, 4, 2, 1, 1), (2, 8, 3, 4, 0, 0, 1),
            (2, 8, 3, 4, 0, 1, 0), (2, 8, 3, 4, 0, 1, 3), (65536, 8, 3, 4, 0, 1, 1), (2, 8, 3, 4097, 0, 1, 1),
            (4097, 8, 3, 4, 0, 1, 1), (2, 8, 65536, 4, 0, 1, 1)]:
        assert f(T, S, B, R, start, every, p_code, ctypes.byref(out)) == -2, (T, S, B, R, start, every, p_code)
    assert f(4097, 8, 3, 4, 1, 2, 1, ctypes.byref(out)) == 0                # M = 2048
    assert f(2, 8, 3, 4, 0, 1, 1, None) == -2
    g = lib.lib.ude_forecast_joint                                          # checked before any launch
    one = ctypes.c_void_p(8)                                                # never dereferenced: a check fails first
    assert g(2, 8, 3, 4, 0, 1, 1, *([None] * 11)) == -2                     # null pointers
    for k in (0, 2, 3, 4, 5, 6, 7, 8, 9):                                   # each required pointer (scale may be null)
        args = [one] * 10
        args[k] = None
        assert g(2, 8, 3, 4, 0, 1, 1, *args, None) == -2, k
    assert g(2, 8, 3, 4, 2, 1, 1, *([one] * 10), None) == -2                # start
    assert g(2, 8, 3, 4, 0, 0, 1, *([one] * 10), None) == -2                # every
    assert g(2, 8, 3, 4, 0, 1, 4, *([one] * 10), None) == -2                # p_code
    assert g(2, 1025, 3, 4, 0, 1, 1, *([one] * 10), None) == -2             # S


@pytest.mark.parametrize("case", ["e2e_forecast_us", "e2e_forecast_state49"])
def test_forecast_fills_joint(pkg, monkeypatch, case):
    from ude_amd.forecast import JointScores
    g = load_golden(case)
    seen, fc = passthrough(g, "cpu", monkeypatch, True)
    assert isinstance(fc.joint, JointScores)
    ref = reference(seen["yhat"], seen["S"], seen["B"], (0, 1), 0.5, g["scaler"], g["y_test"])
    check(fc.joint, ref, case)


def test_forecast_joint_arguments(pkg, monkeypatch):
    from ude_amd.forecast import Joint
    g = load_golden("e2e_forecast_us")
    with pytest.raises(TypeError):
        run_forecast(g, "cpu", monkeypatch, joint="yes")
    with pytest.raises(TypeError):
        run_forecast(g, "cpu", monkeypatch, joint=False)
    import forecast_helpers
    model = forecast_helpers.build_vae(g, "cpu")
    with pytest.raises(ValueError):
        model.forecast(torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), n_samples=4, joint=True)   # no y_true
    seen, fc = passthrough(g, "cpu", monkeypatch, Joint(start=6, every=7, p=1.0))
    check(fc.joint, reference(seen["yhat"], seen["S"], seen["B"], (6, 7), 1.0, g["scaler"], g["y_test"]), "weekly p1")


def test_joint_none_changes_nothing(pkg, monkeypatch):
    g = load_golden("e2e_forecast_us")
    _, plain = run_forecast(g, "cpu", monkeypatch)
    _, none = run_forecast(g, "cpu", monkeypatch, joint=None)
    _, on = run_forecast(g, "cpu", monkeypatch, joint=True)
    assert plain.joint is None and none.joint is None and on.joint is not None
    for f in fields(plain):
        if f.name in ("dynamics", "season", "scenarios", "joint"):
            continue
        assert same_bits(getattr(plain, f.name), getattr(none, f.name)), f.name
        assert same_bits(getattr(plain, f.name), getattr(on, f.name)), f.name


def test_cpu_and_numpy_carry_the_joint_scores(pkg):
    from ude_amd.forecast import Forecast, JointScores
    js = scores("odd_S")
    fc = Forecast(js.energy_series, js.energy_series, joint=js)
    assert [f.name for f in fields(Forecast)][-1] == "joint"               # placed last: positional construction stands
    host = fc.cpu()
    assert isinstance(host.joint, JointScores) and same_bits(host.joint.energy_field, js.energy_field)
    arrays = fc.numpy()
    assert isinstance(arrays["joint"], dict) and set(arrays["joint"]) == set(FIELDS)
    assert all(isinstance(arrays["joint"][k], np.ndarray) for k in FIELDS)
    half = fc._map(lambda t: t * 0.5)
    assert torch.equal(half.joint.variogram_field, js.variogram_field * 0.5)
