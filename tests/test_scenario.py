"""Scenario forecasts on the host: ``ude_amd.forecast.Scenario`` (validation, broadcasting, the expansion of
output intervals to RK4 steps), the eager route ``scenario_latent`` against the fp64 / fp32 oracle restated
with per-step scaled rates (tests/scenario_helpers.py), and ``VAE.forecast(scenarios=...)``: the baseline is the
forecast without scenarios bit for bit, the effect is the summary of the paired difference."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import module_from_golden, normwise_rel, step_of
from forecast_helpers import run_forecast
from scenario_helpers import GAMMA_MIN, MARGIN_MIN, SCN_CASES, bar, reference, scn_table

BASE_FIELDS = ("mean", "std", "quantiles", "nll", "skill", "mae")


# ---- 1. Scenario -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf"), [1.0, -1.0], np.ones((2, 2, 2)), "x"])
def test_scenario_rejects_bad_values(pkg, bad):
    from ude_amd.forecast import Scenario
    with pytest.raises(ValueError):
        Scenario(beta=bad)
    with pytest.raises(ValueError):
        Scenario(gamma=bad)


def test_scenario_rejects_wrong_shapes(pkg):
    from ude_amd.forecast import Scenario
    T, R = 5, 3
    for bad in (np.ones(7), np.ones((4, 2)), np.ones((3, 3)), np.ones((5, 3))):
        with pytest.raises(ValueError):
            Scenario(beta=bad).intervals(T, R)
        with pytest.raises(ValueError):
            Scenario(gamma=bad).intervals(T, R)


def test_scenario_broadcasting(pkg):
    from ude_amd.forecast import Scenario
    T, R = 5, 3
    m = Scenario().intervals(T, R)
    assert m.shape == (4, 3, 2) and m.dtype == np.float32 and (m == 1).all()
    m = Scenario(beta=0.7, gamma=1.5).intervals(T, R)
    assert (m[..., 0] == np.float32(0.7)).all() and (m[..., 1] == np.float32(1.5)).all()
    per_t = np.array([1.0, 0.9, 0.8, 0.7])
    m = Scenario(beta=per_t).intervals(T, R)
    assert np.array_equal(m[..., 0], np.broadcast_to(per_t.astype(np.float32)[:, None], (4, 3))) and (m[..., 1] == 1).all()
    full = np.arange(12, dtype=np.float64).reshape(4, 3) / 10
    m = Scenario(gamma=full, beta=torch.tensor([0.5, 1.0, 2.0])).intervals(T, R)
    assert np.array_equal(m[..., 1], full.astype(np.float32))
    assert np.array_equal(m[..., 0], np.broadcast_to(np.float32([0.5, 1.0, 2.0]), (4, 3)))       # a (R,) row
    assert np.array_equal(Scenario(beta=np.float64([[0.5, 1.0, 2.0]])).intervals(T, R)[..., 0], m[..., 0])   # (1, R)


def test_scenario_from_day(pkg):
    from ude_amd.forecast import Scenario
    T, R = 6, 2
    m = Scenario.from_day(T, 2, beta=0.7).intervals(T, R)
    assert (m[:2] == 1).all() and (m[2:, :, 0] == np.float32(0.7)).all() and (m[..., 1] == 1).all()
    m = Scenario.from_day(T, 0, beta=[0.5, 1.0], gamma=2.0).intervals(T, R)
    assert (m[:, 0, 0] == 0.5).all() and (m[:, 1, 0] == 1).all() and (m[..., 1] == 2).all()
    assert (Scenario.from_day(T, T - 1, beta=0.0).intervals(T, R) == 1).all()                  # starts past the end
    for bad in (-1, T, 1.5):
        with pytest.raises(ValueError):
            Scenario.from_day(T, bad)
    with pytest.raises(ValueError):
        Scenario.from_day(T, 1, beta=-0.5)


def test_interval_to_step_expansion(pkg):
    from ude_amd.forecast import Scenario
    from ude_amd.schedule import build_schedule
    T, R = 4, 3
    t = torch.arange(T, dtype=torch.float32)
    rows = np.arange(9, dtype=np.float64).reshape(3, 3) / 8 + 0.25
    sc = Scenario(beta=rows, gamma=np.array([1.0, 2.0, 3.0]))
    one = sc.table(build_schedule(t, t[1] - t[0]), R)
    assert one.dtype == torch.float32 and tuple(one.shape) == (3, R, 2)
    assert np.array_equal(one.numpy(), sc.intervals(T, R))
    two = sc.table(build_schedule(t, (t[1] - t[0]) / 2), R)
    assert tuple(two.shape) == (6, R, 2)
    assert torch.equal(two[0::2], one) and torch.equal(two[1::2], one)                          # rows repeat pairwise
    with pytest.raises(ValueError):                                                             # outputs between grid points
        sc.table(build_schedule(t, (t[1] - t[0]) * 0.75), R)


# ---- 2. - 4. scenario_latent -----------------------------------------------------------------------------

@pytest.mark.parametrize("case", SCN_CASES)
def test_reference_conditions(case):
    _g, ref64, _ref32, _table = reference(case)
    assert ref64["margin"] >= MARGIN_MIN, ref64["margin"]
    assert ref64["gamma_min"] >= GAMMA_MIN, ref64["gamma_min"]


@pytest.mark.parametrize("case", SCN_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_scenario_latent_matches_the_restated_oracle(pkg, case, dtype):
    from ude_amd.forecast import scenario_latent
    g, ref64, ref32, table = reference(case)
    mod = module_from_golden(pkg, g, "cpu").to(dtype)
    t, step = step_of(g)
    n_p, n_t = len(mod.params), len(mod.tracker)
    latent = scenario_latent(mod, torch.from_numpy(g["y0"]).to(dtype), t.to(dtype), step.to(dtype), table)
    assert mod.rate_scale is None and (len(mod.params), len(mod.tracker)) == (n_p, n_t)
    assert latent.dtype == dtype and tuple(latent.shape) == tuple(ref64["latent"].shape)
    e = normwise_rel(latent[..., :3], ref64["latent"][..., :3])
    print(case, f"{e:.2e}")
    if dtype == torch.float64:
        assert e <= 1e-10, e
    else:
        assert e <= bar({"l": ref64["latent"][..., :3]}, {"l": ref32["latent"][..., :3]}, "l"), e
    assert torch.equal(latent[..., 3:], latent[:1, ..., 3:].expand_as(latent[..., 3:]))           # static dims carried


def test_rate_scale_is_restored_after_an_exception(pkg):
    from ude_amd.forecast import scenario_latent
    g, _r64, _r32, table = reference("e2e_dyn_fafp_r1")
    mod = module_from_golden(pkg, g, "cpu")
    t, step = step_of(g)
    before = [torch.ones(1)]
    mod.params = before
    with pytest.raises(RuntimeError):
        scenario_latent(mod, torch.from_numpy(g["y0"])[:, :, :5], t, step, table)           # a state the net cannot take
    assert mod.rate_scale is None and mod.params is before and mod.tracker == []
    with pytest.raises(ValueError):
        scenario_latent(mod, torch.from_numpy(g["y0"]), t, step, table[:2])


@pytest.mark.parametrize("case", SCN_CASES)
def test_a_table_of_ones_is_odeint(pkg, case):
    from ude_amd.forecast import scenario_latent
    g = load_golden(case)
    mod = module_from_golden(pkg, g, "cpu")
    t, step = step_of(g)
    y0 = torch.from_numpy(g["y0"])
    with torch.no_grad():
        want = pkg.odeint(mod, y0, t, method="rk4", options=dict(step_size=step))
    mod.clear_tracking()
    got = scenario_latent(mod, y0, t, step, torch.ones(len(t) - 1, g["meta"]["n_regions"], 2))
    assert torch.equal(got, want)


def test_no_transmission_keeps_s_and_lets_i_decay(pkg):
    from ude_amd.forecast import scenario_latent
    g = load_golden("e2e_dyn_fp_r10")
    mod = module_from_golden(pkg, g, "cpu")
    t, step = step_of(g)
    y0 = torch.from_numpy(g["y0"])
    table = torch.ones(len(t) - 1, 10, 2)
    table[..., 0] = 0.0
    latent = scenario_latent(mod, y0, t, step, table)
    assert torch.equal(latent[..., 0], y0[..., 0].expand_as(latent[..., 0]))                      # S: bit for bit
    assert bool((y0[..., 1] > 0).all()) and bool((latent[1:, ..., 1] <= latent[:-1, ..., 1]).all())


# ---- 5. VAE.forecast(scenarios=...) ----------------------------------------------------------------------

def _tracking(ode):
    params = [p.clone() for p in ode.params]
    tracker = [torch.as_tensor(v).clone() for v in ode.tracker]
    post = ode.posterior()
    return params, tracker, post.loc.clone(), post.scale.clone()


@pytest.fixture(scope="module")
def us_runs(pkg):
    """The US forecast fixture on the host without scenarios and with two (one the identity), same draw; the
    generator state after each call (from the same state before)."""
    from ude_amd.forecast import Scenario, Season
    g = load_golden("e2e_forecast_us")
    T = len(g["t"])
    season = Season(start=6, every=7, baseline=None)
    scen = {"same": Scenario(), "less": Scenario.from_day(T, 0, beta=0.7)}
    out = {}
    for key, kw in (("plain", {}), ("scn", dict(scenarios=scen))):
        mp = pytest.MonkeyPatch()
        torch.manual_seed(11)
        model, fc = run_forecast(g, "cpu", mp, season=season, dynamics=True, **kw)
        out[key] = (model, fc, torch.get_rng_state(), model.latent.detach().clone(), _tracking(model.ode))
    return g, season, out


def test_baseline_is_untouched_by_scenarios(us_runs):
    _g, _season, runs = us_runs
    (_, fc0, rng0, lat0, tr0), (_, fc1, rng1, lat1, tr1) = runs["plain"], runs["scn"]
    assert fc0.scenarios is None and set(fc1.scenarios) == {"same", "less"}
    a, b = [v for _, v in fc0._tensors()], [v for _, v in fc1._map(lambda v: v)._tensors()]
    n0 = len(a)
    assert n0 > 6 and all(torch.equal(x, y) for x, y in zip(a, b[:n0]))                           # every baseline field
    for k in BASE_FIELDS:
        assert torch.equal(getattr(fc0, k), getattr(fc1, k)), k
    assert torch.equal(rng0, rng1) and torch.equal(lat0, lat1)
    assert len(tr0[0]) == len(tr1[0]) > 0 and all(torch.equal(x, y) for x, y in zip(tr0[0], tr1[0]))
    assert len(tr0[1]) == len(tr1[1]) > 0 and all(torch.equal(x, y) for x, y in zip(tr0[1], tr1[1]))
    assert torch.equal(tr0[2], tr1[2]) and torch.equal(tr0[3], tr1[3])
    assert runs["scn"][0].ode.rate_scale is None


def test_effect_is_the_summary_of_the_paired_difference(pkg, us_runs):
    from ude_amd.forecast import ScenarioForecast, ensemble_season, ensemble_summary, scenario_latent, Scenario
    from ude_amd.schedule import build_schedule
    g, season, runs = us_runs
    model, fc, _rng, latent, _ = runs["scn"]
    m = g["meta"]
    S, B, R, Q = m["n_samples"], m["B"], m["n_regions"], m["quantiles"]
    t = torch.from_numpy(g["t"])
    T = len(t)
    less = fc.scenarios["less"]
    assert isinstance(less, ScenarioForecast)
    assert less.forecast.nll is None and less.forecast.skill is None and less.forecast.scenarios is None
    assert less.forecast.dynamics is not None and less.forecast.season is not None
    assert less.forecast.season.peak_crps is None                                                 # no targets
    # by hand: the same z (latent[0]), the eager route, the decoder, the difference
    table = torch.ones(T - 1, R, 2)
    table[..., 0] = 0.7
    with torch.no_grad():
        lat_s = scenario_latent(model.ode, latent[0], t, t[1] - t[0], table)
        yhat_s = model.dec(lat_s[..., :3]).reshape(T, S * B, R)
        yhat_b = model.dec(latent[..., :3]).reshape(T, S * B, R)
    want = ensemble_summary(yhat_s - yhat_b, S, B, scale=g["scaler"], quantiles=Q)
    for k in ("mean", "std", "quantiles"):
        assert torch.equal(getattr(less.effect, k), getattr(want, k)), k
    own = ensemble_summary(yhat_s, S, B, scale=g["scaler"], quantiles=Q)
    assert torch.equal(less.forecast.mean, own.mean) and torch.equal(less.forecast.quantiles, own.quantiles)
    st = ensemble_season(yhat_s - yhat_b, S, B, season, scale=g["scaler"], quantiles=Q)
    assert torch.equal(less.effect_season.total_mean, st.total_mean)
    assert torch.equal(less.effect_season.total_std, st.total_std)
    assert torch.equal(less.effect_season.total_quantiles, st.total_quantiles)
    # less transmission from day 0 lowers the mean season total, and beta' is what the dynamics report
    assert float(less.forecast.season.total_mean.mean()) < float(fc.season.total_mean.mean())
    assert float(less.effect_season.total_mean.mean()) < 0
    e = normwise_rel(less.forecast.dynamics["beta"][0][:, 0], 0.7 * fc.dynamics["beta"][0][:, 0])
    assert e <= 1e-6, e                                                                           # day 0: the same state
    assert less.rates.mean.shape == (2,) and float(less.rates.mean[0]) < float(fc.scenarios["same"].rates.mean[0])


def test_identity_scenario_has_no_effect(us_runs):
    _g, _season, runs = us_runs
    fc = runs["scn"][1]
    same = fc.scenarios["same"]
    assert bool((same.effect.mean == 0).all()) and bool((same.effect.std == 0).all())
    assert torch.equal(same.forecast.mean, fc.mean) and torch.equal(same.forecast.std, fc.std)
    assert torch.equal(same.forecast.dynamics.mean, fc.dynamics.mean)
    assert bool((same.effect_season.total_mean == 0).all())


def test_cpu_and_numpy_carry_the_nesting(us_runs):
    _g, _season, runs = us_runs
    fc = runs["scn"][1]
    assert fc.cpu() is fc
    half = fc._map(lambda v: v.float())
    assert half.scenarios["less"].effect.mean.dtype == torch.float32
    assert half.scenarios["less"].forecast.dynamics.names == fc.dynamics.names
    assert half.scenarios["less"].rates.mean.dtype == torch.float32
    names = [n for n, _ in fc._tensors()]
    assert len(names) == len(runs["plain"][1]._tensors()) + 2 * len(fc.scenarios["less"]._tensors())
    n = fc.numpy()
    assert set(n["scenarios"]) == {"same", "less"}
    assert isinstance(n["scenarios"]["less"]["effect"]["mean"], np.ndarray)
    assert n["scenarios"]["less"]["effect_season"]["total_mean"].shape == tuple(fc.season.total_mean.shape)
    assert runs["plain"][1].numpy()["scenarios"] is None


# ---- 6. models without a scenario ------------------------------------------------------------------------

def test_fa_only_and_bayes_raise(pkg, monkeypatch):
    import lib.VAE as vae_mod
    import lib.models as models
    from ude_amd.forecast import Scenario
    torch.manual_seed(5)
    model = vae_mod.VAE(models.Encoder_Back_GRU, models.Fa, models.Decoder, 4, 8, 2,
                        ode_params=dict(aug_net_sizes=[16, 16]),
                        enc_params={"q_sizes": [16, 8], "ff_sizes": [8, 8], "SIR_scaler": [0.1, 0.05, 1.0]},
                        uncertainty=True, ode_kl_w=1 / 153)
    x, t = torch.rand(3, 8, 10), torch.arange(5, dtype=torch.float32) / 7
    rng = torch.get_rng_state()
    with pytest.raises(ValueError, match="rate net"):
        model.forecast(x, t, n_samples=4, scenarios={"a": Scenario(beta=0.5)})
    assert torch.equal(torch.get_rng_state(), rng)                                                # refused before the draw
    with pytest.raises(TypeError):
        model.forecast(x, t, n_samples=4, scenarios={"a": 0.5})
    g = load_golden("e2e_forecast_us_bayes")
    with pytest.raises(ValueError, match="Bayesian"):
        run_forecast(g, "cpu", monkeypatch, scenarios={"a": Scenario(beta=0.5)})
