"""Scenario forecasts on the MI355X: the inference decoder-epilogue solve with the rates scaled per RK4 step
and region (ude_rk4_forecast_scn) -- a table of ones against the plain forecast solves bit for bit, the test
table against the fp64 oracle restated with scaled rates (tests/scenario_helpers.py), guard bands behind the
output and around the table, several steps per output interval, the models without such a kernel, and
``VAE.forecast(scenarios=...)`` end to end."""
import ctypes

import pytest
import torch

from conftest import load_golden
from helpers import module_from_golden, normwise_rel, step_of
from forecast_helpers import build_vae, run_forecast
from scenario_helpers import GAMMA_MIN, MARGIN_MIN, SCN_CASES, bar, reference, scn_table

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 4096


def _decoder(R):
    torch.manual_seed(R)
    return torch.nn.Linear(3 * R, R).cuda()


def _stats(ode):
    n_eval, stats, sums = ode._fused_sums[-1]
    return [s.detach().clone() for s in stats]


def _identity_checks(ode, y0, t, step, lin):
    """ude_rk4_forecast_scn with a table of ones is ude_rk4_forecast_dec / _dyn: y_hat, dyn, statistics."""
    from ude_amd import solvers
    from ude_amd.forecast import _forecast_plan, solve_decode_dynamics, solve_decode_forecast, solve_decode_scenario
    R = y0.shape[1]
    ode.clear_tracking()
    y_dec = solve_decode_forecast(ode, y0, t, step, lin)
    assert y_dec is not None
    st_dec = _stats(ode)
    ode.clear_tracking()
    _y, dyn_ref, names_ref = solve_decode_dynamics(ode, y0, t, step, lin)
    ode.clear_tracking()
    ones = torch.ones(_forecast_plan(ode, y0, t, step).prob.n_steps, R, 2, device="cuda")
    for flag in (False, True):
        y_scn, dyn, names, rates = solve_decode_scenario(ode, y0, t, step, lin, ones, dynamics=flag)
        torch.cuda.synchronize()
        assert torch.equal(y_scn, y_dec)
        assert torch.equal(rates.mean, st_dec[0]) and torch.equal(rates.std, st_dec[1])
        assert torch.equal(rates.fa_norm, st_dec[2])
        assert names == names_ref
        if flag:
            assert torch.equal(dyn, dyn_ref)
        else:
            assert dyn is None
    assert ode._fused_sums == [] and ode._fused_rates == [] and ode.tracker == []     # nothing recorded on the RHS


# ---- 1. identity -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SCN_CASES)
def test_table_of_ones_is_the_plain_solve(pkg, case):
    g = load_golden(case)
    mod = module_from_golden(pkg, g, "cuda")
    t, step = step_of(g)
    y0 = torch.from_numpy(g["y0"]).cuda()
    assert y0.shape[0] == 20                                            # one full tile and a ragged one: resident kernel
    _identity_checks(mod, y0, t, step, _decoder(g["meta"]["n_regions"]))


def test_table_of_ones_more_tiles_than_cus(pkg):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 16 * cus + 3                                                    # the plain (non-resident) kernel
    torch.manual_seed(0)
    mod = pkg.FaFp(1, latent_dim=8, net_sizes=[64, 64, 32], aug_net_sizes=[64, 64])
    with torch.no_grad():                                               # gamma away from 0, as the fixtures
        mod.net[-1].weight.mul_(0.1)
        mod.net[-1].bias.copy_(torch.tensor([0.8, 0.55]))
    mod = mod.cuda()
    gen = torch.Generator().manual_seed(1)
    S = torch.rand(N, 1, generator=gen) * 0.4 + 0.5
    I = torch.rand(N, 1, generator=gen) * 0.05
    y0 = torch.cat([S[..., None], I[..., None], (1 - S - I)[..., None], torch.randn(N, 1, 5, generator=gen)], -1)
    t = torch.arange(3, dtype=torch.float32)
    _identity_checks(mod, y0.cuda(), t, t[1] - t[0], _decoder(1))


# ---- 2. against fp64, 3. bounds --------------------------------------------------------------------------

@pytest.mark.parametrize("case", SCN_CASES)
def test_scenario_solve_matches_the_restated_oracle(pkg, case):
    from ude_amd.forecast import dynamics_names, solve_decode_scenario
    g, ref64, ref32, table = reference(case)
    assert ref64["margin"] >= MARGIN_MIN and ref64["gamma_min"] >= GAMMA_MIN
    mod = module_from_golden(pkg, g, "cuda")
    t, step = step_of(g)
    y0 = torch.from_numpy(g["y0"]).cuda()
    R = g["meta"]["n_regions"]
    lin = _decoder(R)
    T, N, C = len(t), y0.shape[0], len(dynamics_names(mod))
    n = C * T * N * R
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    # the table inside a larger buffer, NaN in front and behind (an even number of floats in front: the
    # table is read in place, 8-byte aligned)
    wide = torch.full((table.numel() + 2 * GUARD,), float("nan"), device="cuda")
    wide[GUARD:GUARD + table.numel()] = table.reshape(-1).cuda()
    inplace = wide[GUARD:GUARD + table.numel()].view(table.shape)
    y_hat, dyn, names, rates = solve_decode_scenario(mod, y0, t, step, lin, inplace, dynamics=True,
                                                     out=buf[:n].view(C, T, N, R))
    y_tight, dyn_tight, _names, rates_tight = solve_decode_scenario(mod, y0, t, step, lin, table.cuda(), dynamics=True)
    y_nodyn, none, _names, _rates = solve_decode_scenario(mod, y0, t, step, lin, table.cuda())
    torch.cuda.synchronize()
    # 3. bounds: nothing behind the channels, everything in front written; the table's neighbours never read
    assert bool((buf[n:] == SENTINEL).all()) and dyn.data_ptr() == buf.data_ptr()
    assert not bool((dyn == SENTINEL).any()) and bool(torch.isfinite(dyn).all()) and bool(torch.isfinite(y_hat).all())
    assert torch.equal(y_hat, y_tight) and torch.equal(dyn, dyn_tight) and torch.equal(rates.mean, rates_tight.mean)
    assert none is None and torch.equal(y_nodyn, y_hat)                 # the channels do not touch the solve
    assert names == dynamics_names(mod)
    # 2. y_hat against Linear64(latent64[..., :3]), every channel against the restated oracle
    W, b = lin.weight.detach().double().cpu(), lin.bias.detach().double().cpu()
    dec = lambda lat: lat[..., :3].reshape(T, N, 3 * R) @ W.T + b
    want, want32 = dec(ref64["latent"]), dec(ref32["latent"].double())
    e, e_last = normwise_rel(y_hat, want), normwise_rel(y_hat[-1], want[-1])
    b_all, b_last = max(1e-5, 2 * normwise_rel(want32, want)), max(1e-5, 2 * normwise_rel(want32[-1], want[-1]))
    print(case, "y_hat", f"{e:.2e} (bar {b_all:.1e}); last time {e_last:.2e} (bar {b_last:.1e})")
    assert e <= b_all and e_last <= b_last, (e, e_last)
    for c, nm in enumerate(names):
        e, e_last = normwise_rel(dyn[c], ref64["dyn"][c]), normwise_rel(dyn[c, -1], ref64["dyn"][c, -1])
        b_all, b_last = bar(ref64, ref32, "dyn", c), bar(ref64, ref32, "dyn", c, last=True)
        print(case, nm, f"{e:.2e} (bar {b_all:.1e}); last time {e_last:.2e} (bar {b_last:.1e})")
        assert e <= b_all, (nm, e)
        assert e_last <= b_last, (nm, e_last)
    h = {nm: dyn[c].cpu() for c, nm in enumerate(names)}
    assert torch.equal(h["r_eff"], (h["beta"] * h["s"]) / h["gamma"])   # one fp32 division of the emitted channels
    # the returned statistics: the scaled rates' mean / std of the restated fp32 oracle
    assert normwise_rel(rates.mean, ref32["mean"]) <= 1e-5 and normwise_rel(rates.std, ref32["std"]) <= 1e-5


# ---- 4. several steps per interval, the snapped daily grid ------------------------------------------------

def _check_against_eager_route(mod, y0, t, step, lin, scenario, latent_step):
    """The kernel against ``scenario_latent`` on the device's eager route and ``latent_dynamics`` of it: 1e-5,
    normwise per channel (two fp32 orderings of the same layers), the last time index also alone."""
    from ude_amd.forecast import (_forecast_plan, _output_rows, latent_dynamics, scenario_latent,
                                  solve_decode_scenario)
    R = y0.shape[1]
    y_hat, dyn, names, _rates = solve_decode_scenario(mod, y0, t, step, lin, scenario, dynamics=True)
    table = scenario.table(_forecast_plan(mod, y0, t, step), R)
    latent = scenario_latent(mod, y0, t, latent_step, table)
    assert mod.rate_scale is None
    ref, rnames = latent_dynamics(mod, latent, rate_scale=_output_rows(scenario, len(t), R))
    assert rnames == names
    for c, nm in enumerate(names):
        e, e_last = normwise_rel(dyn[c], ref[c]), normwise_rel(dyn[c, -1], ref[c, -1])
        print(nm, f"{e:.2e} (last time {e_last:.2e})")
        assert e <= 1e-5 and e_last <= 1e-5, (nm, e, e_last)
    with torch.no_grad():
        want = lin(latent[..., :3].reshape(len(t), y0.shape[0], 3 * R))
    assert normwise_rel(y_hat, want) <= 1e-5


def _interval_scenario(T, R):
    from ude_amd.forecast import Scenario
    m = scn_table(T - 1, R)
    return Scenario(beta=m[..., 0].numpy(), gamma=m[..., 1].numpy())


def test_two_steps_per_output_interval(pkg):
    from ude_amd import solvers
    g = load_golden("e2e_dyn_fafp_r3_l5")
    mod = module_from_golden(pkg, g, "cuda")
    t, step = step_of(g)
    y0 = torch.from_numpy(g["y0"]).cuda()
    sc = _interval_scenario(len(t), 3)
    plan = solvers.plan_for(mod, y0, t, step / 2)
    assert plan.prob.n_steps == 2 * (len(t) - 1)
    tab = sc.table(plan, 3)
    assert torch.equal(tab[0::2], tab[1::2]) and not torch.equal(tab[0], tab[2])
    _check_against_eager_route(mod, y0, t, step / 2, _decoder(3), sc, step / 2)


def test_snapped_daily_grid(pkg):
    from ude_amd import solvers
    g = load_golden("e2e_dyn_fafp_r3_l5")
    mod = module_from_golden(pkg, g, "cuda")
    t = torch.arange(8, dtype=torch.float32) / 7
    y0 = torch.from_numpy(g["y0"]).cuda()
    assert solvers.plan_for(mod, y0, t, t[1] - t[0]).out_k is None      # not grid hits until the grid is snapped
    _check_against_eager_route(mod, y0, t, t[1] - t[0], _decoder(3), _interval_scenario(8, 3), None)


# ---- 5. no kernel path -----------------------------------------------------------------------------------

def test_models_without_a_scenario_kernel(pkg):
    from ude_amd import _native, decoder_head, solvers
    from ude_amd.forecast import Scenario, solve_decode_scenario
    t = torch.arange(3, dtype=torch.float32)
    g = load_golden("e2e_forecast_us_bayes")
    model = build_vae(g, "cuda")
    z = torch.rand(16, 1, 8, device="cuda")
    assert solve_decode_scenario(model.ode, z, t, t[1] - t[0], decoder_head.decoder_linear(model.dec), Scenario()) is None
    fa = pkg.Fa(1, latent_dim=8, aug_net_sizes=[64, 64]).cuda()
    assert solve_decode_scenario(fa, z, t, t[1] - t[0], _decoder(1), Scenario()) is None
    # the C-ABI entry: UDE_E_UNSUPPORTED for both, UDE_E_INVALID for a null table
    good = pkg.FaFp(1, latent_dim=8, net_sizes=[64, 64, 32], aug_net_sizes=[64, 64]).cuda()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")      # stands for every device argument
    st = _native.UdeSideStats(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None)
    for ode, table, want in ((fa, buf, _native.UDE_E_UNSUPPORTED), (model.ode, buf, _native.UDE_E_UNSUPPORTED),
                             (good, None, _native.UDE_E_INVALID)):
        plan = solvers.plan_for(ode, z, t, t[1] - t[0])
        p = buf.data_ptr()
        rc = plan.lib._rc("ude_rk4_forecast_scn", plan.desc, plan.prob, p, plan.sched_dev.data_ptr(), z.data_ptr(), p,
                          None if table is None else p, p, None, p, None, st, 0)
        assert rc == want, (type(ode).__name__, rc)
    torch.cuda.synchronize()


# ---- 6. end to end ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["e2e_forecast_us", "e2e_forecast_state49"])
def test_forecast_scenarios_end_to_end(pkg, monkeypatch, case):
    from ude_amd import fused
    from ude_amd.forecast import Scenario, Season
    g = load_golden(case)
    T, R = len(g["t"]), g["meta"]["n_regions"]
    season = Season(start=6, every=7)
    less = Scenario.from_day(T, 10, beta=[0.7] + [1.0] * (R - 1) if R > 1 else 0.7)
    scen = {"same": Scenario(), "less": less}
    events = []
    monkeypatch.setattr(fused, "EVENTS", events)
    model, fc = run_forecast(g, "cuda", monkeypatch, season=season, scenarios=scen)
    torch.cuda.synchronize()
    kinds = [e[0] for e in events]
    per = ["forecast_scn", "forecast_summary", "forecast_summary", "forecast_season", "forecast_season"]
    assert kinds == ["forecast_dec", "forecast_summary", "forecast_season"] + per + per, kinds
    assert model.latent is None and model.ode.rate_scale is None
    _, plain = run_forecast(g, "cuda", monkeypatch, season=season)
    _, again = run_forecast(g, "cuda", monkeypatch, season=season, scenarios=scen)
    assert plain.scenarios is None
    a, b, c = (v for v in (plain._tensors(), fc._tensors(), again._tensors()))
    assert len(b) == len(c) > len(a) > 6
    assert all(torch.equal(x[1], y[1]) for x, y in zip(a, b))           # the baseline: the call without scenarios
    assert all(x[0] == y[0] and torch.equal(x[1], y[1]) for x, y in zip(b, c))     # a second call: the same bits
    same, low = fc.scenarios["same"], fc.scenarios["less"]
    assert bool((same.effect.mean == 0).all()) and bool((same.effect.std == 0).all())
    assert bool((same.effect_season.total_mean == 0).all())
    assert torch.equal(same.forecast.mean, fc.mean) and torch.equal(same.forecast.quantiles, fc.quantiles)
    assert torch.equal(same.forecast.season.total_mean, fc.season.total_mean)
    assert same.forecast.nll is None and low.forecast.season.total_crps is None
    # days 0 .. 10 are the baseline's (ones before interval 10); region 0's transmission falls afterwards
    assert bool((low.effect.mean[:, :11] == 0).all()) and bool((low.effect.std[:, :11] == 0).all())
    assert float(low.effect.mean[:, 11:, 0].abs().max()) > 0
    assert float(low.rates.mean[0]) < float(same.rates.mean[0])
    host = fc.cpu()
    assert not host.scenarios["less"].effect.mean.is_cuda
    assert torch.equal(host.scenarios["less"].effect.mean, low.effect.mean.cpu())
    assert torch.equal(host.scenarios["less"].rates.std, low.rates.std.cpu())
