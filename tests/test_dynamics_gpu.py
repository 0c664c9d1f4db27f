"""The forecast's dynamics on the MI355X: the inference decoder-epilogue solve that also emits S, I, R,
beta, gamma, R_eff and Fa at every output time (ude_rk4_forecast_dyn) against the solve without them
(bit for bit), the plain inference odeint (the state channels, bit for bit), the reference modules' own
appends in fp64 (tests/golden/e2e_dyn_*.npz), a guard band behind the output, and
``VAE.forecast(dynamics=True)`` end to end."""
import pytest
import torch

from conftest import load_golden
from helpers import module_from_golden, normwise_rel, step_of
from forecast_helpers import build_vae, run_forecast
from test_dynamics import ALL, DYN_CASES, GAMMA_MIN, bar

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 4096


def _decoder(R):
    torch.manual_seed(R)
    return torch.nn.Linear(3 * R, R).cuda()


def _stats(ode):
    n_eval, stats, sums = ode._fused_sums[-1]
    return [n_eval] + [s.detach().clone() for s in stats] + [sums.clone()]


def _solve_both(pkg, ode, y0, t, step, lin, latent_step="same"):
    """The solve without and with the dynamics, the latter into a buffer with a guard band behind it:
    (y_hat, stats) of ude_rk4_forecast_dec, (y_hat, stats, dyn, names) of ude_rk4_forecast_dyn, and the
    plain inference odeint's latent (``latent_step``: that solve's step size when it is not ``step`` --
    the snapped daily grid steps on ``t`` itself, torchdiffeq's grid without a step size).  Checks 1, 2
    and 4 of every case are asserted here."""
    from ude_amd.forecast import dynamics_names, solve_decode_dynamics, solve_decode_forecast
    ode.clear_tracking()
    y_dec = solve_decode_forecast(ode, y0, t, step, lin)
    assert y_dec is not None
    st_dec = _stats(ode)
    T, (N, R, _L), C = len(t), y0.shape, len(dynamics_names(ode))
    n = C * T * N * R
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    ode.clear_tracking()
    res = solve_decode_dynamics(ode, y0, t, step, lin, out=buf[:n].view(C, T, N, R))
    assert res is not None
    y_dyn, dyn, names = res
    st_dyn = _stats(ode)
    torch.cuda.synchronize()
    # 1. the solve is untouched
    assert torch.equal(y_dyn, y_dec)
    assert st_dyn[0] == st_dec[0] == 4.0 * (T - 1) * N * R           # n_eval: the extra evaluation is not counted
    for a, b in zip(st_dyn[1:], st_dec[1:]):
        assert torch.equal(a, b)
    # 4. rows n >= n_traj do not exist: nothing behind the last channel, everything in front written
    assert bool((buf[n:] == SENTINEL).all())
    assert names == dynamics_names(ode) and dyn.data_ptr() == buf.data_ptr()
    assert not bool((dyn == SENTINEL).any()) and bool(torch.isfinite(dyn).all())
    # 2. the state channels are the plain inference solve's latent
    ode.clear_tracking()
    with torch.no_grad():
        latent = pkg.odeint(ode, y0, t, method="rk4",
                            options=dict(step_size=step if latent_step == "same" else latent_step))
    assert torch.equal(dyn[:3], latent[..., :3].permute(3, 0, 1, 2))
    ode.clear_tracking()
    return dyn, names, latent


def _check_r_eff_is_one_division(dyn, names):
    """r_eff = (beta * s) / gamma in fp32, IEEE (formed on the host from the emitted channels)."""
    if "r_eff" in names:
        h = {nm: dyn[c].cpu() for c, nm in enumerate(names)}
        assert torch.equal(h["r_eff"], (h["beta"] * h["s"]) / h["gamma"])


def _check_against_evaluation_kernel(ode, dyn, names, latent):
    """Cases without a fixture: every net channel against one evaluation of the RHS kernel per output
    state (ude_amd.forecast.latent_dynamics on the device), normwise per channel within 1e-5 (the
    suite's floor for two fp32 orderings of the same layers), the last time index also on its own."""
    from ude_amd.forecast import latent_dynamics
    ref, rnames = latent_dynamics(ode, latent)
    assert rnames == names
    for c, nm in enumerate(names):
        e, e_last = normwise_rel(dyn[c], ref[c]), normwise_rel(dyn[c, -1], ref[c, -1])
        print(nm, f"{e:.2e} (last time {e_last:.2e})")
        assert e <= 1e-5 and e_last <= 1e-5, (nm, e, e_last)


@pytest.mark.parametrize("case", DYN_CASES)
def test_dyn_solve_matches_reference(pkg, case):
    g = load_golden(case)
    mod = module_from_golden(pkg, g, "cuda")
    t, step = step_of(g)
    y0 = torch.from_numpy(g["y0"]).cuda()
    assert y0.shape[0] == 20                                            # one full tile and a ragged one
    dyn, names, _ = _solve_both(pkg, mod, y0, t, step, _decoder(g["meta"]["n_regions"]))
    assert names == tuple(g["meta"]["channels"])
    ref = g["ref64_dyn"]
    if "gamma" in names:
        assert ref[names.index("gamma")].min() >= GAMMA_MIN
    # 3. every channel against the fixture's fp64, and the last time index (the extra evaluation) alone
    for c, nm in enumerate(names):
        e, e_last = normwise_rel(dyn[c], ref[c]), normwise_rel(dyn[c, -1], ref[c, -1])
        print(case, nm, f"{e:.2e} (bar {bar(g, nm):.1e}); last time {e_last:.2e} (bar {bar(g, nm, last=True):.1e})")
        assert e <= bar(g, nm), (nm, e)
        assert e_last <= bar(g, nm, last=True), (nm, e_last)
    _check_r_eff_is_one_division(dyn, names)


def test_dyn_solve_one_step(pkg):
    g = load_golden("e2e_dyn_fafp_r1")
    mod = module_from_golden(pkg, g, "cuda")
    t = torch.arange(2, dtype=torch.float32)                            # output 0 and the extra evaluation only
    dyn, names, latent = _solve_both(pkg, mod, torch.from_numpy(g["y0"]).cuda(), t, t[1] - t[0], _decoder(1))
    ref = g["ref64_dyn"][:, :2]
    for c, nm in enumerate(names):
        assert normwise_rel(dyn[c], ref[c]) <= bar(g, nm), nm           # the fixture's first step is this solve
    _check_against_evaluation_kernel(mod, dyn, names, latent)


def test_dyn_solve_snapped_daily_grid(pkg):
    from ude_amd import solvers
    g = load_golden("e2e_dyn_fafp_r3_l5")
    mod = module_from_golden(pkg, g, "cuda")
    t = torch.arange(8, dtype=torch.float32) / 7
    y0 = torch.from_numpy(g["y0"]).cuda()
    assert solvers.plan_for(mod, y0, t, t[1] - t[0]).out_k is None      # not grid hits until the grid is snapped
    dyn, names, latent = _solve_both(pkg, mod, y0, t, t[1] - t[0], _decoder(3), latent_step=None)
    _check_against_evaluation_kernel(mod, dyn, names, latent)


def test_dyn_solve_more_tiles_than_cus(pkg):
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
    dyn, names, latent = _solve_both(pkg, mod, y0.cuda(), t, t[1] - t[0], _decoder(1))
    assert float(dyn[names.index("gamma")].min()) >= GAMMA_MIN
    _check_r_eff_is_one_division(dyn, names)
    _check_against_evaluation_kernel(mod, dyn, names, latent)


def test_bayes_has_no_kernel_path(pkg):
    from ude_amd import decoder_head
    from ude_amd.forecast import solve_decode_dynamics
    g = load_golden("e2e_forecast_us_bayes")
    model = build_vae(g, "cuda")
    z = torch.rand(16, 1, 8, device="cuda")
    t = torch.arange(3, dtype=torch.float32)
    assert solve_decode_dynamics(model.ode, z, t, t[1] - t[0], decoder_head.decoder_linear(model.dec)) is None


# ---- end to end ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["e2e_forecast_us", "e2e_forecast_state49"])
def test_forecast_dynamics_end_to_end(pkg, monkeypatch, case):
    import lib.models as models
    from ude_amd import decoder_head, fused
    from ude_amd.forecast import ensemble_summary, solve_decode_dynamics
    g = load_golden(case)
    m = g["meta"]
    S, B, R, Q, T = m["n_samples"], m["B"], m["n_regions"], m["quantiles"], len(g["t"])
    events = []
    monkeypatch.setattr(fused, "EVENTS", events)
    model, fc = run_forecast(g, "cuda", monkeypatch, dynamics=True)
    torch.cuda.synchronize()
    kinds = [e[0] for e in events]
    assert kinds == ["forecast_dyn", "forecast_summary", "forecast_summary"], kinds   # one solve, one summary each
    assert model.latent is None
    d = fc.dynamics
    assert d.names == ALL and d.mean.is_cuda
    assert tuple(d.mean.shape) == (9, B, T, R) and tuple(d.quantiles.shape) == (len(Q), 9, B, T, R)
    # the same solve by hand, summarised by one call on the stacked channels
    eps = torch.from_numpy(g["eps"]).cuda()
    with torch.no_grad():
        mean, std = model.enc(torch.from_numpy(g["x"]).cuda())
        z = models.reparam(eps, std, mean, S, B, uncertainty=True) + 1e-5
    t = torch.from_numpy(g["t"])
    yhat, dyn, names = solve_decode_dynamics(model.ode, z, t, t[1] - t[0], decoder_head.decoder_linear(model.dec))
    ref = ensemble_summary(dyn.view(9 * T, S * B, R), S, B, quantiles=Q)
    assert torch.equal(d.mean, ref.mean.view(B, 9, T, R).permute(1, 0, 2, 3))
    assert torch.equal(d.std, ref.std.view(B, 9, T, R).permute(1, 0, 2, 3))
    assert torch.equal(d.quantiles, ref.quantiles.view(len(Q), B, 9, T, R).permute(0, 2, 1, 3, 4))
    # the prediction side is the forecast without dynamics, and a second call gives the same bits
    _, plain = run_forecast(g, "cuda", monkeypatch)
    _, again = run_forecast(g, "cuda", monkeypatch, dynamics=True)
    assert plain.dynamics is None
    for k in ("mean", "std", "quantiles", "nll", "skill", "mae"):
        assert torch.equal(getattr(fc, k), getattr(plain, k)), k
        assert torch.equal(getattr(fc, k), getattr(again, k)), k
    for k in ("mean", "std", "quantiles"):
        assert torch.equal(getattr(d, k), getattr(again.dynamics, k)), k
    host = fc.cpu()
    assert not host.dynamics.mean.is_cuda and torch.equal(host.dynamics.mean, d.mean.cpu())
    assert torch.equal(host.mean, fc.mean.cpu())
