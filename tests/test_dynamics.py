"""The forecast's dynamics (S, I, R, beta, gamma, R_eff, Fa per day) on the host: the latent fallback
(ude_amd.forecast.latent_dynamics) against the reference modules' own appends
(tests/golden/e2e_dyn_*.npz, make_golden_dynamics.py), and ``VAE.forecast(dynamics=True)``:
``Forecast.dynamics`` is one ensemble summary of the stacked channels, leaves the RHS's tracking as
``dynamics=False`` leaves it, and ``dynamics=False`` is the forecast as it was."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import module_from_golden, normwise_rel, step_of
from forecast_helpers import build_vae, run_forecast

DYN_CASES = ["e2e_dyn_fafp_r1", "e2e_dyn_fafp_r3_l5", "e2e_dyn_fp_r10", "e2e_dyn_fa_r1", "e2e_dyn_fafp_r49"]
ALL = ("s", "i", "r", "beta", "gamma", "r_eff", "fa_s", "fa_i", "fa_r")
GAMMA_MIN = 0.1
TENSOR_FIELDS = ("mean", "std", "quantiles", "nll", "skill", "mae")


def bar(g, name, last=False):
    """max(1e-5, 2 x the fixture's own fp32-vs-fp64 distance of this channel), normwise."""
    return max(1e-5, 2.0 * g["meta"]["ref32_vs_ref64_last" if last else "ref32_vs_ref64"][name])


@pytest.mark.parametrize("case", DYN_CASES)
def test_fixture_conditions(case):
    g = load_golden(case)
    names = g["meta"]["channels"]
    assert tuple(names) == tuple(n for n in ALL if n in names)
    assert g["ref64_dyn"].shape == (len(names), 4, 20, g["meta"]["n_regions"]) == g["ref32_dyn"].shape
    if "gamma" in names:
        assert g["ref64_dyn"][names.index("gamma")].min() >= GAMMA_MIN
        assert g["ref32_dyn"][names.index("gamma")].min() >= GAMMA_MIN


@pytest.mark.parametrize("case", DYN_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_latent_fallback_matches_reference(pkg, case, dtype):
    """fp32: the fixture's fp32 arrays within the distance the fixture's own fp32 has from its fp64;
    fp64 (the fallback works in the latent's dtype): the fp64 arrays to 1e-10 (fp64 roundings, 2.2e-16
    each, of two orderings of the same few thousand operations)."""
    from ude_amd.forecast import dynamics_names, latent_dynamics
    g = load_golden(case)
    mod = module_from_golden(pkg, g, "cpu").to(dtype)
    t, step = step_of(g)
    with torch.no_grad():
        latent = pkg.odeint(mod, torch.from_numpy(g["y0"]).to(dtype), t.to(dtype), method="rk4",
                            options=dict(step_size=step.to(dtype)))
    n_p, n_t = len(mod.params), len(mod.tracker)
    rng = torch.get_rng_state()
    dyn, names = latent_dynamics(mod, latent)
    assert (len(mod.params), len(mod.tracker)) == (n_p, n_t)          # no append
    assert torch.equal(torch.get_rng_state(), rng)
    assert names == tuple(g["meta"]["channels"]) == dynamics_names(mod)
    assert dyn.dtype == dtype and tuple(dyn.shape) == g["ref64_dyn"].shape
    assert torch.equal(dyn[:3], latent[..., :3].permute(3, 0, 1, 2))
    ref = g["ref32_dyn"] if dtype == torch.float32 else g["ref64_dyn"]
    for c, n in enumerate(names):
        e, e_last = normwise_rel(dyn[c], ref[c]), normwise_rel(dyn[c, -1], ref[c, -1])
        print(case, n, f"{e:.2e} (last time {e_last:.2e})")
        if dtype == torch.float32:
            assert e <= bar(g, n) and e_last <= bar(g, n, last=True), (n, e, e_last)
        else:
            assert e <= 1e-10 and e_last <= 1e-10, (n, e, e_last)
    if "r_eff" in names:
        i = {n: c for c, n in enumerate(names)}
        assert torch.equal(dyn[i["r_eff"]], dyn[i["beta"]] * dyn[i["s"]] / dyn[i["gamma"]])


# ---- VAE.forecast(dynamics=...) on the host ----------------------------------------------------------

def _tracking(ode):
    """What the forecast leaves on the RHS: (params, tracker, posterior loc / scale)."""
    params = [p.clone() for p in ode.params]
    tracker = [torch.as_tensor(v).clone() for v in ode.tracker]
    post = ode.posterior()
    return params, tracker, post.loc.clone(), post.scale.clone()


@pytest.fixture(scope="module")
def us_runs(pkg):
    """The US forecast fixture on the host with and without dynamics, on the same draw."""
    g = load_golden("e2e_forecast_us")
    out = {}
    for flag in (False, True):
        mp = pytest.MonkeyPatch()
        model, fc = run_forecast(g, "cpu", mp, dynamics=flag)
        latent = model.latent.detach().clone()
        out[flag] = (model, fc, latent, _tracking(model.ode))
    return g, out


def test_forecast_dynamics_is_one_summary_of_the_stacked_channels(pkg, us_runs):
    from ude_amd.forecast import Dynamics, ensemble_summary, latent_dynamics
    g, runs = us_runs
    model, fc, latent, _ = runs[True]
    m = g["meta"]
    S, B, T, R, Q = m["n_samples"], m["B"], len(g["t"]), m["n_regions"], len(m["quantiles"])
    d = fc.dynamics
    assert isinstance(d, Dynamics) and d.names == ALL
    assert tuple(d.mean.shape) == tuple(d.std.shape) == (9, B, T, R) and tuple(d.quantiles.shape) == (Q, 9, B, T, R)
    assert d.mean.dtype == torch.float64
    dyn, names = latent_dynamics(model.ode, latent)
    ref = ensemble_summary(dyn.reshape(9 * T, S * B, R), S, B, quantiles=m["quantiles"])
    assert torch.equal(d.mean, ref.mean.view(B, 9, T, R).permute(1, 0, 2, 3))
    assert torch.equal(d.std, ref.std.view(B, 9, T, R).permute(1, 0, 2, 3))
    assert torch.equal(d.quantiles, ref.quantiles.view(Q, B, 9, T, R).permute(0, 2, 1, 3, 4))
    mean, std, quant = d["r_eff"]
    assert torch.equal(mean, d.mean[5]) and torch.equal(std, d.std[5]) and torch.equal(quant, d.quantiles[:, 5])
    # the definition, against NumPy on the latent: r_eff per trajectory, then the ensemble mean
    lat = latent.double().numpy().reshape(T, S, B, R, -1)
    assert normwise_rel(d["s"][0], lat[..., 0].mean(1).transpose(1, 0, 2)) <= 1e-12
    with pytest.raises(ValueError):
        d["no_such_channel"]


def test_tracking_is_untouched_by_dynamics(us_runs):
    _, runs = us_runs
    (p0, t0, loc0, scale0), (p1, t1, loc1, scale1) = runs[False][3], runs[True][3]
    assert len(p0) == len(p1) > 0 and len(t0) == len(t1) > 0
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    assert all(torch.equal(a, b) for a, b in zip(t0, t1))
    assert torch.equal(loc0, loc1) and torch.equal(scale0, scale1)


def test_dynamics_false_is_the_forecast_as_it_was(us_runs):
    _, runs = us_runs
    fc0, fc1 = runs[False][1], runs[True][1]
    assert fc0.dynamics is None and fc1.dynamics is not None
    for k in TENSOR_FIELDS:
        assert torch.equal(getattr(fc0, k), getattr(fc1, k)), k
    assert torch.equal(runs[False][2], runs[True][2])                  # the same latent: the same draw
    # cpu / numpy / _map with and without the field
    assert fc0.cpu() is fc0 and fc0.numpy()["dynamics"] is None
    assert fc0._map(lambda v: v.float()).dynamics is None
    n1 = fc1.numpy()
    assert n1["dynamics"]["names"] == ALL and n1["dynamics"]["mean"].shape == tuple(fc1.dynamics.mean.shape)
    assert isinstance(n1["mean"], np.ndarray)
    half = fc1._map(lambda v: v.float())
    assert half.dynamics.mean.dtype == torch.float32 and half.dynamics.names == ALL and half.mean.dtype == torch.float32


def _small_vae(ode_cls, R=2, **ode_params):
    import lib.VAE as vae_mod
    import lib.models as models
    torch.manual_seed(5)
    return vae_mod.VAE(models.Encoder_Back_GRU, ode_cls, models.Decoder, 4, 8, R, ode_params=ode_params,
                       enc_params={"q_sizes": [16, 8], "ff_sizes": [8, 8], "SIR_scaler": [0.1, 0.05, 1.0]},
                       uncertainty=True, ode_kl_w=1 / 153)


@pytest.mark.parametrize("kind,present,absent", [("Fa", "fa_s", "beta"), ("Fp", "beta", "fa_s")])
def test_channels_follow_the_model_kind(pkg, kind, present, absent):
    import lib.models as models
    R, B, S, T = 2, 3, 4, 5
    model = _small_vae(getattr(models, kind), R, net_sizes=[16, 16], aug_net_sizes=[16, 16])
    torch.manual_seed(1)
    x = torch.rand(B, 8, R * 5)
    fc = model.forecast(x, torch.arange(T, dtype=torch.float32) / 7, n_samples=S, dynamics=True)
    d = fc.dynamics
    assert len(d.names) == 6 and d.names[:3] == ("s", "i", "r") and present in d.names and absent not in d.names
    assert tuple(d.mean.shape) == (6, B, T, R) and d.quantiles is None
    assert d[present][2] is None and bool(torch.isfinite(d.mean).all())
    with pytest.raises(ValueError):
        d[absent]


def test_bayes_goes_through_the_fallback_at_mean_weights(pkg, monkeypatch):
    from ude_amd.forecast import latent_dynamics, solve_decode_dynamics
    from ude_amd import decoder_head
    g = load_golden("e2e_forecast_us_bayes")
    model, fc = run_forecast(g, "cpu", monkeypatch, dynamics=True)
    ode, latent = model.ode, model.latent
    assert ode.uncertainty == "bayes" and fc.dynamics.names == ALL
    assert bool(torch.isfinite(fc.dynamics.mean).all()) and bool(torch.isfinite(fc.dynamics.std).all())
    assert solve_decode_dynamics(ode, latent[0], torch.from_numpy(g["t"]), None, decoder_head.decoder_linear(model.dec)) is None
    rng = torch.get_rng_state()
    dyn, names = latent_dynamics(ode, latent)
    assert torch.equal(torch.get_rng_state(), rng)                     # no weight draw
    T, N, R, L = latent.shape

    def mean_net(stack):
        h = latent.reshape(T * N, R * L)
        lays = [m for m in stack if hasattr(m, "w_mean")]
        for k, lay in enumerate(lays):
            h = torch.nn.functional.linear(h, lay.w_mean, lay.b_mean)
            if k < len(lays) - 2:
                h = torch.nn.functional.elu(h)
        return h
    with torch.no_grad():
        rates = mean_net(ode.Fp_net).abs().reshape(T, N, R, 2)
        fa = mean_net(ode.aug_net).reshape(T, N, R, 3)
    assert torch.equal(dyn[3], rates[..., 0]) and torch.equal(dyn[4], rates[..., 1])
    assert torch.equal(dyn[6:], fa.permute(3, 0, 1, 2))
    assert torch.equal(dyn[5], rates[..., 0] * latent[..., 0] / rates[..., 1])
