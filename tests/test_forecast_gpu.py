"""The fused forecast on the MI355X: the ensemble summary kernels (csrc/ude_forecast.h) against NumPy /
SciPy in fp64, the inference solve with the decoder epilogue (ude_rk4_forecast_dec) bit for bit
against the training decoder forward, VAE.forecast against the reference's own forecast
(tests/golden/e2e_forecast_*.npz) and the callers (lib.utils.test, evaluate) against the host scoring
of ``__call__(training=False)``."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import module_from_golden, normwise_rel, step_of
from forecast_helpers import (FORECAST_CASES, build_vae, check_against_fixture, numpy_summary, run_forecast,
                              synth)

pytestmark = pytest.mark.gpu

LEVELS = [0.0, 0.025, 0.5, 0.9, 1.0]
MASS_FLOOR = 4.5399929762484854e-05


def _summary(yhat, S, B, scale, y, q):
    from ude_amd.forecast import ensemble_summary
    return ensemble_summary(torch.from_numpy(yhat).cuda(), S, B, y_true=None if y is None else torch.from_numpy(y).cuda(),
                            scale=scale, quantiles=q)


@pytest.mark.parametrize("shape,targets,ties,q,scaled", [
    ((3, 5, 4, 1), True, False, LEVELS, True),          # odd S, 12 groups: fewer than a wave
    ((2, 128, 3, 49), True, False, LEVELS, True),       # B * R = 147: no multiple of any tile width
    ((2, 64, 7, 10), True, True, LEVELS, True),         # repeated values inside every group
    ((1, 1024, 2, 3), True, False, LEVELS, True),       # the largest S with quantiles
    ((2, 1, 5, 2), False, False, LEVELS, True),         # S = 1: std 0
    ((1, 4100, 1, 3), True, False, None, True),         # S above the tile: rows == 0, y_hat read twice
    ((1, 3000, 2, 3), True, False, None, True),         # a tile of 3000 rows (no power of two), G = 1
    ((2, 2, 90, 49), True, False, LEVELS, True),        # nbx = 69 > 64: the scores kernel's strided loop
    ((2, 9, 3, 10), True, False, LEVELS, False),        # no scale vector
], ids=["shape0-True-False", "shape1-True-False", "shape2-True-True", "shape3-True-False", "shape4-False-False",
        "untiled_S4100", "tile_3000_rows_G1", "nbx69", "no_scale"])
def test_summary_kernel_matches_numpy(pkg, shape, targets, ties, q, scaled):
    T, S, B, R = shape
    yhat, scale, y = synth(T, S, B, R, seed=100 + S, targets=targets, ties=ties)
    if not scaled:
        scale = None
    ref = numpy_summary(yhat, S, B, scale, y, q)
    if targets:
        assert np.exp(ref["mb_log"]).min() >= 1e-6        # the group masses are larger still
    fc = _summary(yhat, S, B, scale, y, q)
    torch.cuda.synchronize()
    assert (fc.quantiles is None) == (q is None)
    keys = ("mean", "std") + (("quantiles",) if q is not None else ()) + (("nll", "mae") if targets else ())
    errs = {k: normwise_rel(getattr(fc, k), ref[k]) for k in keys}
    if targets:
        errs["mb_log"] = normwise_rel(fc.skill.log(), ref["mb_log"])
    print(shape, {k: f"{v:.2e}" for k, v in errs.items()})
    if S == 1:
        assert float(fc.std.abs().max()) == 0.0
        errs.pop("std")
    for k, e in errs.items():
        assert e <= (1e-8 if k == "mb_log" else 1e-10), (k, e)
    again = _summary(yhat, S, B, scale, y, q)
    for k in ("mean", "std", "quantiles", "nll", "skill", "mae"):
        a, b = getattr(fc, k), getattr(again, k)
        assert (a is None and b is None) or torch.equal(a, b), k


def test_summary_mass_floor(pkg):
    T, S, B, R = 2, 16, 3, 2
    yhat, scale, y = synth(T, S, B, R, seed=7, far=60.0)
    fc = _summary(yhat, S, B, scale, y, None)
    assert torch.allclose(fc.skill.log().cpu(), torch.full((T,), math.log(MASS_FLOOR), dtype=torch.float64),
                          rtol=0.0, atol=1e-12)
    assert bool(torch.isfinite(fc.nll).all())
    ref = numpy_summary(yhat, S, B, scale, y, None)
    assert normwise_rel(fc.nll, ref["nll"]) <= 1e-10


# ---- inference solve == training decoder forward, bit for bit ------------------------------------

def _both_solves(ode, y0, t, step, lin, ode_eps=None):
    """(training y_hat, training stats, forecast y_hat, forecast stats, plan, peaks)."""
    from ude_amd import decoder_head, solvers
    from ude_amd.forecast import solve_decode_forecast
    plan = solvers.plan_for(ode, y0, t, step)
    out = []
    peaks = []
    for train in (True, False):
        ode.clear_tracking()
        if ode_eps is not None:
            ode.set_eps_stream(ode_eps)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        if train:
            yhat = decoder_head.solve_decode(ode, y0, t, step, lin)[0].detach()
        else:
            yhat = solve_decode_forecast(ode, y0, t, step, lin)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        n_eval, stats, sums = ode._fused_sums[-1]
        out += [yhat.clone(), [s.detach().clone() for s in stats] + [sums.clone()]]
        del yhat
    return out[0], out[1], out[2], out[3], plan, peaks


def _assert_same(res):
    y_tr, st_tr, y_fc, st_fc, plan, peaks = res
    assert y_fc is not None and y_fc.dtype == torch.float32 and y_fc.shape == y_tr.shape
    assert torch.equal(y_fc, y_tr)
    for a, b in zip(st_fc, st_tr):
        assert torch.equal(a, b)


def _vae_inputs(name):
    g = load_golden(name)
    import lib.models as models
    from ude_amd import decoder_head
    model = build_vae(g, "cuda")
    m = g["meta"]
    S, B = m["n_samples"], m["B"]
    eps = torch.from_numpy(g["eps"]).cuda()
    with torch.no_grad():
        mean, std = model.enc(torch.from_numpy(g["x"]).cuda())
        z = (models.reparam(eps, std, mean, S, B, uncertainty=True) + 1e-5).contiguous()
    t = torch.from_numpy(g["t"])[g["eval_pts"]]
    ode_eps = torch.from_numpy(g["ode_eps"]).cuda() if "ode_eps" in g else None
    return model.ode, z, t, t[1] - t[0], decoder_head.decoder_linear(model.dec), ode_eps


def _decoder(R):
    torch.manual_seed(R)
    return torch.nn.Linear(3 * R, R).cuda()


def test_forecast_solve_bitwise_toy64(pkg):
    ode, z, t, step, lin, _ = _vae_inputs("e2e_vae_toy64")
    assert z.shape[0] == 20                                   # a ragged tile
    _assert_same(_both_solves(ode, z, t, step, lin))


def test_forecast_dec_without_ctl_is_the_same_solve(pkg):
    """ude_rk4_forecast_dec with ``ctl = NULL`` (the spare control word behind stats_slab, zeroed by the
    call) against the plan's caller-zeroed ``ctl``: the same bits, the NULL call repeated on the same
    buffers included, and the plan's words left zero."""
    from ude_amd import fused
    from ude_amd.forecast import _forecast_plan
    from test_legacy_cabi import dirty_words
    ode, z, t, step, lin, _ = _vae_inputs("e2e_vae_toy64")
    plan = _forecast_plan(ode, z, t, step)
    dev, sz = z.device, plan.sizes
    pack = fused.packed_weights(plan, [p for l in ode.ude_linears() for p in (l.weight, l.bias)], dev)
    dec_pack = torch.empty(sz.dec_pack_bytes // 4, dtype=torch.float32, device=dev)
    plan.lib.pack_decoder(plan.desc, lin.weight.data_ptr(), lin.bias.data_ptr(), dec_pack.data_ptr(), fused._stream(dev))
    ctl = fused._ctl(plan, dev)
    res = []
    stats_slab = torch.empty(sz.stats_slab_bytes // 8, dtype=torch.float64, device=dev)
    dirty_words(stats_slab, sz.ctl_bytes)                          # the spare words start out non-zero
    for c in (ctl.data_ptr(), None, None):
        yhat = torch.empty((plan.n_times, z.shape[0], z.shape[1]), dtype=torch.float32, device=dev)
        stats, sums, st = fused._stats_out(plan, dev)
        plan.lib.forecast_dec(plan.desc, plan.prob, pack.data_ptr(), plan.sched_dev.data_ptr(), z.data_ptr(),
                              dec_pack.data_ptr(), yhat.data_ptr(), stats_slab.data_ptr(), c, st, fused._stream(dev))
        res.append([yhat, *stats, sums])
    torch.cuda.synchronize()
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)
    assert int(ctl.abs().max()) == 0


def test_forecast_solve_bitwise_r10(pkg):
    g = load_golden("fafp_r10_weekly")
    mod = module_from_golden(pkg, g, "cuda")
    t, step = step_of(g)
    _assert_same(_both_solves(mod, torch.from_numpy(g["y0"]).cuda(), t, step, _decoder(10)))


def test_forecast_solve_bitwise_state49_and_no_checkpoint(pkg):
    ode, z, t, step, lin, _ = _vae_inputs("e2e_vae_state49")
    assert tuple(z.shape) == (128, 49, 8)                     # the training side runs the SPLIT launch
    res = _both_solves(ode, z, t, step, lin)
    _assert_same(res)
    plan, (peak_train, peak_fc) = res[4], res[5]
    ckpt = int(plan.sizes.ckpt_bytes)
    print(f"checkpoint {ckpt} B; peak above the inputs: training {peak_train} B, forecast {peak_fc} B")
    assert peak_train >= ckpt                                 # the training call allocates the store
    assert peak_fc < ckpt                                     # the forecast allocates nothing of that size


def test_forecast_solve_bitwise_us_bayes(pkg):
    ode, z, t, step, lin, ode_eps = _vae_inputs("e2e_vae_us_bayes")
    assert ode_eps is not None
    _assert_same(_both_solves(ode, z, t, step, lin, ode_eps))


def test_forecast_solve_bitwise_more_tiles_than_cus(pkg):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 16 * cus + 3                                          # the plain (non-resident) kernel
    torch.manual_seed(0)
    mod = pkg.FaFp(1, latent_dim=8, net_sizes=[64, 64, 32], aug_net_sizes=[64, 64]).cuda()
    gen = torch.Generator().manual_seed(1)
    S = torch.rand(N, 1, generator=gen) * 0.4 + 0.5
    I = torch.rand(N, 1, generator=gen) * 0.05
    y0 = torch.cat([S[..., None], I[..., None], (1 - S - I)[..., None], torch.randn(N, 1, 5, generator=gen)], -1)
    t = torch.arange(4, dtype=torch.float32)
    _assert_same(_both_solves(mod, y0.cuda(), t, t[1] - t[0], _decoder(1)))


# ---- end to end ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", FORECAST_CASES)
def test_forecast_fused_matches_reference(pkg, monkeypatch, case):
    g = load_golden(case)
    from ude_amd import fused
    events = []
    monkeypatch.setattr(fused, "EVENTS", events)
    model, fc = run_forecast(g, "cuda", monkeypatch)
    torch.cuda.synchronize()
    kinds = [e[0] for e in events]
    assert kinds == ["forecast_dec", "forecast_summary"], kinds       # the native path ran, nothing else
    assert fc.mean.is_cuda
    check_against_fixture(g, fc.cpu())
    assert model.latent is None
    post = model.ode.posterior()
    assert bool(torch.isfinite(post.loc).all()) and bool((post.scale > 0).all())


# ---- callers -----------------------------------------------------------------------------------------

def test_callers_score_like_the_host_path(pkg, tmp_path):
    """lib.utils.test and evaluate on the device against the host scoring (lib/utils.py:22-26, :53-54
    with lib/Metrics.py) of ``__call__(training=False)`` under the same seed, at run_ode.py's 57 daily
    outputs; targets 0.7 predictive standard deviations around the host path's mean (z = O(1))."""
    import pandas as pd
    import lib.Metrics as Metrics
    import lib.VAE as vae_mod
    import lib.utils as utils
    g = load_golden("e2e_forecast_state49")
    model = build_vae(g, "cuda")
    S, seed, s = 16, 3, g["scaler"]
    x, t = torch.from_numpy(g["x"]).cuda(), torch.arange(57, dtype=torch.float32) / 7
    torch.manual_seed(seed)
    y_pr = model(x, t, n_samples=S, training=False).detach().cpu().numpy() * s[None, None, None, :]
    mu, sd = y_pr.mean(1), y_pr.std(1)
    y_test = ((mu + 0.7 * sd * np.random.default_rng(0).standard_normal(mu.shape)) / s).astype(np.float32)
    y_te = y_test * s[None, None, :]
    nll = np.array([Metrics.nll(y_te[:, k, :], mu[:, k, :], sd[:, k, :]) for k in range(57)])
    skill = np.array([Metrics.skill(y_te[:, k, :], mu[:, k, :], sd[:, k, :]) for k in range(57)])
    y = torch.from_numpy(y_test).cuda()

    name = str(tmp_path / "results_table")
    pd.DataFrame({"ode_name": pd.Series(dtype=object)}).to_csv(name + ".csv")
    torch.manual_seed(seed)
    utils.test(model, s, x, y, t, "2016", window_size=8, variables={"ode_name": "SONN"}, n_samples=S, file_name=name)
    df = pd.read_csv(name + ".csv", index_col=0)
    assert list(df.columns) == ["ode_name", "2016 14", "skill 2016 7", "2016 21", "skill 2016 14", "2016 28",
                                "skill 2016 21", "2016 35", "skill 2016 28"]
    for col, k in zip([7, 14, 21, 28], [14, 21, 28, 35]):
        print(k, df.loc[0, f"2016 {k}"], nll[k], df.loc[0, f"skill 2016 {col}"], skill[k])
        assert abs(df.loc[0, f"2016 {k}"] - nll[k]) <= 2e-5 * abs(nll[k])
        assert abs(df.loc[0, f"skill 2016 {col}"] - skill[k]) <= 2e-5 * abs(skill[k])
    assert model.latent is None                                       # the fused forecast ran

    torch.manual_seed(seed)
    got = vae_mod.evaluate(model, x, y, t, s, n_samples=S)
    want = {"forecast_nll": np.mean(nll[-28:]), "all_nll": np.mean(nll)}
    print(got, want)
    assert list(got) == list(want)
    for k in want:
        assert abs(got[k] - want[k]) <= 2e-5 * abs(want[k])
