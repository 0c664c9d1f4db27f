"""The state model's forward with its weight fragments streamed a phase ahead of their MFMAs (Model::PF_F,
csrc/ude_kernels_mlp.h FS_*) against the same sources compiled with -DUDE_FWD_STREAM=0, bit for bit.

Only the order and the time of the fragment loads differ between the two builds: every MFMA takes the same
operands in the same order, so every output of the forward -- and of the backward, which reads what the
training forward stored -- must be identical.  That says the two builds agree, not that either is right: the
parity tests (test_gpu_parity, test_kernel_order, test_config_lattice_gpu, test_recompute,
test_decoder_epilogue, test_full_size) hold the default build to the fp64 oracle.

The configuration is FaFp_R49_L8_p64-64-32_a64-64, seeded as bench.build.  The two libraries are
tests/fwd_stream_helpers.py's (built by __graft_entry__.build(), or here where missing).  A batch with no more
tiles than CUs would launch the resident-weight forward (Ops::fwd_res), which streams nothing, so both libraries
are loaded and first run under UDE_FWD_RES=0, which the library reads once: N = 35 then runs the kernels under
test.

Which forward variants carry their fragments (state49): every one but the training decoder-epilogue forward,
which is at its register limit and takes the consumption-order loads only; the DYN and SCN forecast variants
carry, and are compared below."""
import contextlib
import os

import pytest
import torch

import fwd_stream_helpers as H

pytestmark = pytest.mark.gpu

R, L = 49, 8
NET, AUG = [64, 64, 32], [64, 64]


@contextlib.contextmanager
def _use(lib):
    """Every solve inside runs on ``lib`` (the selection of tools/ab_flags.py)."""
    from ude_amd import _native, solvers
    saved = _native.library_for
    _native.library_for = lambda cfg, lib=lib: lib
    solvers._PLAN_CACHE.clear()
    try:
        yield
    finally:
        _native.library_for = saved
        solvers._PLAN_CACHE.clear()


def _problem(pkg, N, t):
    """Module, y0, d latent as bench.build makes them (module seed 0, inputs from generator seed 1)."""
    import bench
    torch.manual_seed(0)
    mod = pkg.FaFp(R, latent_dim=L, net_sizes=NET, aug_net_sizes=AUG).cuda()
    gen = torch.Generator().manual_seed(1)
    y0 = bench.synthetic_y0(gen, N, R, L).cuda()
    dlat = torch.randn((len(t), N, R, L), generator=gen).cuda()
    return mod, y0, dlat


@pytest.fixture(scope="module")
def libs(pkg):
    from ude_amd import _native
    paths = H.build_libraries()
    saved = os.environ.get("UDE_FWD_RES")
    os.environ["UDE_FWD_RES"] = "0"
    try:
        out = {w: _native.NativeLib(p) for w, p in paths.items()}
        t = torch.arange(2, dtype=torch.float32)
        mod, y0, _ = _problem(pkg, 3, t)
        for lib in out.values():                     # the switch is read at the library's first forward
            with _use(lib), torch.no_grad():
                pkg.odeint(mod, y0, t, method="rk4", options=dict(step_size=t[1] - t[0]))
        torch.cuda.synchronize()
    finally:
        if saved is None:
            del os.environ["UDE_FWD_RES"]
        else:
            os.environ["UDE_FWD_RES"] = saved
    return out


def _train_step(pkg, mod, y0, t, step, dlat):
    """The training forward and the backward with bench.one_step's cotangents -> {name: tensor}."""
    import bench
    y0 = y0.detach().clone().requires_grad_(True)
    mod.clear_tracking()
    mod.zero_grad(set_to_none=True)
    latent = pkg.odeint(mod, y0, t, method="rk4", options=dict(step_size=step))
    post = mod.posterior()
    norm = torch.norm(torch.stack(mod.tracker))
    torch.autograd.backward([latent, post.loc, post.scale, norm],
                            [dlat, bench._cot([0.3, -0.2], y0.device), bench._cot([0.5, 0.1], y0.device),
                             bench._cot(0.1, y0.device)])
    torch.cuda.synchronize()
    out = {"latent": latent.detach(), "mean": post.loc.detach(), "std": post.scale.detach(), "fa_norm": norm.detach(),
           "d_y0": y0.grad}
    for name, p in mod.named_parameters():
        assert p.grad is not None, name
        out["d_" + name] = p.grad.detach().clone()
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k], b[k]), (k, float((a[k].double() - b[k].double()).abs().max()))


def _both(libs, fn):
    res = {}
    for w, lib in libs.items():
        with _use(lib):
            res[w] = fn()
    _same(res["on"], res["off"])
    return res["on"]


def test_partial_tile_training_step(pkg, libs):
    """N = 35: two full tiles and one of 3; three grid points and an output between two of them."""
    t = torch.tensor([0.0, 1.0, 1.5, 2.0])
    mod, y0, dlat = _problem(pkg, 35, t)
    out = _both(libs, lambda: _train_step(pkg, mod, y0, t, 1.0, dlat))
    assert float(out["latent"][2].abs().sum()) > 0 and float(out["d_y0"].abs().sum()) > 0


def test_tile_boundary_training_step(pkg, libs):
    """N = 16 (2 CUs + 1) + 5 (8,229 on 256 CUs), one RK4 step: the first workgroups run a second tile, whose
    first stage takes the fragments issued in the first tile's last stage."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 16 * (2 * cus + 1) + 5
    t = torch.arange(2, dtype=torch.float32)
    mod, y0, dlat = _problem(pkg, N, t)
    _both(libs, lambda: _train_step(pkg, mod, y0, t, 1.0, dlat))


def test_inference_and_decoder_epilogue(pkg, libs):
    """The inference forward, and decoder_head.solve_decode in training (with its backward) and without grad."""
    from ude_amd import decoder_head
    t = torch.arange(3, dtype=torch.float32)
    mod, y0, dlat = _problem(pkg, 35, t)
    torch.manual_seed(R)
    lin = torch.nn.Linear(3 * R, R).cuda()
    c_yhat = torch.randn(len(t), 35, R, generator=torch.Generator().manual_seed(2)).cuda()

    def run():
        out = {}
        with torch.no_grad():
            mod.clear_tracking()
            out["latent_inf"] = pkg.odeint(mod, y0, t, method="rk4", options=dict(step_size=1.0))
            post = mod.posterior()
            out["mean_inf"], out["std_inf"] = post.loc, post.scale
            mod.clear_tracking()
            yhat, reg, lazy, _plan = decoder_head.solve_decode(mod, y0, t, 1.0, lin)
            out["yhat_inf"], out["reg_inf"], out["latent_dec_inf"] = yhat, reg, lazy.get()
        yg = y0.detach().clone().requires_grad_(True)
        mod.clear_tracking()
        mod.zero_grad(set_to_none=True)
        lin.zero_grad(set_to_none=True)
        assert decoder_head.eligible(mod, yg, lin)
        yhat, reg, lazy, _plan = decoder_head.solve_decode(mod, yg, t, 1.0, lin)
        lat = lazy.get()
        ((yhat * c_yhat).sum() + 0.7 * reg + (lat * dlat).sum()).backward()
        torch.cuda.synchronize()
        out.update(yhat=yhat.detach(), reg=reg.detach(), latent_dec=lat.detach(), d_y0=yg.grad,
                   d_dec_w=lin.weight.grad.detach().clone(), d_dec_b=lin.bias.grad.detach().clone())
        for name, p in mod.named_parameters():
            assert p.grad is not None, name
            out["d_" + name] = p.grad.detach().clone()
        mod.clear_tracking()
        return out

    _both(libs, run)


def test_forecast_variants(pkg, libs):
    """The inference decoder-epilogue forward behind the forecast: plain, with the dynamics channels (DYN), and
    a scenario with and without them (SCN)."""
    from ude_amd.forecast import (_forecast_plan, solve_decode_dynamics, solve_decode_forecast,
                                  solve_decode_scenario)
    t = torch.arange(3, dtype=torch.float32)
    mod, y0, _ = _problem(pkg, 35, t)
    torch.manual_seed(R)
    lin = torch.nn.Linear(3 * R, R).cuda()
    gen = torch.Generator().manual_seed(3)

    def run():
        out = {}
        mod.clear_tracking()
        out["yhat"] = solve_decode_forecast(mod, y0, t, 1.0, lin)
        mod.clear_tracking()
        out["yhat_dyn"], out["dyn"], _names = solve_decode_dynamics(mod, y0, t, 1.0, lin)
        mod.clear_tracking()
        n_steps = int(_forecast_plan(mod, y0, t, 1.0).prob.n_steps)
        table = (0.5 + torch.rand(n_steps, R, 2, generator=torch.Generator().manual_seed(gen.initial_seed()))).cuda()
        for flag in (False, True):
            y, dyn, _names, rates = solve_decode_scenario(mod, y0, t, 1.0, lin, table, dynamics=flag)
            out[f"yhat_scn{int(flag)}"] = y
            out[f"mean_scn{int(flag)}"], out[f"std_scn{int(flag)}"] = rates.mean, rates.std
            if flag:
                out["dyn_scn"] = dyn
        torch.cuda.synchronize()
        mod.clear_tracking()
        return out

    _both(libs, run)
