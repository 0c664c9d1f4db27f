"""The CRPS training head on the MI355X: the gfx950 kernels (csrc/ude_crps.h through ``decoder_head.crps_head``)
against the brute-force NumPy reference of tests/crps_helpers.py, the C-ABI's error codes, the head inside
``VAE.calc_loss`` on the decoder-epilogue route and on the written-latent route, and the training history."""
import ctypes

import numpy as np
import pytest
import torch

import crps_helpers as ch
from conftest import load_golden
from helpers import normwise_rel

pytestmark = pytest.mark.gpu


def _run_head(case, fair, g):
    """(out fp32 scalar tensor, dyhat (T, S*B, R) fp32, event kinds of the forward, of the backward)."""
    from ude_amd import decoder_head, fused
    yhat = torch.tensor(case.yhat).cuda().requires_grad_(True)
    y = torch.tensor(case.y).cuda()
    fused.EVENTS = []
    try:
        out = decoder_head.crps_head(yhat, y, case.S, case.B, fair=fair)
        fwd = [k for k, _, _ in fused.EVENTS]
        fused.EVENTS = []
        (g * out).backward()
        bwd = [k for k, _, _ in fused.EVENTS]
    finally:
        fused.EVENTS = None
    torch.cuda.synchronize()
    return out.detach(), yhat.grad.detach(), fwd, bwd


def _check_against_reference(case, fair, g, out, dyhat):
    ref = ch.reference(case.name, fair)
    v = float(out)
    print(f"{case.name} fair={fair} g={g}: out {v!r} reference {ref.loss!r}")
    assert abs(v - ref.loss) <= 2.4e-7 * abs(ref.loss) + 1e-12 * float(np.abs(case.yhat).max()), (v, ref.loss)
    grad = dyhat.cpu().numpy()
    assert np.array_equal(ch.recovered_numerators(grad, case, fair, g), ref.num)
    want = ch.reference_grad(case.name, fair, g)
    assert np.array_equal(grad == 0.0, want == 0.0)                   # exact zeros where the reference is zero
    nz = want != 0.0
    err = np.abs(grad.astype(np.float64)[nz] - want[nz]) / np.abs(want[nz])
    print(f"  worst relative gradient error {err.max() if err.size else 0.0:.3e}")
    assert not err.size or err.max() <= 2.0 ** -22


@pytest.mark.parametrize("name,fair", ch.CASE_FAIR)
def test_crps_head_matches_brute_force(pkg, name, fair):
    case = ch.make_case(name)
    for g in ch.COTANGENTS:
        out, dyhat, fwd, bwd = _run_head(case, fair, g)
        assert fwd == ["crps_fwd"] and bwd == ["crps_bwd"], (fwd, bwd)      # the native path ran
        assert out.dtype == torch.float32 and dyhat.dtype == torch.float32
        _check_against_reference(case, fair, g, out, dyhat)
        out2, dyhat2, _, _ = _run_head(case, fair, g)                        # the same bits run to run
        assert torch.equal(out, out2) and torch.equal(dyhat, dyhat2)
    if name == "masked_all":
        assert float(out) == 0.0 and not bool(dyhat.any())
    if name == "one_sample":
        y = torch.tensor(case.y).double()
        x = torch.tensor(case.yhat).double().reshape(case.T, case.B, case.R).permute(1, 0, 2)
        mae = float(((x - y).abs() * (y != -1)).mean())
        assert abs(float(out) - mae) <= 2.4e-7 * mae


def test_crps_head_one_sample_fair_raises(pkg):
    from ude_amd import decoder_head
    case = ch.make_case("one_sample")
    with pytest.raises(ValueError):
        decoder_head.crps_head(torch.tensor(case.yhat).cuda(), torch.tensor(case.y).cuda(), 1, case.B, fair=True)


def test_crps_head_above_the_sample_cap_takes_the_torch_definition(pkg):
    """S = 1025: no kernel launch (the sorted tile holds 1024 samples), the same definition in torch on the
    device; against the brute force at fp32's bar for this shape.  The value is formed in fp32 here, not
    rounded once from fp64: per group two recursive sums of S terms, sum |x - y| / S and sum (2 i - S + 1) x_(i)
    / S^2, whose terms' absolute values add up to at most max|x| after the division; the standard bound n u
    sum |terms| with u = 2^-24 gives (S + 1) u max|x| for each, and the mean over the groups does not grow it."""
    import lib.train_functions as tf
    from ude_amd import decoder_head, fused
    T, S, B, R = 1, 1025, 2, 1
    rng = np.random.default_rng(5)
    y = (2.0 + rng.random((B, T, R))).astype(np.float32)
    x = (y.transpose(1, 0, 2)[:, None] + 0.5 * rng.standard_normal((T, S, B, R))).astype(np.float32)
    case = ch.Case("above_cap", T, S, B, R, x.reshape(T, S * B, R), y)
    x64, y64 = x.astype(np.float64), y.astype(np.float64).transpose(1, 0, 2)
    pair = sum(np.abs(x64[:, i:i + 1] - x64).sum(1) for i in range(S))
    want = float((np.abs(x64 - y64[:, None]).sum(1) / S - pair / (2.0 * S * S)).sum() / (B * T * R))
    n_lt = np.stack([(x64 < x64[:, i:i + 1]).sum(1) for i in range(S)], 1)
    n_le = np.stack([(x64 <= x64[:, i:i + 1]).sum(1) for i in range(S)], 1)
    num = (S * np.sign(x64 - y64[:, None]).astype(np.int64) - (n_lt + n_le - S)).reshape(T, S * B, R)
    yhat = torch.tensor(case.yhat).cuda().requires_grad_(True)
    fused.EVENTS = []
    try:
        out = decoder_head.crps_head(yhat, torch.from_numpy(y).cuda(), S, B)
        out.backward()
        kinds = [k for k, _, _ in fused.EVENTS]
    finally:
        fused.EVENTS = None
    assert kinds == []
    # it is the torch definition, bit for bit, and that definition in fp64 on the device is the brute force's
    # value to fp64 rounding (1e-13, the CPU tests' bar); the fp32 value itself only has the worst-case bar
    y_dev = torch.from_numpy(y).cuda()
    y_pred = yhat.detach().reshape(T, S, B, R).permute(2, 1, 0, 3)
    assert torch.equal(out.detach(), tf.crps_loss(y_pred, y_dev))
    v64 = float(tf.crps_loss(y_pred.double(), y_dev.double()))
    assert abs(v64 - want) <= 1e-13 * abs(want), (v64, want)
    assert abs(float(out.detach()) - want) <= 2 * (S + 1) * 2.0 ** -24 * float(np.abs(x).max())
    assert np.array_equal(ch.recovered_numerators(yhat.grad.cpu().numpy(), case, False, 1.0), num)


def test_crps_cabi_error_codes(pkg):
    """Invalid arguments only (valid device memory throughout): S = 1025, fair with S = 1, a null pointer."""
    from ude_amd import _native, forecast
    lib = forecast._library()
    T, B, R = 1, 2, 3
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p, stream = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    n = ctypes.c_int64(-1)
    assert lib._rc("ude_crps_workspace", T, 1025, B, R, n) == _native.UDE_E_INVALID
    assert lib._rc("ude_crps_workspace", T, 4, B, R, None) == _native.UDE_E_INVALID
    assert lib._rc("ude_crps_forward", T, 1025, B, R, 0, p, p, p, p, stream) == _native.UDE_E_INVALID
    assert lib._rc("ude_crps_forward", T, 1, B, R, 1, p, p, p, p, stream) == _native.UDE_E_INVALID
    assert lib._rc("ude_crps_forward", T, 4, B, R, 0, None, p, p, p, stream) == _native.UDE_E_INVALID
    assert lib._rc("ude_crps_backward", T, 1025, B, R, 0, p, p, p, stream) == _native.UDE_E_INVALID
    assert lib._rc("ude_crps_backward", T, 1, B, R, 1, p, p, p, stream) == _native.UDE_E_INVALID
    assert lib._rc("ude_crps_backward", T, 4, B, R, 0, p, p, None, stream) == _native.UDE_E_INVALID
    # a workspace that is not 8-byte aligned (its fp64 partials): refused, not launched
    assert lib._rc("ude_crps_forward", T, 4, B, R, 0, p, p, p + 4, p, stream) == _native.UDE_E_INVALID
    assert lib._rc("ude_crps_backward", T, 4, B, R, 0, p, p + 4, p, stream) == _native.UDE_E_INVALID
    assert lib.crps_workspace(T, 4, B, R) >= T * 4 * B * R * 2 + 8
    assert lib.crps_workspace(1, 3, 43, 1) == 256 + 2 * 129          # every byte counted: no multiple of 4
    torch.cuda.synchronize()
    assert not bool(buf.any())                                       # nothing was launched


# ---- inside VAE.calc_loss ---------------------------------------------------------------------------

def _e2e_step(g, monkeypatch, route, t_shift=0.0, **overrides):
    """One step of a fresh model on the fixture's inputs and eps.  route 'head': calc_loss with {"crps": 1.0}
    added; 'torch': calc_loss without it, plus 1.0 * train_functions.crps_loss(y_pred, y) on the device
    prediction before backward().  Both share the solve and its backward; only d y_hat's source differs.
    ``overrides`` change the fixture's losses on both routes."""
    import lib.train_functions as tf
    from ude_amd import fused
    from test_e2e_vae import _build
    model = _build(None, g, "cuda")
    eps = torch.from_numpy(g["eps"]).cuda()
    monkeypatch.setattr(torch, "randn", lambda *a, **k: eps.clone())
    x, y = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["y"]).cuda()
    t, ev = torch.from_numpy(g["t"]), g["eval_pts"]
    t_out = t[ev].clone()
    if t_shift:
        t_out[2] += t_shift                        # an output time between grid points: the latent is written
    model.optimizer.zero_grad()
    losses = dict(g["meta"]["losses"], **overrides)
    fused.EVENTS = []
    try:
        y_pred = model(x, t_out, n_samples=g["meta"]["n_samples"], training=True)
        if route == "head":
            loss, data, names = model.calc_loss(y_pred, y[:, ev, :], dict(losses, crps=1.0))
        else:
            loss, data, names = model.calc_loss(y_pred, y[:, ev, :], losses)
            loss = loss + 1.0 * tf.crps_loss(y_pred, y[:, ev, :])
        lazy = model.__dict__["_latent"]
        loss.backward()
        kinds = [k for k, _, _ in fused.EVENTS]
    finally:
        fused.EVENTS = None
        monkeypatch.undo()
    torch.cuda.synchronize()
    grads = {f"{part}.{k}": p.grad.detach().clone() for part in ("enc", "ode", "dec")
             for k, p in getattr(model, part).named_parameters()}
    return float(loss.detach()), grads, kinds, names, lazy


def _compare(a, b):
    """This project's own floors (tests/test_e2e_vae.py): loss 2e-5 relative, every gradient 5e-5 normwise."""
    loss_a, grads_a = a[0], a[1]
    loss_b, grads_b = b[0], b[1]
    print(f"loss head {loss_a!r} torch {loss_b!r}")
    assert abs(loss_a - loss_b) <= 2e-5 * abs(loss_b), (loss_a, loss_b)
    worst = {k: normwise_rel(grads_a[k], grads_b[k]) for k in grads_b}
    print("worst normwise gradient differences:", sorted(worst.items(), key=lambda kv: -kv[1])[:4])
    for k, e in worst.items():
        assert e < 5e-5, (k, e)


@pytest.mark.parametrize("fixture", ["e2e_vae_toy64", "e2e_vae_state49"])
def test_calc_loss_crps_head_on_the_epilogue_route(pkg, monkeypatch, fixture):
    from ude_amd.decoder_head import LazyLatent
    g = load_golden(fixture)
    a = _e2e_step(g, monkeypatch, "head")
    b = _e2e_step(g, monkeypatch, "torch")
    names0 = g["meta"]["loss_names"]
    i = names0.index("nll")
    assert a[3] == names0[:i + 1] + ["crps"] + names0[i + 1:] and b[3] == names0
    assert {"fwd_dec", "nll_fwd", "crps_fwd", "crps_bwd", "nll_bwd", "dec_bwd", "bwd"} <= set(a[2]), a[2]
    assert "crps_fwd" not in b[2]
    # the epilogue route: no latent was written
    assert isinstance(a[4], LazyLatent) and not a[4].materialized
    _compare(a, b)


def test_calc_loss_crps_as_the_only_data_term_on_the_epilogue_route(pkg, monkeypatch):
    """"nll": False with the CRPS term: the epilogue's reg is kept, no nll kernel runs, every parameter gets its
    gradient, and the step equals the torch definition's at the same bars (here the data gradient is the CRPS
    term's alone, not a small part of nll's)."""
    from ude_amd.decoder_head import LazyLatent
    g = load_golden("e2e_vae_state49")
    a = _e2e_step(g, monkeypatch, "head", nll=False)
    b = _e2e_step(g, monkeypatch, "torch", nll=False)
    assert "crps" in a[3] and "nll" not in a[3] and "reg_loss" in a[3]
    assert {"fwd_dec", "crps_fwd", "crps_bwd", "dec_bwd", "bwd"} <= set(a[2]) and "nll_fwd" not in a[2], a[2]
    assert isinstance(a[4], LazyLatent) and not a[4].materialized
    assert all(bool(torch.isfinite(v).all()) for v in a[1].values())
    _compare(a, b)


def test_calc_loss_crps_head_on_the_written_latent_route(pkg, monkeypatch):
    """Output times between grid points: the epilogue does not apply, the latent is written and decoded, and the
    CRPS term still runs on the kernels, over y_pred laid out as y_hat."""
    from ude_amd.decoder_head import LazyLatent
    g = load_golden("e2e_vae_toy64")
    t, ev = g["t"], g["eval_pts"]
    shift = 0.25 * float(t[ev[1]] - t[ev[0]])      # a quarter of the solve's step (t_out[1] - t_out[0])
    a = _e2e_step(g, monkeypatch, "head", t_shift=shift)
    b = _e2e_step(g, monkeypatch, "torch", t_shift=shift)
    assert not isinstance(a[4], LazyLatent) and torch.is_tensor(a[4])
    assert "fwd_dec" not in a[2] and "crps_fwd" in a[2] and "crps_bwd" in a[2], a[2]
    assert "crps_fwd" not in b[2]
    _compare(a, b)


def test_train_history_records_the_ensemble_crps(pkg, monkeypatch, tmp_path):
    from test_e2e_vae import _build
    monkeypatch.chdir(tmp_path)
    g = load_golden("e2e_vae_toy64")
    model = _build(None, g, "cuda")
    x, y = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["y"]).cuda()
    t, ev = torch.from_numpy(g["t"]), [int(e) for e in g["eval_pts"]]
    R = y.shape[-1]
    torch.manual_seed(0)
    validate = {"x_test": x, "y_test": y, "t": t, "scaler": np.ones(R), "n_samples": 4}

    def one_epoch(losses):
        model.train([(x, y)], t, 1, losses, ev, n_samples=g["meta"]["n_samples"], grad_lim=1e9, disable=True,
                    norm_file=str(tmp_path / "norms.txt"), validate=validate)
        return model._history.epoch_history[-1]
    h = one_epoch(dict(g["meta"]["losses"], crps=1.0))
    assert np.isfinite(h["forecast_crps"]) and np.isfinite(h["all_crps"]) and h["all_crps"] > 0
    assert np.isfinite(h["forecast_nll"]) and "crps" in h
    h = one_epoch(dict(g["meta"]["losses"]))
    assert "forecast_crps" not in h and "all_crps" not in h and "forecast_nll" in h
