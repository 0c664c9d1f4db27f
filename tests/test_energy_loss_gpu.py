"""The energy-score training head on the MI355X: the gfx950 kernels (csrc/ude_energy.h through
``decoder_head.energy_head``) against the brute-force NumPy reference of tests/energy_helpers.py, the C-ABI's
error codes, the head inside ``VAE.calc_loss`` on the decoder-epilogue route and on the written-latent route, and
the training history."""
import ctypes

import numpy as np
import pytest
import torch

import energy_helpers as eh
from conftest import load_golden
from helpers import normwise_rel

pytestmark = pytest.mark.gpu


def _run_head(case, block, fair, g):
    """(out fp32 scalar tensor, dyhat (T, S*B, R) fp32, event kinds of the forward, of the backward)."""
    from ude_amd import decoder_head, fused
    yhat = torch.tensor(case.yhat).cuda().requires_grad_(True)
    y = torch.tensor(case.y).cuda()
    fused.EVENTS = []
    try:
        out = decoder_head.energy_head(yhat, y, case.S, case.B, block=block, fair=fair)
        fwd = [k for k, _, _ in fused.EVENTS]
        fused.EVENTS = []
        (g * out).backward()
        bwd = [k for k, _, _ in fused.EVENTS]
    finally:
        fused.EVENTS = None
    torch.cuda.synchronize()
    return out.detach(), yhat.grad.detach(), fwd, bwd


def _check_against_reference(case, block, fair, g, out, dyhat):
    ref = eh.reference(case.name, block, fair)
    v = float(out)
    print(f"{case.name} {block} fair={fair} g={g}: out {v!r} reference {ref.loss!r}")
    assert abs(v - ref.loss) <= 2.0 ** -23 * abs(ref.loss), (v, ref.loss)      # one fp32 rounding of an fp64 value
    grad = dyhat.cpu().numpy().astype(np.float64)
    want = g * ref.grad
    excess = np.abs(grad - want) - eh.grad_bound(case, block, want, g)
    print(f"  worst gradient error {np.abs(grad - want).max():.3e}, over the bar by {excess.max():.3e}")
    assert np.isfinite(grad).all() and excess.max() <= 0.0
    assert not grad[ref.dropped].any()                                         # exact zeros exactly zero


@pytest.mark.parametrize("name,block,fair", eh.CASE_BLOCK_FAIR)
def test_energy_head_matches_brute_force(pkg, name, block, fair):
    case = eh.make_case(name)
    for g in eh.COTANGENTS:
        out, dyhat, fwd, bwd = _run_head(case, block, fair, g)
        assert fwd == ["energy_fwd"] and bwd == ["energy_bwd"], (fwd, bwd)     # the native path ran
        assert out.dtype == torch.float32 and dyhat.dtype == torch.float32
        _check_against_reference(case, block, fair, g, out, dyhat)
        out2, dyhat2, _, _ = _run_head(case, block, fair, g)                   # the same bits run to run
        assert torch.equal(out, out2) and torch.equal(dyhat, dyhat2)
    if name == "masked_all":
        assert float(out) == 0.0 and not bool(dyhat.any())


def test_energy_head_rejects_bad_arguments(pkg):
    from ude_amd import decoder_head
    case = eh.make_case("one_sample")
    yhat, y = torch.tensor(case.yhat).cuda(), torch.tensor(case.y).cuda()
    with pytest.raises(ValueError):
        decoder_head.energy_head(yhat, y, 1, case.B, fair=True)
    with pytest.raises(ValueError):
        decoder_head.energy_head(yhat, y, 1, case.B, block="region")


def test_energy_head_above_the_sample_cap_takes_the_torch_definition(pkg):
    """S = 129: no kernel launch (a thread of the pair sweep holds the partners of 128 samples and the target),
    the same definition in torch on the device, bit for bit; that definition in fp64 on the device is the brute
    force's value at the CPU tests' bars.  The fp32 value has fp32's bar for this shape: per block two recursive
    or pairwise sums of at most S^2 roots, each root of C squares: (S^2 + C + 4) u sum |terms| with u = 2^-24
    bounds both sums; after the division their terms' absolute values add up to at most 2 max |x_i - x_j|_C <=
    4 sqrt(C) max|x|."""
    import lib.train_functions as tf
    from ude_amd import decoder_head, fused
    T, S, B, R = 2, 129, 2, 3
    rng = np.random.default_rng(5)
    y = (2.0 + rng.random((B, T, R))).astype(np.float32)
    x = (y.transpose(1, 0, 2)[:, None] + 0.5 * rng.standard_normal((T, S, B, R))).astype(np.float32)
    x64 = x.astype(np.float64)
    want = 0.0
    for b in range(B):
        X = x64[:, :, b].transpose(1, 0, 2).reshape(S, T * R)
        d = X[:, None] - X[None]
        want += np.sqrt(((X - y[b].reshape(-1)) ** 2).sum(-1)).sum() / S - np.sqrt((d * d).sum(-1)).sum() / (2.0 * S * S)
    want /= B
    yhat = torch.tensor(x.reshape(T, S * B, R)).cuda().requires_grad_(True)
    y_dev = torch.from_numpy(y).cuda()
    fused.EVENTS = []
    try:
        out = decoder_head.energy_head(yhat, y_dev, S, B)
        out.backward()
        kinds = [k for k, _, _ in fused.EVENTS]
    finally:
        fused.EVENTS = None
    assert kinds == []
    y_pred = yhat.detach().reshape(T, S, B, R).permute(2, 1, 0, 3)
    assert torch.equal(out.detach(), tf.energy_loss(y_pred, y_dev))
    v64 = float(tf.energy_loss(y_pred.double(), y_dev.double()))
    assert abs(v64 - want) <= 1e-13 * abs(want), (v64, want)
    C = T * R
    assert abs(float(out.detach()) - want) <= (S * S + C + 4) * 2.0 ** -24 * 4 * np.sqrt(C) * float(np.abs(x).max())
    assert bool(torch.isfinite(yhat.grad).all()) and bool(yhat.grad.any())


def test_energy_cabi_error_codes(pkg):
    """Invalid arguments only (valid device memory throughout): S = 129, fair with S = 1, a block kind of 3, T or
    R of 1025, a null pointer, a misaligned workspace."""
    from ude_amd import _native, forecast
    lib = forecast._library()
    T, B, R = 1, 2, 3
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p, stream = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    n = ctypes.c_int64(-1)
    inv = _native.UDE_E_INVALID
    assert lib._rc("ude_energy_workspace", T, 129, B, R, 0, n) == inv
    assert lib._rc("ude_energy_workspace", T, 4, B, R, 3, n) == inv
    assert lib._rc("ude_energy_workspace", T, 4, B, R, -1, n) == inv
    assert lib._rc("ude_energy_workspace", 1025, 4, B, R, 0, n) == inv
    assert lib._rc("ude_energy_workspace", T, 4, B, 1025, 0, n) == inv
    assert lib._rc("ude_energy_workspace", T, 4, B, R, 0, None) == inv
    assert lib._rc("ude_energy_forward", T, 129, B, R, 0, 0, p, p, p, p, stream) == inv
    assert lib._rc("ude_energy_forward", T, 1, B, R, 0, 1, p, p, p, p, stream) == inv
    assert lib._rc("ude_energy_forward", T, 4, B, R, 3, 0, p, p, p, p, stream) == inv
    assert lib._rc("ude_energy_forward", T, 4, B, R, 0, 0, None, p, p, p, stream) == inv
    assert lib._rc("ude_energy_forward", T, 4, B, R, 0, 0, p, p, p, None, stream) == inv
    assert lib._rc("ude_energy_backward", T, 129, B, R, 0, 0, p, p, p, p, stream) == inv
    assert lib._rc("ude_energy_backward", T, 1, B, R, 0, 1, p, p, p, p, stream) == inv
    assert lib._rc("ude_energy_backward", T, 4, B, R, 3, 0, p, p, p, p, stream) == inv
    assert lib._rc("ude_energy_backward", T, 4, B, R, 0, 0, p, p, None, p, stream) == inv
    assert lib._rc("ude_energy_backward", T, 4, B, R, 0, 0, p, p, p, None, stream) == inv
    # a workspace that is not 8-byte aligned (its fp64 partials): refused, not launched
    assert lib._rc("ude_energy_forward", T, 4, B, R, 0, 0, p, p, p + 4, p, stream) == inv
    # the partials of every (window, block, sample tile), and one more per 256 blocks
    assert lib.energy_workspace(T, 4, B, R, 0) == (B * 1 * 1 * 2 + 1) * 8
    assert lib.energy_workspace(9, 64, 320, 49, 1) == (320 * 49 * 4 * 2 + (320 * 49 + 255) // 256) * 8
    assert lib.energy_workspace(9, 64, 320, 49, 2) == (320 * 9 * 4 * 2 + (320 * 9 + 255) // 256) * 8
    torch.cuda.synchronize()
    assert not bool(buf.any())                                       # nothing was launched


# ---- inside VAE.calc_loss ---------------------------------------------------------------------------

def _e2e_step(g, monkeypatch, route, t_shift=0.0, block="joint", **overrides):
    """One step of a fresh model on the fixture's inputs and eps.  route 'head': calc_loss with {"energy": 1.0}
    added; 'torch': calc_loss without it, plus 1.0 * train_functions.energy_loss(y_pred, y) on the device
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
            loss, data, names = model.calc_loss(y_pred, y[:, ev, :], dict(losses, energy=1.0, energy_block=block))
        else:
            loss, data, names = model.calc_loss(y_pred, y[:, ev, :], losses)
            loss = loss + 1.0 * tf.energy_loss(y_pred, y[:, ev, :], block=block)
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
    """The CRPS head's end-to-end bars (tests/test_e2e_vae.py's floors): loss 2e-5 relative, every gradient 5e-5
    normwise."""
    loss_a, grads_a = a[0], a[1]
    loss_b, grads_b = b[0], b[1]
    print(f"loss head {loss_a!r} torch {loss_b!r}")
    assert abs(loss_a - loss_b) <= 2e-5 * abs(loss_b), (loss_a, loss_b)
    worst = {k: normwise_rel(grads_a[k], grads_b[k]) for k in grads_b}
    print("worst normwise gradient differences:", sorted(worst.items(), key=lambda kv: -kv[1])[:4])
    for k, e in worst.items():
        assert e < 5e-5, (k, e)


@pytest.mark.parametrize("fixture,block", [("e2e_vae_toy64", "joint"), ("e2e_vae_state49", "joint"),
                                           ("e2e_vae_state49", "series"), ("e2e_vae_state49", "field")])
def test_calc_loss_energy_head_on_the_epilogue_route(pkg, monkeypatch, fixture, block):
    from ude_amd.decoder_head import LazyLatent
    g = load_golden(fixture)
    a = _e2e_step(g, monkeypatch, "head", block=block)
    b = _e2e_step(g, monkeypatch, "torch", block=block)
    names0 = g["meta"]["loss_names"]
    i = names0.index("nll")
    assert a[3] == names0[:i + 1] + ["energy"] + names0[i + 1:] and b[3] == names0
    assert {"fwd_dec", "nll_fwd", "energy_fwd", "energy_bwd", "nll_bwd", "dec_bwd", "bwd"} <= set(a[2]), a[2]
    assert "energy_fwd" not in b[2]
    # the epilogue route: no latent was written
    assert isinstance(a[4], LazyLatent) and not a[4].materialized
    _compare(a, b)


def test_calc_loss_energy_as_the_only_data_term_on_the_epilogue_route(pkg, monkeypatch):
    """"nll": False with the energy term: the epilogue's reg is kept, no nll kernel runs, every parameter gets
    its gradient, and the step equals the torch definition's at the same bars (here the data gradient is the
    energy term's alone, not a small part of nll's)."""
    from ude_amd.decoder_head import LazyLatent
    g = load_golden("e2e_vae_state49")
    a = _e2e_step(g, monkeypatch, "head", nll=False)
    b = _e2e_step(g, monkeypatch, "torch", nll=False)
    assert "energy" in a[3] and "nll" not in a[3] and "reg_loss" in a[3]
    assert {"fwd_dec", "energy_fwd", "energy_bwd", "dec_bwd", "bwd"} <= set(a[2]) and "nll_fwd" not in a[2], a[2]
    assert isinstance(a[4], LazyLatent) and not a[4].materialized
    assert all(bool(torch.isfinite(v).all()) for v in a[1].values())
    _compare(a, b)


def test_calc_loss_energy_head_on_the_written_latent_route(pkg, monkeypatch):
    """Output times between grid points: the epilogue does not apply, the latent is written and decoded, and the
    energy term still runs on the kernels, over y_pred laid out as y_hat."""
    from ude_amd.decoder_head import LazyLatent
    g = load_golden("e2e_vae_toy64")
    t, ev = g["t"], g["eval_pts"]
    shift = 0.25 * float(t[ev[1]] - t[ev[0]])      # a quarter of the solve's step (t_out[1] - t_out[0])
    a = _e2e_step(g, monkeypatch, "head", t_shift=shift)
    b = _e2e_step(g, monkeypatch, "torch", t_shift=shift)
    assert not isinstance(a[4], LazyLatent) and torch.is_tensor(a[4])
    assert "fwd_dec" not in a[2] and "energy_fwd" in a[2] and "energy_bwd" in a[2], a[2]
    assert "energy_fwd" not in b[2]
    _compare(a, b)


def test_train_history_records_the_joint_energy_score(pkg, monkeypatch, tmp_path):
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
    h = one_epoch(dict(g["meta"]["losses"], energy=1.0))
    assert np.isfinite(h["forecast_energy"]) and h["forecast_energy"] > 0
    assert np.isfinite(h["forecast_nll"]) and "energy" in h and "forecast_crps" not in h
    h = one_epoch(dict(g["meta"]["losses"]))
    assert "forecast_energy" not in h and "forecast_nll" in h
