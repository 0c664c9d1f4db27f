"""The energy-score training loss on the CPU: ``train_functions.energy_loss`` (the torch definition of the head
at ude_energy_forward in include/ude_rk4.h) against the brute-force NumPy reference of tests/energy_helpers.py,
its identities with the scores the forecast reports and with the CRPS loss, its wiring into ``VAE.calc_loss``
and the training history, and the C-ABI declarations."""
import os
import re

import numpy as np
import pytest
import torch

import energy_helpers as eh
from conftest import REPO, load_golden


def _y_pred(case, dtype=torch.float64):
    """(B, S, T, R) as lib/VAE.py reshapes y_hat, a leaf that requires grad."""
    yhat = torch.tensor(case.yhat).to(dtype)
    return yhat.reshape(case.T, case.S, case.B, case.R).permute(2, 1, 0, 3).contiguous().requires_grad_(True)


def _to_yhat_layout(grad, case):
    return grad.permute(2, 1, 0, 3).reshape(case.T, case.S * case.B, case.R)


@pytest.mark.parametrize("name,block,fair", eh.CASE_BLOCK_FAIR)
def test_energy_loss_matches_brute_force(pkg, name, block, fair):
    import lib.train_functions as tf
    case, ref = eh.make_case(name), eh.reference(name, block, fair)
    y = torch.tensor(case.y).double()
    for g in eh.COTANGENTS:
        yp = _y_pred(case)
        loss = tf.energy_loss(yp, y, block=block, fair=fair)
        assert abs(float(loss.detach()) - ref.loss) <= 1e-13 * abs(ref.loss), (float(loss.detach()), ref.loss)
        (g * loss).backward()
        grad = _to_yhat_layout(yp.grad, case).numpy()
        assert np.isfinite(grad).all()
        assert np.abs(grad - g * ref.grad).max() <= 1e-14
        assert not grad[ref.dropped].any()                            # exact zeros at masked coordinates
    if name == "masked_all":
        assert float(loss.detach()) == 0.0 and not grad.any()
    if name == "one_sample":
        # the pair term is exactly 0: the loss is the mean over the blocks of |x - y|_C
        x = torch.tensor(case.yhat).double().reshape(case.T, case.B, case.R).permute(1, 0, 2)
        over = {"joint": (1, 2), "series": (1,), "field": (2,)}[block]
        want = float((((x - y) ** 2) * (y != -1)).sum(over).sqrt().mean())
        assert abs(float(loss.detach()) - want) <= 1e-13 * want


def test_energy_loss_chunks_give_the_same_value(pkg, monkeypatch):
    """Windows, and within a window the samples i, a chunk at a time: the same value and gradient to rounding."""
    import lib.train_functions as tf
    case = eh.make_case("partial_tiles")
    y = torch.tensor(case.y).double()
    a = _y_pred(case)
    (-3.5 * tf.energy_loss(a, y, block="series", fair=True)).backward()
    per_window = case.S * case.S * case.T * case.R * 8
    monkeypatch.setattr(tf, "ENERGY_CHUNK_BYTES", per_window // 5)     # one window and 6 samples i per chunk
    b = _y_pred(case)
    loss = tf.energy_loss(b, y, block="series", fair=True)
    (-3.5 * loss).backward()
    ref = eh.reference("partial_tiles", "series", True)
    assert abs(float(loss.detach()) - ref.loss) <= 1e-13 * abs(ref.loss)
    assert (a.grad - b.grad).abs().max() <= 1e-14


def test_energy_loss_rejects_bad_arguments(pkg):
    import lib.train_functions as tf
    case = eh.make_case("one_sample")
    y = torch.tensor(case.y).double()
    with pytest.raises(ValueError):
        tf.energy_loss(_y_pred(case), y, fair=True)                    # fair needs S >= 2
    with pytest.raises(ValueError):
        tf.energy_loss(_y_pred(case), y, block="region")


@pytest.mark.parametrize("name", ["odd_S", "partial_tiles", "wide_R"])
def test_energy_loss_is_the_score_the_forecast_reports(pkg, name):
    """D = S, no mask, no scaler: the joint / series / field loss is the mean over the windows of
    ensemble_joint's energy_joint / energy_series / energy_field."""
    import lib.train_functions as tf
    from ude_amd import forecast
    case = eh.make_case(name)
    assert not (case.y == -1).any()
    y = torch.tensor(case.y)
    js = forecast.ensemble_joint(torch.tensor(case.yhat), case.S, case.B, y)
    for block, scores in (("joint", js.energy_joint), ("series", js.energy_series), ("field", js.energy_field)):
        loss = float(tf.energy_loss(_y_pred(case), y.double(), block=block).detach())
        assert abs(loss - float(scores.double().mean())) <= 1e-12 * abs(loss), block


@pytest.mark.parametrize("name,block,fair", [("odd_S", "field", False), ("odd_S", "field", True),
                                             ("one_coord", "field", False), ("one_coord", "series", True),
                                             ("max_S", "series", False), ("one_coord", "joint", False)])
def test_energy_loss_of_one_coordinate_blocks_is_the_crps_loss(pkg, name, block, fair):
    """R = 1: field is crps_loss; T = 1: series is crps_loss (T = R = 1: joint too)."""
    import lib.train_functions as tf
    case = eh.make_case(name)
    assert eh.block_coords(case, block) == 1
    y = torch.tensor(case.y).double()
    e = float(tf.energy_loss(_y_pred(case), y, block=block, fair=fair).detach())
    c = float(tf.crps_loss(_y_pred(case), y, fair=fair).detach())
    assert abs(e - c) <= 1e-12 * abs(c), (e, c)


# ---- VAE.calc_loss ----------------------------------------------------------------------------------

def _calc(g, losses, monkeypatch):
    from test_e2e_vae import _build
    model = _build(None, g, "cpu")
    eps = torch.from_numpy(g["eps"])
    monkeypatch.setattr(torch, "randn", lambda *a, **k: eps.clone())
    x, y, t, ev = torch.from_numpy(g["x"]), torch.from_numpy(g["y"]), torch.from_numpy(g["t"]), g["eval_pts"]
    model.optimizer.zero_grad()
    y_pred = model(x, t[ev], n_samples=g["meta"]["n_samples"], training=True)
    loss, data, names = model.calc_loss(y_pred, y[:, ev, :], losses)
    loss.backward()
    monkeypatch.undo()
    grads = {f"{part}.{k}": p.grad.clone() for part in ("enc", "ode", "dec")
             for k, p in getattr(model, part).named_parameters()}
    return loss.detach(), data, names, grads, y_pred.detach(), y[:, ev, :]


def test_calc_loss_energy_term(pkg, monkeypatch):
    import lib.train_functions as tf
    g = load_golden("e2e_vae_step")
    base = dict(g["meta"]["losses"])
    assert base.get("nll", True) and "energy" not in base
    loss0, data0, names0, grads0, y_pred, y = _calc(g, base, monkeypatch)
    assert names0 == g["meta"]["loss_names"]

    # key absent or 0: names, the loss and every gradient bit for bit those of the unmodified call
    for off in (dict(base, energy=0), dict(base, energy=0.0, energy_fair=True, energy_block="series")):
        loss_z, data_z, names_z, grads_z, _, _ = _calc(g, off, monkeypatch)
        assert names_z == names0 and data_z == data0 and torch.equal(loss_z, loss0)
        assert all(torch.equal(grads_z[k], grads0[k]) for k in grads0)

    for block, fair in (("joint", False), ("series", True), ("field", False)):
        on = dict(base, energy=0.5, energy_fair=fair)
        if block != "joint":
            on["energy_block"] = block                                # "joint" is the default
        loss1, data1, names1, grads1, y_pred1, _ = _calc(g, on, monkeypatch)
        i = names0.index("nll")
        assert names1 == names0[:i + 1] + ["energy"] + names0[i + 1:]
        assert torch.equal(y_pred1, y_pred)
        term = 0.5 * tf.energy_loss(y_pred, y, block=block, fair=fair)
        assert data1[names1.index("energy")] == round(float(term), 3)
        # both totals are fp32 sums of the same terms in the same order with this one added between them: at
        # most one rounding (2^-24 relative) per addition, fewer than 8 additions each
        assert abs(float(loss1) - float(loss0) - float(term)) <= 16 * 2.0 ** -24 * abs(float(loss1))
        assert float(term) > 1e-3 * abs(float(loss1)) or float(term) > 1e-3
        assert any(not torch.equal(grads1[k], grads0[k]) for k in grads0)

    # right after crps when both are on
    _, _, names2, _, _, _ = _calc(g, dict(base, crps=0.5, energy=0.5), monkeypatch)
    i = names0.index("nll")
    assert names2 == names0[:i + 1] + ["crps", "energy"] + names0[i + 1:]


def test_calc_loss_energy_as_the_only_data_term(pkg, monkeypatch):
    g = load_golden("e2e_vae_step")
    losses = dict(g["meta"]["losses"], nll=False, energy=1.0)
    loss, data, names, grads, _, _ = _calc(g, losses, monkeypatch)
    assert "energy" in names and "nll" not in names
    assert np.isfinite(float(loss))
    for k, v in grads.items():
        assert v is not None and torch.isfinite(v).all(), k
    # the decoder sees the data through the energy term alone
    assert all(float(v.abs().max()) > 0 for k, v in grads.items() if k.startswith("dec."))


def test_calc_loss_bad_energy_block_raises(pkg, monkeypatch):
    g = load_golden("e2e_vae_step")
    with pytest.raises(ValueError):
        _calc(g, dict(g["meta"]["losses"], energy=1.0, energy_block="region"), monkeypatch)


def test_train_history_records_the_joint_energy_score_cpu(pkg, monkeypatch, tmp_path):
    """VAE.train(validate=...) with the energy term on records forecast_energy (forecast(joint=True)'s
    energy_joint_mean); without the term the history keys are unchanged."""
    from test_e2e_vae import _build
    monkeypatch.chdir(tmp_path)
    g = load_golden("e2e_vae_toy64")
    model = _build(None, g, "cpu")
    x, y, t = torch.from_numpy(g["x"]), torch.from_numpy(g["y"]), torch.from_numpy(g["t"])
    ev = [int(e) for e in g["eval_pts"]]
    torch.manual_seed(0)
    validate = {"x_test": x, "y_test": y, "t": t, "scaler": np.ones(y.shape[-1]), "n_samples": 4}

    def one_epoch(losses):
        model.train([(x, y)], t, 1, losses, ev, n_samples=g["meta"]["n_samples"], grad_lim=1e9, disable=True,
                    norm_file=str(tmp_path / "norms.txt"), validate=validate)
        return model._history.epoch_history[-1]
    h = one_epoch(dict(g["meta"]["losses"], energy=1.0))
    assert np.isfinite(h["forecast_energy"]) and h["forecast_energy"] > 0
    assert np.isfinite(h["forecast_nll"]) and "energy" in h and "forecast_crps" not in h
    h = one_epoch(dict(g["meta"]["losses"]))
    assert "forecast_energy" not in h and "forecast_nll" in h


# ---- C-ABI ------------------------------------------------------------------------------------------

def test_energy_cabi_is_declared_and_bound(pkg):
    from ude_amd import _native
    src = open(os.path.join(REPO, "include", "ude_rk4.h")).read()
    declared = set(re.findall(r"\b(ude_[a-z0-9_]+)\s*\(", src))
    for name in ("ude_energy_workspace", "ude_energy_forward", "ude_energy_backward"):
        assert name in declared and name in _native.EXPORTED_SYMBOLS, name
    assert _native._CABI["ude_energy_forward"][0] == "energy_forward"
    assert _native._CABI["ude_energy_backward"][0] == "energy_backward"
    assert hasattr(_native.NativeLib, "energy_workspace") and hasattr(_native.NativeLib, "energy_supported")
    # the block kinds are named once (train_functions.ENERGY_BLOCKS); their index is the header's integer
    import lib.train_functions as tf
    kinds = {n.lower(): int(v) for n, v in re.findall(r"#define UDE_ENERGY_([A-Z]+) (\d+)", src)}
    assert kinds == {name: i for i, name in enumerate(tf.ENERGY_BLOCKS)}
    from ude_amd import decoder_head
    assert not hasattr(decoder_head, "ENERGY_BLOCKS")


def test_energy_loss_keeps_no_chunk_for_the_backward(pkg, monkeypatch):
    """Under autograd a chunk's (n, ni, S, T, R) differences are formed again in the backward, not kept: the
    tensors saved between the forward and the backward stay below one chunk's size however many chunks there are."""
    import lib.train_functions as tf
    case = eh.make_case("partial_tiles")
    y = torch.tensor(case.y).double()
    chunk = case.S * case.S * case.T * case.R * 8            # one window's pairwise differences: three chunks
    monkeypatch.setattr(tf, "ENERGY_CHUNK_BYTES", chunk)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t.numel() * t.element_size()) or t,
                                                  lambda t: t):
        loss = tf.energy_loss(_y_pred(case), y, block="joint")
    assert max(saved) < chunk and sum(saved) < chunk, (max(saved), sum(saved), chunk)
    assert abs(float(loss.detach()) - eh.reference("partial_tiles", "joint", False).loss) <= 1e-13 * float(loss.detach())
