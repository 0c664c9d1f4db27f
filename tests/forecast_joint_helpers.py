"""Shared pieces of the ``joint=`` tests (test_forecast_joint.py, test_forecast_joint_gpu.py): the cases, a
brute-force NumPy reference written independently of the implementation (loops over the blocks,
``x[:, None] - x[None]`` for the sample pairs, a double loop over the coordinate pairs for the variogram) and
the comparison with the project's bar for fp64 summaries: 1e-10 normwise, and exactly 0 where the definitions
give 0 (the variogram score of a one-coordinate block; the pair term with one sample is checked on the
reference's own first term)."""
import functools

import numpy as np
import torch

from helpers import normwise_rel
import forecast_helpers
from forecast_helpers import same_bits, synth  # noqa: F401 (the tests import them here)

FIELDS = ("energy_joint", "energy_series", "energy_field", "variogram_series", "variogram_field",
          "energy_joint_mean", "energy_series_r", "energy_field_t", "variogram_series_r", "variogram_field_t")

# name -> ((T, S, B, R), (start, every), p); seed 100 + S as in the summary tests
CASES = {
    "odd_S": ((5, 5, 4, 1), (0, 1), 0.5),                # a partial pair tile
    "S17": ((3, 17, 2, 3), (0, 1), 0.5),                 # one full tile plus a one-row tile: both weightings
    "S33": ((2, 33, 1, 2), (0, 1), 0.5),                 # three tiles per side
    "S1": ((4, 1, 5, 2), (0, 1), 0.5),                   # ES = |x - y|; VS = (|dy|^p - |dx|^p)^2
    "S1024": ((2, 1024, 2, 3), (0, 1), 0.5),             # the largest S
    "BR147": ((4, 128, 3, 49), (0, 1), 0.5),             # R not a power of two, the state model's width
    "M1": ((3, 9, 3, 10), (2, 5), 0.5),                  # one considered time
    "weekly": ((29, 16, 3, 2), (6, 7), 0.5),             # every skipped time is 1e30, in y too, and must not show
    "R1": ((6, 16, 3, 1), (0, 1), 0.5),                  # the one-dimensional field block
    "ties": ((4, 64, 7, 10), (0, 1), 0.5),               # duplicated samples, and a target equal to a sample
    "p1": ((3, 17, 2, 3), (0, 1), 1.0),                  # S17 with the absolute-value branch
    "plain": ((3, 9, 3, 10), (0, 1), 0.5),               # no scale
    # beyond the issue's table: where the kernels take another path
    "R70": ((3, 5, 2, 70), (0, 1), 0.5),                 # more regions than a thread keeps series sums for
    "pairs2k": ((68, 3, 1, 2), (0, 1), 1.0),             # 2278 coordinate pairs: a second pass of the variogram threads
    "S200M57": ((57, 200, 1, 2), (0, 1), 0.5),           # a variogram block in two tiles of samples
}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(yhat, scale or None, y, S, B, (start, every), p)"""
    (T, S, B, R), (start, every), p = CASES[name]
    yhat, scale, y = synth(T, S, B, R, seed=100 + S, ties=name == "ties")
    if name == "S1":
        y[:, 1, :] += np.float32(0.25)                   # synth puts an S = 1 target on its sample
    if name == "weekly":
        skipped = np.ones(T, dtype=bool)
        skipped[start::every] = False
        yhat[skipped] = np.float32(1e30)
        y[:, skipped] = np.float32(1e30)
    if name == "ties":
        v = yhat.reshape(T, S, B, R)
        y[0] = v[:, 3, 0]                                # window 0's target is its sample 3, at every time and region
    if name == "plain":
        scale = None
    return yhat, scale, y, S, B, (start, every), p


def energy(x, y):
    """x (S, D) samples, y (D,): (the score, its first term)"""
    S = x.shape[0]
    first = np.sqrt(((x - y) ** 2).sum(1)).sum() / S
    pairs = np.sqrt(((x[:, None] - x[None]) ** 2).sum(2)).sum()
    return first - pairs / (2.0 * S * S), first


def variogram(x, y, p):
    """x (S, D), y (D,): the unweighted variogram score of order p, a double loop over the coordinate pairs"""
    total = 0.0
    for c in range(x.shape[1]):
        for c2 in range(c + 1, x.shape[1]):
            total += (abs(y[c] - y[c2]) ** p - (np.abs(x[:, c] - x[:, c2]) ** p).mean()) ** 2
    return total


def reference(yhat, S, B, opts, p, scale, y_true):
    start, every = opts
    T, N, R = yhat.shape
    sc = np.ones(R) if scale is None else np.asarray(scale, dtype=np.float64)
    idx = np.arange(start, T, every)
    M = len(idx)
    v = yhat.astype(np.float64).reshape(T, S, B, R)[idx] * sc                   # (M, S, B, R)
    y = y_true.astype(np.float64).transpose(1, 0, 2)[idx] * sc                  # (M, B, R)
    out = {"M": M, "energy_joint": np.empty(B), "energy_series": np.empty((B, R)), "energy_field": np.empty((B, M)),
           "variogram_series": np.empty((B, R)), "variogram_field": np.empty((B, M))}
    ratio = []
    for b in range(B):
        x = v[:, :, b].transpose(1, 0, 2)                                       # (S, M, R)
        out["energy_joint"][b], first = energy(x.reshape(S, M * R), y[:, b].reshape(M * R))
        ratio.append(out["energy_joint"][b] / first)
        for r in range(R):
            out["energy_series"][b, r] = energy(x[:, :, r], y[:, b, r])[0]
            out["variogram_series"][b, r] = variogram(x[:, :, r], y[:, b, r], p)
        for m in range(M):
            out["energy_field"][b, m] = energy(x[:, m], y[m, b])[0]
            out["variogram_field"][b, m] = variogram(x[:, m], y[m, b], p)
    out["joint_over_first"] = min(ratio)
    out["energy_joint_mean"] = out["energy_joint"].mean()
    out["energy_series_r"], out["energy_field_t"] = out["energy_series"].mean(0), out["energy_field"].mean(0)
    out["variogram_series_r"], out["variogram_field_t"] = out["variogram_series"].mean(0), out["variogram_field"].mean(0)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(name):
    yhat, scale, y, S, B, opts, p = case_inputs(name)
    return reference(yhat, S, B, opts, p, scale, y)


def check(js, ref, label=""):
    """``js``: a JointScores.  Every field fp64, of the table's shape, within 1e-10 normwise; a quantity the
    reference has as exactly 0 is exactly 0."""
    got = js.numpy()
    assert set(got) == set(FIELDS)
    errs = {}
    for k in FIELDS:
        assert got[k].dtype == np.float64 and got[k].shape == np.shape(ref[k]), (k, got[k].shape, np.shape(ref[k]))
        if not np.any(ref[k]):
            assert not np.any(got[k]), (k, got[k])
            continue
        errs[k] = normwise_rel(got[k], ref[k])
    print(label, {k: f"{e:.2e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e <= 1e-10, (k, e)


def joint_of(name):
    from ude_amd.forecast import Joint
    _, _, _, _, _, (start, every), p = case_inputs(name)
    return Joint(start=start, every=every, p=p)


def scores(name, device="cpu"):
    """ensemble_joint on a case's inputs."""
    from ude_amd.forecast import ensemble_joint
    yhat, scale, y, S, B, _, _ = case_inputs(name)
    return ensemble_joint(torch.from_numpy(yhat).to(device), S, B, torch.from_numpy(y).to(device), joint_of(name),
                          scale=scale)


def one_sample(js):
    """The field norm is the root of a sum of two squares, which has one order: the same bits.  The series norm
    sums four: within two roundings."""
    yhat, scale, y, S, B, _, _ = case_inputs("S1")
    x = torch.from_numpy(yhat).double().reshape(4, 5, 2) * torch.from_numpy(scale)
    t = torch.from_numpy(y).double().permute(1, 0, 2) * torch.from_numpy(scale)
    assert torch.equal(js.energy_field.cpu(), ((x - t) ** 2).sum(2).sqrt().t())
    series = ((x - t) ** 2).sum(0).sqrt()
    assert bool(((js.energy_series.cpu() - series).abs() <= 4.5e-16 * series).all())


def identities(ensemble_joint, Joint, device):
    """R = M = 1: the three energies coincide; and the joint energy dominates every block's."""
    yhat, scale, y = synth(3, 12, 4, 1, seed=7)
    js = ensemble_joint(torch.from_numpy(yhat).to(device), 12, 4, torch.from_numpy(y).to(device), Joint(start=2),
                        scale=scale)
    assert normwise_rel(js.energy_series[:, 0], js.energy_joint) <= 1e-10
    assert normwise_rel(js.energy_field[:, 0], js.energy_joint) <= 1e-10
    for name in ("S17", "BR147", "weekly"):
        yhat, scale, y, S, B, (start, every), p = case_inputs(name)
        js = ensemble_joint(torch.from_numpy(yhat).to(device), S, B, torch.from_numpy(y).to(device),
                            Joint(start, every, p), scale=scale)
        below = torch.maximum(js.energy_field.amax(1), js.energy_series.amax(1))
        assert bool((js.energy_joint >= below * (1 - 1e-12)).all()), name      # a root at the wrong level fails this


def passthrough(g, device, monkeypatch, joint):
    """VAE.forecast(..., joint=joint): (the y_hat it hands to ensemble_summary, the Forecast)."""
    return forecast_helpers.passthrough(g, device, monkeypatch, joint=joint)
