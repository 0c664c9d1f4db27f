"""Shared pieces of the ``aggregate=`` tests (test_forecast_aggregate.py, test_forecast_aggregate_gpu.py): the
cases, and a brute-force NumPy reference that restates the definitions of ude_forecast_aggregate and
ude_forecast_aggregate_dyn (include/ude_rk4.h) with an explicit Python loop over the regions on ``np.float64``
arrays and a final ``np.float32`` -- every product and every sum is one NumPy operation, rounded on its own, r
ascending.  It imports nothing of ``ude_amd``.  The order of operations is pinned, so every comparison is bit
for bit (``same_f32``; a NaN equals a NaN)."""
import functools
from dataclasses import fields

import numpy as np
import torch

import forecast_helpers
from forecast_helpers import same_bits

STATE = ("s", "i", "r")
RATES = ("beta", "gamma", "r_eff")
FLUX = ("fa_s", "fa_i", "fa_r")
KINDS = {"Fp": STATE + RATES, "Fa": STATE + FLUX, "FaFp": STATE + RATES + FLUX}      # C = 6, 6, 9
KIND_CODE = {"Fp": 1, "Fa": 2, "FaFp": 3}

# The kernels (csrc/ude_aggregate.h) own tiles of 64 rows, walk the regions in chunks of 63 (prediction) or 15
# (the rate planes of the dynamics), give each of four waves ceil(G / 4) stacked rows in 4, 16 or 64 accumulators,
# stage the outputs 124 stacked rows at a time and take at most 65536 workgroups per launch.
# name -> (leading shape, R, the levels' group counts, with scale)
CASES = {
    "one": ((1,), 1, (1,), False),                       # rows = 1, R = 1, G = 1
    "state": ((3, 15), 49, (10, 1), True),               # T 3, S 5, B 3: 45 rows, a partial tile; levels 10 + 1
    "R70": ((130,), 70, (3,), True),                     # two tiles and a remainder; R even, above 64: two chunks
    "offsets": ((2, 5), 7, (1, 2, 1), False),            # three levels: the block offsets
    "G256": ((7,), 5, (256,), True),                     # the largest hierarchy: 64 accumulators, three staging rounds
    "split": ((7,), 5, (120, 10, 126), False),           # levels that straddle the staging rounds
    "R4096": ((3,), 4096, (2,), True),                   # the largest R: 66 chunks
    "R63": ((70,), 63, (5,), True),                      # R at the chunk width
    "R64": ((70,), 64, (5,), True),                      # and one above it
    "G40": ((66,), 9, (17, 23), True),                   # 16 accumulators
    "levels16": ((5,), 3, (1,) * 16, False),             # the most levels
    "stride": ((64 * 65536 + 70,), 1, (1,), True),       # more tiles than workgroups
}
# the dynamics, each with all three kinds: name -> (T, N, R, the levels' group counts)
DYN_CASES = {
    "one": (1, 1, 1, (1,)),
    "state": (3, 15, 49, (10, 1)),                       # four chunks of the rate planes
    "R70": (2, 65, 70, (3,)),
    "R15": (2, 35, 15, (5,)),                            # R at the rate planes' chunk width
    "R16": (2, 35, 16, (5,)),                            # and one above it
    "G70": (1, 9, 5, (40, 30)),                          # more than 64 stacked rows: two passes of the rate planes
    "G256": (1, 3, 4, (130, 126)),
}


def values(shape, seed):
    """fp32, magnitudes 1e-3 .. 1e3 of both signs, one in twenty exactly zero: no NaN, no denormal"""
    rng = np.random.default_rng(seed)
    v = 10.0 ** rng.uniform(-3.0, 3.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    v[rng.random(size=shape) < 0.05] = 0.0
    return v.astype(np.float32)


def weights(sizes, R, seed, signed=True):
    """One (G_l, R) fp64 matrix per level: a third of the entries exactly zero, the rest in (0, 2) or (-2, 2)."""
    rng = np.random.default_rng(seed)
    out = []
    for G in sizes:
        w = rng.uniform(-2.0 if signed else 0.0, 2.0, size=(G, R))
        w[rng.random(size=(G, R)) < 1.0 / 3.0] = 0.0
        out.append(w)
    return out


def stacked(ws):
    return np.concatenate(ws), np.cumsum([0] + [w.shape[0] for w in ws]).tolist()


def weighted_sums(v, w):
    """v (rows, R) fp64, w (G, R) fp64 -> (rows, G) fp64: acc = 0, acc = acc + w[g, r] * v_r, r ascending"""
    acc = np.zeros((v.shape[0], w.shape[0]), dtype=np.float64)
    for r in range(v.shape[1]):
        acc = acc + w[None, :, r] * v[:, r, None]
    return acc


def reference(x, ws, scale):
    """x (..., R) fp32, ws the levels' matrices, scale (R,) or None -> one fp32 (..., G_l) array per level"""
    R = x.shape[-1]
    v = x.reshape(-1, R).astype(np.float64)
    if scale is not None:
        v = v * np.asarray(scale, dtype=np.float64)
    return [weighted_sums(v, w).astype(np.float32).reshape(x.shape[:-1] + (w.shape[0],)) for w in ws]


def reference_dyn(dyn, names, ws):
    """dyn (C, T, N, R) fp32 -> one fp32 (C, T, N, G_l) array per level; the r_eff channel is not read"""
    C, T, N, R = dyn.shape
    v = {n: dyn[c].reshape(-1, R).astype(np.float64) for c, n in enumerate(names) if n != "r_eff"}
    out = []
    for w in ws:
        ch = {n: weighted_sums(v[n], w) for n in names if n in STATE + FLUX}
        if "beta" in names:
            inc = weighted_sums((v["beta"] * v["s"]) * v["i"], w)
            rec = weighted_sums(v["gamma"] * v["i"], w)
            with np.errstate(divide="ignore", invalid="ignore"):
                ch["beta"], ch["gamma"], ch["r_eff"] = inc / (ch["s"] * ch["i"]), rec / ch["i"], inc / rec
        out.append(np.stack([ch[n].astype(np.float32) for n in names]).reshape(C, T, N, w.shape[0]))
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, the levels' matrices, scale or None, the reference's arrays)"""
    lead, R, sizes, with_scale = CASES[name]
    seed = 1000 + sum(map(ord, name))
    x = values(lead + (R,), seed)
    ws = weights(sizes, R, seed + 1)
    if name == "state":
        ws = state_levels(R, seed + 1)
    scale = np.random.default_rng(seed + 2).uniform(0.5, 4.0, size=R) if with_scale else None
    ref = reference(x, ws, scale)
    for a in (x, *ws, *ref):
        a.setflags(write=False)
    return x, ws, scale, ref


def state_levels(R, seed):
    """Ten groups that partition the R regions, weighted by share, and the whole: the HHS regions and the nation.
    Written out here, not taken from Aggregate.from_groups."""
    rng = np.random.default_rng(seed)
    share = rng.uniform(0.5, 40.0, size=R)
    member = rng.permutation(np.arange(R) % 10)
    hhs = np.zeros((10, R))
    for g in range(10):
        idx = np.flatnonzero(member == g)
        hhs[g, idx] = share[idx] / share[idx].sum()
    return [hhs, (share / share.sum())[None, :]]


@functools.lru_cache(maxsize=None)
def dyn_case(name, kind):
    """(dyn (C, T, N, R), names, the levels' matrices, the reference's arrays).  s, i, r, beta, gamma > 0 and
    weights >= 0, so the reference has no non-finite ratio but in the one row of the first case of each kind where
    i = 0 across a whole group (every region the group weighs): there beta, gamma and r_eff are 0 / 0."""
    T, N, R, sizes = DYN_CASES[name]
    names = KINDS[kind]
    seed = 2000 + sum(map(ord, name + kind))
    dyn = values((len(names), T, N, R), seed)
    for c, n in enumerate(names):
        if n in STATE + RATES:
            dyn[c] = np.abs(dyn[c]) + np.float32(1e-3)
    ws = state_levels(R, seed + 1) if name == "state" else weights(sizes, R, seed + 1, signed=False)
    for w in ws:                                         # no group without a region
        w[np.arange(w.shape[0]), np.arange(w.shape[0]) % R] += 0.5
    if name == "state":
        dyn[1, 0, 0, ws[0][0] != 0] = 0.0                # i = 0 in every region of the first group, at row 0
    ref = reference_dyn(dyn, names, ws)
    if name == "state" and "beta" in names:
        assert np.isnan(ref[0][3:6, 0, 0, 0]).all() and np.isfinite(ref[0][:, 1:]).all() and np.isfinite(ref[1]).all()
    else:
        assert all(np.isfinite(r).all() for r in ref)
    for a in (dyn, *ws, *ref):
        a.setflags(write=False)
    return dyn, names, ws, ref


def same_f32(a, b):
    """fp32 arrays of one shape with the same bits; a NaN equals a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float32 or b.dtype != np.float32 or a.shape != b.shape:
        return False
    return bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


def levels_of(ws):
    from ude_amd.forecast import Aggregate
    return {f"level{l}": Aggregate(w) for l, w in enumerate(ws)}


def aggregate(name, device="cpu"):
    """ensemble_aggregate on a case's inputs: the list of the levels' tensors"""
    from ude_amd.forecast import ensemble_aggregate
    x, ws, scale, _ = case(name)
    out = ensemble_aggregate(torch.tensor(x, device=device), levels_of(ws), scale=scale)
    assert list(out) == [f"level{l}" for l in range(len(ws))]
    return list(out.values())


def aggregate_dyn(name, kind, device="cpu"):
    from ude_amd.forecast import aggregate_dynamics
    dyn, names, ws, _ = dyn_case(name, kind)
    out = aggregate_dynamics(torch.tensor(dyn, device=device), names, levels_of(ws))
    assert all(v[1] == names for v in out.values())
    return [v[0] for v in out.values()]


def check(got, ref, label=""):
    assert len(got) == len(ref)
    for l, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == torch.float32 and tuple(a.shape) == b.shape, (label, l, a.dtype, tuple(a.shape), b.shape)
        a = a.cpu().numpy()
        bad = ~((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b)))
        assert not bad.any(), (label, l, int(bad.sum()), a[bad][:4], b[bad][:4])


# ---- VAE.forecast(aggregate=...) end to end ----

FORECAST_CASES = ["e2e_forecast_us", "e2e_forecast_state49"]


def forecast_levels(R):
    """name -> (weights, baseline): 49 regions as 10 groups and the nation; one region as itself, doubled"""
    if R == 1:
        return {"double": (np.array([[2.0]]), 1.5)}
    hhs, nation = state_levels(R, 7)
    return {"hhs": (hhs, tuple(np.linspace(0.8, 2.0, 10))), "nation": (nation, None)}


def forecast_options():
    from ude_amd.forecast import Joint, Season
    return dict(verify=True, dynamics=True, season=Season(baseline=1.2, start=1, every=7, run=2),
                joint=Joint(start=1, every=7))


def spied_forecast(g, device, monkeypatch, **kw):
    """VAE.forecast(..., **kw): (what the baseline handed on -- the ``yhat`` of the first ensemble_summary call
    and the ``dyn`` (C, T, N, R) of the first dynamics_summary call, as host arrays, with ``S`` and ``B`` --, the
    Forecast)."""
    from ude_amd import forecast as fmod
    seen = {}
    inner_summary, inner_dyn = fmod.ensemble_summary, fmod.dynamics_summary

    def spy_summary(yhat, n_samples, batch, **k):
        if "yhat" not in seen and yhat.dim() == 3 and not seen.get("in_dyn"):
            seen.update(yhat=yhat.detach().float().cpu().numpy(), S=n_samples, B=batch)
        return inner_summary(yhat, n_samples, batch, **k)

    def spy_dyn(dyn, names, n_samples, batch, **k):
        if "dyn" not in seen:
            seen.update(dyn=dyn.detach().float().cpu().numpy(), names=tuple(names))
        seen["in_dyn"] = True
        try:
            return inner_dyn(dyn, names, n_samples, batch, **k)
        finally:
            seen["in_dyn"] = False

    monkeypatch.setattr(fmod, "ensemble_summary", spy_summary)
    monkeypatch.setattr(fmod, "dynamics_summary", spy_dyn)
    _, fc = forecast_helpers.run_forecast(g, device, monkeypatch, **kw)
    return seen, fc


def expected_level(g, seen, w, baseline, device, opts, scaled=True):
    """The existing ensemble_* functions on the REFERENCE's aggregated arrays: the Forecast a level must equal."""
    from ude_amd.forecast import (Season, dynamics_summary, ensemble_joint, ensemble_season, ensemble_summary)
    S, B = seen["S"], seen["B"]
    scale = g["scaler"] if scaled else None
    to = lambda a: torch.from_numpy(a).to(device)
    yh = to(reference(seen["yhat"], [w], scale)[0])
    yt = to(reference(g["y_test"].astype(np.float32), [w], scale)[0])
    q = g["meta"]["quantiles"]
    fc = ensemble_summary(yh, S, B, y_true=yt, quantiles=q, verify=opts.get("verify"))
    if opts.get("dynamics"):
        fc.dynamics = dynamics_summary(to(reference_dyn(seen["dyn"], seen["names"], [w])[0]), seen["names"], S, B,
                                       quantiles=q)
    if opts.get("season") is not None:
        s = opts["season"]
        fc.season = ensemble_season(yh, S, B, Season(baseline, s.start, s.every, s.run, s.window), y_true=yt,
                                    quantiles=q)
    if opts.get("joint") is not None:
        fc.joint = ensemble_joint(yh, S, B, yt, opts["joint"])
    return fc


def same_container(a, b, label=""):
    """Two result containers with the same fields, every tensor with the same bits."""
    assert type(a) is type(b), (label, type(a), type(b))
    for f in fields(a):
        u, v = getattr(a, f.name), getattr(b, f.name)
        if isinstance(u, torch.Tensor) or isinstance(v, torch.Tensor):
            assert same_bits(u, v), (label, f.name)
        elif hasattr(u, "_tensors") or hasattr(v, "_tensors"):
            same_container(u, v, f"{label}.{f.name}")
        else:
            assert u == v, (label, f.name, u, v)
