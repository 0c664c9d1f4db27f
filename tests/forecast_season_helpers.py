"""Shared pieces of the ``season=`` tests (test_forecast_season.py, test_forecast_season_gpu.py): the
cases, a brute-force NumPy reference written independently of the implementation (a loop over the
samples, numpy.argmax, a direct test of every run for the onset, CRPS over all pairs, numpy.quantile)
and the comparison with the project's bars (forecast_verify_helpers.check's: continuous quantities
1e-10 normwise with skills by their logs, everything derived from a count exactly -- and the quantiles
of the peaks exactly: a maximum is exact and the quantile is numpy's _lerp)."""
import functools

import numpy as np
import torch

from helpers import normwise_rel
import forecast_helpers
from forecast_helpers import LEVELS, MASS_FLOOR, same_bits, synth  # noqa: F401 (the tests import them here)

CONTINUOUS = ("peak_mean", "peak_std", "total_mean", "total_std", "total_quantiles", "peak_crps", "total_crps",
              "peak_crps_r", "total_crps_r")
LOGS = ("peak_time_skill", "onset_skill", "peak_value_skill", "peak_time_skill_r", "onset_skill_r",
        "peak_value_skill_r")
EXACT = ("peak_quantiles", "peak_time", "onset")
SCORES = ("peak_time_skill", "onset_skill", "peak_value_skill", "peak_crps", "total_crps")
FIELDS = CONTINUOUS + LOGS + EXACT

# name -> ((T, S, B, R), (start, every, run, window)); seed 100 + S as in the summary tests
CASES = {
    "odd_S": ((5, 5, 4, 1), (0, 1, 2, 1)),               # padding rows, fewer groups than a wave
    "BR147": ((4, 128, 3, 49), (0, 1, 3, 1)),            # dead columns in the last workgroup
    "S1024": ((3, 1024, 2, 3), (0, 1, 1, 0)),            # the largest S, the narrowest G
    "S1": ((4, 1, 5, 2), (0, 1, 2, 1)),                  # probabilities 0 / 1, std 0, CRPS = |peak - y*|
    "M1": ((3, 9, 3, 10), (2, 5, 1, 0)),                 # one considered time
    "M1_run2": ((3, 9, 3, 10), (2, 5, 2, 0)),            # run > M: onset[:, M] = 1
    "weekly": ((29, 16, 3, 2), (6, 7, 2, 1)),            # M = 4; every skipped time is 1e30 and must not show
    "nbx69": ((3, 2, 90, 49), (0, 1, 1, 1)),             # more than 64 workgroups in the overall reduce
    "ties": ((4, 64, 7, 10), (0, 1, 2, 1)),              # a repeated peak; samples and a target on the baseline
    "edges": ((6, 16, 3, 2), (0, 1, 2, 2)),              # m* = 0 and m* = M - 1; a target above every peak
    "far": ((6, 16, 3, 2), (0, 1, 2, 2)),                # a baseline above everything: no onset, observed none
    "plain": ((3, 9, 3, 10), (0, 1, 3, 1)),              # no scale, no baseline, no targets
}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(yhat, scale or None, y or None, S, B, baseline (R,) or None, (start, every, run, window))"""
    (T, S, B, R), opts = CASES[name]
    yhat, scale, y = synth(T, S, B, R, seed=100 + S)
    base = 2.0 * scale                                   # the middle of synth's group means, scaled
    v = yhat.reshape(T, S, B, R)
    if name == "S1":
        y[:, 1, :] += np.float32(0.25)                   # synth puts an S = 1 target on its sample
    if name == "weekly":
        skipped = np.ones(T, dtype=bool)
        skipped[opts[0]::opts[1]] = False
        yhat[skipped] = np.float32(1e30)
        y[:, skipped] = np.float32(1e30)
    if name == "ties":
        for r in range(R):
            base[r] = float(v[1, 0, 0, r]) * scale[r]    # sample 0 of window 0 at t = 1 sits on the baseline
            v[2, 1, 1, r] = v[1, 0, 0, r]                # and so does another sample of another window
        first = v[:-1].argmax(0)                         # where the peak of t < T - 1 falls
        v[-1] = np.take_along_axis(v[:-1], first[None], 0)[0]       # the last time copies it: the first wins
        y[0, 1, 0] = v[1, 0, 0, 0]                       # and the target of group (0, 0) at t = 1
    if name == "edges":
        y[0, 0, 0] = np.float32(50.0)                    # m* = 0, above every sample's peak: an empty value window
        y[1, T - 1, 0] = np.float32(9.0)                 # m* = M - 1
        y[2, 0, 1] = np.float32(1e3)
    if name == "far":
        base = np.full(R, 1e6)
    if name == "plain":
        return yhat, None, None, S, B, None, opts
    return yhat, scale, y, S, B, base, opts


def walk(series, base, run):
    """One trajectory (M,) or a block (M, ...) of them with base broadcastable: peak, when, total, onset."""
    M = series.shape[0]
    peak, when = series.max(0), np.argmax(series, axis=0)
    total = np.zeros_like(series[0])
    for m in range(M):
        total = total + series[m]
    onset = None
    if base is not None:
        onset = np.full(series.shape[1:], M, dtype=np.int64)
        for m in range(M - run, -1, -1):                 # descending: the smallest m that qualifies stays
            ok = np.ones(series.shape[1:], dtype=bool)
            for k in range(run):
                ok &= series[m + k] >= base
            onset[ok] = m
    return peak, when, total, onset


def crps_pairs(x, y):
    """mean |x - y| - mean |x - x'| / 2 over all pairs; x (S, B, R), y (B, R)"""
    first = np.abs(x - y).mean(0)
    pairs = np.abs(x[:, None] - x[None, :]).mean((0, 1))
    out = first - 0.5 * pairs
    assert (out >= -1e-12 * first).all()
    return out


def reference(yhat, S, B, opts, scale=None, y_true=None, base=None, q=LEVELS):
    start, every, run, window = opts
    T, N, R = yhat.shape
    sc = np.ones(R) if scale is None else np.asarray(scale, dtype=np.float64)
    idx = np.arange(start, T, every)
    M = len(idx)
    v = yhat.astype(np.float64).reshape(T, S, B, R)[idx] * sc                   # (M, S, B, R)
    peak, total = np.empty((S, B, R)), np.empty((S, B, R))
    when = np.empty((S, B, R), dtype=np.int64)
    onset = None if base is None else np.empty((S, B, R), dtype=np.int64)
    for s in range(S):
        p, w, t, o = walk(v[:, s], base, run)
        peak[s], when[s], total[s] = p, w, t
        if base is not None:
            onset[s] = o
    out = {"M": M, "peak_mean": peak.mean(0), "peak_std": peak.std(0), "total_mean": total.mean(0),
           "total_std": total.std(0), "peak_quantiles": np.quantile(peak, q, axis=0),
           "total_quantiles": np.quantile(total, q, axis=0),
           "peak_time": np.stack([(when == m).sum(0) for m in range(M)], 1) / S,
           "onset": None if base is None else np.stack([(onset == m).sum(0) for m in range(M + 1)], 1) / S,
           "distinct_when": float(np.mean([len(np.unique(when[:, b, r])) for b in range(B) for r in range(R)])),
           "no_onset": None if base is None else float((onset == M).mean())}
    if base is not None:
        out["distinct_onset"] = float(np.mean([len(np.unique(onset[:, b, r])) for b in range(B) for r in range(R)]))
    if y_true is None:
        return out
    y = y_true.astype(np.float64).transpose(1, 0, 2)[idx] * sc                  # (M, B, R)
    y_peak, y_when, y_total, y_onset = walk(y, base, run)
    logs = np.zeros((3, B, R))
    for b in range(B):
        for r in range(R):
            lo, hi = max(0, y_when[b, r] - window), min(M - 1, y_when[b, r] + window)
            P = out["peak_time"][b, lo:hi + 1, r].sum()
            logs[0, b, r] = np.log(MASS_FLOOR if P == 0 else P)
            if base is not None:
                o = y_onset[b, r]
                P = out["onset"][b, M, r] if o == M else out["onset"][b, max(0, o - window):min(M - 1, o + window) + 1, r].sum()
                logs[1, b, r] = np.log(MASS_FLOOR if P == 0 else P)
            c = np.floor(10 * y_peak[b, r]) / 10
            n = ((peak[:, b, r] >= c - 0.5) & (peak[:, b, r] < c + 0.6)).sum()
            logs[2, b, r] = np.log(MASS_FLOOR if n == 0 else n / S)
    terms = {"peak_time_skill": logs[0], "onset_skill": logs[1] if base is not None else None,
             "peak_value_skill": logs[2], "peak_crps": crps_pairs(peak, y_peak), "total_crps": crps_pairs(total, y_total)}
    for k, t in terms.items():                                                  # skills are kept as their logs
        out[k] = None if t is None else t.mean()
        out[k + "_r"] = None if t is None else t.mean(0)
    out.update(y_when=y_when, y_onset=y_onset, empty_value_windows=int((logs[2] == np.log(MASS_FLOOR)).sum()))
    return out


@functools.lru_cache(maxsize=None)
def case_reference(name):
    yhat, scale, y, S, B, base, opts = case_inputs(name)
    return reference(yhat, S, B, opts, scale, y, base)


def check(st, ref, label=""):
    """``st``: a SeasonTargets.  Continuous quantities (skills by their logs) within 1e-10 normwise, what
    derives from counts and the quantiles of the peaks exactly; a field the reference has as None is None."""
    got = st.numpy()
    errs, same = {}, {}
    for k in FIELDS:
        if ref.get(k) is None:
            assert got[k] is None, k
            continue
        assert got[k] is not None and got[k].dtype == np.float64 and got[k].shape == np.shape(ref[k]), k
        if k in EXACT:
            same[k] = bool(np.array_equal(got[k], ref[k]))
        else:
            errs[k] = normwise_rel(np.log(got[k]) if k in LOGS else got[k], ref[k])
    print(label, {k: f"{e:.2e}" for k, e in errs.items()}, same)
    for k, e in errs.items():
        assert e <= 1e-10, (k, e)
    for k, ok in same.items():
        assert ok, (k, got[k], ref[k])


def season_of(name):
    from ude_amd.forecast import Season
    _, _, _, _, _, base, (start, every, run, window) = case_inputs(name)
    return Season(baseline=None if base is None else tuple(base), start=start, every=every, run=run, window=window)


def targets(name, device="cpu"):
    """ensemble_season on a case's inputs."""
    from ude_amd.forecast import ensemble_season
    yhat, scale, y, S, B, _, _ = case_inputs(name)
    return ensemble_season(torch.from_numpy(yhat).to(device), S, B, season_of(name),
                           y_true=None if y is None else torch.from_numpy(y).to(device), scale=scale, quantiles=LEVELS)


def golden_baseline(g):
    """Per region, the median of the scaled targets."""
    return np.median(g["y_test"].astype(np.float64) * np.asarray(g["scaler"], dtype=np.float64), axis=(0, 1))


def passthrough(g, device, monkeypatch, season):
    """VAE.forecast(..., season=season): (the y_hat it hands to ensemble_summary, the Forecast)."""
    return forecast_helpers.passthrough(g, device, monkeypatch, season=season)
