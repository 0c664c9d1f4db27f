"""Time the forecast of the reference's test shape on the device: the host-scored path against the
fused forecast.

State model (R = 49, L = 8, FaFp [64, 64, 32] / [64, 64]), S = 128 samples of B = 64 windows
(N = 8192 trajectories), t = arange(57) / 7 (run_ode.py's utils.test call).  After 5 warm-ups, 10
runs each, wall clock between device synchronisations:

  (a) host: model(x, t, 128, training=False) -> host copy -> NumPy mean / std -> Metrics.nll / skill
      at the four horizons (lib/utils.py:21-26, :53-54);
  (b) fused: model.forecast(x, t, 128, y_true, scaler).cpu();
  (c) fused + quantiles: (b) with quantiles=[0.025, 0.5, 0.975] -- the summary kernel sorts its tile;
  (d) fused + verify: (b) with verify=True -- the ensemble's own scores from the sorted tile
      (ude_forecast_verify in place of ude_forecast_summary).  (b), (c) and (d) alternate run by run,
      so their summary times come from the same minutes of the device.

``--dynamics`` times the forecast's dynamics (S, I, R, beta, gamma, R_eff, Fa per day) instead, three
paths taking turns:

  (a) latent route: model(x, t, 128, training=False) (the plain inference solve writes the latent), one
      evaluation-kernel call per output time on latent[j] (ude_amd.eval_rhs.rhs_eval), the channels stacked
      by torch operators, then the two summaries and their host copies;
  (b) fused: model.forecast(x, t, 128, y_true, scaler, dynamics=True).cpu();
  (c) the forecast without dynamics, (b) of the default mode, for the solve kernel's time without DYN.

``--season`` times the seasonal targets (weekly points of the daily grid: start 6, every 7, a baseline per
region, targets given) of one y_hat (57, 8192, 49) resident on the device, two routes taking turns:

  (a) host: a device-to-host copy of y_hat, then NumPy forming the same quantities over the trajectories
      (peak, peak week, total, onset per sample; mean / std / histograms per group; the log scores and the
      sorted-sample CRPS against the observed season);
  (b) device: ude_amd.forecast.ensemble_season(...).cpu() -- ude_forecast_season and one stacked copy of
      its results.

``--scenario`` times the solve kernel under a scenario (ude_rk4_forecast_scn) against the solves without one,
on one draw z (8192, 49, 8) resident on the device, five calls taking turns: ``forecast_dec``; ``forecast_scn``
with a table of ones; ``forecast_scn`` with a table in which every (step, region) differs; ``forecast_dyn``;
``forecast_scn`` with the dynamics channels.  The figure to read is each call's own event time
(``native_calls_ms``).  On a tree without scenarios only the two solves it has are timed (the yardstick of
the commit before).

``--joint`` times the joint scores (energy and variogram scores on the series, field and joint blocks) of one
y_hat (57, 8192, 49) resident on the device, weekly (start 6, every 7) and daily (start 0, every 1), three routes
taking turns per grid:

  (a) device: ude_amd.forecast.ensemble_joint(...).cpu() -- ude_forecast_joint and one stacked copy;
  (b) torch on the device: the torch fp64 definitions of the CPU route on the same device tensor;
  (c) host: a device-to-host copy of y_hat, then the torch fp64 definitions on the host.

``--aggregate`` times the aggregation to 10 groups and the nation (shares of a seeded population; G_tot = 11) of
one y_hat (57, 8192, 49) and one 9-channel dyn (9, 57, 8192, 49) resident on the device, three routes taking
turns, each for the prediction and for the dynamics:

  (a) device: ude_amd.forecast.ensemble_aggregate / aggregate_dynamics -- one native call each (its own event
      time under ``native_calls_ms``), the results left on the device;
  (b) torch on the device: fp64 ``einsum`` on the same device tensors (another order of operations: it agrees to
      rounding, not to the bit);
  (c) host: a device-to-host copy, then NumPy fp64 ``einsum``.

and ``model.forecast(..., aggregate=levels)`` against the same call without it.

Per path: min / median / max of the wall clock, the span between a device event recorded before the
call and one after its last device operation, and the sum of the gfx950 C-ABI calls' own event times
(ude_amd.fused.EVENTS).  Prints one JSON line.

    python tools/forecast_timing.py [--runs 10] [--warmup 5] [--batch 64] [--samples 128]
                                    [--dynamics | --season | --scenario | --joint | --aggregate]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
importlib.import_module("forecasting-influenza-using-universal-differential-equations_amd")

import lib.Metrics as Metrics  # noqa: E402
import lib.VAE as vae_mod  # noqa: E402
import lib.models as models  # noqa: E402
from ude_amd import fused  # noqa: E402


def stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def timed(fn, runs, warmup):
    return timed_alternating([fn], runs, warmup)[0]


def timed_alternating(fns, runs, warmup):
    """One result per function; the functions take turns, run by run."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    acc = [([], [], []) for _ in fns]
    for i in range(runs * len(fns)):
        fn = fns[i % len(fns)]
        wall, span, kern = acc[i % len(fns)]
        fused.EVENTS = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn(e1)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        span.append(e0.elapsed_time(e1))
        per = {}
        for kind, a, b in fused.EVENTS:
            per[kind] = per.get(kind, 0.0) + a.elapsed_time(b)
        kern.append(per)
        fused.EVENTS = None
    return [{"wall_ms": stats(wall), "device_span_ms": stats(span),
             "native_calls_ms": {kind: stats([k[kind] for k in kern]) for kind in kern[0]}} for wall, span, kern in acc]


def _draw(model, x, S, B, R):
    """One draw z (S * B, R, L) of the forecast, as VAE.forecast forms it."""
    mean, std = model.enc(x)
    eps = torch.randn(S, B, R, model.ld_enc, device="cuda")
    return (models.reparam(eps, std, mean, S, B, uncertainty=True) + 1e-5).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--dynamics", action="store_true", help="time the dynamics paths instead (see the docstring)")
    ap.add_argument("--season", action="store_true", help="time the seasonal targets instead (see the docstring)")
    ap.add_argument("--scenario", action="store_true", help="time the scenario solve instead (see the docstring)")
    ap.add_argument("--joint", action="store_true", help="time the joint scores instead (see the docstring)")
    ap.add_argument("--aggregate", action="store_true", help="time the aggregation instead (see the docstring)")
    a = ap.parse_args()
    R, B, S, window = 49, a.batch, a.samples, 8
    torch.manual_seed(0)
    model = vae_mod.VAE(models.Encoder_Back_GRU, models.FaFp, models.Decoder, 8, 8, R,
                        ode_params={"net_sizes": [64, 64, 32], "aug_net_sizes": [64, 64]},
                        enc_params={"q_sizes": [32, 16], "ff_sizes": [16, 16], "SIR_scaler": [0.1, 0.05, 1.0]},
                        uncertainty=True).to("cuda")
    gen = torch.Generator().manual_seed(1)
    x = torch.rand(B, window, R * 9, generator=gen).cuda()
    t = torch.arange(57, dtype=torch.float32) / 7
    scaler = np.linspace(2.0, 9.0, R)
    y_test = (torch.rand(B, 57, R, generator=gen) * 0.5).cuda()
    horizons = [window + 6, window + 13, window + 20, window + 27]

    def host(e1=None):
        y_pred = model(x, t, n_samples=S, training=False)
        y_pr = y_pred.detach().cpu().numpy() * scaler[None, None, None, :]
        if e1 is not None:
            e1.record()
        y_te = y_test.detach().cpu().numpy() * scaler[None, None, :]
        mu, sd = y_pr.mean(1), y_pr.std(1)
        return [(Metrics.nll(y_te[:, g, :], mu[:, g, :], sd[:, g, :]),
                 Metrics.skill(y_te[:, g, :], mu[:, g, :], sd[:, g, :])) for g in horizons]

    def fused_with(**kw):
        def run(e1=None):
            fc = model.forecast(x, t, n_samples=S, y_true=y_test, scaler=scaler, **kw).cpu()
            if e1 is not None:
                e1.record()
            return [(float(fc.nll[g]), float(fc.skill[g])) for g in horizons]
        return run

    fusedf = fused_with()

    def commit_of():
        try:
            return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True,
                                  text=True).stdout.strip() or None
        except OSError:
            return None

    if a.season:
        from ude_amd import forecast as fcast
        T = len(t)
        base = np.median(y_test.cpu().numpy().astype(np.float64) * scaler, axis=(0, 1))
        season = fcast.Season(baseline=base, start=6, every=7)
        with torch.no_grad():
            yhat = model(x, t, n_samples=S, training=False).permute(2, 1, 0, 3).reshape(T, S * B, R).contiguous()
        floor = fcast.MASS_FLOOR

        def host_route(e1=None):
            v = yhat.cpu().numpy()                                              # the copy the device route saves
            if e1 is not None:
                e1.record()
            y = y_test.cpu().numpy().astype(np.float64).transpose(1, 0, 2)[6::7] * scaler      # (M, B, R)
            v = v.astype(np.float64).reshape(T, S, B, R)[6::7] * scaler                        # (M, S, B, R)
            M = v.shape[0]

            def walk(u):
                above = np.concatenate([np.zeros_like(u[:1], dtype=np.int64), (u >= base).cumsum(0)])
                hit = (above[season.run:] - above[:M - season.run + 1]) == season.run
                onset = np.where(hit.any(0), hit.argmax(0), M)
                return u.max(0), u.argmax(0), u.sum(0), onset

            peak, when, total, onset = walk(v)
            y_peak, y_when, y_total, y_onset = walk(y)
            n_when = np.stack([(when == m).sum(0) for m in range(M)])                          # (M, B, R)
            n_onset = np.stack([(onset == m).sum(0) for m in range(M + 1)])
            bins = np.arange(M + 1).reshape(-1, 1, 1)
            near = lambda o: (np.abs(bins - o) <= season.window) & (bins < M)
            flog = lambda n: np.log(np.where(n == 0, floor, n / S))
            cb = np.floor(10 * y_peak) / 10
            rank = (2 * np.arange(S) - S + 1).reshape(-1, 1, 1)
            crps = lambda u, z: np.abs(u - z).sum(0) / S - (rank * np.sort(u, axis=0)).sum(0) / (S * S)
            terms = [flog((n_when * near(y_when)[:M]).sum(0)),
                     flog((n_onset * np.where(y_onset == M, bins == M, near(y_onset))).sum(0)),
                     flog(((peak >= cb - 0.5) & (peak < cb + 0.6)).sum(0)), crps(peak, y_peak), crps(total, y_total)]
            return {"peak_mean": peak.mean(0), "peak_std": peak.std(0), "total_mean": total.mean(0),
                    "total_std": total.std(0), "peak_time": n_when / S, "onset": n_onset / S,
                    "scores": [float(u.mean()) for u in terms], "scores_r": [u.mean(0) for u in terms]}

        def device_route(e1=None):
            st = fcast.ensemble_season(yhat, S, B, season, y_true=y_test, scale=scaler).cpu()
            if e1 is not None:
                e1.record()
            return st

        ha, st = host_route(), device_route()
        got = [float(st.peak_time_skill.log()), float(st.onset_skill.log()), float(st.peak_value_skill.log()),
               float(st.peak_crps), float(st.total_crps)]
        agree = max(abs(p - q) / max(abs(q), 1e-30) for p, q in zip(got, ha["scores"]))
        same_hist = bool(np.array_equal(st.peak_time.numpy().transpose(1, 0, 2), ha["peak_time"]) and
                         np.array_equal(st.onset.numpy().transpose(1, 0, 2), ha["onset"]))
        res_a, res_b = timed_alternating([host_route, device_route], a.runs, a.warmup)
        from ude_amd import _native
        print(json.dumps({"tool": "forecast_timing --season", "commit": commit_of(),
                          "device": torch.cuda.get_device_name(0),
                          "shape": {"R": R, "S": S, "B": B, "N": S * B, "T": T, "M": season.times(T)},
                          "yhat_bytes": T * S * B * R * 4, "considered_bytes": season.times(T) * S * B * R * 4,
                          "result_bytes": sum(int(v.numel()) * 8 for _, v in st._tensors()),
                          "workspace_bytes": _native.prebuilt().forecast_season_workspace(T, S, B, R, 0, 6, 7, 3, 1),
                          "scores_rel_diff_device_vs_host": agree, "histograms_equal": same_hist,
                          "host_route": res_a, "device_route": res_b,
                          "speedup_min_wall": res_a["wall_ms"]["min"] / res_b["wall_ms"]["min"]}))
        return

    if a.aggregate:
        from ude_amd import decoder_head
        from ude_amd import forecast as fcast
        T = len(t)
        rng = np.random.default_rng(3)
        share = rng.uniform(0.5, 40.0, size=R)
        member = rng.permutation(np.arange(R) % 10)
        levels = {"hhs": fcast.Aggregate.from_groups(R, [np.flatnonzero(member == g).tolist() for g in range(10)], share),
                  "nation": fcast.Aggregate.from_groups(R, [range(R)], share)}
        G = sum(lv.n_groups for lv in levels.values())
        with torch.no_grad():
            res = fcast.solve_decode_dynamics(model.ode, _draw(model, x, S, B, R), t, t[1] - t[0],
                                              decoder_head.decoder_linear(model.dec))
        yhat, dyn, names = res
        model.ode.clear_tracking()
        C = len(names)
        w = torch.from_numpy(np.concatenate([lv.weights for lv in levels.values()])).cuda()
        sc = torch.as_tensor(scaler, dtype=torch.float64).cuda()
        state = [c for c, n in enumerate(names) if n not in fcast.DYN_RATES]

        def done(e1, out):
            if e1 is not None:
                e1.record()
            return out

        def einsum_dyn(xp, d, wt):
            """the definitions with einsum in place of the ordered loop (fp64; xp: torch or numpy)"""
            v = d.astype(np.float64) if xp is np else d.to(torch.float64)
            out = {c: xp.einsum("gr,tnr->tng", wt, v[c]) for c in state}
            inc = xp.einsum("gr,tnr->tng", wt, v[3] * v[0] * v[1])
            rec = xp.einsum("gr,tnr->tng", wt, v[4] * v[1])
            out[3], out[4], out[5] = inc / (out[0] * out[1]), rec / out[1], inc / rec
            return xp.stack([out[c] for c in range(C)])

        routes = {
            "device_yhat": lambda e1=None: done(e1, fcast.ensemble_aggregate(yhat, levels, scale=scaler)),
            "torch_on_device_yhat": lambda e1=None: done(
                e1, torch.einsum("gr,tnr->tng", w, yhat.to(torch.float64) * sc).float()),
            "host_yhat": lambda e1=None: np.einsum(
                "gr,tnr->tng", w_host, done(e1, yhat.cpu()).numpy().astype(np.float64) * scaler).astype(np.float32),
            "device_dyn": lambda e1=None: done(e1, fcast.aggregate_dynamics(dyn, names, levels)),
            "torch_on_device_dyn": lambda e1=None: done(e1, einsum_dyn(torch, dyn, w).float()),
            "host_dyn": lambda e1=None: einsum_dyn(np, done(e1, dyn.cpu()).numpy(), w_host).astype(np.float32),
        }
        w_host = w.cpu().numpy()
        got = torch.cat(list(routes["device_yhat"]().values()), -1)
        ref = routes["torch_on_device_yhat"]()
        got_d = torch.cat([v[0] for v in routes["device_dyn"]().values()], -1)
        ref_d = routes["torch_on_device_dyn"]()
        rel = lambda u, v: float(torch.linalg.vector_norm((u - v).double()) / torch.linalg.vector_norm(v.double()))
        res = timed_alternating(list(routes.values()), a.runs, a.warmup)
        opts = dict(dynamics=True, quantiles=[0.025, 0.5, 0.975])
        fc_res = timed_alternating([fused_with(**opts), fused_with(aggregate=levels, **opts)], a.runs, a.warmup)
        n_in, n_dyn = T * S * B * R * 4, (C - 1) * T * S * B * R * 4
        n_out, n_dyn_out = T * S * B * G * 4, C * T * S * B * G * 4
        ev = res[0]["native_calls_ms"]["forecast_aggregate"]["min"]
        ev_d = res[3]["native_calls_ms"]["forecast_aggregate_dyn"]["min"]
        print(json.dumps({"tool": "forecast_timing --aggregate", "commit": commit_of(),
                          "device": torch.cuda.get_device_name(0),
                          "shape": {"R": R, "S": S, "B": B, "N": S * B, "T": T, "C": C, "levels": [10, 1], "G_tot": G},
                          "yhat_bytes_read": n_in, "yhat_bytes_written": n_out,
                          "dyn_bytes_read": n_dyn, "dyn_bytes_written": n_dyn_out,
                          "fp64_operations": {"yhat": 2 * R * G * T * S * B, "dyn": 2 * R * G * T * S * B * (C - 1)},
                          "rel_diff_device_vs_einsum": {"yhat": rel(got, ref), "dyn": rel(got_d, ref_d)},
                          "achieved_bytes_per_s": {"forecast_aggregate": (n_in + n_out) / (ev * 1e-3),
                                                   "forecast_aggregate_dyn": (n_dyn + n_dyn_out) / (ev_d * 1e-3)},
                          **dict(zip(routes, res)),
                          "forecast_dynamics_quantiles": fc_res[0], "forecast_dynamics_quantiles_aggregate": fc_res[1]}))
        return

    if a.joint:
        from ude_amd import forecast as fcast
        from ude_amd import _native
        T = len(t)
        with torch.no_grad():
            yhat = model(x, t, n_samples=S, training=False).permute(2, 1, 0, 3).reshape(T, S * B, R).contiguous()
        sc = torch.as_tensor(scaler, dtype=torch.float64)
        out = {"tool": "forecast_timing --joint", "commit": commit_of(), "device": torch.cuda.get_device_name(0),
               "shape": {"R": R, "S": S, "B": B, "N": S * B, "T": T}, "yhat_bytes": T * S * B * R * 4}
        for grid, (start, every) in (("weekly", (6, 7)), ("daily", (0, 1))):
            joint = fcast.Joint(start=start, every=every)
            M = joint.times(T)

            def device_route(e1=None):
                js = fcast.ensemble_joint(yhat, S, B, y_test, joint, scale=scaler).cpu()
                if e1 is not None:
                    e1.record()
                return js

            def torch_route(e1=None):
                js = fcast._joint_torch(yhat, S, B, joint, M, y_test, sc.cuda()).cpu()
                if e1 is not None:
                    e1.record()
                return js

            def host_route(e1=None):
                v = yhat.cpu()                                                  # the copy the device route saves
                if e1 is not None:
                    e1.record()
                return fcast._joint_torch(v, S, B, joint, M, y_test.cpu(), sc)

            ja, jb = device_route(), torch_route()
            rel = lambda u, v: float(torch.linalg.vector_norm(u - v) / torch.linalg.vector_norm(v))
            agree = {name: rel(u, v) for (name, u), (_, v) in zip(ja._tensors(), jb._tensors())}
            res = timed_alternating([device_route, torch_route, host_route], a.runs, a.warmup)
            out[grid] = {"M": M, "pair_coordinates": S * S * B * M * R,
                         "workspace_bytes": _native.prebuilt().forecast_joint_workspace(T, S, B, R, start, every, 1),
                         "rel_diff_device_vs_torch": agree, "device_route": res[0], "torch_on_device_route": res[1],
                         "host_route": res[2],
                         "device_over_torch_on_device_min_wall": res[0]["wall_ms"]["min"] / res[1]["wall_ms"]["min"],
                         "speedup_vs_host_min_wall": res[2]["wall_ms"]["min"] / res[0]["wall_ms"]["min"]}
        print(json.dumps(out))
        return

    if a.scenario:
        from ude_amd import decoder_head
        from ude_amd import forecast as fcast
        T = len(t)
        lin = decoder_head.decoder_linear(model.dec)
        with torch.no_grad():
            mean, std = model.enc(x)
            eps = torch.randn(S, B, R, model.ld_enc, device="cuda")
            z = (models.reparam(eps, std, mean, S, B, uncertainty=True) + 1e-5).contiguous()
        step = t[1] - t[0]
        C = len(fcast.dynamics_names(model.ode))
        dyn_out = torch.empty((C, T, S * B, R), dtype=torch.float32, device="cuda")

        def solve(fn, *extra, **kw):
            def run(e1=None):
                res = fn(model.ode, z, t, step, lin, *extra, **kw)
                assert res is not None
                model.ode.clear_tracking()
                if e1 is not None:
                    e1.record()
                return res
            return run

        routes = {"forecast_dec": solve(fcast.solve_decode_forecast),
                  "forecast_dyn": solve(fcast.solve_decode_dynamics, out=dyn_out)}
        checks = {}
        if hasattr(fcast, "solve_decode_scenario"):
            n_steps = fcast._forecast_plan(model.ode, z, t, step).prob.n_steps
            k, r = torch.arange(n_steps).view(-1, 1), torch.arange(R).view(1, -1)
            ones = torch.ones(n_steps, R, 2, device="cuda")
            mixed = torch.stack([0.5 + 0.1 * ((3 * k + r) % 7).float(), 0.8 + 0.05 * ((k + 2 * r) % 5).float()], -1).cuda()
            routes = {"forecast_dec": routes["forecast_dec"],
                      "forecast_scn_ones": solve(fcast.solve_decode_scenario, ones),
                      "forecast_scn_table": solve(fcast.solve_decode_scenario, mixed),
                      "forecast_dyn": routes["forecast_dyn"],
                      "forecast_scn_dyn": solve(fcast.solve_decode_scenario, mixed, dynamics=True, out=dyn_out)}
            checks["ones_equal_forecast_dec"] = bool(torch.equal(routes["forecast_scn_ones"]()[0],
                                                                 routes["forecast_dec"]()))
            checks["table_changes_the_forecast"] = not bool(torch.equal(routes["forecast_scn_table"]()[0],
                                                                        routes["forecast_dec"]()))
        res = timed_alternating(list(routes.values()), a.runs, a.warmup)
        print(json.dumps({"tool": "forecast_timing --scenario", "commit": commit_of(),
                          "device": torch.cuda.get_device_name(0),
                          "shape": {"R": R, "L": 8, "S": S, "B": B, "N": S * B, "T": T, "C": C},
                          **checks, **dict(zip(routes, res))}))
        return

    if a.dynamics:
        from ude_amd import eval_rhs
        from ude_amd import forecast as fcast
        T, names = len(t), fcast.dynamics_names(model.ode)

        def latent_route(e1=None):
            with torch.no_grad():
                y_pred = model(x, t, n_samples=S, training=False)
                lat, ode = model.latent, model.ode
                weights = ode._eval_weights()
                rows = []
                for j in range(T):
                    xj = lat[j]
                    _f, rates, fa = eval_rhs.rhs_eval(ode, xj, weights)
                    rows.append(torch.stack([xj[..., 0], xj[..., 1], xj[..., 2], rates[..., 0], rates[..., 1],
                                             rates[..., 0] * xj[..., 0] / rates[..., 1],
                                             fa[..., 0], fa[..., 1], fa[..., 2]]))
                dyn = torch.stack(rows, 1).contiguous()                              # (C, T, N, R)
                yhat = y_pred.permute(2, 1, 0, 3).reshape(T, S * B, R)
                fc = fcast.ensemble_summary(yhat, S, B, y_true=y_test, scale=scaler)
                fc.dynamics = fcast.dynamics_summary(dyn, names, S, B)
                fc = fc.cpu()
            if e1 is not None:
                e1.record()
            return fc

        def fused_dyn(e1=None):
            fc = model.forecast(x, t, n_samples=S, y_true=y_test, scaler=scaler, dynamics=True).cpu()
            if e1 is not None:
                e1.record()
            return fc

        torch.manual_seed(7)
        fa_ = latent_route()
        torch.manual_seed(7)                               # the same draw: the two routes' summaries agree
        fb_ = fused_dyn()
        vnorm = lambda v: torch.linalg.vector_norm(v, dim=(1, 2, 3))      # per channel
        agree = (vnorm(fb_.dynamics.mean - fa_.dynamics.mean) / vnorm(fa_.dynamics.mean).clamp(min=1e-30)).tolist()
        res_a, res_b, res_c = timed_alternating([latent_route, fused_dyn, fusedf], a.runs, a.warmup)
        C = len(names)
        print(json.dumps({"tool": "forecast_timing --dynamics", "commit": commit_of(),
                          "device": torch.cuda.get_device_name(0),
                          "shape": {"R": R, "L": 8, "S": S, "B": B, "N": S * B, "T": T, "C": C},
                          "dyn_bytes": C * T * S * B * R * 4, "latent_bytes": T * S * B * R * 8 * 4,
                          "channel_mean_rel_diff_fused_vs_latent_route": dict(zip(names, agree)),
                          "latent_route": res_a, "fused_dynamics": res_b, "fused_no_dynamics": res_c,
                          "speedup_min_wall": res_a["wall_ms"]["min"] / res_b["wall_ms"]["min"]}))
        return

    torch.manual_seed(7)
    ra = host()
    torch.manual_seed(7)                                   # the same draw: the two paths' scores agree
    rb = fusedf()
    agree = max(abs(p - q) / max(abs(q), 1e-30) for u, v in zip(rb, ra) for p, q in zip(u, v))
    res_a = timed(host, a.runs, a.warmup)
    res_b, res_c, res_d = timed_alternating([fusedf, fused_with(quantiles=[0.025, 0.5, 0.975]),
                                             fused_with(verify=True)], a.runs, a.warmup)
    from ude_amd import _native
    ws = {"summary": _native.prebuilt().forecast_summary_workspace(57, S, B, R, 0),
          "verify": _native.prebuilt().forecast_verify_workspace(57, S, B, R, 0, 11, 10)}
    out = {"tool": "forecast_timing", "commit": commit_of(), "device": torch.cuda.get_device_name(0),
           "shape": {"R": R, "L": 8, "S": S, "B": B, "N": S * B, "T": 57},
           "latent_path_used_by_forecast": model.latent is not None,
           "scores_rel_diff_fused_vs_host": agree, "host": res_a, "fused": res_b,
           "fused_quantiles": res_c, "fused_verify": res_d, "workspace_bytes": ws,
           "speedup_min_wall": res_a["wall_ms"]["min"] / res_b["wall_ms"]["min"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
