"""Time the CRPS training head next to the nll kernels it sits beside.

The state49 training shape of tests/golden/e2e_vae_state49 scaled to the bench batch: y_hat (T = 9, S = 64
samples of B = 320 windows = 20,480 trajectories, R = 49) resident on the device, seeded normals around the
targets.  After 5 warm-ups, 10 runs each, three routes taking turns run by run, each a forward plus a
backward to d y_hat:

  (a) crps: ude_amd.decoder_head.crps_head -- ude_crps_forward, ude_crps_backward;
  (b) nll: ude_amd.decoder_head.nll_head -- ude_nll_forward, ude_nll_backward (state model: FaFp R = 49, L = 8);
  (c) torch: lib.train_functions.crps_loss on the device (sort, searchsorted and torch glue).

Per route: min / median / max of the wall clock, of the span between a device event recorded before the call
and one after its last device operation, and of each gfx950 C-ABI call's own event time
(ude_amd.fused.EVENTS: crps_fwd / crps_bwd, nll_fwd / nll_bwd).  Prints one JSON line.

    python tools/crps_timing.py [--runs 10] [--warmup 5] [--batch 320] [--samples 64] [--times 9] [--fair]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
importlib.import_module("forecasting-influenza-using-universal-differential-equations_amd")

import lib.models as models  # noqa: E402
import lib.train_functions as train_functions  # noqa: E402
from ude_amd import _native, decoder_head, fused  # noqa: E402


def stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


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
        fn()
        e1.record()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=320)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--times", type=int, default=9)
    ap.add_argument("--fair", action="store_true", help="time the fair score (D = S - 1)")
    a = ap.parse_args()
    T, S, B, R = a.times, a.samples, a.batch, 49
    gen = torch.Generator().manual_seed(0)
    y = (2.0 + torch.rand(B, T, R, generator=gen)).cuda()
    yhat = (y.permute(1, 0, 2).unsqueeze(1).cpu() + 0.5 * torch.randn(T, S, B, R, generator=gen)).reshape(T, S * B, R)
    yhat = yhat.cuda().requires_grad_(True)
    ode = models.FaFp(R, latent_dim=8, net_sizes=[64, 64, 32], aug_net_sizes=[64, 64]).cuda()

    def backward(loss):
        yhat.grad = None
        loss.backward()

    def crps():
        backward(decoder_head.crps_head(yhat, y, S, B, fair=a.fair))

    def nll():
        backward(decoder_head.nll_head(ode, yhat, y, S, B)[0])

    def torch_definition():
        backward(train_functions.crps_loss(yhat.reshape(T, S, B, R).permute(2, 1, 0, 3), y, fair=a.fair))

    res = timed_alternating([crps, nll, torch_definition], a.runs, a.warmup)
    try:
        commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True).stdout.strip() or None
    except OSError:
        commit = None
    n = T * S * B * R
    print(json.dumps({"tool": "crps_timing", "commit": commit, "device": torch.cuda.get_device_name(0),
                      "shape": {"T": T, "S": S, "B": B, "R": R, "fair": bool(a.fair)},
                      "yhat_bytes": 4 * n, "dyhat_bytes": 4 * n,
                      "workspace_bytes": _native.prebuilt().crps_workspace(T, S, B, R),
                      "runs": a.runs, "warmup": a.warmup,
                      "crps_head": res[0], "nll_head": res[1], "torch_crps_loss": res[2]}))


if __name__ == "__main__":
    main()
