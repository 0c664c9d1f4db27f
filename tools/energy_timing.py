"""Time the energy-score training head next to the CRPS head and the torch definition.

The state49 training shape of tests/golden/e2e_vae_state49 scaled to the bench batch: y_hat (T = 9, S = 64
samples of B = 320 windows = 20,480 trajectories, R = 49) resident on the device, seeded normals around the
targets.  tools/crps_timing.py's protocol: after 5 warm-ups, 10 runs each, the routes taking turns run by run,
each a forward plus a backward to d y_hat:

  (a) energy, once per block kind: ude_amd.decoder_head.energy_head -- ude_energy_forward, ude_energy_backward;
  (b) crps: ude_amd.decoder_head.crps_head -- ude_crps_forward, ude_crps_backward;
  (c) torch, once per block kind: lib.train_functions.energy_loss on the same device tensor (the baseline: the
      pairwise differences in chunks of at most 256 MB, autograd's backward).

Per route: min / median / max of the wall clock, of the span between a device event recorded before the call
and one after its last device operation, and of each gfx950 C-ABI call's own event time
(ude_amd.fused.EVENTS: energy_fwd / energy_bwd, crps_fwd / crps_bwd).  Prints one JSON line.

    python tools/energy_timing.py [--runs 10] [--warmup 5] [--batch 320] [--samples 64] [--times 9] [--fair] [--commit ID]
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
    ap.add_argument("--commit", default=None, help="the commit the tree stands on, for a copy without git metadata")
    a = ap.parse_args()
    T, S, B, R = a.times, a.samples, a.batch, 49
    gen = torch.Generator().manual_seed(0)
    y = (2.0 + torch.rand(B, T, R, generator=gen)).cuda()
    yhat = (y.permute(1, 0, 2).unsqueeze(1).cpu() + 0.5 * torch.randn(T, S, B, R, generator=gen)).reshape(T, S * B, R)
    yhat = yhat.cuda().requires_grad_(True)
    blocks = train_functions.ENERGY_BLOCKS

    def backward(loss):
        yhat.grad = None
        loss.backward()

    def energy(block):
        return lambda: backward(decoder_head.energy_head(yhat, y, S, B, block=block, fair=a.fair))

    def crps():
        backward(decoder_head.crps_head(yhat, y, S, B, fair=a.fair))

    def torch_definition(block):
        return lambda: backward(train_functions.energy_loss(yhat.reshape(T, S, B, R).permute(2, 1, 0, 3), y,
                                                            block=block, fair=a.fair))

    fns = [energy(k) for k in blocks] + [crps] + [torch_definition(k) for k in blocks]
    res = timed_alternating(fns, a.runs, a.warmup)
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True).stdout.strip() or None
    except OSError:
        commit = None
    n = T * S * B * R
    lib = _native.prebuilt()
    print(json.dumps({"tool": "energy_timing", "commit": commit, "device": torch.cuda.get_device_name(0),
                      "shape": {"T": T, "S": S, "B": B, "R": R, "fair": bool(a.fair)},
                      "yhat_bytes": 4 * n, "dyhat_bytes": 4 * n,
                      "workspace_bytes": {k: lib.energy_workspace(T, S, B, R, i) for i, k in enumerate(blocks)},
                      "runs": a.runs, "warmup": a.warmup,
                      "energy_head": {k: res[i] for i, k in enumerate(blocks)},
                      "crps_head": res[len(blocks)],
                      "torch_energy_loss": {k: res[len(blocks) + 1 + i] for i, k in enumerate(blocks)}}))


if __name__ == "__main__":
    main()
