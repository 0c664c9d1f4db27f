"""The whole-solve comparison of tests/test_kernel_order.py, shared with the configuration lattice
(tests/test_config_lattice_gpu.py): the fused training forward against the kernel-order restatement
(oracle/ude_korder.c) bit for bit, the fused backward against the restatement's exact VJP."""
import os

import numpy as np
import torch

from helpers import kernel_forward_store, normwise_rel
from oracle.ude_korder import KernelOrderOracle, lib as ko_lib
from oracle.ude_oracle import OracleRHS

DEV = "cuda"
THREADS = int(os.environ.get("UDE_ORACLE_THREADS", "16"))
DM = torch.tensor([0.3, -0.2], dtype=torch.float64)
DS = torch.tensor([0.5, 0.1], dtype=torch.float64)
DN = 0.1
BAR_BWD = 1e-6


def _gpu_vjp(pkg, mod, y0, t, dl, h=None):
    """fused forward + VJP with the posterior / |Fa| terms; the cotangents the kernel receives are the
    fp32 roundings of dl, DM, DS, DN (returned, for the oracle)."""
    mg = mod.to(DEV)
    mg.zero_grad(set_to_none=True)
    yg = y0.to(DEV).requires_grad_(True)
    mg.clear_tracking()
    assert pkg.fusable(mg, yg)
    lat = pkg.odeint(mg, yg, t, method="rk4", options=dict(step_size=t[1] - t[0] if h is None else h))
    loss = (lat * dl.float().to(DEV)).sum()
    if mg.ode_type != "Fp":
        loss = loss + np.float32(DN) * torch.norm(torch.stack(mg.tracker))
    if mg.ode_type != "Fa":
        post = mg.posterior()
        loss = loss + (post.loc * DM.float().to(DEV)).sum() + (post.scale * DS.float().to(DEV)).sum()
    loss.backward()
    out = {"y0": yg.grad.cpu()}
    for lin_i, lin in enumerate(mg.ude_linears()):
        out[("w", lin_i)] = lin.weight.grad.cpu()
        out[("b", lin_i)] = lin.bias.grad.cpu()
    mod.cpu()
    return lat.detach().cpu(), out


def _check(pkg, mod, y0, t, dl, label, h=None):
    h = t[1] - t[0] if h is None else h
    mod = mod.to(DEV)
    lat_k, X_k, (m_k, s_k, n_k) = kernel_forward_store(pkg, mod, y0, t, h)
    lat_v, got = _gpu_vjp(pkg, mod, y0, t, dl, h)
    assert torch.equal(lat_v, lat_k)                      # the same forward, bit for bit
    mod = mod.cpu()
    ko = KernelOrderOracle(OracleRHS.from_module(mod, torch.float32))
    out = ko.solve(y0, t, h, stage_inputs=True, threads=THREADS)
    n_lat = int((out["latent"] != lat_k).sum())
    n_x = int((out["stage_inputs"] != X_k).sum())
    bad_traj = ((out["stage_inputs"] != X_k).reshape(X_k.shape[0], X_k.shape[1], -1).any(2).any(0)).nonzero()
    print(f"{label}: latent {lat_k.numel()} values, {n_lat} differ from the kernel-order restatement; "
          f"stage inputs {X_k.numel()} values, {n_x} differ (trajectories {bad_traj.flatten()[:8].tolist()})")
    assert n_lat == 0 and n_x == 0
    kind = mod.ode_type
    if kind != "Fa":
        assert torch.equal(out["mean"], m_k) and torch.equal(out["std"], s_k), (out["mean"], m_k, out["std"], s_k)
    if kind != "Fp":
        assert torch.equal(out["fa_norm"], n_k), (out["fa_norm"], n_k)
    dl32 = dl.float().double()
    dy0, gr, mag = ko.vjp(y0, t, h, dl32, DM.float().double(), DS.float().double(), float(np.float32(DN)),
                          stats=out, threads=THREADS)
    errs = {"y0": normwise_rel(got["y0"], dy0)}
    rel_mag = {}
    wn = [n for n in ko.names if "_w" in n]
    for i, nm in enumerate(wn):
        for kk, key in ((nm, ("w", i)), (nm.replace("_w", "_b"), ("b", i))):
            errs[kk] = normwise_rel(got[key], gr[kk])
            # the same difference against the magnitude of the summed terms (the scale of fp32 rounding)
            rel_mag[kk] = float((got[key].double() - gr[kk]).norm() / max(float(mag[kk].norm()), 1e-30))
    # the size of fp32 backward rounding on this very forward: the same VJP executed in fp32 in the
    # kernel's association (ko_set_assoc(1): the step's adjoint accumulated as the kernel's bwd_body does,
    # one update per stage; per-tile fp32 weight-gradient sums, then the tiles, like the kernel's slabs)
    ko_lib().ko_set_assoc(1)
    try:
        dy0_32, gr32, _ = ko.vjp(y0, t, h, dl32, DM.float().double(), DS.float().double(), float(np.float32(DN)),
                                 stats=out, threads=THREADS, fp32=True)
    finally:
        ko_lib().ko_set_assoc(0)
    ref32 = {"y0": normwise_rel(dy0_32, dy0)}
    ref32.update({k: normwise_rel(gr32[k], gr[k]) for k in gr})
    dd = lambda a, b: normwise_rel(a, b)
    d2 = (got["y0"].double() - dy0).reshape(dy0.shape[0], -1).pow(2).sum(1)
    top = torch.topk(d2, min(4, dy0.shape[0]))
    print(f"  dy0 split: S, I, R dims {dd(got['y0'][..., :3], dy0[..., :3]):.1e} [{dd(dy0_32[..., :3], dy0[..., :3]):.1e}], "
          f"static dims {dd(got['y0'][..., 3:], dy0[..., 3:]):.1e} [{dd(dy0_32[..., 3:], dy0[..., 3:]):.1e}]; worst "
          f"trajectories {top.indices.tolist()} carry {float(top.values.sum() / d2.sum()):.2f} of the kernel's dy0 error^2")
    print(f"  kernel backward vs the exact VJP of the kernel-order forward [fp32 execution of that VJP]: "
          + ", ".join(f"{k} {v:.1e} [{ref32[k]:.1e}]" for k, v in errs.items()))
    print("  (kernel difference / |summed terms|: " + ", ".join(f"{k} {v:.1e}" for k, v in rel_mag.items()) + ")")
    # bar: max(1e-6, 2 x the fp32 execution's distance) normwise; for a weight gradient (a sum of
    # N x E terms) also 1e-6 of the summed terms' magnitude -- the standard measure of a long fp32
    # summation's rounding, which cancellation in the sum does not shrink (Higham, ch. 4)
    bars = {k: max(BAR_BWD, 2.0 * ref32[k]) for k in errs}
    for k in rel_mag:
        bars[k] = max(bars[k], BAR_BWD * float(mag[k].norm()) / max(float(gr[k].norm()), 1e-30))
    over = {k: (v, bars[k]) for k, v in errs.items() if v > bars[k]}
    assert not over, f"{label}: kernel backward vs the exact VJP of its own forward above its bar: {over}"
