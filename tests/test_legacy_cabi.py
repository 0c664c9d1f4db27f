"""The legacy C-ABI entries (ude_rk4_forward, ude_rk4_backward, ude_rk4_backward_sir,
ude_rk4_forward_dec; ``ctl == nullptr`` in csrc/ude_entry.h), driven directly from a ``Plan``.

The Python path uses only the ``*_ex`` entries (one tail kernel, in-kernel statistics finalize); the
legacy ones end in separate launches instead: the statistics and latent_init_loss finalize of the
forward, the gradient finalize of the backward and -- for a model with static features (``HOIST``) --
the static partial / reduce / dy0 kernels.  Statistics travel as one contiguous 5-float vector
{mean[2], std[2], |Fa|}.

Part 1 holds the plain solve to the goldens' fp64 arrays with ``test_fused_matches_golden``'s bars
(tests/test_gpu_parity.py).  Part 2 holds forward_dec -> ude_decoder_backward -> backward_sir on
``fafp_r1_weekly`` to the fp64 chain of tests/epilogue_helpers.py with tests/test_decoder_epilogue.py's
bars, for  loss = g_reg reg + <y_hat, c> + the side-statistics cotangents  (the nll is not part of
these entries).
"""
import math

import pytest
import torch

import epilogue_helpers as H
from conftest import load_golden
from helpers import module_from_golden, normwise_rel, step_of, tol
from test_decoder_epilogue import _check

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _plan_and_pack(mod, y0, t, h):
    """(plan, packed weights, C-ABI ordered parameters) of mod (on the device) for y0 (N, R, L)."""
    from ude_amd import fused
    from ude_amd.schedule import build_schedule
    params = [p for lin in mod.ude_linears() for p in (lin.weight, lin.bias)]
    plan = fused.make_plan(mod.ude_config(), build_schedule(t, h), y0.shape[0], mod.fa_weight(), y0.device,
                           [p.shape for p in params])
    assert plan.prob.recompute == 0
    return plan, fused.packed_weights(plan, params, y0.device), params


def _f32(n, dtype=torch.float32):
    return torch.empty(max(int(n), 1), dtype=dtype, device=DEV)


def _solve_backward(plan, pack, y0, ckpt, dlatent, dl3, stats, dstats):
    """ude_rk4_backward (dl3 None) or ude_rk4_backward_sir: (d y0, the parameter gradients, C-ABI order)."""
    from ude_amd import fused
    sz, lib = plan.sizes, plan.lib
    dy0 = torch.empty_like(y0)
    slab = _f32(sz.grad_slab_bytes // 4)
    dparams = _f32(sz.n_params)
    head = (plan.desc, plan.prob, pack.data_ptr(), plan.sched_dev.data_ptr(), y0.data_ptr(), ckpt.data_ptr())
    tail = (stats.data_ptr(), dstats.data_ptr(), dy0.data_ptr(), slab.data_ptr(), dparams.data_ptr(), fused._stream(y0.device))
    if dl3 is None:
        lib.backward(*head, dlatent.data_ptr(), *tail)
    else:
        lib.backward_sir(*head, None, dl3.data_ptr(), *tail)
    return dy0, fused._split(dparams, plan.param_shapes)


@pytest.mark.parametrize("case", ["fafp_r1_weekly", "fafp_r3_l5_ragged"])
def test_legacy_solve_matches_golden(pkg, case):
    from ude_amd import fused
    g = load_golden(case)
    mod = module_from_golden(pkg, g, DEV)
    t, h = step_of(g)
    y0 = torch.from_numpy(g["y0"]).to(DEV).contiguous()
    plan, pack, params = _plan_and_pack(mod, y0, t, h)
    sz = plan.sizes
    if case == "fafp_r3_l5_ragged":
        assert y0.shape[0] % 16 != 0 and y0.shape[2] > 3         # ragged N, static features
    latent = torch.empty((plan.n_times,) + tuple(y0.shape), dtype=torch.float32, device=DEV)
    ckpt = _f32(sz.ckpt_bytes // 4)
    stats_slab = _f32(sz.stats_slab_bytes // 8, torch.float64)
    stats = torch.zeros(5, dtype=torch.float32, device=DEV)
    plan.lib.forward(plan.desc, plan.prob, pack.data_ptr(), plan.sched_dev.data_ptr(), y0.data_ptr(),
                     latent.data_ptr(), ckpt.data_ptr(), stats_slab.data_ptr(), stats.data_ptr(), fused._stream(y0.device))
    dlatent = torch.from_numpy(g["dlatent"]).to(DEV).to(torch.float32).contiguous()
    dstats = torch.cat([torch.from_numpy(g[k]) for k in ("dmean", "dstd", "dnorm")]).to(DEV).to(torch.float32)
    dy0, grads = _solve_backward(plan, pack, y0, ckpt, dlatent, None, stats, dstats)
    torch.cuda.synchronize()
    out = {"latent": latent, "mean": stats[0:2], "std": stats[2:4], "fa_norm": stats[4:5], "d_y0": dy0}
    names = {id(p): n for n, p in mod.named_parameters()}
    for p, d in zip(params, grads):
        out["d_" + names[id(p)]] = d
    bad = []
    for key in ["latent", "mean", "std", "fa_norm"]:
        err = normwise_rel(out[key], g["ref64_" + key])
        print(f"{case} {key}: {err:.3e} (bar {tol(g, key):.1e})")
        if not err <= tol(g, key):
            bad.append((key, err))
    grad_keys = [k[len("ref64_"):] for k in g if k.startswith("ref64_d_")]
    assert len(grad_keys) == 1 + len(params)
    for k in grad_keys:
        err = normwise_rel(out[k], g["ref64_" + k])
        print(f"{case} {k}: {err:.3e} (bar {tol(g, k, 2e-5):.1e})")
        if not err <= tol(g, k, 2e-5):
            bad.append((k, err))
    assert not bad, f"{case}: {bad}"


def _weekly_epilogue_case(pkg):
    """``fafp_r1_weekly`` as an epilogue_helpers.Case: the golden's model, y0 and grid; decoder weights,
    targets and cotangents drawn as ``epilogue_helpers.make_case`` draws them."""
    g = load_golden("fafp_r1_weekly")
    mod = module_from_golden(pkg, g)
    t, h = step_of(g)
    y0 = torch.from_numpy(g["y0"])
    N, R, L = y0.shape
    S, B, T = 6, N // 6, len(t)
    gen = torch.Generator().manual_seed(1)
    W = torch.randn(R, 3 * R, generator=gen) / math.sqrt(3 * R)
    b = 0.1 * torch.randn(R, generator=gen)
    lat, margin = H._forward(mod, False, y0, t, h, None, torch.float64)
    st = H.group_stats(H.decode(lat[..., :3], W.double(), b.double()), S, B)
    y = (st[..., 0] + 0.7 * st[..., 1] * torch.randn(T, B, R, generator=gen, dtype=torch.float64)).permute(1, 0, 2)
    c_yhat = torch.randn(T, N, R, generator=gen, dtype=torch.float64)
    dl_full = torch.randn(T, N, R, L, generator=gen, dtype=torch.float64)
    return H.Case("FaFp", mod, y0, t, h, W, b, y.float().contiguous(), S, B, None, c_yhat, dl_full, lat, margin)


def test_legacy_decoder_epilogue_matches_fp64(pkg):
    import copy
    from ude_amd import fused
    case = _weekly_epilogue_case(pkg)
    cond = H.conditions(case)
    print("\nfafp_r1_weekly: " + ", ".join(f"{k} {v:.3g}" for k, v in cond.items()))
    # the decoder's and latent_init_loss's share of check_conditions (no nll here; the solve itself is
    # held to this golden at its own mask distance by test_fused_matches_golden)
    assert cond["kink"] >= 1e-4 and cond["outside"] >= 0.05, cond
    ref = H.reference_chain(case, {"yhat", "reg"})
    mod = copy.deepcopy(case.mod).to(DEV)
    y0 = case.y0.to(DEV).contiguous()
    plan, pack, params = _plan_and_pack(mod, y0, case.t, case.h)
    assert plan.out_k is not None
    sz, lib = plan.sizes, plan.lib
    stream = fused._stream(y0.device)
    N, R, L = y0.shape
    T = plan.n_times
    Wd, bd = case.W.to(DEV).contiguous(), case.b.to(DEV).contiguous()
    dec_pack = _f32(sz.dec_pack_bytes // 4)
    lib.pack_decoder(plan.desc, Wd.data_ptr(), bd.data_ptr(), dec_pack.data_ptr(), stream)
    yhat = torch.empty((T, N, R), dtype=torch.float32, device=DEV)
    ckpt = _f32((sz.ckpt_bytes + sz.ckpt_final_bytes) // 4)
    stats_slab = _f32(sz.stats_slab_bytes // 8, torch.float64)
    reg_slab = _f32(sz.grid_fwd, torch.float64)
    stats = torch.zeros(5, dtype=torch.float32, device=DEV)
    reg = _f32(1)
    lib.forward_dec(plan.desc, plan.prob, pack.data_ptr(), plan.sched_dev.data_ptr(), y0.data_ptr(), dec_pack.data_ptr(),
                    yhat.data_ptr(), ckpt.data_ptr(), stats_slab.data_ptr(), reg_slab.data_ptr(), stats.data_ptr(),
                    reg.data_ptr(), stream)
    dyhat = case.c_yhat.to(DEV).to(torch.float32).contiguous()
    g_reg = torch.full((1,), H.G_REG, dtype=torch.float32, device=DEV)
    dl3 = torch.empty((T, N, R, 3), dtype=torch.float32, device=DEV)
    dWd, dbd = torch.empty_like(Wd), torch.empty_like(bd)
    dec_ws = _f32(sz.dec_ws_bytes // 4)
    lib.decoder_backward(plan.desc, plan.prob, plan.sched_dev.data_ptr(), ckpt.data_ptr(), dyhat.data_ptr(),
                         Wd.data_ptr(), g_reg.data_ptr(), dec_ws.data_ptr(), dl3.data_ptr(), dWd.data_ptr(),
                         dbd.data_ptr(), stream)
    dstats = torch.tensor(H.DMEAN + H.DSTD + (H.DNORM,), dtype=torch.float32, device=DEV)
    dy0, grads = _solve_backward(plan, pack, y0, ckpt, None, dl3, stats, dstats)
    torch.cuda.synchronize()
    out = {"yhat": yhat, "reg": reg, "mean": stats[0:2], "std": stats[2:4], "fa_norm": stats[4:5], "d_y0": dy0,
           "d_ode": grads, "dW": dWd, "db": dbd}
    _check("legacy forward_dec / decoder_backward / backward_sir", out, ref,
           ["yhat", "reg", "mean", "std", "fa_norm", "d_y0", "d_ode", "dW", "db"])
