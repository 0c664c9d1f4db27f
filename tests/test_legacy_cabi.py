"""The older C-ABI entries (ude_rk4_forward, ude_rk4_backward, ude_rk4_backward_sir,
ude_rk4_forward_dec), driven directly from a ``Plan``.

They take no control words and carry the statistics as one contiguous 5-float vector {mean[2], std[2],
|Fa|}; behind that they are the launches of the ``*_ex`` entries the Python path uses (in-kernel
statistics finalize, one tail kernel), on spare control words at the end of ``stats_slab`` /
``grad_slab`` that the call zeroes on its stream.

Part 1 holds the plain solve to the goldens' fp64 arrays with ``test_fused_matches_golden``'s bars
(tests/test_gpu_parity.py).  Part 2 holds forward_dec -> ude_decoder_backward -> backward_sir on
``fafp_r1_weekly`` to the fp64 chain of tests/epilogue_helpers.py with tests/test_decoder_epilogue.py's
bars, for  loss = g_reg reg + <y_hat, c> + the side-statistics cotangents  (the nll is not part of
these entries).  Part 3 is a Bayesian model whose backward ends in the tail kernel (both halves of
``dparams``).

Every part also runs the same inputs through the ``*_ex`` entries and asserts bitwise equality of every
output, with ``stats_slab[0:5]`` against ``UdeSideStats.sums``.  Every older entry is called twice on the
same buffers with nothing re-zeroed in between, and must give the same bits again; ``stats_slab`` and the
gradient slab start out with all-ones 32-bit spare words, so a call that did not zero them would finalize
nothing.
"""
import math

import pytest
import torch

import epilogue_helpers as H
from conftest import load_golden
from helpers import module_from_golden, normwise_rel, step_of, tol
from test_bayes import bayes_module
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


def _slab(plan, n_bytes, dtype):
    """A stats_slab / grad_slab of ude_query's size whose spare control words (its last ctl_bytes) start
    out as 0xffffffff each: non-zero, and no ticket a grid can reach."""
    size = torch.empty((), dtype=dtype).element_size()
    buf = _f32(n_bytes // size, dtype)
    dirty_words(buf, plan.sizes.ctl_bytes)
    return buf


def dirty_words(buf, ctl_bytes):
    """Sets the last ``ctl_bytes`` of ``buf`` to all-ones 32-bit words and checks that every one is non-zero."""
    words = buf.view(torch.int32)[-(int(ctl_bytes) // 4):]
    words.fill_(-1)
    assert words.numel() == int(ctl_bytes) // 4 > 0 and bool((words != 0).all())


def _twice(call, *outs):
    """``call()`` twice on the same buffers, nothing re-zeroed in between: the second ``outs`` are the first's."""
    call()
    first = [o.clone() for o in outs]
    call()
    for i, (a, b) in enumerate(zip(first, outs)):
        assert torch.equal(a, b), f"output {i} of the second call differs"


def _same(label, **pairs):
    bad = [k for k, (a, b) in pairs.items() if not torch.equal(a.reshape(-1), b.reshape(-1))]
    assert not bad, f"{label}: older entry != *_ex entry in {bad}"


def _older_forward(plan, pack, y0):
    """ude_rk4_forward: (latent, training store, stats_slab, the 5 statistics)."""
    from ude_amd import fused
    sz = plan.sizes
    latent = torch.empty((plan.n_times,) + tuple(y0.shape), dtype=torch.float32, device=DEV)
    ckpt = _f32(sz.ckpt_bytes // 4)
    stats_slab = _slab(plan, sz.stats_slab_bytes, torch.float64)
    stats = torch.zeros(5, dtype=torch.float32, device=DEV)
    _twice(lambda: plan.lib.forward(plan.desc, plan.prob, pack.data_ptr(), plan.sched_dev.data_ptr(), y0.data_ptr(),
                                    latent.data_ptr(), ckpt.data_ptr(), stats_slab.data_ptr(), stats.data_ptr(),
                                    fused._stream(y0.device)),
           latent, stats, stats_slab[0:5])
    return latent, ckpt, stats_slab, stats


def _older_backward(plan, pack, y0, ckpt, dlatent, dl3, stats, dstats):
    """ude_rk4_backward (dl3 None) or ude_rk4_backward_sir: (d y0, the flat parameter gradient)."""
    from ude_amd import fused
    sz, lib = plan.sizes, plan.lib
    dy0 = torch.empty_like(y0)
    slab = _slab(plan, sz.grad_slab_bytes, torch.float32)
    dparams = _f32(sz.n_params)
    head = (plan.desc, plan.prob, pack.data_ptr(), plan.sched_dev.data_ptr(), y0.data_ptr(), ckpt.data_ptr())
    tail = (stats.data_ptr(), dstats.data_ptr(), dy0.data_ptr(), slab.data_ptr(), dparams.data_ptr(), fused._stream(y0.device))
    if dl3 is None:
        _twice(lambda: lib.backward(*head, dlatent.data_ptr(), *tail), dy0, dparams)
    else:
        _twice(lambda: lib.backward_sir(*head, None, dl3.data_ptr(), *tail), dy0, dparams)
    return dy0, dparams


def _solve_both_ways(label, plan, pack, y0, dlatent, dstats):
    """The plain solve and its backward through the older entries, held bitwise to forward_ex / backward_ex on
    the same inputs: (latent, the 5 statistics, d y0, the flat parameter gradient)."""
    from ude_amd import fused
    latent, ckpt, stats_slab, stats = _older_forward(plan, pack, y0)
    dy0, dparams = _older_backward(plan, pack, y0, ckpt, dlatent, None, stats, dstats)
    x_latent, x_stats, x_ckpt, x_sums = fused._solve_forward(plan, y0, pack, True)
    x_dy0, x_dparams = fused._solve_backward(plan, y0, pack, x_ckpt, x_stats, dlatent, None,
                                             (dstats[0:2], dstats[2:4], dstats[4:5]))
    torch.cuda.synchronize()
    _same(label, latent=(latent, x_latent), mean=(stats[0:2], x_stats[0]), std=(stats[2:4], x_stats[1]),
          fa_norm=(stats[4:5], x_stats[2]), sums=(stats_slab[0:5], x_sums), d_y0=(dy0, x_dy0),
          dparams=(dparams, x_dparams))
    return latent, stats, dy0, dparams


@pytest.mark.parametrize("case", ["fafp_r1_weekly", "fafp_r3_l5_ragged"])
def test_legacy_solve_matches_golden(pkg, case):
    from ude_amd import fused
    g = load_golden(case)
    mod = module_from_golden(pkg, g, DEV)
    t, h = step_of(g)
    y0 = torch.from_numpy(g["y0"]).to(DEV).contiguous()
    plan, pack, params = _plan_and_pack(mod, y0, t, h)
    if case == "fafp_r3_l5_ragged":
        assert y0.shape[0] % 16 != 0 and y0.shape[2] > 3         # ragged N, static features
    dlatent = torch.from_numpy(g["dlatent"]).to(DEV).to(torch.float32).contiguous()
    dstats = torch.cat([torch.from_numpy(g[k]) for k in ("dmean", "dstd", "dnorm")]).to(DEV).to(torch.float32)
    latent, stats, dy0, dparams = _solve_both_ways(case, plan, pack, y0, dlatent, dstats)
    grads = fused._split(dparams, plan.param_shapes)
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


def test_legacy_bayes_solve_is_the_ex_solve(pkg):
    """``bayes_fp_r1_daily``: a Bayesian model small enough to keep both dW accumulators in registers
    (BFp [20, 20] at R = 1: not ``Model::GST``), so its backward ends in the tail kernel, which reduces the
    mean half and the eps-weighted |std| half of every gradient slab.  Bitwise against the ``*_ex`` entries only;
    the fp64 bars of this golden are tests/test_bayes.py's."""
    from ude_amd import fused, solvers
    g = load_golden("bayes_fp_r1_daily")
    mod = bayes_module(pkg, g, DEV)
    t, h = step_of(g)
    y0 = torch.from_numpy(g["y0"]).to(DEV).contiguous()
    plan = solvers.plan_for(mod, y0, t, h)
    mus, sds = mod.ude_mean_std()
    eps = torch.from_numpy(g["eps"]).to(DEV).to(torch.float32)
    assert plan.sizes.n_params == 2 * eps.shape[1]
    # not GST: the gradient slab ends in the spare control words and is one slab per backward workgroup, whatever
    # the number of steps (the GST workspace holds rows per step and has no spare words)
    p2 = type(plan.prob)(plan.prob.n_traj, 2 * plan.prob.n_steps, plan.prob.n_out, plan.prob.fa_w, plan.prob.recompute)
    sz, sz2 = plan.sizes, plan.lib.query(plan.desc, p2, y0.device.index or 0)
    assert sz2.grid_bwd == sz.grid_bwd and sz2.grad_slab_bytes == sz.grad_slab_bytes
    # ... each slab the [mean | eps-weighted] halves of the (tile-padded) parameter gradient
    assert (sz.grad_slab_bytes - sz.ctl_bytes) % 16 == 0
    assert (sz.grad_slab_bytes - sz.ctl_bytes) // (4 * sz.grid_bwd) >= sz.n_params
    pack = fused._bayes_pack(plan, mus, sds, eps, y0.device)
    dlatent = torch.from_numpy(g["dlatent"]).to(DEV).to(torch.float32).contiguous()
    dstats = torch.cat([torch.from_numpy(g[k]) for k in ("dmean", "dstd", "dnorm")]).to(DEV).to(torch.float32)
    _latent, _stats, _dy0, dparams = _solve_both_ways("bayes_fp_r1_daily", plan, pack, y0, dlatent, dstats)
    n = eps.shape[1]
    assert float(dparams[:n].abs().max()) > 0 and float(dparams[n:].abs().max()) > 0


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
    stats_slab = _slab(plan, sz.stats_slab_bytes, torch.float64)
    reg_slab = _f32(sz.grid_fwd, torch.float64)
    stats = torch.zeros(5, dtype=torch.float32, device=DEV)
    reg = _f32(1)
    _twice(lambda: lib.forward_dec(plan.desc, plan.prob, pack.data_ptr(), plan.sched_dev.data_ptr(), y0.data_ptr(),
                                   dec_pack.data_ptr(), yhat.data_ptr(), ckpt.data_ptr(), stats_slab.data_ptr(),
                                   reg_slab.data_ptr(), stats.data_ptr(), reg.data_ptr(), stream),
           yhat, reg, stats, stats_slab[0:5])
    dyhat = case.c_yhat.to(DEV).to(torch.float32).contiguous()
    g_reg = torch.full((1,), H.G_REG, dtype=torch.float32, device=DEV)
    dl3 = torch.empty((T, N, R, 3), dtype=torch.float32, device=DEV)
    dWd, dbd = torch.empty_like(Wd), torch.empty_like(bd)
    dec_ws = _f32(sz.dec_ws_bytes // 4)
    lib.decoder_backward(plan.desc, plan.prob, plan.sched_dev.data_ptr(), ckpt.data_ptr(), dyhat.data_ptr(),
                         Wd.data_ptr(), g_reg.data_ptr(), dec_ws.data_ptr(), dl3.data_ptr(), dWd.data_ptr(),
                         dbd.data_ptr(), stream)
    dstats = torch.tensor(H.DMEAN + H.DSTD + (H.DNORM,), dtype=torch.float32, device=DEV)
    dy0, dparams = _older_backward(plan, pack, y0, ckpt, None, dl3, stats, dstats)
    # the same chain through forward_dec_ex / decoder_backward / backward_ex
    x_yhat, x_reg, x_stats, x_ckpt, x_sums = fused._dec_forward(plan, y0, pack, Wd, bd)
    x_dy0, x_dWd, x_dbd, x_dparams = fused._dec_backward(plan, y0, pack, x_ckpt, x_stats, Wd, dyhat, g_reg,
                                                         (dstats[0:2], dstats[2:4], dstats[4:5]), None)
    torch.cuda.synchronize()
    _same("fafp_r1_weekly epilogue", yhat=(yhat, x_yhat), reg=(reg, x_reg), mean=(stats[0:2], x_stats[0]),
          std=(stats[2:4], x_stats[1]), fa_norm=(stats[4:5], x_stats[2]), sums=(stats_slab[0:5], x_sums),
          d_y0=(dy0, x_dy0), dparams=(dparams, x_dparams), dW=(dWd, x_dWd), db=(dbd, x_dbd))
    out = {"yhat": yhat, "reg": reg, "mean": stats[0:2], "std": stats[2:4], "fa_norm": stats[4:5], "d_y0": dy0,
           "d_ode": fused._split(dparams, plan.param_shapes), "dW": dWd, "db": dbd}
    _check("legacy forward_dec / decoder_backward / backward_sir", out, ref,
           ["yhat", "reg", "mean", "std", "fa_norm", "d_y0", "d_ode", "dW", "db"])
