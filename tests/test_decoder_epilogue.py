"""The decoder-epilogue training path (VAE.train_step on a HIP device: ude_rk4_forward_dec_ex ->
ude_nll_forward / ude_nll_backward -> ude_decoder_backward -> ude_rk4_backward_ex with dlatent_sir)
against the fp64 chain of tests/epilogue_helpers.py, through ``decoder_head.solve_decode`` /
``decoder_head.nll_head`` and autograd.

Inputs put a quarter of the (n, r) rows outside [0, 1] (latent_init_loss and its derivative are
non-zero) with a gap to the kinks at 0 and 1; ``check_conditions`` holds the fp64 reference to that
before any kernel output is read.  Bars are the project's: 1e-5 normwise for y_hat / reg / nll / the
group and side statistics, 2e-5 for d y0, 5e-5 for every weight gradient (tests/test_gpu_parity.py,
tests/test_bayes.py, tests/test_loss_head.py).  Every measured error is printed.

Measured on an MI355X (normwise, against fp64; worst of the eight chain cases, the many-tiles case,
the three consumer variants and the two recompute runs): y_hat 2.1e-7, reg 7.0e-8, nll 1.8e-7, group
statistics 1.5e-7, rate mean / std 5.2e-8, |Fa| 5.0e-8, d y0 1.5e-6, ODE weight gradients 4.2e-6,
d W_dec 1.8e-6, d b_dec 1.9e-6 (the largest at S = 2, at R = 49 and on the GST model); the four
configuration-lattice rows added later (tests/lattice_helpers.py) are in the table below, d b_dec 3.5e-6
at lattice_c7_wide the largest of them.
The same chain in torch fp32 on the host is 8e-8 .. 1.8e-6 from fp64 in d y0 and 5e-8 .. 6e-6 in the
weight gradients on these cases, so no bar needed deriving.  nll kernels alone: nll <= 2.3e-7, group
statistics <= 3.0e-8, d y_hat <= 1.9e-7 except 1.5e-3 at R49_T9_S2_B40 (torch fp32: 3.2e-2; some of
its 17,640 two-sample groups are nearly degenerate).  Far-miss group sums: kernel 2.7e-7, the fp64 gradient
rounded to fp32 1.1e-7 (torch's fp32 autograd, which keeps the group mean in fp32: 1.5e-3).

Per case (seed; kink distance, share outside [0, 1], mask distance, smallest group sd of the fp64
reference; then the kernel's errors):
  case               seed  kink    out   mask  min sd | y_hat   nll     stats   d y0    d ode   d W     d b
  FaFp_R1_two_steps   0   1.5e-3  14%   0.68  0.025  | 4.3e-8  1.9e-8  3.0e-8  3.5e-7  3.3e-7  2.2e-7  2.4e-7
  Fp_R1              15   6.9e-2  31%   0.79  0.017  | 5.2e-8  1.4e-7  6.6e-8  1.5e-6  4.2e-6  8.4e-7  4.7e-7
  FaFp_R10            1   1.3e-4  27%   0.67  0.068  | 9.7e-8  1.1e-7  6.0e-8  6.7e-8  1.9e-7  2.0e-7  1.7e-7
  FaFp_R49_split      0   1.6e-3  25%   0.68  0.023  | 2.1e-7  1.2e-7  1.5e-7  7.6e-8  3.0e-7  1.8e-6  1.9e-6
  FaFp_R3_L5          0   2.6e-4  25%   0.52  0.097  | 6.9e-8  1.8e-7  3.9e-8  9.0e-8  1.8e-7  1.4e-7  2.6e-7
  Fa_R1_three_steps   0   4.9e-3   6%   0.80  0.033  | 5.6e-8  1.1e-7  5.0e-8  3.4e-7  3.9e-7  9.4e-8  1.2e-7
  BFaFp_R1            0   2.7e-2  25%   0.78  0.026  | 3.5e-8  7.2e-8  3.3e-8  4.5e-7  3.5e-7  1.7e-7  2.1e-7
  BFaFp_R10_gst       0   5.4e-3  29%   0.72  0.023  | 1.0e-7  1.4e-7  9.3e-8  1.4e-7  2.6e-7  1.7e-6  1.9e-6
  lattice_c1_L3       0   7.1e-2  14%   0.81  0.039  | 3.8e-8  8.1e-8  3.4e-8  3.2e-7  4.4e-7  3.5e-7  4.6e-7
  lattice_c5_R17      0   1.2e-3  25%   0.69  0.059  | 1.5e-7  1.8e-7  1.1e-7  7.3e-8  2.1e-7  5.7e-7  5.5e-7
  lattice_c7_wide     0   3.3e-2  14%   0.65  0.020  | 6.5e-8  9.9e-8  6.0e-8  2.8e-7  2.1e-7  8.2e-7  3.5e-6
  lattice_c12_R40     0   1.2e-2  25%   0.72  0.030  | 2.0e-7  1.3e-7  1.4e-7  5.9e-8  2.7e-7  1.4e-6  1.4e-6
  3073 tiles / 2048   0   6.9e-2  25%   0.78  0.031  | 3.7e-8  8.5e-8  1.8e-8  5.1e-8  1.2e-7  3.0e-8  1.7e-8
Consumer variants (FaFp_R1_two_steps): d y0 1.2e-7 / 1.4e-7 / 1.1e-7, d ode 1.2e-7 / 3.4e-7 / 5.0e-7, d W, d b
exactly zero without a y_hat consumer, else 2.3e-7 / 1.1e-8; static dims of d y0 6.5e-8.  The recompute
runs repeat the stored runs' figures (bit-identical outputs).
"""
import copy

import pytest
import torch

import epilogue_helpers as H
from helpers import normwise_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"

BARS = {"yhat": 1e-5, "reg": 1e-5, "nll": 1e-5, "stats": 1e-5, "mean": 1e-5, "std": 1e-5, "fa_norm": 1e-5,
        "d_y0": 2e-5, "d_ode": 5e-5, "dW": 5e-5, "db": 5e-5}
CASE_IDS = list(H.CHAIN_CASES)
_CASES = {}


def _case(pkg, name):
    """The case and its fp64 forward: computed once, shared by every test that uses it."""
    if name not in _CASES:
        _CASES[name] = H.make_case(pkg, *H.CHAIN_CASES[name])
    return _CASES[name]


def _run(pkg, case, terms, stats_cot=True, budget=None, read_latent=False):
    """One training step's worth of the epilogue path on the device for the loss ``terms`` select
    (epilogue_helpers.reference_chain), under the stored-activation budget ``budget``."""
    from ude_amd import decoder_head, fused, solvers
    R = case.mod.n_regions
    mg = copy.deepcopy(case.mod).to(DEV)
    lin = torch.nn.Linear(3 * R, R)
    with torch.no_grad():
        lin.weight.copy_(case.W)
        lin.bias.copy_(case.b)
    lin = lin.to(DEV)
    y0 = case.y0.to(DEV).requires_grad_(True)
    solvers._PLAN_CACHE.clear()
    fused.ACT_BUDGET = budget
    try:
        mg.clear_tracking()
        if case.bayes:
            mg.set_eps_stream(case.eps.to(DEV))
        assert decoder_head.eligible(mg, y0, lin)
        res = decoder_head.solve_decode(mg, y0, case.t, case.h, lin)
        assert res is not None, "an output time is off the grid: the epilogue did not run"
        yhat, reg, lazy, plan = res
        assert not lazy.materialized
        out = {"plan": plan, "yhat": yhat.detach(), "reg": reg.detach()}
        loss = torch.zeros((), dtype=torch.float64, device=DEV)
        if "nll" in terms:
            nll, stats = decoder_head.nll_head(mg, yhat, case.y.to(DEV), case.S, case.B)
            out["nll"], out["stats"] = nll.detach(), stats.detach().clone()
            loss = loss + H.G_NLL * nll
        if "reg" in terms:
            loss = loss + H.G_REG * reg
        if "yhat" in terms:
            loss = loss + (yhat.double() * case.c_yhat.to(DEV)).sum()
        if "latent" in terms:
            lat = lazy.get()
            out["latent"] = lat.detach()
            loss = loss + (lat.double() * case.dl_full.to(DEV)).sum()
        kind = mg.ode_type
        if kind != "Fa":
            post = mg.posterior()
            out["mean"], out["std"] = post.loc.detach(), post.scale.detach()
            if stats_cot:
                loss = loss + (post.loc.double() * torch.tensor(H.DMEAN, dtype=torch.float64, device=DEV)).sum() \
                    + (post.scale.double() * torch.tensor(H.DSTD, dtype=torch.float64, device=DEV)).sum()
        if kind != "Fp":
            norm = torch.norm(torch.stack(mg.tracker))
            out["fa_norm"] = norm.detach().reshape(1)
            if stats_cot:
                loss = loss + H.DNORM * norm
        loss.backward()
        if read_latent and "latent" not in out:
            with torch.no_grad():
                out["latent"] = lazy.get().detach()
        torch.cuda.synchronize()
    finally:
        fused.ACT_BUDGET = None
        solvers._PLAN_CACHE.clear()
    out["d_y0"] = y0.grad
    if case.bayes:
        mus, sds = mg.ude_mean_std()
        params = mus + sds
    else:
        params = [p for l in mg.ude_linears() for p in (l.weight, l.bias)]
    out["d_ode"] = [p.grad for p in params]
    out["dW"], out["db"] = lin.weight.grad, lin.bias.grad
    out["mod"] = mg
    return out


def _err(got, ref):
    """Normwise error; a reference that is exactly zero (a loss without that term) asks for exact zeros."""
    if got is None:
        got = torch.zeros_like(ref)
    if float(ref.abs().max()) == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else float("inf")
    return normwise_rel(got, ref)


def _check(label, out, ref, keys=None):
    errs = {}
    for k in keys or BARS:
        if k == "d_ode":
            errs[k] = max(_err(g, r) for g, r in zip(out[k], ref[k]))
            assert len(out[k]) == len(ref[k])
        elif k in out and ref.get(k) is not None:
            errs[k] = _err(out[k], ref[k].reshape(out[k].shape) if k in ("reg", "nll", "fa_norm") else ref[k])
    print(f"\n{label}: " + ", ".join(f"{k} {e:.2e} (bar {BARS[k]:.0e})" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if not e <= BARS[k]}
    assert not bad, f"{label}: {bad}"
    return errs


def _n_tiles(case):
    return (case.y0.shape[0] + 15) // 16


# ---- A: the chain, eight models --------------------------------------------------------------------

@pytest.mark.parametrize("name", CASE_IDS)
def test_epilogue_chain_matches_fp64(pkg, name):
    case = _case(pkg, name)
    cond = H.check_conditions(case)
    print(f"\n{name}: seed {H.CHAIN_CASES[name][-1]}, " + ", ".join(f"{k} {v:.3g}" for k, v in cond.items()))
    ref = H.reference_chain(case, {"nll", "reg"})
    out = _run(pkg, case, {"nll", "reg"})
    plan = out["plan"]
    T, div = H.CHAIN_CASES[name][7], H.CHAIN_CASES[name][8]
    assert plan.out_k == [div * j for j in range(T)] and plan.prob.n_steps == div * (T - 1)
    assert plan.prob.recompute == 0
    if name == "FaFp_R49_split":
        # the launch training takes at this size: stored activations, one tile per CU at the most
        # (ude_entry.h launch_forward: SPLIT_FWD && n_tiles <= CUs -> the 8-wave kernel)
        assert plan.sizes.act_bytes > 0
        assert _n_tiles(case) <= torch.cuda.get_device_properties(0).multi_processor_count
    assert tuple(out["stats"].shape) == (T, case.B, case.mod.n_regions, 2)
    _check(name, out, ref)


# ---- B: more tiles than the decoder backward's grid --------------------------------------------------

def test_decoder_backward_item_loop_more_tiles_than_grid(pkg):
    from ude_amd import _native, configs
    cfg = configs._c("Fp", 1, 8, [32, 32], None)
    assert cfg in configs.PREBUILT
    lib, desc = _native.library_for(cfg), _native.make_desc(cfg)
    SLAB = 16 * 16 + 16                                    # LossDims<1>::SLAB = NP * KP + NP
    p = _native.UdeProblem()
    p.n_traj, p.n_steps, p.n_out, p.fa_w, p.recompute = 16 * 1000000, 2, 2, 1.0, 0
    full = int(lib.query(desc, p, torch.cuda.current_device()).dec_ws_bytes) // (4 * SLAB)   # CUs * occupancy
    k = full + full // 2
    while k % 3 or (k + 1) % full == 0:                    # N = 16 k + 3 = 3 B: S = N / 3 samples, B = 3
        k += 1
    N = 16 * k + 3
    case = H.make_case(pkg, "Fp", 1, 8, [32, 32], None, N // 3, 3, 3, 1, 0)
    cond = H.check_conditions(case)
    print(f"\nN = {N}: seed 0, " + ", ".join(f"{k_} {v:.3g}" for k_, v in cond.items()))
    ref = H.reference_chain(case, {"nll", "reg"})
    out = _run(pkg, case, {"nll", "reg"})
    grid = int(out["plan"].sizes.dec_ws_bytes) // (4 * SLAB)
    n_tiles = _n_tiles(case)
    print(f"decoder backward: {n_tiles} tiles on a grid of {grid}")
    assert grid == full and n_tiles > grid and n_tiles % grid != 0 and N % 16 == 3
    _check("more tiles than the grid", out, ref)


# ---- C: one consumer absent, and both consumers ----------------------------------------------------

@pytest.mark.parametrize("terms", [("reg",), ("yhat",), ("yhat", "reg", "latent")], ids=lambda t: "+".join(t))
def test_epilogue_consumers(pkg, terms):
    case = _case(pkg, CASE_IDS[0])
    H.check_conditions(case)
    ref = H.reference_chain(case, terms, stats_cot=False)
    out = _run(pkg, case, terms, stats_cot=False)
    keys = ["yhat", "reg", "mean", "std", "fa_norm", "d_y0", "d_ode", "dW", "db"]
    _check("+".join(terms), out, ref, keys)
    if "latent" in terms:
        assert float(case.dl_full[..., 3:].abs().min()) > 0.0
        assert float(ref["d_y0"][..., 3:].abs().max()) > 0.0
        err = normwise_rel(out["d_y0"][..., 3:], ref["d_y0"][..., 3:])
        print(f"static dims of d y0: {err:.2e} (bar {BARS['d_y0']:.0e})")
        assert err <= BARS["d_y0"]
        mg = out["mod"]
        mg.clear_tracking()
        with torch.no_grad():
            plain = pkg.odeint(mg, case.y0.to(DEV), case.t, method="rk4", options=dict(step_size=case.h))
        assert torch.equal(out["latent"], plain), "materialised latent != the written latent of a plain solve"
        assert normwise_rel(out["latent"], ref["latent"]) <= 1e-5


# ---- D: recompute ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [CASE_IDS[0], CASE_IDS[3]])
def test_epilogue_recompute_bit_identical_and_vs_fp64(pkg, name):
    case = _case(pkg, name)
    H.check_conditions(case)
    ref = H.reference_chain(case, {"nll", "reg"})
    a = _run(pkg, case, {"nll", "reg"}, budget=None, read_latent=True)
    b = _run(pkg, case, {"nll", "reg"}, budget=0, read_latent=True)        # any stored activation exceeds 0 bytes
    assert a["plan"].prob.recompute == 0 and a["plan"].sizes.act_bytes > 0
    assert b["plan"].prob.recompute == 1 and b["plan"].sizes.act_bytes == 0
    for k in ("yhat", "reg", "nll", "stats", "d_y0", "dW", "db", "latent"):
        assert torch.equal(a[k], b[k]), k
    # ODE weight gradients: tests/test_recompute.py:69-77 (the stored path of small records sums the
    # bias rows in another fp32 order)
    for ga, gb in zip(a["d_ode"], b["d_ode"]):
        if case.mod.n_regions <= 16:
            assert normwise_rel(gb, ga) < 1e-6
        else:
            assert torch.equal(ga, gb)
    _check(name + " recompute", b, ref)
    assert normwise_rel(b["latent"], ref["latent"]) <= 1e-5


# ---- E: the nll kernels alone -------------------------------------------------------------------------

_ODES = {}


def _ode(pkg, R):
    """A prebuilt model of R regions: nll_head takes the library and R from its configuration."""
    if R not in _ODES:
        _ODES[R] = pkg.FaFp(3, latent_dim=5, net_sizes=[40, 24], aug_net_sizes=[36]) if R == 3 else \
            pkg.FaFp(R, latent_dim=8, net_sizes=[64, 64, 32], aug_net_sizes=[64, 64])
    return _ODES[R]


def _nll_kernel(pkg, R, yhat, y, S, B, g):
    from ude_amd import decoder_head
    yh = yhat.to(DEV).requires_grad_(True)
    nll, stats = decoder_head.nll_head(_ode(pkg, R), yh, y.to(DEV), S, B)
    (g * nll).backward()
    torch.cuda.synchronize()
    return {"nll": nll.detach().cpu(), "stats": stats.detach().cpu().clone(), "dyhat": yh.grad.cpu()}


NLL_SHAPES = [(1, 3, 2, 5),          # the smallest S
              (10, 5, 7, 3),         # S < 8: the tail loop only
              (49, 4, 9, 7),         # one batch of 8 and a tail
              (3, 6, 200, 3),        # S above the loss head's cap of 128
              (49, 9, 2, 40)]        # 17,640 groups = 69 blocks: the strided finalize


@pytest.mark.parametrize("shape", NLL_SHAPES, ids=lambda s: "R%d_T%d_S%d_B%d" % s)
def test_nll_kernels_match_fp64(pkg, shape):
    R, T, S, B = shape
    yhat, y, g = H.nll_inputs(R, T, S, B, seed=100 + S)
    masked = (y == -1)
    assert 0.1 < float(masked.float().mean()) < 0.6 and bool(masked[0, 0, 0]) and bool(masked[-1, -1, -1]) \
        and bool(masked[:, T // 2].all())
    if (R, S) == (49, 2):
        assert (T * B * R + 255) // 256 > 64
    ref = H.nll_reference(yhat, y, S, B, g)
    r32 = H.nll_reference(yhat, y, S, B, g, torch.float32)
    got = _nll_kernel(pkg, R, yhat, y, S, B, g)
    bad = {}
    for k in ("nll", "stats", "dyhat"):
        e, e32 = normwise_rel(got[k], ref[k]), normwise_rel(r32[k], ref[k])
        bar = max(1e-6, 2.0 * e32)
        print(f"\n{shape} {k}: kernel {e:.2e}, torch fp32 {e32:.2e}, bar {bar:.1e}")
        if not e <= bar:
            bad[k] = (e, bar)
    assert not bad, bad
    # a masked target's group gets no gradient at all
    dg = H.group_view(got["dyhat"], S, B)                                   # (B, S, T, R)
    assert float(dg[masked[:, None].expand_as(dg)].abs().max()) == 0.0
    assert float(dg[~masked[:, None].expand_as(dg)].abs().min()) > 0.0
    again = _nll_kernel(pkg, R, yhat, y, S, B, g)
    for k in got:
        assert torch.equal(got[k], again[k]), k


def test_nll_kernels_all_targets_masked(pkg):
    R, T, S, B = 10, 5, 7, 3
    yhat, y, g = H.nll_inputs(R, T, S, B, seed=5)
    got = _nll_kernel(pkg, R, yhat, torch.full_like(y, -1.0), S, B, g)
    assert float(got["nll"]) == 0.0
    assert float(got["dyhat"].abs().max()) == 0.0
    assert normwise_rel(got["stats"], H.group_stats(yhat.double(), S, B)) <= 1e-6


# ---- F: the cancellation the backward's fp64 re-mean is there for ----------------------------------

def test_nll_backward_far_miss_group_sums(pkg):
    """Groups with sigma = 1e-3 |mu| whose targets lie 30 sigma away: the std term of d nll / d y_hat_s
    is large and sums to zero over a group's samples, so in exact arithmetic the group sum is S * cm
    (ude_loss.h, ude_nll_bwd_kernel).  The kernel's fp32 d y_hat, summed per group in fp64, may deviate
    from the fp64 reference's group sums by at most 4 x what the reference's own d y_hat rounded to fp32
    deviates (about three fp32 roundings per element against one).  A group mean held in fp32 would leave
    S * ulp(mean) * cs in every sum -- about 2e-3 of it here."""
    R, T, S, B = 10, 3, 64, 4
    yhat, y, g = H.nll_inputs(R, T, S, B, seed=9, rel_sigma=(1e-3, 1e-3), offset=(30.0, 30.0), mask=0.0)
    st = H.group_stats(yhat.double(), S, B)
    z = (y.double().permute(1, 0, 2) - st[..., 0]) / st[..., 1]
    assert float((z - 30).abs().max()) < 1e-2 and float((st[..., 1] / st[..., 0]).max()) < 2e-3
    ref = H.nll_reference(yhat, y, S, B, g)
    got = _nll_kernel(pkg, R, yhat, y, S, B, g)

    def sums(d):
        return H.group_view(d.double(), S, B).sum(1)

    want = sums(ref["dyhat"])
    dev_kernel = normwise_rel(sums(got["dyhat"]), want)
    dev_round = normwise_rel(sums(ref["dyhat"].float()), want)
    dev_t32 = normwise_rel(sums(H.nll_reference(yhat, y, S, B, g, torch.float32)["dyhat"]), want)
    print(f"\ngroup sums of d y_hat vs fp64: kernel {dev_kernel:.2e}, fp64 rounded to fp32 {dev_round:.2e} "
          f"(x4 = {4 * dev_round:.2e}), torch fp32 autograd {dev_t32:.2e}")
    assert dev_kernel <= 4.0 * dev_round
    # the same through autograd into a bias: its gradient is the column sums of d y_hat
    from ude_amd import decoder_head
    bias = torch.zeros(R, device=DEV, requires_grad=True)
    nll, _ = decoder_head.nll_head(_ode(pkg, R), yhat.to(DEV) + bias, y.to(DEV), S, B)
    (g * nll).backward()
    e_db = normwise_rel(bias.grad, ref["dyhat"].sum((0, 1)))
    print(f"bias gradient vs fp64: {e_db:.2e} (bar 5e-05)")
    assert e_db <= 5e-5
