"""The fused kernels across the model-configuration lattice (tests/lattice_helpers.py: one configuration
per combination of csrc/ude_model.h's compile-time traits that configs.PREBUILT does not reach).

Every deterministic case, on the full-step grid and on the three-quarter step (interpolated outputs):
* forward bit for bit against the kernel-order restatement (latent, every stage input, the statistics)
  and backward against the restatement's exact VJP within max(1e-6, 2 x one fp32 execution)
  (kernel_order_helpers._check, as tests/test_kernel_order.py);
* independently against solve_and_grad in fp64 within max(project floor, 2 x the oracle's own
  fp32-vs-fp64 distance): floors 1e-5 latent / mean / std / |Fa|, 2e-5 dy0, 5e-5 weights;
* the planted off-mask components stay exactly at their initial values; static dims are carried bit-unchanged.
Recompute view (fused.ACT_BUDGET = 0): latent / dy0 bit-identical to the stored solve, weight gradients
bit-identical where Model::SPLIT_BWD is off (read from the header's printed traits), within 1e-6 otherwise.
One evaluation + VJP through the module call against fp64 at 1e-5, with all three cotangents and with
f's only (the adjoint's case).  More tiles than workgroups (c4, c5, c7): N = 16 * 2 * CUs + 21 over two
steps against solve_and_grad_chunked at the same bars; the first 37 trajectories solved alone give
bit-identical latent.

Decoder epilogue and forecast (c1, c5, c7, c12; their training chain runs as rows of
epilogue_helpers.CHAIN_CASES in tests/test_decoder_epilogue.py): the inference solve bit for bit against
the training decoder forward, the dynamics channels against the evaluation kernel.  dopri5 (c1, c5, c7) and
the Bayesian cases b1 / b2 run as rows of tests/test_dopri5.py and tests/test_bayes.py.

The JIT libraries of all lattice configurations are built once, in parallel (_native.jit_prebuild).
The margin condition every comparison rests on is asserted by lattice_helpers.references (and by
tests/test_config_lattice.py on the CPU)."""
import copy

import pytest
import torch

import epilogue_helpers as H
import lattice_helpers as lh
from helpers import kernel_forward_store, normwise_rel
from kernel_order_helpers import DEV, _check, _gpu_vjp
from oracle.ude_oracle import OracleRHS, solve_and_grad_chunked
from test_decoder_epilogue import _case as _chain_case
from test_dynamics import GAMMA_MIN
from test_dynamics_gpu import _check_against_evaluation_kernel, _check_r_eff_is_one_division, _solve_both
from test_eval_rhs import _x
from test_forecast_gpu import _assert_same, _both_solves
from test_recompute import _solve

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def lattice_libraries():
    """The lattice's JIT libraries, compiled in parallel before the first test needs one."""
    lh.jit_prebuild()


def _names(mod):
    """oracle gradient names in ude_linears order: rate net, then augmentation net"""
    rhs = OracleRHS.from_module(mod)
    return [("p", i) for i in range(len(rhs.p_w))] + [("a", i) for i in range(len(rhs.a_w))]


def _against_fp64(label, refs_bar, ref, lat, stats, got, mod):
    """kernel outputs against an fp64 SolveResult; refs_bar(key) is the bar.  Prints every figure first."""
    errs = {"latent": normwise_rel(lat, ref.latent)}
    for key, val in zip(("mean", "std", "fa_norm"), stats):
        if getattr(ref, key) is not None:
            errs[key] = normwise_rel(val, getattr(ref, key))
    errs["y0"] = normwise_rel(got["y0"], ref.grads["y0"])
    for i, (net, j) in enumerate(_names(mod)):
        errs[f"{net}_w{j}"] = normwise_rel(got[("w", i)], ref.grads[f"{net}_w{j}"])
        errs[f"{net}_b{j}"] = normwise_rel(got[("b", i)], ref.grads[f"{net}_b{j}"])
    wk = [k for k in errs if "_w" in k or "_b" in k]
    worst = max(wk, key=lambda k: errs[k] / refs_bar(k))
    print(f"{label}: kernel vs fp64 [bar]: " + ", ".join(f"{k} {errs[k]:.1e} [{refs_bar(k):.1e}]"
          for k in errs if k not in wk) + f", weights worst {worst} {errs[worst]:.1e} [{refs_bar(worst):.1e}]")
    over = {k: (v, refs_bar(k)) for k, v in errs.items() if v > refs_bar(k)}
    assert not over, f"{label}: kernel vs fp64 above the bar: {over}"


@pytest.mark.parametrize("which", lh.GRIDS)
@pytest.mark.parametrize("case", lh.DET)
def test_lattice_solve(pkg, case, which):
    refs = lh.references(case, which)                          # asserts the margin condition
    cfg, inp = refs.cfg, refs.inp
    R = cfg[1]
    mod = lh.module_for(pkg, cfg)
    _check(pkg, mod, inp.y0, inp.t, inp.dl, f"{case} {which}", inp.h)
    mod = mod.to(DEV)
    lat, _X, stats = kernel_forward_store(pkg, mod, inp.y0, inp.t, inp.h)
    _lat, got = _gpu_vjp(pkg, mod, inp.y0, inp.t, inp.dl, inp.h)
    assert torch.equal(_lat, lat)
    _against_fp64(f"{case} {which}", lambda k: lh.bar(refs, k), refs.ref, lat, stats, got, mod)
    for (n, r, c), _v in lh.planted_values(R):
        assert torch.equal(lat[:, n, r, c], inp.y0[n, r, c].expand(len(inp.t))), (n, r, c, lat[:, n, r, c])
    assert torch.equal(lat[..., 3:], inp.y0[..., 3:].expand(len(inp.t), -1, -1, -1)), "static dims changed"


@pytest.mark.parametrize("case", lh.DET)
def test_lattice_recompute_view(pkg, case):
    cfg = lh.LATTICE[case]
    inp = lh.inputs(cfg)
    mg = lh.module_for(pkg, cfg).to(DEV)
    y0, dl = inp.y0.to(DEV), inp.dl.float().to(DEV)
    a = _solve(pkg, mg, y0, inp.t, dl, None)
    b = _solve(pkg, mg, y0, inp.t, dl, 0)
    assert a[0] == 0 and a[1] > 0, "default plan stores activations"
    assert b[0] == 1 and b[1] == 0, "a zero budget selects the recompute path"
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), "latent / dy0 differ"
    split = lh.split_bwd(cfg)
    for i, (ga, gb) in enumerate(zip(a[4], b[4])):
        if split:
            assert normwise_rel(gb, ga) < 1e-6, (i, normwise_rel(gb, ga))
        else:
            assert torch.equal(ga, gb), (i, normwise_rel(gb, ga))


@pytest.mark.parametrize("only_f", [False, True], ids=["all_cotangents", "f_only"])
@pytest.mark.parametrize("case", lh.DET)
def test_lattice_eval_and_vjp(pkg, case, only_f):
    kind, R, L, _net, _aug = cfg = lh.LATTICE[case]
    mod = lh.module_for(pkg, cfg)
    N = 45
    x = _x(N, R, L, 100 + R)
    g = torch.Generator().manual_seed(5)
    cf, cr, ca = torch.randn(N, R, L, generator=g), torch.randn(N, R, 2, generator=g), torch.randn(N, R, 3, generator=g)
    ref = OracleRHS.from_module(mod, torch.float64).requires_grad_()
    xr = x.double().requires_grad_(True)
    f_ref = ref(0.0, xr)
    loss = (f_ref * cf.double()).sum()
    if kind != "Fa" and not only_f:
        loss = loss + (ref.params[0] * cr.double()).sum()
    if kind != "Fp" and not only_f:
        loss = loss + (ref.tracker[0] * ca.double()).sum()
    gr = torch.autograd.grad(loss, [xr] + ref.weights())
    mg = mod.to(DEV)
    mg.clear_tracking()
    xg = x.to(DEV).requires_grad_(True)
    f = mg(0.0, xg)
    loss = (f * cf.to(DEV)).sum()
    if kind != "Fa":
        assert normwise_rel(mg.params[0], ref.params[0]) < 1e-5
        if not only_f:
            loss = loss + (mg.params[0] * cr.to(DEV)).sum()
    if kind != "Fp":
        assert normwise_rel(mg.tracker[0], ref.tracker[0]) < 1e-5
        if not only_f:
            loss = loss + (mg.tracker[0] * ca.to(DEV)).sum()
    assert normwise_rel(f, f_ref) < 1e-5
    assert torch.equal(f[..., 3:].cpu(), torch.zeros(N, R, L - 3))
    assert float(f[1, 0, 1].detach()) == 0.0 and float(f[2, -1, 2].detach()) == 0.0
    params = [p for lin in mg.ude_linears() for p in (lin.weight, lin.bias)]
    gk = torch.autograd.grad(loss, [xg] + params)
    errs = [normwise_rel(a, b) for a, b in zip(gk, gr)]
    print(f"{case} eval: f {normwise_rel(f, f_ref):.1e}, dx {errs[0]:.1e}, weights <= {max(errs[1:]):.1e}")
    assert errs[0] < 1e-5, ("dx", errs[0])
    for i, e in enumerate(errs[1:]):
        assert e < 1e-5, (i, e)


@pytest.mark.parametrize("case", ["c4", "c5", "c7"])
def test_lattice_more_tiles_than_workgroups(pkg, case):
    """N = 16 * 2 * CUs + 21 trajectories (more tiles than two workgroups per CU, a ragged last tile) over
    two steps: c4's plain (non-split) training forward and the large-record kernels' tile loops."""
    kind = (cfg := lh.LATTICE[case])[0]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 16 * 2 * cus + 21
    mod, y0, t, h, dl = lh.large_batch(pkg, cfg, N)               # asserts the margin and kink conditions
    dm, ds, dn = lh._cots(kind)
    r64 = OracleRHS.from_module(mod, torch.float64)
    ref = solve_and_grad_chunked(r64, y0.double(), t, h, dl, dm, ds, dn, chunk=2048)
    r32 = solve_and_grad_chunked(OracleRHS.from_module(mod, torch.float32), y0, t, h, dl.float(),
                                 None if dm is None else dm.float(), None if ds is None else ds.float(), dn,
                                 chunk=2048)
    d32 = {"latent": normwise_rel(r32.latent, ref.latent)}
    for key in ("mean", "std", "fa_norm"):
        if getattr(ref, key) is not None:
            d32[key] = normwise_rel(getattr(r32, key), getattr(ref, key))
    d32.update({k: normwise_rel(r32.grads[k], v) for k, v in ref.grads.items()})
    bar = lambda k: max(lh.FLOORS.get(k, lh.FLOOR_W), 2.0 * d32.get(k, 0.0))
    mg = mod.to(DEV)
    lat, _X, stats = kernel_forward_store(pkg, mg, y0, t, h)
    _lat, got = _gpu_vjp(pkg, mg, y0, t, dl, h)
    assert torch.equal(_lat, lat)
    _against_fp64(f"{case} N={N}", bar, ref, lat, stats, got, mg)
    mg = mod.to(DEV)
    lat37, _X, _s = kernel_forward_store(pkg, mg, y0[:lh.N_TRAJ], t, h)
    assert torch.equal(lat37, lat[:, :lh.N_TRAJ]), "the first 37 trajectories differ when solved alone"


@pytest.mark.parametrize("name", [n for n in H.CHAIN_CASES if n.startswith("lattice_")])
def test_lattice_forecast_solve_and_dynamics(pkg, name):
    case = _chain_case(pkg, name)
    H.check_conditions(case)
    R = case.mod.n_regions
    ode = copy.deepcopy(case.mod).to(DEV)
    lin = torch.nn.Linear(3 * R, R)
    with torch.no_grad():
        lin.weight.copy_(case.W)
        lin.bias.copy_(case.b)
    lin = lin.to(DEV)
    y0 = case.y0.to(DEV)
    _assert_same(_both_solves(ode, y0, case.t, case.h, lin))
    with torch.no_grad():                                   # gamma away from 0, as the dynamics fixtures
        last = (ode.net if hasattr(ode, "net") else ode.Fp_net)[-1]
        last.weight.mul_(0.1)
        last.bias.copy_(torch.tensor([0.8, 0.55]).repeat(R))
    dyn, names, latent = _solve_both(pkg, ode, y0, case.t, case.h, lin)
    assert float(dyn[names.index("gamma")].min()) >= GAMMA_MIN
    _check_r_eff_is_one_division(dyn, names)
    _check_against_evaluation_kernel(ode, dyn, names, latent)
