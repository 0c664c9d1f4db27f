"""Adaptive dopri5 (torchdiffeq's default method; BASELINE configs[2]).

torchdiffeq is absent (third-party, unvendored, version unpinned): the oracle
(oracle/ude_oracle_dopri5.py) restates its published algorithm and is pinned by
analytic known-answer tests here -- parity w.r.t. torchdiffeq itself is
"unpinned".  The product paths are checked against that oracle:
* eager (ude_amd/adaptive.py, differentiable, any callable): same steps, same
  values to 1e-12 in fp64;
* fused gfx950 forward (GPU): the oracle's step sequence up to rounding (the
  error estimate's last bits feed the next step size), outputs within 1e-5
  normwise of the oracle run at the kernel's precision (fp32) and within the
  solve tolerance of the fp64 oracle; side statistics over every evaluation
  (exact to rounding when the evaluation points coincide).
"""
import numpy as np
import pytest
import torch

from helpers import normwise_rel
from oracle.ude_oracle import OracleRHS
from oracle.ude_oracle_dopri5 import Dopri5Stats, odeint_dopri5

DEV = "cuda"


def _sir_const(beta, gamma):
    def f(t, y):
        S, I = y[..., 0], y[..., 1]
        return torch.stack([-beta * S * I, beta * S * I - gamma * I, gamma * I], -1)
    return f


def test_oracle_linear_ode_matches_expm():
    from scipy.linalg import expm
    A = torch.tensor([[-0.5, 1.0, 0.0], [-1.0, -0.5, 0.2], [0.0, 0.3, -0.1]], dtype=torch.float64)
    y0 = torch.tensor([[1.0, 0.5, -0.3], [0.2, -0.1, 0.7]], dtype=torch.float64)
    t = torch.linspace(0, 3, 7, dtype=torch.float64)
    st = Dopri5Stats()
    sol = odeint_dopri5(lambda tt, y: y @ A.T, y0, t, rtol=1e-10, atol=1e-12, stats=st)
    ref = torch.stack([y0 @ torch.from_numpy(expm(A.numpy() * float(tt))).T for tt in t])
    assert normwise_rel(sol, ref) < 1e-8
    assert st.n_evals == 2 + 6 * st.n_steps
    assert st.n_accepted <= st.n_steps


def test_oracle_sir_matches_solve_ivp_and_tightens_with_rtol():
    from scipy.integrate import solve_ivp
    beta, gamma = 1.7, 0.6
    y0 = torch.tensor([[0.9, 0.05, 0.05]], dtype=torch.float64)
    t = torch.linspace(0, 10, 11, dtype=torch.float64)
    ref = solve_ivp(lambda tt, y: [-beta * y[0] * y[1], beta * y[0] * y[1] - gamma * y[1], gamma * y[1]],
                    (0, 10), y0[0].numpy(), t_eval=t.numpy(), rtol=1e-12, atol=1e-14, method="DOP853").y.T
    errs, steps = [], []
    for rtol in (1e-4, 1e-7, 1e-10):
        st = Dopri5Stats()
        sol = odeint_dopri5(_sir_const(beta, gamma), y0, t, rtol=rtol, atol=rtol * 1e-2, stats=st)
        errs.append(normwise_rel(sol[:, 0], ref))
        steps.append(st.n_accepted)
    assert errs[2] < 1e-8 and errs[1] < errs[0] and errs[2] < errs[1]
    assert steps[0] < steps[1] < steps[2]


def test_oracle_dense_output_matches_step_ends():
    """Outputs requested exactly at accepted step ends equal the interpolant at x=1,
    which reproduces y1 to rounding."""
    beta, gamma = 1.2, 0.4
    y0 = torch.tensor([[0.8, 0.1, 0.1]], dtype=torch.float64)
    st = Dopri5Stats()
    t = torch.tensor([0.0, 5.0], dtype=torch.float64)
    odeint_dopri5(_sir_const(beta, gamma), y0, t, rtol=1e-6, atol=1e-8, stats=st)
    ends = np.cumsum([s[1] for s in st.steps if s[3]])
    t2 = torch.tensor([0.0] + list(ends[:3]), dtype=torch.float64)
    sol_a = odeint_dopri5(_sir_const(beta, gamma), y0, t2, rtol=1e-6, atol=1e-8)
    sol_b = odeint_dopri5(_sir_const(beta, gamma), y0, torch.linspace(0, float(ends[2]), 50, dtype=torch.float64),
                          rtol=1e-6, atol=1e-8)
    assert torch.allclose(sol_a[-1], sol_b[-1], rtol=1e-12, atol=1e-14)


def _module(pkg, kind, R, net, aug, seed=0, L=8):
    torch.manual_seed(seed)
    kw = {}
    if net is not None:
        kw["net_sizes"] = net
    if aug is not None:
        kw["aug_net_sizes"] = aug
    return getattr(pkg, kind)(R, latent_dim=L, **kw)


def _y0(N, R, seed=1, L=8):
    gen = torch.Generator().manual_seed(seed)
    S = torch.rand(N, R, generator=gen) * 0.4 + 0.5
    I = torch.rand(N, R, generator=gen) * 0.05
    return torch.cat([S[..., None], I[..., None], (1 - S - I)[..., None], torch.randn(N, R, L - 3, generator=gen)], -1) \
        + 1e-5


def test_eager_product_matches_oracle(pkg):
    from ude_amd.adaptive import eager_dopri5
    mod = _module(pkg, "FaFp", 1, [64, 64, 32], [64, 64]).double()
    y0 = _y0(20, 1).double()
    t = torch.arange(9, dtype=torch.float32) / 7
    rhs = OracleRHS.from_module(mod, torch.float64)
    st = Dopri5Stats()
    ref = odeint_dopri5(rhs, y0, t, rtol=1e-6, atol=1e-8, stats=st)
    calls = {"n": 0}

    def f(tt, y):
        calls["n"] += 1
        return mod(tt, y)
    out = eager_dopri5(f, y0, t, rtol=1e-6, atol=1e-8)
    assert calls["n"] == st.n_evals
    assert normwise_rel(out, ref) < 1e-12


def test_eager_controller_checks(pkg):
    """torchdiffeq's per-attempt assertions, now read with the error ratio in one host transfer:
    non-finite state, dt underflow (checked first), max_num_steps."""
    from ude_amd.adaptive import eager_dopri5
    f = lambda tt, y: -y
    t = torch.tensor([0.0, 1.0], dtype=torch.float64)
    y_bad = torch.tensor([1.0, float("inf")], dtype=torch.float64)
    with pytest.raises(AssertionError, match="non-finite values in state"):
        eager_dopri5(f, y_bad, t, first_step=0.1)
    with pytest.raises(AssertionError, match="underflow in dt"):
        eager_dopri5(f, y_bad, t + 1.0, first_step=1e-300)
    with pytest.raises(AssertionError, match="underflow in dt"):
        eager_dopri5(lambda tt, y: y * float("nan"), torch.ones(2, dtype=torch.float64), t, first_step=0.1)
    with pytest.raises(AssertionError, match="max_num_steps exceeded"):
        eager_dopri5(f, torch.ones(2, dtype=torch.float64), t, rtol=1e-12, atol=1e-14, max_num_steps=3)
    # the host mirror of t_end stops exactly at the output time
    out = eager_dopri5(f, torch.ones(2, dtype=torch.float64), t, rtol=1e-9, atol=1e-12)
    assert torch.allclose(out[-1], torch.exp(-torch.ones(2, dtype=torch.float64)), rtol=1e-8)


def test_vector_pass_controller_matches_operator_chain(pkg):
    """The controller with ``vec`` (odeint_adjoint's fused path: the stage / error / midpoint
    combinations and the error ratio as single passes) takes the same steps and gives the same outputs
    as torchdiffeq's operator chain, in fp64.  (Folding the whole dense output into one combination of
    the stages was tried and dropped: more accurate in fp32, but it moves the adjoint's segment-end
    states by rounding, which shifts the next segment's adaptive steps -- fused and generic adjoints then
    differ by the solve tolerance, 3.6e-5, instead of agreeing to 1e-5.)"""
    from ude_amd.adaptive import eager_dopri5

    class Vec:
        @staticmethod
        def comb(base, ks, c):
            acc = ks[0] * c[0]
            for j in range(1, len(ks)):
                acc = acc + ks[j] * c[j]
            return acc if base is None else base + acc

        @staticmethod
        def ratio(err, y, y1):
            return (err / (1e-9 + 1e-7 * torch.max(y.abs(), y1.abs()))).pow(2).mean().sqrt()

    A = torch.tensor([[-0.5, 1.0, 0.0], [-1.0, -0.5, 0.2], [0.0, 0.3, -0.1]], dtype=torch.float64)
    calls = {"a": 0, "b": 0}

    def fa(tt, y):
        calls["a"] += 1
        return y @ A.T + torch.sin(tt)

    def fb(tt, y):
        calls["b"] += 1
        return y @ A.T + torch.sin(tt)
    y0 = torch.tensor([[1.0, 0.5, -0.3], [0.2, -0.1, 0.7]], dtype=torch.float64)
    t = torch.tensor([0.0, 0.37, 1.1, 2.9, 3.0], dtype=torch.float64)
    ra = eager_dopri5(fa, y0, t, rtol=1e-7, atol=1e-9)
    rb = eager_dopri5(fb, y0, t, rtol=1e-7, atol=1e-9, vec=Vec)
    assert calls["a"] == calls["b"]
    assert normwise_rel(rb, ra) < 1e-13


def test_host_scalar_controller_matches_eager_cpu(pkg):
    """adaptive.host_scalar_dopri5 (odeint_adjoint's fused backward) against eager_dopri5 with the
    same vector passes, on CPU in fp32: host-mirrored step ends / sizes and fp32 coefficient products,
    the same attempts, bitwise the same outputs (several output times, so several dense outputs); the
    ratio / step-size callback restates ude_dopri_ratio with PyTorch operators, as vec.ratio + the
    eager update form them.  Plus the controller's assertions."""
    from ude_amd.adaptive import eager_dopri5, host_scalar_dopri5, MAX_NUM_STEPS
    A = torch.tensor([[-0.5, 1.0, 0.0], [-1.0, -0.5, 0.2], [0.0, 0.3, -0.1]])
    atol, rtol = 1e-7, 1e-5

    class Vec:
        @staticmethod
        def comb(base, ks, c):
            acc = ks[0] * c[0]
            for j in range(1, len(ks)):
                acc = acc + ks[j] * c[j]
            return acc if base is None else base + acc

        @staticmethod
        def ratio(err, y, y1):
            return (err / (atol + rtol * torch.max(y.abs(), y1.abs()))).pow(2).mean().sqrt().double()

    class HV:
        @staticmethod
        def comb_hc(base, ks, coef):
            return Vec.comb(base, ks, torch.tensor([float(c) for c in coef], dtype=torch.float32))

        @staticmethod
        def ratio_dt(err, y, y1, dt, nonfinite):
            r = Vec.ratio(err, y, y1)
            rf = float(r)
            if rf == 0:
                dtn = torch.tensor(dt, dtype=torch.float64) * 10.0
            else:
                fac = torch.clamp(0.9 / r.to(torch.float64) ** 0.2, min=1.0 if rf < 1 else 0.2, max=10.0)
                dtn = torch.tensor(dt, dtype=torch.float64) * fac
            return rf, float(dtn), bool(nonfinite)

    calls = {"a": 0, "b": 0}

    def fa(tt, y):
        calls["a"] += 1
        return y @ A.T

    def fb(tt, y):
        calls["b"] += 1
        return y @ A.T
    y0 = torch.tensor([[1.0, 0.5, -0.3], [0.2, -0.1, 0.7]])
    t = torch.tensor([0.0, 0.37, 1.1, 2.9, 3.0], dtype=torch.float64)
    ra = eager_dopri5(fa, y0, t, rtol, atol, None, MAX_NUM_STEPS, norm=None, vec=Vec)
    rb = host_scalar_dopri5(fb, y0, t, rtol, atol, None, MAX_NUM_STEPS,
                            lambda v: v.abs().pow(2).mean().sqrt(), HV)
    assert calls["a"] == calls["b"] > 20
    assert torch.equal(ra, rb)
    with pytest.raises(AssertionError, match="underflow in dt"):
        host_scalar_dopri5(fb, y0, t + 1.0, rtol, atol, 1e-300, MAX_NUM_STEPS, None, HV)
    with pytest.raises(AssertionError, match="non-finite values in state"):
        host_scalar_dopri5(fb, y0 * float("inf"), t, rtol, atol, 0.1, MAX_NUM_STEPS, None, HV)
    with pytest.raises(AssertionError, match="max_num_steps exceeded"):
        host_scalar_dopri5(fb, y0, t, rtol, atol, None, 2, lambda v: v.abs().pow(2).mean().sqrt(), HV)


def test_eager_product_is_differentiable(pkg):
    mod = _module(pkg, "Fp", 1, [32, 32], None)
    y0 = _y0(8, 1).requires_grad_(True)
    lat = pkg.odeint(mod, y0, torch.arange(4, dtype=torch.float32), rtol=1e-5, atol=1e-7)
    lat.sum().backward()
    assert torch.isfinite(y0.grad).all() and y0.grad.abs().sum() > 0


# ---------------------------------------------------------------------------
# GPU: fused forward
# ---------------------------------------------------------------------------
CASES = [
    # kind, R, net, aug, N, T, div, rtol, atol
    ("FaFp", 1, [64, 64, 32], [64, 64], 100, 9, 7.0, 1e-5, 1e-7),
    ("FaFp", 1, [64, 64, 32], [64, 64], 33, 29, 7.0, 1e-7, 1e-9),      # torchdiffeq defaults, daily grid
    ("Fp", 1, [32, 32], None, 64, 9, 1.0, 1e-6, 1e-8),
    ("Fa", 1, None, [64, 64], 17, 6, 7.0, 1e-6, 1e-8),
    ("FaFp", 10, [64, 64, 32], [64, 64], 40, 5, 5.0, 1e-6, 1e-8),
    ("FaFp", 49, [64, 64, 32], [64, 64], 24, 3, 2.0, 1e-6, 1e-8),
    # the configuration lattice (tests/lattice_helpers.py c1, c5, c7; a tenth entry is the latent dim)
    ("Fp", 1, [32, 32], None, 37, 5, 7.0, 1e-6, 1e-8, 3),
    ("FaFp", 17, [64, 64, 32], [64, 64], 37, 5, 7.0, 1e-6, 1e-8),
    ("FaFp", 1, [128, 128, 128], [128, 128], 37, 5, 7.0, 1e-6, 1e-8),
]
# Horizons stop before the random-weight models drive a state across the [-1, 2]
# mask (lib/models.py:130): the RHS is discontinuous there, the controller rejects
# steps until it straddles the jump, and where it lands depends on rounding -- the
# solutions then agree only to ~1e-4 (the last test below).


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}_R{c[1]}_N{c[4]}_T{c[5]}_rtol{c[7]:g}")
def test_fused_dopri5_matches_oracle(pkg, case):
    kind, R, net, aug, N, T, div, rtol, atol = case[:9]
    L = case[9] if len(case) > 9 else 8
    mod = _module(pkg, kind, R, net, aug, L=L)
    if kind == "FaFp":
        mod.Fa_w = 0.8
    y0 = _y0(N, R, L=L)
    t = torch.arange(T, dtype=torch.float32) / div
    rhs32 = OracleRHS.from_module(mod, torch.float32)
    st32 = Dopri5Stats()
    ref32 = odeint_dopri5(rhs32, y0, t, rtol=rtol, atol=atol, stats=st32)
    rhs64 = OracleRHS.from_module(mod, torch.float64)
    st64 = Dopri5Stats()
    ref64 = odeint_dopri5(rhs64, y0.double(), t, rtol=rtol, atol=atol, stats=st64)
    mg = mod.to(DEV)
    mg.clear_tracking()
    with torch.no_grad():
        lat = pkg.odeint(mg, y0.to(DEV), t.to(DEV), rtol=rtol, atol=atol, method="dopri5")
    info = mg.last_solve_info
    # The step sequence is the oracle's up to rounding: the error estimate of a step is a
    # sum of cancelling terms, so its last bits (and, through er^(1/5), the next dt's) are
    # implementation dependent -- the torchdiffeq CPU and GPU runs differ the same way.
    assert abs(info["n_steps"] - st32.n_steps) <= max(1, st32.n_steps // 10)
    assert info["n_evals"] == (2 + 6 * info["n_steps"])
    assert normwise_rel(lat, ref32) < 1e-5
    assert normwise_rel(lat, ref64) < max(50 * rtol, 1e-5)
    assert torch.equal(lat[:, :, :, 3:].cpu(), y0[None, :, :, 3:].expand(T, -1, -1, -1))
    # side statistics average over the solver's evaluation points, which move with the
    # step sequence: equal to 2e-3 (same points: 1e-6, see the fixed-step case below)
    if kind != "Fa":
        post = mg.posterior()
        p = torch.stack(rhs32.params).reshape(-1, 2).double()
        assert normwise_rel(post.loc, p.mean(0)) < 2e-3 and normwise_rel(post.scale, p.std(0)) < 2e-2
    if kind != "Fp":
        nrm = torch.norm(torch.stack(mg.tracker))
        assert normwise_rel(nrm, torch.norm(torch.stack(rhs32.tracker).double())) < 2e-3 * (1 + abs(
            info["n_evals"] - st32.n_evals))


@pytest.mark.gpu
def test_fused_dopri5_one_step_stats_exact(pkg):
    """One accepted step from a given first step: the evaluation points are the
    oracle's, so the side statistics agree to rounding."""
    import copy
    mod = _module(pkg, "FaFp", 1, [64, 64, 32], [64, 64])
    mod.Fa_w = 0.8
    y0 = _y0(48, 1)
    t = torch.tensor([0.0, 0.01])
    rhs = OracleRHS.from_module(mod, torch.float32)
    st = Dopri5Stats()
    ref = odeint_dopri5(rhs, y0, t, rtol=1e-5, atol=1e-7, first_step=0.05, stats=st)
    mg = copy.deepcopy(mod).to(DEV)
    mg.clear_tracking()
    with torch.no_grad():
        lat = pkg.odeint(mg, y0.to(DEV), t.to(DEV), rtol=1e-5, atol=1e-7, method="dopri5",
                         options=dict(first_step=0.05))
    assert mg.last_solve_info["n_evals"] == st.n_evals == 7
    assert normwise_rel(lat, ref) < 1e-6
    p = torch.stack(rhs.params).reshape(-1, 2).double()
    post = mg.posterior()
    assert normwise_rel(post.loc, p.mean(0)) < 1e-6 and normwise_rel(post.scale, p.std(0)) < 1e-5
    nrm = torch.norm(torch.stack(mg.tracker))
    assert normwise_rel(nrm, torch.norm(torch.stack(rhs.tracker).double())) < 1e-6


@pytest.mark.gpu
def test_fused_dopri5_first_step_and_max_steps(pkg):
    mod = _module(pkg, "FaFp", 1, [64, 64, 32], [64, 64]).to(DEV)
    y0 = _y0(32, 1).to(DEV)
    t = torch.arange(5, dtype=torch.float32).to(DEV)
    with torch.no_grad():
        mod.clear_tracking()
        pkg.odeint(mod, y0, t, method="dopri5", options=dict(first_step=0.05))
        assert mod.last_solve_info["n_evals"] == 1 + 6 * mod.last_solve_info["n_steps"]
        mod.clear_tracking()
        with pytest.raises(AssertionError):
            pkg.odeint(mod, y0, t, method="dopri5", rtol=1e-12, atol=1e-14, options=dict(max_num_steps=3))


@pytest.mark.gpu
def test_fused_dopri5_through_mask_discontinuity(pkg):
    """Past t ~ 1 some states of these random models cross the mask bound and the RHS
    jumps: many rejected steps; the kernel and the oracle straddle the jump at
    rounding-dependent places, so only ~1e-4 agreement is meaningful."""
    import copy
    mod = _module(pkg, "FaFp", 10, [64, 64, 32], [64, 64])
    mod.Fa_w = 0.8
    y0 = _y0(40, 10)
    t = torch.arange(5, dtype=torch.float32)
    rhs = OracleRHS.from_module(mod, torch.float32)
    st = Dopri5Stats()
    ref = odeint_dopri5(rhs, y0, t, rtol=1e-6, atol=1e-8, stats=st)
    mg = copy.deepcopy(mod).to(DEV)
    mg.clear_tracking()
    with torch.no_grad():
        lat = pkg.odeint(mg, y0.to(DEV), t.to(DEV), rtol=1e-6, atol=1e-8, method="dopri5")
    info = mg.last_solve_info
    assert info["n_accepted"] < info["n_steps"]                 # rejections happened
    assert abs(info["n_steps"] - st.n_steps) <= 0.25 * st.n_steps
    assert normwise_rel(lat, ref) < 1e-3
