"""The model-configuration lattice (tests/test_config_lattice.py, tests/test_config_lattice_gpu.py).

csrc/ude_model.h turns a configuration (kind, R, L, net, aug) into compile-time traits that select
different kernel code (wave roles, LDS layouts, weight residency).  ``LATTICE`` holds one
configuration per trait combination that ``configs.PREBUILT`` does not reach; ``EXPECTED`` is the
trait vector each was chosen for, asserted against the header itself through
tests/native/ude_traits.cpp, so a moved threshold fails a test instead of emptying a lattice cell.

Every case runs the same inputs (``inputs``): N = 37 (three tiles, the last with five
trajectories), y0 by the suite's rule with three planted states outside the [-1, 2] mask, the grid
t = arange(5) / 7 solved at the full step and at three quarters of it (interpolated outputs).
``references`` is the fp64 oracle of a case and grid, computed once and shared; it asserts the
condition every comparison rests on: each trajectory's closest approach of S, I, R to the mask
bounds over all stage inputs is >= ``MARGIN``, and exactly the planted trajectories take masked
decisions -- so no fp32 execution can take another branch than the fp64 one."""
import functools
import os
import subprocess
from types import SimpleNamespace

import torch

from conftest import REPO, import_pkg

import_pkg()                                         # puts ude_amd on sys.path
from ude_amd import configs  # noqa: E402
from oracle.ude_oracle import OracleRHS, make_grid, normwise_rel, odeint_rk4, solve_and_grad  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(REPO, "forecasting-influenza-using-universal-differential-equations_amd", "csrc")
TRAITS_SRC = os.path.join(HERE, "native", "ude_traits.cpp")
TRAITS_DIR = os.path.join(HERE, "native", "_build", "traits")

_c = configs._c
LATTICE = {
    "c1": _c("Fp", 1, 3, [32, 32], None),
    "c2": _c("FaFp", 1, 16, [20, 20], [32, 32]),
    "c3": _c("FaFp", 5, 4, [24], [36]),
    "c4": _c("FaFp", 16, 8, [64, 64, 32], [64, 64]),
    "c5": _c("FaFp", 17, 8, [64, 64, 32], [64, 64]),
    "c6": _c("Fp", 33, 8, [64, 64, 32], None),
    "c7": _c("FaFp", 1, 8, [128, 128, 128], [128, 128]),
    "c8": _c("FaFp", 2, 8, [48, 40, 24, 20], [56, 36, 20, 12]),
    "c9": _c("FaFp", 3, 8, [64, 64, 32, 16], [20]),
    "c10": _c("Fa", 10, 5, None, [100]),
    "c11": _c("FaFp", 10, 8, [128, 64], [128, 64]),
    "c12": _c("FaFp", 40, 8, [128, 128, 64], [128, 128]),
    "b1": _c("BFp", 3, 5, [40, 24], None),
    "b2": _c("BFaFp", 5, 8, [64, 64, 32], [64, 64]),
}
DET = [k for k in LATTICE if k.startswith("c")]
BAYES = [k for k in LATTICE if k.startswith("b")]

# what each case is the first to run (the issue's table), as values of ude_model.h's traits
EXPECTED = {
    "c1": dict(SLOTS=1, HOIST=0, STORE_ACT=1, SPLIT_FWD=1, SPLIT_BWD=1, SPLITX0=1, DYF=1, WREG=1, FWD_RES=0, D=3),
    "c2": dict(SLOTS=1, HOIST=1, L=16, STORE_ACT=1, SPLIT_BWD=1, SPLITX0=1, DYF=1, WREG=1, D=3),
    "c3": dict(SLOTS=1, HOIST=1, F=15, D=2, STORE_ACT=1, SPLIT_BWD=1, SPLITX0=1, DYF=1, WREG=1),
    "c4": dict(SLOTS=1, F=48, F16=48, STORE_ACT=1, SPLIT_FWD=1, SPLIT_BWD=1, SPLITX0=1, DYF=1, WREG=1, D=4),
    "c5": dict(SLOTS=2, STORE_ACT=0, STORE_ACT_D=1, SPLIT_FWD=0, SPLIT_BWD=0, SPLIT_BWD_L=1, SPLITX0=0, DYF=0,
               WREG=1, FWD_RES=0),
    "c6": dict(SLOTS=3, KIND=1, STORE_ACT_D=1, SPLIT_BWD_L=1, SPLITX0=0, DYF=0),
    "c7": dict(SLOTS=1, ACT_A4=672, STORE_ACT=0, STORE_ACT_D=1, SPLIT_FWD=0, SPLIT_BWD=0, SPLIT_BWD_L=1,
               SPLITX0=1, DYF=1, WREG=0, FWD_RES=1),
    "c8": dict(SLOTS=1, D=5, STORE_ACT=1, SPLIT_BWD=1),
    "c9": dict(SLOTS=1, D=5, STORE_ACT=1, SPLIT_BWD=1),
    "c10": dict(SLOTS=1, KIND=2, L=5, STORE_ACT=1, SPLIT_BWD=1, SPLITX0=1, DYF=0, D=2),
    "c11": dict(SLOTS=1, STORE_ACT=1, SPLIT_FWD=1, SPLIT_BWD=1, WREG=0, FWD_RES=1),
    "c12": dict(SLOTS=3, STORE_ACT_D=1, SPLIT_BWD_L=1, WREG=0, FWD_RES=0, LDS_B=150336),
    "b1": dict(BAYES=1, FULL0=1, HOIST=0, L=5, GST=0, FWD_PFB=1),
    "b2": dict(BAYES=1, FULL0=1, GST=1, SPLIT_FWD=0, R=5),
}
BOOL_TRAITS = ("HOIST", "STORE_ACT", "STORE_ACT_D", "SPLIT_FWD", "SPLIT_BWD", "SPLIT_BWD_L", "SPLITX0", "DYF",
               "WREG", "FWD_RES")

N_TRAJ = 37
PLANTED = (0, 1, 36)
MARGIN = 0.1
FA_W = 0.7
DM = torch.tensor([0.3, -0.2], dtype=torch.float64)
DS = torch.tensor([0.5, 0.1], dtype=torch.float64)
DN = 0.1
GRIDS = ("full", "three_quarter")
FLOORS = {"latent": 1e-5, "mean": 1e-5, "std": 1e-5, "fa_norm": 1e-5, "y0": 2e-5}
FLOOR_W = 5e-5


class TraitError(RuntimeError):
    """ude_model.h refuses the configuration (a static_assert): the message carries the compiler's reason."""


@functools.lru_cache(maxsize=None)
def traits(cfg):
    """{trait name: int} of ude_model.h for cfg, from the host program tests/native/ude_traits.cpp (compiled
    per configuration, g++, rebuilt when the header or the program is newer)."""
    exe = os.path.join(TRAITS_DIR, "traits_" + configs.config_key(cfg))
    newest = max(os.path.getmtime(TRAITS_SRC), os.path.getmtime(os.path.join(CSRC, "ude_model.h")))
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        os.makedirs(TRAITS_DIR, exist_ok=True)
        tmp = f"{exe}.{os.getpid()}.tmp"
        r = subprocess.run(["g++", "-std=c++17", "-O0", "-I", CSRC, f"-DUDE_ONE_CONFIG={configs.template_args(cfg)}",
                            TRAITS_SRC, "-o", tmp], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise TraitError(r.stdout[-4000:])
        os.replace(tmp, exe)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}


def split_bwd(cfg) -> bool:
    """Whether cfg's stored backward is the 8-wave split kernel of small records (Model::SPLIT_BWD), whose
    partner waves sum the weight gradients in another fp32 order than the 4-wave recompute kernel."""
    return bool(traits(cfg)["SPLIT_BWD"])


def module_for(pkg, cfg):
    """The deterministic module of cfg: torch.manual_seed(0), default init, Fa_w = 0.7."""
    kind, R, L, net, aug = cfg
    torch.manual_seed(0)
    kw = {}
    if net is not None:
        kw["net_sizes"] = list(net)
    if aug is not None:
        kw["aug_net_sizes"] = list(aug)
    mod = getattr(pkg, kind)(R, latent_dim=L, **kw)
    if kind == "FaFp":
        mod.Fa_w = FA_W
    return mod


def y0_for(R, L, N=N_TRAJ, seed=1):
    """(y0 (N, R, L) fp32 by the suite's rule with the three planted off-mask states, the generator after it)."""
    gen = torch.Generator().manual_seed(seed)
    S = torch.rand(N, R, generator=gen) * 0.4 + 0.5
    I = torch.rand(N, R, generator=gen) * 0.05
    y0 = torch.cat([S[..., None], I[..., None], (1 - S - I)[..., None], torch.randn(N, R, L - 3, generator=gen)], -1)
    y0 = y0 + 1e-5
    y0[0, 0, 0] = 2.5
    y0[1, R - 1, 2] = -1.2
    y0[N_TRAJ - 1, 0, 1] = 2.25
    return y0, gen


def planted_values(R):
    return (((0, 0, 0), 2.5), ((1, R - 1, 2), -1.2), ((N_TRAJ - 1, 0, 1), 2.25))


def grid(which):
    """(t, step_size): t = arange(5) / 7 at its own step, or at three quarters of it (interpolated outputs)."""
    t = torch.arange(5, dtype=torch.float32) / 7.0
    h = t[1] - t[0]
    return t, (h if which == "full" else h * 0.75)


def inputs(cfg, which="full"):
    """y0, t, step_size, dlatent (fp64) of a lattice case."""
    _kind, R, L, _net, _aug = cfg
    y0, gen = y0_for(R, L)
    t, h = grid(which)
    dl = torch.randn((len(t), N_TRAJ, R, L), generator=gen, dtype=torch.float64)
    return SimpleNamespace(y0=y0, t=t, h=h, dl=dl)


def check_condition(margin, masks, label):
    """margin (N,), masks (E, N, R, 3) of one solve: every trajectory >= MARGIN from the mask bounds at every
    stage input, and exactly the planted trajectories masked."""
    assert float(margin.min()) >= MARGIN, (label, float(margin.min()), int(margin.argmin()))
    masked = masks.reshape(masks.shape[0], masks.shape[1], -1).any(2).any(0).nonzero().flatten().tolist()
    assert masked == list(PLANTED), (label, masked)


def record_condition(rhs, y0, t, h):
    """(margin (N,), masks (E, N, R, 3)) of the solve of rhs (any callable RHS, any dtype): the lib/models.py:130
    decisions (x > 2) | (x < -1) on S, I, R of every stage input and their distance to those bounds."""
    margins, masks = [], []

    def f(tt, x):
        xs = x[..., :3]
        masks.append((xs > 2) | (xs < -1))
        margins.append(torch.minimum((xs - 2).abs(), (xs + 1).abs()).reshape(x.shape[0], -1).amin(1))
        return rhs(tt, x)
    rhs.clear_tracking()
    with torch.no_grad():
        odeint_rk4(f, y0, t, h)
    rhs.clear_tracking()
    return torch.stack(margins).amin(0), torch.stack(masks)


def rate_kink(rhs, y0, t, h):
    """(N,) each trajectory's smallest |q| over every evaluation and region, q the rate net's output before the
    |.| of lib/models.py:134 (OracleRHS, any dtype); None without a rate net.  d|q|/dq flips sign at q = 0, so a
    rate that fp32 rounding (~1e-7 here: K <= 136 products of O(0.1 .. 1)) carries across it gives another
    gradient than fp64 -- a branch difference like the mask's, not a rounding error."""
    if rhs.kind == "Fa":
        return None
    out = []

    def f(tt, x):
        q = rhs._mlp(x.reshape(x.shape[0], -1), rhs.p_w, rhs.p_b, rhs.p_act)
        out.append(q.abs().amin(1))
        return rhs(tt, x)
    rhs.clear_tracking()
    with torch.no_grad():
        odeint_rk4(f, y0, t, h)
    rhs.clear_tracking()
    return torch.stack(out).amin(0)


KINK = 1e-6          # tests/test_full_size.py's distance of a rate from the kink of |.|: 10 x its fp32 rounding


def large_batch(pkg, cfg, N):
    """A batch of N trajectories over two steps of 1/7 for the more-tiles-than-workgroups tests: y0 by the
    suite's rule (seed 1) with the planted states; a trajectory one of whose rates comes within KINK of zero in
    the fp64 oracle (a few dozen of 8,000 x 17 regions x 2 rates x 8 evaluations) is drawn again from the next
    seed until none is left -- N, and so the tile count, stay as they are.  Asserts the margin condition and
    the kink distance.  -> (mod, y0, t, h, dlatent fp64)"""
    _kind, R, L, _net, _aug = cfg
    mod = module_for(pkg, cfg)
    r64 = OracleRHS.from_module(mod, torch.float64)
    y0, gen = y0_for(R, L, N)
    t = torch.arange(3, dtype=torch.float32) / 7.0
    h = t[1] - t[0]
    dl = torch.randn((len(t), N, R, L), generator=gen, dtype=torch.float64)
    seed = 1
    while True:
        kink = rate_kink(r64, y0.double(), t, h)
        if kink is None or float(kink.min()) >= KINK:
            break
        seed += 1
        assert seed < 10, float(kink.min())
        bad = kink < KINK
        y0[bad] = y0_for(R, L, N, seed)[0][bad]
    margin, masks = record_condition(r64, y0.double(), t, h)
    check_condition(margin, masks, ("large batch", cfg))
    return mod, y0, t, h, dl


def _cots(kind):
    return (DM if kind != "Fa" else None, DS if kind != "Fa" else None, DN if kind != "Fp" else None)


@functools.lru_cache(maxsize=None)
def references(case, which):
    """The fp64 oracle of a deterministic lattice case on one grid, shared by every test (read only):
    .ref (SolveResult with grads), .margin / .masks, .kink, .ref32 ({key: the oracle's own fp32-vs-fp64
    distance}), .inp.  Asserts the margin condition, and that every rate keeps KINK from the kink of |.|
    (rate_kink), before anything is compared against it."""
    cfg = LATTICE[case]
    kind = cfg[0]
    mod = module_for(import_pkg(), cfg)
    inp = inputs(cfg, which)
    dm, ds, dn = _cots(kind)
    r64 = OracleRHS.from_module(mod, torch.float64)
    margin, masks = record_condition(r64, inp.y0.double(), inp.t, inp.h)
    check_condition(margin, masks, (case, which))
    kink = rate_kink(r64, inp.y0.double(), inp.t, inp.h)
    assert kink is None or float(kink.min()) >= KINK, (case, which, float(kink.min()))
    ref = solve_and_grad(r64, inp.y0.double(), inp.t, inp.h, inp.dl, dm, ds, dn)
    r32 = solve_and_grad(OracleRHS.from_module(mod, torch.float32), inp.y0, inp.t, inp.h, inp.dl.float(),
                         None if dm is None else dm.float(), None if ds is None else ds.float(), dn)
    d32 = {"latent": normwise_rel(r32.latent, ref.latent)}
    for key in ("mean", "std", "fa_norm"):
        if getattr(ref, key) is not None:
            d32[key] = normwise_rel(getattr(r32, key), getattr(ref, key))
    for k, v in ref.grads.items():
        d32[k] = normwise_rel(r32.grads[k], v)
    return SimpleNamespace(ref=ref, margin=margin, masks=masks, kink=kink, ref32=d32, inp=inp, cfg=cfg)


def bar(refs, key):
    """max(project floor, 2 x the oracle's own fp32-vs-fp64 distance): the rule of helpers.tol."""
    return max(FLOORS.get(key, FLOOR_W), 2.0 * refs.ref32.get(key, 0.0))


# ---------------------------------------------------------------------------------------------------
# Bayesian cases: the same y0 / grids; module seed 0, default init (|std| = 0.1); one eps row per evaluation

def bayes_module_for(cfg):
    import ude_amd.bayes as B
    kind, R, L, net, aug = cfg
    torch.manual_seed(0)
    kw = {}
    if net is not None:
        kw["net_sizes"] = list(net)
    if aug is not None:
        kw["aug_net_sizes"] = list(aug)
    mod = {"BFp": B.Bayes_Fp, "BFa": B.Bayes_Fa, "BFaFp": B.Bayes_FaFp}[kind](R, latent_dim=L, **kw)
    if kind == "BFaFp":
        mod.Fa_w = FA_W
    return mod


def bayes_inputs(cfg, mod, which="full"):
    """y0, t, step_size, eps (4 n_steps, n_params), dlatent (fp64) of a Bayesian lattice case."""
    _kind, R, L, _net, _aug = cfg
    y0, gen = y0_for(R, L)
    t, h = grid(which)
    n_steps = len(make_grid(t, h)) - 1
    n_par = sum(p.numel() for p in mod.ude_mean_std()[0])
    eps = torch.randn(4 * n_steps, n_par, generator=gen)
    dl = torch.randn((len(t), N_TRAJ, R, L), generator=gen, dtype=torch.float64)
    return SimpleNamespace(y0=y0, t=t, h=h, eps=eps, dl=dl)


def bayes_condition(case, which):
    from oracle.ude_oracle_bayes import OracleBayesRHS
    cfg = LATTICE[case]
    mod = bayes_module_for(cfg)
    inp = bayes_inputs(cfg, mod, which)
    rhs = OracleBayesRHS.from_module(mod, torch.float64)
    rhs.eps = inp.eps.double()
    return record_condition(rhs, inp.y0.double(), inp.t, inp.h)


# b2's deterministic twin: the per-evaluation path of a Bayesian model (ude_amd/eval_rhs.py) evaluates each
# weight sample on the deterministic kernels of the same sizes
B2_EVAL = _c("FaFp", 5, 8, [64, 64, 32], [64, 64])


def jit_prebuild(cases=None):
    """The lattice's JIT libraries (all, or those of ``cases``), compiled side by side where missing."""
    from ude_amd import _native
    cfgs = [LATTICE[k] for k in (cases or LATTICE)]
    if cases is None or "b2" in cases:
        cfgs.append(B2_EVAL)
    return _native.jit_prebuild(cfgs, 16)


# FaFp R = 64 with the widest lattice nets: the backward record exceeds the 160 KiB LDS
TOO_LARGE = _c("FaFp", 64, 8, [128, 128, 128], [128, 128])


if __name__ == "__main__":                               # what __graft_entry__.build() runs
    for _p in jit_prebuild():
        print(_p)
