"""Shared pieces of the scenario tests (test_scenario.py, test_scenario_gpu.py): the fp64 / fp32 oracle
restated with per-step scaled rates, the test table and the bars.

The reference has no scenarios; the yardstick is the project's own oracle (oracle/ude_oracle.py) with the one
change a scenario makes: the rates ``p = |q|`` of region r are multiplied by ``scale[r]`` right after ``abs``,
and the integrator sets the scale of step k before the four stage evaluations of that step."""
import functools
from dataclasses import dataclass
from typing import Optional

import torch

from conftest import load_golden
from helpers import module_from_golden, normwise_rel, step_of
from oracle.ude_oracle import OracleRHS, make_grid, rk4_alt_step

SCN_CASES = ["e2e_dyn_fafp_r1", "e2e_dyn_fafp_r3_l5", "e2e_dyn_fp_r10", "e2e_dyn_fafp_r49"]
MARGIN_MIN = 1e-3          # the fp64 reference stays this far from the mask boundary on every evaluation
GAMMA_MIN = 0.05           # and its scaled gamma this far from zero (r_eff divides by it)


@dataclass
class ScenarioOracleRHS(OracleRHS):
    """OracleRHS whose rates are scaled by ``scale`` (R, 2) after ``abs`` (None: the plain RHS)."""
    scale: Optional[torch.Tensor] = None

    def __call__(self, t, x):
        R = self.n_regions
        mask = (x > 2) | (x < -1)
        if self.record_masks:
            xs = x[..., :3].detach()
            self.margins.append(torch.minimum((xs - 2).abs(), (xs + 1).abs()).reshape(x.shape[0], -1).amin(1))
        flat = x.reshape(x.shape[0], -1)
        if self.kind in ("Fp", "FaFp"):
            p = torch.abs(self._mlp(flat, self.p_w, self.p_b, self.p_act)).reshape(-1, R, 2)
            if self.scale is not None:
                p = p * self.scale.to(p)
            self.params.append(p)
            plus_i = p[..., 0] * x[..., 0] * x[..., 1]
            minus_i = p[..., 1] * x[..., 1]
            flux = torch.stack([-plus_i, plus_i - minus_i, minus_i], dim=-1)
        if self.kind in ("Fa", "FaFp"):
            fa = self._mlp(flat, self.a_w, self.a_b, self.a_act).reshape(-1, R, 3)
            self.tracker.append(fa)
            flux = fa if self.kind == "Fa" else flux + self.fa_w * fa
        res = torch.cat([flux, torch.zeros_like(x[..., 3:])], -1)
        return torch.where(mask, torch.zeros_like(res), res)


def scn_table(n_steps, R):
    """Every (step, region) differs: m_beta = 0.5 + 0.1 ((3k + r) mod 7), m_gamma = 0.8 + 0.05 ((k + 2r) mod 5)."""
    k = torch.arange(n_steps).view(-1, 1)
    r = torch.arange(R).view(1, -1)
    return torch.stack([0.5 + 0.1 * ((3 * k + r) % 7).double(), 0.8 + 0.05 * ((k + 2 * r) % 5).double()],
                       -1).to(torch.float32)


def oracle_solve(rhs, y0, t, step_size, table):
    """The restated solve: per-step loop over rk4_alt_step, ``rhs.scale = table[k]`` during step k, every output
    a grid hit.  Returns a dict: latent (T, N, R, L), dyn (C, T, N, R) by the kernel's definitions (an output
    that starts a step evaluated under that step's row, the last under the last step's), the scaled rates'
    mean / unbiased std over the solve's evaluations, the smallest mask margin and the smallest gamma'."""
    dt_ = y0.dtype
    grid = t if step_size is None else make_grid(t, step_size)
    n_steps = len(grid) - 1
    assert tuple(table.shape) == (n_steps, rhs.n_regions, 2)
    rhs.clear_tracking()
    rhs.record_masks = True
    sol, at_step, y, j = [y0], [0], y0, 1
    with torch.no_grad():
        for n in range(n_steps):
            rhs.scale = table[n]
            t0, t1 = grid[n].to(dt_), grid[n + 1].to(dt_)
            y = y + rk4_alt_step(rhs, t0, t1 - t0, t1, y)
            while j < len(t) and grid[n + 1] >= t[j]:
                assert t[j] == grid[n + 1], "every output must be a grid hit"
                sol.append(y)
                at_step.append(n + 1)
                j += 1
        latent = torch.stack(sol)
        out = {"latent": latent, "margin": float(torch.stack(rhs.margins).min())}
        p = torch.stack(rhs.params).reshape(-1, 2)
        out["mean"], out["std"], out["gamma_min"] = p.mean(0), p.std(0), float(p[:, 1].min())
        chans = []
        for jo, k in enumerate(at_step):
            rhs.clear_tracking()
            rhs.scale = table[min(k, n_steps - 1)]
            rhs(t[jo].to(dt_), latent[jo])
            x = latent[jo]
            ch = [x[..., 0], x[..., 1], x[..., 2]]
            if rhs.params:
                b, g = rhs.params[-1][..., 0], rhs.params[-1][..., 1]
                ch += [b, g, b * x[..., 0] / g]
            if rhs.tracker:
                ch += [rhs.tracker[-1][..., c] for c in range(3)]
            chans.append(torch.stack(ch))
        out["dyn"] = torch.stack(chans, 1)
    rhs.clear_tracking()
    rhs.scale, rhs.record_masks = None, False
    return out


@functools.lru_cache(maxsize=None)
def reference(case, halves=1):
    """(fixture, fp64 restated oracle, fp32 restated oracle, the table) of ``case`` under the test table,
    ``halves`` RK4 steps per output interval.  Computed once; treat as read-only."""
    import conftest
    pkg = conftest.import_pkg()
    g = load_golden(case)
    t, step = step_of(g)
    step = step / halves
    n_steps = (len(t) - 1) * halves
    table = scn_table(n_steps, g["meta"]["n_regions"])
    y0 = torch.from_numpy(g["y0"])
    mod = module_from_golden(pkg, g, "cpu")
    res = {}
    for dt_ in (torch.float64, torch.float32):
        rhs = ScenarioOracleRHS.from_module(mod, dt_)
        res[dt_] = oracle_solve(rhs, y0.to(dt_), t.to(dt_), step.to(dt_), table.to(dt_))
    return g, res[torch.float64], res[torch.float32], table


def bar(ref64, ref32, key, c=None, last=False):
    """max(1e-5, 2 x the restated oracle's own fp32-vs-fp64 distance of this quantity), normwise."""
    a, b = ref32[key], ref64[key]
    if c is not None:
        a, b = a[c], b[c]
    if last:
        a, b = a[-1], b[-1]
    return max(1e-5, 2.0 * normwise_rel(a, b))
