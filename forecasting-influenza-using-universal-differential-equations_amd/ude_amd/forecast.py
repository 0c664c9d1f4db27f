"""The ensemble forecast: inference solve with the decoder epilogue + on-device summary.

The reference's forecast side (lib/utils.py:20-56 ``test``, lib/VAE.py ``evaluate`` and the
``validate=`` branch of ``VAE.train``) solves ``n_samples`` trajectories per test window, decodes
the whole (T, N, R, L) latent, copies the (B, S, T, R) prediction to the host and forms the
per-(window, day, region) mean / std with NumPy and the per-horizon scores with SciPy.

``solve_decode_forecast`` is that solve without autograd on the gfx950 kernels
(ude_rk4_forecast_dec): the forward kernel's decoder epilogue emits ``y_hat (T, N, R) =
Decoder(latent[..., :3])`` at every output time; no latent, checkpoint or stored activation is
written.  ``ensemble_summary`` turns ``y_hat`` into a ``Forecast`` (mean, population std, quantiles,
and against targets the per-day Metrics.nll / skill / mae) in one read of ``y_hat``
(ude_forecast_summary; fp64 after the load, fixed-order sums: the same bits run to run).  On a CPU
tensor the same definitions run on torch fp64 operators.

``verify=`` adds scores of the ensemble itself, from the tile the summary kernel has sorted
(ude_forecast_verify): CRPS, the weighted interval score, interval coverage, the PIT histogram and
the empirical multibin skill (lib/Metrics.py ``mb_log(bins=True)``'s window on the samples), per day
and per (day, region).

``solve_decode_dynamics`` is the same solve that also emits what the model has learned about the
epidemic at every output time (ude_rk4_forecast_dyn): the compartments S, I, R, the rates beta and
gamma the rate net gives at that state, R_eff = beta S / gamma, and the augmentation flux Fa -- a
``(C, T, N, R)`` array that ``dynamics_summary`` turns into a ``Dynamics`` by one ``ensemble_summary``
call.  ``latent_dynamics`` forms the same channels from a written latent (CPU, Bayesian RHS, output
times between grid points).

``ensemble_season`` reduces the same ``y_hat`` along its trajectories instead of per day
(ude_forecast_season): per sample the peak over the considered output times, when it falls, the total
and the onset against a baseline -- the FluSight seasonal targets -- as a ``SeasonTargets`` of their
distributions over the ensemble, scored against the observed season when targets are given.

``Scenario`` is a counterfactual of the same forecast: multipliers of the rate net's beta and gamma per
output interval and region.  ``solve_decode_scenario`` is the solve under it (ude_rk4_forecast_scn: every
stage of an RK4 step scales the rates by the step's row before the flux), ``scenario_latent`` the same on
the module's layers, and ``VAE.forecast(scenarios=...)`` returns per scenario a ``ScenarioForecast``: its
own summaries and those of the paired difference to the baseline, solved on the same draw.

``ensemble_joint`` scores the trajectories jointly (ude_forecast_joint): the energy score and the variogram
score of a window's S trajectories against the observed one, on region r's series, on the field of the
regions at one time and on all considered coordinates at once -- the scores that tell an ensemble whose days
and regions move together from one with the same marginals that does not -- as a ``JointScores``.

``Aggregate`` is a level of a hierarchy over the regions (the HHS regions, the nation): ``ensemble_aggregate``
sums ``y_hat`` over the regions with the level's weights trajectory by trajectory (ude_forecast_aggregate: one
read for all levels, fp64 in a stated order, stored as fp32), ``aggregate_dynamics`` the dynamics
(ude_forecast_aggregate_dyn: the aggregate's own beta, gamma and R_eff from its infections and recoveries), and
``VAE.forecast(aggregate={...})`` returns per level a whole ``Forecast`` of that coherent ensemble in
``Forecast.aggregates``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from . import decoder_head
from . import fused as _fused

MASS_FLOOR = 4.5399929762484854e-05      # lib/Metrics.py mb_log: an exactly zero mass -> e^-10
MAX_QUANTILE_SAMPLES = 1024              # FC_MAX_SQ (csrc/ude_forecast.h)
FLUSIGHT_ALPHAS = (0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)
MAX_ALPHAS = 16                          # FC_MAX_ALPHA
MAX_PIT_BINS = 64                        # FC_MAX_PIT


@dataclass(frozen=True)
class Verify:
    """What ``verify=`` scores: the central intervals ``1 - alpha`` of the weighted interval score
    and of ``coverage`` (each alpha in (0, 1), at most 16), and the number of PIT bins (at most 64)."""
    alphas: Tuple[float, ...] = FLUSIGHT_ALPHAS
    pit_bins: int = 10

    def __post_init__(self):
        alphas = tuple(float(a) for a in self.alphas)
        object.__setattr__(self, "alphas", alphas)
        if not 1 <= len(alphas) <= MAX_ALPHAS:
            raise ValueError(f"Verify: {len(alphas)} alphas (1 to {MAX_ALPHAS})")
        if not all(0.0 < a < 1.0 for a in alphas):
            raise ValueError("Verify: every alpha must lie in (0, 1)")
        if int(self.pit_bins) != self.pit_bins or not 1 <= self.pit_bins <= MAX_PIT_BINS:
            raise ValueError(f"Verify: pit_bins {self.pit_bins} (1 to {MAX_PIT_BINS})")


@dataclass(frozen=True)
class Season:
    """What ``season=`` considers.  The output indices ``t_m = start + m * every``, ``m = 0 .. M-1`` with
    ``M = ceil((T - start) / every)`` (weekly points of a daily grid: ``start=6, every=7``); ``baseline``:
    None (no onset), a number or one per region, in scaled units; the onset is the first ``m`` that starts
    ``run`` consecutive considered values at or above the baseline; ``window``: the half-width, in
    considered times, of the bins the peak-time and onset log scores count as a hit."""
    baseline: Optional[object] = None
    start: int = 0
    every: int = 1
    run: int = 3
    window: int = 1

    def __post_init__(self):
        for name, low in (("start", 0), ("every", 1), ("run", 1), ("window", 0)):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or int(v) < low or int(v) > 2 ** 31 - 1:
                raise ValueError(f"Season: {name} {v!r} (an integer >= {low})")
            object.__setattr__(self, name, int(v))
        if self.baseline is not None:
            base = np.asarray(self.baseline.values if hasattr(self.baseline, "values") else self.baseline,
                              dtype=np.float64)
            if base.ndim > 1 or base.size < 1 or not np.isfinite(base).all():
                raise ValueError("Season: baseline is a finite number or one per region")
            object.__setattr__(self, "baseline", float(base) if base.ndim == 0 else tuple(base.tolist()))

    def without_baseline(self) -> "Season":
        """The same considered times without an onset: for values that are not incidences (a difference)."""
        return Season(None, self.start, self.every, self.run, self.window)

    def times(self, T: int) -> int:
        """M, the number of considered output indices of a T-point forecast."""
        if not self.start < T:
            raise ValueError(f"Season: start {self.start} is not below the {T} output times")
        return -((self.start - T) // self.every)

    def baseline_vector(self, R: int, device) -> Optional[torch.Tensor]:
        if self.baseline is None:
            return None
        base = torch.as_tensor(self.baseline, dtype=torch.float64, device=device).reshape(-1)
        if base.numel() == 1:
            base = base.expand(R)
        if base.numel() != R:
            raise ValueError(f"Season: baseline has {base.numel()} entries for {R} regions")
        return base.contiguous()


SEASON_SCORES = ("peak_time_skill", "onset_skill", "peak_value_skill", "peak_crps", "total_crps")

MAX_JOINT_COORDS = 4096                  # JS_MAX_C (csrc/ude_joint.h): regions and considered times on the device


@dataclass(frozen=True)
class Joint:
    """What ``joint=`` considers: the output indices ``t_m = start + m * every`` as ``Season`` has them, and
    the variogram's order ``p``, 0.5 or 1.0."""
    start: int = 0
    every: int = 1
    p: float = 0.5

    def __post_init__(self):
        for name, low in (("start", 0), ("every", 1)):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or int(v) < low or int(v) > 2 ** 31 - 1:
                raise ValueError(f"Joint: {name} {v!r} (an integer >= {low})")
            object.__setattr__(self, name, int(v))
        if isinstance(self.p, bool) or self.p not in (0.5, 1.0):
            raise ValueError(f"Joint: p {self.p!r} (0.5 or 1.0)")
        object.__setattr__(self, "p", float(self.p))

    def times(self, T: int) -> int:
        """M, the number of considered output indices of a T-point forecast."""
        if not self.start < T:
            raise ValueError(f"Joint: start {self.start} is not below the {T} output times")
        return -((self.start - T) // self.every)


MAX_AGGREGATE_REGIONS = 4096             # AG_MAX_R (csrc/ude_aggregate.h): the device's limits
MAX_AGGREGATE_GROUPS = 256               # AG_MAX_G, over all levels
MAX_AGGREGATE_LEVELS = 16                # AG_MAX_LEVELS


@dataclass(frozen=True, eq=False)
class Aggregate:
    """One level of a hierarchy over the regions: ``weights`` (G, R), finite, any sign -- group g of the level
    is ``sum_r weights[g, r] * value_r``, trajectory by trajectory (population shares: rows that sum to 1).
    ``names``: None or one name per group.  ``baseline``: None, a number or one per group, in data units -- the
    onset baseline ``VAE.forecast(season=...)`` uses at this level (None: no onset there)."""
    weights: object
    names: Optional[Tuple[str, ...]] = None
    baseline: Optional[object] = None

    def __post_init__(self):
        w = self.weights
        if isinstance(w, torch.Tensor):
            w = w.detach().cpu().numpy()
        try:
            w = np.array(w.values if hasattr(w, "values") else w, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError("Aggregate: weights are not numeric") from e
        if w.ndim != 2 or w.shape[0] < 1 or w.shape[1] < 1 or not np.isfinite(w).all():
            raise ValueError(f"Aggregate: weights are a finite (G, R) matrix, not {w.shape}")
        w.setflags(write=False)
        object.__setattr__(self, "weights", w)
        if self.names is not None:
            names = tuple(self.names)
            if len(names) != w.shape[0]:
                raise ValueError(f"Aggregate: {len(names)} names for {w.shape[0]} groups")
            object.__setattr__(self, "names", names)
        if self.baseline is not None:
            try:
                base = np.asarray(self.baseline.values if hasattr(self.baseline, "values") else self.baseline,
                                  dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError("Aggregate: baseline is not numeric") from e
            if base.ndim > 1 or base.size not in (1, w.shape[0]) or not np.isfinite(base).all():
                raise ValueError(f"Aggregate: baseline is a finite number or one per group ({w.shape[0]})")
            object.__setattr__(self, "baseline", float(base) if base.ndim == 0 else tuple(base.tolist()))

    def on(self, device) -> torch.Tensor:
        """The weights as an fp64 tensor on ``device``, copied there once."""
        cache = self.__dict__.setdefault("_on", {})
        key = str(torch.device(device))
        if key not in cache:
            cache[key] = torch.from_numpy(np.array(self.weights)).to(device)
        return cache[key]

    @property
    def n_groups(self) -> int:
        return self.weights.shape[0]

    @property
    def n_regions(self) -> int:
        return self.weights.shape[1]

    @classmethod
    def from_groups(cls, R: int, groups, share, names=None, baseline=None) -> "Aggregate":
        """The level whose group g holds the regions ``groups[g]`` weighted by their share of the group:
        ``a[g, r] = share[r] / sum_{r' in groups[g]} share[r']`` for r in the group, else 0.  ``share``: one
        non-negative value per region (populations); each group's shares must sum to more than 0."""
        if isinstance(R, bool) or int(R) != R or int(R) < 1:
            raise ValueError(f"Aggregate.from_groups: R {R!r} (at least one region)")
        R = int(R)
        try:
            sh = np.asarray(share.values if hasattr(share, "values") else share, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError) as e:
            raise ValueError("Aggregate.from_groups: share is not numeric") from e
        if sh.shape != (R,) or not np.isfinite(sh).all() or (sh < 0).any():
            raise ValueError(f"Aggregate.from_groups: share is one finite value >= 0 per region ({R})")
        groups = [list(g) for g in groups]
        if not groups:
            raise ValueError("Aggregate.from_groups: no group")
        a = np.zeros((len(groups), R))
        for g, members in enumerate(groups):
            if not members or any(isinstance(r, bool) or int(r) != r or not 0 <= int(r) < R for r in members) \
                    or len(set(int(r) for r in members)) != len(members):
                raise ValueError(f"Aggregate.from_groups: group {g} is a set of region indices in [0, {R})")
            idx = [int(r) for r in members]
            total = sh[idx].sum()
            if not total > 0:
                raise ValueError(f"Aggregate.from_groups: the shares of group {g} sum to {total}")
            a[g, idx] = sh[idx] / total
        return cls(a, names, baseline)


class _Result:
    """What the result containers (dataclasses) share.  A field holds a tensor, None, another container
    (``Forecast.dynamics`` / ``.season`` / ``.joint``: handled by recursion), a dict of containers by name
    (``Forecast.scenarios`` / ``.aggregates``: each in its place, in the dict's order) or something else that is carried
    through (``Dynamics.names``)."""

    def _tensors(self):
        """``[(field name, tensor)]`` in field order, a nested container's in its place."""
        out = []
        for f in fields(self):
            v = getattr(self, f.name)
            for u in (v.values() if isinstance(v, dict) else (v,)):
                if isinstance(u, _Result):
                    out += u._tensors()
                elif isinstance(u, torch.Tensor):
                    out.append((f.name, u))
        return out

    def _map(self, fn):
        """The same container with ``fn`` applied to every tensor, in the order of ``_tensors``."""
        def go(v):
            if isinstance(v, dict):
                return {k: go(u) for k, u in v.items()}
            return v._map(fn) if isinstance(v, _Result) else fn(v) if isinstance(v, torch.Tensor) else v
        return type(self)(**{f.name: go(getattr(self, f.name)) for f in fields(self)})

    def cpu(self):
        """One stacked device-to-host copy of every tensor (nested containers' included); ``self`` when
        already on the host."""
        parts = [v for _, v in self._tensors()]
        if not parts[0].is_cuda:
            return self
        chunks = iter(torch.cat([v.reshape(-1) for v in parts]).cpu().split([v.numel() for v in parts]))
        return self._map(lambda v: next(chunks).view(v.shape))

    def numpy(self):
        """dict of numpy arrays by field name (absent fields None; a nested container: its ``numpy()`` dict;
        a dict of containers: the dict of theirs; ``Dynamics.names`` as it is)."""
        host, out = self.cpu(), {}
        conv = lambda v: v.numpy() if isinstance(v, (_Result, torch.Tensor)) else v
        for f in fields(host):
            v = getattr(host, f.name)
            out[f.name] = {k: conv(u) for k, u in v.items()} if isinstance(v, dict) else conv(v)
        return out


@dataclass
class SeasonTargets(_Result):
    """The seasonal targets of an ensemble forecast (fp64 tensors on the forecast's device), over the M
    considered output indices of a ``Season``.  Per (window, region) group over the S trajectories:
    ``peak_mean`` / ``peak_std`` (B, R) and ``peak_quantiles`` (Q, B, R) or None of each trajectory's
    highest considered value; ``total_*``: the same of each trajectory's sum; ``peak_time`` (B, M, R): the
    fraction of trajectories whose peak falls on index m (the first, where several tie); ``onset``
    (B, M + 1, R) or None without a baseline: the fraction whose onset is m, bin M being "no onset within
    the horizon".

    With targets, against the observed season (the same rules on ``y_true``): ``peak_time_skill`` /
    ``onset_skill`` = exp(mean log mass the histogram gives to the bins within ``window`` of the observed
    one; "none" only matches "none"), ``peak_value_skill`` = exp(mean log empirical mass of the multibin
    window around the observed peak), an empty window or zero mass counting as MASS_FLOOR; ``peak_crps``
    / ``total_crps``.  Each is the mean over the B * R groups (0-dim); ``*_r`` (R,) per region over the B
    windows."""
    peak_mean: torch.Tensor
    peak_std: torch.Tensor
    total_mean: torch.Tensor
    total_std: torch.Tensor
    peak_time: torch.Tensor
    peak_quantiles: Optional[torch.Tensor] = None
    total_quantiles: Optional[torch.Tensor] = None
    onset: Optional[torch.Tensor] = None
    peak_time_skill: Optional[torch.Tensor] = None
    onset_skill: Optional[torch.Tensor] = None
    peak_value_skill: Optional[torch.Tensor] = None
    peak_crps: Optional[torch.Tensor] = None
    total_crps: Optional[torch.Tensor] = None
    peak_time_skill_r: Optional[torch.Tensor] = None
    onset_skill_r: Optional[torch.Tensor] = None
    peak_value_skill_r: Optional[torch.Tensor] = None
    peak_crps_r: Optional[torch.Tensor] = None
    total_crps_r: Optional[torch.Tensor] = None


@dataclass
class JointScores(_Result):
    """The joint scores of an ensemble forecast against the observed trajectory (fp64 tensors on the
    forecast's device), over the M considered output indices of a ``Joint``: the energy score ``ES_C = mean_i
    |x_i - y|_C - mean_ij |x_i - x_j|_C / 2`` (Euclidean norm over the block's coordinates) and the unweighted
    variogram score of order p ``VS_C = sum_{c < c'} (|y_c - y_c'|^p - mean_s |x_sc - x_sc'|^p)^2`` of a window's
    S trajectories, on the blocks series (b, r) -- region r's M times: ``energy_series`` / ``variogram_series``
    (B, R) --, field (b, m) -- the R regions at time m: ``energy_field`` / ``variogram_field`` (B, M) -- and
    joint (b) -- all M * R coordinates: ``energy_joint`` (B,).  ``energy_joint_mean`` (0-dim), ``*_r`` (R,) and
    ``*_t`` (M,) are their means over the B windows.  In one dimension the energy score is the CRPS; a block of
    one coordinate has variogram score 0."""
    energy_joint: torch.Tensor
    energy_series: torch.Tensor
    energy_field: torch.Tensor
    variogram_series: torch.Tensor
    variogram_field: torch.Tensor
    energy_joint_mean: torch.Tensor
    energy_series_r: torch.Tensor
    energy_field_t: torch.Tensor
    variogram_series_r: torch.Tensor
    variogram_field_t: torch.Tensor


DYN_STATE = ("s", "i", "r")
DYN_RATES = ("beta", "gamma", "r_eff")
DYN_FLUX = ("fa_s", "fa_i", "fa_r")


def dynamics_names(ode) -> Tuple[str, ...]:
    """The channels of ``ode``'s dynamics, in their fixed order: ``s, i, r`` always, ``beta, gamma,
    r_eff`` with a rate net (Fp, FaFp), ``fa_s, fa_i, fa_r`` with an augmentation net (Fa, FaFp)."""
    kind = ode.ode_type
    return DYN_STATE + (DYN_RATES if kind in ("Fp", "FaFp") else ()) + (DYN_FLUX if kind in ("Fa", "FaFp") else ())


@dataclass
class Dynamics(_Result):
    """Per-(channel, window, day, region) summary of the learned dynamics over the ensemble (fp64):
    ``names`` (C channel names, ``dynamics_names``), ``mean`` / ``std`` (C, B, T, R) (population std)
    and ``quantiles`` (Q, C, B, T, R) or None.  ``dyn["r_eff"]`` is that channel's
    ``(mean (B, T, R), std (B, T, R), quantiles (Q, B, T, R) or None)``.  The rates are the nets' outputs
    at the state of each output time (unmasked, as the RHS appends them to ``params``), ``r_eff`` =
    beta * s / gamma per trajectory, ``fa_*`` the raw augmentation flux (as appended to ``tracker``)."""
    names: Tuple[str, ...]
    mean: torch.Tensor
    std: torch.Tensor
    quantiles: Optional[torch.Tensor] = None

    def __getitem__(self, name: str):
        c = self.names.index(name)
        return self.mean[c], self.std[c], (None if self.quantiles is None else self.quantiles[:, c])


@dataclass
class Forecast(_Result):
    """Per-(window, day, region) summary of an ensemble forecast (fp64 tensors on the forecast's
    device): ``mean`` / ``std`` (B, T, R) (population std, as numpy.std), ``quantiles`` (Q, B, T, R)
    or None, and -- when targets were given -- ``nll`` / ``skill`` / ``mae`` (T,): lib/Metrics.py's
    scores of every time index over its B * R groups.

    With ``verify`` (K alphas, J PIT bins), scores of the ensemble itself: ``crps`` / ``wis`` (T,)
    (means over the B * R groups), ``ens_skill`` (T,) = exp(mean log empirical mass of the multibin
    window, an empty window counting as MASS_FLOOR), ``coverage`` (K, T) (fraction of groups whose
    central 1 - alpha_k interval holds the target), ``pit`` (T, J) (fraction of groups per bin of the
    target's mid-rank; rows sum to 1), and the per-region forms (means over the B windows)
    ``nll_r`` / ``skill_r`` / ``mae_r`` / ``crps_r`` / ``wis_r`` / ``ens_skill_r`` (T, R) and
    ``coverage_r`` (K, T, R).

    ``dynamics``: the ``Dynamics`` of the same ensemble when it was asked for
    (``VAE.forecast(dynamics=True)``), else None.  ``season``: its ``SeasonTargets``
    (``VAE.forecast(season=Season(...))``), else None.  ``scenarios``: name -> ``ScenarioForecast`` of
    every scenario solved beside it on the same draw (``VAE.forecast(scenarios={...})``), else None.
    ``joint``: its ``JointScores`` (``VAE.forecast(joint=True)`` or a ``Joint``), else None.
    ``aggregates``: name -> the ``Forecast`` of that level of ``VAE.forecast(aggregate={...})`` -- the same
    fields with the level's G groups in place of the R regions --, else None (declared before ``joint``, which
    stays the last field)."""
    mean: torch.Tensor
    std: torch.Tensor
    quantiles: Optional[torch.Tensor] = None
    nll: Optional[torch.Tensor] = None
    skill: Optional[torch.Tensor] = None
    mae: Optional[torch.Tensor] = None
    crps: Optional[torch.Tensor] = None
    wis: Optional[torch.Tensor] = None
    ens_skill: Optional[torch.Tensor] = None
    coverage: Optional[torch.Tensor] = None
    pit: Optional[torch.Tensor] = None
    nll_r: Optional[torch.Tensor] = None
    skill_r: Optional[torch.Tensor] = None
    mae_r: Optional[torch.Tensor] = None
    crps_r: Optional[torch.Tensor] = None
    wis_r: Optional[torch.Tensor] = None
    ens_skill_r: Optional[torch.Tensor] = None
    coverage_r: Optional[torch.Tensor] = None
    dynamics: Optional[Dynamics] = None
    season: Optional[SeasonTargets] = None
    scenarios: Optional[Dict[str, "ScenarioForecast"]] = None
    aggregates: Optional[Dict[str, "Forecast"]] = None
    joint: Optional[JointScores] = None


@dataclass
class RateStats(_Result):
    """The side statistics of one solve (fp32, as the kernel's last workgroup writes them): ``mean`` / ``std``
    (2,) of every beta and gamma that entered the flux (unbiased std) and ``fa_norm`` (1,), the norm of every
    raw Fa -- what a fused solve records on the RHS for ``posterior()`` and the tracker.  Under a scenario
    they are the scaled rates' and are returned with the scenario's result instead."""
    mean: torch.Tensor
    std: torch.Tensor
    fa_norm: Optional[torch.Tensor] = None


@dataclass
class SeasonEffect(_Result):
    """A scenario's effect on each trajectory's season total: the ``total_*`` fields of ``ensemble_season`` of
    the paired difference (scenario - baseline).  The total is linear in the prediction, so this is the
    distribution over the ensemble of the burden added (negative: averted), sample by sample."""
    total_mean: torch.Tensor
    total_std: torch.Tensor
    total_quantiles: Optional[torch.Tensor] = None


@dataclass
class ScenarioForecast(_Result):
    """One scenario of ``VAE.forecast(scenarios=...)``, solved on the baseline's draw.  ``forecast``: the
    ``Forecast`` of the scenario's prediction (mean / std / quantiles; no scores: the observation did not
    happen under the scenario; ``.dynamics`` / ``.season`` when they were asked for, the season without
    targets).  ``effect``: the ``ensemble_summary`` of the paired difference ``y_hat_scenario - y_hat_baseline``
    (same scale and quantiles).  ``effect_season``: its ``SeasonEffect`` when ``season`` was given.
    ``rates``: the ``RateStats`` of the scenario's solve."""
    forecast: Forecast
    effect: Forecast
    effect_season: Optional[SeasonEffect] = None
    rates: Optional[RateStats] = None


def _as_array(name: str, v) -> np.ndarray:
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    try:
        a = np.array(v.values if hasattr(v, "values") else v, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"Scenario: {name} is not numeric") from e
    if a.ndim > 2 or a.size < 1:
        raise ValueError(f"Scenario: {name} is a scalar, a (T-1,) vector, a (R,) row or a (T-1, R) array, "
                         f"not {a.shape}")
    if not np.isfinite(a).all() or (a < 0).any():
        raise ValueError(f"Scenario: every {name} multiplier must be finite and >= 0")
    a.setflags(write=False)
    return a


@dataclass(frozen=True, eq=False)
class Scenario:
    """A counterfactual of the forecast: multipliers of the rate net's ``beta`` (transmission) and ``gamma``
    (recovery) per output interval ``[t_j, t_{j+1})``, j = 0 .. T-2, and region.  Each of ``beta`` / ``gamma``
    is a scalar, a ``(T-1,)`` vector (all regions), a ``(T-1, R)`` array, or a row that broadcasts over the
    intervals -- ``(R,)`` (a 1-D argument of length T-1 is read per interval) or ``(1, R)``; every value
    finite and >= 0.  ``table`` expands the intervals to the RK4 steps of a solve: all four stages of a step
    use its interval's row, beta' = m_beta * |q0|, gamma' = m_gamma * |q1|; Fa is not scaled."""
    beta: object = 1.0
    gamma: object = 1.0

    def __post_init__(self):
        object.__setattr__(self, "beta", _as_array("beta", self.beta))
        object.__setattr__(self, "gamma", _as_array("gamma", self.gamma))

    @classmethod
    def from_day(cls, T: int, start: int, beta=1.0, gamma=1.0) -> "Scenario":
        """Ones before output interval ``start`` (0 <= start <= T-1) and ``beta`` / ``gamma`` (each a scalar
        or one value per region) from it on, for a forecast of T output times."""
        if isinstance(T, bool) or int(T) != T or int(T) < 2:
            raise ValueError(f"Scenario.from_day: T {T!r} (at least 2 output times)")
        if isinstance(start, bool) or int(start) != start or not 0 <= int(start) <= int(T) - 1:
            raise ValueError(f"Scenario.from_day: start {start!r} (0 to {int(T) - 1})")

        def ramp(name, v):
            v = _as_array(name, v)
            if v.ndim > 1:
                raise ValueError(f"Scenario.from_day: {name} is a scalar or one value per region")
            a = np.ones((int(T) - 1,) + v.shape)
            a[int(start):] = v
            return a
        return cls(ramp("beta", beta), ramp("gamma", gamma))

    def intervals(self, T: int, R: int) -> np.ndarray:
        """The multipliers per output interval and region, ``(T-1, R, 2)`` fp32 ([..., 0]: beta)."""
        n = int(T) - 1
        out = np.empty((n, int(R), 2), dtype=np.float32)
        for c, (name, a) in enumerate((("beta", self.beta), ("gamma", self.gamma))):
            if a.ndim == 1 and a.shape[0] == n:
                a = a[:, None]
            if a.ndim == 1 and a.shape[0] not in (1, R) or a.ndim == 2 and (a.shape[0] not in (1, n)
                                                                          or a.shape[1] not in (1, R)):
                raise ValueError(f"Scenario: {name} {a.shape} does not fit {n} intervals x {R} regions")
            out[..., c] = np.broadcast_to(a, (n, int(R)))
        return out

    def table(self, plan, R: int, T: Optional[int] = None) -> torch.Tensor:
        """The ``(n_steps, R, 2)`` fp32 table (host) of a solve: ``plan`` is its launch plan or its
        ``schedule.Schedule``.  Every output must be a grid hit, so that every step lies in one interval
        (``step_intervals`` gives ``plan`` for an eager solve where they are not; ``T``: its output times)."""
        steps = getattr(plan, "step_interval", None)
        if steps is None:
            out_k = _grid_hits(plan)
            steps = np.repeat(np.arange(len(out_k) - 1), np.diff(np.asarray(out_k)))
            n_int = len(out_k) - 1
        else:
            n_int = int(steps.max()) + 1 if T is None else int(T) - 1
        rows = self.intervals(n_int + 1, R)
        return torch.from_numpy(np.ascontiguousarray(rows[steps]))


@dataclass
class _Intervals:
    step_interval: np.ndarray


def step_intervals(schedule, t: torch.Tensor) -> _Intervals:
    """What ``Scenario.table`` needs of a solve stepped by ``odeint(..., options=dict(step_size=...))`` on the
    module's layers, whose outputs need not be grid hits: the output interval of every step, the last j with
    ``t[j] <= grid[n]`` up to GRID_SNAP_ULPS roundings of the largest time.  On the forecast's daily grid
    ``arange(T) / 7`` stepped by ``t[1] - t[0]`` the grid ``k * fl(1/7)`` misses ``fl(k / 7)`` by a rounding
    (``_forecast_plan``): step k is then output interval k.  Where every output is a grid hit this is the
    schedule's own expansion."""
    th = t.detach().cpu().to(torch.float64)
    tol = GRID_SNAP_ULPS * torch.finfo(t.dtype).eps * float(th.abs().max())
    starts = schedule.grid[:-1].to(torch.float64) + tol
    j = torch.searchsorted(th, starts, right=True) - 1
    return _Intervals(j.clamp(0, len(th) - 2).numpy())


def _grid_hits(plan) -> Sequence[int]:
    """The grid point of every output time of a launch plan or schedule whose outputs are all grid hits."""
    out_k = getattr(plan, "out_k", None)
    if out_k is None and hasattr(plan, "out_start"):
        if plan.n_steps >= 1 and all(int(m) == 1 for m in plan.out_mode):
            out_k = [0] + [n + 1 for n in range(plan.n_steps)
                           for _ in range(int(plan.out_start[n + 1] - plan.out_start[n]))]
    if out_k is None:
        raise ValueError("Scenario: an output time of this solve is not a grid point (intervals do not map to steps)")
    return out_k


def _scale_vector(scale, R: int, device) -> Optional[torch.Tensor]:
    """What ``_scale_forecast`` accepts (something with ``.values``, or array-like) -> (R,) fp64."""
    if scale is None:
        return None
    if isinstance(scale, torch.Tensor):
        s = scale.detach().to(device=device, dtype=torch.float64).reshape(-1)
    else:
        s = torch.from_numpy(np.asarray(scale.values if hasattr(scale, "values") else scale,
                                        dtype=np.float64).reshape(-1)).to(device)
    if s.numel() != R:
        raise ValueError(f"scale has {s.numel()} entries for {R} regions")
    return s.contiguous()


def _ndtr(x: torch.Tensor) -> torch.Tensor:
    """scipy.special.ndtr's branches (cephes ndtr.c), as the kernel's fc_ndtr.  torch.special.ndtr forms
    (1 + erf) / 2 in the upper tail, which rounds twice: a mass of 1e-9 six standard deviations above the
    mean then differs from SciPy's in its seventh digit."""
    a = x * 0.70710678118654752440
    z = a.abs()
    half = 0.5 * torch.erfc(z)
    return torch.where(z < 0.70710678118654752440, 0.5 + 0.5 * torch.erf(a), torch.where(a > 0, 1.0 - half, half))


def _lerp_quantile(vs: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """numpy.quantile 'linear' (_lerp) of ``vs`` (T, S, B, R), sorted along dim 1, at the levels ``q``
    (Q,): (Q, T, B, R).  The arithmetic of the kernel's fc_quantile."""
    S = vs.shape[1]
    h = (S - 1) * q
    lo = h.floor().clamp(0, S - 1)
    gm = (h - lo).view(-1, 1, 1, 1)
    lo = lo.long()
    hi = (lo + 1).clamp(max=S - 1)
    x, y = vs[:, lo].movedim(1, 0), vs[:, hi].movedim(1, 0)
    d = y - x
    return torch.where(gm >= 0.5, y - d * (1.0 - gm), x + d * gm)


def _sorted_crps(xs: torch.Tensor, y: torch.Tensor, dim: int = 0, v: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The kernels' CRPS (fc_col_crps) of the samples ``xs``, sorted along ``dim``, against ``y`` (xs's
    shape without ``dim``).  ``v``: the tensor whose ``|v - y|`` are summed when it is not ``xs``
    (``_verify_torch`` sums the unsorted samples: another order, other bits)."""
    S = xs.shape[dim]
    rank = (torch.arange(S, dtype=torch.float64, device=xs.device) * 2 - (S - 1)).view(
        [S if d == dim else 1 for d in range(xs.dim())])
    return ((xs if v is None else v) - y.unsqueeze(dim)).abs().sum(dim) / S - (rank * xs).sum(dim) / (S * S)


def _floored_log(count: torch.Tensor, S: int) -> torch.Tensor:
    """log(count / S), an exactly zero count as MASS_FLOOR."""
    return torch.where(count == 0, torch.full(count.shape, MASS_FLOOR, dtype=torch.float64, device=count.device),
                       count.to(torch.float64) / S).log()


def _window_log_mass(v: torch.Tensor, y: torch.Tensor, dim: int) -> torch.Tensor:
    """The kernels' fc_window_log_mass: the floored log of the fraction of the samples ``v`` (along ``dim``)
    in the multibin window ``[cb - 0.5, cb + 0.6)``, ``cb = floor(10 y) / 10``, of ``y`` (v's shape without
    ``dim``)."""
    cb = (y * 10.0).floor() / 10.0
    return _floored_log(((v >= (cb - 0.5).unsqueeze(dim)) & (v < (cb + 0.6).unsqueeze(dim))).sum(dim), v.shape[dim])


def _verify_torch(out: Forecast, v, y, mean, nll, mass, verify: Verify) -> None:
    """The ``verify`` fields from v (T, S, B, R) and y / mean / nll / mass (T, B, R), all scaled fp64."""
    T, S, B, R = v.shape
    n = float(B * R)
    vs = v.sort(dim=1).values
    crps = _sorted_crps(vs, y, 1, v)
    al = torch.tensor(verify.alphas, dtype=torch.float64, device=v.device)
    K, J = al.numel(), int(verify.pit_bins)
    lo, up = _lerp_quantile(vs, 0.5 * al), _lerp_quantile(vs, 1.0 - 0.5 * al)          # (K, T, B, R)
    med = _lerp_quantile(vs, torch.tensor([0.5], dtype=torch.float64, device=v.device))[0]
    a4 = al.view(K, 1, 1, 1)
    wis = (0.5 * (y - med).abs() + (0.5 * a4 * ((up - lo) + (2.0 / a4) * (lo - y).clamp(min=0)
                                                + (2.0 / a4) * (y - up).clamp(min=0))).sum(0)) / (K + 0.5)
    cover = ((lo <= y) & (y <= up)).to(torch.float64)
    mid = (v < y.unsqueeze(1)).sum(1) + (v <= y.unsqueeze(1)).sum(1)                   # n_lt + n_le
    pit_bin = torch.div(J * mid, 2 * S, rounding_mode="floor").clamp(max=J - 1)
    log_emp = _window_log_mass(v, y, 1)
    out.crps, out.wis = crps.mean((1, 2)), wis.mean((1, 2))
    out.ens_skill = log_emp.mean((1, 2)).exp()
    out.coverage = cover.sum((2, 3)) / n
    out.pit = torch.nn.functional.one_hot(pit_bin, J).to(torch.float64).sum((1, 2)) / n
    out.nll_r, out.skill_r, out.mae_r = nll.mean(1), mass.log().mean(1).exp(), (y - mean).abs().mean(1)
    out.crps_r, out.wis_r, out.ens_skill_r = crps.mean(1), wis.mean(1), log_emp.mean(1).exp()
    out.coverage_r = cover.sum(2) / float(B)


def _summary_torch(yhat, S, B, y_true, scale, q, verify: Optional[Verify] = None) -> Forecast:
    T, N, R = yhat.shape
    v = yhat.detach().to(torch.float64).reshape(T, S, B, R)
    if scale is not None:
        v = v * scale
    mean = v.mean(1)
    std = ((v - mean.unsqueeze(1)) ** 2).mean(1).sqrt()
    out = Forecast(mean.permute(1, 0, 2).contiguous(), std.permute(1, 0, 2).contiguous())
    if q is not None and q.numel() > 0:
        out.quantiles = torch.quantile(v, q, dim=1).permute(0, 2, 1, 3).contiguous()     # (Q, T, B, R) -> (Q, B, T, R)
    if y_true is not None:
        y = y_true.detach().to(torch.float64).permute(1, 0, 2)                           # (T, B, R)
        if scale is not None:
            y = y * scale
        z = (y - mean) / std
        nll = 0.5 * z * z + std.log() + 0.5 * math.log(2 * math.pi)
        mass = _ndtr((y + 0.6 - mean) / std) - _ndtr((y - 0.5 - mean) / std)
        mass = torch.where(mass == 0, torch.full_like(mass, MASS_FLOOR), mass)
        out.nll = nll.mean((1, 2))
        out.skill = mass.log().mean((1, 2)).exp()
        out.mae = (y - mean).abs().mean((1, 2))
        if verify is not None:
            _verify_torch(out, v, y, mean, nll, mass, verify)
    return out


def _library() -> Optional["_native.NativeLib"]:
    """Any loaded / loadable library (the summary kernels have no model)."""
    import os
    if os.path.exists(_native.PREBUILT_LIB):
        return _native.prebuilt()
    for path in _native.loaded_paths():
        return _native._load(path)
    return None


def _prepare(who: str, values, n_samples, batch, y_true, scale, quantiles, sorts: bool):
    """The arguments ``ensemble_summary`` and ``ensemble_season`` (``who``, for the messages) share, checked:
    ``(T, S, B, R, device, scale (R,) fp64 or None, levels fp64 or None, their number, lib, values, y_true)``.
    ``sorts``: the kernel sorts its tile whatever the levels, so the device's sample cap holds without them.
    ``lib`` is None where the torch definitions run (a CPU tensor, no library); otherwise ``values`` and
    ``y_true`` come back as the kernels read them, fp32 and contiguous on the device."""
    if values.dim() != 3 or values.shape[1] != n_samples * batch:
        raise ValueError(f"{who}: values {tuple(values.shape)} are not (T, {n_samples}*{batch}, R)")
    T, N, R = (int(v) for v in values.shape)
    S, B = int(n_samples), int(batch)
    if y_true is not None and tuple(y_true.shape) != (B, T, R):
        raise ValueError(f"{who}: targets {tuple(y_true.shape)} are not ({B}, {T}, {R})")
    dev = values.device
    sc = _scale_vector(scale, R, dev)
    q = None
    if quantiles is not None and len(quantiles) > 0:
        q = torch.as_tensor(np.asarray(quantiles, dtype=np.float64), device=dev)
        if bool(((q < 0) | (q > 1)).any()):
            raise ValueError(f"{who}: quantile levels must lie in [0, 1]")
    if (sorts or q is not None) and S > MAX_QUANTILE_SAMPLES and values.is_cuda:
        raise ValueError(f"{who}: n_samples <= {MAX_QUANTILE_SAMPLES} on the device (the kernel sorts its tile)")
    lib = _library() if values.is_cuda else None
    if lib is not None:
        values = values.detach().to(torch.float32).contiguous()
        y_true = None if y_true is None else y_true.detach().to(device=dev, dtype=torch.float32).contiguous()
    return T, S, B, R, dev, sc, q, (0 if q is None else int(q.numel())), lib, values, y_true


def ensemble_summary(yhat: torch.Tensor, n_samples: int, batch: int, y_true: Optional[torch.Tensor] = None,
                     scale=None, quantiles: Optional[Sequence[float]] = None, verify=None) -> Forecast:
    """Summary of ``yhat`` (T, S*B, R) (sample n = s*B + b, as the solve emits it) over its S
    samples: see ``Forecast``.  ``scale``: per-region multiplier of predictions and targets (the
    data scaler); ``y_true`` (B, T, R); ``quantiles``: levels in [0, 1] (numpy.quantile, 'linear').
    ``verify``: None, True (``Verify()``) or a ``Verify`` -- with targets, also the scores of the
    ensemble itself (``Forecast``); the other fields keep their bits.  A HIP tensor runs
    ude_forecast_summary (ude_forecast_verify with ``verify``, n_samples <= 1024); a CPU tensor (or no
    library) the same definitions in torch fp64."""
    if verify is True:
        verify = Verify()
    if verify is not None:
        if not isinstance(verify, Verify):
            raise TypeError("ensemble_summary: verify is None, True or a Verify")
        if y_true is None:
            raise ValueError("ensemble_summary: verify needs the targets y_true")
    T, S, B, R, dev, sc, q, n_q, lib, yh, yt = _prepare("ensemble_summary", yhat, n_samples, batch, y_true, scale,
                                                        quantiles, sorts=verify is not None)
    if lib is None:
        return _summary_torch(yhat, S, B, y_true, sc, q, verify)
    with torch.cuda.device(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        mean = torch.empty((B, T, R), **f64)
        std = torch.empty((B, T, R), **f64)
        quant = torch.empty((n_q, B, T, R), **f64) if n_q else None
        scores = torch.empty((3, T), **f64) if yt is not None else None
        p = _fused._ptr
        if verify is None:
            ws = torch.empty(max(lib.forecast_summary_workspace(T, S, B, R, n_q) // 8, 1), **f64) if yt is not None else None
            with _fused._timed("forecast_summary"):
                lib.forecast_summary(T, S, B, R, yh.data_ptr(), p(sc), p(yt), p(q), n_q, p(ws), mean.data_ptr(),
                                     std.data_ptr(), p(quant), p(scores), _fused._stream(dev))
        else:
            K, J = len(verify.alphas), int(verify.pit_bins)
            al = torch.tensor(verify.alphas, **f64)
            day = torch.empty((3 + K + J, T), **f64)
            region = torch.empty((6 + K, T, R), **f64)
            ws = torch.empty(lib.forecast_verify_workspace(T, S, B, R, n_q, K, J) // 8, **f64)
            with _fused._timed("forecast_verify"):
                lib.forecast_verify(T, S, B, R, yh.data_ptr(), p(sc), p(yt), p(q), n_q, al.data_ptr(), K, J,
                                    ws.data_ptr(), mean.data_ptr(), std.data_ptr(), p(quant), scores.data_ptr(),
                                    day.data_ptr(), region.data_ptr(), _fused._stream(dev))
    out = Forecast(mean, std, quant)
    if scores is not None:
        out.nll, out.skill, out.mae = scores[0], scores[1].exp(), scores[2]
    if verify is not None:
        out.crps, out.wis, out.ens_skill = day[0], day[1], day[2].exp()
        out.coverage, out.pit = day[3:3 + K], day[3 + K:].t().contiguous()
        out.nll_r, out.skill_r, out.mae_r = region[0], region[1].exp(), region[2]
        out.crps_r, out.wis_r, out.ens_skill_r = region[3], region[4], region[5].exp()
        out.coverage_r = region[6:]
    return out


def _season_walk(v: torch.Tensor, base: Optional[torch.Tensor], run: int):
    """``(peak, when, total, onset or None)`` over dim 0 of ``v`` (M, ..., R) (scaled fp64): the largest
    value, the first index that attains it, the sum with m ascending, and with ``base`` (R,) the first m
    that starts ``run`` consecutive values at or above it, M where there is none."""
    M = v.shape[0]
    idx = torch.arange(M, device=v.device).view(M, *([1] * (v.dim() - 1)))
    peak = v.amax(0)
    when = torch.where(v == peak, idx, M).amin(0)
    total = v[0].clone()
    for m in range(1, M):
        total = total + v[m]
    if base is None:
        return peak, when, total, None
    onset = torch.full_like(when, M)
    if run <= M:
        above = torch.cat([torch.zeros_like(v[:1], dtype=torch.int64), (v >= base).to(torch.int64).cumsum(0)])
        hit = (above[run:] - above[:M - run + 1]) == run                                  # (M - run + 1, ...)
        onset = torch.where(hit, idx[:M - run + 1], M).amin(0)
    return peak, when, total, onset


def _set_season_scores(out: SeasonTargets, overall, region, has_onset: bool) -> None:
    """``overall[k]`` / ``region[k]`` of ``SEASON_SCORES[k]`` into ``out`` and its ``*_r`` fields.  Both
    routes hold a skill as its mean log: ``exp`` on the way out.  Without a baseline there is no onset score."""
    for k, name in enumerate(SEASON_SCORES):
        if name == "onset_skill" and not has_onset:
            continue
        skill = name.endswith("_skill")
        setattr(out, name, overall[k].exp() if skill else overall[k])
        setattr(out, name + "_r", region[k].exp() if skill else region[k])


def _season_torch(yhat, S, B, season: Season, M, y_true, scale, base, q) -> SeasonTargets:
    T, N, R = yhat.shape
    v = yhat.detach()[season.start::season.every].to(torch.float64).reshape(M, S, B, R)
    if scale is not None:
        v = v * scale
    peak, when, total, onset = _season_walk(v, base, season.run)                          # (S, B, R)
    stat = lambda x: (x.mean(0), ((x - x.mean(0)) ** 2).mean(0).sqrt())
    hist = lambda i, n: torch.nn.functional.one_hot(i, n).sum(0)                           # (B, R, n) counts
    n_when = hist(when, M)
    out = SeasonTargets(*stat(peak), *stat(total), (n_when.to(torch.float64) / S).permute(0, 2, 1).contiguous())
    ps, ts = peak.sort(dim=0).values, total.sort(dim=0).values
    if q is not None and q.numel() > 0:
        out.peak_quantiles = _lerp_quantile(ps.unsqueeze(0), q)[:, 0].contiguous()
        out.total_quantiles = _lerp_quantile(ts.unsqueeze(0), q)[:, 0].contiguous()
    n_onset = None
    if onset is not None:
        n_onset = hist(onset, M + 1)
        out.onset = (n_onset.to(torch.float64) / S).permute(0, 2, 1).contiguous()
    if y_true is None:
        return out
    y = y_true.detach().to(torch.float64).permute(1, 0, 2)[season.start::season.every]      # (M, B, R)
    if scale is not None:
        y = y * scale
    y_peak, y_when, y_total, y_onset = _season_walk(y, base, season.run)                   # (B, R)
    bins = torch.arange(M + 1, device=v.device)
    near = lambda o: ((bins - o.unsqueeze(-1)).abs() <= season.window) & (bins < M)       # (B, R, M + 1)
    logs = [_floored_log((n_when * near(y_when)[..., :M]).sum(-1), S)]
    if onset is not None:
        mask = torch.where((y_onset == M).unsqueeze(-1), bins == M, near(y_onset))
        logs.append(_floored_log((n_onset * mask).sum(-1), S))
    else:
        logs.append(None)
    logs.append(_window_log_mass(peak, y_peak, 0))
    terms = logs + [_sorted_crps(ps, y_peak), _sorted_crps(ts, y_total)]
    _set_season_scores(out, [t if t is None else t.mean() for t in terms],
                       [t if t is None else t.mean(0) for t in terms], onset is not None)
    return out


def ensemble_season(values: torch.Tensor, n_samples: int, batch: int, season: Season,
                    y_true: Optional[torch.Tensor] = None, scale=None,
                    quantiles: Optional[Sequence[float]] = None) -> SeasonTargets:
    """The seasonal targets of ``values`` (T, S*B, R) fp32 (sample n = s*B + b: ``y_hat`` as the solve
    emits it, or one dynamics channel ``dyn[c]``) over the output indices ``season`` considers: see
    ``SeasonTargets``.  ``scale`` / ``y_true`` (B, T, R) / ``quantiles`` as ``ensemble_summary`` takes them;
    ``season.baseline`` is in scaled units.  A HIP tensor runs ude_forecast_season (one read of the
    considered values, n_samples <= 1024); a CPU tensor (or no library) the same definitions in torch
    fp64."""
    if not isinstance(season, Season):
        raise TypeError("ensemble_season: season is a Season")
    T, S, B, R, dev, sc, q, n_q, lib, yh, yt = _prepare("ensemble_season", values, n_samples, batch, y_true, scale,
                                                        quantiles, sorts=True)
    M = season.times(T)
    base = season.baseline_vector(R, dev)
    if lib is None:
        return _season_torch(values, S, B, season, M, y_true, sc, base, q)
    opts = (season.start, season.every, season.run, season.window)
    with torch.cuda.device(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        stats = torch.empty((4, B, R), **f64)
        quant = torch.empty((2, n_q, B, R), **f64) if n_q else None
        peak_time = torch.empty((B, M, R), **f64)
        onset = torch.empty((B, M + 1, R), **f64) if base is not None else None
        overall = torch.empty(len(SEASON_SCORES), **f64) if yt is not None else None
        region = torch.empty((len(SEASON_SCORES), R), **f64) if yt is not None else None
        ws = torch.empty(lib.forecast_season_workspace(T, S, B, R, n_q, *opts) // 8, **f64) if yt is not None else None
        p = _fused._ptr
        with _fused._timed("forecast_season"):
            lib.forecast_season(T, S, B, R, *opts, yh.data_ptr(), p(sc), p(base), p(yt), p(q), n_q, p(ws),
                                stats.data_ptr(), p(quant), peak_time.data_ptr(), p(onset), p(overall), p(region),
                                _fused._stream(dev))
    out = SeasonTargets(stats[0], stats[1], stats[2], stats[3], peak_time, onset=onset)
    if quant is not None:
        out.peak_quantiles, out.total_quantiles = quant[0], quant[1]
    if yt is not None:
        _set_season_scores(out, overall, region, base is not None)
    return out


JOINT_CHUNK = 1 << 25                    # elements of the torch route's largest temporary (fp64: 256 MB)


def _window_mean(x: torch.Tensor) -> torch.Tensor:
    """The mean over dim 0 as the kernels' fc_group_mean forms it: x[0] + x[1] + .., divided once."""
    acc = x[0].clone()
    for b in range(1, x.shape[0]):
        acc = acc + x[b]
    return acc / x.shape[0]


def _variogram_torch(x: torch.Tensor, y: torch.Tensor, p: float) -> torch.Tensor:
    """The variogram score of every block: x (C, S, ...) the samples and y (C, ...) the target at the block's C
    coordinates -> (...).  One coordinate at a time against those after it: the temporary is (C, S, ...)."""
    power = (lambda d: d.abs().sqrt()) if p == 0.5 else (lambda d: d.abs())
    out = torch.zeros(y.shape[1:], dtype=torch.float64, device=x.device)
    for c in range(x.shape[0] - 1):
        mean = power(x[c + 1:] - x[c]).sum(1) / x.shape[1]
        out = out + ((power(y[c + 1:] - y[c]) - mean) ** 2).sum(0)
    return out


def _joint_torch(yhat, S, B, joint: Joint, M, y_true, scale) -> JointScores:
    T, N, R = yhat.shape
    v_all = yhat.detach()[joint.start::joint.every].to(torch.float64).reshape(M, S, B, R)
    y_all = y_true.detach().to(device=yhat.device, dtype=torch.float64).permute(1, 0, 2)[joint.start::joint.every]
    if scale is not None:
        v_all, y_all = v_all * scale, y_all * scale                                    # (M, S, B, R), (M, B, R)
    nb = max(1, min(B, JOINT_CHUNK // (M * S * R)))                                   # windows per chunk
    cols = [[] for _ in range(5)]
    for b0 in range(0, B, nb):
        v, y = v_all[:, :, b0:b0 + nb], y_all[:, b0:b0 + nb]
        n = v.shape[2]
        d2 = (v - y.unsqueeze(1)) ** 2                                                 # the first term
        first = [d2.sum((0, 3)).sqrt().sum(0), d2.sum(0).sqrt().sum(0), d2.sum(3).sqrt().sum(1)]
        pairs = [torch.zeros_like(f) for f in first]                                   # (n,), (n, R), (M, n)
        ni = max(1, min(S, JOINT_CHUNK // (M * S * n * R)))                            # samples i per chunk
        for i0 in range(0, S, ni):
            d2 = (v[:, i0:i0 + ni, None] - v[:, None]) ** 2                            # (M, ni, S, n, R)
            pairs[0] = pairs[0] + d2.sum((0, 4)).sqrt().sum((0, 1))
            pairs[1] = pairs[1] + d2.sum(0).sqrt().sum((0, 1))
            pairs[2] = pairs[2] + d2.sum(4).sqrt().sum((1, 2))
        es = [f / S - q / (2.0 * S * S) for f, q in zip(first, pairs)]
        cols[0].append(es[0])
        cols[1].append(es[1])
        cols[2].append(es[2].t())
        cols[3].append(_variogram_torch(v, y, joint.p))                                # blocks (n, R) over M
        cols[4].append(_variogram_torch(v.permute(3, 1, 2, 0), y.permute(2, 1, 0), joint.p))  # blocks (n, M) over R
    e_joint, e_series, e_field, v_series, v_field = (torch.cat(c).contiguous() for c in cols)
    return JointScores(e_joint, e_series, e_field, v_series, v_field, _window_mean(e_joint), _window_mean(e_series),
                       _window_mean(e_field), _window_mean(v_series), _window_mean(v_field))


def ensemble_joint(values: torch.Tensor, n_samples: int, batch: int, y_true: torch.Tensor, joint: Joint = Joint(),
                   scale=None) -> JointScores:
    """The joint scores of ``values`` (T, S*B, R) fp32 (sample n = s*B + b: ``y_hat`` as the solve emits it, or
    one dynamics channel) against ``y_true`` (B, T, R) over the output indices ``joint`` considers: see
    ``JointScores``.  ``scale`` as ``ensemble_summary`` takes it.  A HIP tensor runs ude_forecast_joint (one read
    of the considered values for the energy scores, direct fp64 differences, fixed-order sums; n_samples <= 1024,
    at most 4096 regions and considered times); a CPU tensor (or no library) the same definitions in torch fp64,
    in chunks of at most about 256 MB."""
    if not isinstance(joint, Joint):
        raise TypeError("ensemble_joint: joint is a Joint")
    if y_true is None:
        raise ValueError("ensemble_joint: the joint scores need the targets y_true")
    T, S, B, R, dev, sc, _q, _nq, lib, yh, yt = _prepare("ensemble_joint", values, n_samples, batch, y_true, scale,
                                                         None, sorts=True)
    M = joint.times(T)
    if lib is None:
        return _joint_torch(values, S, B, joint, M, y_true, sc)
    if R > MAX_JOINT_COORDS or M > MAX_JOINT_COORDS:
        raise ValueError(f"ensemble_joint: at most {MAX_JOINT_COORDS} regions and considered times on the device")
    opts = (joint.start, joint.every, int(2 * joint.p))
    with torch.cuda.device(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        e_joint, e_series, e_field = torch.empty(B, **f64), torch.empty((B, R), **f64), torch.empty((B, M), **f64)
        v_series, v_field = torch.empty((B, R), **f64), torch.empty((B, M), **f64)
        means = torch.empty(1 + 2 * R + 2 * M, **f64)
        ws = torch.empty(lib.forecast_joint_workspace(T, S, B, R, *opts) // 8, **f64)
        with _fused._timed("forecast_joint"):
            lib.forecast_joint(T, S, B, R, *opts, yh.data_ptr(), _fused._ptr(sc), yt.data_ptr(), ws.data_ptr(),
                               e_joint.data_ptr(), e_series.data_ptr(), e_field.data_ptr(), v_series.data_ptr(),
                               v_field.data_ptr(), means.data_ptr(), _fused._stream(dev))
    parts = means.split([1, R, M, R, M])
    return JointScores(e_joint, e_series, e_field, v_series, v_field, parts[0].reshape(()), *parts[1:])


def check_levels(who: str, levels, R: Optional[int] = None) -> Dict[str, Aggregate]:
    """``levels`` as a dict name -> ``Aggregate`` (TypeError for anything else, ValueError for none or, with
    ``R``, for a level whose weights have another number of regions)."""
    if not hasattr(levels, "items"):
        raise TypeError(f"{who}: the levels are a mapping name -> ude_amd.forecast.Aggregate")
    levels = dict(levels.items())
    for name, lv in levels.items():
        if not isinstance(lv, Aggregate):
            raise TypeError(f"{who}: level {name!r} is not an ude_amd.forecast.Aggregate")
        if R is not None and lv.n_regions != R:
            raise ValueError(f"{who}: level {name!r} has weights for {lv.n_regions} regions, the values have {R}")
    if not levels:
        raise ValueError(f"{who}: no level")
    return levels


def _stack_levels(who: str, levels, R: int, dev, native: bool):
    """``(levels, w (G_tot, R) fp64 on dev, g_off)``: the levels' rows stacked in the mapping's order, level l's
    first row ``g_off[l]``; with ``native`` the device's limits hold."""
    levels = check_levels(who, levels, R)
    g_off = [0]
    for lv in levels.values():
        g_off.append(g_off[-1] + lv.n_groups)
    if native and (R > MAX_AGGREGATE_REGIONS or g_off[-1] > MAX_AGGREGATE_GROUPS or len(levels) > MAX_AGGREGATE_LEVELS):
        raise ValueError(f"{who}: at most {MAX_AGGREGATE_REGIONS} regions, {MAX_AGGREGATE_GROUPS} groups over all "
                         f"levels and {MAX_AGGREGATE_LEVELS} levels on the device")
    return levels, torch.cat([lv.on(dev) for lv in levels.values()]).contiguous(), g_off


def _weighted_sums(v: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """``acc = 0; acc = acc + w[:, r] * v[..., r]`` for r ascending: v (..., R) fp64, w (G, R) -> (..., G) fp64.
    Elementwise, so every product and sum is rounded on its own in the order the kernel has."""
    acc = torch.zeros(v.shape[:-1] + (w.shape[0],), dtype=torch.float64, device=v.device)
    for r in range(v.shape[-1]):
        acc = acc + w[:, r] * v[..., r, None]
    return acc


def ensemble_aggregate(values: torch.Tensor, levels, scale=None) -> Dict[str, torch.Tensor]:
    """The weighted sums over the regions of ``values`` (..., R) (read as fp32; any leading dimensions: ``y_hat``
    (T, S*B, R), targets (B, T, R)) for every level of ``levels``, a mapping name -> ``Aggregate``: a dict name
    -> fp32 tensor (..., G_l).  Per element of the leading dimensions and group g, in fp64: ``acc = 0``, then
    ``acc = acc + w[g, r] * (values[..., r] * scale[r])`` for r ascending, every product and sum rounded on its own,
    stored as fp32 -- the aggregated ensemble is that fp32 array, which ``ensemble_summary`` and the others read
    with ``scale=None``.  A HIP tensor runs ude_forecast_aggregate, one call and one read of ``values`` for all
    levels (at most 4096 regions, 256 groups in all, 16 levels); a CPU tensor (or no library) the same operations
    in torch fp64, r by r: the same bits."""
    if values.dim() < 1 or values.shape[-1] < 1:
        raise ValueError(f"ensemble_aggregate: values {tuple(values.shape)} are not (..., R)")
    R, lead = int(values.shape[-1]), tuple(values.shape[:-1])
    dev = values.device
    lib = _library() if values.is_cuda else None
    levels, w, g_off = _stack_levels("ensemble_aggregate", levels, R, dev, lib is not None)
    sc = _scale_vector(scale, R, dev)
    x = values.detach().to(torch.float32)
    if lib is None:
        v = x.to(torch.float64)
        if sc is not None:
            v = v * sc
        acc = _weighted_sums(v, w).to(torch.float32)
        return {name: acc[..., g_off[l]:g_off[l + 1]].contiguous() for l, name in enumerate(levels)}
    x = x.contiguous()
    rows = x.numel() // R
    with torch.cuda.device(dev):
        out = torch.empty(rows * g_off[-1], dtype=torch.float32, device=dev)
        if rows:                                 # an empty tensor has no address to hand over
            with _fused._timed("forecast_aggregate"):
                lib.forecast_aggregate(rows, R, len(levels), _i32_array(g_off), x.data_ptr(), _fused._ptr(sc),
                                       w.data_ptr(), out.data_ptr(), _fused._stream(dev))
    return {name: out[rows * g_off[l]:rows * g_off[l + 1]].view(*lead, g_off[l + 1] - g_off[l])
            for l, name in enumerate(levels)}


def _i32_array(v: Sequence[int]):
    import ctypes
    return (ctypes.c_int32 * len(v))(*v)


def aggregate_dynamics(dyn: torch.Tensor, names: Sequence[str], levels) -> Dict[str, Tuple[torch.Tensor, Tuple[str, ...]]]:
    """The dynamics ``dyn`` (C, T, N, R) (read as fp32; the channels ``names`` of ``dynamics_names``) of every
    level of ``levels``: a dict name -> ``(dyn_l (C, T, N, G_l) fp32, names)``.  With the summation of
    ``ensemble_aggregate`` (fp64, r ascending, no scale): s, i, r and fa_* are the weighted sums; with ``inc =
    sum w (beta s) i`` and ``rec = sum w gamma i``, the aggregate's new infections and recoveries per unit time,
    ``beta = inc / (s i)``, ``gamma = rec / i`` and ``r_eff = inc / rec`` of the aggregate's own s and i -- the
    rates one SIR population with the aggregate's S and I would need, so ``r_eff = beta s / gamma``; the regional
    ``r_eff`` is not read (its mean is not the aggregate's reproduction number).  Plain IEEE divisions (i = 0:
    inf or NaN), each channel rounded once to fp32.  A HIP tensor runs ude_forecast_aggregate_dyn, one call for
    all levels; a CPU tensor (or no library) the same operations in torch fp64."""
    names = tuple(names)
    rates, flux = "beta" in names, "fa_s" in names
    if dyn.dim() != 4 or names != DYN_STATE + (DYN_RATES if rates else ()) + (DYN_FLUX if flux else ()) \
            or dyn.shape[0] != len(names) or not (rates or flux):
        raise ValueError(f"aggregate_dynamics: dyn {tuple(dyn.shape)} is not (C, T, N, R) with the channels of "
                         f"dynamics_names, {names}")
    C, T, N, R = (int(v) for v in dyn.shape)
    dev = dyn.device
    lib = _library() if dyn.is_cuda else None
    levels, w, g_off = _stack_levels("aggregate_dynamics", levels, R, dev, lib is not None)
    x = dyn.detach().to(torch.float32)
    if lib is None:
        v = x.to(torch.float64)
        ch = {n: _weighted_sums(v[c], w) for c, n in enumerate(names) if n != "r_eff" and n not in ("beta", "gamma")}
        if rates:
            s, i, beta, gamma = v[0], v[1], v[names.index("beta")], v[names.index("gamma")]
            inc, rec = _weighted_sums((beta * s) * i, w), _weighted_sums(gamma * i, w)
            ch["beta"], ch["gamma"], ch["r_eff"] = inc / (ch["s"] * ch["i"]), rec / ch["i"], inc / rec
        acc = torch.stack([ch[n] for n in names]).to(torch.float32)
        return {name: (acc[..., g_off[l]:g_off[l + 1]].contiguous(), names) for l, name in enumerate(levels)}
    x = x.contiguous()
    rows = T * N
    kind = (1 if rates else 0) | (2 if flux else 0)
    with torch.cuda.device(dev):
        out = torch.empty(C * rows * g_off[-1], dtype=torch.float32, device=dev)
        if rows:
            with _fused._timed("forecast_aggregate_dyn"):
                lib.forecast_aggregate_dyn(kind, rows, R, len(levels), _i32_array(g_off), x.data_ptr(), w.data_ptr(),
                                           out.data_ptr(), _fused._stream(dev))
    return {name: (out[C * rows * g_off[l]:C * rows * g_off[l + 1]].view(C, T, N, g_off[l + 1] - g_off[l]), names)
            for l, name in enumerate(levels)}


def aggregate_forecasts(levels, yhat, n_samples: int, batch: int, y_true=None, scale=None, quantiles=None,
                        verify=None, dyn=None, season: Optional[Season] = None, joint: Optional[Joint] = None
                        ) -> Dict[str, Forecast]:
    """What ``VAE.forecast(aggregate=levels)`` adds: per level the ``Forecast`` of the aggregated ensemble.
    ``y_hat`` and the targets are aggregated with the scaler, ``dyn = (dyn, names)`` without, one call each for
    all levels; then every level's block goes through ``ensemble_summary`` (``quantiles``, ``verify``),
    ``dynamics_summary``, ``ensemble_season`` (``season`` with the level's ``baseline``, or without an onset) and
    ``ensemble_joint`` as the baseline did, with ``scale=None``."""
    levels = check_levels("forecast", levels, int(yhat.shape[-1]))
    yh = ensemble_aggregate(yhat, levels, scale)
    yt = ensemble_aggregate(y_true.to(yhat.device), levels, scale) if y_true is not None else None
    dy = aggregate_dynamics(dyn[0], dyn[1], levels) if dyn is not None else None
    out = {}
    for name, lv in levels.items():
        y_l = None if yt is None else yt[name]
        fc = ensemble_summary(yh[name], n_samples, batch, y_true=y_l, quantiles=quantiles, verify=verify)
        if dy is not None:
            fc.dynamics = dynamics_summary(dy[name][0], dy[name][1], n_samples, batch, quantiles=quantiles)
        if season is not None:
            s_l = Season(lv.baseline, season.start, season.every, season.run, season.window)
            fc.season = ensemble_season(yh[name], n_samples, batch, s_l, y_true=y_l, quantiles=quantiles)
        if joint is not None:
            fc.joint = ensemble_joint(yh[name], n_samples, batch, y_l, joint)
        out[name] = fc
    return out


GRID_SNAP_ULPS = 8


def _forecast_plan(ode, y0, t, step_size):
    """The launch plan of the forecast solve.  The decoder epilogue needs every output time on the
    grid.  torchdiffeq builds the grid of a ``step_size`` solve as ``t[0] + k * step`` in t's dtype; on
    the forecast's daily grid ``arange(T) / 7`` with ``step = t[1] - t[0]`` (lib/utils.py:21 through
    lib/VAE.py:137) that is ``k * fl(1/7)`` against ``t[k] = fl(k / 7)``: the same points up to a
    rounding, which makes about half of the outputs "interpolations" with slope 1 - O(1e-7).  When the
    two grids have the same length and agree to GRID_SNAP_ULPS roundings of the largest time, the
    solve steps on ``t`` itself (torchdiffeq's grid without a step size): every output is then a grid
    hit.  Against the interpolating schedule that moves an output by at most (1 - slope) = O(1e-6) of
    one step's change, and each step size by a rounding of t."""
    from . import solvers
    from .schedule import fixed_grid
    plan = solvers.plan_for(ode, y0, t, step_size)
    if plan.out_k is not None or step_size is None:
        return plan
    th = t.detach().cpu()
    grid = fixed_grid(th, step_size)
    tol = GRID_SNAP_ULPS * torch.finfo(th.dtype).eps * float(th.abs().max())
    if len(grid) == len(th) and float((grid - th).abs().max()) <= tol:
        return solvers.plan_for(ode, y0, t, None)
    return plan


def _scenario_table(scenario, plan, R: int, dev) -> torch.Tensor:
    """The device table of ``scenario`` -- a ``Scenario``, or an fp32 ``(n_steps, R, 2)`` tensor that is read in
    place when it is contiguous and 8-byte aligned on ``dev``."""
    shape = (int(plan.prob.n_steps), int(R), 2)
    if isinstance(scenario, Scenario):
        return scenario.table(plan, R).to(dev)
    if not isinstance(scenario, torch.Tensor) or tuple(scenario.shape) != shape:
        raise ValueError(f"solve_decode_scenario: scenario is a Scenario or a {shape} table")
    table = scenario.detach().to(device=dev, dtype=torch.float32).contiguous()
    return table.clone() if table.data_ptr() % 8 else table


def _solve_decode(ode, y0: torch.Tensor, t: torch.Tensor, step_size, linear, n_dyn: int = 0,
                  out: Optional[torch.Tensor] = None, scenario=None):
    """The inference solve with the decoder epilogue behind ``solve_decode_forecast`` (``n_dyn`` = 0:
    ude_rk4_forecast_dec), ``solve_decode_dynamics`` (``n_dyn`` channels into ``out`` or a new tensor:
    ude_rk4_forecast_dyn) and ``solve_decode_scenario`` (``scenario``: ude_rk4_forecast_scn): ``(y_hat, dyn or
    None, RateStats)``, or None when an output time is not a grid point.  Without a scenario the solve's
    side statistics are recorded on ``ode``; a scenario's belong to the counterfactual and are only returned."""
    with torch.no_grad(), torch.cuda.device(y0.device):
        plan = _forecast_plan(ode, y0, t, step_size)
        if plan.out_k is None:
            return None
        dev = y0.device
        stream = _fused._stream(dev)
        sz = plan.sizes
        y0 = y0.detach().contiguous()
        if getattr(ode, "uncertainty", "none") == "bayes":
            mus, sds = ode.ude_mean_std()
            eps = ode.take_eps(4 * plan.prob.n_steps, sum(int(p.numel()) for p in mus), dev)
            pack = _fused._bayes_pack(plan, mus, sds, eps, dev)
        else:
            params = []
            for lin in ode.ude_linears():
                params += [lin.weight, lin.bias]
            pack = _fused.packed_weights(plan, params, dev)
        Wd, bd = linear.weight.detach().contiguous(), linear.bias.detach().contiguous()
        dec_pack = torch.empty(sz.dec_pack_bytes // 4, dtype=torch.float32, device=dev)
        plan.lib.pack_decoder(plan.desc, Wd.data_ptr(), bd.data_ptr(), dec_pack.data_ptr(), stream)
        N, R, L = y0.shape
        yhat = torch.empty((plan.n_times, N, R), dtype=torch.float32, device=dev)
        dyn = None
        if n_dyn:
            shape = (n_dyn, plan.n_times, N, R)
            if out is None:
                dyn = torch.empty(shape, dtype=torch.float32, device=dev)
            else:
                if tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
                    raise ValueError(f"solve_decode_dynamics: out must be a contiguous fp32 {shape} tensor on {dev}")
                dyn = out
        stats_slab = torch.empty(max(sz.stats_slab_bytes // 8, 1), dtype=torch.float64, device=dev)
        stats, sums, st = _fused._stats_out(plan, dev)
        head = (plan.desc, plan.prob, pack.data_ptr(), plan.sched_dev.data_ptr(), y0.data_ptr(), dec_pack.data_ptr(),
                yhat.data_ptr())
        tail = (stats_slab.data_ptr(), _fused._ctl(plan, dev).data_ptr(), st, stream)
        rates = RateStats(*stats)
        if scenario is not None:
            table = _scenario_table(scenario, plan, R, dev)
            with _fused._timed("forecast_scn"):
                plan.lib.forecast_scn(*head[:-1], table.data_ptr(), yhat.data_ptr(), _fused._ptr(dyn), *tail)
            return yhat, dyn, rates
        if dyn is None:
            with _fused._timed("forecast_dec"):
                plan.lib.forecast_dec(*head, *tail)
        else:
            with _fused._timed("forecast_dyn"):
                plan.lib.forecast_dyn(*head, dyn.data_ptr(), *tail)
        ode._record_fused(stats, plan.n_eval, sums=sums)
    return yhat, dyn, rates


def solve_decode_forecast(ode, y0: torch.Tensor, t: torch.Tensor, step_size, linear) -> Optional[torch.Tensor]:
    """y_hat (T, N, R) = Decoder(odeint(ode, y0, t)[..., :3]) of the inference solve
    (ude_rk4_forecast_dec: no autograd, no latent, no checkpoint), or None when the decoder epilogue
    does not apply (``decoder_head.eligible``) or an output time is not a grid point.  Records the
    solve's side statistics on ``ode`` as every fused solve does (``posterior()``, the tracker)."""
    if not decoder_head.eligible(ode, y0, linear):
        return None
    res = _solve_decode(ode, y0, t, step_size, linear)
    return None if res is None else res[0]


def solve_decode_dynamics(ode, y0: torch.Tensor, t: torch.Tensor, step_size, linear,
                          out: Optional[torch.Tensor] = None
                          ) -> Optional[Tuple[torch.Tensor, torch.Tensor, Tuple[str, ...]]]:
    """``solve_decode_forecast`` that also emits the dynamics (ude_rk4_forecast_dyn): ``(y_hat (T, N, R),
    dyn (C, T, N, R) fp32, names)`` with the channels of ``dynamics_names(ode)`` -- at every output time
    the state ``latent[..., :3]``, the rate net's beta / gamma at that state and ``r_eff = beta * s /
    gamma`` (fp32), the augmentation net's raw Fa -- or None where ``solve_decode_forecast`` gives None
    and for a Bayesian RHS (the evaluation at the last output time is not one of the solve's, so it has
    no weight sample).  ``y_hat`` and the side statistics recorded on ``ode`` are ``solve_decode_forecast``'s
    bit for bit: the evaluation at the last output time is not counted.  ``out``: a contiguous fp32
    (C, T, N, R) tensor on y0's device to receive ``dyn`` (exactly its C * T * N * R floats are written)."""
    if getattr(ode, "uncertainty", "none") == "bayes" or not decoder_head.eligible(ode, y0, linear):
        return None
    names = dynamics_names(ode)
    res = _solve_decode(ode, y0, t, step_size, linear, len(names), out)
    return None if res is None else (res[0], res[1], names)


def solve_decode_scenario(ode, y0: torch.Tensor, t: torch.Tensor, step_size, linear, scenario, dynamics: bool = False,
                          out: Optional[torch.Tensor] = None):
    """``solve_decode_forecast`` under a scenario (ude_rk4_forecast_scn): ``(y_hat (T, N, R), dyn (C, T, N, R)
    or None, names, RateStats)``.  ``scenario``: a ``Scenario``, or its ``(n_steps, R, 2)`` fp32 table.  All
    four stages of RK4 step k scale the rate net's outputs of region r by row k before the flux (beta' =
    m_beta |q0|, gamma' = m_gamma |q1|; Fa, the mask and the update unchanged), so a scenario of ones gives
    ``solve_decode_forecast``'s bits.  With ``dynamics`` the channels of ``solve_decode_dynamics`` (into
    ``out`` when given) report what entered the flux: beta', gamma', r_eff = beta' s / gamma'; an output that
    starts a step uses that step's row, the last output the last step's.  The ``RateStats`` are the scaled
    rates'; nothing is recorded on ``ode``.  None where ``solve_decode_dynamics`` gives None and for a model
    without a rate net (Fa)."""
    if getattr(ode, "uncertainty", "none") == "bayes" or ode.ode_type not in ("Fp", "FaFp") \
            or not decoder_head.eligible(ode, y0, linear):
        return None
    names = dynamics_names(ode)
    res = _solve_decode(ode, y0, t, step_size, linear, len(names) if dynamics else 0, out, scenario)
    return None if res is None else (res[0], res[1], names, res[2])


def _output_rows(scenario: Scenario, T: int, R: int) -> torch.Tensor:
    """The multipliers behind every output's dynamics, ``(T, R, 2)``: those of the step that starts at the
    output -- its interval's --, the last interval's for the last output."""
    rows = scenario.intervals(T, R)
    return torch.from_numpy(rows[list(range(T - 1)) + [T - 2]])


def _scenario_latent(ode, y0: torch.Tensor, t: torch.Tensor, step_size, table: torch.Tensor):
    """``scenario_latent`` and the ``RateStats`` of its evaluations (in the latent's dtype)."""
    from .solvers import _step_rk4
    from .schedule import fixed_grid
    grid = fixed_grid(t, step_size).to(y0.device)
    if tuple(table.shape) != (len(grid) - 1, ode.n_regions, 2):
        raise ValueError(f"scenario_latent: table {tuple(table.shape)} is not ({len(grid) - 1}, {ode.n_regions}, 2)")
    table = table.detach().to(device=y0.device, dtype=y0.dtype)
    tt = t.to(y0.device)
    kept = (ode._params, ode.tracker)
    ode._params, ode.tracker = [], []                 # the attribute, not the property: no reset of fused statistics
    try:
        with torch.no_grad():
            out, j, y = [y0], 1, y0
            for n in range(len(grid) - 1):
                ode.rate_scale = table[n]
                t0, t1 = grid[n], grid[n + 1]
                y1 = y + _step_rk4(ode, t0, t1 - t0, t1, y)
                while j < len(tt) and t1 >= tt[j]:
                    out.append(y if tt[j] == t0 else y1 if tt[j] == t1 else y + (tt[j] - t0) / (t1 - t0) * (y1 - y))
                    j += 1
                y = y1
            latent = torch.stack(out, 0)
            p = torch.stack(ode._params).reshape(-1, 2)
            fa = torch.norm(torch.stack(ode.tracker)).reshape(1) if ode.tracker else None
            return latent, RateStats(p.mean(0), p.std(0), fa)
    finally:
        ode.rate_scale = None
        ode._params, ode.tracker = kept


def scenario_latent(ode, y0: torch.Tensor, t: torch.Tensor, step_size, table: torch.Tensor) -> torch.Tensor:
    """The latent ``(T, N, R, L)`` of the solve under a scenario on the module's own layers: the fixed-grid
    3/8-rule loop of ``odeint(method='rk4')`` (``solvers.eager_fixed_grid``, the same operations in the same
    order) with ``ode.rate_scale = table[k]`` during step k -- all four stages, the one at the step's end
    time included -- under ``no_grad``.  ``table``: ``(n_steps, R, 2)`` for the grid of ``t`` / ``step_size``.
    Leaves ``ode.params`` / ``ode.tracker`` as they were and ``rate_scale`` None, also after an exception.
    Serves a CPU model, an ineligible decoder and every case ``solve_decode_scenario`` gives None for."""
    if ode.ode_type not in ("Fp", "FaFp"):
        raise ValueError("scenario_latent: a scenario scales the rate net's beta and gamma; this model has none")
    return _scenario_latent(ode, y0, t, step_size, table)[0]


def _mean_stack(stack, h: torch.Tensor) -> torch.Tensor:
    """A net's layers on ``h`` (N, R * L): Linears as they are, variational layers at their mean weights."""
    for m in stack:
        if isinstance(m, torch.nn.Flatten):
            continue
        if hasattr(m, "w_mean"):
            h = torch.nn.functional.linear(h, m.w_mean, m.b_mean)
        else:
            h = m(h)
    return h


def latent_dynamics(ode, latent: torch.Tensor, rate_scale: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, Tuple[str, ...]]:
    """The channels of ``solve_decode_dynamics`` from a written latent (T, N, R, L), in its dtype:
    ``(dyn (C, T, N, R), names)``.  The state is ``latent[..., :3]``; the nets are evaluated once at every
    output state without touching ``ode.params`` / ``ode.tracker`` (on a HIP device by the evaluation
    kernel, ude_amd/eval_rhs.py, else by the module's layers); ``r_eff = beta * s / gamma`` in the latent's
    dtype.  A Bayesian RHS is evaluated at its MEAN weights (no draw is taken from its stream): the
    rates and flux of the posterior mean network, not of the per-evaluation samples of the solve.
    ``rate_scale`` (T, R, 2): a scenario's multipliers per output time -- beta and gamma are scaled by them
    (one rounding each) before ``r_eff``, as ``solve_decode_scenario`` reports them."""
    names = dynamics_names(ode)
    with torch.no_grad():
        lat = latent.detach()
        T, N, R, L = lat.shape
        x = lat.reshape(T * N, R, L).contiguous()
        bayes = getattr(ode, "uncertainty", "none") == "bayes"
        rates = fa = None
        from . import eval_rhs
        if x.is_cuda and eval_rhs.eligible(ode, x):
            weights = [w.detach() for w in (ode.ude_mean_std()[0] if bayes else
                                            [p for lin in ode.ude_linears() for p in (lin.weight, lin.bias)])]
            _f, rates, fa = eval_rhs.rhs_eval(ode, x, weights)
        else:
            h = x.reshape(T * N, R * L)
            if "beta" in names:
                rates = torch.abs(_mean_stack(ode.Fp_net if bayes else ode._p_stack(), h)).reshape(T * N, R, 2)
            if "fa_s" in names:
                fa = _mean_stack(ode.aug_net if bayes else ode._a_stack(), h).reshape(T * N, R, 3)
        ch = [x[..., 0], x[..., 1], x[..., 2]]
        if rate_scale is not None and rates is not None:
            rates = (rates.reshape(T, N, R, 2) * rate_scale.to(rates).reshape(T, 1, R, 2)).reshape(T * N, R, 2)
        if "beta" in names:
            ch += [rates[..., 0], rates[..., 1], rates[..., 0] * x[..., 0] / rates[..., 1]]
        if "fa_s" in names:
            ch += [fa[..., 0], fa[..., 1], fa[..., 2]]
        dyn = torch.stack(ch).reshape(len(names), T, N, R)
    return dyn, names


def dynamics_summary(dyn: torch.Tensor, names: Sequence[str], n_samples: int, batch: int,
                     quantiles: Optional[Sequence[float]] = None) -> Dynamics:
    """``Dynamics`` of ``dyn`` (C, T, S*B, R): one ``ensemble_summary`` of the stacked channels
    ``(C*T, S*B, R)``, without scale or targets."""
    C, T, N, R = (int(v) for v in dyn.shape)
    fc = ensemble_summary(dyn.reshape(C * T, N, R), n_samples, batch, quantiles=quantiles)
    B = int(batch)
    quant = None if fc.quantiles is None else fc.quantiles.view(-1, B, C, T, R).permute(0, 2, 1, 3, 4)
    return Dynamics(tuple(names), fc.mean.view(B, C, T, R).permute(1, 0, 2, 3),
                    fc.std.view(B, C, T, R).permute(1, 0, 2, 3), quant)
