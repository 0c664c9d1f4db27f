"""MI355X-native UDE influenza forecaster: the batched RK4 solve of the SIR-UDE
right-hand side (forward + backward through the solver) as gfx950 kernels,
behind the reference's own API (lib/models.py classes, torchdiffeq.odeint).
"""
from .rhs import Fp, Fa, FaFp, UDE_CLASSES
from .solvers import odeint, fusable
from .adjoint import odeint_adjoint
from .forecast import (Aggregate, Dynamics, Forecast, Joint, JointScores, Scenario, ScenarioForecast, Season, SeasonTargets, Verify,
                       aggregate_dynamics, ensemble_aggregate, ensemble_joint, ensemble_season, ensemble_summary, scenario_latent, solve_decode_dynamics,
                       solve_decode_forecast, solve_decode_scenario)
from . import _native, configs

__all__ = ["Fp", "Fa", "FaFp", "odeint", "odeint_adjoint", "fusable", "UDE_CLASSES", "Forecast",
           "Verify", "ensemble_summary", "solve_decode_forecast", "Dynamics", "solve_decode_dynamics", "Season",
           "SeasonTargets", "ensemble_season", "Scenario", "ScenarioForecast", "solve_decode_scenario",
           "scenario_latent", "Joint", "JointScores", "ensemble_joint", "Aggregate",
           "ensemble_aggregate", "aggregate_dynamics"]
