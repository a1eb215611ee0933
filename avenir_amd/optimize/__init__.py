"""Stochastic optimisation (reference J/optimize, S/optimize, P/mlextra/opti*.py): batched search
domains and population / multi-chain optimisers on device tensors."""
from .domain import AssignmentDomain, CallbackDomain, FunctionDomain, SearchDomain
from .domains import FeatureSubsetDomain, MeetingScheduleDomain, TaskScheduleSearch, geo_distance, read_lenient_json
from .eo import EoRun, eo_assign_advance, eo_assign_reference, eo_islands_reference
from .ga_meeting import eo_meeting_advance, eo_meeting_reference, sa_meeting_reference, sa_meeting_run
from .ga_subset import eo_subset_advance, eo_subset_reference, sa_subset_reference, sa_subset_run
from .sa import SaDomain, SaRun, sa_chains_init, sa_chains_reference, sa_exp
from .search import (BayesianOptimizer, EvolutionaryOptimizer, GeneticAlgorithm, OptResult, RandomSearch,
                     SimulatedAnnealing, TabuSearch, local_focussed, local_trajectory, parameter_search, sa_assign,
                     sa_assign_reference)
from .tabu import TabuRun, tabu_assign_advance, tabu_assign_reference

__all__ = [
    "AssignmentDomain", "CallbackDomain", "FunctionDomain", "SearchDomain", "FeatureSubsetDomain",
    "MeetingScheduleDomain", "TaskScheduleSearch", "geo_distance", "read_lenient_json", "BayesianOptimizer",
    "EvolutionaryOptimizer", "GeneticAlgorithm", "OptResult", "RandomSearch", "SimulatedAnnealing", "TabuSearch",
    "local_focussed", "local_trajectory", "parameter_search", "sa_assign", "sa_assign_reference",
    "SaDomain", "SaRun", "sa_chains_init", "sa_chains_reference", "sa_exp", "sa_meeting_reference", "sa_meeting_run",
    "sa_subset_reference", "sa_subset_run", "TabuRun", "tabu_assign_advance", "tabu_assign_reference",
    "EoRun", "eo_assign_advance", "eo_assign_reference", "eo_islands_reference", "eo_meeting_advance",
    "eo_meeting_reference", "eo_subset_advance", "eo_subset_reference",
]
