"""
lqrrt_amd -- MI355X-native expansion engine behind the jnez71/lqRRT Python API.

    import lqrrt_amd as lqrrt
    boat = lqrrt.systems.BoatAdvanced()
    constraints = lqrrt.Constraints(nstates=6, ncontrols=3, goal_buffer=boat.goal_buffer,
                                    is_feasible=boat.is_feasible)
    planner = lqrrt.Planner(boat.dynamics, boat.lqr, constraints, horizon=2, dt=0.1, FPR=0.9,
                            error_tol=boat.error_tol, erf=boat.erf, goal0=boat.goal)
    planner.update_plan(boat.x0, boat.sample_space, goal_bias=boat.goal_bias)

Exports mirror lqrrt/__init__.py:1-2 of the reference (Constraints, Planner) plus Tree and
the native problem plugins (systems), update_plans (several planners through shared native calls: one GPU, many
trees -- planner.py), refine_plans (their found plans shortened through shared calls), connect_goals (the plans whose
budget ran out before a goal hit connected to the goal through shared calls), connect_vias (the same through each planner's own
list of waypoints), fleet_goal_costs (what every planner's tree would pay to reach each of a shared list of places, one matrix
through shared calls), retargets (every planner given a new goal from the tree it holds, through shared calls) and deconflict
(prioritised planning over the trees as they stand: every planner picks the best plan of its tree that stays clear of the plans of
those before it, Planner.avoid) and avoids (Planner.avoid for a fleet against shared or
per-planner traffic: the trees of a group checked in one native call; with connect=goal_tries also the goal chains that stay clear
of that traffic, searched for all trees in the same call and committed in one more) and avoids_rects (Planner.avoid_rects for a
fleet: the same against moving oriented rectangles, other hulls).  Importing works without a GPU; computing does not.
"""
from .constraints import Constraints
from .planner import (Planner, update_plans, refine_plans, connect_goals, connect_vias, fleet_goal_costs, retargets, deconflict, avoids,
                      avoids_rects)
from .tree import Tree
from . import systems
from . import dare

__all__ = ["Constraints", "Planner", "Tree", "systems", "dare", "update_plans", "refine_plans", "connect_goals", "connect_vias",
           "fleet_goal_costs", "retargets", "deconflict", "avoids", "avoids_rects"]
