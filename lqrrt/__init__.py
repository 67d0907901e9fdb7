"""
`lqrrt` -- the reference's package name (lqrrt/__init__.py:1-2 exports Constraints and Planner), served by the
MI355X build: code written against jnez71/lqRRT keeps its `import lqrrt` line and gets lqrrt_amd's classes.
Tree and the native problem plugins (`systems`) are exported as well.
"""
from lqrrt_amd import (Constraints, Planner, Tree, systems, update_plans, refine_plans, connect_goals, connect_vias,  # noqa: F401
                       fleet_goal_costs, retargets, deconflict, avoids, avoids_rects)

__all__ = ["Constraints", "Planner", "Tree", "systems", "update_plans", "refine_plans", "connect_goals", "connect_vias",
           "fleet_goal_costs", "retargets", "deconflict", "avoids", "avoids_rects"]
