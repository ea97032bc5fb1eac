"""Drop-in `Solver` for the reference's `--solver stabilized_schur_velocity_vascular_backflow`
(`src/solvers/stabilized_schur_velocity_vascular_backflow.py:57-412` there): the outlet half of
`stabilized_schur_pressure_backflow` with a velocity inlet.  Velocity Dirichlet data as given in `bcu` (walls and inlet profile),
`bcp` ignored (:221), no ds pair; on `tags["outlet"]` the traction terms `0.5 p_c v . n - (2 mu eps(u) n) . v` (:192-193) with the
resistance pressure `p_c = R |Q(u_prev)|`, damped between steps exactly as in the sibling (:188-191, :376-386), and the backflow
stabilisation (:197-205).  One traction boundary of cfdh_set_traction_boundaries, on the closed-form P1 kernels.

Constructor as in the reference: `v_max` and `R_resistance` are required (ValueError otherwise, :71-82), `p_grade` 1,
`beta_backflow` 0.2, `alpha_damping` 0.75.  The same meshes and refusals as the sibling.
"""
from __future__ import annotations

from typing import Callable

import numpy as np

from ..boundaryCondition import BoundaryCondition
from .stabilized_schur import Solver as _MidpointSolver
from .stabilized_schur_pressure_backflow import _FOREIGN, ResistanceOutlet, refuse_unsupported


class Solver(ResistanceOutlet, _MidpointSolver):
    MAX_ITER = 20

    def __init__(self, mesh, dt: float, rho: float, mu: float, f: list,
                 initial_velocity: Callable[[np.ndarray], np.ndarray] = None,
                 v_max: float = None, p_grade: int = 1, beta_backflow: float = 0.2, R_resistance: float = None,
                 alpha_damping: float = 0.75, **kwargs):
        if v_max is None:
            raise ValueError(
                "v_max is required for stabilized_schur_velocity_vascular_backflow. "
                "Pass it via CLI: --v_max <value>"
            )
        if R_resistance is None:
            raise ValueError(
                "R_resistance is required for stabilized_schur_velocity_vascular_backflow. "
                "Pass it via CLI: --R_resistance <value>"
            )
        refuse_unsupported("stabilized_schur_velocity_vascular_backflow", mesh, p_grade, kwargs)
        self.v_max = float(v_max)
        self.beta_nitsche = 0.0   # no boundary with tangential terms
        self.beta_backflow = float(beta_backflow)
        self.R_resistance = float(R_resistance)
        self.alpha_damping = float(alpha_damping)
        self.p_grade = int(p_grade)
        self.outlet_history = []  # (Q(u_prev), p_c) after every step
        self._p_c = 0.0
        for k in _FOREIGN:
            kwargs.pop(k, None)
        super().__init__(mesh, dt, rho, mu, f, initial_velocity, **kwargs)
        if mesh.comm.rank == 0 and not self._quiet:
            print(f"[Solver] p_grade={p_grade}, v_max={self.v_max:.4f}, beta_backflow={self.beta_backflow:.2f}, "
                  f"R_resistance={self.R_resistance:.4e}, alpha_damping={self.alpha_damping:.2f}", flush=True)

    def _tb_values(self):
        return [0.5 * self._p_c]   # :192

    def setup(self, bcu: list[BoundaryCondition], bcp: list[BoundaryCondition], facet_tags=None, tags=None) -> None:
        if tags is None or tags.get("outlet") is None:
            raise KeyError("outlet")  # the reference indexes tags["outlet"] (:175)
        self._outlet_marker = int(tags["outlet"])
        self._tb_markers = [self._outlet_marker]
        self._tb_tangential = [False]
        self._tb_backflow = [self.beta_backflow]
        self._ds_terms = False
        self.ctx.set_traction_boundaries([], [])
        self.ctx.set_boundary_terms(ds_terms=False)
        super().setup(bcu, [], facet_tags, tags)  # self.bcp_d = [] (:221); uploads u_prev
        self._init_outlet_pressure()

    def solveStep(self):
        super().solveStep()
        self._update_outlet_pressure()  # :412
