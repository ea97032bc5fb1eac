"""`--solver stabilized_pcd_bdf2`: `stabilized_pcd` (implicit spatial terms, Eisenstat-Walker forcing, PCD Schur approximation,
`pc_type 2`) with the time term (a0 u + a1 u_prev + a2 u_prev2)/dt of `stabilized_schur_bdf2` -- BDF1 on the first step, BDF2
afterwards.  K of the PCD operator follows the scheme through its time coefficient c_t = rho a0 / (theta dt)
(include/cfdh.h: cfdh_set_schur_pcd), so it carries 1.5 rho / dt from the second step on.

Public attributes as in `stabilized_schur_bdf2`: `u_prev2`, `step_count`, `bdf_a0/bdf_a1/bdf_a2`.  Cells, refusals and `setup` as
in `stabilized_pcd`: P1 triangles and tetrahedra on one GPU, `tags["inlet"]` / `tags["outlet"]` required.
"""
from __future__ import annotations

from typing import Callable

import numpy as np

from ._bdf2_history import Bdf2History
from .stabilized_pcd import Solver as _PcdSolver


class Solver(Bdf2History, _PcdSolver):
    MAX_ITER = 20

    def __init__(self, mesh, dt: float, rho: float, mu: float, f: list,
                 initial_velocity: Callable[[np.ndarray], np.ndarray] = None, **kwargs):
        super().__init__(mesh, dt, rho, mu, f, initial_velocity, **kwargs)
        self._init_bdf2_history(mesh)
