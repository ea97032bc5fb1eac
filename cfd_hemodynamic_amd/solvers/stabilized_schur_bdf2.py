"""Drop-in `Solver` for the reference's `--solver stabilized_schur_bdf2`
(/root/reference/src/solvers/stabilized_schur_bdf2.py:39-326): the same SUPG/PSPG/LSIC P1/P1
Newton/Schur-FGMRES step as `stabilized_schur`, but fully implicit in space (u_mid = u_sol,
:79-92) with the time term (a0 u + a1 u_prev + a2 u_prev2)/dt (:82-86,105-110): BDF1 on the
first step, BDF2 afterwards (:298-305).

Runs on the same gfx950 kernels: `cfdh_set_time_scheme(theta=1, a0, a1, a2)` selects the
scheme, `u_prev2` lives in HBM and is shifted on the device (`cfdh_shift_history`, the copy of
:324) at the end of every `solveStep()`.

Public attributes follow the reference: `u_prev2` (Function on V), `step_count`,
`bdf_a0/bdf_a1/bdf_a2` (objects with a `.value`, as the reference's Constants).
"""
from __future__ import annotations

from typing import Callable

import numpy as np

from ._bdf2_history import Bdf2History
from .stabilized_schur import Solver as _MidpointSolver


class Solver(Bdf2History, _MidpointSolver):
    MAX_ITER = 20

    def __init__(self, mesh, dt: float, rho: float, mu: float, f: list,
                 initial_velocity: Callable[[np.ndarray], np.ndarray] = None, **kwargs):
        super().__init__(mesh, dt, rho, mu, f, initial_velocity, **kwargs)
        self._init_bdf2_history(mesh)  # u_prev2, bdf_a0/a1/a2, step_count; solveStep of the mixin
