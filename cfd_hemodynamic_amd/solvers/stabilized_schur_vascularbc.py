"""Drop-in `Solver` for the reference's `--solver stabilized_schur_vascularbc`
(/root/reference/src/solvers/stabilized_schur_vascularbc.py): the `stabilized_schur_pressurebc` step (rotational form, natural
pressure on inlet and outlet, Nitsche tangential condition) with a resistance outlet `p_out = R |Q|`, Q = int_outlet u . n,
updated between steps by a fixed point (:324-336, :387-408): after each converged step the outlet flux of the new solution sets
the outlet pressure of the next step.

The halving convention of the reference is kept: the inlet enters the form as `p_inlet / 2`, the first step's outlet as
`initial_ffr * p_inlet / 2` (:80-83) and every update as `R |Q| / 2` (:333-334).  `p_inlet` and `R_resistance` are required
(ValueError otherwise, :70-79); `initial_ffr` defaults to 0.8.  The per-step update changes only the boundary VALUE: the Jacobian
and the preconditioner of the context stay valid (cfdh_set_pressure_boundaries).
"""
from __future__ import annotations

from typing import Callable

import numpy as np

from .stabilized_schur_pressurebc import Solver as _PressureSolver


class Solver(_PressureSolver):
    MAX_ITER = 20

    def __init__(self, mesh, dt: float, rho: float, mu: float, f: list,
                 initial_velocity: Callable[[np.ndarray], np.ndarray] = None,
                 p_inlet: float = None, R_resistance: float = None, initial_ffr: float = 0.8, beta_nitsche: float = 100.0,
                 p_grade: int = 1, **kwargs):
        if p_inlet is None:
            raise ValueError("p_inlet is required for stabilized_schur_vascularbc. Pass it via CLI: --p_inlet <value>")
        if R_resistance is None:
            raise ValueError("R_resistance is required for stabilized_schur_vascularbc. Pass it via CLI: --R_resistance <value>")
        self.R_resistance = float(R_resistance)
        self.initial_ffr = float(initial_ffr)
        self.outlet_history = []  # (Q, p_outlet) after every step
        # p_outlet_0 = initial_ffr * p_inlet, halved like every pressure of the form (:80-83)
        self._init_pressure_driven(mesh, dt, rho, mu, f, initial_velocity, float(p_inlet), self.initial_ffr * float(p_inlet), beta_nitsche,
                                   p_grade, kwargs)

    def _banner(self):
        return (f"[Solver] p_grade={self.p_grade}, beta_nitsche={self.beta_nitsche}, R_resistance={self.R_resistance}, "
                f"initial_ffr={self.initial_ffr}, p_outlet_0={self._p_outlet_val * 2:.4f}")

    def _update_outlet_pressure(self):
        """p_outlet = R |Q| from the outlet flux of the current solution (:324-336)."""
        Q = self.ctx.functional(7, self._pb_markers[1])
        p_outlet_phys = self.R_resistance * abs(Q)
        self._p_outlet_val = p_outlet_phys / 2
        self._apply_pressures()  # value-only change
        self.outlet_history.append((Q, p_outlet_phys))
        if self.mesh.comm.rank == 0 and not self._quiet:
            print(f"  Resistance BC: Q={Q:.6e}, p_outlet={p_outlet_phys:.4f}")

    def solveStep(self):
        super().solveStep()
        self._update_outlet_pressure()  # fixed-point update for the next step (:407-408)
