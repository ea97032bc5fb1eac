"""Drop-in `Solver` for the reference's `--solver stabilized_schur_vascularbc_backflow`
(src/solvers/stabilized_schur_vascularbc_backflow.py there): the `stabilized_schur_pressurebc` step (rotational form,
natural pressures) for a pressure-driven vessel whose outlet may see flow reversal during a pulsatile cycle.

* inlet (`tags["inlet"]`): natural pressure `p_inlet / 2` and the three Nitsche tangential terms, as in
  `stabilized_schur_pressurebc` (:219, :225-235);
* outlet (`tags["outlet"]`): a pure traction boundary (:220, :237-244) -- the natural pressure `initial_ffr * p_inlet / 2`, FIXED
  (no per-step resistance update; `R_resistance` is accepted and unused, :71), none of the Nitsche / curl terms, and the backflow
  stabilisation `-beta_backflow rho (u_prev . n)_- (u_mid . v)`, `(s)_- = (s - |s|) / 2` (Moghadam et al. 2011, eq. 10), the term
  of `stabilized_schur_backflow` with the coefficient from `u_prev` and the velocity `u_mid`.

Constructor as in the reference: `p_inlet` is required (ValueError otherwise, :78-82); `initial_ffr` 0.8, `beta_nitsche` 100,
`beta_backflow` 0.2, `p_grade` 1; `v_max` is accepted (:83).  The per-boundary switches of `cfdh_set_pressure_boundaries_ex` select
the terms: `nitsche = [1, 0]`, `beta_backflow = [0, beta]` for `[inlet, outlet]`.  Runs where the other pressure-driven plugins
run (gdim 2; hexahedra and P2 tetrahedra in gdim 3; one GPU).
"""
from __future__ import annotations

import math
from typing import Callable

import numpy as np

from .stabilized_schur_pressurebc import Solver as _PressureSolver


class Solver(_PressureSolver):
    MAX_ITER = 20

    def __init__(self, mesh, dt: float, rho: float, mu: float, f: list,
                 initial_velocity: Callable[[np.ndarray], np.ndarray] = None,
                 p_inlet: float = None, R_resistance: float = None, initial_ffr: float = 0.8, beta_nitsche: float = 100.0,
                 beta_backflow: float = 0.2, p_grade: int = 1, v_max: float = None, **kwargs):
        if p_inlet is None:
            raise ValueError("p_inlet is required for stabilized_schur_vascularbc_backflow. Pass it via CLI: --p_inlet <value>")
        self.v_max = float(v_max) if v_max is not None else None
        self.initial_ffr = float(initial_ffr)
        # taken here, before the pressure-driven base drops the scenario-level keywords of the other stenosis solvers
        self.beta_backflow = float(beta_backflow)
        if not (self.beta_backflow >= 0.0 and math.isfinite(self.beta_backflow)):
            raise ValueError("beta_backflow must be finite and >= 0")
        # p_outlet = initial_ffr * p_inlet, halved like every pressure of the form (:85-88)
        self._init_pressure_driven(mesh, dt, rho, mu, f, initial_velocity, float(p_inlet), self.initial_ffr * float(p_inlet), beta_nitsche,
                                   p_grade, kwargs)

    def _banner(self):
        return (f"[Solver] p_grade={self.p_grade}, beta_nitsche={self.beta_nitsche}, beta_backflow={self.beta_backflow:.2f}, "
                f"initial_ffr={self.initial_ffr}, p_outlet={self._p_outlet_val * 2:.4f}, v_max={self.v_max}")

    def _apply_pressures(self):
        # [inlet, outlet]: Nitsche on the inlet only; the outlet is a traction boundary with backflow stabilisation
        self.ctx.set_pressure_boundaries(self._pb_markers, [self._p_inlet_val, self._p_outlet_val], self.beta_nitsche,
                                         nitsche=[1, 0], beta_backflow=[0.0, self.beta_backflow])
