"""2-D stenosed channel driven by pressure -- the reference's `src/scenarios/stenosis_pressure.py` on the structured mesh of
`stenosis.StenosisSimulation`, for `--solver stabilized_schur_pressure_backflow`:

  * walls no-slip ONLY: no inlet velocity, even when `v_max` is given (it then shapes the initial velocity alone, :150-191);
  * no pressure condition (`bcp` empty, :145-148): the solver imposes the inlet pressure weakly and a resistance outlet;
  * `p_inlet` in mmHg (default 80), forwarded as `p_inlet * 133.322 * 0.5` (`_MMHG_2D`, :24-25: the halving of the 2-D form is done
    here, not in the solver); `R_resistance` is required (ValueError otherwise, :93-97);
  * `beta_nitsche` 100, `beta_backflow` 0.2, `alpha_damping` 0.75 and `p_grade` 1 are forwarded (:57-60, :99-106).

FFR is computed as in `stenosis` after `solve`.
"""
from __future__ import annotations

from ..boundaryCondition import BoundaryCondition
from ..fem import Function
from . import stenosis as _stenosis

_MMHG_2D = _stenosis._MMHG * 0.5  # stenosis_pressure.py:24-25


class StenosisPressureSimulation(_stenosis.StenosisSimulation):
    def __init__(self, solver_name, dt, T, f: tuple[float, float] = (0, 0), grade="severe", p_inlet: float = 80.0,
                 R_resistance: float = None, v_max: float = None, *, p_grade: int = 1, beta_nitsche: float = 100.0,
                 beta_backflow: float = 0.2, alpha_damping: float = 0.75, **kwargs):
        if R_resistance is None:
            raise ValueError(
                "R_resistance is required for pressure-driven inlet. "
                "Pass it via CLI: --R_resistance <value>"
            )
        for k in ("outlet_pressure", "p_outlet", "initial_ffr"):
            kwargs.pop(k, None)  # no pressure condition, no outlet pressure in this scenario
        # the parent forwards p_inlet * 133.322: half the value gives p_inlet * _MMHG_2D (a factor 1/2 is exact)
        super().__init__(solver_name, dt, T, f, grade, v_max=v_max, outlet_pressure=None, p_inlet=0.5 * float(p_inlet),
                         beta_nitsche=beta_nitsche, R_resistance=float(R_resistance), p_grade=p_grade, beta_backflow=beta_backflow,
                         alpha_damping=alpha_damping, **kwargs)
        self.scenario_name = "stenosis_pressure"

    @property
    def bcu(self):
        """Wall no-slip only: the inlet velocity is not prescribed (:131-143)."""
        if not self._bcu:
            bc_w = BoundaryCondition(Function(self.solver.V))
            bc_w.initTopological(1, self._ft.find(self.wall_marker))
            self._bcu = [bc_w]
        return self._bcu
