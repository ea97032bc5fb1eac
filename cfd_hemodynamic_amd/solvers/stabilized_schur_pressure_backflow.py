"""Drop-in `Solver` for the reference's `--solver stabilized_schur_pressure_backflow`
(`src/solvers/stabilized_schur_pressure_backflow.py:58-419` there): pressure-driven flow in the CONVECTIVE epsilon-form,
the volume form of `stabilized_schur_backflow`, which the closed-form P1 kernels assemble.  Only boundary terms are new
(cfdh_set_traction_boundaries, csrc/cfdh_traction.hip):

* inlet (`tags["inlet"]`): weak pressure `p_inlet v . n` with the Nitsche condition on the tangential velocity
  `- (2 mu eps(u) n) . v_T - (2 mu eps(v) n) . u_T + (beta_nitsche mu / h) u_T . v_T` (:191-201);
* outlet (`tags["outlet"]`): `0.5 p_c v . n - (2 mu eps(u) n) . v` (:208-209) with the resistance pressure `p_c = R |Q|` and the
  backflow stabilisation `- beta_backflow rho (u_prev . n)_- u . v` (:213-217);
* no ds pair of the base form, no pressure Dirichlet condition: `bcp` is ignored (:233); walls as given in `bcu`.

`p_inlet` enters the form as given (:192-193; the scenario halves it), the outlet value is `0.5 p_c` (:208).

Resistance update, literally as in the reference (:204-207, :383-392, :419): Q is the flux of **u_prev** through the outlet.
`p_c = R |Q(u_prev)|` at setup, and after every step `p_c <- alpha R |Q(u_prev)| + (1 - alpha) p_c` -- at that point u_prev is
still the PREVIOUS step's solution (the scenario copies u_sol into it after solveStep returns), so the outlet pressure trails the
flow by one step.  The update changes only the boundary VALUE: Jacobian and preconditioner of the context stay valid.

Constructor as in the reference: `p_inlet` and `R_resistance` are required (ValueError otherwise, :73-83), `beta_nitsche` 100,
`beta_backflow` 0.2, `alpha_damping` 0.75, `p_grade` 1.  P1 triangles and P1 tetrahedra on one GPU; `p_grade=2`, quadrilateral
and hexahedral meshes and a partitioned `comm` are refused before any device work.
"""
from __future__ import annotations

from typing import Callable

import numpy as np

from ..boundaryCondition import BoundaryCondition
from .stabilized_schur import Solver as _MidpointSolver

# scenario-level keywords meant for the other stenosis solvers (stenosis.py:84-99)
_FOREIGN = ("v_max", "p_inlet", "p_outlet", "initial_ffr", "beta_nitsche", "beta_backflow", "R_resistance", "alpha_damping")


def damped_outlet_pressure(p_old: float, Q: float, R_resistance: float, alpha_damping: float) -> float:
    """p_c <- alpha R |Q| + (1 - alpha) p_c (:389-391)."""
    return alpha_damping * (R_resistance * abs(Q)) + (1 - alpha_damping) * p_old


def refuse_unsupported(name, mesh, p_grade, kwargs):
    """What the closed-form traction kernels do not cover, before a context exists."""
    if int(p_grade) != 1:
        raise NotImplementedError("%s: p_grade=%r is not supported, the traction boundaries run on the closed-form P1 kernels "
                                  "(p_grade=1)" % (name, p_grade))
    cell = mesh.topology.cell_name()
    if cell not in ("triangle", "tetrahedron"):
        raise NotImplementedError("%s: %s cells are not supported, the traction boundaries run on P1 triangles and tetrahedra"
                                  % (name, cell))
    comm = kwargs.get("comm", None)
    if comm is not None and comm.size > 1:
        raise NotImplementedError("%s runs on one GPU: partitioned runs are not supported" % name)


class ResistanceOutlet:
    """The outlet half shared with `stabilized_schur_velocity_vascular_backflow`: traction outlet with backflow stabilisation whose
    value 0.5 p_c follows the damped resistance rule.  The host class provides ctx, R_resistance, alpha_damping, beta_backflow,
    _tb_markers / _tb_tangential / _tb_backflow and _tb_values()."""

    def _apply_tractions(self):
        self.ctx.set_traction_boundaries(self._tb_markers, self._tb_values(), self.beta_nitsche, tangential=self._tb_tangential,
                                         beta_backflow=self._tb_backflow)

    def _outlet_flux_prev(self):
        return self.ctx.functional(8, self._outlet_marker)   # int u_prev . n ds_out (:211, :383-385)

    def _init_outlet_pressure(self):
        Q = self._outlet_flux_prev()
        self._p_c = self.R_resistance * abs(Q)                # :204-207
        self.p_c_initial = self._p_c
        self._apply_tractions()

    def _update_outlet_pressure(self):
        Q = self._outlet_flux_prev()
        self._p_c = damped_outlet_pressure(self._p_c, Q, self.R_resistance, self.alpha_damping)
        self._apply_tractions()                               # value-only change
        self.outlet_history.append((Q, self._p_c))
        if self.mesh.comm.rank == 0 and not self._quiet:
            print(f"  Resistance BC: Q={Q:.6e}, p_new={self.R_resistance * abs(Q):.4f}, "
                  f"p_damped={self._p_c:.4f} (alpha={self.alpha_damping:.2f})")


class Solver(ResistanceOutlet, _MidpointSolver):
    MAX_ITER = 20

    def __init__(self, mesh, dt: float, rho: float, mu: float, f: list,
                 initial_velocity: Callable[[np.ndarray], np.ndarray] = None,
                 p_inlet: float = None, beta_nitsche: float = 100.0, beta_backflow: float = 0.2, R_resistance: float = None,
                 alpha_damping: float = 0.75, p_grade: int = 1, **kwargs):
        if p_inlet is None:
            raise ValueError(
                "p_inlet is required for stabilized_schur_pressure_backflow. "
                "Pass it via CLI: --p_inlet <value> (in physical units, e.g. Pa)"
            )
        if R_resistance is None:
            raise ValueError(
                "R_resistance is required for stabilized_schur_pressure_backflow. "
                "Pass it via CLI: --R_resistance <value>"
            )
        refuse_unsupported("stabilized_schur_pressure_backflow", mesh, p_grade, kwargs)
        self.p_inlet = float(p_inlet)
        self.beta_nitsche = float(beta_nitsche)
        self.beta_backflow = float(beta_backflow)
        self.R_resistance = float(R_resistance)
        self.alpha_damping = float(alpha_damping)
        self.p_grade = int(p_grade)
        self.outlet_history = []  # (Q(u_prev), p_c) after every step
        self._p_c = 0.0
        for k in _FOREIGN + ("p_grade",):
            kwargs.pop(k, None)
        super().__init__(mesh, dt, rho, mu, f, initial_velocity, **kwargs)
        if mesh.comm.rank == 0 and not self._quiet:
            print(f"[Solver] p_grade={p_grade}, p_inlet={self.p_inlet:.4f}, beta_nitsche={self.beta_nitsche:.2f}, "
                  f"beta_backflow={self.beta_backflow:.2f}, R_resistance={self.R_resistance:.4e}, "
                  f"alpha_damping={self.alpha_damping:.2f}", flush=True)

    def _tb_values(self):
        return [self.p_inlet, 0.5 * self._p_c]   # :193, :208

    def setup(self, bcu: list[BoundaryCondition], bcp: list[BoundaryCondition], facet_tags=None, tags=None) -> None:
        if tags is None or tags.get("inlet") is None or tags.get("outlet") is None:
            raise KeyError("inlet/outlet")  # the reference indexes tags["inlet"], tags["outlet"] (:174, :180)
        self._outlet_marker = int(tags["outlet"])
        self._tb_markers = [int(tags["inlet"]), self._outlet_marker]
        self._tb_tangential = [True, False]
        self._tb_backflow = [0.0, self.beta_backflow]
        self._ds_terms = False
        self.ctx.set_traction_boundaries([], [])
        self.ctx.set_boundary_terms(ds_terms=False)
        super().setup(bcu, [], facet_tags, tags)  # self.bcp_d = [] (:233); uploads u_prev
        self._init_outlet_pressure()

    def solveStep(self):
        super().solveStep()
        self._update_outlet_pressure()  # :419
