"""Drop-in `Solver` for the reference's `--solver stabilized_schur_pressurebc`
(/root/reference/src/solvers/stabilized_schur_pressurebc.py:43-205): flow driven by pressure.

* rotational (curl-curl) form: `mu omega(u_mid) omega(v)`, convection `rho (omega(u_mid) x u_mid) . v - rho/2 |u_mid|^2 div v`,
  no viscous part in the strong residual of SUPG / PSPG (:123-160); same tau, tau_L and time scheme as the base solver;
* natural pressure conditions `P v . n` on the inlet and outlet facets (`tags["inlet"]`, `tags["outlet"]`) with a Nitsche
  condition on the tangential velocity there (:177-205, penalty `beta_nitsche mu / h`);
* no ds pair of the base form, no pressure Dirichlet condition: `bcp` is ignored (:221); velocity Dirichlet data as given.

The reference stores HALF the given pressures (`_p_inlet_val = p_inlet / 2`, :64-65) and that is what enters the form; the same
halving is reproduced here.  Constructor as in the reference: `p_inlet` and `p_outlet` are required (ValueError otherwise, :59-63),
`beta_nitsche` defaults to 100, `p_grade` 1 or 2.  Runs on the generic element kernels on one GPU: gdim 2 (csrc/cfdh_gen.hip,
P1 triangles through CFDH_ELEM_P1_GENERIC), and gdim 3 (csrc/cfdh_gen3.hip, the curl form of :111-121) on hexahedra (Q1/Q1) and on
tetrahedra with `p_grade=2` (P2/P2).  P1 tetrahedra and a partitioned `comm` are refused before any device work.
"""
from __future__ import annotations

from typing import Callable

import numpy as np

from .. import _lib
from ..boundaryCondition import BoundaryCondition
from .stabilized_schur import Solver as _MidpointSolver

# scenario-level keywords meant for the other stenosis solvers (stenosis.py:84-99)
_FOREIGN = ("v_max", "beta_backflow", "R_resistance", "initial_ffr", "p_outlet")


def _refuse_unsupported(mesh, p_grade, kwargs):
    if int(p_grade) not in (1, 2):
        raise NotImplementedError("p_grade=%r: P1/P1 and P2/P2 run on the gfx950 kernels" % (p_grade,))
    if mesh.geometry.dim == 3 and mesh.topology.cell_name() == "tetrahedron" and int(p_grade) == 1:
        raise NotImplementedError("the pressure-driven solvers have no P1 tetrahedron variant in 3-D: "
                                  "pass p_grade=2 (P2/P2 tetrahedra) or use hexahedra (Q1/Q1)")
    comm = kwargs.get("comm", None)
    if comm is not None and comm.size > 1:
        raise NotImplementedError("the pressure-driven solvers run on one GPU: partitioned runs are not supported")


class Solver(_MidpointSolver):
    MAX_ITER = 20

    def __init__(self, mesh, dt: float, rho: float, mu: float, f: list,
                 initial_velocity: Callable[[np.ndarray], np.ndarray] = None,
                 p_inlet: float = None, p_outlet: float = None, beta_nitsche: float = 100.0, p_grade: int = 1, **kwargs):
        if p_inlet is None or p_outlet is None:
            raise ValueError(
                "p_inlet and p_outlet are required for stabilized_schur_pressurebc. "
                "Pass them via CLI: --p_inlet <value> --p_outlet <value>"
            )
        self._init_pressure_driven(mesh, dt, rho, mu, f, initial_velocity, float(p_inlet), float(p_outlet), beta_nitsche, p_grade, kwargs)

    def _init_pressure_driven(self, mesh, dt, rho, mu, f, initial_velocity, p_inlet, p_outlet, beta_nitsche, p_grade, kwargs):
        _refuse_unsupported(mesh, p_grade, kwargs)
        self._p_inlet_val = p_inlet / 2   # :64-65
        self._p_outlet_val = p_outlet / 2
        self.beta_nitsche = float(beta_nitsche)
        self.p_grade = int(p_grade)
        for k in _FOREIGN:
            kwargs.pop(k, None)
        kwargs["_degree"] = self.p_grade
        kwargs["generic_kernels"] = True  # P1 triangles through the quadrature kernels, where the rotational form lives
        super().__init__(mesh, dt, rho, mu, f, initial_velocity, **kwargs)
        self.ctx.set_formulation(_lib.FORM_ROTATIONAL)
        self._pb_markers = None
        if mesh.comm.rank == 0 and not self._quiet:
            print(self._banner(), flush=True)

    def _banner(self):
        return f"[Solver] p_grade={self.p_grade}, beta_nitsche={self.beta_nitsche}"

    def _apply_pressures(self):
        self.ctx.set_pressure_boundaries(self._pb_markers, [self._p_inlet_val, self._p_outlet_val], self.beta_nitsche)

    def setup(self, bcu: list[BoundaryCondition], bcp: list[BoundaryCondition], facet_tags=None, tags=None) -> None:
        if tags is None or tags.get("inlet") is None or tags.get("outlet") is None:
            raise KeyError("inlet/outlet")  # the reference indexes tags["inlet"], tags["outlet"] (:180-191)
        self._pb_markers = [int(tags["inlet"]), int(tags["outlet"])]
        self._ds_terms = False
        self.ctx.set_boundary_terms(ds_terms=False)
        super().setup(bcu, [], facet_tags, tags)  # self.bcp_d = [] (:221)
        self._apply_pressures()
