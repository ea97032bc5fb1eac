"""Drop-in `Solver` for the reference's `--solver stabilized_pcd_pressurebc`
(/root/reference/src/solvers/stabilized_pcd_pressurebc.py): the pressure-driven rotational form of `stabilized_schur_pressurebc`
(natural pressures on `tags["inlet"]` / `tags["outlet"]`, Nitsche tangential condition, `bcp` ignored, midpoint scheme) solved with
the settings of `stabilized_pcd`: Newton with Eisenstat-Walker forcing and FGMRES preconditioned by the pressure
convection-diffusion Schur approximation (`pc_type 2`, include/cfdh.h: cfdh_set_schur_pcd) on the generic element kernels.

Constructor as in the reference (:49-69): `p_inlet` and `p_outlet` are required (ValueError otherwise), half of each enters the
form, `beta_nitsche` defaults to 100; there is no `p_grade` (degree 1 is fixed, :73-76): the value 1 is tolerated, anything else
raises NotImplementedError.  Caps as in `stabilized_pcd`: snes_rtol 1e-4, snes_max_it 50, ksp_max_it 10000, restart 150, no
null-space handling.  Runs on one GPU on triangles (P1 through the generic kernels), quadrilaterals and hexahedra (Q1); tetrahedra
(the rotational form has no P1 tetrahedron variant) and a partitioned `comm` are refused before any device work.  DESIGN.md
section 9 records what differs from the reference's configuration (the wind of K is the library's theta-weighted velocity).
"""
from __future__ import annotations

from typing import Callable

import numpy as np

from .. import _lib
from ..boundaryCondition import BoundaryCondition
from .stabilized_pcd import TIME_TERM
from .stabilized_schur_pressurebc import Solver as _PressureSolver


def _refuse_unsupported(mesh, p_grade, kwargs):
    if int(p_grade) != 1:
        raise NotImplementedError("p_grade=%r: stabilized_pcd_pressurebc is a degree-1 solver (P1/P1, Q1/Q1)" % (p_grade,))
    if mesh.topology.cell_name() == "tetrahedron":
        raise NotImplementedError("stabilized_pcd_pressurebc has no tetrahedron variant (the rotational form needs P2 there, the PCD "
                                  "operator degree 1): use hexahedra (Q1/Q1)")
    comm = kwargs.get("comm", None)
    if comm is not None and comm.size > 1:
        raise NotImplementedError("stabilized_pcd_pressurebc runs on one GPU: partitioned runs are not supported")


class Solver(_PressureSolver):
    MAX_ITER = 20

    def __init__(self, mesh, dt: float, rho: float, mu: float, f: list,
                 initial_velocity: Callable[[np.ndarray], np.ndarray] = None,
                 p_inlet: float = None, p_outlet: float = None, beta_nitsche: float = 100.0, **kwargs):
        if p_inlet is None or p_outlet is None:
            raise ValueError(
                "p_inlet and p_outlet are required for stabilized_pcd_pressurebc. "
                "Pass them via CLI: --p_inlet <value> --p_outlet <value>"
            )
        _refuse_unsupported(mesh, kwargs.pop("p_grade", 1), kwargs)
        user_options = dict(kwargs.pop("options", {}))
        self._init_pressure_driven(mesh, dt, rho, mu, f, initial_velocity, float(p_inlet), float(p_outlet), beta_nitsche, 1, kwargs)
        o = self.options
        o.snes_rtol, o.snes_max_it = 1.0e-4, 50          # stabilized_pcd.py:247-248
        o.ksp_max_it, o.ksp_restart = 10000, 150         # :252-254
        o.remove_p_mean = 0
        o.pc_type = _lib.PC_PCD
        if "newton_rtol" in kwargs:
            o.snes_rtol = float(kwargs["newton_rtol"])
        for k, v in user_options.items():
            setattr(o, k, v)
        self.ctx.set_options(o)
        self.ctx.set_ksp_forcing(2)                       # snes_ksp_ew, PETSc's defaults

    def _banner(self):
        return f"[Solver] PCD, beta_nitsche={self.beta_nitsche}"

    def setup(self, bcu: list[BoundaryCondition], bcp: list[BoundaryCondition], facet_tags=None, tags=None) -> None:
        if tags is None or tags.get("inlet") is None or tags.get("outlet") is None:
            raise KeyError("inlet/outlet")
        self.ctx.set_schur_pcd(int(tags["inlet"]), int(tags["outlet"]), TIME_TERM)
        super().setup(bcu, bcp, facet_tags, tags)
