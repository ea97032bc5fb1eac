"""Drop-in `Solver` for the reference's `--solver stabilized_pcd` (/root/reference/src/solvers/stabilized_pcd.py): the form of
`stabilized_schur` with fully implicit spatial terms (u_sol wherever stabilized_schur.py has u_mid, :67-121 -- the same ds pair,
SUPG, PSPG and LSIC), Newton with Eisenstat-Walker forcing (`snes_ksp_ew`, :249) and FGMRES right-preconditioned by the block
upper-triangular Schur factorisation with a pressure convection-diffusion (PCD) Schur approximation (PCDPC_vY, :204-276).

Here: `cfdh_set_time_scheme(1, 1, -1, 0)` with the ds pair and no null-space handling (the reference has none, :311-316), the
reference's caps (snes_rtol 1e-4, snes_max_it 50, ksp_max_it 10000, ksp_restart 150, :247-254), EW version 2 with PETSc's defaults
and `pc_type 2` (include/cfdh.h: cfdh_set_schur_pcd; DESIGN.md section 9 lists what differs from the reference's configuration).
`setup` needs `tags["inlet"]` (Robin term of K) and `tags["outlet"]` (Dirichlet rows of A_p) and raises KeyError without them, as
the reference's `tags[...]` indexing does.  P1 triangles and P1 tetrahedra on one GPU: quadrilateral / hexahedral meshes and a
partitioned `comm` are refused before any device work (stabilized_schur runs those).
"""
from __future__ import annotations

from typing import Callable

import numpy as np

from .. import _lib
from ..boundaryCondition import BoundaryCondition
from .stabilized_schur import Solver as _SchurSolver

# K carries the time term rho a0 / (theta dt) M (1) or not (0, the reference's literal operator): the measured choice, DESIGN.md
# section 9 (fewer FGMRES iterations on the stenosis workloads)
TIME_TERM = 1


def _refuse_unsupported(mesh, kwargs):
    cell = mesh.topology.cell_name()
    if cell in ("quadrilateral", "hexahedron"):
        raise NotImplementedError("stabilized_pcd runs on P1 triangles and tetrahedra; on %s meshes use stabilized_schur" % cell)
    comm = kwargs.get("comm", None)
    if comm is not None and comm.size > 1:
        raise NotImplementedError("stabilized_pcd runs on one GPU: for a partitioned run use stabilized_schur")


class Solver(_SchurSolver):
    MAX_ITER = 20

    def __init__(self, mesh, dt: float, rho: float, mu: float, f: list,
                 initial_velocity: Callable[[np.ndarray], np.ndarray] = None, **kwargs):
        _refuse_unsupported(mesh, kwargs)
        kwargs.pop("_degree", None)
        kwargs.pop("generic_kernels", None)
        user_options = dict(kwargs.pop("options", {}))
        super().__init__(mesh, dt, rho, mu, f, initial_velocity, **kwargs)
        self.ctx.set_time_scheme(1.0, 1.0, -1.0, 0.0)   # u_sol in every spatial term, (u - u_prev) / dt
        o = self.options
        o.snes_rtol, o.snes_max_it = 1.0e-4, 50          # :247-248
        o.ksp_max_it, o.ksp_restart = 10000, 150         # :252-254
        o.remove_p_mean = 0                               # no null-space handling (:311-316)
        o.pc_type = _lib.PC_PCD
        if "newton_rtol" in kwargs:
            o.snes_rtol = float(kwargs["newton_rtol"])
        for k, v in user_options.items():
            setattr(o, k, v)
        self.ctx.set_options(o)
        self.ctx.set_ksp_forcing(2)                       # snes_ksp_ew (:249), PETSc's defaults

    def setup(self, bcu: list[BoundaryCondition], bcp: list[BoundaryCondition], facet_tags=None, tags=None) -> None:
        if tags is None:
            raise KeyError("inlet")
        inlet, outlet = tags["inlet"], tags["outlet"]    # :205-210 index both
        if inlet is None or outlet is None:
            raise KeyError("inlet" if inlet is None else "outlet")
        self.ctx.set_schur_pcd(int(inlet), int(outlet), TIME_TERM)
        super().setup(bcu, bcp, facet_tags, tags)
