"""Drop-in `Solver` for the reference's `--solver ipcs_bdf2` (/root/reference/src/solvers/ipcs_bdf2.py:33-172): the incremental
pressure-correction scheme on P2 velocity / P1 pressure (Taylor-Hood) triangles and tetrahedra -- linear, no stabilisation terms,
no Schur complement; a step is a convection-diffusion solve for the tentative velocity u*, a Poisson solve for the pressure
correction phi and a mass solve for the velocity, all on the device (include/cfdh.h: cfdh_create_ipcs, cfdh_ipcs_step).

Same constructor, `setup(bcu, bcp, facet_tags=None, tags=None)`, `solveStep()` and state Functions as the reference, plus `u_star`,
`u_n1`, `phi`; `initial_velocity` goes into `u_prev` AND `u_n1` (:61-63).  A failed solve raises RuntimeError("Did not converge,
reason: r.") like the other plugins.  What differs from the reference's configuration:

* `consistent=True` (default) solves the momentum equation rho u_t + rho (w . grad) u - mu lap u + grad p = rho f; the
  reference's literal form has no rho on the convection term and the force with the opposite sign (`consistent=False`), which is
  invisible for rho = 1, f = 0 and wrong otherwise;
* linear solvers: BiCGStab + Jacobi, flexible PCG + one smoothed-aggregation V-cycle (reference: MINRES + BoomerAMG), CG + Jacobi
  (reference: CG + SOR); every solve stops on the true residual at `rtol` (default 1e-5, PETSc's), `atol`, `max_it`;
* a pressure Dirichlet VALUE goes into phi as in the reference (right for homogeneous data only): one warning when it is non-zero.

`assemble_wss()` computes the wall shear stress of the P2 velocity on the device as a P1 field on the vertices (`shear_stress`, filled
when it is read); `wall_stats_reset / wall_stats_accumulate / wall_indices` give the cycle-averaged indices (TAWSS, OSI, RRT).

Keyword arguments: `consistent`, `rtol` (one value or three), `atol`, `max_it`, `device`, `verbose`, `quiet`, `options` (AMG fields
of cfdh_options).  Quadrilateral / hexahedral meshes and a partitioned `comm` are refused before any device work.
"""
from __future__ import annotations

import warnings
from typing import Callable

import numpy as np

from .. import _lib
from ..boundaryCondition import BoundaryCondition
from ..fem import Function, FunctionSpace
from ..solverBase import SolverBase
from .stabilized_schur import Solver as _SchurSolver


def _refuse_unsupported(mesh, kwargs, name="ipcs_bdf2"):
    cell = mesh.topology.cell_name()
    if cell in ("quadrilateral", "hexahedron"):
        raise NotImplementedError("%s runs on P2/P1 triangles and tetrahedra; on %s meshes use stabilized_schur" % (name, cell))
    comm = kwargs.get("comm", None)
    if comm is not None and comm.size > 1:
        raise NotImplementedError("%s runs on one GPU: for a partitioned run use stabilized_schur" % name)


class Solver(SolverBase):
    _name = "ipcs_bdf2"   # in messages; solvers/ipcs_midpoint.py runs the other scheme on the same context

    def __init__(self, mesh, dt: float, rho: float, mu: float, f: list,
                 initial_velocity: Callable[[np.ndarray], np.ndarray] = None, **kwargs):
        _refuse_unsupported(mesh, kwargs, self._name)
        super().__init__(mesh, dt, rho, mu, f)
        gdim = mesh.geometry.dim
        super().initVelocitySpace("Lagrange", mesh.topology.cell_name(), 2, shape=(gdim,))
        super().initPressureSpace("Lagrange", mesh.topology.cell_name(), 1)
        self.u_star = Function(self.V, name="u_star")
        self.u_n1 = Function(self.V, name="u_n1")
        self.phi = Function(self.Q, name="phi")
        if initial_velocity:
            self.u_prev.interpolate(initial_velocity)
            self.u_n1.interpolate(initial_velocity)
        self._verbose = int(kwargs.get("verbose", 0))
        self._quiet = bool(kwargs.get("quiet", False))
        self._part = None
        self._comm = kwargs.get("comm", None)
        self.consistent = bool(kwargs.get("consistent", True))
        dm = self._dm
        self.ctx = _lib.IpcsContext(dm.x, dm.cells, mesh.num_vertices, dm.facet_cells, dm.facet_local, dm.facet_marker,
                                    device=int(kwargs.get("device", 0)))
        ff = np.atleast_1d(np.asarray(f, dtype=np.float64))
        self.ctx.set_params(float(dt), float(rho), float(mu), f=ff)
        self._configure_scheme(float(rho))
        self.ctx.set_tolerances(kwargs.get("rtol", 1e-5), kwargs.get("atol", 1e-50), kwargs.get("max_it", 10000))
        if kwargs.get("options"):
            o = self.ctx.default_options()
            for k, v in dict(kwargs["options"]).items():
                setattr(o, k, v)
            self.ctx.set_options(o)
        self.last_stats = None
        self._bcs = []
        self._bc_cache = self._bc_nodes = self._bc_owned = None
        self._warned_p = False
        # lazy host/device synchronisation of the state Functions
        self._sol_dev_newer = False      # u_sol, p_sol
        self._wss_dev_newer = False      # shear_stress
        self._mid_dev_newer = False      # u_star, phi
        self._prev_dev_newer = False     # u_prev, p_prev, u_n1
        self._prev_host_dirty = True
        self.transfers = {"downloads": 0, "uploads": 0}
        for fn in (self._u_sol, self._p_sol):
            fn.x._pre_access = self._sync_solution
        for fn in (self.u_star, self.phi):
            fn.x._pre_access = self._sync_intermediate
        for fn in (self._u_prev, self._p_prev, self.u_n1):
            fn.x._pre_access = self._sync_previous
            fn.x._post_access = self._mark_prev_dirty
        self._u_prev.x._assign_hook = lambda src: self._assign_previous(0, src)
        self._p_prev.x._assign_hook = lambda src: self._assign_previous(1, src)

    def _configure_scheme(self, rho):
        if not self.consistent:
            self.ctx.set_form(1.0, -1.0)   # ipcs_bdf2.py:67-80: no rho on the convection term, + f . v in the residual

    _bc_nodes_values = _SchurSolver._bc_nodes_values
    _upload_bcs = _SchurSolver._upload_bcs
    _wall_stats_one_gpu = _SchurSolver._wall_stats_one_gpu
    wall_stats_reset = _SchurSolver.wall_stats_reset
    wall_stats_accumulate = _SchurSolver.wall_stats_accumulate
    wall_indices = _SchurSolver.wall_indices

    # -- lazy sync ---------------------------------------------------------------
    def _sync_solution(self):
        if self._sol_dev_newer:
            self._sol_dev_newer = False
            self.transfers["downloads"] += 1
            self.ctx.get_solution(self._u_sol.x._array, self._p_sol.x._array)

    def _sync_intermediate(self):
        if self._mid_dev_newer:
            self._mid_dev_newer = False
            self.transfers["downloads"] += 1
            self.u_star.x._array[:] = self.ctx.get_intermediate(0)
            self.phi.x._array[:] = self.ctx.get_intermediate(1)

    def _sync_previous(self):
        if self._prev_dev_newer:
            self._prev_dev_newer = False
            self.transfers["downloads"] += 1
            self.ctx.get_previous(self._u_prev.x._array, self._p_prev.x._array)
            self.u_n1.x._array[:] = self.ctx.get_previous2()

    def _mark_prev_dirty(self):
        self._prev_host_dirty = True

    def _upload_previous(self):
        if self._prev_host_dirty and not self._prev_dev_newer:
            self.transfers["uploads"] += 1
            self.ctx.set_state(u_prev=self._u_prev.x._array, p_prev=self._p_prev.x._array)
            self.ctx.set_previous2(self.u_n1.x._array)
        self._prev_host_dirty = False

    def _assign_previous(self, field, src):
        if src is not (self._u_sol.x if field == 0 else self._p_sol.x) or not self._sol_dev_newer:
            return False
        self._upload_previous()
        self.ctx.advance_field(field)
        self._prev_dev_newer = True
        return True

    # -- reference API -------------------------------------------------------------
    def setup(self, bcu: list[BoundaryCondition], bcp: list[BoundaryCondition], facet_tags=None, tags=None) -> None:
        self.bcu_d = [bc.getBC(self.V) for bc in bcu]
        self.bcp_d = [bc.getBC(self.Q) for bc in bcp]
        self._bcs = [(0, bc) for bc in self.bcu_d] + [(1, bc) for bc in self.bcp_d]
        self._bc_cache = self._bc_nodes = self._bc_owned = None
        if facet_tags is not None:
            mk = np.zeros(self.mesh.num_facets, dtype=np.int32)
            mk[np.asarray(facet_tags.indices, dtype=np.int64)] = np.asarray(facet_tags.values, dtype=np.int32)
            self.ctx.set_facet_markers(mk)
        self._upload_bcs()
        self._check_pressure_values()
        self._sync_previous()
        self._sync_solution()
        self.ctx.set_state(u_prev=self._u_prev.x._array, p_prev=self._p_prev.x._array, u=self._u_sol.x._array, p=self._p_sol.x._array)
        self.ctx.set_previous2(self.u_n1.x._array)
        self._prev_host_dirty = False

    def _check_pressure_values(self):
        if self._warned_p:
            return
        for bc in getattr(self, "bcp_d", []):
            if np.any(bc.g.x._array[bc.dofs] != 0.0):
                self._warned_p = True
                warnings.warn("ipcs_bdf2: a pressure Dirichlet value is non-zero; as in the reference it is imposed on the pressure "
                              "CORRECTION phi of every step, which is only right for homogeneous data", RuntimeWarning, stacklevel=3)
                return

    def solveStep(self):
        for _, bc in self._bcs:
            bc.update()  # ipcs_bdf2.py:128-129
        self._upload_bcs()
        self._check_pressure_values()
        self._upload_previous()
        st = self.ctx.step()  # raises RuntimeError("Did not converge, reason: r.")
        self.last_stats = st
        self._sol_dev_newer = self._mid_dev_newer = True
        self._prev_dev_newer = True   # u_n1 <- u_prev happened on the device
        if self._verbose and not self._quiet:
            print("%s: iterations %s, |r|/|b| %s" % (self._name, list(st.its), ["%.2e" % r for r in st.rel_res]))

    def initStressForm(self):
        """The stress fields live on the vertex (degree-1) space whatever the velocity degree (solverBase.py:144-162: `vector` is
        CG1); the base class would put them on the P2 node mesh of V."""
        self.normal_stress = Function(FunctionSpace(self.mesh, 1), name="normal_stress")
        self.shear_stress = Function(FunctionSpace(self.mesh, self.mesh.geometry.dim), name="shear_stress")

    def _sync_wss(self):
        if self._wss_dev_newer:
            self._wss_dev_newer = False
            self.shear_stress.x._array[:] = self.ctx.wall_shear_stress(download=True)

    def assemble_wss(self):
        """solverBase.py:185-195 for the P2 u_sol on the device (cfdh_wall_shear_stress); the host array behind `shear_stress.x.array`
        is filled when it is read."""
        if not hasattr(self, "shear_stress"):
            return
        self.shear_stress.x._pre_access = self._sync_wss
        self.ctx.wall_shear_stress(download=False)
        self._wss_dev_newer = True

    # -- device-resident extras ------------------------------------------------------
    def advance(self):
        """u_prev <- u_sol, p_prev <- p_sol without leaving HBM (the copy of /root/reference/src/scenario.py:306-307)."""
        self._upload_previous()
        self.ctx.advance()
        self._prev_dev_newer = True
        self._prev_host_dirty = False

    def functional(self, kind, marker=0):
        return self.ctx.functional(kind, marker)
