"""`SolverBase` with the reference's plugin surface
(/root/reference/src/solverBase.py:25-195): Constants dt/rho/mu/f, spaces V/Q,
state Functions u_sol/p_sol/u_prev/p_prev/u_residual/p_residual, the stress
helpers and `assemble_wss`."""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Callable

import numpy as np

from .boundaryCondition import BoundaryCondition
from .fem import Constant, Function, FunctionSpace


class SolverBase(ABC):
    @abstractmethod
    def __init__(self, mesh, dt: float, rho: float, mu: float, f: list,
                 initial_velocity: Callable[[np.ndarray], np.ndarray] = None):
        self.mesh = mesh
        self.dt = Constant(mesh, dt)
        self.rho = Constant(mesh, rho)
        self.mu = Constant(mesh, mu)
        self.f = Constant(mesh, f)
        self._u_sol = self._p_sol = self._u_prev = self._p_prev = None
        self._V = self._Q = None

    def _need(self, attr: str, initialiser: str):
        value = getattr(self, attr)
        if value is None:
            raise AssertionError(f"{type(self).__name__}.{attr.lstrip('_')} does not exist before {initialiser}() was called")
        return value

    u_sol = property(lambda self: self._need("_u_sol", "initVelocitySpace"))
    u_prev = property(lambda self: self._need("_u_prev", "initVelocitySpace"))
    V = property(lambda self: self._need("_V", "initVelocitySpace"))
    p_sol = property(lambda self: self._need("_p_sol", "initPressureSpace"))
    p_prev = property(lambda self: self._need("_p_prev", "initPressureSpace"))
    Q = property(lambda self: self._need("_Q", "initPressureSpace"))

    @abstractmethod
    def setup(self, bcu: list[BoundaryCondition], bcp: list[BoundaryCondition]) -> None:
        pass

    @abstractmethod
    def solveStep(self) -> None:
        pass

    def _dof_mesh(self, degree):
        """The node set of Lagrange elements of `degree` on the mesh: the mesh itself for P1 / Q1, vertices + edge midpoints
        for P2 triangles (`p_grade = 2`, stabilized_schur_backflow.py:84-87)."""
        from .elements import dof_mesh
        dm = dof_mesh(self.mesh, degree)
        if getattr(self, "_dm", None) not in (None, dm):
            # the one mixed pair: P2 velocity with P1 pressure on simplices (Taylor-Hood, ipcs_bdf2.py:45-48).  Q lives on the base
            # mesh, whose vertices are the first nodes of V's node mesh (elements.NodeMesh / NodeMesh3D)
            if getattr(self._dm, "base", None) is self.mesh and dm is self.mesh and self._V is not None and self._Q is None:
                return dm
            raise ValueError("velocity and pressure must use the same Lagrange degree (equal-order elements), or degree 2 / 1 on simplices")
        self._dm = dm
        return dm

    def initVelocitySpace(self, family, cell, degree, shape=None) -> None:
        if str(family) not in ("Lagrange", "CG", "P"):
            raise ValueError("only Lagrange spaces are implemented")
        dm = self._dof_mesh(degree)
        self._V = FunctionSpace(dm, self.mesh.geometry.dim if shape is None else int(shape[0]))
        self._u_sol = Function(self.V, name="velocity")
        self._u_prev = Function(self.V)
        self.u_residual = Function(self.V, name="u_residual")

    def initPressureSpace(self, family, cell, degree, shape=None) -> None:
        if str(family) not in ("Lagrange", "CG", "P"):
            raise ValueError("only Lagrange spaces are implemented")
        self._Q = FunctionSpace(self._dof_mesh(degree), 1)
        self._p_sol = Function(self.Q, name="pressure")
        self._p_prev = Function(self.Q)
        self.p_residual = Function(self.Q, name="p_residual")

    def initStressForm(self):
        """Allocates the stress fields the Scenario writes
        (/root/reference/src/solverBase.py:144-173)."""
        dm = getattr(self, "_dm", None) or self.mesh
        self.normal_stress = Function(FunctionSpace(dm, 1), name="normal_stress")
        self.shear_stress = Function(FunctionSpace(dm, self.mesh.geometry.dim), name="shear_stress")

    def assemble_wss(self):
        """Wall shear stress  (1/|e|) oint w . (T - (T.n) n),  T = -sigma(u,p) n
        (/root/reference/src/solverBase.py:163-195), assembled on the host from
        the current solution.  Post-processing, outside the timed hot path."""
        if not hasattr(self, "shear_stress"):
            return
        mesh = self.mesh
        if mesh.geometry.dim != 2 or getattr(getattr(self, "_dm", mesh), "etype", 0) != 0:
            raise NotImplementedError("host restatement of the wall shear stress: P1 triangles only (the device path covers the other elements)")
        u = self.u_sol.x.array.reshape(-1, 2)
        mu = float(self.mu.value)
        fc, fl, fv = mesh.facet_cells, mesh.facet_local, mesh.facet_vertices
        cells = mesh.cells[fc]
        X = mesh.x[cells]
        det = (X[:, 1, 0] - X[:, 0, 0]) * (X[:, 2, 1] - X[:, 0, 1]) - (X[:, 1, 1] - X[:, 0, 1]) * (X[:, 2, 0] - X[:, 0, 0])
        g = np.empty((len(fc), 3, 2))
        g[:, 0, 0] = (X[:, 1, 1] - X[:, 2, 1]) / det
        g[:, 0, 1] = (X[:, 2, 0] - X[:, 1, 0]) / det
        g[:, 1, 0] = (X[:, 2, 1] - X[:, 0, 1]) / det
        g[:, 1, 1] = (X[:, 0, 0] - X[:, 2, 0]) / det
        g[:, 2, 0] = (X[:, 0, 1] - X[:, 1, 1]) / det
        g[:, 2, 1] = (X[:, 1, 0] - X[:, 0, 0]) / det
        idx = np.arange(len(fc))
        gf = g[idx, fl]
        n = -gf / np.linalg.norm(gf, axis=1)[:, None]
        G = np.einsum("cai,caj->cij", g, u[cells])  # d_i u_j
        E = 0.5 * (G + np.transpose(G, (0, 2, 1)))
        # tangential part of T = -(2 mu E - p I) n : the pressure part is purely normal
        T = -2.0 * mu * np.einsum("cij,cj->ci", E, n)
        Tt = T - np.einsum("ci,ci->c", T, n)[:, None] * n
        out = self.shear_stress.x.array.reshape(-1, 2)
        out[:] = 0.0
        # (1/|e|) oint lambda_a Tt = Tt / 2 per facet vertex
        np.add.at(out, fv[:, 0], 0.5 * Tt)
        np.add.at(out, fv[:, 1], 0.5 * Tt)

    # -- passive scalar transport on the device (cfdh_scalar_*: blood age, contrast bolus) -----------------------------------
    def _transport_ctx(self, what="transport", noun="passive scalar"):
        """The context, when the scalar (or the particle tracker) exists on it: closed-form P1 kernels, whole mesh on one GPU.
        Raises before any device work otherwise."""
        from . import _lib
        ctx = getattr(self, "ctx", None)
        comm = getattr(self, "_comm", None)
        why = None
        if ctx is None:
            why = "the solver holds no device context"
        elif isinstance(ctx, _lib.IpcsContext):
            why = "the pressure-correction (IPCS) solvers have no " + noun
        elif int(getattr(ctx, "etype", 0)) != 0:
            why = "the " + noun + " runs on the closed-form P1 kernels, not on the generic-element (P2 / Q1) contexts"
        elif getattr(self, "_part", None) is not None or (comm is not None and comm.size > 1):
            why = "the " + noun + " runs on one GPU, not on a part of a partitioned run"
        if why:
            raise NotImplementedError(what + ": " + why)
        return ctx

    def transport_enable(self, D=0.0, s=0.0, theta_c=0.5, nodes=None, values=None, rtol=None):
        """Switch on dc/dt + w . grad c - D lap c = s on the vertices (c = 0 at first use; a later call keeps c).  `nodes` /
        `values`: the Dirichlet set (None keeps it)."""
        ctx = self._transport_ctx()
        ctx.scalar_enable(D, s, theta_c)
        if rtol is not None:
            ctx.scalar_set_tolerances(rtol=float(rtol))
        if nodes is not None:
            ctx.scalar_set_dirichlet(nodes, 0.0 if values is None else values)

    def transport_set_dirichlet(self, nodes, values):
        """Replace the Dirichlet set of the scalar (empty: none)."""
        self._transport_ctx().scalar_set_dirichlet(nodes, values)

    def transport_functional(self, kind, marker=0):
        """0: int c dx, 1: int c (u_sol . n) ds over the facets of `marker`, 2 / 3: min / max."""
        return self._transport_ctx().scalar_functional(kind, marker)

    def transport_step(self):
        """One step with the velocity of the flow step just solved: call after solveStep() and before advance() / the copy of
        u_sol into u_prev."""
        self.last_transport_stats = self._transport_ctx().scalar_step()
        return self.last_transport_stats

    def transport_field(self, c=None):
        """The scalar on the vertices [nv]; with an argument: sets it."""
        return self._transport_ctx().scalar_state(c)

    # -- Lagrangian particle tracking on the device (cfdh_particles_*: pathlines, residence times, shear exposure) -----------
    def _particles_ctx(self):
        return self._transport_ctx("particles", "particle tracker")

    def particles_enable(self, capacity, nsub=2):
        """Room for `capacity` massless particles, `nsub` explicit-midpoint substeps per flow step (a later call changes nsub only)."""
        self._particles_ctx().particles_enable(capacity, nsub)

    def particles_seed(self, x, cells, t_birth=0.0):
        """Append particles at x [n, gdim] in the mesh cells `cells` [n] (particles.py has helpers that produce both)."""
        self._particles_ctx().particles_seed(x, cells, t_birth)

    def particles_step(self, t0):
        """Move the particles over [t0, t0 + dt] with the velocity of the flow step just solved: call after solveStep() and before
        advance() / the copy of u_sol into u_prev."""
        self.last_particle_stats = self._particles_ctx().particles_step(t0)
        return self.last_particle_stats

    def particles_get(self, which=None):
        """One field (a _lib.PARTICLE_* code), or with no argument the dict x, cell, status, age, path, exposure, t_end."""
        ctx = self._particles_ctx()
        if which is not None:
            return ctx.particles_get(which)
        names = ("x", "cell", "status", "age", "path", "exposure", "t_end")  # the order of _lib.PARTICLE_X .. PARTICLE_T_END
        return {k: ctx.particles_get(w) for w, k in enumerate(names)}

    # -- volumetric flow diagnostics on the device (cfdh_flow_*: vorticity, Q, shear rate, dissipation, helicity, energy) ------
    def _flow_ctx(self):
        return self._transport_ctx("flow diagnostics", "flow diagnostics kernel")

    def flow_field(self, name):
        """One vertex field of the current u_sol, recovered from the cell gradients: "gradient" [nv, d, d], "vorticity" [nv] in 2-D
        and [nv, 3] in 3-D, "q_criterion", "shear_rate", "dissipation", and in 3-D "helicity" and "lnh" [nv] (or a _lib.FLOW_* code)."""
        from . import _lib
        ctx = self._flow_ctx()
        if isinstance(name, str):
            if name not in _lib.FLOW_FIELDS:
                raise ValueError("flow_field: unknown field %r (one of %s)" % (name, ", ".join(_lib.FLOW_FIELDS)))
            name = _lib.FLOW_FIELDS[name]
        return ctx.flow_field(name)

    def flow_integrals(self):
        """[8]: volume, kinetic energy, enstrophy, viscous dissipation, helicity, int div u, int Q, int (div u)^2 of the current u_sol
        (_lib.FLOW_INT_*)."""
        return self._flow_ctx().flow_integrals()

    def flow_stats_reset(self):
        """Zero the window averages of the flow field (allocated on first use)."""
        self._flow_ctx().flow_stats_reset()

    def flow_stats_accumulate(self, w):
        """Add the current u_sol, its shear rate and dissipation to the window averages with weight w (the step's dt)."""
        self._flow_ctx().flow_stats_accumulate(w)

    def flow_stats(self):
        """The window averages: mean_velocity [nv, d], fluctuation (k'), mean_dissipation, mean_shear_rate, peak_shear_rate [nv],
        with W (the sum of the weights) and steps."""
        from . import _lib
        ctx = self._flow_ctx()
        W, count = ctx.flow_stats_get(_lib.FLOW_TOTALS)
        names = ("mean_velocity", "fluctuation", "mean_dissipation", "mean_shear_rate", "peak_shear_rate")  # _lib.FLOW_MEAN_U ..
        out = {k: ctx.flow_stats_get(w) for w, k in enumerate(names)}
        out["W"], out["steps"] = float(W), int(count)
        return out

    # -- point sampler on the device (cfdh_sample_*: probe points, lines, voxel grids) ------------------------------------------
    def _sample_ctx(self):
        return self._transport_ctx("sampling", "point sampler")

    def sample_set_points(self, x, tol=1e-9):
        """The sample set: explicit points [n, gdim], located once on the device (an empty array removes the set)."""
        self._sample_ctx().sample_set_points(x, tol)

    def sample_set_grid(self, origin, spacing, dims, tol=1e-9):
        """The sample set: the nodes origin + (i, j, k) * spacing of a regular grid, in the point order of VTK ImageData."""
        self._sample_ctx().sample_set_grid(origin, spacing, dims, tol)

    def sample_location(self):
        """(cell, lambda, x) of the set: the lowest-indexed cell that holds each point (-1: none), its barycentric coordinates and
        the coordinates the device used."""
        return self._sample_ctx().sample_location()

    def sample_now(self):
        """(u [n, gdim], p [n]) of the current u_sol at the points of the set; zeros at unlocated points."""
        rows = self._sample_ctx().sample_now()
        return rows[:, :-1], rows[:, -1]

    def sample_record(self, t, rows=None):
        """Append the current state to the series on the device (no copy, no synchronisation); `rows` (first call, or to resize)
        is the capacity in records."""
        ctx = self._sample_ctx()
        if rows is not None:
            ctx.sample_series_enable(rows)
        ctx.sample_record(t)

    def sample_series(self):
        """(t [rows], u [rows, n, gdim], p [rows, n]) recorded since the last call; empties the device buffer."""
        t, rows = self._sample_ctx().sample_series_get()
        return t, rows[:, :, :-1], rows[:, :, -1]

    def sample_mean_reset(self):
        """Zero the per-point means (allocated on first use)."""
        self._sample_ctx().sample_mean_reset()

    def sample_mean_accumulate(self, w):
        """Add the current state at the points of the set to the means with weight w (the step's dt)."""
        self._sample_ctx().sample_mean_accumulate(w)

    def sample_mean(self):
        """The means: mean_velocity [n, gdim], mean_pressure, fluctuation (k') [n], with W (the sum of the weights) and steps."""
        from . import _lib
        ctx = self._sample_ctx()
        W, count = ctx.sample_mean_get(_lib.SAMPLE_TOTALS)
        names = ("mean_velocity", "mean_pressure", "fluctuation")  # _lib.SAMPLE_MEAN_U ..
        out = {k: ctx.sample_mean_get(w) for w, k in enumerate(names)}
        out["W"], out["steps"] = float(W), int(count)
        return out

    # -- cut-plane sections on the device (cfdh_section_*: flow rate, mean pressure, energy flux through planes) -----------------
    def _section_ctx(self):
        return self._transport_ctx("sections", "section kernel")

    def section_set(self, planes):
        """The sections: a list of sections.plane(...) / sections.stations(...) entries, or (origin [K, gdim], normal [K, gdim],
        radius [K] or None).  The cut is built once; an empty list removes the set."""
        from . import sections
        ctx = self._section_ctx()
        origin, normal, radius = sections.as_arrays(planes)
        ctx.section_set(origin, normal, radius)

    def section_cut(self):
        """(ptr [K + 1], cell [entries], measure [entries], straddling [K]): per section the cut and taken cells in ascending index,
        the measure of their polygons and the number of polygons that straddle the clip ball."""
        return self._section_ctx().section_get_cut()

    def section_now(self):
        """[K, 10]: area, flow rate, int p, int (u.n)^2, int |u|^2, int p u.n, int rho/2 |u|^2 u.n, int u_i of the current u_sol."""
        return self._section_ctx().section_now()

    def section_record(self, t, rows=None):
        """Append the rows of the current state to the series on the device (no copy, no synchronisation); `rows` (first call, or
        to resize) is the capacity in records."""
        ctx = self._section_ctx()
        if rows is not None:
            ctx.section_series_enable(rows)
        ctx.section_record(t)

    def section_series(self):
        """(t [rows], rows [rows, K, 10]) recorded since the last call; empties the device buffer."""
        return self._section_ctx().section_series_get()

    def section_mean_reset(self):
        """Zero the window means of the rows (allocated on first use)."""
        self._section_ctx().section_mean_reset()

    def section_mean_accumulate(self, w):
        """Add the rows of the current state to the window means with weight w (the step's dt)."""
        self._section_ctx().section_mean_accumulate(w)

    def section_mean(self):
        """dict: rows [K, 10] (sum w row / W; None while nothing is accumulated), W and steps."""
        rows, W, count = self._section_ctx().section_mean_get()
        return {"rows": rows, "W": W, "steps": count}

    @staticmethod
    def _simplex_gradients(mesh):
        """grad(lambda_a) of every cell of a P1 simplex mesh, [nc, d + 1, d]."""
        X = np.asarray(mesh.x)[np.asarray(mesh.cells)]
        d = X.shape[2]
        if X.shape[1] != d + 1:
            raise NotImplementedError("epsilon / sigma: cell-wise values exist for P1 simplices (constant gradients) only")
        M = X[:, 1:, :] - X[:, :1, :]                     # rows x_a - x_0
        Minv = np.linalg.inv(M)                           # columns = grad(lambda_a), a >= 1
        g = np.empty((len(X), d + 1, d))
        g[:, 1:, :] = np.transpose(Minv, (0, 2, 1))
        g[:, 0, :] = -g[:, 1:, :].sum(axis=1)
        return g

    @staticmethod
    def epsilon(u):
        """`sym(nabla_grad(u))` of solverBase.py:176-178, evaluated: the reference returns the UFL expression, this mirror has no
        form language, so it returns what the expression IS on a P1 field -- one symmetric d x d matrix per cell, [nc, d, d]
        (`nabla_grad(u)[i, j] = d_i u_j`)."""
        mesh = u.function_space.mesh
        g = SolverBase._simplex_gradients(mesh)
        uv = np.asarray(u.x.array, dtype=float).reshape(-1, u.function_space.bs)[np.asarray(mesh.cells)]
        G = np.einsum("cai,caj->cij", g, uv)
        return 0.5 * (G + np.transpose(G, (0, 2, 1)))

    @staticmethod
    def sigma(u, p, mu):
        """`2 mu sym(nabla_grad(u)) - p I` of solverBase.py:180-182 per cell, [nc, d, d]; p enters with its cell mean (the value of
        a P1 field at the centroid)."""
        E = SolverBase.epsilon(u)
        mesh = u.function_space.mesh
        pc = np.asarray(p.x.array, dtype=float)[np.asarray(mesh.cells)].mean(axis=1)
        d = E.shape[1]
        return 2.0 * float(mu) * E - pc[:, None, None] * np.eye(d)[None, :, :]
