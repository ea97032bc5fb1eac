"""`Scenario` ABC + the time loop that calls the hot path, with the reference's
semantics (/root/reference/src/scenario.py:20-360): solver loaded by name,
kwargs filtered by the constructor signature, `setup()`, `solve()` with the
float-accumulated `while t < T`, the every-10th-step early stop evaluated before
the prev-copy, final L2 norms written to norms.txt.

Differences, all outside the hot path: no ADIOS2/VTX output (results are kept in
memory and, optionally, written as .npz snapshots), no tqdm bar.  When the
solver offers `advance()`/`functional()` the loop keeps the fields in HBM
(`device_resident=True`, default) instead of copying `*.x.array` through the
host every step; `device_resident=False` runs the reference's literal loop.
"""
from __future__ import annotations

import inspect
import os
import time
from abc import ABC, abstractmethod
from importlib import import_module
from typing import Callable

import numpy as np

from .boundaryCondition import BoundaryCondition
from .fem import Function
from .solverBase import SolverBase


class Scenario(ABC):
    @property
    @abstractmethod
    def mesh(self):
        pass

    @property
    @abstractmethod
    def bcu(self) -> list[BoundaryCondition]:
        pass

    @property
    @abstractmethod
    def bcp(self) -> list[BoundaryCondition]:
        pass

    @abstractmethod
    def initial_velocity(self, x: np.ndarray) -> np.ndarray:
        pass

    def exact_velocity(self, t):
        pass

    def __init__(self, solver_name: str, scenario_name: str, rho: float, mu: float, dt: float, T: float, f: list,
                 early_stop_tolerance: float = 1e-3, **solver_kwargs):
        """Loads `solvers/<solver_name>.py`, keeps the keyword arguments its `Solver.__init__` can take
        (all of them when it declares **kwargs) and builds the solver on `self.mesh` -- the plugin
        protocol of /root/reference/src/scenario.py:44-133 (ImportError: no such module, ValueError: module
        without a `Solver`, RuntimeError: the constructor failed)."""
        self.solver_name, self.scenario_name = solver_name, scenario_name
        self.early_stop_tolerance = early_stop_tolerance
        self.dt, self.T = dt, T
        self.solverClass: type[SolverBase] = self._find_solver_class(solver_name)
        self.solver = self._build_solver(self.solverClass, (self.mesh, dt, rho, mu, f), solver_kwargs)
        self.has_exact_solution = type(self).exact_velocity is not Scenario.exact_velocity
        self.step_stats = []

    @staticmethod
    def _solver_names() -> list[str]:
        """Plugin modules present next to this file."""
        folder = os.path.join(os.path.dirname(os.path.abspath(__file__)), "solvers")
        if not os.path.isdir(folder):
            return []
        return sorted(n[:-3] for n in os.listdir(folder) if n.endswith(".py") and n[0] != "_")

    @classmethod
    def _find_solver_class(cls, name: str):
        try:
            module = import_module(f"{__package__}.solvers.{name}")
        except ImportError as exc:
            known = ", ".join(cls._solver_names()) or "none"
            raise ImportError(f"no solver plugin '{name}' could be imported from {__package__}/solvers "
                              f"({exc}); plugins present: {known}") from exc
        solver_class = getattr(module, "Solver", None)
        if solver_class is None:
            raise ValueError(f"{__package__}/solvers/{name}.py has no class named Solver")
        return solver_class

    def _build_solver(self, solver_class, positional, keywords: dict):
        params = inspect.signature(solver_class.__init__).parameters
        if not any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values()):
            keywords = {k: v for k, v in keywords.items() if k in params}  # silently dropped, as in the reference
        try:
            return solver_class(*positional, initial_velocity=self.initial_velocity, **keywords)
        except TypeError as exc:
            raise RuntimeError(f"solver '{self.solver_name}' rejected its constructor arguments: {exc}") from exc
        except Exception as exc:
            raise RuntimeError(f"solver '{self.solver_name}' failed during construction "
                               f"({type(exc).__name__}: {exc})") from exc

    @property
    def facet_tags(self):
        return getattr(self, "_ft", None)

    @property
    def tags(self) -> dict:
        return {
            "inlet": getattr(self, "inlet_marker", None),
            "outlet": getattr(self, "outlet_marker", None),
            "wall": getattr(self, "wall_marker", None),
            "obstacle": getattr(self, "obstacle_marker", None),
        }

    def setup(self):
        self.solver.setup(self.bcu, self.bcp, facet_tags=self.facet_tags, tags=self.tags)
        if self.mesh.comm.rank == 0 and not getattr(self, "quiet", False):
            nV = self.solver.V.dofmap.index_map.size_global * self.solver.V.dofmap.index_map_bs
            nQ = self.solver.Q.dofmap.index_map.size_global * self.solver.Q.dofmap.index_map_bs
            print(f"DOFs: {nV + nQ} (Velocity: {nV}, Pressure: {nQ})")
            print(f"Suggested cores: {(nV + nQ) / 20000:.1f}")

    def solve(self, output_folder: str = None, afterStepCallback: Callable[[float], None] = None,
              device_resident: bool = True, max_steps: int = None, write_every: int = 1, wall_indices=None, transport=None,
              transport_diffusivity: float = 0.0, particles=None, flow_diagnostics=None, probes=None, sample_grid=None, sections=None) -> str:
        """wall_indices: None (default) -- nothing; True -- the cycle-averaged wall shear indices (TAWSS, OSI, RRT, mean and peak
        wall shear stress: wall_indices.py) over the whole run; (t0, t1) -- over the steps that end in (t0, t1].  They are accumulated
        on the device with weight dt right after the step's `assemble_wss()`; afterwards `self.wall_indices` holds the fields, `W` and
        `steps`, and with an output folder wall_indices.npz / .vtu / .txt are written.

        transport: None (default) -- nothing; "age" -- blood age: source 1, c = 0 on the nodes of the facets tagged tags["inlet"];
        ("bolus", t0, t1) -- a contrast bolus: no source, inlet c = 1 for the steps that end in (t0, t1], 0 otherwise.  A passive
        scalar with diffusivity `transport_diffusivity`, stepped on the device right after the flow step and before the state is
        advanced (closed-form P1 solvers on one GPU; NotImplementedError elsewhere).  A scenario without an inlet tag runs with no
        Dirichlet set.  The field joins the VTU series as the point field `transport`; afterwards `self.transport` holds the field
        and the per-step integral, and with an output folder transport.npz is written.

        particles: None (default) -- nothing; a dict -- massless particles tracked on the device (particles.py, cfdh_particles_*):
        "n" particles per release on the facets tagged tags[release] ("release", default "inlet"), released at t = 0 and, with
        "every": K, again after every K-th step; "nsub" midpoint substeps per flow step (default 2); "seed" of the random
        positions (default 0).  They are moved right after the flow step and before the state is advanced (closed-form P1 solvers
        on one GPU; NotImplementedError elsewhere) and stop for good at the first boundary facet they meet.  Afterwards
        `self.particles` holds the final fields (x, cell, status, age, path, exposure, t_end), `seeded`, `counts` per status
        (0 active, 1 + marker exit, -1 lost) and the residence-time `summary`; with an output folder particles.npz / .txt and, at
        `write_every`, the point clouds particles/particles_NNNNNN.vtu are written.

        flow_diagnostics: None (default) -- nothing; a dict -- the volumetric diagnostics of the velocity (cfdh_flow_*), computed on
        the device right after the flow step and before the state is advanced (closed-form P1 solvers on one GPU;
        NotImplementedError elsewhere).  The 8 integrals (volume, kinetic energy, enstrophy, viscous dissipation, helicity,
        int div u, int Q, int (div u)^2) are recorded every step; "fields": a tuple of names out of vorticity, q_criterion,
        shear_rate, dissipation, helicity, lnh (the last two in 3-D) joins the VTU series as point fields at `write_every`;
        "window": True or (t0, t1) accumulates, with weight dt and the window rule of the wall indices, the mean velocity, the
        fluctuation energy k' and the mean / peak shear rate and mean dissipation.  Afterwards `self.flow_diagnostics` holds
        `integrals` [steps, 8], `times` and, under "window", those fields with `W`, `steps` and `energy_loss`; with an output folder
        flow_diagnostics.npz and flow_diagnostics.txt (per-step kinetic energy, dissipation and enstrophy, and the window's
        time-integrated dissipation: the energy loss) are written.

        probes: None (default) -- nothing; a dict -- (u, p) at the points "points" [n, gdim] (cfdh_sample_*, sampling.py), recorded
        on the device after every "every"-th step (default 1) once the step's other features have run and before the state is
        advanced; the series is downloaded when its device buffer ("rows" records, default 256) is full and at the end.
        Afterwards `self.probes` holds t [records], x, cell (-1: outside the mesh; such a probe reads zeros), u [records, n, gdim]
        and p [records, n]; with an output folder probes.npz holds the same.

        sample_grid: None (default) -- nothing; a dict -- the velocity and the pressure on a regular grid over the mesh's bounding
        box ("spacing": h, a number or one per axis, or "dims": nodes per axis; "pad": widening of the box, default 0), located
        once on the device.  With an output folder grid/grid_NNNNNN.vti (ImageData: velocity, pressure and the mask `located`) is
        written after every "every"-th step (default: `write_every`; 0: never); "window": True or (t0, t1) accumulates the means
        with weight dt under the window rule of the wall indices and writes grid_mean.vti (mean_velocity, mean_pressure,
        fluctuation).  Afterwards `self.sample_grid` holds origin, spacing, dims, cell, located and, under "window", the means with
        `W` and `steps`.  The sampler holds one set: probes and sample_grid exclude each other (ValueError).  Closed-form P1
        solvers on one GPU; NotImplementedError elsewhere.  The sample set, with its location and its means, stays on the solver
        after solve() so that `solver.sample_now()`, `sample_location()` and `sample_mean()` can still be asked about the last
        state (68 bytes per point in 3-D, 108 with the means: 1.1 to 1.8 GB for 1.6e7 nodes); only the probes' series buffer is
        freed.  `solver.sample_set_points(np.zeros((0, gdim)))` frees the rest, and so does the next set or closing the context.

        sections: None (default) -- nothing; a dict -- exact integrals over cut planes inside the domain (cfdh_section_*,
        sections.py): "planes" is a list of sections.plane(...) / sections.stations(...) entries, "every" (default 1) records the
        ten-slot rows after every such step on the device, after the step's other features and before advance(), "rows" (default
        256) is the capacity of the device buffer, which is emptied when full and at the end; "window" (t0, t1) adds the means of
        the rows with weight dt under the window rule of the wall indices.  Afterwards `self.sections` holds t, origin, normal,
        radius, rows [records, K, 10], straddling [K] and, under "window", window_mean [K, 10] with W and steps; with an output
        folder sections.npz holds the same and sections.txt one block of lines per section.  The sections have state of their
        own: they go with probes, a grid, particles and the flow diagnostics.  Closed-form P1 solvers on one GPU;
        NotImplementedError elsewhere."""
        mesh, T, solver = self.mesh, self.T, self.solver
        self.probes = self.sample_grid = None
        pr, sg = self._sample_setup(probes, sample_grid, output_folder, write_every)
        self.sections = None
        sc = self._sections_setup(sections)
        self.flow_diagnostics = None
        fd = self._flow_setup(flow_diagnostics)
        self.transport = None
        tr = self._transport_setup(transport, transport_diffusivity)
        self.particles = None
        pt = self._particles_setup(particles, output_folder if write_every else None)
        self.wall_indices = None
        if wall_indices is not None and wall_indices is not True:
            wall_indices = (float(wall_indices[0]), float(wall_indices[1]))
        if wall_indices is not None:
            from .wall_indices import step_in_window, write_outputs
            solver.wall_stats_reset()
        wi_steps = 0
        quiet = getattr(self, "quiet", False)
        if output_folder and mesh.comm.rank == 0:
            os.makedirs(output_folder, exist_ok=True)
        mesh.comm.barrier()
        solver.initStressForm()
        # v / p / u_residual / p_residual / wss time series (scenario.py:208-228): VTU + PVD instead of ADIOS2 VTX.
        # write_every = 1 is the reference's behaviour (every step); 0 disables the series.
        writers = []
        if output_folder and write_every:
            from .io import VTUWriter
            writers = [VTUWriter(mesh.comm, f"{output_folder}/v.bp", solver.u_sol, "v"),
                       VTUWriter(mesh.comm, f"{output_folder}/p.bp", solver.p_sol, "p"),
                       VTUWriter(mesh.comm, f"{output_folder}/u_residual.bp", solver.u_residual, "u_residual"),
                       VTUWriter(mesh.comm, f"{output_folder}/p_residual.bp", solver.p_residual, "p_residual"),
                       VTUWriter(mesh.comm, f"{output_folder}/wss.bp", solver.shear_stress, "shear_stress")]
            if tr is not None:
                writers.append(VTUWriter(mesh.comm, f"{output_folder}/transport.bp", tr["function"], "transport"))
            if fd is not None:
                writers += [VTUWriter(mesh.comm, f"{output_folder}/{k}.bp", fn, k) for k, fn in fd["functions"].items()]
        t = 0.0
        solver.u_sol.interpolate(self.initial_velocity)
        if writers:
            solver.assemble_wss()
            if fd is not None:
                self._flow_fields(fd)
            for w in writers:
                w.write(t)
        error_log = None
        self.errors = []  # (t, relative L2 velocity error) when the scenario has an exact solution
        if self.has_exact_solution:
            error_log = open(f"{output_folder}/err.txt", "w") if (output_folder and mesh.comm.rank == 0) else None
            u_e = Function(solver.V)
            u_e.interpolate(lambda x: self.exact_velocity(t)(x))
            error = self.compute_error(solver.u_sol, u_e, mesh)
            self.errors.append((t, error))
            if error_log:
                error_log.write("t = %.3f: error = %.3g" % (t, error) + "\n")
        fast = device_resident and hasattr(solver, "advance") and hasattr(solver, "functional")
        i = 0
        self.step_stats = []
        self.stopped_early = False
        while t < T:
            t0 = time.perf_counter()
            solver.solveStep()
            st = getattr(solver, "last_stats", None)
            self.step_stats.append((time.perf_counter() - t0, st))
            i += 1
            t += self.dt
            if self.has_exact_solution:
                u_e.interpolate(self.exact_velocity(t))
                error = self.compute_error(u_e, solver.u_sol, mesh)
                self.errors.append((t, error))
                if error_log:
                    error_log.write("t = %.3f: error = %.3g" % (t, error) + "\n")
            if tr is not None:
                self._transport_step(tr, t, bool(writers) and i % write_every == 0)
            if pt is not None:
                self._particles_step(pt, t - self.dt, i, bool(write_every) and i % write_every == 0)
            if fd is not None:
                self._flow_step(fd, t, bool(writers) and i % write_every == 0)
            solver.assemble_wss()
            if wall_indices is not None and step_in_window(t, self.dt, wall_indices):
                solver.wall_stats_accumulate(self.dt)
                wi_steps += 1
            if pr is not None and i % pr["every"] == 0:
                self._probes_record(pr, t)
            if sg is not None:
                self._grid_step(sg, t, i)
            if sc is not None:
                self._sections_step(sc, t, i)
            if writers and i % write_every == 0:
                for w in writers:
                    w.write(t)
            if afterStepCallback:
                afterStepCallback(t)
            if (i + 1) % 10 == 0:
                if fast:
                    u_sol_norm = solver.functional(4)
                    u_prev_norm = solver.functional(5)
                    u_diff_norm = solver.functional(6)
                else:
                    u_sol_arr = solver.u_sol.x.array
                    u_prev_arr = solver.u_prev.x.array
                    u_sol_norm = mesh.comm.allreduce(np.linalg.norm(u_sol_arr, ord=np.inf))
                    u_prev_norm = mesh.comm.allreduce(np.linalg.norm(u_prev_arr, ord=np.inf))
                    u_diff_norm = mesh.comm.allreduce(np.linalg.norm(u_sol_arr - u_prev_arr, ord=np.inf))
                rel_diff = (u_diff_norm / max(u_sol_norm, 1e-12)) / self.dt
                if mesh.comm.rank == 0 and not quiet:
                    print(f"Step {i+1}: t={t:.3f} ||u_sol||={u_sol_norm:.6e}, ||u_prev||={u_prev_norm:.6e}, "
                          f"||diff||={u_diff_norm:.6e} rel_diff/dt={rel_diff:.6e}")
                if rel_diff < self.early_stop_tolerance:
                    if mesh.comm.rank == 0 and not quiet:
                        print(f"Early stopping at t={t:.3f}, because (||u_sol - u_prev||_inf / ||u_sol||_inf) / dt = "
                              f"{rel_diff:.20e} < {self.early_stop_tolerance}")
                    self.stopped_early = True
                    break
            if fast:
                solver.advance()
            else:
                solver.u_prev.x.array[:] = solver.u_sol.x.array[:]
                solver.p_prev.x.array[:] = solver.p_sol.x.array[:]
            if max_steps is not None and i >= max_steps:
                break
        self.num_steps = i
        self.t_end = t
        if fast:
            norm_v, norm_p = solver.functional(2), solver.functional(3)
        else:
            norm_v, norm_p = self._l2_norms_host()
        self.norm_v, self.norm_p = norm_v, norm_p
        solver.assemble_wss()
        if output_folder:
            # reading `x.array` gathers the owned slices in a partitioned run: every rank takes part, rank 0 writes
            fields = {k: np.asarray(f.x.array) for k, f in (('velocity', solver.u_sol), ('pressure', solver.p_sol), ('wss', solver.shear_stress))}
            if mesh.comm.rank == 0:
                with open(os.path.join(output_folder, "norms.txt"), "w") as f:
                    f.write(f"L2 norm of velocity: {norm_v}\n")
                    f.write(f"L2 norm of pressure: {norm_p}\n")
                np.savez(os.path.join(output_folder, "final.npz"), x=mesh.x, cells=mesh.cells, **fields)
            mesh.comm.barrier()
        if wall_indices is not None:
            if wi_steps > 0:
                self.wall_indices = solver.wall_indices()
                if output_folder and mesh.comm.rank == 0:
                    fields = self.wall_indices
                    write_outputs(output_folder, solver.shear_stress.function_space.mesh, fields, fields["W"], fields["steps"])
            elif mesh.comm.rank == 0:
                print("wall_indices: no step ended inside the window %s (the run stopped at t=%.6g): nothing written" % (wall_indices, t))
        if tr is not None:
            self.transport = {"mode": tr["mode"], "field": np.asarray(solver.transport_field()), "integral": np.array(tr["integral"]),
                              "times": np.array(tr["times"]), "iterations": np.array(tr["its"], dtype=np.int64)}
            if output_folder and mesh.comm.rank == 0:
                np.savez(os.path.join(output_folder, "transport.npz"), x=mesh.x, cells=mesh.cells,
                         **{k: v for k, v in self.transport.items() if k != "mode"})
        if fd is not None:
            self.flow_diagnostics = {"integrals": np.array(fd["integrals"]).reshape(-1, 8), "times": np.array(fd["times"])}
            if fd["window_steps"] > 0:
                self.flow_diagnostics["window"] = dict(solver.flow_stats(), energy_loss=fd["energy_loss"])
            elif fd["window"] is not None and mesh.comm.rank == 0:
                print("flow_diagnostics: no step ended inside the window %s (the run stopped at t=%.6g)" % (fd["window"], t))
            if output_folder and mesh.comm.rank == 0:
                self._flow_write(output_folder, self.flow_diagnostics)
        if pr is not None:
            self._probes_drain(pr)
            solver._sample_ctx().sample_series_enable(0)  # the series buffer is of no use after the run; the set stays (docstring)
            self.probes = {"t": np.concatenate(pr["t"]) if pr["t"] else np.zeros(0), "x": pr["x"], "cell": pr["cell"],
                           "u": np.concatenate(pr["u"]) if pr["u"] else np.zeros((0,) + pr["x"].shape),
                           "p": np.concatenate(pr["p"]) if pr["p"] else np.zeros((0, len(pr["x"])))}
            if output_folder and mesh.comm.rank == 0:
                from .sampling import write_npz
                write_npz(os.path.join(output_folder, "probes.npz"), **self.probes)
        if sg is not None:
            self.sample_grid = {k: sg[k] for k in ("origin", "spacing", "dims", "cell", "located")}
            if sg["window_steps"] > 0:
                self.sample_grid["window"] = solver.sample_mean()
                if output_folder and mesh.comm.rank == 0:
                    from .sampling import write_vti
                    win = self.sample_grid["window"]
                    write_vti(os.path.join(output_folder, "grid_mean.vti"), sg["origin"], sg["spacing"], sg["dims"],
                              {k: win[k] for k in ("mean_velocity", "mean_pressure", "fluctuation")}, located=sg["cell"] >= 0)
            elif sg["window"] is not None and mesh.comm.rank == 0:
                print("sample_grid: no step ended inside the window %s (the run stopped at t=%.6g)" % (sg["window"], t))
        if sc is not None:
            self._sections_finish(sc, output_folder, t)
        if pt is not None:
            from . import particles as P
            fields = solver.particles_get()
            summary = P.residence_times(fields["status"], fields["age"])
            self.particles = dict(fields, seeded=pt["seeded"], counts={s: r["count"] for s, r in summary.items()}, summary=summary,
                                  stepped=np.array(pt["stepped"], dtype=np.int64), ms_kernel=np.array(pt["ms_kernel"]))
            if output_folder and mesh.comm.rank == 0:
                P.write_npz(os.path.join(output_folder, "particles.npz"), fields, summary)
                P.write_summary(os.path.join(output_folder, "particles.txt"), summary, t)
        for w in writers:
            w.close()
        if error_log:
            error_log.close()
        return output_folder

    def _sample_setup(self, probes, sample_grid, output_folder, write_every):
        """Parses `probes` and `sample_grid` of solve() and puts the sample set on the solver; (None, None) when off."""
        if probes is None and sample_grid is None:
            return None, None
        if probes is not None and sample_grid is not None:
            raise ValueError("the sampler holds one sample set: give either probes or sample_grid")
        solver = self.solver
        gdim = self.mesh.geometry.dim
        if probes is not None:
            if not isinstance(probes, dict) or set(probes) - {"points", "every", "rows"} or "points" not in probes:
                raise ValueError('probes must be None or a dict with "points" and optionally "every" and "rows"')
            pts = np.asarray(probes["points"], dtype=float).reshape(-1, gdim)
            every, rows = int(probes.get("every", 1)), int(probes.get("rows", 256))
            if len(pts) == 0 or every < 1 or rows < 1:
                raise ValueError("probes: at least one point, every >= 1 and rows >= 1")
            solver._sample_ctx()  # the solver kinds without the sampler raise here, before the time loop
            solver.sample_set_points(pts)
            cell, _, x = solver.sample_location()
            solver._sample_ctx().sample_series_enable(rows)
            return {"every": every, "rows": rows, "waiting": 0, "x": x, "cell": cell, "t": [], "u": [], "p": []}, None
        if not isinstance(sample_grid, dict) or set(sample_grid) - {"spacing", "dims", "pad", "every", "window"}:
            raise ValueError('sample_grid must be None or a dict with "spacing" or "dims" and optionally "pad", "every" and "window"')
        from .sampling import grid_over
        origin, spacing, dims = grid_over(self.mesh, spacing=sample_grid.get("spacing"), pad=float(sample_grid.get("pad", 0.0)),
                                          dims=sample_grid.get("dims"))
        window = sample_grid.get("window")
        if window is not None and window is not True:
            window = (float(window[0]), float(window[1]))
        every = int(sample_grid.get("every", write_every or 0))
        if every < 0:
            raise ValueError("sample_grid: every >= 0")
        solver._sample_ctx()
        solver.sample_set_grid(origin, spacing, dims)
        cell = solver.sample_location()[0]
        if window is not None:
            solver.sample_mean_reset()
        folder = None
        if output_folder and every and self.mesh.comm.rank == 0:
            folder = os.path.join(output_folder, "grid")
            os.makedirs(folder, exist_ok=True)
        return None, {"origin": origin, "spacing": spacing, "dims": dims, "cell": cell, "located": int((cell >= 0).sum()), "every": every,
                      "window": window, "window_steps": 0, "folder": folder, "frames": 0}

    def _sections_setup(self, sections):
        """Parses `sections` of solve() and puts the sections on the solver; None when off."""
        if sections is None:
            return None
        if not isinstance(sections, dict) or set(sections) - {"planes", "every", "rows", "window"} or "planes" not in sections:
            raise ValueError('sections must be None or a dict with "planes" and optionally "every", "rows" and "window"')
        from .sections import as_arrays
        origin, normal, radius = as_arrays(sections["planes"])
        every, rows = int(sections.get("every", 1)), int(sections.get("rows", 256))
        if len(origin) < 1 or every < 1 or rows < 1:
            raise ValueError("sections: at least one plane, every >= 1 and rows >= 1")
        window = sections.get("window")
        if window is not None:
            window = (float(window[0]), float(window[1]))
        solver = self.solver
        ctx = solver._section_ctx()  # the solver kinds without the sections raise here, before the time loop
        solver.section_set((origin, normal, radius))
        ctx.section_series_enable(rows)
        if window is not None:
            solver.section_mean_reset()
        return {"origin": origin, "normal": normal, "radius": radius, "every": every, "rows": rows, "window": window, "window_steps": 0,
                "straddling": solver.section_cut()[3], "t": [], "out": []}

    def _sections_step(self, sc, t, i):
        solver = self.solver
        if sc["window"] is not None:
            from .wall_indices import step_in_window
            if step_in_window(t, self.dt, sc["window"]):
                solver.section_mean_accumulate(self.dt)
                sc["window_steps"] += 1
        if i % sc["every"] == 0:
            if solver._section_ctx().info(124) == sc["rows"]:
                self._sections_drain(sc)
            solver.section_record(t)

    def _sections_drain(self, sc):
        t, out = self.solver.section_series()
        if len(t):
            sc["t"].append(t)
            sc["out"].append(out)

    def _sections_finish(self, sc, output_folder, t):
        solver = self.solver
        self._sections_drain(sc)
        solver._section_ctx().section_series_enable(0)  # the buffer is of no use after the run; the sections stay on the solver
        K = len(sc["origin"])
        self.sections = {"t": np.concatenate(sc["t"]) if sc["t"] else np.zeros(0), "origin": sc["origin"], "normal": sc["normal"],
                         "radius": sc["radius"], "rows": np.concatenate(sc["out"]) if sc["out"] else np.zeros((0, K, 10)),
                         "straddling": sc["straddling"]}
        if sc["window_steps"] > 0:
            win = solver.section_mean()
            self.sections.update(window_mean=win["rows"], window_W=win["W"], window_steps=win["steps"])
        elif sc["window"] is not None and self.mesh.comm.rank == 0:
            print("sections: no step ended inside the window %s (the run stopped at t=%.6g)" % (sc["window"], t))
        if output_folder and self.mesh.comm.rank == 0:
            from .sections import write_npz, write_txt
            write_npz(os.path.join(output_folder, "sections.npz"), **self.sections)
            write_txt(os.path.join(output_folder, "sections.txt"), self.sections["t"], self.sections["rows"], sc["origin"], sc["normal"],
                      sc["radius"], sc["straddling"])

    def _probes_record(self, pr, t):
        if pr["waiting"] == pr["rows"]:
            self._probes_drain(pr)
        self.solver.sample_record(t)
        pr["waiting"] += 1

    def _probes_drain(self, pr):
        if pr["waiting"]:
            t, u, p = self.solver.sample_series()
            pr["t"].append(t); pr["u"].append(u); pr["p"].append(p)
            pr["waiting"] = 0

    def _grid_step(self, sg, t, i):
        from .wall_indices import step_in_window
        solver = self.solver
        if sg["window"] is not None and step_in_window(t, self.dt, sg["window"]):
            solver.sample_mean_accumulate(self.dt)
            sg["window_steps"] += 1
        if sg["folder"] and i % sg["every"] == 0:
            from .sampling import write_vti
            u, p = solver.sample_now()
            write_vti(os.path.join(sg["folder"], "grid_%06d.vti" % sg["frames"]), sg["origin"], sg["spacing"], sg["dims"],
                      {"velocity": u, "pressure": p}, located=sg["cell"] >= 0)
            sg["frames"] += 1

    FLOW_FIELD_NAMES = ("vorticity", "q_criterion", "shear_rate", "dissipation", "helicity", "lnh")

    def _flow_setup(self, flow_diagnostics):
        """Parses `flow_diagnostics` of solve() and resets the window averages on the solver; None when off."""
        if flow_diagnostics is None:
            return None
        unknown = set(flow_diagnostics) - {"fields", "window"}
        names = tuple(flow_diagnostics.get("fields", ()))
        gdim = self.mesh.geometry.dim
        bad = [k for k in names if k not in self.FLOW_FIELD_NAMES or (gdim == 2 and k in ("helicity", "lnh"))]
        if unknown or bad:
            raise ValueError('flow_diagnostics must be None or a dict with "fields" (out of %s; helicity and lnh in 3-D only) and "window"'
                             % ", ".join(self.FLOW_FIELD_NAMES))
        window = flow_diagnostics.get("window")
        if window is not None and window is not True:
            window = (float(window[0]), float(window[1]))
        solver = self.solver
        solver._flow_ctx()  # the solver kinds without the diagnostics raise here, before the time loop
        if window is not None:
            solver.flow_stats_reset()
        functions = {k: Function(solver.V if (k == "vorticity" and gdim == 3) else solver.Q, name=k) for k in names}
        return {"functions": functions, "window": window, "window_steps": 0, "energy_loss": 0.0, "integrals": [], "times": []}

    def _flow_fields(self, fd):
        for k, fn in fd["functions"].items():
            fn.x.array[:] = np.asarray(self.solver.flow_field(k)).reshape(-1)

    def _flow_step(self, fd, t, write):
        from .wall_indices import step_in_window
        solver = self.solver
        fd["integrals"].append(solver.flow_integrals())
        fd["times"].append(t)
        if fd["window"] is not None and step_in_window(t, self.dt, fd["window"]):
            solver.flow_stats_accumulate(self.dt)
            fd["window_steps"] += 1
            fd["energy_loss"] += self.dt * fd["integrals"][-1][3]
        if write:
            self._flow_fields(fd)

    @staticmethod
    def _flow_write(output_folder, fd):
        """flow_diagnostics.npz (everything) and flow_diagnostics.txt (energies per step, the window's energy loss)."""
        flat = {"integrals": fd["integrals"], "times": fd["times"]}
        win = fd.get("window")
        if win is not None:
            flat.update({"window_" + k: np.asarray(v) for k, v in win.items()})  # the fields, W, steps, energy_loss
        np.savez(os.path.join(output_folder, "flow_diagnostics.npz"), **flat)
        with open(os.path.join(output_folder, "flow_diagnostics.txt"), "w") as f:
            f.write("# t  kinetic_energy  viscous_dissipation  enstrophy\n")
            for t, row in zip(fd["times"], fd["integrals"]):
                f.write("%.9g %.12e %.12e %.12e\n" % (t, row[1], row[3], row[2]))
            if win is not None:
                f.write("# window: %d steps, W = %.9g\n" % (win["steps"], win["W"]))
                f.write("# mean shear rate: max over the vertices %.12e; peak shear rate: %.12e\n"
                        % (win["mean_shear_rate"].max(), win["peak_shear_rate"].max()))
                f.write("# energy loss: time-integrated viscous dissipation over the window = %.12e\n" % win["energy_loss"])

    def _particles_setup(self, particles, cloud_folder):
        """Parses `particles` of solve(), enables the tracker on the solver and makes the first release; None when off."""
        if particles is None:
            return None
        unknown = set(particles) - {"n", "release", "every", "nsub", "seed"}
        if unknown or "n" not in particles or int(particles["n"]) < 1:
            raise ValueError('particles must be None or a dict with "n" >= 1 and optionally "release", "every", "nsub", "seed"')
        from . import particles as P
        n, every = int(particles["n"]), particles.get("every")
        if every is not None and int(every) < 1:
            raise ValueError('particles["every"] must be >= 1')
        release = particles.get("release", "inlet")
        marker, ft = self.tags.get(release), self.facet_tags
        if marker is None or ft is None or len(ft.find(marker)) == 0:
            raise ValueError("particles: the scenario has no facets tagged %r to release from" % release)
        nsteps = int(np.ceil(self.T / self.dt - 1e-9))
        releases = 1 if every is None else 1 + (nsteps - 1) // int(every)
        solver = self.solver
        solver.particles_enable(n * releases, int(particles.get("nsub", 2)))
        pt = {"n": n, "every": None if every is None else int(every), "facets": np.asarray(ft.find(marker)), "seeded": 0,
              "rng": np.random.default_rng(int(particles.get("seed", 0))), "capacity": n * releases, "stepped": [], "ms_kernel": [],
              "cloud": P.CloudWriter(os.path.join(cloud_folder, "particles")) if cloud_folder and self.mesh.comm.rank == 0 else None}
        self._particles_release(pt, 0.0)
        return pt

    def _particles_release(self, pt, t):
        from . import particles as P
        if pt["seeded"] + pt["n"] > pt["capacity"]:
            return
        x, cells = P.sample_on_marker(self.mesh, pt["facets"], pt["n"], pt["rng"])
        self.solver.particles_seed(x, cells, t)
        pt["seeded"] += pt["n"]

    def _particles_step(self, pt, t0, i, write):
        st = self.solver.particles_step(t0)
        pt["stepped"].append(st.stepped)
        pt["ms_kernel"].append(st.ms_kernel)
        if write and pt["cloud"] is not None:
            pt["cloud"].write(t0 + self.dt, self.solver.particles_get())
        if pt["every"] is not None and i % pt["every"] == 0 and t0 + self.dt < self.T:
            self._particles_release(pt, t0 + self.dt)

    def _transport_setup(self, transport, diffusivity):
        """Parses `transport` of solve(), enables the scalar on the solver and sets the inlet Dirichlet set; None when off."""
        if transport is None:
            return None
        if isinstance(transport, str):
            transport = (transport,)
        mode = transport[0]
        if mode == "age" and len(transport) == 1:
            window, source = None, 1.0
        elif mode == "bolus" and len(transport) == 3:
            window, source = (float(transport[1]), float(transport[2])), 0.0
        else:
            raise ValueError('transport must be None, "age" or ("bolus", t0, t1)')
        solver = self.solver
        inlet, ft = self.tags.get("inlet"), self.facet_tags
        nodes = np.zeros(0, dtype=np.int32)
        if inlet is not None and ft is not None:
            nodes = np.unique(np.asarray(self.mesh.facet_vertices)[ft.find(inlet)]).astype(np.int32)
        solver.transport_enable(D=float(diffusivity), s=source, theta_c=0.5, nodes=nodes, values=0.0)
        solver.transport_field(np.zeros(self.mesh.num_vertices))
        fn = Function(solver.Q, name="transport")
        return {"mode": mode, "window": window, "nodes": nodes, "value": 0.0, "function": fn, "integral": [], "times": [], "its": []}

    def _transport_step(self, tr, t, write):
        solver = self.solver
        if tr["window"] is not None and len(tr["nodes"]):
            value = 1.0 if tr["window"][0] < t - 1e-12 * self.dt and t <= tr["window"][1] + 1e-12 * self.dt else 0.0
            if value != tr["value"]:
                solver.transport_set_dirichlet(tr["nodes"], value)
                tr["value"] = value
        st = solver.transport_step()
        tr["integral"].append(solver.transport_functional(0))
        tr["times"].append(t)
        tr["its"].append(st.its)
        if write:
            tr["function"].x.array[:] = solver.transport_field()

    @staticmethod
    def _mass_weights(mesh):
        """int_K l_a l_b = |K| (1 + d_ab) / ((d+1)(d+2)) per cell."""
        n1 = mesh.cells.shape[1]
        vol = mesh.cell_areas() if n1 == 3 else mesh.cell_volumes()
        return vol[:, None, None] * (1.0 + np.eye(n1))[None] / (n1 * (n1 + 1.0))

    def _l2_norms_host(self):
        m = self.mesh
        mab = self._mass_weights(m)
        ue = np.asarray(self.solver.u_sol.x.array).reshape(-1, m.geometry.dim)[m.cells]
        pe = np.asarray(self.solver.p_sol.x.array)[m.cells]
        return (float(np.sqrt(np.einsum("cab,cai,cbi->", mab, ue, ue))),
                float(np.sqrt(np.einsum("cab,ca,cb->", mab, pe, pe))))

    @staticmethod
    def compute_error(u: Function, u_aprox: Function, mesh) -> float:
        """Relative L2 error (/root/reference/src/scenario.py:350-360)."""
        mab = Scenario._mass_weights(mesh)
        bs = u.function_space.bs
        a = u.x.array.reshape(-1, bs)[mesh.cells]
        b = u_aprox.x.array.reshape(-1, bs)[mesh.cells]
        d = b - a
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.sqrt(np.einsum("cab,cai,cbi->", mab, d, d)) / np.sqrt(np.einsum("cab,cai,cbi->", mab, a, a)))
