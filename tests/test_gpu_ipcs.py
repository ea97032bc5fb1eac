"""GPU tests of the incremental pressure-correction solver (csrc/cfdh_ipcs*, the `ipcs_bdf2` plugin) against its NumPy/SciPy
twin (tests/ipcs_twin.py): operator parity, bitwise reproducibility, steps against direct solves, the symmetry of the pressure
preconditioner, Taylor-Green and DFG 2D-1 through the Scenario loop, iteration counts and wrong-context calls."""
import ctypes

import numpy as np
import pytest

import ipcs_twin as T
from util import dfg_case, stenosis_case

from cfd_hemodynamic_amd import _lib
from cfd_hemodynamic_amd.elements import NodeMesh, NodeMesh3D
from cfd_hemodynamic_amd.mesh import create_unit_square
from cfd_hemodynamic_amd.mesh3d import create_bifurcation, create_unit_cube

pytestmark = pytest.mark.gpu


def _cube_markers(m):
    fx = m.x[m.facet_vertices][:, :, 0]
    mk = np.zeros(len(m.facet_cells), dtype=np.int32)
    mk[np.isclose(fx, 0.0).all(axis=1)] = 2
    mk[np.isclose(fx, 1.0).all(axis=1)] = 3
    return mk


def _mesh(name):
    """(base mesh, P2 node mesh, facet markers, inlet marker, outlet marker): the mesh set of tests/test_gpu_pcd.py."""
    if name == "dfg":
        m = dfg_case(6).mesh
        return m, NodeMesh(m), np.asarray(m.facet_marker), 2, 3
    if name == "stenosis":
        m = stenosis_case(6, L=12.0, x_sten=5.0).mesh
        return m, NodeMesh(m), np.asarray(m.facet_marker), 2, 3
    if name == "bifurcation":
        m, _ = create_bifurcation(1.2e-3)
        return m, NodeMesh3D(m), np.asarray(m.facet_marker), 8, 9
    m = create_unit_cube(4)
    return m, NodeMesh3D(m), _cube_markers(m), 2, 3


def _objects(m, nm, mk, inlet, outlet, rng):
    """Two overlapping velocity Dirichlet objects (the inlet facets, then every facet that is neither inlet nor outlet) and one
    pressure object on the outlet vertices, random values."""
    d = m.x.shape[1]
    n_in = np.unique(nm.facet_vertices[mk == inlet].ravel()).astype(np.int32)
    n_wall = np.unique(nm.facet_vertices[(mk != inlet) & (mk != outlet)].ravel()).astype(np.int32)
    v_out = np.unique(m.facet_vertices[mk == outlet].ravel()).astype(np.int32)
    bcu = [(n_in, rng.standard_normal((len(n_in), d))), (n_wall, rng.standard_normal((len(n_wall), d)))]
    bcp = [(v_out, rng.standard_normal(len(v_out)))]
    return bcu, bcp


def _ctx(m, nm, mk, dt, rho, mu, f, bcu, bcp):
    ctx = _lib.IpcsContext(nm.x, nm.cells, m.num_vertices, nm.facet_cells, nm.facet_local, mk)
    ctx.set_params(dt, rho, mu, f=np.asarray(f, dtype=float))
    for nodes, vals in bcu:
        ctx.add_dirichlet(0, nodes, vals)
    for nodes, vals in bcp:
        ctx.add_dirichlet(1, nodes, vals)
    return ctx


def _rowerr(A, At, scale=None):
    """largest row-wise relative error of the CSR values: max_j |A_ij - At_ij| / max_j |At_ij| (or / max_j scale_ij)"""
    D = abs((A - At).tocsr())
    rowmax = np.asarray(abs(At if scale is None else scale).max(axis=1).todense()).ravel()
    err = np.asarray(D.max(axis=1).todense()).ravel()
    assert (rowmax > 0).all()
    return float((err / rowmax).max())


@pytest.mark.parametrize("name", ["dfg", "stenosis", "cube", "bifurcation"])
def test_operators_and_right_hand_sides_match_the_twin(name):
    m, nm, mk, inlet, outlet = _mesh(name)
    d, nn, nv = m.x.shape[1], nm.num_vertices, m.num_vertices
    rng = np.random.default_rng(7)
    bcu, bcp = _objects(m, nm, mk, inlet, outlet, rng)
    up, un1, p = rng.standard_normal((nn, d)), rng.standard_normal((nn, d)), rng.standard_normal(nv)
    dt, rho, mu, f = 0.013, 1.06, 3.5e-3, (0.3, -0.7, 0.2)[:d]
    tw = T.Twin(nm.x, nm.cells, nv, dt, rho, mu, f=f, bcu=bcu, bcp=bcp)
    tw.u_prev, tw.u_n1, tw.p = up.copy(), un1.copy(), p.copy()
    A1t, b1t, Af = tw.assemble1()
    op = tw.op

    def make():
        c = _ctx(m, nm, mk, dt, rho, mu, f, bcu, bcp)
        c.set_state(u_prev=up.ravel(), p_prev=p, u=up.ravel(), p=p)
        c.set_previous2(un1.ravel())
        return c

    ctx = make()
    A1 = ctx.get_operator(0)
    b1 = ctx.get_intermediate(2).reshape(nn, d)
    errs = {"A1": _rowerr(A1, A1t), "L": _rowerr(ctx.get_operator(1), tw.Lbc), "rhoM": _rowerr(ctx.get_operator(2), tw.rhoM)}
    for k in range(d):
        errs["B%d" % k] = _rowerr(ctx.get_operator(3 + k), op.B[k])
        # int phi_a vanishes for the vertex functions of a P2 triangle: those rows of G_d are zero up to round-off, so the rows are
        # scaled by the entries assembled from |phi_a| |d_k psi_b| (the sum of absolute contributions) instead of their own values
        Gabs = T._csr(np.repeat(op.c2, d + 1, 1), np.tile(op.c1, (1, op.nloc)),
                      np.einsum("q,c,qa,cb->cab", op.w, op.adet, np.abs(op.phi), np.abs(op.gl[..., k])), (nn, nv))
        errs["G%d" % k] = _rowerr(ctx.get_operator(3 + d + k), op.G[k], Gabs)
    # vectors: error relative to the row's sum of absolute contributions
    g = np.where(tw.uflag[:, None], np.abs(tw.uval), 0.0)
    s1 = (2 * rho / dt * abs(op.M) + abs(Af)) @ np.abs(up) + abs(Af) @ g + np.stack([abs(op.B[k].T) @ np.abs(p) for k in range(d)], 1) \
        + np.abs(rho * op.m1[:, None] * np.asarray(f)[None, :]) + np.abs(b1t)
    errs["b1"] = float((np.abs(b1 - b1t) / s1).max())
    # bitwise: a second pass and a second, fresh context
    ctx2 = make()
    A1b = ctx2.get_operator(0)
    b1b = ctx2.get_intermediate(2)
    assert A1.data.tobytes() == A1b.data.tobytes()
    assert b1.tobytes() == b1b.tobytes()
    ctx2.close()
    # b2, b3 from the device's own u*, phi of one step at tight tolerances
    ctx.set_tolerances(1e-11, 1e-50, 10000)
    st = ctx.step()
    assert min(st.reason) > 0, list(st.reason)
    us, ph = ctx.get_intermediate(0).reshape(nn, d), ctx.get_intermediate(1)
    b2, b3 = ctx.get_intermediate(3), ctx.get_intermediate(4).reshape(nn, d)
    b2t, b3t = tw.rhs2(us), tw.rhs3(us, ph)
    s2 = rho / dt * sum(abs(op.B[k]) @ np.abs(us[:, k]) for k in range(d)) + abs(op.L) @ np.where(tw.pflag, np.abs(tw.pval), 0.0) + np.abs(b2t)
    s3 = rho * (abs(op.M) @ np.abs(us)) + dt * np.stack([abs(op.G[k]) @ np.abs(ph) for k in range(d)], 1)
    errs["b2"] = float((np.abs(b2 - b2t) / s2).max())
    errs["b3"] = float((np.abs(b3 - b3t) / s3).max())
    print("ipcs parity %s (nn %d, nvert %d): %s" % (name, nn, nv, {k: "%.2e" % v for k, v in errs.items()}))
    ctx.close()
    for k, v in errs.items():
        assert v <= 1e-13, (k, v)


def _case(dim):
    """Small transient cases of the step test.  2-D: Taylor-Green on the unit square (8 x 8), exact velocity on the boundary, no
    pressure condition (singular Poisson problem).  3-D: channel flow in the unit cube (4^3), inlet profile at x = 0, no-slip
    walls, p = 0 at x = 1, from rest."""
    if dim == 2:
        m = create_unit_square(8, 8)
        nm = NodeMesh(m)
        k, nu = 2 * np.pi, 1.0 / 50.0
        x = nm.x
        u0 = np.stack([-np.cos(k * x[:, 0]) * np.sin(k * x[:, 1]), np.sin(k * x[:, 0]) * np.cos(k * x[:, 1])], 1)
        bnd = np.unique(nm.facet_vertices.ravel()).astype(np.int32)
        bcu = [(bnd, u0[bnd] * np.exp(-2 * nu * k * k * 0.02))]
        return m, nm, np.zeros(len(nm.facet_cells), np.int32), dict(dt=0.02, rho=1.0, mu=1.0 / 50.0), bcu, [], u0
    m = create_unit_cube(4)
    nm = NodeMesh3D(m)
    mk = _cube_markers(m)
    x = nm.x
    n_in = np.unique(nm.facet_vertices[mk == 2].ravel()).astype(np.int32)
    n_wall = np.unique(nm.facet_vertices[mk == 0].ravel()).astype(np.int32)
    v_out = np.unique(m.facet_vertices[mk == 3].ravel()).astype(np.int32)
    uin = np.zeros((len(n_in), 3))
    uin[:, 0] = 16 * x[n_in, 1] * (1 - x[n_in, 1]) * x[n_in, 2] * (1 - x[n_in, 2])
    bcu = [(n_in, uin), (n_wall, np.zeros((len(n_wall), 3)))]
    return m, nm, mk, dict(dt=0.05, rho=1.0, mu=0.1), bcu, [(v_out, np.zeros(len(v_out)))], np.zeros((len(x), 3))


def _twin_steps(dim, tol, nsteps=3):
    m, nm, mk, par, bcu, bcp, u0 = _case(dim)
    tw = T.Twin(nm.x, nm.cells, m.num_vertices, bcu=bcu, bcp=bcp, tol=tol, **par)
    tw.u_prev, tw.u_n1 = u0.copy(), u0.copy()
    out = []
    for _ in range(nsteps):
        tw.step()
        out.append((tw.u_star.copy(), tw.phi.copy(), tw.u_sol.copy(), tw.p.copy()))
        tw.advance()
    return out, tw


def _gap(a, b):
    """largest relative l2 difference per field (u*, phi, u_sol, p_sol) over the steps"""
    return [max(np.linalg.norm(x[i] - y[i]) / np.linalg.norm(y[i]) for x, y in zip(a, b)) for i in range(4)]


# Gap between the twin's own iterative solves (all tolerances 1e-12, true residual) and its direct solves over three steps,
# measured on the CPU (python -c "import test_gpu_ipcs as t; print(t.measure_twin_gaps())"): relative l2, fields u*, phi, u_sol,
# p_sol.  The device is held to 10 x these; all are far below the 1e-8 above which something other than the solver tolerance
# would be in the difference.
TWIN_GAP = {2: [7.8e-13, 2.6e-11, 2.2e-12, 2.8e-12], 3: [3.7e-11, 1.2e-11, 1.1e-11, 6.5e-12]}


def measure_twin_gaps():
    return {dim: _gap(_twin_steps(dim, 1e-12)[0], _twin_steps(dim, None)[0]) for dim in (2, 3)}


@pytest.mark.parametrize("dim", [2, 3])
def test_three_steps_against_direct_solves(dim):
    m, nm, mk, par, bcu, bcp, u0 = _case(dim)
    ref, _ = _twin_steps(dim, None)
    ctx = _ctx(m, nm, mk, par["dt"], par["rho"], par["mu"], np.zeros(dim), bcu, bcp)
    ctx.set_tolerances(1e-12, 1e-50, 10000)
    z = np.zeros(m.num_vertices)
    ctx.set_state(u_prev=u0.ravel(), p_prev=z, u=u0.ravel(), p=z)
    ctx.set_previous2(u0.ravel())
    got = []
    for _ in range(3):
        st = ctx.step()
        assert min(st.reason) > 0
        u, p = ctx.get_solution()
        got.append((ctx.get_intermediate(0).reshape(-1, dim), ctx.get_intermediate(1), u.reshape(-1, dim), p))
        ctx.advance()
    ctx.close()
    gap = _gap(got, ref)
    print("ipcs three steps, gdim %d: device vs direct %s; twin iterative vs direct %s; iterations of the last step %s"
          % (dim, ["%.2e" % g for g in gap], ["%.2e" % g for g in TWIN_GAP[dim]], list(st.its)))
    assert max(TWIN_GAP[dim]) < 1e-8
    for g, t in zip(gap, TWIN_GAP[dim]):
        assert g <= 10 * t, (gap, TWIN_GAP[dim])


@pytest.mark.parametrize("dim", [2, 3])
def test_pressure_preconditioner_symmetry_is_recorded(dim):
    """|x . V y - y . V x| / (|x| |V y|) of the V-cycle on meshes large enough for a real hierarchy (2-D: 160 x 160 unit square, no
    pressure condition, 25 921 vertices; 3-D: 16^3 unit cube with p fixed at x = 1).  The cycle keeps fp32 matrix values and fused
    composite operators, so it is symmetric to fp32 round-off at best -- the pressure solve therefore runs FLEXIBLE PCG (one more
    fused dot product per iteration).  Asserted: a cap of 1e-3 that only a structurally non-symmetric cycle (restriction !=
    prolongation^T, unequal pre- and post-smoothing) would exceed, and positivity."""
    if dim == 2:
        m = create_unit_square(160, 160)
        nm, mk, bcp = NodeMesh(m), np.zeros(len(m.facet_cells), np.int32), []
    else:
        m = create_unit_cube(16)
        nm, mk = NodeMesh3D(m), _cube_markers(m)
        v_out = np.unique(m.facet_vertices[mk == 3].ravel()).astype(np.int32)
        bcp = [(v_out, np.zeros(len(v_out)))]
    ctx = _ctx(m, nm, mk, 0.01, 1.0, 0.01, np.zeros(dim), [], bcp)
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(4):
        x, y = rng.standard_normal(m.num_vertices), rng.standard_normal(m.num_vertices)
        if not bcp:
            x, y = x - x.mean(), y - y.mean()
        Vx, Vy = ctx.apply_pressure_pc(x), ctx.apply_pressure_pc(y)
        worst = max(worst, abs(x @ Vy - y @ Vx) / (np.linalg.norm(x) * np.linalg.norm(Vy)))
        assert x @ Vx > 0 and y @ Vy > 0
    print("ipcs pressure V-cycle asymmetry, gdim %d (%d vertices, %d levels): %.3e" % (dim, m.num_vertices, ctx.info(6), worst))
    ctx.close()
    assert worst <= 1e-3


def _tg_sim(nx, dt, **kw):
    from cfd_hemodynamic_amd.scenarios.taylor_green import TaylorGreenSimulation

    class VelocityOnly(TaylorGreenSimulation):
        """No pressure condition (the scenario's own imposes the exact pressure VALUE, which the scheme puts into phi), and the
        boundary velocity of a step taken at the step's NEW time level, as the twin's Taylor-Green run does."""

        @property
        def bcp(self):
            return []

        def solve(self, output_folder=None, afterStepCallback=None, **k):
            from cfd_hemodynamic_amd.scenario import Scenario
            self._u_bc.interpolate(self.exact_velocity(self.dt))
            return Scenario.solve(self, output_folder, lambda t: self._u_bc.interpolate(self.exact_velocity(t + self.dt)), **k)

    return VelocityOnly("ipcs_bdf2", dt, 0.2, nx=nx, quiet=True, **kw)


def _tg_error(sim):
    m = sim.mesh
    nm = sim.solver.V.mesh
    op = T.Operators(nm.x, nm.cells, m.num_vertices)
    u = np.asarray(sim.solver.u_sol.x.array).reshape(-1, 2)
    ex = sim.exact_velocity(sim.t_end)(nm.x.T).T
    return T.l2_norm(op.M, u - ex) / T.l2_norm(op.M, ex)


def test_taylor_green_through_the_plugin_and_the_scenario_loop():
    nx, dt = 16, 0.01
    e_twin = T.taylor_green(nx, dt)[0]
    tw_it = T.taylor_green(nx, dt, tol=1e-5)[3]
    sim = _tg_sim(nx, dt, rtol=1e-10)
    sim.solve(max_steps=20)
    assert sim.num_steps == 20
    e_tight = _tg_error(sim)
    sim = _tg_sim(nx, dt)
    sim.solve(max_steps=20)
    e_default = _tg_error(sim)
    stats = [st for _, st in sim.step_stats]
    assert all(min(st.reason) > 0 for st in stats)
    its = np.array([list(st.its) for st in stats])
    print("ipcs Taylor-Green (16, 0.01): error twin %.4e, device rtol 1e-10 %.4e, device default %.4e" % (e_twin, e_tight, e_default))
    print("ipcs default-tolerance iterations per solve, last step: device (BiCGStab+Jacobi, FPCG+AMG, CG+Jacobi) %s, mean %s; "
          "twin (BiCGStab+Jacobi, CG+Jacobi, CG+Jacobi) %s; launches %d, host synchronisations %d, ms %.3f"
          % (list(its[-1]), ["%.1f" % v for v in its.mean(axis=0)], tw_it.its, stats[-1].launches, stats[-1].host_syncs, stats[-1].ms_total))
    assert abs(e_tight - e_twin) <= 0.01 * e_twin
    assert e_default <= 2.0 * e_twin
    # a cap that catches a broken operator or preconditioner, nothing tighter (BiCGStab counts move with the summation order)
    assert its[-1][0] <= 2 * tw_it.its[0] + 5
    assert its[-1][2] <= 2 * tw_it.its[2] + 5


def _drag_lift_host(m, nm, mk, marker, u, p, mu):
    """The boundary integral of cfdh_functional kinds 0 / 1 on the downloaded fields: P2 velocity gradient, P1 pressure, two-point
    Gauss on every edge of `marker`, n = -FacetNormal."""
    FD = FL = 0.0
    for k in np.nonzero(mk == marker)[0]:
        e, f = nm.facet_cells[k], nm.facet_local[k]
        cv = nm.cells[e]
        X = nm.x[cv[:3]]
        J = (X[1:] - X[0]).T
        Ji = np.linalg.inv(J)
        gl = np.vstack([-Ji.sum(axis=0), Ji])
        n = gl[f] / np.linalg.norm(gl[f])
        t = np.array([n[1], -n[0]])
        va, vb = (f + 1) % 3, (f + 2) % 3
        length = np.linalg.norm(X[vb] - X[va])
        for s in (0.5 - 0.5 / np.sqrt(3.0), 0.5 + 0.5 / np.sqrt(3.0)):
            lam = np.zeros(3)
            lam[va], lam[vb] = 1 - s, s
            _, dl = T.p2_tabulate(lam[None, :], 2)
            gphi = dl[0] @ gl
            ut = u[cv] @ t
            dn = (ut @ gphi) @ n
            pv = lam @ p[cv[:3]]
            FD += 0.5 * length * (mu * dn * n[1] - pv * n[0])
            FL -= 0.5 * length * (mu * dn * n[0] + pv * n[1])
    return FD, FL


def test_dfg_through_the_scenario_loop_stays_on_the_device():
    from cfd_hemodynamic_amd.scenarios.dfg_1 import DFG1Benchmark as Sim
    sim = Sim("ipcs_bdf2", 0.01, 1.0, m=8, quiet=True)
    sim.setup()
    solver = sim.solver
    nV = solver.V.dofmap.index_map.size_global * solver.V.dofmap.index_map_bs
    nQ = solver.Q.dofmap.index_map.size_global
    assert nV != 2 * nQ and nQ == sim.mesh.num_vertices
    copies0, marks = solver.ctx.info(82), []
    sim.solve(max_steps=20, afterStepCallback=lambda t: marks.append(solver.ctx.info(82)))
    assert sim.num_steps == 20 and len(marks) == 20
    assert marks[0] == marks[-1] == copies0, "a whole field crossed the host inside the time loop"
    assert all(min(st.reason) > 0 for _, st in sim.step_stats)
    FD, FL = solver.functional(0, sim.obstacle_marker), solver.functional(1, sim.obstacle_marker)
    u = np.asarray(solver.u_sol.x.array).reshape(-1, 2)
    p = np.asarray(solver.p_sol.x.array)
    m, nm = sim.mesh, solver.V.mesh
    hD, hL = _drag_lift_host(m, nm, np.asarray(m.facet_marker), sim.obstacle_marker, u, p, float(solver.mu.value))
    print("ipcs dfg_1 (m = 8, 20 steps): drag %.10e (host %.10e), lift %.10e (host %.10e), |u|_L2 %.6e, iterations of the last step %s"
          % (FD, hD, FL, hL, solver.functional(2), list(sim.step_stats[-1][1].its)))
    assert np.isfinite(FD) and FD != 0.0
    assert abs(FD - hD) <= 1e-10 * abs(hD)
    assert abs(FL - hL) <= 1e-10 * max(abs(hL), abs(hD))
    # the L2 norms of the Scenario loop against the twin's mass matrices
    op = T.Operators(nm.x, nm.cells, m.num_vertices)
    assert abs(solver.functional(2) - T.l2_norm(op.M, u)) <= 1e-12 * T.l2_norm(op.M, u)
    assert abs(solver.functional(3) - T.l2_norm(op.Mp, p)) <= 1e-12 * T.l2_norm(op.Mp, p)
    assert abs(solver.functional(4) - np.abs(u).max()) == 0.0


def test_wrong_context_calls_return_state_errors():
    m = create_unit_square(3, 3)
    nm = NodeMesh(m)
    ipcs = _lib.IpcsContext(nm.x, nm.cells, m.num_vertices, nm.facet_cells, nm.facet_local, m.facet_marker)
    newton = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, m.facet_marker)
    L = _lib.lib()
    st = _lib.Stats()
    assert L.cfdh_solve_step(ipcs.h, ctypes.byref(st)) == -3
    assert b"pressure-correction" in L.cfdh_last_error(ipcs.h)
    assert L.cfdh_assemble(ipcs.h, 1) == -3
    assert L.cfdh_set_time_scheme(ipcs.h, 1.0, 1.0, -1.0, 0.0) == -3
    z = np.zeros(3 * nm.num_vertices)
    assert L.cfdh_apply_preconditioner(ipcs.h, _lib._dp(z), _lib._dp(z)) == -3
    assert L.cfdh_get_amg_operator(ipcs.h, 1, 0, 0, ctypes.byref(ctypes.c_int64()), ctypes.byref(ctypes.c_int64()), ctypes.byref(ctypes.c_int64()), None, None, None) == -3
    assert L.cfdh_get_amg_vectors(ipcs.h, 1, 0, 0, ctypes.byref(ctypes.c_int64()), None) == -3
    ist = _lib.IpcsStats()
    assert L.cfdh_ipcs_step(newton.h, ctypes.byref(ist)) == -3
    assert b"cfdh_create_ipcs" in L.cfdh_last_error(newton.h)
    assert L.cfdh_ipcs_set_form(newton.h, 1.0, 1.0) == -3
    nnz = ctypes.c_int64()
    assert L.cfdh_ipcs_get_operator(newton.h, 0, ctypes.byref(nnz), None, None, None) == -3
    assert L.cfdh_ipcs_step(None, None) == -1
    # a step before cfdh_set_params is a state error too, not a crash
    assert L.cfdh_ipcs_step(ipcs.h, ctypes.byref(ist)) == -3
    ipcs.close()
    newton.close()


def test_drag_and_lift_of_a_shear_flow_with_known_traction():
    """u = (y, 0), p = c on the unit square, marker 7 on the bottom wall: with n = -FacetNormal = (0, 1), t = (1, 0), u_t = y and
    d_n u_t = 1 the integrals are F_D = mu |wall| = mu and F_L = -c |wall| = -c (values worked out by hand, no shared code)."""
    m = create_unit_square(6, 5)
    nm = NodeMesh(m)
    mk = np.zeros(len(m.facet_cells), np.int32)
    mk[np.isclose(m.x[m.facet_vertices][:, :, 1], 0.0).all(axis=1)] = 7
    ctx = _lib.IpcsContext(nm.x, nm.cells, m.num_vertices, nm.facet_cells, nm.facet_local, mk)
    mu, c = 0.37, 2.5
    ctx.set_params(0.1, 1.0, mu, f=np.zeros(2))
    u = np.stack([nm.x[:, 1], 0 * nm.x[:, 1]], 1)
    pc = np.full(m.num_vertices, c)
    ctx.set_state(u_prev=u.ravel(), p_prev=pc, u=u.ravel(), p=pc)
    FD, FL = ctx.functional(0, 7), ctx.functional(1, 7)
    assert ctx.functional(0, 9) == 0.0
    ctx.close()
    assert abs(FD - mu) <= 1e-13 and abs(FL + c) <= 1e-13, (FD, FL)


def _raw_step(ctx):
    st = _lib.IpcsStats()
    rc = ctx.L.cfdh_ipcs_step(ctx.h, ctypes.byref(st))
    return rc, st


@pytest.mark.parametrize("which", [0, 1, 2])
def test_iteration_cap_ends_a_solve_with_diverged_its(which):
    """max_it = 1 with a tolerance one iteration cannot meet: the step returns CFDH_E_DIVERGED, reason DIVERGED_ITS for that solve,
    no more than max_it iterations, and the binding raises RuntimeError("Did not converge, reason: -3.")."""
    m, nm, mk, par, bcu, bcp, u0 = _case(3)
    ctx = _ctx(m, nm, mk, par["dt"], par["rho"], par["mu"], np.zeros(3), bcu, bcp)
    rtol, max_it = [1e-5, 1e-5, 1e-5], [10000, 10000, 10000]
    rtol[which], max_it[which] = (0.0 if which == 1 else 1e-14), 1
    ctx.set_tolerances(rtol, 0.0, max_it)      # atol 0: the one-level pressure hierarchy is a direct solve, only |r| = 0 would pass
    z = np.zeros(m.num_vertices)
    ctx.set_state(u_prev=u0.ravel(), p_prev=z, u=u0.ravel(), p=z)
    ctx.set_previous2(u0.ravel())
    rc, st = _raw_step(ctx)
    assert rc == -4
    assert st.reason[which] == -3 and 0 < st.its[which] <= 1, (list(st.reason), list(st.its))
    assert all(st.reason[k] == 2 for k in range(which))
    assert b"did not converge" in ctx.L.cfdh_last_error(ctx.h)
    with pytest.raises(RuntimeError, match=r"Did not converge, reason: -3\."):
        ctx.step()
    # the context is still usable
    ctx.set_tolerances(1e-5, 1e-50, 10000)
    assert min(ctx.step().reason) > 0
    ctx.close()


def test_nan_in_the_state_ends_the_step_with_nanorinf():
    m, nm, mk, par, bcu, bcp, u0 = _case(2)
    ctx = _ctx(m, nm, mk, par["dt"], par["rho"], par["mu"], np.zeros(2), bcu, bcp)
    ctx.set_tolerances(1e-5, 1e-50, 50)
    bad = u0.copy()
    free = np.setdiff1d(np.arange(len(u0)), bcu[0][0])
    bad[free[3], 0] = np.nan
    z = np.zeros(m.num_vertices)
    ctx.set_state(u_prev=bad.ravel(), p_prev=z, u=u0.ravel(), p=z)
    ctx.set_previous2(u0.ravel())
    rc, st = _raw_step(ctx)
    assert rc == -4 and st.reason[0] == -9 and st.its[0] <= 50, (rc, list(st.reason), list(st.its))
    with pytest.raises(RuntimeError, match=r"Did not converge, reason: -9\."):
        ctx.step()
    ctx.close()


@pytest.mark.parametrize("args", [
    ["--simulation", "dfg_1", "--T", "0.02", "--dt", "0.01", "--m", "6"],
    ["--simulation", "lid_driven2D", "--T", "0.02", "--dt", "0.01", "--nx", "8"],
    ["--simulation", "stenosis", "--T", "0.002", "--dt", "0.001", "--ny", "6", "--v_max", "100", "--L", "12.0", "--x_sten", "5.0"],
    ["--simulation", "taylor_green", "--T", "0.02", "--dt", "0.01", "--nx", "8"],
    ["--simulation", "simple_bifurcation", "--T", "0.0002", "--dt", "0.0001", "--res", "1.2e-3"],
], ids=lambda a: a[1])
def test_command_line_run_with_output(args, tmp_path, capsys):
    """`python -m cfd_hemodynamic_amd simulate --solver ipcs_bdf2 ...` end to end with an output folder: the DOF line with two
    different counts, the VTU series (velocity on the P2 node mesh, pressure on the P1 base mesh) and the final files."""
    import re
    import warnings

    from cfd_hemodynamic_amd.__main__ import main
    from cfd_hemodynamic_amd.io import read_vtu
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # taylor_green imposes a non-zero pressure value (the plugin warns once)
        assert main(["simulate", "--solver", "ipcs_bdf2", "--name", "run", "--output_dir", str(tmp_path)] + args) == 0
    out = capsys.readouterr().out
    nV, nQ = map(int, re.search(r"DOFs: \d+ \(Velocity: (\d+), Pressure: (\d+)\)", out).groups())
    folder = tmp_path / args[1] / "run"
    v, p = read_vtu(str(folder / "v_000001.vtu")), read_vtu(str(folder / "p_000001.vtu"))
    d = 3 if args[1] == "simple_bifurcation" else 2
    assert len(v["points"]) * d == nV and len(p["points"]) == nQ and nQ < len(v["points"])
    assert v["cells"].shape[1] == (6 if d == 2 else 10) and p["cells"].shape[1] == d + 1
    assert np.isfinite(v["v"]).all() and np.abs(v["v"]).max() > 0 and np.isfinite(p["p"]).all()
    fin = np.load(str(folder / "final.npz"))
    assert fin["velocity"].size == nV and fin["pressure"].size == nQ
    assert (folder / "v.pvd").exists() and (folder / "p.pvd").exists() and (folder / "norms.txt").exists()
