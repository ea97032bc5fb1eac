"""The rotational form of the pressure-driven solvers on the GPU (gen_asm_kernel<ET, JAC, true>, csrc/cfdh_gen.hip) against the
NumPy twin (tests/rot_twin.py): assembly, SpMV, reproducibility, the value-only boundary update, time steps, and the plugins
`stabilized_schur_pressurebc` / `stabilized_schur_vascularbc` (/root/reference/src/solvers/stabilized_schur_pressurebc.py,
stabilized_schur_vascularbc.py)."""
import os

import numpy as np
import pytest

from cfd_hemodynamic_amd import _lib
from cfd_hemodynamic_amd.elements import NodeMesh
from cfd_hemodynamic_amd.mesh import create_unit_square
from gen_util import ETYPE, LIB_ETYPE, facet_node_set, node_mesh, stenosis_nodes
from oracle import np_twin as T
import rot_twin as RT

pytestmark = pytest.mark.gpu
MMHG = 133.322


def _sides(m, kind=None, distort=0.0):
    """Left / right ends and the remaining (wall) facets, from the undistorted end vertices of each facet."""
    x = m.x[np.asarray(m.facet_vertices)[:, :2]]
    x0 = x[..., 0] - distort * (x[..., 1] if kind == "Q1" else np.sin(3.0 * x[..., 1]))
    left = np.nonzero(np.all(np.isclose(x0, x0.min()), axis=1))[0]
    right = np.nonzero(np.all(np.isclose(x0, x0.max()), axis=1))[0]
    return left, right, np.setdiff1d(np.arange(m.num_facets), np.concatenate([left, right]))


def _pair(kind, m, prm, sets, values, beta, markers_ids=(2, 3)):
    """Twin and context with the same mesh, parameters and pressure boundaries (facet sets -> markers 2, 3)."""
    pb = RT.Problem(ETYPE[kind], m.x, m.cells, m.facet_cells, m.facet_local, prm)
    pb.set_pressure_boundaries(sets, values, beta)
    markers = np.zeros(m.num_facets, dtype=np.int32)
    for mk, fs in zip(markers_ids, sets):
        markers[fs] = mk
    ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, markers, etype=LIB_ETYPE[kind])
    ctx.set_params(prm.dt, prm.rho, prm.mu, f=prm.f)
    ctx.set_time_scheme(prm.theta, prm.a0, prm.a1, prm.a2)
    ctx.set_boundary_terms(ds_terms=False)
    ctx.set_formulation(_lib.FORM_ROTATIONAL)
    ctx.set_pressure_boundaries(list(markers_ids[: len(sets)]), values, beta)
    return pb, ctx


@pytest.mark.parametrize("kind", ["P1", "P2", "Q1"])
@pytest.mark.parametrize("scheme", [dict(), dict(theta=1.0, a0=1.5, a1=-2.0, a2=0.5)])
def test_assembly_matches_the_twin(kind, scheme):
    rng = np.random.default_rng(5)
    m = node_mesh(kind, 12, distort=0.05)
    nv = m.num_vertices
    prm = T.Params(0.02, 1.3, 0.04, (0.2, -0.1), **scheme)
    left, right, walls = _sides(m, kind, 0.05)
    pb, ctx = _pair(kind, m, prm, [left, right], [1.7, -0.4], 30.0)
    wn = facet_node_set(m, walls)[::2]
    vals = rng.standard_normal((len(wn), 2))
    pb.add_bc_u(wn, vals)
    ctx.add_dirichlet(0, wn, vals)
    xv, un, un2 = 0.3 * rng.standard_normal(3 * nv), 0.3 * rng.standard_normal((nv, 2)), 0.3 * rng.standard_normal((nv, 2))
    F, J = pb.assemble(xv, un, un2=un2)
    ctx.set_state(u_prev=un.ravel(), p_prev=np.zeros(nv), u=xv[: 2 * nv], p=xv[2 * nv:])
    ctx.set_previous2(un2.ravel())
    ctx.assemble(True)
    Fg = np.concatenate(ctx.get_residual())
    Jg = ctx.get_csr()
    assert np.abs(Fg - F).max() <= 1e-12 * np.abs(F).max()
    assert abs(Jg - J).max() <= 1e-12 * abs(J).max()
    y = rng.standard_normal(3 * nv)
    assert np.abs(ctx.spmv(y) - J @ y).max() <= 1e-12 * np.abs(J @ y).max()
    # the residual-only pass (line-search trial points) gives the same bits
    ctx.assemble(False)
    assert np.array_equal(np.concatenate(ctx.get_residual()), Fg)
    assert ctx.info(77) == _lib.FORM_ROTATIONAL
    ctx.close()


@pytest.mark.parametrize("kind", ["P1", "P2", "Q1"])
def test_rotational_assembly_is_bitwise_reproducible(kind):
    rng = np.random.default_rng(12)
    m = node_mesh(kind, 30, distort=0.05)
    nv = m.num_vertices
    prm = T.Params(0.02, 1.3, 0.04, (0.2, -0.1))
    left, right, walls = _sides(m, kind, 0.05)
    wn = facet_node_set(m, walls)
    xv, un = 0.3 * rng.standard_normal(3 * nv), 0.3 * rng.standard_normal((nv, 2))
    out = []
    for _ in range(2):
        _, ctx = _pair(kind, m, prm, [left, right], [1.7, -0.4], 30.0)
        ctx.add_dirichlet(0, wn, np.zeros((len(wn), 2)))
        ctx.set_state(u_prev=un.ravel(), p_prev=np.zeros(nv), u=xv[: 2 * nv], p=xv[2 * nv:])
        for _rep in range(2):
            ctx.assemble(True)
            out.append((np.concatenate(ctx.get_residual()), ctx.get_csr().data.copy()))
        ctx.close()
    for F, A in out[1:]:
        assert np.array_equal(F, out[0][0]) and np.array_equal(A, out[0][1])


def _channel(kind, n):
    if kind == "Q1":
        return node_mesh("Q1", n)
    m = create_unit_square(2 * n, n)
    m.x[:, 0] *= 2.0
    return m if kind == "P1" else NodeMesh(m)


def test_value_only_update_keeps_jacobian_and_preconditioner():
    """The per-step resistance update: new VALUES of the pressure boundaries leave the assembled Jacobian (bit for bit) and the
    preconditioner valid; the residual equals that of a fresh context created with the new values."""
    m = _channel("P1", 8)
    nv = m.num_vertices
    prm = T.Params(0.01, 1.0, 0.05, (0.0, 0.0))
    left, right, walls = _sides(m)
    wn = facet_node_set(m, walls)
    _, ctx = _pair("P1", m, prm, [left, right], [4.0, 1.0], 100.0)
    ctx.add_dirichlet(0, wn, np.zeros((len(wn), 2)))
    z2, z1 = np.zeros(2 * nv), np.zeros(nv)
    ctx.set_state(u_prev=z2, p_prev=z1, u=z2, p=z1)
    ctx.solve_step()
    assert ctx.info(75) == 1 and ctx.info(76) == 0   # preconditioner built; the pressure level is fixed: not singular
    builds = ctx.info(74)
    u, p = ctx.get_solution()
    ctx.assemble(True)
    J0 = ctx.get_csr().data.copy()
    ctx.set_pressure_boundaries([2, 3], [4.0, 2.5], 100.0)   # value only
    assert ctx.info(75) == 1 and np.array_equal(ctx.get_csr().data, J0)
    ctx.assemble(True)
    F1 = np.concatenate(ctx.get_residual())
    assert np.array_equal(ctx.get_csr().data, J0) and ctx.info(75) == 1 and ctx.info(74) == builds
    _, fresh = _pair("P1", m, prm, [left, right], [4.0, 2.5], 100.0)
    fresh.add_dirichlet(0, wn, np.zeros((len(wn), 2)))
    fresh.set_state(u_prev=z2, p_prev=z1, u=u, p=p)
    fresh.assemble(True)
    assert np.array_equal(np.concatenate(fresh.get_residual()), F1)
    fresh.close()
    # any other change invalidates both
    ctx.set_pressure_boundaries([2, 3], [4.0, 2.5], 50.0)
    assert ctx.info(75) == 0
    ctx.close()


def _steps(pb, ctx, nv, nsteps, tol_u=1e-8, tol_p=1e-7, x0=None, update=None):
    o = ctx.default_options()
    o.snes_rtol, o.snes_stol, o.ksp_rtol = 1e-12, 0.0, 1e-10
    ctx.set_options(o)
    x = np.zeros(3 * nv) if x0 is None else x0.copy()
    ctx.set_state(u_prev=x[: 2 * nv], p_prev=x[2 * nv:], u=x[: 2 * nv], p=x[2 * nv:])
    un = x[: 2 * nv].reshape(-1, 2).copy()
    for step in range(nsteps):
        st = ctx.solve_step()
        assert st.reason > 0 and ctx.info(76) == 0
        u, p = ctx.get_solution()
        ctx.advance()
        x, _ = pb.newton(x, un)
        un = x[: 2 * nv].reshape(-1, 2).copy()
        assert np.abs(u - x[: 2 * nv]).max() <= tol_u * np.abs(x[: 2 * nv]).max(), step
        assert np.abs(p - x[2 * nv:]).max() <= tol_p * np.abs(x[2 * nv:]).max(), step
    return x


@pytest.mark.parametrize("kind", ["P1", "P2", "Q1"])
def test_time_steps_on_a_channel_match_the_twin(kind):
    """Three steps, walls no-slip, natural pressures on both ends: device Newton + FGMRES vs the twin's direct Newton."""
    m = _channel(kind, 6)
    nv = m.num_vertices
    prm = T.Params(0.02, 1.0, 0.05, (0.0, 0.0))
    left, right, walls = _sides(m)
    pb, ctx = _pair(kind, m, prm, [left, right], [2.0, 0.5], 100.0)
    wn = facet_node_set(m, walls)
    pb.add_bc_u(wn, np.zeros((len(wn), 2)))
    ctx.add_dirichlet(0, wn, np.zeros((len(wn), 2)))
    x = _steps(pb, ctx, nv, 3)
    assert pb.flux(x, right) > 0   # down the pressure drop
    ctx.close()


@pytest.mark.parametrize("kind", ["P1", "P2"])
def test_time_steps_on_the_stenosis_match_the_twin(kind):
    m, ft = stenosis_nodes(kind, 6)
    nv = m.num_vertices
    prm = T.Params(0.01, 1.06e-3, 3.5e-3, (0.0, 0.0))
    pb, ctx = _pair(kind, m, prm, [ft.find(2), ft.find(3)], [MMHG / 2, 0.8 * MMHG / 2], 100.0)
    wn = facet_node_set(m, ft.find(4))
    pb.add_bc_u(wn, np.zeros((len(wn), 2)))
    ctx.add_dirichlet(0, wn, np.zeros((len(wn), 2)))
    _steps(pb, ctx, nv, 3)
    ctx.close()


def test_poiseuille_channel_through_the_plugin_equals_the_twin():
    """stabilized_schur_pressurebc on the straight channel of the twin's Poiseuille study (Re ~ 1e-3): three midpoint steps of
    the plugin equal the twin's discrete solution."""
    from cfd_hemodynamic_amd.boundaryCondition import BoundaryCondition
    from cfd_hemodynamic_amd.fem import Function
    from cfd_hemodynamic_amd.mesh import meshtags
    from cfd_hemodynamic_amd.solvers.stabilized_schur_pressurebc import Solver
    L, mu, rho, p_in, p_out, dt = 4.0, 1.0, 0.01, 8.0, 0.0, 0.05
    m = create_unit_square(32, 8)
    m.x[:, 0] *= L
    nv = m.num_vertices
    left, right, walls = _sides(m)
    idx = np.concatenate([left, right, walls])
    ft = meshtags(m, 1, idx, np.concatenate([np.full(len(left), 2), np.full(len(right), 3), np.full(len(walls), 4)]).astype(np.int32))
    s = Solver(m, dt, rho, mu, [0.0, 0.0], p_inlet=p_in, p_outlet=p_out, quiet=True,
               options=dict(snes_rtol=1e-12, snes_stol=0.0, ksp_rtol=1e-10))
    bc = BoundaryCondition(Function(s.V))
    bc.initTopological(1, ft.find(4))
    s.setup([bc], [], facet_tags=ft, tags=dict(inlet=2, outlet=3, wall=4))
    assert s.ctx.info(28) == 0 and s.ctx.info(77) == _lib.FORM_ROTATIONAL   # P1 through the generic kernels
    prm = T.Params(dt, rho, mu, (0.0, 0.0))
    pb = RT.Problem(ETYPE["P1"], m.x, m.cells, m.facet_cells, m.facet_local, prm)
    pb.set_pressure_boundaries([left, right], [p_in / 2, p_out / 2], 100.0)
    wn = facet_node_set(m, walls)
    pb.add_bc_u(wn, np.zeros((len(wn), 2)))
    x, un = np.zeros(3 * nv), np.zeros((nv, 2))
    for _ in range(3):
        s.solveStep()
        s.advance()
        x, _ = pb.newton(x, un)
        un = x[: 2 * nv].reshape(-1, 2).copy()
    xg = np.concatenate([np.asarray(s.u_sol.x.array), np.asarray(s.p_sol.x.array)])
    assert np.abs(xg - x).max() <= 1e-8 * np.abs(x).max()
    assert abs(s.functional(7, 3) - pb.flux(x, right)) <= 1e-10 * pb.flux(x, right)


def test_vascular_outlet_sequence_matches_the_twin(tmp_path):
    """stabilized_schur_vascularbc on the small stenosis: five steps of the fixed point p_out = R |Q| against the twin's loop;
    the first step runs with initial_ffr * p_inlet / 2; FFR of the final field in (0, 1)."""
    from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
    R, ffr0 = 0.5, 0.8
    sc = StenosisSimulation("stabilized_schur_vascularbc", 0.01, 0.045, ny=6, L=12.0, x_sten=5.0, p_inlet=1.0, R_resistance=R,
                            initial_ffr=ffr0, quiet=True, options=dict(snes_rtol=1e-12, snes_stol=0.0, ksp_rtol=1e-10))
    s = sc.solver
    assert s._p_inlet_val == MMHG / 2 and s._p_outlet_val == ffr0 * MMHG / 2
    sc.solve(str(tmp_path))
    assert sc.num_steps == 5 and len(s.outlet_history) == 5
    m, ft = stenosis_nodes("P1", 6)
    nv = m.num_vertices
    prm = T.Params(0.01, 1.06e-3, 3.5e-3, (0.0, 0.0))
    pb = RT.Problem(ETYPE["P1"], m.x, m.cells, m.facet_cells, m.facet_local, prm)
    wn = facet_node_set(m, ft.find(4))
    pb.add_bc_u(wn, np.zeros((len(wn), 2)))
    x, un, p_out = np.zeros(3 * nv), np.zeros((nv, 2)), ffr0 * MMHG
    for step in range(5):
        pb.set_pressure_boundaries([ft.find(2), ft.find(3)], [MMHG / 2, p_out / 2], 100.0)
        x, _ = pb.newton(x, un)
        un = x[: 2 * nv].reshape(-1, 2).copy()
        q = pb.flux(x, ft.find(3))
        p_out = R * abs(q)
        qg, pg = s.outlet_history[step]
        assert abs(qg - q) <= 1e-8 * abs(q) and abs(pg - p_out) <= 1e-8 * p_out, step
    xg = np.concatenate([np.asarray(s.u_sol.x.array), np.asarray(s.p_sol.x.array)])
    assert np.abs(xg - x).max() <= 1e-8 * np.abs(x).max()
    assert 0.0 < sc.ffr < 1.0 and os.path.exists(tmp_path / "ffr.txt")


def test_pressurebc_stenosis_run_writes_ffr(tmp_path):
    from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
    sc = StenosisSimulation("stabilized_schur_pressurebc", 0.01, 0.025, ny=6, L=12.0, x_sten=5.0, p_inlet=1.0, p_outlet=0.8, quiet=True)
    assert sc.solver._p_inlet_val == MMHG / 2 and sc.solver._p_outlet_val == 0.8 * MMHG / 2
    sc.solve(str(tmp_path))
    assert sc.num_steps == 3 and 0.0 < sc.ffr < 1.0 and os.path.exists(tmp_path / "ffr.txt")
    assert sc.solver.functional(7, 3) > 0


def test_unsupported_combinations_are_refused():
    m = node_mesh("P1", 4)
    fm = np.zeros(m.num_facets, dtype=np.int32)
    # closed-form P1 path
    c0 = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, fm)
    with pytest.raises(ValueError, match="CFDH_ELEM_P1_GENERIC"):
        c0.set_formulation(_lib.FORM_ROTATIONAL)
    c0.close()
    c = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, fm, etype=3)
    with pytest.raises(ValueError, match="rotational formulation"):
        c.set_pressure_boundaries([1], [1.0], 10.0)   # convective form
    c.set_boundary_terms(False, 1, 0.2)
    with pytest.raises(ValueError, match="backflow"):
        c.set_formulation(_lib.FORM_ROTATIONAL)
    c.set_boundary_terms(False, -1, 0.0)
    c.set_formulation(_lib.FORM_ROTATIONAL)
    with pytest.raises(ValueError, match="backflow"):
        c.set_boundary_terms(False, 1, 0.2)
    c.set_pressure_boundaries([1], [1.0], 10.0)
    with pytest.raises(ValueError, match="pressure boundaries are set"):
        c.set_formulation(_lib.FORM_CONVECTIVE)
    with pytest.raises(ValueError):
        c.set_formulation(5)
    c.close()
    # gdim 3
    from cfd_hemodynamic_amd.mesh3d import create_unit_cube
    m3 = create_unit_cube(2)
    c3 = _lib.Context(m3.x, m3.cells, m3.facet_cells, m3.facet_local, m3.facet_marker, etype=3)
    with pytest.raises(ValueError, match="gdim 2"):
        c3.set_formulation(_lib.FORM_ROTATIONAL)
    c3.close()
    # one part of a partitioned run (owned nodes first, the last one a ghost)
    cp = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, fm, nv_owned=m.num_vertices - 1, etype=3)
    with pytest.raises(ValueError, match="partitioned"):
        cp.set_formulation(_lib.FORM_ROTATIONAL)
    cp.close()
