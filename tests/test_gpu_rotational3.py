"""The rotational form of the pressure-driven solvers in 3-D on the GPU (gen3_asm_kernel<ET, JAC, true> and
gen3_facet_kernel<ET, true>, csrc/cfdh_gen3.hip) against the NumPy twin (tests/rot_twin3.py) on Q1 hexahedra and P2 tetrahedra:
assembly, reproducibility, the value-only boundary update, time steps, and the plugins `stabilized_schur_pressurebc` /
`stabilized_schur_vascularbc` on `unit_cube_pipe` (the reference's src/scenarios/unit_cube_pipe.py)."""
import numpy as np
import pytest

from cfd_hemodynamic_amd import _lib
from gen3_util import ETYPE3, LIB_ETYPE3, facet_node_set3, node_mesh3
from oracle import np_twin_nd as TN
import rot_twin3 as RT3
from test_rot_twin3 import duct, ends3

pytestmark = pytest.mark.gpu


def _pair(kind, m, prm, sets, values, beta, markers_ids=(2, 3)):
    """Twin and context with the same mesh, parameters and pressure boundaries (facet sets -> markers 2, 3)."""
    pb = RT3.Problem(ETYPE3[kind], m.x, m.cells, m.facet_cells, m.facet_local, prm)
    pb.set_pressure_boundaries(sets, values, beta)
    markers = np.zeros(m.num_facets, dtype=np.int32)
    for mk, fs in zip(markers_ids, sets):
        markers[fs] = mk
    ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, markers, etype=LIB_ETYPE3[kind])
    ctx.set_params(prm.dt, prm.rho, prm.mu, f=prm.f)
    ctx.set_time_scheme(prm.theta, prm.a0, prm.a1, prm.a2)
    ctx.set_boundary_terms(ds_terms=False)
    ctx.set_formulation(_lib.FORM_ROTATIONAL)
    ctx.set_pressure_boundaries(list(markers_ids[: len(sets)]), values, beta)
    return pb, ctx


@pytest.mark.parametrize("kind", ["P2", "Q1"])
@pytest.mark.parametrize("scheme", [dict(), dict(theta=1.0, a0=1.5, a1=-2.0, a2=0.5)])
def test_assembly_matches_the_twin(kind, scheme):
    """Distorted cells, two pressure boundaries with different values, random Dirichlet data on part of the walls, random state
    and history: the residual and every CSR block agree to 1e-12; the residual-only pass gives the same bits."""
    rng = np.random.default_rng(5)
    m = node_mesh3(kind, 2 if kind == "P2" else 3, distort=0.05)
    nv = m.num_vertices
    prm = TN.Params(0.02, 1.3, 0.04, (0.2, -0.1, 0.3), **scheme)
    left, right, walls = ends3(m, kind, 0.05)
    pb, ctx = _pair(kind, m, prm, [left, right], [1.7, -0.4], 30.0)
    wn = facet_node_set3(m, walls)[::2]
    vals = rng.standard_normal((len(wn), 3))
    pb.add_bc_u(wn, vals)
    ctx.add_dirichlet(0, wn, vals)
    xv, un, un2 = 0.3 * rng.standard_normal(4 * nv), 0.3 * rng.standard_normal((nv, 3)), 0.3 * rng.standard_normal((nv, 3))
    F, J = pb.assemble(xv, un, un2=un2)
    ctx.set_state(u_prev=un.ravel(), p_prev=np.zeros(nv), u=xv[: 3 * nv], p=xv[3 * nv:])
    ctx.set_previous2(un2.ravel())
    ctx.assemble(True)
    Fg = np.concatenate(ctx.get_residual())
    Jg = ctx.get_csr()
    assert np.abs(Fg - F).max() <= 1e-12 * np.abs(F).max()
    assert abs(Jg - J).max() <= 1e-12 * abs(J).max()
    y = rng.standard_normal(4 * nv)
    assert np.abs(ctx.spmv(y) - J @ y).max() <= 1e-12 * np.abs(J @ y).max()
    ctx.assemble(False)
    assert np.array_equal(np.concatenate(ctx.get_residual()), Fg)
    assert ctx.info(77) == _lib.FORM_ROTATIONAL
    ctx.close()


@pytest.mark.parametrize("kind", ["P2", "Q1"])
def test_rotational_assembly_is_bitwise_reproducible(kind):
    rng = np.random.default_rng(12)
    m = node_mesh3(kind, 3, distort=0.05)
    nv = m.num_vertices
    prm = TN.Params(0.02, 1.3, 0.04, (0.2, -0.1, 0.3))
    left, right, walls = ends3(m, kind, 0.05)
    wn = facet_node_set3(m, walls)
    xv, un = 0.3 * rng.standard_normal(4 * nv), 0.3 * rng.standard_normal((nv, 3))
    out = []
    for _ in range(2):
        _, ctx = _pair(kind, m, prm, [left, right], [1.7, -0.4], 30.0)
        ctx.add_dirichlet(0, wn, np.zeros((len(wn), 3)))
        ctx.set_state(u_prev=un.ravel(), p_prev=np.zeros(nv), u=xv[: 3 * nv], p=xv[3 * nv:])
        for _rep in range(2):
            ctx.assemble(True)
            out.append((np.concatenate(ctx.get_residual()), ctx.get_csr().data.copy()))
        ctx.close()
    for F, A in out[1:]:
        assert np.array_equal(F, out[0][0]) and np.array_equal(A, out[0][1])


def test_value_only_update_keeps_jacobian_and_preconditioner():
    """New VALUES of the pressure boundaries leave the Jacobian (bit for bit) and the preconditioner valid, and the residual equals
    that of a fresh context created with the new values; a marker change invalidates both."""
    m = duct("Q1", 4, 2, 1.0)
    nv = m.num_vertices
    prm = TN.Params(0.01, 1.0, 0.05, (0.0, 0.0, 0.0))
    left, right, walls = ends3(m)
    wn = facet_node_set3(m, walls)
    _, ctx = _pair("Q1", m, prm, [left, right], [4.0, 1.0], 100.0)
    ctx.add_dirichlet(0, wn, np.zeros((len(wn), 3)))
    z3, z1 = np.zeros(3 * nv), np.zeros(nv)
    ctx.set_state(u_prev=z3, p_prev=z1, u=z3, p=z1)
    ctx.solve_step()
    assert ctx.info(75) == 1 and ctx.info(76) == 0
    builds = ctx.info(74)
    u, p = ctx.get_solution()
    ctx.assemble(True)
    J0 = ctx.get_csr().data.copy()
    ctx.set_pressure_boundaries([2, 3], [4.0, 2.5], 100.0)   # value only
    assert ctx.info(75) == 1 and np.array_equal(ctx.get_csr().data, J0)
    ctx.assemble(True)
    F1 = np.concatenate(ctx.get_residual())
    assert np.array_equal(ctx.get_csr().data, J0) and ctx.info(75) == 1 and ctx.info(74) == builds
    _, fresh = _pair("Q1", m, prm, [left, right], [4.0, 2.5], 100.0)
    fresh.add_dirichlet(0, wn, np.zeros((len(wn), 3)))
    fresh.set_state(u_prev=z3, p_prev=z1, u=u, p=p)
    fresh.assemble(True)
    assert np.array_equal(np.concatenate(fresh.get_residual()), F1)
    fresh.close()
    ctx.set_pressure_boundaries([3, 2], [2.5, 4.0], 100.0)   # markers in another order: a rebuild
    assert ctx.info(75) == 0
    ctx.close()


@pytest.mark.parametrize("kind", ["P2", "Q1"])
def test_time_steps_on_a_duct_match_the_twin(kind):
    """Three midpoint steps, walls no-slip, natural pressures on both ends: device Newton + FGMRES vs the twin's direct Newton."""
    m = duct(kind, 3, 2, 0.75)
    nv = m.num_vertices
    prm = TN.Params(0.02, 1.0, 0.05, (0.0, 0.0, 0.0))
    left, right, walls = ends3(m)
    pb, ctx = _pair(kind, m, prm, [left, right], [2.0, 0.5], 100.0)
    wn = facet_node_set3(m, walls)
    pb.add_bc_u(wn, np.zeros((len(wn), 3)))
    ctx.add_dirichlet(0, wn, np.zeros((len(wn), 3)))
    o = ctx.default_options()
    o.snes_rtol, o.snes_stol, o.ksp_rtol = 1e-12, 0.0, 1e-10
    ctx.set_options(o)
    x = np.zeros(4 * nv)
    ctx.set_state(u_prev=x[: 3 * nv], p_prev=x[3 * nv:], u=x[: 3 * nv], p=x[3 * nv:])
    un = np.zeros((nv, 3))
    for step in range(3):
        st = ctx.solve_step()
        assert st.reason > 0 and ctx.info(76) == 0
        u, p = ctx.get_solution()
        ctx.advance()
        x, _ = pb.newton(x, un)
        un = x[: 3 * nv].reshape(-1, 3).copy()
        assert np.abs(u - x[: 3 * nv]).max() <= 1e-8 * np.abs(x[: 3 * nv]).max(), step
        assert np.abs(p - x[3 * nv:]).max() <= 1e-7 * np.abs(x[3 * nv:]).max(), step
    assert pb.flux(x, right) > 0   # down the pressure drop
    ctx.close()


_PIPE = dict(nx=12, ny=2, nz=2, L=6.0, quiet=True)


def test_vascular_outlet_sequence_matches_the_twin(tmp_path):
    """stabilized_schur_vascularbc on a short unit_cube_pipe (hexahedra): five steps of the fixed point p_out = R |Q| against the
    twin's loop; the first step runs with initial_ffr * p_inlet / 2."""
    from cfd_hemodynamic_amd.scenarios.unit_cube_pipe import UnitCubePipeSimulation
    R, ffr0, p_in, dt = 2.0, 0.8, 8.85, 0.01
    sc = UnitCubePipeSimulation("stabilized_schur_vascularbc", dt, 0.045, p_inlet=p_in, p_outlet=0.0, R_resistance=R, initial_ffr=ffr0,
                                options=dict(snes_rtol=1e-12, snes_stol=0.0, ksp_rtol=1e-10), **_PIPE)
    s = sc.solver
    assert s.ctx.info(28) == 2 and s.ctx.info(77) == _lib.FORM_ROTATIONAL
    sc.solve(str(tmp_path))
    assert sc.num_steps == 5 and len(s.outlet_history) == 5
    m, ft = sc.mesh, sc._ft
    nv = m.num_vertices
    prm = TN.Params(dt, 1.06e-3, 3.5e-3, (0.0, 0.0, 0.0))
    pb = RT3.Problem(ETYPE3["Q1"], m.x, m.cells, m.facet_cells, m.facet_local, prm)
    wn = facet_node_set3(m, ft.find(3))
    pb.add_bc_u(wn, np.zeros((len(wn), 3)))
    x, un, p_out = np.zeros(4 * nv), np.zeros((nv, 3)), ffr0 * p_in
    for step in range(5):
        pb.set_pressure_boundaries([ft.find(1), ft.find(2)], [p_in / 2, p_out / 2], 100.0)
        x, _ = pb.newton(x, un)
        un = x[: 3 * nv].reshape(-1, 3).copy()
        q = pb.flux(x, ft.find(2))
        p_out = R * abs(q)
        qg, pg = s.outlet_history[step]
        assert abs(qg - q) <= 1e-8 * abs(q) and abs(pg - p_out) <= 1e-8 * p_out, step
    xg = np.concatenate([np.asarray(s.u_sol.x.array), np.asarray(s.p_sol.x.array)])
    assert np.abs(xg - x).max() <= 1e-8 * np.abs(x).max()


@pytest.mark.parametrize("solver", ["stabilized_schur_pressurebc", "stabilized_schur_vascularbc"])
@pytest.mark.parametrize("cell", [dict(), dict(cell_type="tetrahedron", p_grade=2)])
def test_unit_cube_pipe_runs_through_the_plugins(tmp_path, solver, cell):
    """unit_cube_pipe through Scenario.solve on hexahedra and on P2 tetrahedra: converged steps, inflow = outflow, flow from the
    high to the low pressure."""
    from cfd_hemodynamic_amd.scenarios.unit_cube_pipe import UnitCubePipeSimulation
    extra = dict(R_resistance=0.5) if solver.endswith("vascularbc") else {}
    sc = UnitCubePipeSimulation(solver, 0.01, 0.025, p_inlet=8.85, p_outlet=0.0, options=dict(snes_rtol=1e-12, snes_stol=0.0, ksp_rtol=1e-10),
                                **_PIPE, **cell, **extra)
    s = sc.solver
    assert s.ctx.info(28) == (1 if cell else 2) and s.ctx.info(77) == _lib.FORM_ROTATIONAL
    sc.solve(str(tmp_path))
    assert sc.num_steps == 3
    q_in, q_out = -s.functional(7, sc.inlet_marker), s.functional(7, sc.outlet_marker)
    assert q_out > 0 and abs(q_in - q_out) <= 1e-8 * q_out
