"""Traction boundaries of the convective form on the closed-form P1 kernels (cfdh_set_traction_boundaries, csrc/cfdh_traction.hip)
against their NumPy twin (tests/trac_twin.py): assembly (residual, every CSR value, SpMV) at states violating the Dirichlet data,
repeatability, the value-only update, refusals, the flux of u_prev, one time step against the twin's Newton step, and the two
plugins through their scenarios.  fp64; bounds of the neighbouring closed-form tests (tests/test_gpu_3d.py)."""
import numpy as np
import pytest

from cfd_hemodynamic_amd import _lib
from oracle import np_twin_nd as TN
import trac_twin as TT
import trac_util as U

pytestmark = pytest.mark.gpu

BDF2 = dict(theta=1.0, a0=1.5, a1=-2.0, a2=0.5)
F3 = (0.2, -0.1, 0.3)


def _mesh(d):
    """4 x 3 unit square / the 4 x 3 cube of tests/test_gpu_3d.py::_cube, with inlet, outlet and wall markers; one cell has an
    outlet facet and an inlet facet."""
    mesh, rng = U.square(4, 3, 3) if d == 2 else U.cube(4, 3)
    return mesh, U.mark_ends(mesh), rng


def _pair(d, scheme=None, dt=0.02, rho=1.3, mu=0.04, f=F3):
    """Twin and context with Dirichlet walls (one object on all wall vertices, a second one on a few of them: multiplicity 2)."""
    scheme = scheme or {}
    mesh, marker, rng = _mesh(d)
    prm = TN.Params(dt, rho, mu, f, ds_terms=False, **scheme)
    pb = TT.Problem(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, prm)
    ctx = _lib.Context(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, marker)
    assert ctx.dim == d and ctx.info(28) == 0
    ctx.set_params(dt, rho, mu, f=f[:d] if d == 2 else f)
    ctx.set_boundary_terms(False)
    if scheme:
        ctx.set_time_scheme(scheme["theta"], scheme["a0"], scheme["a1"], scheme["a2"])
    wn = U.wall_nodes(mesh, marker)
    for nodes in (wn, wn[:3]):
        vals = rng.standard_normal((len(nodes), d))
        pb.add_bc_u(nodes, vals)
        ctx.add_dirichlet(0, nodes, vals)
    return mesh, marker, rng, pb, ctx


def _state(mesh, rng, ctx, d, scheme):
    nv = mesh.num_vertices
    xv = 0.3 * rng.standard_normal((d + 1) * nv)
    un, un2 = 0.3 * rng.standard_normal((nv, d)), 0.3 * rng.standard_normal((nv, d))
    ctx.set_state(u_prev=un.ravel(), p_prev=np.zeros(nv), u=xv[: d * nv], p=xv[d * nv:])
    if scheme:
        ctx.set_previous2(un2.ravel())
    return xv, un, un2


def _both_signs_on(pb, un, facets):
    d = pb.d
    fc, fl = pb.facet_cells[facets], pb.facet_local[facets]
    g, _, _ = TN.geometry(pb.x, pb.cells[fc])
    s = np.einsum("cai,ci->ca", un[pb.cells[fc]], -g[np.arange(len(fc)), fl])
    s = np.array([s[k, a] for k in range(len(fc)) for a in range(d + 1) if a != fl[k]])
    return s.min() < 0 < s.max()


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("scheme", [{}, BDF2])
@pytest.mark.parametrize("tangential", [(1, 0), (0, 1)])
@pytest.mark.parametrize("bf", [0.0, 0.4])
def test_assembly_and_spmv_match_twin(d, scheme, tangential, bf):
    mesh, marker, rng, pb, ctx = _pair(d, scheme)
    nv = mesh.num_vertices
    inl, out, _ = U.sets_of(marker)
    cells_in, cells_out = set(mesh.facet_cells[inl].tolist()), set(mesh.facet_cells[out].tolist())
    assert cells_in & cells_out                                  # one cell with two traction facets
    xv, un, un2 = _state(mesh, rng, ctx, d, scheme)
    assert _both_signs_on(pb, un, out)                           # (u_prev . n)_- is active on part of the outlet
    args = dict(tangential=list(tangential), beta_backflow=[0.0, bf])
    pb.set_traction_boundaries([inl, out], [1.7, -0.4], beta=30.0, **args)
    ctx.set_traction_boundaries([U.INLET, U.OUTLET], [1.7, -0.4], 30.0, **args)
    assert ctx.info(93) == 2
    F, J = pb.assemble(xv, un, un2=un2)
    F0 = TN.Problem.assemble(pb, xv, un, un2=un2)[0]            # the same without the boundary terms
    assert np.abs(F - F0).max() > 1e-3 * np.abs(F).max()
    ctx.assemble(True)
    Fg = np.concatenate(ctx.get_residual())
    assert np.abs(F - Fg).max() <= 1e-12 * np.abs(F).max()
    Jg = ctx.get_csr()
    assert abs(J - Jg).max() <= 1e-12 * abs(J).max()
    v = rng.standard_normal((d + 1) * nv)
    assert np.abs(ctx.spmv(v) - J @ v).max() <= 1e-12 * np.abs(J @ v).max()
    ctx.assemble(False)                                          # mode 2: residual with lifting, no Jacobian write
    assert np.abs(np.concatenate(ctx.get_residual()) - F).max() <= 1e-12 * np.abs(F).max()
    assert ctx.info(94) == 2
    ctx.close()


@pytest.mark.parametrize("d", [2, 3])
def test_residual_without_lifting_matches_twin(d):
    """A state that meets the Dirichlet data: nothing is lifted, the residual-only assembly equals the twin's want_jac=False
    path (where the kernel's modes 0 and 2 coincide; the library itself only ever asks for modes 1 and 2)."""
    mesh, marker, rng, pb, ctx = _pair(d)
    nv = mesh.num_vertices
    inl, out, _ = U.sets_of(marker)
    xv, un, _ = _state(mesh, rng, ctx, d, {})
    xv[pb.isbc] = pb.bcval[pb.isbc]
    ctx.set_state(u=xv[: d * nv], p=xv[d * nv:])
    pb.set_traction_boundaries([inl, out], [1.7, -0.4], beta=30.0, tangential=[1, 0], beta_backflow=[0.0, 0.4])
    ctx.set_traction_boundaries([U.INLET, U.OUTLET], [1.7, -0.4], 30.0, tangential=[1, 0], beta_backflow=[0.0, 0.4])
    F = pb.assemble(xv, un, want_jac=False)[0]
    ctx.assemble(False)
    assert np.abs(np.concatenate(ctx.get_residual()) - F).max() <= 1e-12 * np.abs(F).max()
    ctx.close()


@pytest.mark.parametrize("d", [2, 3])
def test_two_assemblies_give_identical_bits_and_values_change_the_residual_only(d):
    mesh, marker, rng, pb, ctx = _pair(d)
    inl, out, _ = U.sets_of(marker)
    xv, un, _ = _state(mesh, rng, ctx, d, {})
    kw = dict(tangential=[1, 0], beta_backflow=[0.0, 0.4])
    ctx.set_traction_boundaries([U.INLET, U.OUTLET], [1.7, -0.4], 30.0, **kw)
    ctx.assemble(True)
    F1, J1 = np.concatenate(ctx.get_residual()), ctx.get_csr()
    ctx.assemble(True)
    F2, J2 = np.concatenate(ctx.get_residual()), ctx.get_csr()
    assert np.array_equal(F1, F2) and np.array_equal(J1.data, J2.data) and np.array_equal(J1.indices, J2.indices)
    # a value-only update keeps the preconditioner and moves F by exactly the twin's difference
    o = ctx.default_options()
    ctx.set_options(o)
    ctx.apply_preconditioner(np.ones((d + 1) * mesh.num_vertices))
    assert ctx.info(75) == 1
    builds = ctx.info(74)
    ctx.set_traction_boundaries([U.INLET, U.OUTLET], [0.3, 2.5], 30.0, **kw)
    assert ctx.info(75) == 1 and ctx.info(74) == builds
    ctx.assemble(True)
    F3_, J3 = np.concatenate(ctx.get_residual()), ctx.get_csr()
    assert np.array_equal(J3.data, J1.data)
    pb.set_traction_boundaries([inl, out], [1.7, -0.4], beta=30.0, **kw)
    Fa = pb.assemble(xv, un)[0]
    pb.set_traction_boundaries([inl, out], [0.3, 2.5], beta=30.0, **kw)
    Fb = pb.assemble(xv, un)[0]
    assert np.abs(Fb - Fa).max() > 0
    assert np.abs((F3_ - F1) - (Fb - Fa)).max() <= 1e-12 * np.abs(Fa).max()
    # any other change invalidates the preconditioner; so does a marker change while boundaries are set
    ctx.set_traction_boundaries([U.INLET, U.OUTLET], [0.3, 2.5], 30.0, tangential=[1, 0], beta_backflow=[0.0, 0.1])
    assert ctx.info(75) == 0
    with pytest.raises(_lib.CfdhError, match="no Jacobian"):             # ... and the Jacobian
        ctx.apply_preconditioner(np.ones((d + 1) * mesh.num_vertices))
    ctx.assemble(True)
    ctx.apply_preconditioner(np.ones((d + 1) * mesh.num_vertices))
    assert ctx.info(75) == 1
    ctx.set_facet_markers(marker)
    assert ctx.info(75) == 0
    # n = 0 removes the terms: the parent's residual again
    ctx.set_traction_boundaries([], [])
    assert ctx.info(93) == 0
    ctx.assemble(True)
    F0 = TN.Problem.assemble(pb, xv, un)[0]
    assert np.abs(np.concatenate(ctx.get_residual()) - F0).max() <= 1e-12 * np.abs(F0).max()
    ctx.close()


def test_refusals_leave_the_context_usable():
    mesh, marker, rng, pb, ctx = _pair(2)
    xv, un, _ = _state(mesh, rng, ctx, 2, {})
    ok = ([U.INLET, U.OUTLET], [1.0, 0.0], 30.0)
    for bad, pat in [(([1, 1], [1.0, 0.0], 30.0), "twice"), (([1, 2], [np.nan, 0.0], 30.0), "finite"),
                     (([1, 2], [1.0, 0.0], -1.0), "beta_nitsche"), (([1, 2], [1.0, 0.0], np.inf), "beta_nitsche"),
                     ((list(range(9)), [0.0] * 9, 1.0), "n <= 8")]:
        with pytest.raises(ValueError, match=pat):
            ctx.set_traction_boundaries(*bad)
    with pytest.raises(ValueError, match="beta_backflow"):
        ctx.set_traction_boundaries(*ok, beta_backflow=[0.0, -0.1])
    with pytest.raises(ValueError, match="beta_backflow"):
        ctx.set_traction_boundaries(*ok, beta_backflow=[0.0, np.nan])
    ctx.set_boundary_terms(True)
    with pytest.raises(ValueError, match="ds_terms"):
        ctx.set_traction_boundaries(*ok)
    ctx.set_boundary_terms(False, U.OUTLET, 0.2)
    with pytest.raises(ValueError, match="backflow"):
        ctx.set_traction_boundaries(*ok)
    ctx.set_boundary_terms(False)
    with pytest.raises(ValueError, match="generic"):                     # still refused on closed-form contexts
        ctx.set_pressure_boundaries([U.INLET], [1.0], 10.0)
    assert ctx.info(93) == 0
    ctx.set_traction_boundaries(*ok)
    with pytest.raises(ValueError, match="traction"):
        ctx.set_boundary_terms(True)
    with pytest.raises(ValueError, match="traction"):
        ctx.set_boundary_terms(False, U.OUTLET, 0.2)
    with pytest.raises(ValueError, match="traction"):
        ctx.set_formulation(_lib.FORM_ROTATIONAL)
    ctx.set_boundary_terms(False)                                        # unchanged settings stay allowed
    # the context still assembles what the twin does
    inl, out, _ = U.sets_of(marker)
    pb.set_traction_boundaries([inl, out], [1.0, 0.0], beta=30.0)
    F = pb.assemble(xv, un)[0]
    ctx.assemble(True)
    assert np.abs(np.concatenate(ctx.get_residual()) - F).max() <= 1e-12 * np.abs(F).max()
    ctx.close()
    # generic-element contexts (convective and rotational form), a part of a partitioned run, a pressure-correction context
    g = _lib.Context(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, marker, etype=3)
    g.set_boundary_terms(False)
    with pytest.raises(ValueError, match="closed-form"):
        g.set_traction_boundaries(*ok)
    g.set_formulation(_lib.FORM_ROTATIONAL)
    with pytest.raises(ValueError):
        g.set_traction_boundaries(*ok)
    g.close()
    part = _lib.Context(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, marker, nv_owned=mesh.num_vertices - 1)
    part.set_boundary_terms(False)
    with pytest.raises(ValueError, match="partitioned"):
        part.set_traction_boundaries(*ok)
    part.close()
    from cfd_hemodynamic_amd.elements import NodeMesh
    nm = NodeMesh(mesh)
    ipcs = _lib.IpcsContext(nm.x, nm.cells, mesh.num_vertices, nm.facet_cells, nm.facet_local, np.zeros(len(nm.facet_cells), dtype=np.int32))
    with pytest.raises(ValueError, match="pressure-correction"):
        ipcs.set_traction_boundaries(*ok)
    ipcs.close()


@pytest.mark.parametrize("d", [2, 3])
def test_flux_of_u_prev_is_functional_8(d):
    mesh, marker, rng, pb, ctx = _pair(d)
    _, out, _ = U.sets_of(marker)
    xv, un, _ = _state(mesh, rng, ctx, d, {})
    q = pb.flux_prev(un, out)
    assert abs(ctx.functional(8, U.OUTLET) - q) <= 1e-12 * np.abs(un).max()
    assert abs(ctx.functional(7, U.OUTLET) - pb.flux(xv, out)) <= 1e-12 * np.abs(xv).max()
    assert abs(ctx.functional(7, U.OUTLET) - ctx.functional(8, U.OUTLET)) > 1e-3
    u, p = ctx.get_solution()                                            # the iterate is where it was
    assert np.array_equal(np.concatenate([u, p]), xv)
    ctx.close()


def _step_case(d):
    if d == 2:
        from util import stenosis_case
        case = stenosis_case(6)
        mesh, marker = case.mesh, case.mesh.facet_marker.copy()
        tags = (2, 3, 4)
        par = dict(dt=case.dt, rho=case.rho, mu=case.mu, f=(0.0, 0.0, 0.0))
        values = [5.0, 0.3]
    else:
        mesh = U.duct(6, 2, 3.0)
        marker = U.mark_ends(mesh, corner=False)
        tags = (U.INLET, U.OUTLET, U.WALL)
        par = dict(dt=0.01, rho=1.0, mu=0.05, f=(0.0, 0.0, 0.0))
        values = [1.0, 0.05]
    return mesh, marker, tags, par, values


@pytest.mark.parametrize("d", [2, 3])
def test_time_step_matches_the_twins_newton_step(d):
    """Walls no-slip, weak pressure inlet with the tangential terms, traction outlet with backflow stabilisation, from rest: one
    step, both sides converged tightly (twin: Newton with a direct solve), the Jacobian found non-singular."""
    mesh, marker, (t_in, t_out, t_wall), par, values = _step_case(d)
    nv = mesh.num_vertices
    inl, out, wall = [np.nonzero(marker == t)[0] for t in (t_in, t_out, t_wall)]
    prm = TN.Params(par["dt"], par["rho"], par["mu"], par["f"], ds_terms=False)
    pb = TT.Problem(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, prm)
    ctx = _lib.Context(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, marker)
    ctx.set_params(par["dt"], par["rho"], par["mu"], f=par["f"][:d] if d == 2 else par["f"])
    ctx.set_boundary_terms(False)
    wn = np.unique(np.asarray(mesh.facet_vertices)[wall]).astype(np.int32)
    pb.add_bc_u(wn, np.zeros((len(wn), d)))
    ctx.add_dirichlet(0, wn, np.zeros((len(wn), d)))
    kw = dict(tangential=[1, 0], beta_backflow=[0.0, 0.2])
    pb.set_traction_boundaries([inl, out], values, beta=100.0, **kw)
    ctx.set_traction_boundaries([t_in, t_out], values, 100.0, **kw)
    o = ctx.default_options()
    o.snes_rtol, o.snes_stol, o.ksp_rtol = 1e-12, 0.0, 1e-10
    ctx.set_options(o)
    z = np.zeros(d * nv)
    ctx.set_state(u_prev=z, p_prev=np.zeros(nv), u=z, p=np.zeros(nv))
    st = ctx.solve_step()
    print("traction step d=%d: newton %d, krylov %d, reason %d" % (d, st.newton_its, st.krylov_its, st.reason))
    assert st.reason > 0 and ctx.info(76) == 0
    xg = np.concatenate(ctx.get_solution())
    x, _ = pb.newton(np.zeros((d + 1) * nv), np.zeros((nv, d)))
    assert np.linalg.norm(xg[: d * nv] - x[: d * nv]) <= 1e-8 * np.linalg.norm(x[: d * nv])
    assert np.linalg.norm(xg[d * nv:] - x[d * nv:]) <= 1e-7 * np.linalg.norm(x[d * nv:])
    assert pb.flux(x, out) > 0 and abs(ctx.functional(7, t_out) - pb.flux(x, out)) <= 1e-7 * pb.flux(x, out)
    assert ctx.info(94) > 0
    ctx.close()


def test_a_context_without_traction_boundaries_never_launches_the_kernel():
    from util import make_ctx, stenosis_case
    case = stenosis_case(6)
    ctx = make_ctx(case)
    z = np.zeros(2 * case.nv)
    ctx.set_state(u_prev=z, p_prev=np.zeros(case.nv), u=z, p=np.zeros(case.nv))
    st = ctx.solve_step()
    assert st.reason > 0 and ctx.info(93) == 0 and ctx.info(94) == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------ the plugins through scenarios
def _check_run(sc, n_boundaries):
    """Three steps: the recorded (Q(u_prev), p_c) pairs follow the damped rule from the recorded fluxes, the flow leaves through the
    outlet, the norms are finite, the context is closed-form P1 with the traction boundaries set."""
    from cfd_hemodynamic_amd.solvers.stabilized_schur_pressure_backflow import damped_outlet_pressure
    s = sc.solver
    assert sc.num_steps == 3 and len(s.outlet_history) == 3
    p = s.p_c_initial
    for Q, p_c in s.outlet_history:
        p = damped_outlet_pressure(p, Q, s.R_resistance, s.alpha_damping)
        assert abs(p_c - p) <= 1e-14 * abs(p), (p_c, p)
    print("outlet history:", s.p_c_initial, s.outlet_history, "newton/krylov of the last step:", s.last_stats.newton_its, s.last_stats.krylov_its)
    assert s.outlet_history[-1][0] > 0 and s.ctx.functional(7, sc.outlet_marker) > 0
    assert np.isfinite(sc.norm_v) and np.isfinite(sc.norm_p) and sc.norm_v > 0
    assert s.ctx.info(28) == 0 and s.ctx.info(93) == n_boundaries and s.ctx.info(76) == 0 and s.ctx.info(94) > 0


def test_stenosis_pressure_scenario(tmp_path):
    from cfd_hemodynamic_amd.scenarios.stenosis_pressure import _MMHG_2D, StenosisPressureSimulation
    sc = StenosisPressureSimulation("stabilized_schur_pressure_backflow", 0.01, 0.025, p_inlet=1.0, R_resistance=0.01, ny=8, quiet=True)
    s = sc.solver
    assert s.p_inlet == _MMHG_2D and len(sc.bcu) == 1 and sc.bcp == [] and s.p_c_initial == 0.0
    sc.solve(str(tmp_path), device_resident=False, write_every=0)
    _check_run(sc, 2)
    assert np.isfinite(sc.ffr)


def test_unit_cube_pipe_scenario_on_p1_tetrahedra(tmp_path):
    from cfd_hemodynamic_amd.scenarios.unit_cube_pipe import UnitCubePipeSimulation
    kw = dict(p_inlet=50.0, p_outlet=0.0, R_resistance=0.1, nx=12, ny=2, nz=2, cell_type="tetrahedron", p_grade=1)
    sc = UnitCubePipeSimulation("stabilized_schur_pressure_backflow", 0.01, 0.025, quiet=True, **kw)
    assert sc.solver.p_inlet == 50.0 and sc.mesh.topology.cell_name() == "tetrahedron"
    sc.solve(str(tmp_path), write_every=0)
    _check_run(sc, 2)
    # ... and through the command line
    from cfd_hemodynamic_amd.__main__ import main
    argv = ["simulate", "--simulation", "unit_cube_pipe", "--solver", "stabilized_schur_pressure_backflow", "--T", "0.015", "--dt", "0.01",
            "--output_dir", str(tmp_path / "cli"), "--quiet", "True"]
    for k, v in kw.items():
        argv += ["--" + k, str(v)]
    assert main(argv) == 0


def test_simple_bifurcation_scenario_driven_by_pressure(tmp_path):
    from cfd_hemodynamic_amd.scenarios.simple_bifurcation import MicrovasculatureSimulation
    sc = MicrovasculatureSimulation("stabilized_schur_pressure_backflow", 0.01, 0.025, res=8e-4, p_inlet=50.0, R_resistance=1e5, quiet=True)
    assert len(sc.bcu) == 1                                       # walls only: the inlet profile is not imposed
    sc.solve(str(tmp_path), write_every=0)
    _check_run(sc, 2)
    qi, q1, q2 = sc.flow_rates()
    assert qi > 0 and q1 > 0 and q2 > 0
    # other solvers keep the inlet profile
    ref = MicrovasculatureSimulation("stabilized_schur", 0.01, 0.025, res=1.2e-3, quiet=True)
    assert len(ref.bcu) == 2


def test_velocity_inlet_sibling_on_the_stenosis(tmp_path):
    from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
    sc = StenosisSimulation("stabilized_schur_velocity_vascular_backflow", 0.01, 0.025, ny=8, v_max=100.0, R_resistance=0.01, quiet=True)
    s = sc.solver
    assert len(sc.bcu) == 2 and s.p_c_initial == 0.01 * abs(s.ctx.functional(8, 3)) > 0   # the initial velocity carries flow
    sc.solve(str(tmp_path), write_every=0)
    _check_run(sc, 1)
