"""GPU tests of the PCD Schur approximation (pc_type 2) on the degree-1 generic elements in the rotational form
(pcd_k_assemble_gen_kernel, csrc/cfdh_pcd.hip) and of the plugins `stabilized_pcd_pressurebc` / `stabilized_pcd_bdf2`: the operator
against the quadrature twin (tests/pcd_gen_twin.py), the apply pass, one pressure-driven step against the twins of the rotational
form (tests/rot_twin.py, tests/rot_twin3.py), the scenarios, and the error codes.

Meshes: the smallest that span two SELL-64 slices with a ragged tail and mixed row lengths -- the small stenosis (P1 triangles),
9 x 7 quadrilaterals and 4 x 3 x 3 hexahedra (80 nodes each; rows of 8, 12, 18 and 27 entries on the hexahedra).  The Q1
coordinates go through a fixed non-symmetric affine map, so a transposed or inverted Jacobian shows; inlet (2) / outlet (3) are the
unmapped x = 0 / x = max faces, the rest is wall (4)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pcd_gen_twin as PG
import pcd_twin as P
from util import stenosis_case

from cfd_hemodynamic_amd import _lib
from cfd_hemodynamic_amd.elements import create_box, create_rectangle

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MMHG = 133.322
A2 = np.array([[1.3, 0.35], [-0.2, 0.9]])
A3 = np.array([[1.3, 0.35, -0.15], [-0.2, 0.9, 0.25], [0.1, -0.3, 1.1]])
LIB_ETYPE = {"tri": 3, "quad": 2, "hex": 2}   # CFDH_ELEM_P1_GENERIC, CFDH_ELEM_Q1
KINDS = ["tri", "quad", "hex"]
SCHEMES = {"midpoint": (0.5, 1.0, -1.0, 0.0), "implicit15": (1.0, 1.5, -2.0, 0.5)}


def _build(kind):
    if kind == "tri":
        m = stenosis_case(6, L=12.0, x_sten=5.0).mesh
        return m, np.asarray(m.facet_marker, dtype=np.int32).copy()
    if kind == "quad":
        m, xmax = create_rectangle((0.0, 0.0), (1.8, 0.7), (9, 7)), 1.8
    else:
        m, xmax = create_box((0.0, 0.0, 0.0), (1.6, 0.9, 0.6), (4, 3, 3)), 1.6
    fx = m.x[np.asarray(m.facet_vertices)][:, :, 0]
    mk = np.full(len(m.facet_cells), 4, dtype=np.int32)
    mk[np.isclose(fx, 0.0).all(axis=1)] = 2
    mk[np.isclose(fx, xmax).all(axis=1)] = 3
    m.x[:] = m.x @ (A2 if kind == "quad" else A3).T
    assert m.num_vertices == 80
    return m, mk


_MESHES = {}


def _get(kind):
    if kind not in _MESHES:
        _MESHES[kind] = _build(kind)
    return _MESHES[kind]


def _rot_ctx(kind, m, mk, dt, rho, mu, scheme=SCHEMES["midpoint"], etype=None):
    d = m.x.shape[1]
    ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, mk, etype=LIB_ETYPE[kind] if etype is None else etype)
    ctx.set_params(dt, rho, mu, f=np.zeros(d))
    ctx.set_time_scheme(*scheme)
    ctx.set_boundary_terms(ds_terms=False)
    ctx.set_formulation(_lib.FORM_ROTATIONAL)
    return ctx


def _rowrel(K, Kt):
    D = (K - Kt).tocsr()
    rowmax = np.asarray(abs(Kt).max(axis=1).todense()).ravel()
    return (np.asarray(abs(D).max(axis=1).todense()).ravel() / rowmax).max()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scheme", ["midpoint", "implicit15"])
@pytest.mark.parametrize("time_term", [0, 1])
def test_pcd_operator_matches_the_twin(kind, scheme, time_term):
    m, mk = _get(kind)
    d, nv = m.x.shape[1], m.num_vertices
    rng = np.random.default_rng(7)
    u, un, p = rng.standard_normal((nv, d)), rng.standard_normal((nv, d)), rng.standard_normal(nv)
    theta, a0 = SCHEMES[scheme][:2]
    dt, rho, mu = 0.013, 1.06, 3.5e-3

    def ctx_k():
        ctx = _rot_ctx(kind, m, mk, dt, rho, mu, SCHEMES[scheme])
        ctx.set_schur_pcd(2, 3, time_term)
        ctx.set_state(u_prev=un.ravel(), p_prev=p, u=u.ravel(), p=p)
        return ctx

    ctx = ctx_k()
    K, md = ctx.get_pcd_operator()
    w = theta * u + (1.0 - theta) * un
    Kt = PG.pcd_operator(kind, m.x, m.cells, m.facet_cells, m.facet_local, mk, 2, w, rho, P.time_coefficient(rho, dt, theta, a0, time_term))
    err = _rowrel(K, Kt)
    mdt = PG.mass_diag(kind, m.x, m.cells)
    err_md = np.abs(md - mdt).max() / mdt.max()
    print("K row-wise relative error %.3e, M_d error %.3e" % (err, err_md))
    assert err <= 1e-13, err
    assert err_md <= 1e-14, err_md
    # two passes and two contexts: the same bytes
    K2, _ = ctx.get_pcd_operator()
    ctx2 = ctx_k()
    K3, _ = ctx2.get_pcd_operator()
    assert K.data.tobytes() == K2.data.tobytes() == K3.data.tobytes()
    ctx.close()
    ctx2.close()


def test_generic_triangles_give_the_operator_of_the_closed_form_context():
    m, mk = _get("tri")
    nv = m.num_vertices
    rng = np.random.default_rng(9)
    u, un, p = rng.standard_normal((nv, 2)), rng.standard_normal((nv, 2)), rng.standard_normal(nv)
    Ks = []
    for generic in (True, False):
        if generic:
            ctx = _rot_ctx("tri", m, mk, 0.013, 1.06, 3.5e-3)
        else:
            ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, mk)
            ctx.set_params(0.013, 1.06, 3.5e-3, f=np.zeros(2))
        ctx.set_schur_pcd(2, 3, 1)
        ctx.set_state(u_prev=un.ravel(), p_prev=p, u=u.ravel(), p=p)
        Ks.append(ctx.get_pcd_operator())
        ctx.close()
    err = _rowrel(Ks[0][0], Ks[1][0])
    print("generic vs closed-form K: %.3e" % err)
    assert err <= 1e-13, err
    assert np.abs(Ks[0][1] - Ks[1][1]).max() <= 1e-14 * Ks[1][1].max()


def _walls(m, mk):
    return np.unique(np.asarray(m.facet_vertices)[mk == 4].ravel()).astype(np.int32)


def _outlet_nodes(kind, m, mk):
    return PG.facet_node_set(kind, m.cells, m.facet_cells, m.facet_local, np.flatnonzero(mk == 3))


def _physics(kind):
    """dt, rho, mu and the pair of (halved) pressures: the stenosis in mm-g-s units, the Q1 boxes as the channels of the rotational tests."""
    if kind == "tri":
        return 0.01, 1.06e-3, 3.5e-3, [MMHG / 2, 0.8 * MMHG / 2]
    return 0.02, 1.0, 0.05, [2.0, 0.5]


def _apply_ctx(kind, seed=11):
    m, mk = _get(kind)
    d, nv = m.x.shape[1], m.num_vertices
    dt, rho, mu, pv = _physics(kind)
    ctx = _rot_ctx(kind, m, mk, dt, rho, mu)
    ctx.set_pressure_boundaries([2, 3], pv, 100.0)
    wn = _walls(m, mk)
    ctx.add_dirichlet(0, wn, np.zeros((len(wn), d)))
    o = ctx.default_options()
    o.pc_type, o.remove_p_mean = 2, 0
    ctx.set_options(o)
    ctx.set_schur_pcd(2, 3, 1)
    rng = np.random.default_rng(seed)
    u, un = rng.standard_normal((nv, d)), rng.standard_normal((nv, d))
    ctx.set_state(u_prev=un.ravel(), p_prev=np.zeros(nv), u=u.ravel(), p=np.zeros(nv))
    ctx.assemble(True)
    return ctx, m, mk, 0.5 * (u + un), (dt, rho, mu)


@pytest.mark.parametrize("kind", KINDS)
def test_apply_preconditioner_rows_and_linearity(kind):
    ctx, m, mk, _, (dt, rho, mu) = _apply_ctx(kind)
    d, nv = m.x.shape[1], m.num_vertices
    rng = np.random.default_rng(2)
    r1, r2 = rng.standard_normal((d + 1) * nv), rng.standard_normal((d + 1) * nv)
    z1, z2 = ctx.apply_preconditioner(r1), ctx.apply_preconditioner(r2)
    assert ctx.info(78) == 2
    out = _outlet_nodes(kind, m, mk)
    assert len(out) > 0
    md = PG.mass_diag(kind, m.x, m.cells)
    assert np.allclose(z1[d * nv:][out], mu * r1[d * nv:][out] / md[out], rtol=1e-14, atol=0)
    z3 = ctx.apply_preconditioner(2.0 * r1 - 3.0 * r2)
    assert np.abs(z3 - (2.0 * z1 - 3.0 * z2)).max() <= 1e-10 * np.abs(z3).max()
    ctx.close()


def _exact_action_error():
    """Run in a child process with CFDH_L_CYCLES set: z_p of the device against the twin's exact action on the hexahedra."""
    ctx, m, mk, w, (dt, rho, mu) = _apply_ctx("hex")
    nv = m.num_vertices
    r = np.random.default_rng(5).standard_normal(4 * nv)
    z = ctx.apply_preconditioner(r)
    Kt = PG.pcd_operator("hex", m.x, m.cells, m.facet_cells, m.facet_local, mk, 2, w, rho, 2.0 * rho / dt)
    out = _outlet_nodes("hex", m, mk)
    zt = P.pcd_action(r[3 * nv:], Kt, PG.mass_diag("hex", m.x, m.cells), PG.laplacian("hex", m.x, m.cells), out, np.zeros(0, dtype=np.int64), mu)
    return np.abs(z[3 * nv:] - zt).max() / np.abs(zt).max()


def test_apply_preconditioner_with_converged_ap_solve_matches_the_exact_action():
    code = "import sys; sys.path.insert(0, %r); import test_gpu_pcd_pressurebc as t; print('ERR', t._exact_action_error())" % HERE
    env = dict(os.environ, CFDH_L_CYCLES="30")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=HERE)
    assert res.returncode == 0, res.stderr[-2000:]
    err = float([ln for ln in res.stdout.splitlines() if ln.startswith("ERR")][-1].split()[1])
    print("exact-action error %.3e" % err)
    assert err <= 1e-5, err


def _step(kind, pc_type):
    """One pressure-driven midpoint step from rest, walls no-slip, Newton to 1e-11 with the caps and the forcing of the plugin."""
    m, mk = _get(kind)
    d, nv = m.x.shape[1], m.num_vertices
    dt, rho, mu, pv = _physics(kind)
    ctx = _rot_ctx(kind, m, mk, dt, rho, mu)
    ctx.set_pressure_boundaries([2, 3], pv, 100.0)
    wn = _walls(m, mk)
    ctx.add_dirichlet(0, wn, np.zeros((len(wn), d)))
    o = ctx.default_options()
    o.pc_type, o.remove_p_mean = pc_type, 0
    o.snes_rtol, o.snes_stol, o.snes_max_it, o.ksp_max_it, o.ksp_restart = 1e-11, 0.0, 50, 10000, 150
    ctx.set_options(o)
    ctx.set_schur_pcd(2, 3, 1)
    ctx.set_ksp_forcing(2)
    z = np.zeros(d * nv)
    ctx.set_state(u_prev=z, p_prev=np.zeros(nv), u=z, p=np.zeros(nv))
    st = ctx.solve_step()
    u, p = ctx.get_solution()
    return ctx, st, u, p


def _twin_step(kind):
    m, mk = _get(kind)
    d, nv = m.x.shape[1], m.num_vertices
    dt, rho, mu, pv = _physics(kind)
    if d == 2:
        from oracle import np_twin as T
        from oracle import np_twin_gen as G
        import rot_twin as RT
        pb = RT.Problem(G.P1_TRI if kind == "tri" else G.Q1_QUAD, m.x, m.cells, m.facet_cells, m.facet_local, T.Params(dt, rho, mu, (0.0, 0.0)))
    else:
        from oracle import np_twin_gen3 as G3
        from oracle import np_twin_nd as TN
        import rot_twin3 as RT3
        pb = RT3.Problem(G3.Q1_HEX, m.x, m.cells, m.facet_cells, m.facet_local, TN.Params(dt, rho, mu, (0.0, 0.0, 0.0)))
    pb.set_pressure_boundaries([np.flatnonzero(mk == 2), np.flatnonzero(mk == 3)], pv, 100.0)
    wn = _walls(m, mk)
    pb.add_bc_u(wn, np.zeros((len(wn), d)))
    x, _ = pb.newton(np.zeros((d + 1) * nv), np.zeros((nv, d)))
    return x[: d * nv], x[d * nv:]


@pytest.mark.parametrize("kind", KINDS)
def test_pressure_driven_step_matches_the_twin_newton_step(kind):
    ctx, st, u, p = _step(kind, 2)
    assert st.reason > 0
    assert ctx.info(78) == 2 and ctx.info(79) == 2 and ctx.info(76) == 0
    h = ctx.newton_history()
    assert len(h["fnorm"]) == st.newton_its
    assert np.allclose(h["ksp_rtol"], P.ew_tolerances(list(h["fnorm"])), rtol=1e-14, atol=0)
    ut, pt = _twin_step(kind)
    eu, ep = np.abs(u - ut).max() / np.abs(ut).max(), np.abs(p - pt).max() / np.abs(pt).max()
    print("%s: newton %d, fgmres %d, u error %.3e, p error %.3e" % (kind, st.newton_its, st.krylov_its, eu, ep))
    # the tolerances of the rotational step tests (test_gpu_rotational.py, test_gpu_rotational3.py)
    assert eu <= 1e-8, eu
    assert ep <= 1e-7, ep
    ctx1, st1, u1, p1 = _step(kind, 1)
    assert st1.reason > 0 and ctx1.info(78) == 1
    e1 = np.abs(u1 - u).max() / np.abs(ut).max()
    print("%s: pc_type 1 fgmres %d, difference %.3e" % (kind, st1.krylov_its, e1))
    assert e1 <= 1e-6, e1
    assert np.abs(p1 - p).max() <= 1e-6 * np.abs(pt).max()
    ctx.close()
    ctx1.close()


_SCENARIOS = [("stenosis", "StenosisSimulation", dict(ny=6, L=12.0, x_sten=5.0, p_inlet=1.0, p_outlet=0.8)),
              ("unit_square_pipe", "UnitSquarePipeSimulation", dict(nx=24, ny=4, L=6.0, p_inlet=8.85, p_outlet=0.0)),
              ("unit_cube_pipe", "UnitCubePipeSimulation", dict(nx=12, ny=2, nz=2, L=6.0, p_inlet=8.85, p_outlet=0.0))]


@pytest.mark.parametrize("sim,cls,kw", _SCENARIOS)
def test_scenarios_run_with_stabilized_pcd_pressurebc(sim, cls, kw, tmp_path):
    from importlib import import_module
    sc = getattr(import_module("cfd_hemodynamic_amd.scenarios." + sim), cls)("stabilized_pcd_pressurebc", 0.01, 0.015, quiet=True, **kw)
    c = sc.solver.ctx
    assert c.info(77) == _lib.FORM_ROTATIONAL
    sc.solve(str(tmp_path))
    assert sc.num_steps == 2
    assert c.info(78) == 2 and c.info(79) == 2
    assert len(os.listdir(tmp_path)) > 0
    assert sc.solver.functional(7, sc.outlet_marker) > 0   # down the pressure drop


@pytest.mark.parametrize("sim,cls,kw", [("stenosis", "StenosisSimulation", dict(ny=6, L=12.0, x_sten=5.0, v_max=100.0)),
                                        ("simple_bifurcation", "MicrovasculatureSimulation", dict(res=1.2e-3))])
def test_stabilized_pcd_bdf2_third_step_is_the_bdf2_newton_step_of_the_twin(sim, cls, kw, tmp_path):
    from importlib import import_module
    from oracle import np_twin_nd as TN
    dt = 0.01
    sc = getattr(import_module("cfd_hemodynamic_amd.scenarios." + sim), cls)("stabilized_pcd_bdf2", dt, 0.025, quiet=True, newton_rtol=1e-11,
                                                                             options=dict(snes_stol=0.0), **kw)
    s = sc.solver
    coef, sols = [], []

    def record(t):
        coef.append((s.bdf_a0.value, s.bdf_a1.value, s.bdf_a2.value))
        sols.append((np.array(s.u_sol.x.array, copy=True), np.array(s.p_sol.x.array, copy=True)))

    sc.solve(str(tmp_path), afterStepCallback=record)
    assert sc.num_steps == 3 and s.step_count == 3
    assert coef == [(1.0, -1.0, 0.0), (1.5, -2.0, 0.5), (1.5, -2.0, 0.5)]
    assert s.ctx.info(78) == 2 and s.ctx.info(79) == 2
    m = sc.mesh
    d, nv = m.x.shape[1], m.num_vertices
    pb = TN.Problem(m.x, m.cells, m.facet_cells, m.facet_local,
                    TN.Params(dt, float(s.rho.value), float(s.mu.value), np.zeros(d), theta=1.0, a0=1.5, a1=-2.0, a2=0.5))
    for fld, bc in s._bcs:   # in the plugin's order: a later object overrides an earlier one on a shared dof
        g = np.asarray(bc.g.x.array)
        if fld == 0:
            pb.add_bc_u(bc.dofs, g.reshape(-1, d)[bc.dofs])
        else:
            pb.add_bc_p(bc.dofs, g[bc.dofs])
    (u1, _), (u2, p2), (u3, p3) = sols
    x, _ = pb.newton(np.concatenate([u2, p2]), u2.reshape(-1, d), rtol=1e-11, un2=u1.reshape(-1, d))
    ut, pt = x[: d * nv], x[d * nv:]
    eu, ep = np.abs(u3 - ut).max() / np.abs(ut).max(), np.abs(p3 - pt).max() / np.abs(pt).max()
    print("%s: u error %.3e, p error %.3e" % (sim, eu, ep))
    assert eu <= 1e-6, eu
    assert ep <= 1e-6, ep


def test_error_codes():
    m, mk = _get("tri")
    nv = m.num_vertices
    # generic context in the convective form: CFDH_E_ARG, the message still names the closed-form kernels
    g = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, mk, etype=3)
    g.set_params(0.01, 1.06e-3, 3.5e-3)
    with pytest.raises(ValueError, match="closed-form"):
        g.set_schur_pcd(2, 3, 1)
    # rotational: pc_type 2 without cfdh_set_schur_pcd is CFDH_E_STATE at the solve and at the operator query
    g.set_boundary_terms(ds_terms=False)
    g.set_formulation(_lib.FORM_ROTATIONAL)
    g.set_pressure_boundaries([2, 3], [MMHG / 2, 0.8 * MMHG / 2], 100.0)   # a residual at rest: the solve reaches the preconditioner
    o = g.default_options()
    o.pc_type = 2
    g.set_options(o)
    wn = _walls(m, mk)
    g.add_dirichlet(0, wn, np.zeros((len(wn), 2)))
    g.set_state(u_prev=np.zeros(2 * nv), p_prev=np.zeros(nv), u=np.zeros(2 * nv), p=np.zeros(nv))
    with pytest.raises(_lib.CfdhError, match="cfdh_set_schur_pcd") as ei:
        g.solve_step()
    assert not isinstance(ei.value, ValueError)
    with pytest.raises(_lib.CfdhError, match="cfdh_set_schur_pcd"):
        g.get_pcd_operator()
    # once set, the form cannot go back to convective
    g.set_schur_pcd(2, 3, 1)
    with pytest.raises(ValueError, match="pressure boundaries are set"):
        g.set_formulation(_lib.FORM_CONVECTIVE)
    g.set_pressure_boundaries([], [], 0.0)
    with pytest.raises(ValueError, match="PCD"):
        g.set_formulation(_lib.FORM_CONVECTIVE)
    with pytest.raises(ValueError):
        g.set_schur_pcd(2, 3, 2)
    g.close()
    # rotational P2 context: CFDH_E_ARG
    from cfd_hemodynamic_amd.elements import NodeMesh
    from cfd_hemodynamic_amd.mesh import create_unit_square
    m2 = NodeMesh(create_unit_square(3))
    c2 = _lib.Context(m2.x, m2.cells, m2.facet_cells, m2.facet_local, np.zeros(m2.num_facets, dtype=np.int32), etype=1)
    c2.set_params(0.01, 1.0, 0.01)
    c2.set_formulation(_lib.FORM_ROTATIONAL)
    with pytest.raises(ValueError, match="degree-1"):
        c2.set_schur_pcd(2, 3, 1)
    c2.close()
