"""The per-boundary Nitsche switch and backflow stabilisation of the rotational form on the GPU (cfdh_set_pressure_boundaries_ex;
gen_asm_kernel<ET, JAC, true> in csrc/cfdh_gen.hip, gen3_facet_kernel<ET, true> in csrc/cfdh_gen3.hip) against the NumPy twin
(tests/rot_backflow_twin.py), and the plugin `stabilized_schur_vascularbc_backflow` (the reference's
src/solvers/stabilized_schur_vascularbc_backflow.py)."""
import ctypes as C

import numpy as np
import pytest

from cfd_hemodynamic_amd import _lib
from gen_util import LIB_ETYPE
from gen3_util import LIB_ETYPE3
import rot_backflow_util as U
from test_rot_twin3 import duct, ends3

pytestmark = pytest.mark.gpu

VALUES = [1.7, -0.4]
BETA = 30.0
# seeds of U.random_state for which u_prev . n at the outlet points has both signs, and both within one facet (found on the CPU)
SEED = {(2, "P1"): 0, (2, "P2"): 0, (2, "Q1"): 0, (3, "P2"): 0, (3, "Q1"): 0}


def _context(dim, kind, m, prm, sets, markers_ids=(2, 3)):
    markers = np.zeros(m.num_facets, dtype=np.int32)
    for mk, fs in zip(markers_ids, sets):
        markers[fs] = mk
    ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, markers, etype=(LIB_ETYPE if dim == 2 else LIB_ETYPE3)[kind])
    ctx.set_params(prm.dt, prm.rho, prm.mu, f=prm.f)
    ctx.set_time_scheme(prm.theta, prm.a0, prm.a1, prm.a2)
    ctx.set_boundary_terms(ds_terms=False)
    ctx.set_formulation(_lib.FORM_ROTATIONAL)
    return ctx


class _Case:
    """Mesh, twin, random Dirichlet data on part of the walls, random state and history of one (dim, kind, scheme)."""

    def __init__(self, dim, kind, scheme="midpoint"):
        self.dim, self.kind = dim, kind
        self.m, (self.left, self.right, walls) = U.small_mesh(dim, kind)
        self.nv = self.m.num_vertices
        self.prm = U.params(dim, scheme=scheme)
        self.pb = U.twin(dim, kind, self.m, self.prm)
        rng = np.random.default_rng(5)
        self.wn = U.wall_nodes(dim, self.m, walls)[::2]
        self.g = rng.standard_normal((len(self.wn), dim))
        self.pb.add_bc_u(self.wn, self.g)
        self.xv, self.un, self.un2 = U.random_state(dim, self.nv, SEED[dim, kind])

    def twin(self, nitsche, beta_backflow):
        self.pb.set_pressure_boundaries([self.left, self.right], VALUES, BETA, nitsche=nitsche, beta_backflow=beta_backflow)
        return self.pb.assemble(self.xv, self.un, un2=self.un2)

    def context(self):
        d, nv = self.dim, self.nv
        ctx = _context(d, self.kind, self.m, self.prm, [self.left, self.right])
        ctx.add_dirichlet(0, self.wn, self.g)
        ctx.set_state(u_prev=self.un.ravel(), p_prev=np.zeros(nv), u=self.xv[: d * nv], p=self.xv[d * nv:])
        ctx.set_previous2(self.un2.ravel())
        return ctx


def _assembled(ctx):
    ctx.assemble(True)
    return np.concatenate(ctx.get_residual()), ctx.get_csr()


def _close(Fg, Jg, F, J):
    return np.abs(Fg - F).max() <= 1e-12 * np.abs(F).max() and abs(Jg - J).max() <= 1e-12 * abs(J).max()


@pytest.mark.parametrize("dim,kind", U.KINDS, ids=U.IDS)
@pytest.mark.parametrize("scheme", ["midpoint", "bdf2"])
def test_assembly_matches_the_twin(dim, kind, scheme):
    """Inlet with Nitsche terms, outlet a traction boundary with beta_bf = 0.2; u_prev . n changes sign over the outlet and inside
    one of its facets.  Residual, every CSR block and one SpMV agree with the twin to 1e-12; the residual-only pass gives the bits
    of the full pass; two passes and two contexts give the same bytes."""
    c = _Case(dim, kind, scheme)
    F, J = c.twin([1, 0], [0.0, 0.2])
    neg, pos, both = U.sign_pattern(c.pb.prev_normal_velocity(c.un, 1))
    assert neg and pos and both
    F0, J0 = c.twin([1, 0], [0.0, 0.0])
    assert np.abs(F - F0).max() > 1e-6 * np.abs(F).max() and abs(J - J0).max() > 1e-6 * abs(J).max()   # far above the tolerance
    out = []
    for _ in range(2):
        ctx = c.context()
        ctx.set_pressure_boundaries([2, 3], VALUES, BETA, nitsche=[1, 0], beta_backflow=[0.0, 0.2])
        for _rep in range(2):
            Fg, Jg = _assembled(ctx)
            out.append((Fg, Jg.data.copy()))
        ctx.assemble(False)
        assert np.array_equal(np.concatenate(ctx.get_residual()), Fg)
        if not out[2:]:
            assert np.abs(Fg - F).max() <= 1e-12 * np.abs(F).max()
            assert abs(Jg - J).max() <= 1e-12 * abs(J).max()
            y = np.random.default_rng(7).standard_normal(len(F))
            assert np.abs(ctx.spmv(y) - J @ y).max() <= 1e-12 * np.abs(J @ y).max()
        ctx.close()
    for Fk, Ak in out[1:]:
        assert np.array_equal(Fk, out[0][0]) and np.array_equal(Ak, out[0][1])


@pytest.mark.parametrize("dim,kind", U.KINDS, ids=U.IDS)
def test_switches_are_per_boundary(dim, kind):
    """Swapping which boundary carries the Nitsche terms and which the backflow term gives the swapped twin (and not the other
    one); both arrays NULL through the _ex entry give the bytes of cfdh_set_pressure_boundaries."""
    c = _Case(dim, kind)
    ctx = c.context()
    twins = {}
    for nit, bf in (([1, 0], [0.0, 0.2]), ([0, 1], [0.2, 0.0]), ([0, 0], [0.0, 0.0]), ([1, 1], [0.2, 0.2])):
        F, J = c.twin(nit, bf)
        ctx.set_pressure_boundaries([2, 3], VALUES, BETA, nitsche=nit, beta_backflow=bf)
        Fg, Jg = _assembled(ctx)
        assert _close(Fg, Jg, F, J), (nit, bf)
        for F2, J2 in twins.values():   # the cases are told apart: the others are far from this result
            assert not _close(Fg, Jg, F2, J2)
        twins[tuple(nit), tuple(bf)] = (F, J)
    ctx.set_pressure_boundaries([2, 3], VALUES, BETA)
    Fp, Jp = _assembled(ctx)
    ctx.set_pressure_boundaries([], [], 0.0)
    mk, vl = np.array([2, 3], dtype=np.int32), np.array(VALUES)
    rc = ctx.L.cfdh_set_pressure_boundaries_ex(ctx.h, 2, mk.ctypes.data_as(C.POINTER(C.c_int32)), vl.ctypes.data_as(C.POINTER(C.c_double)),
                                               BETA, None, None)
    assert rc == 0
    Fe, Je = _assembled(ctx)
    assert np.array_equal(Fe, Fp) and np.array_equal(Je.data, Jp.data)
    ctx.close()


def _rest_problem(dim, kind, p_out, beta_bf, m=None):
    """Twin and context at rest on a small channel / duct, walls no-slip, inlet pressure 0.5 (Nitsche), outlet pressure p_out
    (traction boundary with beta_bf)."""
    if m is None:
        m = U.channel(kind, 6, 3) if dim == 2 else duct(kind, 3, 2, 0.75)
    left, right, walls = U.channel_ends(m, kind) if dim == 2 else ends3(m)
    prm = U.params(dim, 0.02, 1.0, 0.05, f=(0.0, 0.0, 0.0))
    pb = U.twin(dim, kind, m, prm)
    pb.set_pressure_boundaries([left, right], [0.5, p_out], 100.0, nitsche=[1, 0], beta_backflow=[0.0, beta_bf])
    wn = U.wall_nodes(dim, m, walls)
    pb.add_bc_u(wn, np.zeros((len(wn), dim)))
    return m, pb, (left, right), wn, prm


@pytest.mark.parametrize("dim,kind", [(2, "P1"), (3, "Q1")], ids=["2d-P1", "3d-Q1"])
def test_validity_bookkeeping(dim, kind):
    """cfdh_info 74 (preconditioner builds) / 75 (preconditioner valid): a value-only _ex call keeps Jacobian and preconditioner; a
    change of beta_backflow[k] or of a Nitsche bit invalidates them; negative / NaN beta_backflow is CFDH_E_ARG."""
    m, pb, sets, wn, prm = _rest_problem(dim, kind, 2.0, 0.2)
    nv = m.num_vertices
    ctx = _context(dim, kind, m, prm, sets)
    ctx.add_dirichlet(0, wn, np.zeros((len(wn), dim)))
    kw = dict(nitsche=[1, 0], beta_backflow=[0.0, 0.2])
    ctx.set_pressure_boundaries([2, 3], [0.5, 2.0], 100.0, **kw)
    zu, zp = np.zeros(dim * nv), np.zeros(nv)
    ctx.set_state(u_prev=zu, p_prev=zp, u=zu, p=zp)
    ctx.solve_step()
    assert ctx.info(75) == 1 and ctx.info(76) == 0
    builds = ctx.info(74)
    ctx.assemble(True)
    J0 = ctx.get_csr().data.copy()
    ctx.set_pressure_boundaries([2, 3], [0.5, 1.5], 100.0, **kw)   # value only
    assert ctx.info(75) == 1 and np.array_equal(ctx.get_csr().data, J0)
    ctx.assemble(True)
    assert np.array_equal(ctx.get_csr().data, J0) and ctx.info(75) == 1 and ctx.info(74) == builds
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta_backflow"):
            ctx.set_pressure_boundaries([2, 3], [0.5, 1.5], 100.0, nitsche=[1, 0], beta_backflow=[0.0, bad])
    assert ctx.info(75) == 1   # a refused call changes nothing
    ctx.set_pressure_boundaries([2, 3], [0.5, 1.5], 100.0, nitsche=[1, 0], beta_backflow=[0.0, 0.3])
    assert ctx.info(75) == 0
    ctx.solve_step()
    assert ctx.info(75) == 1
    ctx.set_pressure_boundaries([2, 3], [0.5, 1.5], 100.0, nitsche=[1, 1], beta_backflow=[0.0, 0.3])
    assert ctx.info(75) == 0
    ctx.close()


@pytest.mark.parametrize("dim,kind", [(2, "P1"), (3, "Q1")], ids=["2d-P1", "3d-Q1"])
def test_time_steps_with_inflow_through_the_outlet_match_the_twin(dim, kind):
    """Three steps from rest with the outlet pressure ABOVE the inlet pressure: fluid enters through the outlet, so the backflow term
    is active from the second step on.  Device Newton + FGMRES against the twin's direct Newton, options and tolerances of
    test_time_steps_on_a_duct_match_the_twin; the twin's own solution without the term lies more than 100 tolerances away."""
    p_out = 2.0
    m, pb, sets, wn, prm = _rest_problem(dim, kind, p_out, 0.2)
    nv = m.num_vertices
    ctx = _context(dim, kind, m, prm, sets)
    ctx.add_dirichlet(0, wn, np.zeros((len(wn), dim)))
    ctx.set_pressure_boundaries([2, 3], [0.5, p_out], 100.0, nitsche=[1, 0], beta_backflow=[0.0, 0.2])
    o = ctx.default_options()
    o.snes_rtol, o.snes_stol, o.ksp_rtol = 1e-12, 0.0, 1e-10
    ctx.set_options(o)
    x = np.zeros((dim + 1) * nv)
    ctx.set_state(u_prev=x[: dim * nv], p_prev=x[dim * nv:], u=x[: dim * nv], p=x[dim * nv:])
    un = np.zeros((nv, dim))
    for step in range(3):
        st = ctx.solve_step()
        assert st.reason > 0 and ctx.info(76) == 0
        u, p = ctx.get_solution()
        ctx.advance()
        if step > 0:
            assert (pb.prev_normal_velocity(un, 1) < 0).all()   # inflow at every outlet point: the term is active
        x, _ = pb.newton(x, un)
        un = x[: dim * nv].reshape(-1, dim).copy()
        assert np.abs(u - x[: dim * nv]).max() <= 1e-8 * np.abs(x[: dim * nv]).max(), step
        assert np.abs(p - x[dim * nv:]).max() <= 1e-7 * np.abs(x[dim * nv:]).max(), step
    ctx.close()
    assert pb.flux(x, sets[1]) < 0   # in through the outlet
    # the comparison sees the term: the twin without it ends more than 100 tolerances away
    _, pb0, _, _, _ = _rest_problem(dim, kind, p_out, 0.0, m)
    x0, un0 = np.zeros((dim + 1) * nv), np.zeros((nv, dim))
    for _ in range(3):
        x0, _ = pb0.newton(x0, un0)
        un0 = x0[: dim * nv].reshape(-1, dim).copy()
    assert np.abs(x0[: dim * nv] - x[: dim * nv]).max() > 100 * 1e-8 * np.abs(x[: dim * nv]).max()


_OPT = dict(snes_rtol=1e-12, snes_stol=0.0, ksp_rtol=1e-10)
NAME = "stabilized_schur_vascularbc_backflow"


def test_unit_square_pipe_through_the_plugin_equals_the_twin(tmp_path):
    """unit_square_pipe (Q1) through Scenario.solve with initial_ffr > 1, so that the outlet sees inflow: the outlet value stays
    initial_ffr * p_inlet / 2 over the steps (no resistance update, R_resistance unused), and the final field is the twin's with
    Nitsche on the inlet only and the backflow term on the outlet only."""
    from cfd_hemodynamic_amd.scenarios.unit_square_pipe import UnitSquarePipeSimulation
    p_in, ffr, dt = 8.85, 1.5, 0.01
    sc = UnitSquarePipeSimulation(NAME, dt, 0.025, p_inlet=p_in, p_outlet=0.0, initial_ffr=ffr, R_resistance=7.0, beta_backflow=0.2,
                                  nx=12, ny=3, L=6.0, quiet=True, options=_OPT)
    s = sc.solver
    assert s.ctx.info(28) == 2 and s.ctx.info(77) == _lib.FORM_ROTATIONAL
    assert s._p_inlet_val == p_in / 2 and s._p_outlet_val == ffr * p_in / 2 and s.beta_backflow == 0.2
    sc.solve(str(tmp_path))
    assert sc.num_steps == 3 and s._p_outlet_val == ffr * p_in / 2 and not hasattr(s, "outlet_history")
    m, ft = sc.mesh, sc._ft
    nv = m.num_vertices
    pb = U.twin(2, "Q1", m, U.T.Params(dt, 1.06e-3, 3.5e-3, (0.0, 0.0)))
    wn = U.wall_nodes(2, m, ft.find(3))
    pb.add_bc_u(wn, np.zeros((len(wn), 2)))
    pb.set_pressure_boundaries([ft.find(1), ft.find(2)], [p_in / 2, ffr * p_in / 2], 100.0, nitsche=[1, 0], beta_backflow=[0.0, 0.2])
    x, un = np.zeros(3 * nv), np.zeros((nv, 2))
    for _ in range(3):
        x, _ = pb.newton(x, un)
        un = x[: 2 * nv].reshape(-1, 2).copy()
    assert (pb.prev_normal_velocity(un, 1) < 0).any()
    xg = np.concatenate([np.asarray(s.u_sol.x.array), np.asarray(s.p_sol.x.array)])
    assert np.abs(xg - x).max() <= 1e-8 * np.abs(x).max()


@pytest.mark.parametrize("cell", [dict(), dict(cell_type="tetrahedron", p_grade=2)], ids=["hexahedra", "P2-tetrahedra"])
def test_unit_cube_pipe_runs_through_the_plugin(tmp_path, cell):
    """unit_cube_pipe on hexahedra and on P2 tetrahedra: converged steps, fixed outlet value, inflow = outflow, flow from the high
    to the low pressure."""
    from cfd_hemodynamic_amd.scenarios.unit_cube_pipe import UnitCubePipeSimulation
    p_in = 8.85
    sc = UnitCubePipeSimulation(NAME, 0.01, 0.025, p_inlet=p_in, p_outlet=0.0, options=_OPT, nx=12, ny=2, nz=2, L=6.0, quiet=True, **cell)
    s = sc.solver
    assert s.ctx.info(28) == (1 if cell else 2) and s.ctx.info(77) == _lib.FORM_ROTATIONAL
    assert s._p_outlet_val == 0.8 * p_in / 2   # the plugin's own default initial_ffr
    sc.solve(str(tmp_path))
    assert sc.num_steps == 3 and s._p_outlet_val == 0.8 * p_in / 2
    q_in, q_out = -s.functional(7, sc.inlet_marker), s.functional(7, sc.outlet_marker)
    assert q_out > 0 and abs(q_in - q_out) <= 1e-8 * q_out


def test_plugin_refusals():
    from cfd_hemodynamic_amd.mesh import create_unit_square
    from cfd_hemodynamic_amd.mesh3d import create_unit_cube
    from cfd_hemodynamic_amd.solvers.stabilized_schur_vascularbc_backflow import Solver
    with pytest.raises(ValueError, match="p_inlet is required for stabilized_schur_vascularbc_backflow"):
        Solver(create_unit_square(2), 0.01, 1.0, 0.01, [0.0, 0.0])
    with pytest.raises(NotImplementedError, match="p_grade=2"):
        Solver(create_unit_cube(1), 0.01, 1.0, 0.01, [0.0, 0.0, 0.0], p_inlet=1.0)   # P1 tetrahedra
    s = Solver(create_unit_square(2), 0.01, 1.0, 0.01, [0.0, 0.0], p_inlet=1.0, quiet=True)
    with pytest.raises(KeyError):
        s.setup([], [], None, None)
    with pytest.raises(KeyError):
        s.setup([], [], None, dict(inlet=1))
