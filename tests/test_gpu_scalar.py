"""Passive scalar transport on the device (cfdh_scalar_*, csrc/cfdh_scalar.hip) against the NumPy / SciPy twin (scalar_twin.py):
operator and right-hand side, reproducibility, time steps, the steady uniform-flow age, functionals, refusals, the untouched flow
path of a context that never enables the scalar, and the scenario / command-line routes.

Two meshes carry most tests: a 9 x 7 rectangle of triangles (80 vertices) and a 4 x 3 x 4 box of tetrahedra (100 vertices) -- more
than 64 rows and no multiple of 64 (a full and a partial slice of the work list), the meshes' maximal-valence rows included; the
velocity is non-uniform with u_sol != u_prev and has a zero cell mean in exactly one cell; the Dirichlet set holds an interior vertex
shared by several cells."""
import os

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import scalar_twin as T
import scalar_util as U
from cfd_hemodynamic_amd import _lib

pytestmark = pytest.mark.gpu

RHO, MU = 1.3, 0.04
_CACHE = {}


def case(name):
    """Mesh and fields, built once per mesh and left unchanged."""
    if name not in _CACHE:
        mesh = U.MESHES[name]()
        _CACHE[name] = (mesh, U.fields(mesh))
    return _CACHE[name]


def make_ctx(mesh, fl=None, dt=U.DT, **kw):
    ctx = _lib.Context(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, mesh.facet_marker, **kw)
    ctx.set_params(dt, RHO, MU)
    if fl is not None:
        z = np.zeros(mesh.num_vertices)
        ctx.set_state(u_prev=fl["u_prev"].ravel(), p_prev=z, u=fl["u_sol"].ravel(), p=z)
    return ctx


def twin_system(mesh, fl, c0, theta, D, s, dt=U.DT):
    return T.assemble(mesh.x, mesh.cells, fl["u_sol"], fl["u_prev"], c0, dt, D, s, theta, fl["nodes"], fl["vals"])


def test_meshes_are_what_the_tests_need():
    for name, nv in (("rectangle", 80), ("box", 100)):
        mesh, fl = case(name)
        assert mesh.num_vertices == nv and nv > 64 and nv % 64 != 0
        assert fl["valence"][fl["shared"]] == fl["valence"].max() >= 6  # a maximal-valence row, constrained, shared by several cells
        assert not np.array_equal(fl["u_sol"], fl["u_prev"])


@pytest.mark.parametrize("name", ["rectangle", "box"])
@pytest.mark.parametrize("theta,D,s", U.PARAMS)
def test_operator_matches_the_twin(name, theta, D, s):
    """Left-hand matrix and right-hand side row-wise within 1e-12 (row max); two assemblies return identical bytes."""
    mesh, fl = case(name)
    ctx = make_ctx(mesh, fl)
    ctx.scalar_enable(D, s, theta)
    ctx.scalar_state(fl["c0"])
    ctx.scalar_set_dirichlet(fl["nodes"], fl["vals"])
    n0 = ctx.info(_lib.INFO_SCALAR_ASSEMBLIES)
    A, b = ctx.scalar_operator()
    A2, b2 = ctx.scalar_operator()
    assert ctx.info(_lib.INFO_SCALAR_ASSEMBLIES) == n0 + 2 and ctx.info(_lib.INFO_SCALAR_STEPS) == 0
    assert A.data.tobytes() == A2.data.tobytes() and b.tobytes() == b2.tobytes() and np.array_equal(A.indices, A2.indices)
    At, bt = twin_system(mesh, fl, fl["c0"], theta, D, s)
    # the device stores the whole vertex-graph pattern (zeros on Dirichlet rows), the twin only what it assembled
    diff = abs(A - At).toarray()
    rowmax = np.maximum(np.abs(At.toarray()).max(axis=1), np.abs(bt))
    print("%s theta=%g D=%g s=%g: max row-relative difference matrix %.2e rhs %.2e" % (name, theta, D, s, (diff.max(axis=1) / rowmax).max(), (np.abs(b - bt) / rowmax).max()))
    assert np.all(diff.max(axis=1) <= 1e-12 * rowmax)
    assert np.all(np.abs(b - bt) <= 1e-12 * rowmax)
    assert np.array_equal(b[fl["nodes"]], fl["vals"])
    assert np.array_equal(ctx.scalar_state(), fl["c0"])  # the getter assembles, it does not step
    ctx.close()


def _margin(mesh, fl, theta, D, s, nsteps, dt=U.DT):
    """Twin states of nsteps direct solves, and the largest distance a NumPy BiCGStab + Jacobi at rtol 1e-12 keeps from the direct
    solve on the same systems (same initial guess as the device: c0 with the Dirichlet values imposed)."""
    c, states, dist = fl["c0"].copy(), [], 0.0
    for _ in range(nsteps):
        A, b = twin_system(mesh, fl, c, theta, D, s, dt)
        direct = spla.spsolve(A.tocsc(), b)
        x0 = c.copy()
        x0[fl["nodes"]] = fl["vals"]
        it, _ = T.bicgstab_jacobi(A, b, x0, 1e-12)
        dist = max(dist, np.abs(it - direct).max())
        c = direct
        states.append(c)
    return states, dist


@pytest.mark.parametrize("name", ["rectangle", "box"])
@pytest.mark.parametrize("theta,D,s", U.PARAMS)
def test_three_steps_match_the_direct_solves(name, theta, D, s):
    """Three steps at rtol 1e-12 against the twin's direct solves.  The bound is 100 x the distance that a NumPy BiCGStab with the
    same preconditioner and tolerance keeps from the direct solve on the same systems, computed here and printed: 2.3e-12 .. 1.5e-11 over the
    eight cases (fields of size one, cond_2(A) 18 .. 68), so bounds of 2.3e-10 .. 1.5e-9; the device measured 2.6e-12 .. 1.8e-11
    from the direct solves on an MI355X."""
    mesh, fl = case(name)
    states, dist = _margin(mesh, fl, theta, D, s, 3)
    ctx = make_ctx(mesh, fl)
    ctx.scalar_enable(D, s, theta)
    ctx.scalar_set_tolerances(rtol=1e-12)
    ctx.scalar_state(fl["c0"])
    ctx.scalar_set_dirichlet(fl["nodes"], fl["vals"])
    worst = 0.0
    for k in range(3):
        st = ctx.scalar_step()
        assert st.reason == 2 and 0 < st.its < 200 and st.rel_res <= 1e-12
        worst = max(worst, np.abs(ctx.scalar_state() - states[k]).max())
    print("%s theta=%g D=%g s=%g: NumPy BiCGStab distance %.3e, device distance %.3e" % (name, theta, D, s, dist, worst))
    assert dist > 0
    assert worst <= 100 * dist
    assert ctx.info(_lib.INFO_SCALAR_STEPS) == 3 and ctx.info(_lib.INFO_SCALAR_ASSEMBLIES) == 3  # one assembly launch per step
    ctx.close()


@pytest.mark.parametrize("name", ["rectangle", "box"])
def test_uniform_flow_age_is_x_over_U(name):
    """Uniform flow (U, 0[, 0]), inlet c = 0, s = 1, D = 0, theta_c = 1: the device reaches c = x / U within the margin of the
    solve test (100 x the NumPy BiCGStab's distance from the direct solves of the same steps)."""
    mesh, _ = case(name)
    d = mesh.x.shape[1]
    Uf, dt, nsteps = 2.0, 0.5, 40
    u = np.zeros((mesh.num_vertices, d))
    u[:, 0] = Uf
    inlet = np.unique(mesh.facet_vertices[mesh.facet_marker == U.INLET]).astype(np.int32)
    fl = dict(u_sol=u, u_prev=u, c0=np.zeros(mesh.num_vertices), nodes=inlet, vals=np.zeros(len(inlet)))
    states, dist = _margin(mesh, fl, 1.0, 0.0, 1.0, nsteps, dt)
    exact = mesh.x[:, 0] / Uf
    assert np.abs(states[-1] - exact).max() <= 1e-12 * mesh.L / Uf
    ctx = make_ctx(mesh, fl, dt=dt)
    ctx.scalar_enable(0.0, 1.0, 1.0)
    ctx.scalar_set_tolerances(rtol=1e-12)
    ctx.scalar_set_dirichlet(inlet, 0.0)
    for _ in range(nsteps):
        ctx.scalar_step()
    err = np.abs(ctx.scalar_state() - exact).max()
    print("%s: NumPy BiCGStab distance %.3e, device |c - x/U| %.3e" % (name, dist, err))
    assert err <= 100 * dist
    ctx.close()


@pytest.mark.parametrize("name", ["rectangle", "box"])
def test_functionals_match_the_twin(name):
    mesh, fl = case(name)
    ctx = make_ctx(mesh, fl)
    ctx.scalar_enable(0.0, 0.0, 0.5)
    c = fl["c0"] - 0.2
    ctx.scalar_state(c)
    want = [T.integral(mesh.x, mesh.cells, c), None, c.min(), c.max()]
    for kind in (0, 2, 3):
        got = ctx.scalar_functional(kind)
        assert abs(got - want[kind]) <= 1e-12 * abs(want[kind]), kind
    assert ctx.scalar_functional(2) == c.min() and ctx.scalar_functional(3) == c.max()
    for marker in (U.INLET, U.OUTLET, 0):
        w = T.flux(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, mesh.facet_marker, marker, fl["u_sol"], c)
        got = ctx.scalar_functional(1, marker)
        assert abs(got - w) <= 1e-12 * abs(w), (marker, got, w)
    assert ctx.scalar_functional(1, 77) == 0.0
    with pytest.raises(ValueError, match="kind"):
        ctx.scalar_functional(4)
    ctx.close()


def test_refusals_change_nothing():
    mesh, fl = case("rectangle")
    E, S, A_ = _lib.INFO_SCALAR_ENABLED, _lib.INFO_SCALAR_STEPS, _lib.INFO_SCALAR_ASSEMBLIES
    # contexts without the scalar: generic elements, a part of a partitioned run, pressure correction
    g = _lib.Context(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, mesh.facet_marker, etype=3)
    with pytest.raises(ValueError, match="closed-form"):
        g.scalar_enable(0.0, 1.0, 0.5)
    assert g.info(E) == 0 and g.info(A_) == 0
    g.close()
    part = _lib.Context(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, mesh.facet_marker, nv_owned=mesh.num_vertices - 1)
    with pytest.raises(ValueError, match="partitioned"):
        part.scalar_enable(0.0, 1.0, 0.5)
    assert part.info(E) == 0 and part.info(A_) == 0
    part.close()
    from cfd_hemodynamic_amd.elements import NodeMesh
    nm = NodeMesh(mesh)
    ipcs = _lib.IpcsContext(nm.x, nm.cells, mesh.num_vertices, nm.facet_cells, nm.facet_local, np.zeros(len(nm.facet_cells), dtype=np.int32))
    with pytest.raises(ValueError, match="pressure-correction"):
        ipcs.scalar_enable(0.0, 1.0, 0.5)
    with pytest.raises(_lib.CfdhError):
        ipcs.scalar_step()
    ipcs.close()
    # every call before cfdh_scalar_enable: CFDH_E_STATE
    ctx = make_ctx(mesh, fl)
    for call in (lambda: ctx.scalar_set_dirichlet([0], [1.0]), lambda: ctx.scalar_state(), lambda: ctx.scalar_state(fl["c0"]),
                 lambda: ctx.scalar_set_tolerances(), lambda: ctx.scalar_step(), lambda: ctx.scalar_operator(), lambda: ctx.scalar_functional(0)):
        with pytest.raises(_lib.CfdhError, match="cfdh_scalar_enable was not called"):
            call()
    # bad parameters leave the scalar off
    for args in ((-1e-3, 0.0, 0.5), (np.inf, 0.0, 0.5), (np.nan, 0.0, 0.5), (0.0, np.inf, 0.5), (0.0, np.nan, 0.5), (0.0, 0.0, 0.0), (0.0, 0.0, 1.5),
                 (0.0, 0.0, -0.5), (0.0, 0.0, np.nan)):
        with pytest.raises(ValueError):
            ctx.scalar_enable(*args)
        assert ctx.info(E) == 0
    ctx.scalar_enable(1e-2, 1.0, 0.5)
    assert ctx.info(E) == 1 and ctx.info(S) == 0 and ctx.info(A_) == 0
    ctx.scalar_state(fl["c0"])
    ctx.scalar_set_dirichlet(fl["nodes"], fl["vals"])
    A0, b0 = ctx.scalar_operator()
    # ... and, once it is on, keep parameters, set, state and tolerances
    for args in ((-1e-3, 0.0, 0.5), (0.0, np.nan, 0.5), (0.0, 0.0, 1.5)):
        with pytest.raises(ValueError):
            ctx.scalar_enable(*args)
    nv = mesh.num_vertices
    for nodes, vals in (([0, nv], [1.0, 1.0]), ([-1], [1.0]), ([0, 1], [1.0, np.nan]), ([0], [np.inf])):
        with pytest.raises(ValueError):
            ctx.scalar_set_dirichlet(nodes, vals)
    bad = fl["c0"].copy()
    bad[7] = np.nan
    with pytest.raises(ValueError):
        ctx.scalar_state(bad)
    for kw in (dict(rtol=1.0), dict(rtol=-1e-3), dict(atol=-1.0), dict(max_it=0)):
        with pytest.raises(ValueError):
            ctx.scalar_set_tolerances(**kw)
    A1, b1 = ctx.scalar_operator()
    assert A0.data.tobytes() == A1.data.tobytes() and b0.tobytes() == b1.tobytes() and np.array_equal(ctx.scalar_state(), fl["c0"])
    # a second enable changes the parameters and keeps c; n = 0 clears the Dirichlet set
    ctx.scalar_enable(0.0, 0.0, 1.0)
    assert np.array_equal(ctx.scalar_state(), fl["c0"])
    ctx.scalar_set_dirichlet([], [])
    A2, b2 = ctx.scalar_operator()
    At, bt = T.assemble(mesh.x, mesh.cells, fl["u_sol"], fl["u_prev"], fl["c0"], U.DT, 0.0, 0.0, 1.0)
    assert abs(A2 - At).max() <= 1e-12 * abs(At).max() and np.abs(b2 - bt).max() <= 1e-12 * np.abs(bt).max()
    # the cap: CFDH_E_DIVERGED, reason DIVERGED_ITS, c unchanged
    ctx.scalar_set_tolerances(rtol=1e-14, max_it=1)
    with pytest.raises(RuntimeError, match="reason: -3"):
        ctx.scalar_step()
    assert np.array_equal(ctx.scalar_state(), fl["c0"]) and ctx.info(S) == 0
    ctx.close()


@pytest.mark.parametrize("name", ["rectangle", "box"])
def test_flow_path_is_untouched(name):
    """A context that never enables the scalar reports 0 launches and allocates nothing; its Jacobian and residual bytes equal
    those of a fresh context that does run the scalar."""
    mesh, fl = case(name)
    d = mesh.x.shape[1]
    bnd = np.unique(mesh.facet_vertices).astype(np.int32)

    def flow(with_scalar):
        ctx = make_ctx(mesh, fl)
        ctx.add_dirichlet(0, bnd, np.ones((len(bnd), d)))
        if with_scalar:
            ctx.scalar_enable(1e-2, 1.0, 0.5)
            ctx.scalar_set_dirichlet(fl["nodes"], fl["vals"])
            ctx.scalar_step()
        ctx.assemble(True)
        J, (ru, rp) = ctx.get_csr(), ctx.get_residual()
        info = [ctx.info(k) for k in (_lib.INFO_SCALAR_ENABLED, _lib.INFO_SCALAR_STEPS, _lib.INFO_SCALAR_ASSEMBLIES)]
        ctx.close()
        return J, ru, rp, info
    J0, ru0, rp0, i0 = flow(False)
    J1, ru1, rp1, i1 = flow(True)
    assert i0 == [0, 0, 0] and i1 == [1, 1, 1]
    assert J0.data.tobytes() == J1.data.tobytes() and np.array_equal(J0.indices, J1.indices)
    assert ru0.tobytes() == ru1.tobytes() and rp0.tobytes() == rp1.tobytes()


# ---------------------------------------------------------------------------------------------------- scenario level
def test_stenosis_age(tmp_path):
    from cfd_hemodynamic_amd.io import read_vtu
    from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
    sc = StenosisSimulation("stabilized_schur", 0.01, 0.05, ny=6, L=12.0, x_sten=5.0, v_max=100.0, quiet=True)
    sc.early_stop_tolerance = 0
    sc.setup()
    out = str(tmp_path / "age")
    sc.solve(out, transport="age")
    tr = sc.transport
    nv = sc.mesh.num_vertices
    assert sc.num_steps == 5 and tr["mode"] == "age" and tr["field"].shape == (nv,) and len(tr["integral"]) == 5
    assert np.all(np.isfinite(tr["field"])) and np.all(np.diff(tr["integral"]) > 0) and tr["integral"][0] > 0
    inlet = np.unique(sc.mesh.facet_vertices[sc._ft.find(sc.inlet_marker)])
    assert len(inlet) and np.all(tr["field"][inlet] == 0.0)
    print("stenosis age after 5 steps: min %.3e max %.3e (t = 0.05)" % (tr["field"].min(), tr["field"].max()))
    assert 0.5 * 0.05 <= tr["field"].max() <= 2 * 0.05  # sanity only: SUPG over- and undershoots at the inlet layer are not clipped
    assert sc.solver.ctx.info(_lib.INFO_SCALAR_STEPS) == 5 and sc.solver.ctx.info(_lib.INFO_SCALAR_ASSEMBLIES) == 5
    z = np.load(os.path.join(out, "transport.npz"))
    assert np.array_equal(z["field"], tr["field"]) and np.array_equal(z["integral"], tr["integral"]) and z["x"].shape == (nv, 2)
    v = read_vtu(os.path.join(out, "transport_000005.vtu"))
    assert np.array_equal(v["transport"].ravel(), tr["field"])
    assert np.all(read_vtu(os.path.join(out, "transport_000000.vtu"))["transport"] == 0.0)
    # off: nothing written, nothing allocated
    sc2 = StenosisSimulation("stabilized_schur", 0.01, 0.02, ny=6, L=12.0, x_sten=5.0, v_max=100.0, quiet=True)
    sc2.setup()
    out2 = str(tmp_path / "off")
    sc2.solve(out2)
    assert sc2.transport is None and not os.path.exists(os.path.join(out2, "transport.npz")) and sc2.solver.ctx.info(_lib.INFO_SCALAR_ENABLED) == 0
    with pytest.raises(ValueError):
        sc2.solve(None, transport="dye")


def test_closed_cavity_age_equals_time():
    """lid_driven2D has no inlet: no Dirichlet set, and with s = 1 the age is c = t everywhere (constants lie in the kernel of the
    spatial operators, the mass rows sum to the source's).  Bound from the solver's stopping rule |b - A c| <= rtol |b|: the error
    of one step is at most rtol cond_2(A) |c|_2 <= rtol cond_2(A) t sqrt(nv) in the maximum norm, and the steps add up."""
    from cfd_hemodynamic_amd.scenarios.lid_driven2D import LidDriven2DSimulation
    sc = LidDriven2DSimulation("stabilized_schur", 0.01, 0.05, nx=8, quiet=True)
    sc.early_stop_tolerance = 0
    sc.setup()
    sc.solve(None, transport="age")
    c = sc.transport["field"]
    A, _ = sc.solver.ctx.scalar_operator()
    bound = sc.num_steps * 1e-8 * np.linalg.cond(A.toarray()) * sc.t_end * np.sqrt(len(c))
    print("closed cavity: |c - t| = %.3e, bound %.3e" % (np.abs(c - sc.t_end).max(), bound))
    assert sc.num_steps == 5 and np.abs(c - sc.t_end).max() <= bound
    vol = 1.0
    assert np.abs(sc.transport["integral"] - vol * sc.transport["times"]).max() <= bound * vol


def test_unit_cube_pipe_bolus_through_the_command_line(tmp_path):
    from cfd_hemodynamic_amd.__main__ import main
    kw = dict(p_inlet=50.0, p_outlet=0.0, R_resistance=0.1, nx=12, ny=2, nz=2, cell_type="tetrahedron", p_grade=1)
    argv = ["simulate", "--simulation", "unit_cube_pipe", "--solver", "stabilized_schur_pressure_backflow", "--T", "0.04", "--dt", "0.01",
            "--output_dir", str(tmp_path), "--quiet", "True", "--transport", "bolus", "--bolus_from", "0.01", "--bolus_to", "0.03",
            "--transport_diffusivity", "1e-3"]
    for k, v in kw.items():
        argv += ["--" + k, str(v)]
    assert main(argv) == 0
    z = np.load(str(tmp_path / "unit_cube_pipe" / "run" / "transport.npz"))
    assert z["x"].shape[1] == 3 and z["cells"].shape[1] == 4 and z["field"].shape == (len(z["x"]),) and np.all(np.isfinite(z["field"]))
    assert len(z["integral"]) == 4 and z["integral"][0] == 0.0 and z["integral"][1] > 0 and z["integral"][2] > z["integral"][1]
    inlet = np.nonzero(z["x"][:, 0] == 0.0)[0]
    assert np.all(z["field"][inlet] == 0.0)  # the bolus has ended: inlet value back to 0


@pytest.mark.filterwarnings("ignore::RuntimeWarning")   # taylor_green imposes a non-zero pressure value (the ipcs plugin warns once)
def test_solvers_without_the_scalar_raise_before_device_work():
    from cfd_hemodynamic_amd.scenarios.taylor_green import TaylorGreenSimulation
    sc = TaylorGreenSimulation("ipcs_bdf2", 0.01, 0.02, nx=8, quiet=True)
    with pytest.raises(NotImplementedError, match="IPCS"):
        sc.solver.transport_enable()
    sc.setup()
    with pytest.raises(NotImplementedError):
        sc.solve(None, transport="age")
    from cfd_hemodynamic_amd.scenarios.dfg_1 import DFG1Benchmark
    g = DFG1Benchmark("stabilized_schur_backflow", 0.01, 0.02, m=6, quiet=True, v_max=0.3, p_grade=2, beta_backflow=0.2)
    with pytest.raises(NotImplementedError, match="generic"):
        g.solver.transport_step()
    assert g.solver.ctx.info(_lib.INFO_SCALAR_ENABLED) == 0
