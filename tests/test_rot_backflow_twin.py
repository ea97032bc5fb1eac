"""The rotational form with per-boundary Nitsche switch and backflow stabilisation (the boundary terms of the reference's
stabilized_schur_vascularbc_backflow.py:214-244) in its NumPy twin (tests/rot_backflow_twin.py), and the host-side checks of the
plugin `stabilized_schur_vascularbc_backflow` -- no GPU needed."""
import numpy as np
import pytest

from cfd_hemodynamic_amd.mesh import create_unit_square
from cfd_hemodynamic_amd.mesh3d import create_unit_cube
from gen_util import ETYPE, node_mesh
from gen3_util import ETYPE3, node_mesh3
import rot_backflow_util as U
import rot_twin as RT
import rot_twin3 as RT3
from test_rot_twin import _ends
from test_rot_twin3 import ends3


def _fd_mesh(dim, kind):
    """The distorted meshes of the Jacobian checks of test_rot_twin.py / test_rot_twin3.py."""
    if dim == 2:
        m = node_mesh(kind, 3, distort=0.1)
        return m, _ends(m, kind, 0.1)
    m = node_mesh3(kind, 1, distort=0.1)   # six P2 tetrahedra / 1 x 2 x 1 hexahedra: the smallest with both ends and walls
    return m, ends3(m, kind, 0.1)


@pytest.mark.parametrize("dim,kind", U.KINDS, ids=U.IDS)
def test_switches_at_their_defaults_reproduce_the_rotational_twin(dim, kind):
    """Every Nitsche switch on, every beta_bf = 0: residual and Jacobian of rot_twin / rot_twin3, bit for bit."""
    m, (left, right, walls) = _fd_mesh(dim, kind)
    nv = m.num_vertices
    prm = U.params(dim, 0.05, scheme="bdf2")
    base = (RT.Problem if dim == 2 else RT3.Problem)((ETYPE if dim == 2 else ETYPE3)[kind], m.x, m.cells, m.facet_cells, m.facet_local,
                                                     U.params(dim, 0.05, scheme="bdf2"))
    base.set_pressure_boundaries([left, right], [1.7, -0.4], beta=30.0)
    xv, un, un2 = U.random_state(dim, nv, 0)
    F0, J0 = base.assemble(xv, un, un2=un2)
    for kw in (dict(), dict(nitsche=[1, 1], beta_backflow=[0.0, 0.0])):
        pb = U.twin(dim, kind, m, prm)
        pb.set_pressure_boundaries([left, right], [1.7, -0.4], beta=30.0, **kw)
        F, J = pb.assemble(xv, un, un2=un2)
        assert np.array_equal(F, F0) and np.array_equal(J.toarray(), J0.toarray())


@pytest.mark.parametrize("dim,kind", U.KINDS, ids=U.IDS)
@pytest.mark.parametrize("scheme", ["midpoint", "bdf2"])
def test_jacobian_is_the_derivative_of_the_residual(dim, kind, scheme):
    """Exact Jacobian = central differences of the residual (step and tolerance of test_rot_twin.py / test_rot_twin3.py): distorted
    cells, Dirichlet data on part of the walls, two pressure boundaries with Nitsche on / off and beta_bf = 0 / 0.2, random state
    and u_prev.  u_prev is data: the residual is smooth in u and the kink of (.)_- is not differentiated."""
    m, (left, right, walls) = _fd_mesh(dim, kind)
    nv = m.num_vertices
    pb = U.twin(dim, kind, m, U.params(dim, 0.05, scheme=scheme))
    pb.set_pressure_boundaries([left, right], [1.7, -0.4], beta=30.0, nitsche=[1, 0], beta_backflow=[0.0, 0.2])
    rng = np.random.default_rng(0)
    wn = U.wall_nodes(dim, m, walls)[::2]
    g = rng.standard_normal((len(wn), dim))
    pb.add_bc_u(wn, g)
    xv, un, un2 = U.random_state(dim, nv, 1)
    xv[: dim * nv].reshape(-1, dim)[wn] = g  # the lifting vanishes at the base point
    sn = pb.prev_normal_velocity(un, 1)
    assert (sn < 0).any() and (sn > 0).any()  # the term is active at some outlet points and switched off at others
    F, J = pb.assemble(xv, un, un2=un2)
    J = J.toarray()
    Jfd = np.empty_like(J)
    e = 1e-6
    for k in range(len(xv)):
        d = np.zeros(len(xv))
        d[k] = e
        Jfd[:, k] = (pb.assemble(xv + d, un, want_jac=False, un2=un2)[0] - pb.assemble(xv - d, un, want_jac=False, un2=un2)[0]) / (2 * e)
    assert np.abs(J - Jfd).max() <= 1e-7 * np.abs(J).max()
    # the term is seen by the check: without it the Jacobian differs by more than a hundred times the tolerance
    pb.set_pressure_boundaries([left, right], [1.7, -0.4], beta=30.0, nitsche=[1, 0], beta_backflow=[0.0, 0.0])
    assert np.abs(pb.assemble(xv, un, un2=un2)[1].toarray() - J).max() > 100 * 1e-7 * np.abs(J).max()


@pytest.mark.parametrize("dim,kind", U.KINDS, ids=U.IDS)
def test_backflow_block_is_symmetric_positive_semidefinite(dim, kind):
    """J(beta_bf = 0.2) - J(beta_bf = 0) at the same state: symmetric, smallest eigenvalue >= -1e-14 x the largest, confined to the
    velocity block; exactly zero when u_prev . n >= 0 at every outlet point."""
    m, (left, right, walls) = _fd_mesh(dim, kind)
    nv = m.num_vertices
    pb = U.twin(dim, kind, m, U.params(dim, 0.05))
    xv, un, _ = U.random_state(dim, nv, 2)

    def block(un):
        out = []
        for b in (0.2, 0.0):
            pb.set_pressure_boundaries([left, right], [1.7, -0.4], beta=30.0, nitsche=[1, 0], beta_backflow=[0.0, b])
            out.append(pb.assemble(xv, un)[1].toarray())
        return out[0] - out[1], np.abs(out[0]).max()

    B, jmax = block(un)
    assert (pb.prev_normal_velocity(un, 1) < 0).any() and np.abs(B).max() > 0
    # symmetric up to the rounding of the two sums it is the difference of: half an ulp of |J| per entry, two entries
    assert np.abs(B - B.T).max() <= np.finfo(float).eps * jmax
    assert np.abs(B[dim * nv:]).max() == 0.0 and np.abs(B[:, dim * nv:]).max() == 0.0
    ev = np.linalg.eigvalsh(0.5 * (B + B.T))
    assert ev[-1] > 0 and ev[0] >= -1e-14 * ev[-1]
    out = np.zeros((nv, dim))
    out[:, 0] = 1.0   # leaves through the right end everywhere
    assert (pb.prev_normal_velocity(out, 1) > 0).all()
    assert np.abs(block(out)[0]).max() == 0.0


# ---- the plugin, before any device work ----------------------------------------------------------------------------------------

class _Comm:
    size, rank = 2, 0


def _solver():
    from cfd_hemodynamic_amd.solvers.stabilized_schur_vascularbc_backflow import Solver
    return Solver


def test_missing_p_inlet_raises_before_a_context_exists():
    with pytest.raises(ValueError, match="p_inlet is required for stabilized_schur_vascularbc_backflow"):
        _solver()(create_unit_square(2), 0.01, 1.0, 0.01, [0.0, 0.0], R_resistance=1.0, beta_backflow=0.2)


def test_unsupported_runs_are_refused_before_a_context_exists():
    S = _solver()
    with pytest.raises(NotImplementedError, match="partitioned"):
        S(create_unit_square(2), 0.01, 1.0, 0.01, [0.0, 0.0], p_inlet=1.0, comm=_Comm())
    with pytest.raises(NotImplementedError, match="p_grade=2"):
        S(create_unit_cube(1), 0.01, 1.0, 0.01, [0.0, 0.0, 0.0], p_inlet=1.0)
    with pytest.raises(NotImplementedError, match="p_grade=3"):
        S(create_unit_square(2), 0.01, 1.0, 0.01, [0.0, 0.0], p_inlet=1.0, p_grade=3)
    with pytest.raises(ValueError, match="beta_backflow"):
        S(create_unit_square(2), 0.01, 1.0, 0.01, [0.0, 0.0], p_inlet=1.0, beta_backflow=-0.1)


@pytest.mark.parametrize("extra,expect", [
    (dict(p_inlet=80.0), dict(p_inlet=80.0 * 133.322)),
    (dict(p_inlet=80.0, beta_backflow=0.35, beta_nitsche=50.0), dict(p_inlet=80.0 * 133.322, beta_backflow=0.35, beta_nitsche=50.0)),
    (dict(p_inlet=80.0, R_resistance=3.5, initial_ffr=0.7), dict(p_inlet=80.0 * 133.322, initial_ffr=0.7)),
])
def test_stenosis_forwards_the_keywords_of_the_plugin(monkeypatch, extra, expect):
    """The stenosis scenario hands p_inlet (mmHg -> Pa), beta_backflow, beta_nitsche and -- together with R_resistance, as in the
    reference's stenosis.py:84-99 -- initial_ffr to the plugin; the plugin's constructor accepts everything the scenario sends."""
    import inspect
    from cfd_hemodynamic_amd.scenario import Scenario
    from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
    seen = {}

    class _Stop(Exception):
        pass

    def capture(self, cls, positional, keywords):
        seen.update(keywords)
        seen["cls"] = cls
        raise _Stop()

    monkeypatch.setattr(Scenario, "_build_solver", capture)
    with pytest.raises(_Stop):
        StenosisSimulation("stabilized_schur_vascularbc_backflow", 0.01, 0.02, ny=4, quiet=True, **extra)
    for k, v in expect.items():
        assert seen[k] == pytest.approx(v, rel=1e-15), k
    assert seen["cls"] is _solver()
    sig = inspect.signature(_solver().__init__).parameters
    assert sig["initial_ffr"].default == 0.8 and sig["beta_nitsche"].default == 100.0 and sig["beta_backflow"].default == 0.2
    assert sig["p_grade"].default == 1 and sig["p_inlet"].default is None and "v_max" in sig and "R_resistance" in sig


def test_command_line_reaches_the_plugin(monkeypatch):
    """--solver stabilized_schur_vascularbc_backflow --p_inlet .. --initial_ffr .. --beta_backflow .. on the command line of the
    package: the three values arrive in the scenario's keyword arguments."""
    import cfd_hemodynamic_amd.__main__ as M
    from cfd_hemodynamic_amd.scenario import Scenario
    seen = {}

    class _Stop(Exception):
        pass

    def capture(self, cls, positional, keywords):
        seen.update(keywords)
        raise _Stop()

    monkeypatch.setattr(Scenario, "_build_solver", capture)
    argv = ["simulate", "--simulation", "unit_square_pipe", "--T", "0.02", "--dt", "0.01", "--solver", "stabilized_schur_vascularbc_backflow", "--p_inlet", "8.85",
            "--p_outlet", "0.0", "--initial_ffr", "1.2", "--beta_backflow", "0.3"]
    with pytest.raises(_Stop):
        M.main(argv)
    assert seen["p_inlet"] == 8.85 and seen["initial_ffr"] == 1.2 and seen["beta_backflow"] == 0.3
