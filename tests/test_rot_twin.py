"""The rotational form of the pressure-driven solvers (stabilized_schur_pressurebc.py:123-205) in its NumPy twin (tests/rot_twin.py)
and the host-side checks of the two plugins -- no GPU needed."""
import numpy as np
import pytest

from cfd_hemodynamic_amd.mesh import create_unit_square
from gen_util import ETYPE, facet_node_set, node_mesh
from oracle import np_twin as T, np_twin_gen as G
import rot_twin as RT


def _ends(m, kind=None, distort=0.0):
    """Left / right ends and walls of a (distorted) node_mesh or channel, from the undistorted end vertices of each facet."""
    x = m.x[np.asarray(m.facet_vertices)[:, :2]]                 # [facet, 2 vertices, 2]
    x0 = x[..., 0] - distort * (x[..., 1] if kind == "Q1" else np.sin(3.0 * x[..., 1]))
    left = np.nonzero(np.all(np.isclose(x0, x0.min()), axis=1))[0]
    right = np.nonzero(np.all(np.isclose(x0, x0.max()), axis=1))[0]
    return left, right, np.setdiff1d(np.arange(m.num_facets), np.concatenate([left, right]))


@pytest.mark.parametrize("kind", ["P1", "P2", "Q1"])
def test_jacobian_is_the_derivative_of_the_residual(kind):
    """Exact Jacobian = central differences of the residual: wall Dirichlet nodes, two pressure boundaries with different values,
    beta != 0, random state and history, the midpoint scheme."""
    m = node_mesh(kind, 3, distort=0.1)
    nv = m.num_vertices
    prm = T.Params(0.05, 1.3, 0.04, (0.2, -0.1))
    pb = RT.Problem(ETYPE[kind], m.x, m.cells, m.facet_cells, m.facet_local, prm)
    left, right, walls = _ends(m, kind, 0.1)
    assert len(left) == len(right) == (4 if kind == "Q1" else 3)
    pb.set_pressure_boundaries([left, right], [1.7, -0.4], beta=30.0)
    rng = np.random.default_rng(0)
    wn = facet_node_set(m, walls)
    g = rng.standard_normal((len(wn), 2))
    pb.add_bc_u(wn, g)
    xv, un = 0.3 * rng.standard_normal(3 * nv), 0.3 * rng.standard_normal((nv, 2))
    xv[: 2 * nv].reshape(-1, 2)[wn] = g  # the lifting vanishes at the base point
    F, J = pb.assemble(xv, un)
    J = J.toarray()
    Jfd = np.empty_like(J)
    e = 1e-6
    for k in range(3 * nv):
        d = np.zeros(3 * nv)
        d[k] = e
        Jfd[:, k] = (pb.assemble(xv + d, un, want_jac=False)[0] - pb.assemble(xv - d, un, want_jac=False)[0]) / (2 * e)
    assert np.abs(J - Jfd).max() <= 1e-7 * np.abs(J).max()
    # the pressure values enter the residual only
    pb.set_pressure_boundaries([left, right], [0.3, 2.5], beta=30.0)
    F2, J2 = pb.assemble(xv, un)
    assert np.abs(F2 - F).max() > 0 and abs(J2.toarray() - J).max() == 0.0


def _channel(n, L=4.0):
    m = create_unit_square(4 * n, n)
    m.x[:, 0] *= L
    return m


def test_pressure_driven_channel_tends_to_poiseuille():
    """Straight channel H = 1, L = 4 at Re ~ 1e-3, walls no-slip, natural pressures p_in / 2 and p_out / 2 (the reference's halving):
    the steady flow rate tends to Q = dP H^3 / (12 mu L) with dP = (p_in - p_out) / 2, second order in h."""
    L, mu, rho, p_in, p_out = 4.0, 1.0, 0.01, 8.0, 0.0
    q_exact = (p_in - p_out) / 2 / (12 * mu * L)
    errs = []
    for n in (4, 8, 16):
        m = _channel(n, L)
        nv = m.num_vertices
        # backward Euler with a very large step: three steps reach the steady state
        prm = T.Params(1e6, rho, mu, (0.0, 0.0), theta=1.0)
        pb = RT.Problem(G.P1_TRI, m.x, m.cells, m.facet_cells, m.facet_local, prm)
        left, right, walls = _ends(m)
        pb.set_pressure_boundaries([left, right], [p_in / 2, p_out / 2], beta=100.0)
        wn = facet_node_set(m, walls)
        pb.add_bc_u(wn, np.zeros((len(wn), 2)))
        x, un = np.zeros(3 * nv), np.zeros((nv, 2))
        for _ in range(3):
            x, _ = pb.newton(x, un)
            un = x[: 2 * nv].reshape(-1, 2).copy()
        q_out, q_in = pb.flux(x, right), -pb.flux(x, left)
        assert abs(q_out - q_in) <= 1e-10 * q_out  # mass is conserved through the channel
        errs.append(abs(q_out - q_exact) / q_exact)
    # measured: 0.293, 0.0767, 0.0194 (n = 4, 8, 16)
    assert errs[0] > errs[1] > errs[2] and errs[2] < 0.025, errs


class _Comm:
    size, rank = 2, 0


@pytest.mark.parametrize("name,kw,msg", [
    ("stabilized_schur_pressurebc", dict(p_outlet=10.0), "p_inlet and p_outlet are required"),
    ("stabilized_schur_pressurebc", dict(p_inlet=10.0), "p_inlet and p_outlet are required"),
    ("stabilized_schur_vascularbc", dict(R_resistance=1.0), "p_inlet is required"),
    ("stabilized_schur_vascularbc", dict(p_inlet=10.0), "R_resistance is required"),
])
def test_missing_pressure_arguments_raise_before_a_context_exists(name, kw, msg):
    """ValueError texts of stabilized_schur_pressurebc.py:59-63 / stabilized_schur_vascularbc.py:70-79, raised before any device
    work (without a GPU a context would fail with RuntimeError instead)."""
    from importlib import import_module
    Solver = import_module("cfd_hemodynamic_amd.solvers." + name).Solver
    with pytest.raises(ValueError, match=msg):
        Solver(create_unit_square(2), 0.01, 1.0, 0.01, [0.0, 0.0], **kw)


@pytest.mark.parametrize("name,kw", [("stabilized_schur_pressurebc", dict(p_inlet=1.0, p_outlet=0.0)),
                                     ("stabilized_schur_vascularbc", dict(p_inlet=1.0, R_resistance=2.0))])
def test_partitioned_runs_are_refused_before_a_context_exists(name, kw):
    from importlib import import_module
    Solver = import_module("cfd_hemodynamic_amd.solvers." + name).Solver
    with pytest.raises(NotImplementedError, match="partitioned"):
        Solver(create_unit_square(2), 0.01, 1.0, 0.01, [0.0, 0.0], comm=_Comm(), **kw)


@pytest.mark.parametrize("extra,expect", [
    (dict(), dict(p_inlet=75.0 * 133.322, p_outlet=10.0 * 133.322, beta_nitsche=100.0)),
    (dict(p_inlet=10.6, p_outlet=10.0, beta_nitsche=50.0), dict(p_inlet=10.6 * 133.322, p_outlet=10.0 * 133.322, beta_nitsche=50.0)),
    (dict(p_inlet=80.0, R_resistance=3.5), dict(p_inlet=80.0 * 133.322, R_resistance=3.5, initial_ffr=0.8)),
])
def test_stenosis_forwards_pressures_in_pascal(monkeypatch, extra, expect):
    """stenosis.py:84-99: mmHg -> Pa; with R_resistance, R_resistance and initial_ffr replace p_outlet."""
    from cfd_hemodynamic_amd.scenario import Scenario
    from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
    seen = {}

    class _Stop(Exception):
        pass

    def capture(self, cls, positional, keywords):
        seen.update(keywords)
        raise _Stop()

    monkeypatch.setattr(Scenario, "_build_solver", capture)
    with pytest.raises(_Stop):
        StenosisSimulation("stabilized_schur", 0.01, 0.02, ny=4, quiet=True, **extra)
    for k, v in expect.items():
        assert seen[k] == pytest.approx(v, rel=1e-15), k
    assert ("p_outlet" in seen) == ("R_resistance" not in extra)
