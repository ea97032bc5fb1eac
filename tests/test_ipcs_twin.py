"""The NumPy/SciPy twin of the pressure-correction scheme (tests/ipcs_twin.py) pinned without a GPU: operator identities on
triangles and tetrahedra, the Taylor-Green table, steady Poiseuille flow, density scaling and the force term, and what the
`ipcs_bdf2` plugin and `SolverBase` accept and refuse."""
import numpy as np
import pytest

import ipcs_twin as T

from cfd_hemodynamic_amd.elements import NodeMesh, NodeMesh3D, create_box, create_rectangle
from cfd_hemodynamic_amd.mesh import create_unit_square
from cfd_hemodynamic_amd.mesh3d import create_unit_cube
from cfd_hemodynamic_amd.solverBase import SolverBase


def _node_mesh(dim):
    if dim == 2:
        m = create_unit_square(5, 4)
        return m, NodeMesh(m), 1.0
    m = create_unit_cube(3)
    return m, NodeMesh3D(m), 1.0


@pytest.mark.parametrize("dim", [2, 3])
def test_operator_identities(dim):
    m, nm, vol = _node_mesh(dim)
    op = T.Operators(nm.x, nm.cells, m.num_vertices)
    rng = np.random.default_rng(3)
    one = np.ones(op.nn)
    w = rng.standard_normal((op.nn, dim))
    N = op.N(w)
    assert np.abs(op.K @ one).max() <= 1e-12 * abs(op.K).max()
    assert np.abs(N @ one).max() <= 1e-12 * abs(N).max()
    assert abs(op.M.sum() - vol) <= 1e-13
    assert abs(op.Mp.sum() - vol) <= 1e-13
    # B_d of a linear velocity field = its divergence tested against psi; G_d of a linear pressure = its gradient tested against phi
    a = rng.standard_normal((dim, dim))
    u = nm.x[:, :dim] @ a.T                       # u_i = a_ij x_j, div u = trace a
    psi_int = np.asarray(op.Mp.sum(axis=1)).ravel()
    div = sum(op.B[k] @ u[:, k] for k in range(dim))
    assert np.abs(div - np.trace(a) * psi_int).max() <= 1e-13
    g = rng.standard_normal(dim)
    p = m.x[:, :dim] @ g
    for k in range(dim):
        assert np.abs(op.G[k] @ p - g[k] * op.m1).max() <= 1e-13
        assert abs(op.B[k].T - (-op.G[k])).max() > 1e-3    # no integration by parts hidden in the pair (boundary terms differ)


def _header_rule(dim):
    """The degree-13 rule of include/cfdh_quad_tri.h / cfdh_quad_tet.h (weights summing to 1, barycentric points): other points
    than the twin's collapsed Gauss rule."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "cfdh_quad_tri.h" if dim == 2 else "cfdh_quad_tet.h")).read()
    num = r"[-+]?\d\.\d+e[-+]\d+"
    wsrc, lsrc = re.search(r"Q?W\[\w+\] = \{(.*?)\};", src, re.S).group(1), re.search(r"QL\[\w+\]\[\d\] = \{(.*?)\};", src, re.S).group(1)
    w = np.array([float(v) for v in re.findall(num, wsrc)])
    lam = np.array([float(v) for v in re.findall(num, lsrc)]).reshape(-1, dim + 1)
    assert len(w) == len(lam) and abs(w.sum() - 1.0) < 1e-14 and np.abs(lam.sum(axis=1) - 1.0).max() < 1e-14
    return lam, w / (2.0 if dim == 2 else 6.0)


def _nodal_p2(dim):
    """P2 nodal basis from the Vandermonde matrix of the monomials of degree <= 2 at the reference nodes (vertices, then the edge
    midpoints in the local edge order): returns functions giving the values [nq, nloc] and reference gradients [nq, nloc, dim]."""
    edges = T.TRI_EDGES if dim == 2 else T.TET_EDGES
    verts = np.vstack([np.zeros(dim), np.eye(dim)])
    nodes = np.vstack([verts, [0.5 * (verts[i] + verts[j]) for i, j in edges]])
    expo = [e for e in np.ndindex(*(3,) * dim) if sum(e) <= 2]

    def mono(x):
        return np.stack([np.prod(x ** np.array(e), axis=1) for e in expo], 1)

    def dmono(x, k):
        cols = []
        for e in expo:
            e2 = np.array(e)
            c = e2[k]
            e2[k] = max(c - 1, 0)
            cols.append(c * np.prod(x ** e2, axis=1))
        return np.stack(cols, 1)

    C = np.linalg.inv(mono(nodes))                      # column a: coefficients of phi_a
    return (lambda x: mono(x) @ C), (lambda x: np.stack([dmono(x, k) @ C for k in range(dim)], 2))


@pytest.mark.parametrize("dim", [2, 3])
def test_convection_matrix_against_a_literal_quadrature(dim):
    """N(w) cell by cell with a rule and a basis written independently of the twin's: the degree-13 tables of include/ and a nodal
    basis obtained by inverting a Vandermonde matrix in reference coordinates (the integrand has degree 5)."""
    m, nm, _ = _node_mesh(dim)
    op = T.Operators(nm.x, nm.cells, m.num_vertices)
    rng = np.random.default_rng(5)
    w = rng.standard_normal((op.nn, dim))
    lam, wt = _header_rule(dim)
    xi = lam[:, 1:]                                             # reference coordinates
    val, grad = _nodal_p2(dim)
    phi, dphi = val(xi), grad(xi)
    assert np.abs(phi.sum(axis=1) - 1.0).max() < 1e-13
    N = np.zeros((op.nn, op.nn))
    for cv in nm.cells:
        X = nm.x[cv[: dim + 1], :dim]
        J = (X[1:] - X[0]).T                                   # x = x0 + J xi
        Ji = np.linalg.inv(J)
        det = abs(np.linalg.det(J))
        for q in range(len(wt)):
            gphi = dphi[q] @ Ji                                 # d phi / d x = d phi / d xi . d xi / d x
            wq = phi[q] @ w[cv]
            N[np.ix_(cv, cv)] += wt[q] * det * np.outer(phi[q], gphi @ wq)
    assert np.abs(op.N(w).toarray() - N).max() <= 1e-12 * np.abs(N).max()


# the prototype's table (issue): nx, dt -> relative L2 velocity error at T = 0.2
TG = {(8, 0.02): 2.51e-2, (16, 0.01): 1.21e-3, (32, 0.005): 1.20e-4}
_tg_cache = {}


def _tg(nx, dt, **kw):
    key = (nx, dt, tuple(sorted(kw.items())))
    if key not in _tg_cache:
        _tg_cache[key] = T.taylor_green(nx, dt, **kw)[:3]
    return _tg_cache[key]


def test_taylor_green_reproduces_the_prototype_and_converges():
    err = {k: _tg(*k)[0] for k in TG}
    for k, ref in TG.items():
        assert abs(err[k] - ref) <= 0.05 * ref, (k, err[k], ref)
    assert err[(8, 0.02)] / err[(16, 0.01)] >= 8
    assert err[(16, 0.01)] / err[(32, 0.005)] >= 6


def test_iterative_solves_agree_with_direct_solves():
    d = T.taylor_green(8, 0.02)
    i = T.taylor_green(8, 0.02, tol=1e-12)
    assert abs(d[0] - i[0]) <= 1e-8 * d[0]
    assert all(k > 0 for k in i[3].its)


def _steady(tw, nmax):
    for s in range(nmax):
        tw.step()
        chg = np.abs(tw.u_sol - tw.u_prev).max() / tw.dt
        tw.advance()
        if chg < 1e-10:
            return s + 1
    return nmax


def test_poiseuille_flow_is_held_exactly():
    m = create_unit_square(8, 8)
    nm = NodeMesh(m)
    x, mu = nm.x, 0.05
    inlet = np.nonzero(np.abs(x[:, 0]) < 1e-12)[0]
    walls = np.nonzero((np.abs(x[:, 1]) < 1e-12) | (np.abs(x[:, 1] - 1) < 1e-12))[0]
    outlet = np.nonzero(np.abs(m.x[:, 0] - 1) < 1e-12)[0]
    uin = np.stack([4 * x[inlet, 1] * (1 - x[inlet, 1]), 0 * inlet], 1)
    tw = T.Twin(nm.x, nm.cells, m.num_vertices, 0.01, 1.0, mu, bcu=[(inlet, uin), (walls, np.zeros((len(walls), 2)))],
                bcp=[(outlet, np.zeros(len(outlet)))])
    steps = _steady(tw, 4000)
    assert steps < 4000
    uex = np.stack([4 * x[:, 1] * (1 - x[:, 1]), 0 * x[:, 0]], 1)
    pex = 8 * mu * (1 - m.x[:, 0])
    assert np.abs(tw.u_sol - uex).max() <= 1e-9
    assert np.abs(tw.p - pex).max() / np.abs(pex).max() <= 1e-9


def test_density_scaling_and_the_consistent_switch():
    for nx, dt in ((8, 0.02), (16, 0.01)):
        e1 = _tg(nx, dt)
        e2 = _tg(nx, dt, rho=2.0, mu=2.0 / 50.0)
        assert abs(e2[0] - e1[0]) <= 1e-9 * e1[0], (nx, e1[0], e2[0])
    lit = _tg(16, 0.01, rho=2.0, mu=2.0 / 50.0, consistent=False)
    assert lit[1] >= 5.0 * _tg(16, 0.01, rho=2.0, mu=2.0 / 50.0)[1]


def _hydrostatic(consistent):
    m = create_unit_square(8, 8)
    nm = NodeMesh(m)
    bnd = np.unique(nm.facet_vertices.ravel())
    tw = T.Twin(nm.x, nm.cells, m.num_vertices, 0.01, 2.0, 0.05, f=(0.0, -1.0), consistent=consistent,
                bcu=[(bnd, np.zeros((len(bnd), 2)))], bcp=[(np.array([0]), np.zeros(1))])
    steps = _steady(tw, 4000)
    return m, tw, steps


def test_force_term_gives_the_hydrostatic_pressure():
    m, tw, steps = _hydrostatic(True)
    assert steps < 4000
    pex = -2.0 * m.x[:, 1]
    pex, pp = pex - pex.mean(), tw.p - tw.p.mean()
    assert np.abs(tw.u_sol).max() <= 1e-9
    assert np.abs(pp - pex).max() / np.abs(pex).max() <= 1e-9
    # the literal coefficients: dp/dy comes out as +1 instead of -rho
    m, tw, _ = _hydrostatic(False)
    slope = np.polyfit(m.x[:, 1], tw.p, 1)[0]
    assert slope > 0 and abs(slope - 1.0) <= 1e-6


class _Spaces(SolverBase):
    def __init__(self, mesh):
        super().__init__(mesh, 0.1, 1.0, 1.0, [0.0] * mesh.geometry.dim)

    def setup(self, bcu, bcp):
        pass

    def solveStep(self):
        pass


@pytest.mark.parametrize("dim", [2, 3])
def test_solver_base_accepts_taylor_hood_on_simplices(dim):
    m = create_unit_square(3, 3) if dim == 2 else create_unit_cube(2)
    s = _Spaces(m)
    s.initVelocitySpace("Lagrange", m.topology.cell_name(), 2, shape=(dim,))
    s.initPressureSpace("Lagrange", m.topology.cell_name(), 1)
    nn = s.V.dofmap.index_map.size_global
    assert s.Q.dofmap.index_map.size_global == m.num_vertices < nn
    assert s.Q.mesh is m and np.array_equal(s.V.mesh.x[: m.num_vertices], m.x)
    assert s.u_sol.x.array.size == dim * nn and s.p_sol.x.array.size == m.num_vertices
    # equal order stays as it is; (1, 2) is still refused
    e = _Spaces(m)
    e.initVelocitySpace("Lagrange", m.topology.cell_name(), 2, shape=(dim,))
    e.initPressureSpace("Lagrange", m.topology.cell_name(), 2)
    assert e.Q.dofmap.index_map.size_global == nn
    r = _Spaces(m)
    r.initVelocitySpace("Lagrange", m.topology.cell_name(), 1, shape=(dim,))
    with pytest.raises(ValueError):
        r.initPressureSpace("Lagrange", m.topology.cell_name(), 2)


@pytest.mark.parametrize("dim", [2, 3])
def test_solver_base_refuses_degree_two_on_tensor_cells(dim):
    m = create_rectangle((0, 0), (1, 1), (2, 2)) if dim == 2 else create_box((0, 0, 0), (1, 1, 1), (2, 2, 2))
    s = _Spaces(m)
    with pytest.raises(NotImplementedError):
        s.initVelocitySpace("Lagrange", m.topology.cell_name(), 2, shape=(dim,))


def test_plugin_refusals_come_before_any_device_work(monkeypatch):
    from cfd_hemodynamic_amd import _lib
    from cfd_hemodynamic_amd.solvers import ipcs_bdf2

    def boom(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(_lib, "IpcsContext", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    with pytest.raises(NotImplementedError, match="quadrilateral"):
        ipcs_bdf2.Solver(create_rectangle((0, 0), (1, 1), (2, 2)), 0.1, 1.0, 1.0, [0, 0])
    with pytest.raises(NotImplementedError, match="hexahedron"):
        ipcs_bdf2.Solver(create_box((0, 0, 0), (1, 1, 1), (2, 2, 2)), 0.1, 1.0, 1.0, [0, 0, 0])

    class Comm:
        size = 2

    with pytest.raises(NotImplementedError, match="one GPU"):
        ipcs_bdf2.Solver(create_unit_square(2, 2), 0.1, 1.0, 1.0, [0, 0], comm=Comm())
