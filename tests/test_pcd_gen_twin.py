"""CPU checks of the quadrature twin of the PCD operator on the degree-1 generic elements (tests/pcd_gen_twin.py) -- against the exact
simplex twin (tests/pcd_twin.py) on triangles, against identities of the operator on sheared Q1 cells -- and the refusals of the
`stabilized_pcd_pressurebc` / `stabilized_pcd_bdf2` plugins (no GPU needed)."""
import numpy as np
import pytest

import pcd_gen_twin as PG
import pcd_twin as P
from cfd_hemodynamic_amd.elements import create_box, create_rectangle
from cfd_hemodynamic_amd.mesh import create_unit_square
from cfd_hemodynamic_amd.mesh3d import create_unit_cube

# fixed non-symmetric affine maps (parallelograms / parallelepipeds)
A2 = np.array([[1.3, 0.35], [-0.2, 0.9]])
A3 = np.array([[1.3, 0.35, -0.15], [-0.2, 0.9, 0.25], [0.1, -0.3, 1.1]])


def _mesh(kind):
    if kind == "tri":
        m = create_unit_square(7, 5)
        m.x[:, 0] *= 1.7
    elif kind == "quad":
        m = create_rectangle((0.0, 0.0), (1.0, 0.8), (5, 4))
    else:
        m = create_box((0.0, 0.0, 0.0), (1.0, 0.8, 0.6), (3, 2, 2))
    inlet = np.flatnonzero(np.isclose(m.x[np.asarray(m.facet_vertices)][:, :, 0], 0.0).all(axis=1))
    marker = np.zeros(len(m.facet_cells), dtype=np.int32)
    marker[inlet] = 2
    if kind != "tri":
        m.x[:] = m.x @ (A2 if kind == "quad" else A3).T
    return m, marker


def _rowrel(A, B):
    D = (A - B).tocsr()
    rowmax = np.asarray(abs(B).max(axis=1).todense()).ravel()
    return (np.asarray(abs(D).max(axis=1).todense()).ravel() / rowmax).max()


def test_quadrature_twin_equals_the_exact_simplex_twin_on_triangles():
    m, marker = _mesh("tri")
    rng = np.random.default_rng(4)
    w = rng.standard_normal((m.num_vertices, 2))
    Kq = PG.pcd_operator("tri", m.x, m.cells, m.facet_cells, m.facet_local, marker, 2, w, 1.3, 7.0)
    Ke = P.pcd_operator(m.x, m.cells, m.facet_cells, m.facet_local, marker, 2, w, 1.3, 7.0)
    assert _rowrel(Kq, Ke) <= 1e-13
    md = P.mass_diag(m.x, m.cells)
    assert np.abs(PG.mass_diag("tri", m.x, m.cells) - md).max() <= 1e-13 * md.max()
    assert _rowrel(PG.laplacian("tri", m.x, m.cells), P.laplacian(m.x, m.cells)) <= 1e-13
    Bq = PG.facet_matrix("tri", m.x, m.cells, m.facet_cells, m.facet_local, w, np.arange(len(m.facet_cells)))
    Be = P.facet_matrix(m.x, m.cells, m.facet_cells, m.facet_local, w, np.arange(len(m.facet_cells)))
    assert abs(Bq - Be).max() <= 1e-13 * abs(Be).max()


@pytest.mark.parametrize("kind", ["quad", "hex"])
def test_k_of_a_linear_pressure_and_a_constant_velocity_on_sheared_q1_cells(kind):
    """c_t = 0: (N p)_a = (w . grad p) int phi_a for linear p and constant w, so K p = rho (w . grad p) int phi - rho R_in p."""
    m, marker = _mesh(kind)
    d = m.x.shape[1]
    rng = np.random.default_rng(1)
    wc, gp = rng.standard_normal(d), rng.standard_normal(d)
    w = np.tile(wc, (m.num_vertices, 1))
    p = m.x @ gp + 0.3
    rho = 1.3
    K = PG.pcd_operator(kind, m.x, m.cells, m.facet_cells, m.facet_local, marker, 2, w, rho, 0.0)
    R = PG.facet_matrix(kind, m.x, m.cells, m.facet_cells, m.facet_local, w, PG.marked_facets(marker, 2))
    M = PG.mass(kind, m.x, m.cells)
    phi_int = M @ np.ones(m.num_vertices)
    N = PG.convection(kind, m.x, m.cells, w)
    assert np.abs(N @ p - (wc @ gp) * phi_int).max() <= 1e-12 * np.abs((wc @ gp) * phi_int).max()
    expect = rho * (wc @ gp) * phi_int - rho * (R @ p)
    assert np.abs(K @ p - expect).max() <= 1e-12 * np.abs(expect).max()
    assert abs(R).sum() > 0  # the inlet term is present
    # the measure of the mapped box, M_d = diag(M), and a Laplacian that annihilates constants and reproduces |grad p|^2 |Omega|
    vol = abs(np.linalg.det(A2 if kind == "quad" else A3)) * (0.8 if kind == "quad" else 0.48)
    assert abs(phi_int.sum() - vol) <= 1e-13 * vol
    assert np.allclose(PG.mass_diag(kind, m.x, m.cells), M.diagonal(), rtol=1e-14)
    L = PG.laplacian(kind, m.x, m.cells)
    assert np.abs(L @ np.ones(m.num_vertices)).max() <= 1e-12 * abs(L).max()
    assert abs(p @ (L @ p) - (gp @ gp) * vol) <= 1e-12 * (gp @ gp) * vol


@pytest.mark.parametrize("kind", ["tri", "quad", "hex"])
def test_convection_plus_transpose_is_the_boundary_flux_matrix(kind):
    """Constant w: N + N^T = int_dOmega (w . n) phi_i phi_j."""
    m, _ = _mesh(kind)
    d = m.x.shape[1]
    wc = np.array([0.7, -1.2, 0.45])[:d]
    w = np.tile(wc, (m.num_vertices, 1))
    N = PG.convection(kind, m.x, m.cells, w)
    B = PG.facet_matrix(kind, m.x, m.cells, m.facet_cells, m.facet_local, w, np.arange(len(m.facet_cells)))
    assert abs(B).max() > 0
    assert np.abs((N + N.T - B).toarray()).max() <= 1e-12 * abs(B).max()


class _Comm:
    size, rank = 2, 0


def test_pressurebc_plugin_refuses_before_a_context():
    from cfd_hemodynamic_amd.solvers.stabilized_pcd_pressurebc import Solver
    tri, z2 = create_unit_square(2), [0.0, 0.0]
    with pytest.raises(ValueError, match="p_inlet and p_outlet are required for stabilized_pcd_pressurebc"):
        Solver(tri, 0.01, 1.0, 0.01, z2)
    with pytest.raises(ValueError, match="p_inlet and p_outlet are required"):
        Solver(tri, 0.01, 1.0, 0.01, z2, p_inlet=1.0)
    with pytest.raises(NotImplementedError, match="hexahedra"):
        Solver(create_unit_cube(1), 0.01, 1.0, 0.01, [0.0, 0.0, 0.0], p_inlet=1.0, p_outlet=0.0)
    with pytest.raises(NotImplementedError, match="p_grade"):
        Solver(tri, 0.01, 1.0, 0.01, z2, p_inlet=1.0, p_outlet=0.0, p_grade=2)
    meshes = ((tri, z2), (create_rectangle((0.0, 0.0), (1.0, 1.0), (2, 2)), z2),
              (create_box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1)), [0.0, 0.0, 0.0]))
    for mesh, f in meshes:
        with pytest.raises(NotImplementedError, match="partitioned"):
            Solver(mesh, 0.01, 1.0, 0.01, f, p_inlet=1.0, p_outlet=0.0, comm=_Comm())


def test_bdf2_plugin_refuses_what_stabilized_pcd_refuses_before_a_context():
    from cfd_hemodynamic_amd.solvers.stabilized_pcd_bdf2 import Solver
    with pytest.raises(NotImplementedError, match="stabilized_schur"):
        Solver(create_rectangle((0.0, 0.0), (1.0, 1.0), (2, 2)), 0.01, 1.0, 0.01, [0.0, 0.0])
    with pytest.raises(NotImplementedError, match="stabilized_schur"):
        Solver(create_box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1)), 0.01, 1.0, 0.01, [0.0, 0.0, 0.0])
    for mesh, f in ((create_unit_square(2), [0.0, 0.0]), (create_unit_cube(1), [0.0, 0.0, 0.0])):
        with pytest.raises(NotImplementedError, match="partitioned run.*stabilized_schur"):
            Solver(mesh, 0.01, 1.0, 0.01, f, comm=_Comm())


def test_bdf2_plugins_share_the_history_mixin():
    from cfd_hemodynamic_amd.solvers import stabilized_pcd_bdf2, stabilized_schur_bdf2
    from cfd_hemodynamic_amd.solvers._bdf2_history import Bdf2History
    for mod in (stabilized_pcd_bdf2, stabilized_schur_bdf2):
        assert issubclass(mod.Solver, Bdf2History) and mod.Solver.solveStep is Bdf2History.solveStep
        assert isinstance(mod.Solver.u_prev2, property)
