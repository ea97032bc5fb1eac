"""The rotational form of the pressure-driven solvers in 3-D (stabilized_schur_pressurebc.py:111-121, :123-205) in its NumPy twin
(tests/rot_twin3.py) and the host-side refusals of the two plugins on 3-D meshes -- no GPU needed."""
import numpy as np
import pytest

from cfd_hemodynamic_amd.elements import NodeMesh3D, create_box
from cfd_hemodynamic_amd.mesh3d import Mesh3D, _voxel_tets, create_unit_cube
from gen3_util import ETYPE3, facet_node_set3, node_mesh3
from oracle import np_twin_nd as TN
import rot_twin3 as RT3

SQUARE_DUCT = 0.0351443   # Q = SQUARE_DUCT a^4 dP / (mu L): fully developed flow in a square duct of side a


def ends3(m, kind=None, distort=0.0):
    """Facets at the smallest / largest undistorted x (node_mesh3 shears x by y and y by z / 2 on Q1, x by z on tetrahedra) and
    the rest."""
    x = m.x[np.asarray(m.facet_vertices)[:, :3]]                  # [facet, 3 vertices, 3]
    x0 = x[..., 0] - distort * ((x[..., 1] - 0.5 * distort * x[..., 2]) if kind == "Q1" else x[..., 2])
    left = np.nonzero(np.all(np.isclose(x0, x0.min()), axis=1))[0]
    right = np.nonzero(np.all(np.isclose(x0, x0.max()), axis=1))[0]
    return left, right, np.setdiff1d(np.arange(m.num_facets), np.concatenate([left, right]))


def duct(kind, nx, n, L):
    """[0, L] x [0, 1]^2 with nx x n x n bricks: hexahedra (Q1) or six Kuhn tetrahedra per brick (P1 / P2)."""
    if kind == "Q1":
        return create_box((0.0, 0.0, 0.0), (L, 1.0, 1.0), (nx, n, n), cell_type="hexahedron")
    xs, ys, zs = np.linspace(0.0, L, nx + 1), np.linspace(0.0, 1.0, n + 1), np.linspace(0.0, 1.0, n + 1)
    cells, pts = _voxel_tets(np.ones((nx, n, n), bool), xs, ys, zs)
    m = Mesh3D(cells, pts, name="duct")
    return m if kind == "P1" else NodeMesh3D(m)


@pytest.mark.parametrize("kind", ["P1", "P2", "Q1"])
@pytest.mark.parametrize("scheme", [dict(), dict(theta=1.0, a0=1.5, a1=-2.0, a2=0.5)])
def test_jacobian_is_the_derivative_of_the_residual(kind, scheme):
    """Exact Jacobian = central differences of the residual on distorted cells: Dirichlet data on part of the walls, two pressure
    boundaries with different values, beta != 0, random state and history, midpoint and BDF2 coefficients."""
    n = 1 if kind == "P2" else 2
    m = node_mesh3(kind, n, distort=0.1)
    nv = m.num_vertices
    prm = TN.Params(0.05, 1.3, 0.04, (0.2, -0.1, 0.3), **scheme)
    pb = RT3.Problem(ETYPE3[kind], m.x, m.cells, m.facet_cells, m.facet_local, prm)
    left, right, walls = ends3(m, kind, 0.1)
    assert len(left) == len(right) > 0
    pb.set_pressure_boundaries([left, right], [1.7, -0.4], beta=30.0)
    rng = np.random.default_rng(0)
    wn = facet_node_set3(m, walls)[::2]
    g = rng.standard_normal((len(wn), 3))
    pb.add_bc_u(wn, g)
    xv, un, un2 = 0.3 * rng.standard_normal(4 * nv), 0.3 * rng.standard_normal((nv, 3)), 0.3 * rng.standard_normal((nv, 3))
    xv[: 3 * nv].reshape(-1, 3)[wn] = g  # the lifting vanishes at the base point
    F, J = pb.assemble(xv, un, un2=un2)
    J = J.toarray()
    Jfd = np.empty_like(J)
    e = 1e-6
    for k in range(4 * nv):
        d = np.zeros(4 * nv)
        d[k] = e
        Jfd[:, k] = (pb.assemble(xv + d, un, want_jac=False, un2=un2)[0] - pb.assemble(xv - d, un, want_jac=False, un2=un2)[0]) / (2 * e)
    assert np.abs(J - Jfd).max() <= 1e-7 * np.abs(J).max()
    # the pressure values enter the residual only
    pb.set_pressure_boundaries([left, right], [0.3, 2.5], beta=30.0)
    F2, J2 = pb.assemble(xv, un, un2=un2)
    assert np.abs(F2 - F).max() > 0 and abs(J2.toarray() - J).max() == 0.0


def _duct_flow_rate(kind, n, L=0.25, mu=1.0, rho=0.01, p_in=8.0, p_out=0.0):
    m = duct(kind, 1, n, L)
    nv = m.num_vertices
    # backward Euler with a very large step: three steps reach the steady state
    prm = TN.Params(1e6, rho, mu, (0.0, 0.0, 0.0), theta=1.0)
    pb = RT3.Problem(ETYPE3[kind], m.x, m.cells, m.facet_cells, m.facet_local, prm)
    left, right, walls = ends3(m)
    pb.set_pressure_boundaries([left, right], [p_in / 2, p_out / 2], beta=100.0)
    wn = facet_node_set3(m, walls)
    pb.add_bc_u(wn, np.zeros((len(wn), 3)))
    x, un = np.zeros(4 * nv), np.zeros((nv, 3))
    for _ in range(3):
        x, _ = pb.newton(x, un)
        un = x[: 3 * nv].reshape(-1, 3).copy()
    q_out, q_in = pb.flux(x, right), -pb.flux(x, left)
    assert abs(q_out - q_in) <= 1e-10 * q_out  # mass is conserved through the duct
    return q_out, SQUARE_DUCT * (p_in - p_out) / 2 / (mu * L)


def test_pressure_driven_duct_tends_to_the_square_duct_flow_rate():
    """Square duct a = 1 in the Stokes regime (rho = 0.01, mu = 1), walls no-slip, natural pressures p_in / 2 and p_out / 2 (the
    reference's halving), one cell along the flow (the flow is x-invariant): on Q1 the flow rate tends to
    Q = 0.0351443 a^4 dP / (mu L), dP = (p_in - p_out) / 2, under cross-section refinement, second order in h."""
    errs = []
    for n in (2, 4, 8):
        q, q_exact = _duct_flow_rate("Q1", n)
        errs.append(abs(q - q_exact) / q_exact)
    # measured: 0.333, 0.0902, 0.0231 (n = 2, 4, 8); the same for L = 0.01
    assert errs[0] > errs[1] > errs[2] and errs[2] < 0.025, errs


def test_p2_duct_conserves_mass():
    """The same duct on P2 tetrahedra: inflow = outflow to 1e-10 (inside _duct_flow_rate), flow down the pressure drop.  The P2
    flow rate does NOT tend to the square-duct value in this setting (relative errors measured with one cell along the flow:
    0.63, 1.09, 0.69 for n = 1, 2, 4, and they depend on L and on the axial resolution), so only conservation is pinned here."""
    for n in (1, 2):
        q, _ = _duct_flow_rate("P2", n)
        assert q > 0


class _Comm:
    size, rank = 2, 0


def _hex_mesh():
    return create_box((0.0, 0.0, 0.0), (2.0, 1.0, 1.0), (2, 1, 1), cell_type="hexahedron")


@pytest.mark.parametrize("name,kw", [("stabilized_schur_pressurebc", dict(p_inlet=1.0, p_outlet=0.0)),
                                     ("stabilized_schur_vascularbc", dict(p_inlet=1.0, R_resistance=2.0))])
def test_p1_tetrahedra_are_refused_before_a_context_exists(name, kw):
    """P1 tetrahedra run on the closed-form kernels, which have no rotational variant: NotImplementedError (not the RuntimeError a
    context would raise without a GPU), pointing to p_grade=2 or hexahedra."""
    from importlib import import_module
    Solver = import_module("cfd_hemodynamic_amd.solvers." + name).Solver
    with pytest.raises(NotImplementedError, match="p_grade=2"):
        Solver(create_unit_cube(1), 0.01, 1.0, 0.01, [0.0, 0.0, 0.0], **kw)
    with pytest.raises(NotImplementedError, match="hexahedra"):
        Solver(create_unit_cube(1), 0.01, 1.0, 0.01, [0.0, 0.0, 0.0], p_grade=1, **kw)


@pytest.mark.parametrize("name,kw", [("stabilized_schur_pressurebc", dict(p_inlet=1.0, p_outlet=0.0)),
                                     ("stabilized_schur_vascularbc", dict(p_inlet=1.0, R_resistance=2.0))])
@pytest.mark.parametrize("mesh", ["hexahedron", "tetrahedron"])
def test_partitioned_3d_runs_are_refused_before_a_context_exists(name, kw, mesh):
    from importlib import import_module
    Solver = import_module("cfd_hemodynamic_amd.solvers." + name).Solver
    m = _hex_mesh() if mesh == "hexahedron" else create_unit_cube(1)
    with pytest.raises(NotImplementedError, match="partitioned"):
        Solver(m, 0.01, 1.0, 0.01, [0.0, 0.0, 0.0], comm=_Comm(), p_grade=2 if mesh == "tetrahedron" else 1, **kw)
