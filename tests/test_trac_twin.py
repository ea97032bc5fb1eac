"""The traction boundaries of the convective form (stabilized_schur_pressure_backflow.py:191-217) in their NumPy twin
(tests/trac_twin.py) -- no GPU needed."""
import numpy as np
import pytest

from oracle import np_twin_nd as TN
import trac_twin as TT
import trac_util as U

SQUARE_DUCT = 0.0351443   # Q = SQUARE_DUCT a^4 dP / (mu L), the constant of tests/test_rot_twin3.py
SCHEMES = [dict(), dict(theta=1.0, a0=1.5, a1=-2.0, a2=0.5)]


def _problem(d, scheme, shift=0.0, seed=0):
    mesh, rng = U.square(4, 3, seed) if d == 2 else U.cube(2, seed)
    nv = mesh.num_vertices
    marker = U.mark_ends(mesh)
    inl, out, wall = U.sets_of(marker)
    prm = TN.Params(0.05, 1.3, 0.04, (0.2, -0.1, 0.3), ds_terms=False, **scheme)
    pb = TT.Problem(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, prm)
    wn = U.wall_nodes(mesh, marker)[::2]
    g = rng.standard_normal((len(wn), d))
    pb.add_bc_u(wn, g)
    xv = 0.3 * rng.standard_normal((d + 1) * nv)
    un, un2 = 0.3 * rng.standard_normal((nv, d)), 0.3 * rng.standard_normal((nv, d))
    un[:, 0] += shift
    xv[: d * nv].reshape(-1, d)[wn] = g  # the lifting vanishes at the base point
    return pb, (inl, out, wall), xv, un, un2


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_jacobian_is_the_derivative_of_the_residual(d, scheme):
    """Exact Jacobian = central differences of the residual (step and bound of tests/test_rot_twin3.py): random state, midpoint
    and BDF2 coefficients, inlet with the tangential terms, outlet without, backflow term with u_prev . n of both signs on the
    outlet, one cell with facets of both boundaries."""
    pb, (inl, out, _), xv, un, un2 = _problem(d, scheme)
    pb.set_traction_boundaries([inl, out], [1.7, -0.4], beta=30.0, tangential=[1, 0], beta_backflow=[0.0, 0.4])
    fc, fl = pb.facet_cells[out], pb.facet_local[out]
    g, _, _ = TN.geometry(pb.x, pb.cells[fc])
    nrm = -g[np.arange(len(fc)), fl]
    s = np.einsum("cai,ci->ca", un[pb.cells[fc]], nrm)
    s = np.array([s[k, a] for k in range(len(fc)) for a in range(d + 1) if a != fl[k]])
    assert s.min() < 0 < s.max()
    n = len(xv)
    F, J = pb.assemble(xv, un, un2=un2)
    J = J.toarray()
    Jfd = np.empty_like(J)
    e = 1e-6
    for k in range(n):
        dx = np.zeros(n)
        dx[k] = e
        Jfd[:, k] = (pb.assemble(xv + dx, un, want_jac=False, un2=un2)[0] - pb.assemble(xv - dx, un, want_jac=False, un2=un2)[0]) / (2 * e)
    assert np.abs(J - Jfd).max() <= 1e-7 * np.abs(J).max()
    # the values enter the residual only
    pb.set_traction_boundaries([inl, out], [0.3, 2.5], beta=30.0, tangential=[1, 0], beta_backflow=[0.0, 0.4])
    F2, J2 = pb.assemble(xv, un, un2=un2)
    assert np.abs(F2 - F).max() > 0 and abs(J2.toarray() - J).max() == 0.0


@pytest.mark.parametrize("d", [2, 3])
def test_without_a_boundary_the_tensors_are_the_parents(d):
    pb, _, xv, un, un2 = _problem(d, SCHEMES[1])
    ref = TN.Problem(pb.x, pb.cells, pb.facet_cells, pb.facet_local, pb.prm)
    ref.isbc, ref.bcval, ref.bcmult = pb.isbc, pb.bcval, pb.bcmult
    F, J = pb.assemble(xv, un, un2=un2)
    Fr, Jr = ref.assemble(xv, un, un2=un2)
    assert np.array_equal(F, Fr) and (J != Jr).nnz == 0
    # ... also with boundaries that hold no facet, and after the boundaries are removed again
    e = np.zeros(0, dtype=np.int64)
    pb.set_traction_boundaries([e, e], [1.0, 2.0], beta=10.0, beta_backflow=[0.3, 0.3])
    F, J = pb.assemble(xv, un, un2=un2)
    assert np.array_equal(F, Fr) and (J != Jr).nnz == 0
    assert TN.element_tensors.__module__ == "oracle.np_twin_nd"


@pytest.mark.parametrize("d", [2, 3])
def test_the_two_nitsche_terms_form_a_symmetric_block(d):
    """- int (2 mu eps(u) n) . v_T - int (2 mu eps(v) n) . u_T + penalty is symmetric in (u, v): the difference of the Jacobians
    with and without the tangential terms (no Dirichlet data, outlet stress term excluded by using inlet facets only)."""
    pb, (inl, out, _), xv, un, un2 = _problem(d, SCHEMES[0])
    pb.clear_bcs()
    sets = [np.concatenate([inl, out])]
    J0 = pb.assemble(xv, un)[1]
    pb.set_traction_boundaries(sets, [0.7], beta=30.0, tangential=[1])
    J1 = pb.assemble(xv, un)[1]
    D = (J1 - J0).toarray()
    assert np.abs(D).max() > 0 and np.abs(D - D.T).max() <= 1e-13 * np.abs(D).max()
    assert not D[pb.nu:].any() and not D[:, pb.nu:].any()   # A00 only


def _flow_rate(mesh, L, dp=8.0, mu=1.0, rho=0.01):
    d = mesh.x.shape[1]
    nv = mesh.num_vertices
    marker = U.mark_ends(mesh, corner=False)
    inl, out, _ = U.sets_of(marker)
    # backward Euler with a very large step: three steps reach the steady state
    prm = TN.Params(1e6, rho, mu, (0.0, 0.0, 0.0), theta=1.0, ds_terms=False)
    pb = TT.Problem(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, prm)
    pb.set_traction_boundaries([inl, out], [dp, 0.0], beta=100.0, tangential=[1, 0], beta_backflow=[0.0, 0.2])
    wn = U.wall_nodes(mesh, marker)
    pb.add_bc_u(wn, np.zeros((len(wn), d)))
    x, un = np.zeros((d + 1) * nv), np.zeros((nv, d))
    for _ in range(3):
        x, _ = pb.newton(x, un)
        un = x[: d * nv].reshape(-1, d).copy()
    q_out, q_in = pb.flux(x, out), -pb.flux(x, inl)
    assert abs(q_out - q_in) <= 1e-10 * q_out
    return q_out


def test_pressure_driven_channel_tends_to_the_plane_poiseuille_flow_rate():
    """Channel of height H = 1, length L = 0.25, Stokes regime (rho = 0.01, mu = 1), walls no-slip, inlet value dP with the
    tangential terms, outlet value 0 (R = 0) without, one cell along the flow (the flow is x-invariant): the flow rate tends to
    dP H^3 / (12 mu L) under refinement across the channel, second order."""
    L, dp = 0.25, 8.0
    exact = dp / (12.0 * L)
    errs = [abs(_flow_rate(U.channel(1, ny, L), L, dp) - exact) / exact for ny in (4, 8, 16)]
    # measured: 0.0625, 0.015625, 0.00390625
    assert errs[0] > errs[1] > errs[2] and errs[2] <= 1.5 * 0.00390625, errs


def test_pressure_driven_duct_tends_to_the_square_duct_flow_rate():
    """The same in the square duct a = 1 on Kuhn tetrahedra: Q tends to 0.0351443 a^4 dP / (mu L)."""
    L, dp = 0.25, 8.0
    exact = SQUARE_DUCT * dp / L
    errs = [abs(_flow_rate(U.duct(1, n, L), L, dp) - exact) / exact for n in (2, 4, 8)]
    # measured: 0.5554, 0.1803, 0.04898
    assert errs[0] > errs[1] > errs[2] and errs[2] <= 1.5 * 0.04898, errs
