"""CPU tests of tests/cc_gen_twin.py: the element stiffness, the HRZ-lumped mass and the Dirichlet Laplacian of the generic elements, and
the P1 interpolation of P2 simplices, against exact statements and against the independent element tensors of oracle/."""
import itertools

import numpy as np
import pytest

import amg_twin as T
import cc_gen_twin as C
import part_pc_twin as PT
from gen3_util import node_mesh3
from gen_util import node_mesh
from oracle import np_twin_gen as G
from oracle import np_twin_gen3 as G3

from cfd_hemodynamic_amd.mesh import create_unit_square
from cfd_hemodynamic_amd.mesh3d import create_unit_cube

KINDS = ["P2tri", "Q1quad", "P2tet", "Q1hex"]
ORACLE = {"P2tri": (G, G.P2_TRI), "Q1quad": (G, G.Q1_QUAD), "P2tet": (G3, G3.P2_TET), "Q1hex": (G3, G3.Q1_HEX)}


def mesh_of(kind, distort=0.3):
    """A small sheared mesh of the element: a transposed or mis-indexed inverse Jacobian changes its matrices."""
    if kind in ("P2tri", "Q1quad"):
        return node_mesh(kind[:2], 3, distort)
    return node_mesh3(kind[:2], 2, distort)


def sheared_cell(kind, rng):
    """One cell under a random affine map with all off-diagonal entries of the Jacobian non-zero."""
    d, nl, nvert = C.KINDS[kind]
    pts = np.zeros((nl, d))
    if kind.startswith("Q1"):
        for a in range(nl):
            pts[a] = [(a >> k) & 1 for k in range(d)]
    else:
        pts[1:nvert] = np.eye(d)
        for q, (i, j) in enumerate(C.TRI_EDGES if d == 2 else C.TET_EDGES):
            pts[nvert + q] = 0.5 * (pts[i] + pts[j])
    J = np.eye(d) + 0.4 * rng.uniform(-1.0, 1.0, (d, d))
    return pts, pts @ J.T + rng.standard_normal(d), J


@pytest.mark.parametrize("kind", KINDS)
def test_rules_integrate_the_reference_measure_and_the_basis_is_nodal(kind):
    pts, w = C.cell_rule(kind)
    d, nl, _ = C.KINDS[kind]
    assert (w > 0).all() and abs(float(w.sum()) - {"tri": 0.5, "uad": 1.0, "tet": 1.0 / 6.0, "hex": 1.0}[kind[-3:]]) <= 1e-16
    ref, _, _ = sheared_cell(kind, np.random.default_rng(0))
    phi, g = C.tabulate(kind, ref)
    assert np.abs(phi.astype(np.float64) - np.eye(nl)).max() <= 1e-15                    # nodal basis in the library's node order
    phi, g = C.tabulate(kind, pts)
    assert np.abs(phi.sum(axis=1) - 1).max() <= 1e-15 and np.abs(g.sum(axis=1)).max() <= 1e-14     # partition of unity


@pytest.mark.parametrize("kind", KINDS)
def test_stiffness_rows_sum_to_zero(kind):
    m = mesh_of(kind)
    K, B = C.element_stiffness(kind, m.x, m.cells)
    assert np.abs(K.sum(axis=2)).max() <= 64 * T.EPS * B.sum(axis=2).max()
    assert np.abs(K - np.swapaxes(K, 1, 2)).max() == 0.0 or np.abs(K - np.swapaxes(K, 1, 2)).max() <= 4 * T.EPS * B.max()
    assert (np.abs(K) <= B * (1 + 1e-15)).all(), "the bound of the terms dominates the entry"
    L, Lb, terms = C.stiffness(kind, m.x, m.cells, nq=7)
    assert np.abs(L @ np.ones(len(m.x))).max() <= 64 * T.EPS * Lb.sum(axis=1).max() and terms % (7 * C.KINDS[kind][0]) == 0


def _poly_energy_q1(c, M, d):
    """int over the unit cube of grad f^T M grad f for f = sum_S c_S prod_{k in S} xi_k (S: subsets of the directions), by monomials."""
    subsets = [s for n in range(d + 1) for s in itertools.combinations(range(d), n)]
    total = 0.0
    for k in range(d):
        for l in range(d):
            for s, cs in zip(subsets, c):
                if k not in s:
                    continue
                for t, ct in zip(subsets, c):
                    if l not in t:
                        continue
                    e = np.zeros(d)
                    for i in s:
                        e[i] += i != k
                    for i in t:
                        e[i] += i != l
                    total += M[k, l] * cs * ct / np.prod(e + 1.0)
    return total, subsets


@pytest.mark.parametrize("kind", KINDS)
def test_energy_of_a_field_of_the_element_space_on_a_sheared_cell(kind):
    """x^T K x is the exact Dirichlet energy: of a quadratic on a P2 simplex (its gradient is linear: the edge-midpoint rule of the
    triangle and the 4-point rule of the tetrahedron are exact for |grad f|^2), of a multilinear field on a Q1 cell (by monomials)."""
    rng = np.random.default_rng(3)
    d, nl, nvert = C.KINDS[kind]
    for _ in range(3):
        ref, X, J = sheared_cell(kind, rng)
        K, _ = C.element_stiffness(kind, X, np.arange(nl)[None])
        adet = abs(np.linalg.det(J))
        if kind.startswith("P2"):
            A = rng.standard_normal((d, d))
            A, b = A + A.T, rng.standard_normal(d)
            f = np.einsum("ni,ij,nj->n", X, A, X) + X @ b + 0.7
            V = X[:nvert]
            if d == 2:
                qp, qw = 0.5 * (V[[1, 2, 0]] + V[[2, 0, 1]]), np.full(3, adet / 6.0)
            else:
                a_, b_ = (5.0 + 3.0 * np.sqrt(5.0)) / 20.0, (5.0 - np.sqrt(5.0)) / 20.0
                lam = np.full((4, 4), b_) + (a_ - b_) * np.eye(4)
                qp, qw = lam @ V, np.full(4, adet / 24.0)
            gq = 2.0 * qp @ A + b
            exact = (qw * (gq * gq).sum(axis=1)).sum()
        else:
            c = rng.standard_normal(nl)
            Ji = np.linalg.inv(J)
            e, subsets = _poly_energy_q1(c, Ji @ Ji.T, d)
            exact = adet * e
            f = np.array([sum(cs * np.prod(ref[a, list(s)]) for s, cs in zip(subsets, c)) for a in range(nl)])
        got = f @ K[0] @ f
        assert abs(got - exact) <= 1e-13 * abs(exact), (kind, got, exact)


@pytest.mark.parametrize("kind", KINDS)
def test_stiffness_agrees_with_the_element_tensors_of_the_oracle(kind):
    """At rest (u = u_n = 0, p = 0) the pressure-pressure block of the oracle's element Jacobian is tau / rho times the stiffness, with
    tau constant on the cell."""
    m = mesh_of(kind)
    mod, et = ORACLE[kind]
    d, nl, _ = C.KINDS[kind]
    prm = mod.Params(0.01, 1.3, 0.02, np.zeros(d))
    x, cells = np.asarray(m.x, dtype=np.float64)[:, :d], np.asarray(m.cells, dtype=np.int64)
    z = np.zeros((len(x), d))
    _, Je = mod.element_tensors(et, x, cells, z, z, np.zeros(len(x)), prm)
    h = mod.cell_geometry(mod.element(et), x, cells)[2]
    tau, _ = G.tau_pair(np.zeros(len(cells)), h, prm)
    K, B = C.element_stiffness(kind, x, cells)
    ref = Je[:, d * nl:, d * nl:] * (prm.rho / tau)[:, None, None]
    nq = len(mod.element(et).w)
    assert (np.abs(ref - K) <= T.gamma(4 * nq * d) * B).all(), np.abs((ref - K) / B).max()


@pytest.mark.parametrize("kind", KINDS)
def test_lumped_mass_sums_to_the_measure_and_is_positive(kind):
    m = mesh_of(kind)
    d, nl, nvert = C.KINDS[kind]
    ml = C.lumped_mass(kind, m.x[:, :d], m.cells)
    measure = {"P2tri": 1.0, "Q1quad": 0.8, "P2tet": 1.0, "Q1hex": 0.48}[kind]         # shearing keeps the measure
    assert abs(ml.sum() - measure) <= 1e-14 * measure
    assert (ml > 0).all()
    verts = np.unique(np.asarray(m.cells)[:, :nvert])
    assert ml[verts].min() > 1e-3 * ml.max()
    if kind.startswith("P2"):
        # ... where the row sums of the consistent mass vanish (triangle) or are negative (tetrahedron)
        pts, w = C.cell_rule(kind)
        phi, _ = C.tabulate(kind, pts)
        rows = np.einsum("q,qa->a", w, phi).astype(np.float64)
        assert (rows[:nvert] <= 1e-16).all() and (rows[nvert:] > 0).all()
    md, meas = C.element_mass_diag(kind, m.x[:, :d], m.cells)
    assert np.abs(md.sum(axis=1) / meas - (md.sum() / meas.sum())).max() <= 1e-14     # affine cells: one factor for the whole mesh


@pytest.mark.parametrize("dim", [2, 3])
def test_p1_interpolation_reproduces_linear_fields_at_edge_nodes(dim):
    m = node_mesh("P2", 3, 0.3) if dim == 2 else node_mesh3("P2", 2, 0.3)
    x = np.asarray(m.x)[:, :dim]
    P, verts = T.p1_interpolation(x, m.cells, dim + 1)
    assert P.shape == (len(x), len(verts)) and len(verts) < len(x)
    assert np.array_equal(verts, np.unique(np.asarray(m.cells)[:, : dim + 1]))
    f = x @ np.arange(1.0, dim + 1.0) + 0.25
    edge = np.setdiff1d(np.arange(len(x)), verts)
    assert np.abs(P @ f[verts] - f).max() <= 4 * T.EPS * np.abs(f).max()
    assert (np.diff(P.indptr)[edge] == 2).all() and (np.diff(P.indptr)[verts] == 1).all()
    # and not quadratic ones: the edge nodes carry values of their own
    q = (x * x).sum(axis=1)
    assert np.abs(P @ q[verts] - q)[edge].min() > 1e-4


@pytest.mark.parametrize("dim", [2, 3])
def test_generic_dirichlet_laplacian_on_a_p1_mesh_is_the_p1_one(dim):
    m = create_unit_square(5) if dim == 2 else create_unit_cube(3)
    x = np.asarray(m.x)[:, :dim].copy()
    x[:, 0] += 0.3 * x[:, dim - 1]
    pbc = (np.isclose(m.x[:, 0], 1.0)).astype(np.uint8)
    assert pbc.any() and not pbc.all()
    L, Lb, k = PT.dirichlet_laplacian(x, m.cells, pbc)
    kind = C.kind_of(dim, dim + 1)
    Lg, Lgb, kg = C.dirichlet_laplacian(kind, x, m.cells, pbc, nq=1)
    assert kg == k
    v = T.check_operator("generic against P1", T.raw_csr(Lg), (L, Lb, k))
    assert v.ratio <= 1.0, v.where
    assert np.abs(T.canonical(Lgb).data - T.canonical(Lb).data).max() <= 1e-14 * Lb.data.max()
    rows = np.nonzero(pbc)[0]
    assert (Lg[rows].toarray()[np.arange(len(rows)), rows] == 1.0).all() and Lg[rows].nnz == len(rows) and Lg[:, rows].nnz == len(rows)
    ml = C.lumped_mass(kind, x, m.cells)       # HRZ on P1 simplices is the row-sum lumping
    assert np.abs(ml - PT.lumped_mass(x, m.cells)).max() <= 16 * T.EPS * ml.max()
