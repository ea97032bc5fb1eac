"""NumPy twin of what the Cahouet-Chabard preconditioner takes from the ELEMENT of a generic context (csrc/cfdh_gen.hip, csrc/cfdh_gen3.hip,
scatter_stiffness_mass in csrc/cfdh_mesh_host.hpp)  --  TEST INFRASTRUCTURE, independent of the product:

    K_ab = int grad phi_a . grad phi_b        the pressure Laplacian on the node graph
    M_l  = diag(M) |Omega| / sum diag(M)      HRZ lumping of the consistent mass M (the row sums vanish at the vertices of a P2 simplex)

for P2 triangles (6 nodes), Q1 parallelograms, P2 tetrahedra (10 nodes) and Q1 parallelepipeds; P1 simplices are included so that the
same statements can be compared with the closed-form P1 twin (part_pc_twin.py).

Everything by over-integrated quadrature on affine cells, with rules built here: collapsed Gauss-Jacobi rules with 6 points per
direction on simplices (exact to degree 11; the integrands have degree 2 and 4), 4 Gauss points per direction on Q1 cells (exact to
degree 7; the integrands have degree 2 per direction).  The inverse of the cell's Jacobian (by cofactors), the physical gradients and the
sums over the points are carried in numpy.longdouble and rounded to fp64 once, so the twin's own rounding stays below that of a
fp64 evaluation wherever longdouble is wider than fp64.

Local node order (the library's): simplex vertices first, then the edge nodes, P2 node NV + q on the edge TRI_EDGES[q] / TET_EDGES[q];
Q1 node a at the reference corner (a & 1, a >> 1 & 1, a >> 2 & 1).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
from scipy.special import roots_jacobi, roots_legendre

import amg_twin as T

LD = np.longdouble
TRI_EDGES = [(1, 2), (0, 2), (0, 1)]
TET_EDGES = [(2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1)]
# kind -> (dimension, nodes per cell, vertices per cell)
KINDS = {"P1tri": (2, 3, 3), "P2tri": (2, 6, 3), "Q1quad": (2, 4, 4), "P1tet": (3, 4, 4), "P2tet": (3, 10, 4), "Q1hex": (3, 8, 8)}


def kind_of(dim, nloc):
    for k, (d, nl, _) in KINDS.items():
        if (d, nl) == (dim, nloc):
            return k
    raise KeyError((dim, nloc))


def _unit(n, alpha):
    """n points on [0, 1] for the weight (1 - t)^alpha."""
    t, w = roots_jacobi(n, float(alpha), 0.0) if alpha else roots_legendre(n)
    return 0.5 * (t + 1.0), w / 2.0 ** (alpha + 1)


def cell_rule(kind):
    """Reference points [nq, d] and weights (longdouble, normalised to the reference measure exactly)."""
    d = KINDS[kind][0]
    if kind.endswith(("tri", "tet")):
        per = [_unit(6, d - 1 - k) for k in range(d)]      # x = u, y = v (1 - u), z = w (1 - u) (1 - v)
        G = np.meshgrid(*[p[0] for p in per], indexing="ij")
        W = np.meshgrid(*[p[1] for p in per], indexing="ij")
        u = [g.ravel().astype(LD) for g in G]
        pts = [u[0], u[1] * (1 - u[0])] + ([u[2] * (1 - u[0]) * (1 - u[1])] if d == 3 else [])
        meas = LD(1) / (2 if d == 2 else 6)
    else:
        t, w = _unit(4, 0)
        G = np.meshgrid(*([t] * d), indexing="ij")
        W = np.meshgrid(*([w] * d), indexing="ij")
        pts = [g.ravel().astype(LD) for g in G]
        meas = LD(1)
    wq = np.prod(np.stack([g.ravel().astype(LD) for g in W], axis=1), axis=1)
    return np.stack(pts, axis=1), wq * (meas / wq.sum())


def tabulate(kind, pts):
    """phi [nq, nloc] and the reference gradients [nq, nloc, d] at the reference points."""
    pts = np.asarray(pts, dtype=LD)
    n = len(pts)
    d, nl, nvert = KINDS[kind]
    phi, g = np.zeros((n, nl), dtype=LD), np.zeros((n, nl, d), dtype=LD)
    if kind.startswith("Q1"):
        phi[:], g[:] = 1, 1
        for a in range(nl):
            for k in range(d):
                bit = (a >> k) & 1
                lk = pts[:, k] if bit else 1 - pts[:, k]
                phi[:, a] *= lk
                for m in range(d):
                    g[:, a, m] *= (1 if bit else -1) if m == k else lk
        return phi, g
    lam = np.concatenate([(1 - pts.sum(axis=1))[:, None], pts], axis=1)          # barycentric coordinates
    dl = np.concatenate([-np.ones((1, d)), np.eye(d)], axis=0).astype(LD)
    if kind.startswith("P1"):
        phi[:] = lam
        g[:] = dl[None]
        return phi, g
    for i in range(nvert):
        phi[:, i] = lam[:, i] * (2 * lam[:, i] - 1)
        g[:, i] = (4 * lam[:, i] - 1)[:, None] * dl[i]
    for q, (i, j) in enumerate(TRI_EDGES if d == 2 else TET_EDGES):
        phi[:, nvert + q] = 4 * lam[:, i] * lam[:, j]
        g[:, nvert + q] = 4 * (lam[:, i, None] * dl[j] + lam[:, j, None] * dl[i])
    return phi, g


def geometry(kind, x, cells):
    """Jinv [nc, d, d] (longdouble, by cofactors) with grad phi = sum_k dphi_ref_k Jinv[k, :], and |det J|; Q1 cells must be affine."""
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    d = KINDS[kind][0]
    assert x.shape[1] == d and cells.shape[1] == KINDS[kind][1]
    P = x[cells].astype(LD)
    ax = [1 << k for k in range(d)] if kind.startswith("Q1") else [k + 1 for k in range(d)]
    J = np.stack([P[:, a] - P[:, 0] for a in ax], axis=2)        # J[:, i, k] = d x_i / d xi_k
    if kind.startswith("Q1"):
        for a in range(1 << d):
            ex = P[:, 0] + sum(((a >> k) & 1) * (P[:, 1 << k] - P[:, 0]) for k in range(d))
            assert np.abs(P[:, a] - ex).max() <= 1e-10 * np.abs(P).max(), "Q1 cells must be affine"
    C = np.empty_like(J)                                          # cofactors: inv(J) = C^T / det
    if d == 2:
        C[:, 0, 0], C[:, 0, 1], C[:, 1, 0], C[:, 1, 1] = J[:, 1, 1], -J[:, 1, 0], -J[:, 0, 1], J[:, 0, 0]
    else:
        for i in range(3):
            for k in range(3):
                i1, i2, k1, k2 = (i + 1) % 3, (i + 2) % 3, (k + 1) % 3, (k + 2) % 3
                C[:, i, k] = J[:, i1, k1] * J[:, i2, k2] - J[:, i1, k2] * J[:, i2, k1]
    det = (J[:, 0, :] * C[:, 0, :]).sum(axis=1)
    assert (np.abs(det) > 0).all(), "degenerate cell"
    return np.swapaxes(C, 1, 2) / det[:, None, None], np.abs(det)


def _tables(kind, x, cells):
    pts, wq = cell_rule(kind)
    phi, dref = tabulate(kind, pts)
    Jinv, adet = geometry(kind, x, cells)
    return phi, np.einsum("qak,cki->cqai", dref, Jinv), adet[:, None] * wq[None, :]


def element_stiffness(kind, x, cells):
    """(K [nc, nloc, nloc], B [nc, nloc, nloc]) in fp64: K_ab = sum_q |det| w_q grad phi_a . grad phi_b and the bound of its terms
    B_ab = sum_q |det| w_q |grad phi_a| |grad phi_b| with Euclidean norms -- every gradient component carries an absolute error of a few
    eps |grad phi| from the inversion of the cell's Jacobian, so componentwise products would be too small where they cancel."""
    _, grad, dv = _tables(kind, x, cells)
    gn = np.sqrt((grad * grad).sum(axis=3))
    K = np.einsum("cq,cqai,cqbi->cab", dv, grad, grad)
    B = np.einsum("cq,cqa,cqb->cab", dv, gn, gn)
    return K.astype(np.float64), B.astype(np.float64)


def element_mass_diag(kind, x, cells):
    """(diag of the consistent element mass [nc, nloc], cell measures [nc]) in fp64."""
    phi, _, dv = _tables(kind, x, cells)
    return np.einsum("cq,qa->ca", dv, phi * phi).astype(np.float64), dv.sum(axis=1).astype(np.float64)


def _scatter(cells, loc, n):
    cells = np.asarray(cells, dtype=np.int64)
    nl = cells.shape[1]
    return sp.coo_matrix((loc.ravel(), (np.repeat(cells, nl, axis=1).ravel(), np.tile(cells, (1, nl)).ravel())), shape=(n, n)).tocsr()


def stiffness(kind, x, cells, nq=1):
    """(L, bound, terms) on the full node graph.  terms: the number of products the longest sum of an entry has when every cell is
    integrated with `nq` points -- (cells sharing the entry) x nq x dimension; the caller names the point count of whoever evaluated
    the sum under test (1 for a closed form)."""
    K, B = element_stiffness(kind, x, cells)
    n, d = len(x), KINDS[kind][0]
    cnt = int(_scatter(cells, np.ones_like(K), n).data.max())
    return T.canonical(_scatter(cells, K, n)), T.canonical(_scatter(cells, B, n)), cnt * int(nq) * d


def lumped_mass(kind, x, cells):
    """HRZ lumping: the diagonal of the consistent mass scaled so that it sums to the measure of the mesh."""
    md, meas = element_mass_diag(kind, x, cells)
    ml = np.zeros(len(x))
    np.add.at(ml, np.asarray(cells, dtype=np.int64), md)
    return ml * (float(meas.astype(LD).sum()) / float(md.astype(LD).sum()))


def lumped_mass_tolerance(kind, cells):
    """Tolerance of the library's M_l against `lumped_mass`, as a multiple of max M_l: the factor msum / dsum is the quotient of two
    serial fp64 sums of nc and nc * nloc positive terms, so its relative error is bounded by about (nc * nloc) eps (the longer sum;
    positive terms: no cancellation); the node's own sum over a few cells and its quadrature are what the 16 eps of the P1 test allow."""
    nc, nl = np.asarray(cells).shape
    return (nc * nl + 16) * T.EPS


def dirichlet_laplacian(kind, x, cells, pbc, nq=1):
    """The element's stiffness with identity rows and dropped columns on the flagged nodes (the level-0 operator of the pressure
    hierarchies); (values, bound, terms) as part_pc_twin.dirichlet_laplacian returns them."""
    Lp, Lb, terms = stiffness(kind, x, cells, nq)
    n = len(x)
    on = np.asarray(pbc) == 0
    off = np.nonzero(~on)[0]
    eye = sp.csr_matrix((np.ones(len(off)), (off, off)), shape=(n, n))
    return T.add_keep(T._filter(Lp, on, on), eye), T.add_keep(T._filter(Lb, on, on), eye), terms
