"""NumPy twin of the PCD operator (pc_type 2, include/cfdh.h: cfdh_set_schur_pcd) on the degree-1 generic elements: P1 triangles,
Q1 parallelograms, Q1 parallelepipeds  --  TEST INFRASTRUCTURE, independent of the product.

  K = rho N(w) - rho R_in(w) + c_t M,  N_ij = int phi_i (w . grad phi_j),  R_in,ij = int_{inlet} (w . n) phi_i phi_j ds,  M the consistent
  mass, M_d its diagonal, and the element's Laplacian, with w in the element space (nodal values).

Everything by over-integrated quadrature on affine cells: the 49-point collapsed rule on triangles and 3-point Gauss per direction
on Q1 cells and on every facet (the integrands have degree <= 3 per direction).  The facet integrals use the facet's own geometry
and its own nodal basis (linear on an edge, bilinear on a parallelogram face), not the cell's reference map.

Local node order: triangle vertices 0, 1, 2 (facet f opposite vertex f); Q1 nodes at the reference corners (a & 1, a >> 1 & 1,
a >> 2 & 1), quadrilateral facets (0,1) (0,2) (1,3) (2,3), hexahedron facets (0,1,2,3) (0,1,4,5) (0,2,4,6) (1,3,5,7) (2,3,6,7)
(4,5,6,7).  The action z_p = mu t + A_p^-1 K t and the Eisenstat-Walker sequence are those of tests/pcd_twin.py.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
from scipy.special import roots_jacobi, roots_legendre

FACETS = {
    "tri": [(1, 2), (0, 2), (0, 1)],
    "quad": [(0, 1), (0, 2), (1, 3), (2, 3)],
    "hex": [(0, 1, 2, 3), (0, 1, 4, 5), (0, 2, 4, 6), (1, 3, 5, 7), (2, 3, 6, 7), (4, 5, 6, 7)],
}
NLOC = {"tri": 3, "quad": 4, "hex": 8}


def _gauss01(n):
    t, w = roots_legendre(n)
    return 0.5 * (t + 1.0), 0.5 * w


def _cell_rule(kind):
    """Reference points [nq, d] and weights (summing to the reference measure)."""
    if kind == "tri":
        tj, wj = roots_jacobi(7, 1.0, 0.0)
        tl, wl = roots_legendre(7)
        u, v = 0.5 * (tj + 1.0), 0.5 * (tl + 1.0)
        U, V = np.meshgrid(u, v, indexing="ij")
        W = np.outer(0.25 * wj, 0.5 * wl)
        return np.stack([U.ravel(), (V * (1.0 - U)).ravel()], axis=1), W.ravel()
    t, w = _gauss01(3)
    d = 2 if kind == "quad" else 3
    G = np.meshgrid(*([t] * d), indexing="ij")
    Wg = np.meshgrid(*([w] * d), indexing="ij")
    return np.stack([g.ravel() for g in G], axis=1), np.prod(np.stack([g.ravel() for g in Wg], axis=1), axis=1)


def tabulate(kind, pts):
    """phi [nq, nloc], reference gradients [nq, nloc, d]."""
    pts = np.asarray(pts, dtype=np.float64)
    n, d = pts.shape
    if kind == "tri":
        phi = np.stack([1.0 - pts[:, 0] - pts[:, 1], pts[:, 0], pts[:, 1]], axis=1)
        g = np.zeros((n, 3, 2))
        g[:, 0] = (-1.0, -1.0); g[:, 1] = (1.0, 0.0); g[:, 2] = (0.0, 1.0)
        return phi, g
    nl = 1 << d
    phi = np.ones((n, nl))
    g = np.ones((n, nl, d))
    for a in range(nl):
        for k in range(d):
            bit = (a >> k) & 1
            lk = pts[:, k] if bit else 1.0 - pts[:, k]
            phi[:, a] *= lk
            for m in range(d):
                g[:, a, m] *= (1.0 if bit else -1.0) if m == k else lk
    return phi, g


def geometry(kind, x, cells):
    """Jinv [nc, d, d] with grad phi_i = sum_k dphi_ref_k Jinv[k, i], and |det J|; Q1 cells must be affine."""
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    d = x.shape[1]
    P = x[cells]
    ax = [k + 1 for k in range(d)] if kind == "tri" else [1 << k for k in range(d)]
    J = np.stack([P[:, a] - P[:, 0] for a in ax], axis=2)     # J[:, i, k] = d x_i / d xi_k
    if kind != "tri":
        for a in range(1 << d):
            ex = P[:, 0] + sum(((a >> k) & 1) * (P[:, 1 << k] - P[:, 0]) for k in range(d))
            assert np.abs(P[:, a] - ex).max() <= 1e-10 * np.abs(P).max(), "Q1 cells must be affine"
    return np.linalg.inv(J), np.abs(np.linalg.det(J))


def _scatter(cells, loc, n):
    nl = cells.shape[1]
    rows = np.repeat(cells, nl, axis=1).ravel()
    cols = np.tile(cells, (1, nl)).ravel()
    return sp.coo_matrix((loc.ravel(), (rows, cols)), shape=(n, n)).tocsr()


def _tables(kind, x, cells):
    pts, wq = _cell_rule(kind)
    phi, dref = tabulate(kind, pts)
    Jinv, adet = geometry(kind, x, cells)
    grad = np.einsum("qak,cki->cqai", dref, Jinv)
    return phi, grad, adet[:, None] * wq[None, :]


def mass(kind, x, cells):
    phi, _, dv = _tables(kind, x, cells)
    return _scatter(np.asarray(cells, dtype=np.int64), np.einsum("cq,qa,qb->cab", dv, phi, phi), len(x))


def mass_diag(kind, x, cells):
    phi, _, dv = _tables(kind, x, cells)
    md = np.zeros(len(x))
    np.add.at(md, np.asarray(cells, dtype=np.int64), np.einsum("cq,qa->ca", dv, phi * phi))
    return md


def laplacian(kind, x, cells):
    _, grad, dv = _tables(kind, x, cells)
    return _scatter(np.asarray(cells, dtype=np.int64), np.einsum("cq,cqai,cqbi->cab", dv, grad, grad), len(x))


def convection(kind, x, cells, w):
    """N_ij = int phi_i (w . grad phi_j), w in the element space (nodal values [nv, d])."""
    cells = np.asarray(cells, dtype=np.int64)
    phi, grad, dv = _tables(kind, x, cells)
    wq = np.einsum("qa,cai->cqi", phi, np.asarray(w, dtype=np.float64)[cells])
    return _scatter(cells, np.einsum("cq,qa,cqi,cqbi->cab", dv, phi, wq, grad), len(x))


def facet_matrix(kind, x, cells, facet_cells, facet_local, w, facets):
    """B_ij = int (w . n) phi_i phi_j ds over the given exterior facets, outward n."""
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64)
    n, d = x.shape
    t, wt = _gauss01(3)
    rows, cols, vals = [], [], []
    for k in np.asarray(facets, dtype=np.int64):
        e, f = int(facet_cells[k]), int(facet_local[k])
        nodes = cells[e, list(FACETS[kind][f])]
        X = x[nodes]
        cen = x[cells[e]].mean(axis=0)
        if d == 2:
            tv = X[1] - X[0]
            nF = np.array([tv[1], -tv[0]])                     # n |F|
            psi = np.stack([1.0 - t, t], axis=1)               # [q, node]
            wq = wt
        elif kind == "hex":
            nF = np.cross(X[1] - X[0], X[2] - X[0])            # parallelogram face: nodes 0, 1, 2 span it, node 3 = 1 + 2 - 0
            S, T = np.meshgrid(t, t, indexing="ij")
            s, r = S.ravel(), T.ravel()
            psi = np.stack([(1 - s) * (1 - r), s * (1 - r), (1 - s) * r, s * r], axis=1)
            wq = np.outer(wt, wt).ravel()
        else:
            raise ValueError(kind)
        if np.dot(nF, X.mean(axis=0) - cen) < 0:
            nF = -nF
        sig = psi @ (w[nodes] @ nF)                            # (w . n) |F| at the points
        loc = np.einsum("q,q,qa,qb->ab", wq, sig, psi, psi)
        for ia, a in enumerate(nodes):
            for ib, b in enumerate(nodes):
                rows.append(a); cols.append(b); vals.append(loc[ia, ib])
    return sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()


def marked_facets(facet_marker, marker):
    return np.flatnonzero(np.asarray(facet_marker) == marker)


def facet_node_set(kind, cells, facet_cells, facet_local, facets):
    cells = np.asarray(cells)
    out = set()
    for k in facets:
        out.update(int(v) for v in cells[int(facet_cells[k]), list(FACETS[kind][int(facet_local[k])])])
    return np.array(sorted(out), dtype=np.int64)


def pcd_operator(kind, x, cells, facet_cells, facet_local, facet_marker, inlet, w, rho, ct):
    """K = rho N(w) - rho R_in(w) + ct M (scipy CSR, nv x nv)."""
    N = convection(kind, x, cells, w)
    R = facet_matrix(kind, x, cells, facet_cells, facet_local, w, marked_facets(facet_marker, inlet))
    return (rho * N - rho * R + ct * mass(kind, x, cells)).tocsr()
