"""NumPy twin of the pressure convection-diffusion (PCD) Schur approximation of pc_type 2 (include/cfdh.h: cfdh_set_schur_pcd) and of
Eisenstat-Walker forcing (cfdh_set_ksp_forcing), independent of the product: exact element and facet integrals, direct solves.

  M_d = diag of the consistent P1 mass;  K = rho N(w) - rho R_in(w) + c_t M;  A_p = P1 Laplacian, Dirichlet rows on the outlet
  vertices and the pressure-Dirichlet ones;  z_p = mu t + A_p^-1 (K t) with t = M_d^-1 r_p (s = K t and y zero on A_p's Dirichlet
  rows), z_p = r_p on the pressure-Dirichlet rows.
"""
from __future__ import annotations

from math import factorial

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def geometry(x, cells):
    """Barycentric gradients g [nc, d+1, d] and volumes [nc] of P1 simplices."""
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    d = x.shape[1]
    P = x[cells]                                    # [nc, d+1, d]
    J = np.transpose(P[:, 1:, :] - P[:, :1, :], (0, 2, 1))   # columns = edges
    det = np.linalg.det(J)
    Jinv = np.linalg.inv(J)                          # rows = grad lambda_1..d
    g = np.concatenate([-Jinv.sum(axis=1, keepdims=True), Jinv], axis=1)
    return g, np.abs(det) / factorial(d)


def _mass_local(vol, d):
    n1 = d + 1
    return vol[:, None, None] * (1.0 + np.eye(n1))[None] / ((d + 1) * (d + 2))


def _scatter(cells, loc, n, ncol=None):
    n1 = cells.shape[1]
    rows = np.repeat(cells, n1, axis=1).ravel()
    cols = np.tile(cells, (1, n1)).ravel()
    return sp.coo_matrix((loc.ravel(), (rows, cols)), shape=(n, ncol or n)).tocsr()


def mass_diag(x, cells):
    g, vol = geometry(x, cells)
    d = np.asarray(x).shape[1]
    md = np.zeros(len(x))
    np.add.at(md, np.asarray(cells).ravel(), np.repeat(vol * 2.0 / ((d + 1) * (d + 2)), d + 1))
    return md


def mass(x, cells):
    g, vol = geometry(x, cells)
    return _scatter(np.asarray(cells), _mass_local(vol, np.asarray(x).shape[1]), len(x))


def laplacian(x, cells):
    g, vol = geometry(x, cells)
    return _scatter(np.asarray(cells), vol[:, None, None] * np.einsum("cai,cbi->cab", g, g), len(x))


def convection(x, cells, w):
    """N_ij = int phi_i (w . grad phi_j) with w P1 (nodal values [nv, d])."""
    g, vol = geometry(x, cells)
    d = np.asarray(x).shape[1]
    cells = np.asarray(cells)
    W = np.einsum("eab,ebi->eai", _mass_local(vol, d), np.asarray(w)[cells])   # int phi_a w
    return _scatter(cells, np.einsum("eai,ebi->eab", W, g), len(x))


def _facet_monomial(k, alpha):
    """int_F prod lambda^alpha / |F| on a k-simplex."""
    return factorial(k) * np.prod([factorial(a) for a in alpha]) / factorial(k + sum(alpha))


def facet_matrix(x, cells, facet_cells, facet_local, w, facets):
    """B_ij = int (w . n) phi_i phi_j ds over the given exterior facets (outward n), exact for P1 w."""
    x = np.asarray(x, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    d = x.shape[1]
    n = len(x)
    g, vol = geometry(x, cells)
    rows, cols, vals = [], [], []
    for k in np.asarray(facets, dtype=np.int64):
        e, f = int(facet_cells[k]), int(facet_local[k])
        nF = -d * vol[e] * g[e, f]                  # n |F|
        fv = [cells[e, m] for m in range(d + 1) if m != f]
        s = [np.dot(np.asarray(w)[v], nF) for v in fv]
        for ia, a in enumerate(fv):
            for ib, b in enumerate(fv):
                acc = 0.0
                for ic in range(d):
                    alpha = [0] * d
                    alpha[ia] += 1
                    alpha[ib] += 1
                    alpha[ic] += 1
                    acc += s[ic] * _facet_monomial(d - 1, [q for q in alpha if q])
                rows.append(a); cols.append(b); vals.append(acc)
    return sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()


def marked_facets(facet_marker, marker):
    return np.flatnonzero(np.asarray(facet_marker) == marker)


def facet_vertex_set(cells, facet_cells, facet_local, facets):
    cells = np.asarray(cells)
    out = set()
    for k in facets:
        e, f = int(facet_cells[k]), int(facet_local[k])
        out.update(int(cells[e, m]) for m in range(cells.shape[1]) if m != f)
    return np.array(sorted(out), dtype=np.int64)


def pcd_operator(x, cells, facet_cells, facet_local, facet_marker, inlet, w, rho, ct):
    """K = rho N(w) - rho R_in(w) + ct M (scipy CSR, nv x nv)."""
    N = convection(x, cells, w)
    R = facet_matrix(x, cells, facet_cells, facet_local, w, marked_facets(facet_marker, inlet))
    return (rho * N - rho * R + ct * mass(x, cells)).tocsr()


def time_coefficient(rho, dt, theta, a0, time_term):
    return rho * a0 / (theta * dt) if time_term else 0.0


def pcd_action(r_p, K, md, L, dir_rows, pdir_rows, mu):
    """Exact PCD action: z = mu t + y, t = r / m_d, s = K t (0 on dir_rows), L_II y_I = s_I, y = 0 on dir_rows; z = r on pdir_rows."""
    n = len(r_p)
    t = r_p / md
    s = K @ t
    isdir = np.zeros(n, dtype=bool)
    isdir[np.asarray(dir_rows, dtype=np.int64)] = True
    I = np.flatnonzero(~isdir)
    y = np.zeros(n)
    if len(I):
        y[I] = spla.spsolve(L[I][:, I].tocsc(), s[I])
    z = mu * t + y
    z[np.asarray(pdir_rows, dtype=np.int64)] = r_p[np.asarray(pdir_rows, dtype=np.int64)]
    return z


def ew_tolerances(fnorms, rtol_0=0.3, rtol_max=0.9, gamma=1.0, alpha=(1.0 + 5.0 ** 0.5) / 2.0, threshold=0.1):
    """Eisenstat-Walker version 2 (PETSc's SNESKSPEW default) for the residual norms |F_0|, |F_1|, ... of one Newton solve."""
    out = []
    for k, fn in enumerate(fnorms):
        if k == 0:
            rt = rtol_0
        else:
            rt = gamma * (fn / fnorms[k - 1]) ** alpha
            stol = gamma * out[-1] ** alpha
            if stol > threshold:
                rt = max(rt, stol)
            rt = min(rt, rtol_max)
        out.append(rt)
    return np.array(out)
