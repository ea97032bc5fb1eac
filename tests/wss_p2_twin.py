"""NumPy twin of the wall shear stress on the P2/P1 context (cfdh_wall_shear_stress on a context of cfdh_create_ipcs) that does
NOT use the device's closed form: per exterior facet the P2 velocity gradient is evaluated at the points of the degree-3 facet
rule of oracle/np_twin_nd.py and (1/|f|) sum_q w_q lambda_v Tt(x_q) is deposited at the facet's vertices, with
T = -mu (grad u + grad u^T) n and Tt = T - (T.n) n.  The integrand is quadratic, so the rule is exact."""
import numpy as np

from ipcs_twin import p2_tabulate
from oracle import np_twin_nd as TN


def edge_rule():
    """The edge rule of np_twin_nd.facet_rule(2), or 3-point Gauss should that table ever hold fewer than two points."""
    pts, w = TN.facet_rule(2)
    if len(pts) >= 2:
        return np.asarray(pts, dtype=float), np.asarray(w, dtype=float)
    g, gw = np.polynomial.legendre.leggauss(3)
    s = 0.5 * (g + 1.0)
    return np.stack([1.0 - s, s], axis=1), 0.5 * gw


def wall_shear_stress(x, cells, nvert, facet_cells, facet_local, u, mu):
    """x [nn, d] and cells [nc, 6 | 10]: the P2 node mesh (vertices first); u [nn, d]; returns the field on the vertices [nvert, d]."""
    x, u = np.asarray(x, dtype=float), np.asarray(u, dtype=float)
    d = x.shape[1]
    nv = d + 1
    pts, wq = edge_rule() if d == 2 else (np.asarray(TN.facet_rule(3)[0]), np.asarray(TN.facet_rule(3)[1]))
    out = np.zeros((nvert, d))
    for e, fl in zip(np.asarray(facet_cells), np.asarray(facet_local)):
        cv = np.asarray(cells[e])
        X = x[cv[:nv]]
        Ji = np.linalg.inv((X[1:] - X[0]).T)            # rows: grad lambda_1 .. lambda_d
        gl = np.vstack([-Ji.sum(axis=0), Ji])           # [d + 1, d]
        n = -gl[fl] / np.linalg.norm(gl[fl])
        fv = [a for a in range(nv) if a != fl]          # the facet's vertices in increasing local index
        for pq, w in zip(pts, wq):
            lam = np.zeros(nv)
            lam[fv] = pq
            _, dl = p2_tabulate(lam[None, :], d)
            gphi = dl[0] @ gl                            # [nloc, d]: d_i phi_a
            G = gphi.T @ u[cv]                           # G[i, j] = d_i u_j
            T = -mu * (G + G.T) @ n
            Tt = T - (T @ n) * n
            for a in fv:
                out[cv[a]] += w * lam[a] * Tt
    return out
