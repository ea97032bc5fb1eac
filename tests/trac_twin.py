"""NumPy twin of the traction boundaries of the convective form  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Restates the boundary terms of the reference's src/solvers/stabilized_schur_pressure_backflow.py:191-217 on top of the P1 simplex
twin oracle/np_twin_nd.py, whose volume form, assembly, Dirichlet logic and Newton are reused by import.  Traction boundary k
(value P_k, outward normal n, w_T = w - (w . n) n, ubar = theta u + (1 - theta) u_prev, h the owning cell's largest vertex distance):

  always                 + P_k int v . n                                                             (residual only, :193, :208)
  tangential[k] on       - int (2 mu eps(ubar) n) . v_T - int (2 mu eps(v) n) . ubar_T + (beta mu / h) int ubar_T . v_T   (:197-201)
  tangential[k] off      - int (2 mu eps(ubar) n) . v                                                             (:209)
  beta_backflow[k] > 0   - beta_backflow[k] rho int (u_prev . n)_- ubar . v,   (s)_- = (s - |s|) / 2                (:213-217)

The terms are written the way the UFL reads: every test function v = lambda_a e_i is a tensor entry, eps(v) is formed from its
gradient, and the facet integrals of the P1 polynomials are taken in closed form (oint l_a = |F| / d,
oint l_a l_b = |F| (1 + d_ab) / (d (d + 1))); the backflow term, whose coefficient is not polynomial, uses np_twin_nd.facet_rule.
All four terms are linear in ubar, so the Jacobian is theta times the same expression applied to the unit trial functions.
Without a boundary set the element tensors are the parent's, bit for bit (nothing is added).
"""
from __future__ import annotations

import numpy as np

from oracle import np_twin_nd as ND


def _facet_terms(d, g, vol, h, f, ub, une, prm, beta_nitsche, tangential, beta_bf):
    """Fu [c, d+1, d]: the terms linear in ubar on local facet f of the cells whose gradients / volumes / sizes are g, vol, h and
    whose nodal ubar and u_prev are ub, une [c, d+1, d]."""
    n1 = d + 1
    mu, rho = prm.mu, prm.rho
    gf = g[:, f]
    gl = np.linalg.norm(gf, axis=1)
    n = -gf / gl[:, None]
    fm = d * vol * gl                                            # |F|
    ev = [a for a in range(n1) if a != f]
    I = np.eye(d)
    P = I[None] - np.einsum("ci,cj->cij", n, n)                  # w_T = P w
    lam1 = np.zeros(n1)                                          # oint l_a / |F|
    lam1[ev] = 1.0 / d
    lam2 = np.zeros((n1, n1))                                    # oint l_a l_b / |F|
    for a in ev:
        for b in ev:
            lam2[a, b] = (2.0 if a == b else 1.0) / (d * (d + 1.0))
    # grad(v)[a, i, k, l] = d_k v_l for v = lambda_a e_i;  grad(ubar)[k, l] = d_k ubar_l
    gradv = np.einsum("cak,il->caikl", g, I)
    epsv = 0.5 * (gradv + np.swapaxes(gradv, 3, 4))
    gradu = np.einsum("cak,cal->ckl", g, ub)
    epsu = 0.5 * (gradu + np.swapaxes(gradu, 1, 2))
    sn_u = 2.0 * mu * np.einsum("ckl,cl->ck", epsu, n)           # 2 mu eps(ubar) n, a cell constant
    sn_v = 2.0 * mu * np.einsum("caikl,cl->caik", epsv, n)       # 2 mu eps(v) n
    Fu = np.zeros((len(vol), n1, d))
    if tangential:
        # int v_T = P e_i oint l_a;  int ubar_T = P sum_b ubar_b oint l_b
        Fu -= np.einsum("ck,cki,a,c->cai", sn_u, P, lam1, fm)
        uT = np.einsum("ckl,b,cbl,c->ck", P, lam1, ub, fm)
        Fu -= np.einsum("caik,ck->cai", sn_v, uT)
        Fu += np.einsum("c,ab,cil,cbl,c->cai", beta_nitsche * mu / h, lam2, P, ub, fm)
    else:
        Fu -= np.einsum("ci,a,c->cai", sn_u, lam1, fm)
    if beta_bf > 0.0:
        QF, WF = ND.facet_rule(d)
        sv = [np.einsum("ci,ci->c", une[:, a], n) for a in ev]
        for lam, wq in zip(QF, WF):
            sq = sum(l * s_ for l, s_ in zip(lam, sv))
            cq = beta_bf * rho * 0.5 * (sq - np.abs(sq)) * wq * fm
            uq = sum(l * ub[:, a] for l, a in zip(lam, ev))
            for la, a in zip(lam, ev):
                Fu[:, a, :] -= (cq * la)[:, None] * uq
    return Fu, n, fm, lam1


class Problem(ND.Problem):
    """np_twin_nd.Problem with traction boundaries."""

    def __init__(self, x, cells, facet_cells, facet_local, prm):
        super().__init__(x, cells, facet_cells, facet_local, prm)
        self.set_traction_boundaries([], [])

    def set_traction_boundaries(self, facet_sets, values, beta=0.0, tangential=None, beta_backflow=None):
        """facet_sets[k]: exterior facet ids (indices into facet_cells / facet_local) of boundary k with value values[k];
        tangential[k] (None: all on); beta_backflow[k] (None: all 0)."""
        nb = len(facet_sets)
        self.tb_sets = [np.asarray(s, dtype=np.int64) for s in facet_sets]
        self.tb_values = [float(v) for v in values]
        self.tb_beta = float(beta)
        self.tb_tangential = [True] * nb if tangential is None else [bool(t) for t in tangential]
        self.tb_backflow = [0.0] * nb if beta_backflow is None else [float(b) for b in beta_backflow]
        assert len(self.tb_values) == nb and len(self.tb_tangential) == nb and len(self.tb_backflow) == nb
        assert all(b >= 0.0 for b in self.tb_backflow)

    def _add_traction(self, Fe, Je, u, un):
        d, n1 = self.d, self.d + 1
        prm = self.prm
        th = prm.theta
        for k, fs in enumerate(self.tb_sets):
            for f in range(n1):
                sel = self.facet_cells[fs[self.facet_local[fs] == f]]
                if len(sel) == 0:
                    continue
                cells = self.cells[sel]
                g, vol, h = ND.geometry(self.x, cells)
                une = un[cells]
                ub = th * u[cells] + (1.0 - th) * une
                args = (d, g, vol, h, f)
                tail = (prm, self.tb_beta, self.tb_tangential[k], self.tb_backflow[k])
                Fu, n, fm, lam1 = _facet_terms(*args, ub, une, *tail)
                Fu += self.tb_values[k] * np.einsum("ci,a,c->cai", n, lam1, fm)
                Fe[sel, : d * n1] += Fu.reshape(len(sel), d * n1)
                if Je is not None:
                    for b in range(n1):
                        for j in range(d):
                            e = np.zeros_like(ub)
                            e[:, b, j] = 1.0
                            col = _facet_terms(*args, e, une, *tail)[0]
                            Je[sel, : d * n1, d * b + j] += th * col.reshape(len(sel), d * n1)

    def assemble(self, xvec, un, want_jac=True, apply_bc=True, un2=None):
        if not self.tb_sets:
            return super().assemble(xvec, un, want_jac=want_jac, apply_bc=apply_bc, un2=un2)
        parent = ND.element_tensors

        def tensors(x, cells, u, un_, p, prm, facet_flags=None, want_jac=True, un2=None):
            Fe, Je = parent(x, cells, u, un_, p, prm, facet_flags, want_jac=want_jac, un2=un2)
            self._add_traction(Fe, Je, u, un_)
            return Fe, Je

        # Problem.assemble looks element_tensors up in its module at call time: its assembly and Dirichlet logic run unchanged
        ND.element_tensors = tensors
        try:
            return super().assemble(xvec, un, want_jac=want_jac, apply_bc=apply_bc, un2=un2)
        finally:
            ND.element_tensors = parent

    def flux_prev(self, un, facets):
        """int u_prev . n ds over the given exterior facets."""
        un = np.asarray(un, dtype=np.float64).reshape(-1)
        return self.flux(np.concatenate([un, np.zeros(self.nv)]), facets)
