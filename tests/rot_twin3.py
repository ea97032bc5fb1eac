"""NumPy twin of the rotational form of the pressure-driven solvers in 3-D  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The gdim-3 branch of the reference's src/solvers/stabilized_schur_pressurebc.py:111-121 (curl, cross(curl(w), w),
cross(curl(w), n)) with the volume form of :123-160 and the facets of :177-205, restated for the nodal 3-D elements of
oracle/np_twin_gen3.py (P1 / P2 tetrahedra, Q1 parallelepipeds), whose element tables, cell and facet geometry, facet rules,
tau pair, assembly with Dirichlet handling and direct-solve Newton are reused by import.  With ubar = theta u + (1 - theta) u_prev,
w_t = (a0 u + a1 u_prev + a2 u_prev2)/dt and omega = curl ubar:

  F =  rho w_t . v + mu curl ubar . curl v - p div v + rho (omega x ubar) . v - rho/2 |ubar|^2 div v - rho f . v
     + q div ubar + tau R_i ubar_k d_k v_i + (tau/rho) R . grad q + tau_L rho div ubar div v,
  R  = rho (w_t + omega x ubar) + grad p - rho f                 (no viscous part: no Hessians, :142-144)

and on the facets of pressure boundary k (value P_k, outward n, w_T = w - (w . n) n, h = largest vertex distance of the cell):

  + P_k v . n - mu (omega x n) . v_T - mu (curl v x n) . ubar_T + (beta mu / h) ubar_T . v_T.

(omega x n) and (curl v x n) are tangential, so the projections on v and ubar can be dropped in those two terms.  Jacobian: the
exact derivative (theta times the derivative in ubar plus the time term); P_k enters the residual only.
"""
from __future__ import annotations

import numpy as np

from oracle import np_twin_gen3 as G3

EPS = np.zeros((3, 3, 3))
EPS[0, 1, 2] = EPS[1, 2, 0] = EPS[2, 0, 1] = 1.0
EPS[0, 2, 1] = EPS[2, 1, 0] = EPS[1, 0, 2] = -1.0


def _curl_basis(grad):
    """curl(phi_a e_i) = grad phi_a x e_i: [..., a, i, m] from grad [..., a, j]."""
    return np.einsum("mji,...aj->...aim", EPS, grad)


def element_tensors_rot3(etype, x, cells, u, un, p, prm, pval=None, beta=0.0, want_jac=True, un2=None):
    """Fe [nc, 4 nloc], Je [nc, 4 nloc, 4 nloc] of the rotational form.  pval [nc, nfacets]: P_k of the pressure boundary holding
    local facet f of the cell, NaN elsewhere."""
    el = G3.element(etype)
    nl, nc = el.nloc, len(cells)
    rho, mu, dt, th, a0 = prm.rho, prm.mu, prm.dt, prm.theta, prm.a0
    Jinv, adet, h, _ = G3.cell_geometry(el, x, cells)
    ue, une, pe = u[cells], un[cells], p[cells]
    ubn = th * ue + (1.0 - th) * une
    wn = (a0 * ue + prm.a1 * une) / dt
    if prm.a2 != 0.0:
        wn = wn + prm.a2 * un2[cells] / dt
    phi = el.phi
    grad = np.einsum("qak,cki->cqai", el.dphi, Jinv)             # [c,q,a,i]
    cb = _curl_basis(grad)                                       # [c,q,a,i,m]: curl(phi_a e_i)
    ub = np.einsum("qa,cai->cqi", phi, ubn)
    w = np.einsum("qa,cai->cqi", phi, wn)
    unq = np.einsum("qa,cai->cqi", phi, une)
    Gd = np.einsum("cqai,caj->cqij", grad, ubn)                  # d_i ubar_j
    divu = np.einsum("cqii->cq", Gd)
    om = np.einsum("ijk,cqjk->cqi", EPS, Gd)                     # curl ubar
    Cr = np.cross(om, ub)
    ke = 0.5 * rho * np.einsum("cqi,cqi->cq", ub, ub)
    gp = np.einsum("cqai,ca->cqi", grad, pe)
    pq = np.einsum("qa,ca->cq", phi, pe)
    f = np.asarray(prm.f, dtype=float)[None, None, :]
    R = rho * (w + Cr) + gp - rho * f
    tau, tauL = G3.tau_pair(np.einsum("cqi,cqi->cq", unq, unq), h[:, None], prm)
    bgr = np.einsum("cqi,cqai->cqa", ub, grad)
    dv = adet[:, None] * (el.w * el.meas)[None, :]

    Fu = np.einsum("cq,qa,cqi->cai", dv, phi, rho * (w + Cr - f))
    Fu += mu * np.einsum("cq,cqm,cqaim->cai", dv, om, cb)
    Fu -= np.einsum("cq,cqai->cai", dv * (pq + ke), grad)
    Fu += np.einsum("cq,cq,cqi,cqa->cai", dv, tau, R, bgr)
    Fu += np.einsum("cq,cqai->cai", dv * tauL * rho * divu, grad)
    Fp = np.einsum("cq,qa,cq->ca", dv, phi, divu) + np.einsum("cq,cq,cqi,cqai->ca", dv, tau / rho, R, grad)

    Je = None
    if want_jac:
        I3 = np.eye(3)
        # d (omega x ubar)_i / d u_(b,j) / theta = (curl(phi_b e_j) x ubar)_i + phi_b (omega x e_j)_i
        dC = np.einsum("ikl,cqbjk,cql->cqbij", EPS, cb, ub) + np.einsum("qb,ikj,cqk->cqbij", phi, EPS, om)
        dR = rho * (a0 / dt * np.einsum("qb,ij->qbij", phi, I3)[None] + th * dC)
        Juu = np.einsum("cq,qa,cqbij->caibj", dv, phi, dR)
        Juu += mu * th * np.einsum("cq,cqaim,cqbjm->caibj", dv, cb, cb)
        Juu -= rho * th * np.einsum("cq,qb,cqj,cqai->caibj", dv, phi, ub, grad)
        Juu += np.einsum("cq,cq,cqbij,cqa->caibj", dv, tau, dR, bgr)
        Juu += th * np.einsum("cq,cq,cqi,qb,cqaj->caibj", dv, tau, R, phi, grad)
        Juu += rho * th * np.einsum("cq,cq,cqbj,cqai->caibj", dv, tauL, grad, grad)
        Jup = -np.einsum("cq,qb,cqai->caib", dv, phi, grad) + np.einsum("cq,cq,cqbi,cqa->caib", dv, tau, grad, bgr)
        Jpu = th * np.einsum("cq,qa,cqbj->cabj", dv, phi, grad) + np.einsum("cq,cq,cqbij,cqai->cabj", dv, tau / rho, dR, grad)
        Jpp = np.einsum("cq,cq,cqbi,cqai->cab", dv, tau / rho, grad, grad)

    if pval is not None:
        for fl in range(len(el.facets)):
            sel = np.nonzero(~np.isnan(pval[:, fl]))[0]
            if len(sel) == 0:
                continue
            n, area = G3.facet_geometry(el, x, cells, sel, fl)            # outward unit normals [c,3], measures [c]
            fphi = el.fphi[fl]                                              # [qf, a]
            fgrad = np.einsum("qak,cki->cqai", el.fdphi[fl], Jinv[sel])     # [c,qf,a,i]
            fcb = _curl_basis(fgrad)                                        # [c,qf,a,i,m]
            cbn = np.cross(fcb, n[:, None, None, None, :])                  # curl(phi_a e_i) x n
            m = area[:, None] * el.fw[None, :]                              # [c,qf]
            ubf = np.einsum("qa,cai->cqi", fphi, ubn[sel])
            Gf = np.einsum("cqai,caj->cqij", fgrad, ubn[sel])
            omf = np.einsum("ijk,cqjk->cqi", EPS, Gf)
            uT = ubf - np.einsum("cqi,ci->cq", ubf, n)[..., None] * n[:, None, :]
            nit = beta * mu / h[sel]
            Pk = pval[sel, fl]
            Fu[sel] += np.einsum("cq,qa,ci->cai", m, fphi, Pk[:, None] * n)
            Fu[sel] += np.einsum("cq,qa,cqi->cai", m, fphi, nit[:, None, None] * uT - mu * np.cross(omf, n[:, None, :]))
            Fu[sel] -= mu * np.einsum("cq,cqaim,cqm->cai", m, cbn, ubf)
            if want_jac:
                PT = np.eye(3)[None] - np.einsum("ci,cj->cij", n, n)
                Juu[sel] += th * (-mu * np.einsum("cq,qa,cqbji->caibj", m, fphi, cbn)
                                  - mu * np.einsum("cq,cqaij,qb->caibj", m, cbn, fphi)
                                  + np.einsum("cq,qa,qb,cij->caibj", m * nit[:, None], fphi, fphi, PT))
    if want_jac:
        Je = np.zeros((nc, 4 * nl, 4 * nl))
        Je[:, : 3 * nl, : 3 * nl] = Juu.reshape(nc, 3 * nl, 3 * nl)
        Je[:, : 3 * nl, 3 * nl:] = Jup.reshape(nc, 3 * nl, nl)
        Je[:, 3 * nl:, : 3 * nl] = Jpu.reshape(nc, nl, 3 * nl)
        Je[:, 3 * nl:, 3 * nl:] = Jpp
    Fe = np.concatenate([Fu.reshape(nc, 3 * nl), Fp], axis=1)
    return Fe, Je


class Problem(G3.Problem):
    """np_twin_gen3.Problem (assembly, Dirichlet handling, direct-solve Newton) with the rotational element tensors and pressure
    boundaries in place of the convective form's facet terms."""

    def __init__(self, etype, x, cells, facet_cells, facet_local, prm):
        super().__init__(etype, x, cells, facet_cells, facet_local, prm)
        self.prm.ds_terms, self.prm.beta_backflow = False, 0.0
        self.pval = None
        self.beta = 0.0

    def set_pressure_boundaries(self, facet_sets, values, beta=0.0):
        """facet_sets[k]: exterior facet ids of boundary k (value values[k])."""
        pv = np.full((self.nc, len(self.el.facets)), np.nan)
        for fs, val in zip(facet_sets, values):
            fs = np.asarray(fs, dtype=np.int64)
            pv[self.facet_cells[fs], self.facet_local[fs]] = float(val)
        self.pval = pv if len(facet_sets) else None
        self.beta = float(beta)

    def _tensors(self, etype, x, cells, u, un, p, prm, facet_flags=None, want_jac=True, un2=None):
        return element_tensors_rot3(etype, x, cells, u, un, p, prm, self.pval, self.beta, want_jac=want_jac, un2=un2)

    def assemble(self, xvec, un, want_jac=True, apply_bc=True, un2=None):
        saved = G3.element_tensors
        G3.element_tensors = self._tensors   # the parent's assembly calls the module-level element routine
        try:
            return super().assemble(xvec, un, want_jac=want_jac, apply_bc=apply_bc, un2=un2)
        finally:
            G3.element_tensors = saved
