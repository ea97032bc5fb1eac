"""NumPy twin of the rotational form of the pressure-driven solvers  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Restates /root/reference/src/solvers/stabilized_schur_pressurebc.py:123-160 (volume) and :177-205 (facets) for the nodal 2-D
elements of oracle/np_twin_gen.py (P1 / P2 triangles, Q1 parallelograms), whose element tables, cell geometry, tau pair, assembly
with Dirichlet handling and direct-solve Newton are reused by import.  With ubar = theta u + (1 - theta) u_prev,
w_t = (a0 u + a1 u_prev + a2 u_prev2)/dt, omega(w) = d_x w_y - d_y w_x and omega x a := (-omega a_y, omega a_x):

  F =  rho w_t . v + mu omega(ubar) omega(v) - p div v + rho (omega(ubar) x ubar) . v - rho/2 |ubar|^2 div v - rho f . v
     + q div ubar + tau R_i ubar_k d_k v_i + (tau/rho) R . grad q + tau_L rho div ubar div v,
  R  = rho (w_t + omega(ubar) x ubar) + grad p - rho f                 (no viscous part, :142-144)

and on the facets of pressure boundary k (value P_k, outward n, tangent t = (-n_y, n_x), h of the owning cell):

  + P_k v . n - mu omega(ubar) (t . v) - mu omega(v) (t . ubar) + (beta mu / h) (t . ubar)(t . v)

(in 2-D (omega x n) . v_T = omega (t . v) and (omega(v) x n) . ubar_T = omega(v) (t . ubar)).  The ds pair and the backflow term of
the convective form do not exist here.  Jacobian: the exact derivative (theta times the derivative in ubar plus the time term).
"""
from __future__ import annotations

import numpy as np

from oracle import np_twin_gen as G


def element_tensors_rot(etype, x, cells, u, un, p, prm, pval=None, beta=0.0, want_jac=True, un2=None):
    """Fe [nc, 3 nloc], Je [nc, 3 nloc, 3 nloc] of the rotational form.  pval [nc, nfacets]: P_k of the pressure boundary holding
    local facet f of the cell, NaN elsewhere."""
    el = G.element(etype)
    nl, nc = el.nloc, len(cells)
    rho, mu, dt, th, a0 = prm.rho, prm.mu, prm.dt, prm.theta, prm.a0
    Jinv, adet, h, _ = G.cell_geometry(el, x, cells)
    ue, une, pe = u[cells], un[cells], p[cells]
    ubn = th * ue + (1.0 - th) * une
    wn = (a0 * ue + prm.a1 * une) / dt
    if prm.a2 != 0.0:
        wn = wn + prm.a2 * un2[cells] / dt
    phi = el.phi
    grad = np.einsum("qak,cki->cqai", el.dphi, Jinv)             # [c,q,a,i]
    oma = np.stack([-grad[..., 1], grad[..., 0]], axis=-1)       # omega(phi_a e_i)
    ub = np.einsum("qa,cai->cqi", phi, ubn)
    w = np.einsum("qa,cai->cqi", phi, wn)
    unq = np.einsum("qa,cai->cqi", phi, une)
    Gd = np.einsum("cqai,caj->cqij", grad, ubn)                  # d_i ubar_j
    divu = Gd[..., 0, 0] + Gd[..., 1, 1]
    om = Gd[..., 0, 1] - Gd[..., 1, 0]
    Cr = np.stack([-om * ub[..., 1], om * ub[..., 0]], axis=-1)
    ke = 0.5 * rho * np.einsum("cqi,cqi->cq", ub, ub)
    gp = np.einsum("cqai,ca->cqi", grad, pe)
    pq = np.einsum("qa,ca->cq", phi, pe)
    f = prm.f[None, None, :]
    R = rho * (w + Cr) + gp - rho * f
    tau, tauL = G.tau_pair(np.einsum("cqi,cqi->cq", unq, unq), h[:, None], prm)
    bgr = np.einsum("cqi,cqai->cqa", ub, grad)
    dv = adet[:, None] * (el.w * el.meas)[None, :]

    Fu = np.einsum("cq,qa,cqi->cai", dv, phi, rho * (w + Cr - f))
    Fu += np.einsum("cq,cqai->cai", dv * mu * om, oma)
    Fu -= np.einsum("cq,cqai->cai", dv * (pq + ke), grad)
    Fu += np.einsum("cq,cq,cqi,cqa->cai", dv, tau, R, bgr)
    Fu += np.einsum("cq,cqai->cai", dv * tauL * rho * divu, grad)
    Fp = np.einsum("cq,qa,cq->ca", dv, phi, divu) + np.einsum("cq,cq,cqi,cqai->ca", dv, tau / rho, R, grad)

    Je = None
    if want_jac:
        I2 = np.eye(2)
        # d (omega x ubar)_i / d u_(b,j) / theta = omega(phi_b e_j) x ubar + omega x (phi_b e_j)
        dC = np.zeros((nc, len(el.w), nl, 2, 2))
        dC[..., 0, :] = -oma * ub[:, :, None, None, 1]
        dC[..., 1, :] = oma * ub[:, :, None, None, 0]
        dC[..., 0, 1] -= om[:, :, None] * phi[None]
        dC[..., 1, 0] += om[:, :, None] * phi[None]
        dR = rho * (a0 / dt * np.einsum("qb,ij->qbij", phi, I2)[None] + th * dC)
        Juu = np.einsum("cq,qa,cqbij->caibj", dv, phi, dR)
        Juu += mu * th * np.einsum("cq,cqai,cqbj->caibj", dv, oma, oma)
        Juu -= rho * th * np.einsum("cq,qb,cqj,cqai->caibj", dv, phi, ub, grad)
        Juu += np.einsum("cq,cq,cqbij,cqa->caibj", dv, tau, dR, bgr)
        Juu += th * np.einsum("cq,cq,cqi,qb,cqaj->caibj", dv, tau, R, phi, grad)
        Juu += rho * th * np.einsum("cq,cq,cqbj,cqai->caibj", dv, tauL, grad, grad)
        Jup = -np.einsum("cq,qb,cqai->caib", dv, phi, grad) + np.einsum("cq,cq,cqbi,cqa->caib", dv, tau, grad, bgr)
        Jpu = th * np.einsum("cq,qa,cqbj->cabj", dv, phi, grad) + np.einsum("cq,cq,cqbij,cqai->cabj", dv, tau / rho, dR, grad)
        Jpp = np.einsum("cq,cq,cqbi,cqai->cab", dv, tau / rho, grad, grad)

    if pval is not None:
        cen = x[cells[:, : el.nvert]].mean(axis=1)
        for fl, (va, vb) in enumerate(el.facets):
            sel = np.nonzero(~np.isnan(pval[:, fl]))[0]
            if len(sel) == 0:
                continue
            xa, xb = x[cells[sel, va]], x[cells[sel, vb]]
            tv = xb - xa
            elen = np.linalg.norm(tv, axis=1)
            n = np.stack([tv[:, 1], -tv[:, 0]], axis=1) / elen[:, None]
            n *= np.sign(np.einsum("ci,ci->c", 0.5 * (xa + xb) - cen[sel], n))[:, None]   # outward
            t = np.stack([-n[:, 1], n[:, 0]], axis=1)
            fphi = el.fphi[fl]                                              # [qf, a]
            fgrad = np.einsum("qak,cki->cqai", el.fdphi[fl], Jinv[sel])     # [c,qf,a,i]
            foma = np.stack([-fgrad[..., 1], fgrad[..., 0]], axis=-1)
            m = elen[:, None] * el.fw[None, :]                              # [c,qf]
            ubf = np.einsum("qa,cai->cqi", fphi, ubn[sel])
            Gf = np.einsum("cqai,caj->cqij", fgrad, ubn[sel])
            omf = Gf[..., 0, 1] - Gf[..., 1, 0]
            ut = np.einsum("cqi,ci->cq", ubf, t)
            nit = beta * mu / h[sel]
            Pk = pval[sel, fl]
            Fu[sel] += np.einsum("cq,qa,ci->cai", m, fphi, Pk[:, None] * n)
            Fu[sel] += np.einsum("cq,qa,ci->cai", m * (nit[:, None] * ut - mu * omf), fphi, t)
            Fu[sel] -= mu * np.einsum("cq,cqai->cai", m * ut, foma)
            if want_jac:
                Juu[sel] += th * (-mu * np.einsum("cq,cqbj,qa,ci->caibj", m, foma, fphi, t)
                                  - mu * np.einsum("cq,cqai,qb,cj->caibj", m, foma, fphi, t)
                                  + np.einsum("cq,qa,ci,qb,cj->caibj", m * nit[:, None], fphi, t, fphi, t))
    if want_jac:
        Je = np.zeros((nc, 3 * nl, 3 * nl))
        Je[:, : 2 * nl, : 2 * nl] = Juu.reshape(nc, 2 * nl, 2 * nl)
        Je[:, : 2 * nl, 2 * nl:] = Jup.reshape(nc, 2 * nl, nl)
        Je[:, 2 * nl:, : 2 * nl] = Jpu.reshape(nc, nl, 2 * nl)
        Je[:, 2 * nl:, 2 * nl:] = Jpp
    Fe = np.concatenate([Fu.reshape(nc, 2 * nl), Fp], axis=1)
    return Fe, Je


class Problem(G.Problem):
    """np_twin_gen.Problem (assembly, Dirichlet handling, direct-solve Newton) with the rotational element tensors and pressure
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
        return element_tensors_rot(etype, x, cells, u, un, p, prm, self.pval, self.beta, want_jac=want_jac, un2=un2)

    def assemble(self, xvec, un, want_jac=True, apply_bc=True, un2=None):
        saved = G.element_tensors
        G.element_tensors = self._tensors   # the parent's assembly calls the module-level element routine
        try:
            return super().assemble(xvec, un, want_jac=want_jac, apply_bc=apply_bc, un2=un2)
        finally:
            G.element_tensors = saved
