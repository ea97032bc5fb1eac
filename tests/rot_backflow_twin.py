"""NumPy twin of the rotational form with per-boundary switches  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Restates the boundary terms of the reference's src/solvers/stabilized_schur_vascularbc_backflow.py:214-244 on top of the twins of the
rotational form (tests/rot_twin.py, tests/rot_twin3.py), whose volume form, Nitsche boundaries, assembly and Newton are reused by
import.  Pressure boundary k (value P_k, outward n) carries two switches:

  nitsche[k]   on:  P_k v . n and the three tangential terms, exactly as in rot_twin / rot_twin3 (the inlet);
               off: P_k v . n alone (a pure traction boundary, the outlet);
  beta_bf[k]:  - beta_bf[k] rho (u_prev . n)_- (ubar . v),  (s)_- = (s - |s|) / 2,  ubar = theta u + (1 - theta) u_prev  (:237-244, the
               term of stabilized_schur_backflow.py:166-176).  The coefficient is taken from u_prev, so the Jacobian gains
               theta (- beta_bf[k] rho (u_prev . n)_-) phi_a phi_b delta_ij in the velocity block and nothing else.

The boundaries with the Nitsche switch on go through the parent twin unchanged (same arithmetic: with every switch on and every
beta_bf = 0 the element tensors are the parent's, bit for bit); the rest is added here with the elements' own facet tables
(el.fphi, el.fw; normals and facet measures as the parent twins form them).
"""
from __future__ import annotations

import numpy as np

from oracle import np_twin_gen as G, np_twin_gen3 as G3
import rot_twin as RT
import rot_twin3 as RT3


def _facet_geometry(dim, el, x, cells, sel, fl):
    """Outward unit normals [c, dim] and measures [c] of local facet fl of the cells sel."""
    if dim == 3:
        return G3.facet_geometry(el, x, cells, sel, fl)
    va, vb = el.facets[fl]
    xa, xb = x[cells[sel, va]], x[cells[sel, vb]]
    tv = xb - xa
    elen = np.linalg.norm(tv, axis=1)
    n = np.stack([tv[:, 1], -tv[:, 0]], axis=1) / elen[:, None]
    cen = x[cells[sel][:, : el.nvert]].mean(axis=1)
    n *= np.sign(np.einsum("ci,ci->c", 0.5 * (xa + xb) - cen, n))[:, None]
    return n, elen


class _Switches:
    """Mixin over rot_twin.Problem / rot_twin3.Problem: per-boundary Nitsche switch and backflow coefficient."""
    DIM = 2

    def __init__(self, etype, x, cells, facet_cells, facet_local, prm):
        super().__init__(etype, x, cells, facet_cells, facet_local, prm)
        self.set_pressure_boundaries([], [])

    def set_pressure_boundaries(self, facet_sets, values, beta=0.0, nitsche=None, beta_backflow=None):
        """facet_sets[k]: exterior facet ids of boundary k (value values[k]); nitsche[k] (None: all on), beta_backflow[k] (None: 0)."""
        n = len(facet_sets)
        nitsche = [True] * n if nitsche is None else [bool(s) for s in nitsche]
        beta_backflow = [0.0] * n if beta_backflow is None else [float(b) for b in beta_backflow]
        assert len(values) == n and len(nitsche) == n and len(beta_backflow) == n and all(b >= 0 for b in beta_backflow)
        on = [k for k in range(n) if nitsche[k]]
        super().set_pressure_boundaries([facet_sets[k] for k in on], [values[k] for k in on], beta)
        nf = len(self.el.facets)
        self.pv_off = np.full((self.nc, nf), np.nan)   # P_k on the facets of the boundaries without tangential terms
        self.bf = np.zeros((self.nc, nf))              # beta_bf on the facets that carry the backflow term
        self.pb_sets = [np.asarray(fs, dtype=np.int64) for fs in facet_sets]
        for k, fs in enumerate(self.pb_sets):
            if not nitsche[k]:
                self.pv_off[self.facet_cells[fs], self.facet_local[fs]] = float(values[k])
            self.bf[self.facet_cells[fs], self.facet_local[fs]] = beta_backflow[k]

    def prev_normal_velocity(self, un, k):
        """u_prev . n at the facet points of pressure boundary k: [facet of the set, point]."""
        el, d = self.el, self.DIM
        un = np.asarray(un).reshape(-1, d)
        out = []
        for f in self.pb_sets[k]:
            c, fl = self.facet_cells[f], self.facet_local[f]
            n, _ = _facet_geometry(d, el, self.x, self.cells, np.array([c]), fl)
            out.append(el.fphi[fl] @ un[self.cells[c]] @ n[0])
        return np.array(out)

    def _tensors(self, etype, x, cells, u, un, p, prm, facet_flags=None, want_jac=True, un2=None):
        Fe, Je = super()._tensors(etype, x, cells, u, un, p, prm, facet_flags, want_jac=want_jac, un2=un2)
        el, d = self.el, self.DIM
        nl, th, rho = el.nloc, prm.theta, prm.rho
        ubn = th * u[cells] + (1.0 - th) * un[cells]
        une = un[cells]
        for fl in range(len(el.facets)):
            off, bfs = ~np.isnan(self.pv_off[:, fl]), self.bf[:, fl] != 0.0
            sel = np.nonzero(off | bfs)[0]
            if len(sel) == 0:
                continue
            n, meas = _facet_geometry(d, el, x, cells, sel, fl)
            fphi = el.fphi[fl]                                              # [qf, a]
            m = meas[:, None] * el.fw[None, :]                              # [c, qf]
            Pk = np.where(off[sel], self.pv_off[sel, fl], 0.0)
            sn = np.einsum("qa,cai,ci->cq", fphi, une[sel], n)              # u_prev . n
            cq = self.bf[sel, fl][:, None] * rho * 0.5 * (sn - np.abs(sn)) * m
            ubf = np.einsum("qa,cai->cqi", fphi, ubn[sel])
            Fu = np.einsum("cq,qa,ci->cai", m, fphi, Pk[:, None] * n) - np.einsum("cq,qa,cqi->cai", cq, fphi, ubf)
            Fe[sel, : d * nl] += Fu.reshape(len(sel), d * nl)
            if Je is not None:
                Juu = -th * np.einsum("cq,qa,qb,ij->caibj", cq, fphi, fphi, np.eye(d))
                Je[sel, : d * nl, : d * nl] += Juu.reshape(len(sel), d * nl, d * nl)
        return Fe, Je


class Problem(_Switches, RT.Problem):
    DIM = 2


class Problem3(_Switches, RT3.Problem):
    DIM = 3
