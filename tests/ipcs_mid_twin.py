"""NumPy/SciPy twin of the pressure-correction scheme `ipcs_midpoint` on P2/P1 simplices, on top of `ipcs_twin.Operators`: the
vector-coupled epsilon form at the midpoint with its ds pair and explicit convection (include/cfdh.h, cfdh_ipcs_set_scheme;
DESIGN.md section 9).  A second, independent writing: every integral is a quadrature sum of pointwise values, the facet normals
come from the coordinates.

Unknowns are interleaved, dof = d * node + component.  With sigma = 2 mu eps(u) - p I, eps = sym(nabla_grad):
  V = mu (K x I + E) - mu S,  E(ia, jb) = int d_b phi_i d_a phi_j,  S(ia, jb) = int_{dOmega} phi_i d_a phi_j n_b ds,
  Pn(ia, k) = int_{dOmega} phi_i psi_k n_a ds,  C(w)(ia) = int phi_i (w . grad) w_a
  1. A1 u* = b1,  A1_free = rho/dt M x I + V / 2,  b1 = (rho/dt M x I - V / 2) u_prev - c C(u_prev) + (B^T - Pn) p_prev + s_f f m1
  2. L phi = -rho/dt sum_d B_d u*_d with phi = g - p_prev on the pressure Dirichlet vertices;  p = p_prev + phi
  3. rho M u = rho M u* - dt G phi
c = rho; s_f = rho (`consistent=True`) or 1 (the reference's literal dot(f, v)).  `ds=False` leaves S and Pn out (the CPU test
uses it to show that the Poiseuille fixed point tells the ds pair apart).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import ipcs_twin as T


def facet_rule(dim, n=4):
    """Barycentric points on the reference facet [nq, dim] and weights summing to 1."""
    if dim == 2:
        g, w = np.polynomial.legendre.leggauss(n)
        g, w = (g + 1) / 2, w / 2
        return np.stack([1 - g, g], 1), w
    lam, w = T.simplex_rule(2, n)
    return lam, w / w.sum()


def facet_geometry(x, verts, opposite):
    """Outward unit normals [nf, d] and measures [nf] of the facets with vertex coordinates x[verts]; `opposite`: the cell's vertex
    that is not on the facet."""
    X = x[verts]
    d = X.shape[2]
    if d == 2:
        t = X[:, 1] - X[:, 0]
        n = np.stack([t[:, 1], -t[:, 0]], 1)
        meas = np.linalg.norm(t, axis=1)
    else:
        n = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
        meas = 0.5 * np.linalg.norm(n, axis=1)
    n = n / np.linalg.norm(n, axis=1)[:, None]
    sign = np.sign(np.einsum("fd,fd->f", n, X[:, 0] - x[opposite]))
    return n * sign[:, None], meas


class MidOperators:
    """E, S [d nn, d nn] and Pn [d nn, nvert] as CSR; C(w) [nn, d].  `facet_cells`, `facet_local`: ALL exterior facets (local
    index = the cell vertex opposite the facet)."""

    def __init__(self, op, facet_cells, facet_local):
        self.op = op
        d, nn, nv, nl = op.dim, op.nn, op.nvert, op.nloc
        self.fc, self.fl = np.asarray(facet_cells, dtype=np.int64), np.asarray(facet_local, dtype=np.int64)
        comp = np.arange(d)
        # E: rows (node a, alpha), columns (node b, beta)
        Ee = np.einsum("q,c,cqae,cqbf->cafbe", op.w, op.adet, op.gphi, op.gphi, optimize=True)       # [c, a, alpha=f, b, beta=e]: d_beta phi_a d_alpha phi_b
        rows = (d * op.c2[:, :, None, None, None] + comp[None, None, :, None, None]) + 0 * op.c2[:, None, None, :, None] + 0 * comp[None, None, None, None, :]
        cols = (d * op.c2[:, None, None, :, None] + comp[None, None, None, None, :]) + 0 * rows
        self.E = T._csr(rows, cols, Ee, (d * nn, d * nn))
        # facet terms, one local facet index at a time
        flam, fw = facet_rule(d)
        Sr, Sc, Sv, Pr, Pc, Pv = [], [], [], [], [], []
        self.facets = []
        for f in range(d + 1):
            sel = self.fc[self.fl == f]
            if len(sel) == 0:
                continue
            on = [v for v in range(d + 1) if v != f]
            lam = np.zeros((len(fw), d + 1))
            lam[:, on] = flam
            phi, dl = T.p2_tabulate(lam, d)
            c2, c1 = op.c2[sel], op.c1[sel]
            n, meas = facet_geometry(op.x, c1[:, on], c1[:, f])
            gphi = np.einsum("qae,ced->cqad", dl, op.gl[sel])
            self.facets.append((sel, lam, fw, phi, gphi, n, meas))
            Se = np.einsum("q,c,qa,cqbe,cf->caebf", fw, meas, phi, gphi, n, optimize=True)           # [c, a, alpha, b, beta]
            r = (d * c2[:, :, None, None, None] + comp[None, None, :, None, None]) + 0 * c2[:, None, None, :, None] + 0 * comp[None, None, None, None, :]
            c = (d * c2[:, None, None, :, None] + comp[None, None, None, None, :]) + 0 * r
            Sr.append(r.ravel()); Sc.append(c.ravel()); Sv.append(Se.ravel())
            Pe = np.einsum("q,c,qa,qv,ce->caev", fw, meas, phi, lam, n, optimize=True)               # [c, a, alpha, v]
            r = (d * c2[:, :, None, None] + comp[None, None, :, None]) + 0 * c1[:, None, None, :]
            c = c1[:, None, None, :] + 0 * r
            Pr.append(r.ravel()); Pc.append(c.ravel()); Pv.append(Pe.ravel())
        cat = lambda a: np.concatenate(a) if a else np.zeros(0)
        self.S = T._csr(cat(Sr).astype(np.int64), cat(Sc).astype(np.int64), cat(Sv), (d * nn, d * nn))
        self.Pn = T._csr(cat(Pr).astype(np.int64), cat(Pc).astype(np.int64), cat(Pv), (d * nn, nv))
        self.MI = sp.kron(op.M, sp.identity(d), format="csr")
        self.KI = sp.kron(op.K, sp.identity(d), format="csr")
        # B^T on the interleaved rows
        self.BT = sum(sp.kron(op.B[k].T, sp.csr_matrix(([1.0], ([k], [0])), shape=(d, 1))) for k in range(d)).tocsr()

    def C(self, w):
        """C(w)[i, a] = int phi_i (w . grad) w_a, from the values and gradients of w at the quadrature points (no matrix N)."""
        op = self.op
        wc = np.asarray(w)[op.c2]
        wq = np.einsum("qa,cad->cqd", op.phi, wc)
        conv = np.einsum("cqi,cqai,caj->cqj", wq, op.gphi, wc, optimize=True)
        Ce = np.einsum("q,c,qa,cqj->caj", op.w, op.adet, op.phi, conv, optimize=True)
        out = np.zeros((op.nn, op.dim))
        np.add.at(out, op.c2.ravel(), Ce.reshape(-1, op.dim))
        return out


class MidTwin:
    """The scheme on one mesh; the interface of `ipcs_twin.Twin` (`p` is the new pressure, `p_prev` the old one)."""

    def __init__(self, x, cells, nvert, facet_cells, facet_local, dt, rho, mu, f=None, consistent=True, bcu=(), bcp=(), tol=None, ops=None,
                 ds=True, mops=None):
        self.op = op = ops or T.Operators(x, cells, nvert)
        self.mo = mops or MidOperators(op, facet_cells, facet_local)
        d = op.dim
        self.dt, self.rho, self.mu = float(dt), float(rho), float(mu)
        self.f = np.zeros(d) if f is None else np.asarray(f, dtype=float)[:d]
        self.conv, self.sf = self.rho, (self.rho if consistent else 1.0)
        self.ds = bool(ds)
        self.tol = None if tol is None else np.broadcast_to(np.asarray(tol, dtype=float), (3,))
        self.u_prev, self.u_sol, self.u_star = np.zeros((op.nn, d)), np.zeros((op.nn, d)), np.zeros((op.nn, d))
        self.p_prev, self.p, self.phi = np.zeros(op.nvert), np.zeros(op.nvert), np.zeros(op.nvert)
        self.its = [0, 0, 0]
        self.rhoM = (self.rho * op.M).tocsr()
        self._A1 = self._Ms = self._Ls = self._A1s = None
        self.set_dirichlet(bcu, bcp)

    def set_dirichlet(self, bcu, bcp):
        op = self.op
        uflag, ucnt, self.uval = T.dirichlet_sets(op.nn, bcu, op.dim)
        new_set = getattr(self, "ucnt", None) is None or not np.array_equal(ucnt, self.ucnt)
        self.uflag, self.ucnt = uflag, ucnt
        pflag, pcnt, pval = T.dirichlet_sets(op.nvert, bcp, 1)
        if getattr(self, "pcnt", None) is None or not np.array_equal(pcnt, self.pcnt):
            self._Ls = None
            self.Lbc = T.constrain(op.L, pflag, pcnt)
        self.pflag, self.pcnt, self.pval = pflag, pcnt, pval[:, 0]
        self.singular = not self.pflag.any()
        if new_set:
            self._A1 = self._A1s = None

    def V(self):
        mo = self.mo
        V = self.mu * (mo.KI + mo.E)
        return (V - self.mu * mo.S).tocsr() if self.ds else V.tocsr()

    def A1_free(self):
        return (self.rho / self.dt * self.mo.MI + 0.5 * self.V()).tocsr()

    def matrix1(self):
        """(A1 with the Dirichlet treatment, A1_free); constant, cached."""
        if self._A1 is None:
            d = self.op.dim
            Af = self.A1_free()
            self._A1 = (T.constrain(Af, np.repeat(self.uflag, d), np.repeat(self.ucnt, d)), Af)
        return self._A1

    def assemble1(self):
        """A1 (constrained), b1 [nn, d] and the unconstrained matrix at the current state."""
        op, mo, d = self.op, self.mo, self.op.dim
        A1, Af = self.matrix1()
        up = self.u_prev.ravel()
        b = 2.0 * self.rho / self.dt * (mo.MI @ up) - Af @ up
        b += mo.BT @ self.p_prev
        if self.ds:
            b -= mo.Pn @ self.p_prev
        b = b.reshape(op.nn, d) + self.sf * op.m1[:, None] * self.f[None, :] - self.conv * mo.C(self.u_prev)
        g = np.where(self.uflag[:, None], self.uval, 0.0)
        b -= (Af @ g.ravel()).reshape(op.nn, d)
        b[self.uflag] = (self.ucnt[:, None] * self.uval)[self.uflag]
        return A1, b, Af

    def rhs2(self, us):
        op = self.op
        b = -self.rho / self.dt * sum(op.B[k] @ us[:, k] for k in range(op.dim))
        g = np.where(self.pflag, self.pval - self.p_prev, 0.0)
        b = b - op.L @ g
        b[self.pflag] = (self.pcnt * (self.pval - self.p_prev))[self.pflag]
        return b

    def rhs3(self, us, ph):
        op = self.op
        return self.rho * (op.M @ us) - self.dt * np.stack([op.G[k] @ ph for k in range(op.dim)], 1)

    def solve2(self, b2):
        if self.tol is not None:
            ph, self.its[1] = T.cg_jacobi(self.Lbc, b2, np.zeros_like(b2), self.tol[1], mean_free=self.singular)
            return ph
        n = self.op.nvert
        if self._Ls is None:
            if self.singular:
                one = np.ones((n, 1))
                self._Ls = spl.splu(sp.bmat([[self.Lbc, one], [one.T, None]]).tocsc())
            else:
                self._Ls = spl.splu(self.Lbc.tocsc())
        return self._Ls.solve(np.append(b2, 0.0))[:n] if self.singular else self._Ls.solve(b2)

    def step(self):
        op, d = self.op, self.op.dim
        A1, b1, _ = self.assemble1()
        if self.tol is not None:
            us, self.its[0] = T.bicgstab_jacobi(A1, b1.ravel(), self.u_star.ravel(), self.tol[0])
        else:
            if self._A1s is None:
                self._A1s = spl.splu(A1.tocsc())
            us = self._A1s.solve(b1.ravel())
        us = us.reshape(op.nn, d)
        b2 = self.rhs2(us)
        ph = self.solve2(b2)
        b3 = self.rhs3(us, ph)
        if self.tol is not None:
            u, self.its[2] = T.cg_jacobi(self.rhoM, b3, self.u_sol, self.tol[2])
        else:
            if self._Ms is None:
                self._Ms = spl.splu(self.rhoM.tocsc())
            u = self._Ms.solve(b3)
        self.A1, self.b1, self.b2, self.b3 = A1, b1, b2, b3
        self.u_star, self.phi, self.u_sol = us, ph, u
        self.p = self.p_prev + ph

    def advance(self):
        self.u_prev = self.u_sol.copy()
        self.p_prev = self.p.copy()


def taylor_green(nx, dt, nsteps, rho=1.0, mu=1.0 / 50.0, tol=None):
    """The decaying Taylor-Green vortex of `ipcs_twin.taylor_green` (exact velocity on the whole boundary at the step's new time
    level, no pressure condition) for `nsteps` steps.  Returns (relative L2 velocity error at the end, the twin)."""
    from cfd_hemodynamic_amd.elements import NodeMesh
    from cfd_hemodynamic_amd.mesh import create_unit_square
    m = create_unit_square(nx, nx)
    nm = NodeMesh(m)
    k, nu = 2 * np.pi, mu / rho

    def ue(x, t):
        dec = np.exp(-2 * nu * k * k * t)
        return np.stack([-np.cos(k * x[:, 0]) * np.sin(k * x[:, 1]) * dec, np.sin(k * x[:, 0]) * np.cos(k * x[:, 1]) * dec], 1)

    x = nm.x
    bnd = np.unique(nm.facet_vertices.ravel())
    tw = MidTwin(nm.x, nm.cells, m.num_vertices, nm.facet_cells, nm.facet_local, dt, rho, mu, tol=tol)
    tw.u_prev = ue(x, 0.0)
    t = 0.0
    for _ in range(nsteps):
        t += dt
        tw.set_dirichlet([(bnd, ue(x[bnd], t))], [])
        tw.step()
        tw.advance()
    ex = ue(x, t)
    return T.l2_norm(tw.op.M, tw.u_sol - ex) / T.l2_norm(tw.op.M, ex), tw
