"""NumPy restatement of the volumetric flow diagnostics (include/cfdh.h, cfdh_flow_*), definition by definition and in the stated
summation order: the recovery of a vertex adds its cells in ascending cell index, one after the other.  The cell gradients come from
numpy.linalg.inv of the edge matrix, not from the cofactor formulas of the kernels.  Shared by test_flow_twin.py (CPU) and
test_gpu_flow.py (GPU)."""
import math

import numpy as np

SLICE = 64


def cell_gradients(x, cells, u):
    """|c| [nc] and G_c[i][j] = d u_i / d x_j [nc, d, d] of the P1 field u [nv, d]."""
    x, u = np.asarray(x, dtype=float), np.asarray(u, dtype=float)
    d = cells.shape[1] - 1
    X, U = x[cells], u[cells]
    E = X[:, 1:] - X[:, :1]                  # E[c, k] = x_{k+1} - x_0
    vol = np.abs(np.linalg.det(E)) / math.factorial(d)
    g = np.linalg.inv(E)                     # g[c, :, k] = grad lambda_{k+1}
    dU = U[:, 1:] - U[:, :1]                 # dU[c, k, i]
    G = np.einsum("cki,cjk->cij", dU, g)
    return vol, G


def vertex_cells(nv, cells):
    """The cells of every vertex in ascending cell index: rptr [nv + 1], inc [ninc]."""
    n1 = cells.shape[1]
    vert = cells.ravel()
    cell = np.repeat(np.arange(len(cells)), n1)
    order = np.lexsort((cell, vert))
    rptr = np.zeros(nv + 1, dtype=np.int64)
    np.add.at(rptr, vert + 1, 1)
    return np.cumsum(rptr), cell[order].astype(np.int32)


def sliced(nv, rptr, inc):
    """The by-row lists in the slice layout of cfdh_flow_host.hpp: sptr [nslices + 1], dinc [sptr[-1] * 64] (-1: no incidence)."""
    ns = (nv + SLICE - 1) // SLICE
    length = np.diff(rptr)
    sptr = np.zeros(ns + 1, dtype=np.int64)
    for s in range(ns):
        sptr[s + 1] = sptr[s] + length[s * SLICE:(s + 1) * SLICE].max(initial=0)
    dinc = np.full(sptr[-1] * SLICE, -1, dtype=np.int32)
    for v in range(nv):
        s, lane = divmod(v, SLICE)
        for j in range(length[v]):
            dinc[(sptr[s] + j) * SLICE + lane] = inc[rptr[v] + j]
    return sptr, dinc


def recover(nv, cells, vol, G):
    """G_v = sum |c| G_c / sum |c| over the cells of v in ascending cell index, added one by one (column k of all rows at once)."""
    rptr, inc = vertex_cells(nv, cells)
    d = G.shape[1]
    num, den = np.zeros((nv, d, d)), np.zeros(nv)
    length = np.diff(rptr)
    for k in range(int(length.max(initial=0))):
        rows = np.nonzero(length > k)[0]
        c = inc[rptr[rows] + k]
        den[rows] += vol[c]
        num[rows] += vol[c][:, None, None] * G[c]
    out = np.zeros_like(num)
    ok = den > 0
    out[ok] = num[ok] / den[ok][:, None, None]
    return out


def vorticity(G):
    """[n] in 2-D, [n, 3] in 3-D, of gradients G [n, d, d]."""
    if G.shape[1] == 2:
        return G[:, 1, 0] - G[:, 0, 1]
    return np.stack([G[:, 2, 1] - G[:, 1, 2], G[:, 0, 2] - G[:, 2, 0], G[:, 1, 0] - G[:, 0, 1]], axis=1)


def strain_sq(G):
    S = 0.5 * (G + G.transpose(0, 2, 1))
    return np.einsum("nij,nij->n", S, S)


def spin_sq(G):
    W = 0.5 * (G - G.transpose(0, 2, 1))
    return np.einsum("nij,nij->n", W, W)


def q_criterion(G):
    return 0.5 * (spin_sq(G) - strain_sq(G))


def shear_rate(G):
    return np.sqrt(2.0 * strain_sq(G))


def dissipation(G, mu):
    return 2.0 * mu * strain_sq(G)


def helicity(u, G):
    return np.einsum("ni,ni->n", u, vorticity(G))


def lnh(u, G):
    """u . omega / (|u| |omega|), exactly 0 where either norm is 0; also returns |u| |omega|."""
    w = vorticity(G)
    nu, nw = np.linalg.norm(u, axis=1), np.linalg.norm(w, axis=1)
    prod = nu * nw
    out = np.zeros(len(u))
    ok = (nu != 0) & (nw != 0)
    out[ok] = np.einsum("ni,ni->n", u, w)[ok] / prod[ok]
    return out, prod


def fields(x, cells, u, mu):
    """Every vertex field of cfdh_flow_field, keyed as Scenario.solve names them (plus "gradient")."""
    x, u = np.asarray(x, dtype=float), np.asarray(u, dtype=float)
    vol, G = cell_gradients(x, cells, u)
    Gv = recover(len(x), cells, vol, G)
    out = dict(gradient=Gv, vorticity=vorticity(Gv), q_criterion=q_criterion(Gv), shear_rate=shear_rate(Gv), dissipation=dissipation(Gv, mu))
    if Gv.shape[1] == 3:
        out["helicity"] = helicity(u, Gv)
        out["lnh"], out["lnh_weight"] = lnh(u, Gv)
    return out


def integrals(x, cells, u, rho, mu):
    """The 8 integrals of cfdh_flow_integrals."""
    x, u = np.asarray(x, dtype=float), np.asarray(u, dtype=float)
    d = cells.shape[1] - 1
    vol, G = cell_gradients(x, cells, u)
    U = u[cells]
    w = vorticity(G)
    w2 = w * w if d == 2 else np.einsum("ci,ci->c", w, w)
    sq = np.einsum("cai,cai->c", U, U)
    sm = U.sum(axis=1)
    div = np.trace(G, axis1=1, axis2=2)
    out = np.zeros(8)
    out[0] = vol.sum()
    out[1] = 0.5 * rho * (vol * (sq + np.einsum("ci,ci->c", sm, sm))).sum() / ((d + 1) * (d + 2))
    out[2] = 0.5 * (vol * w2).sum()
    out[3] = (vol * dissipation(G, mu)).sum()
    out[4] = (vol * np.einsum("ci,ci->c", sm / (d + 1), w)).sum() if d == 3 else 0.0
    out[5] = (vol * div).sum()
    out[6] = (vol * q_criterion(G)).sum()
    out[7] = (vol * div * div).sum()
    return out


class Window:
    """The accumulators of cfdh_flow_stats_*."""

    def __init__(self, x, cells, mu):
        self.x, self.cells, self.mu = np.asarray(x, dtype=float), cells, mu
        self.reset()

    def reset(self):
        nv, d = self.x.shape
        self.sU, self.sU2, self.sPhi, self.sGam, self.sMax = np.zeros((nv, d)), np.zeros(nv), np.zeros(nv), np.zeros(nv), np.zeros(nv)
        self.W, self.count = 0.0, 0

    def accumulate(self, u, w):
        f = fields(self.x, self.cells, u, self.mu)
        self.sU += w * u
        self.sU2 += w * np.einsum("ni,ni->n", u, u)
        self.sPhi += w * f["dissipation"]
        self.sGam += w * f["shear_rate"]
        self.sMax = np.maximum(self.sMax, f["shear_rate"])
        self.W += w
        self.count += 1

    def get(self):
        m = self.sU / self.W
        return dict(mean_velocity=m, fluctuation=np.maximum(0.0, 0.5 * (self.sU2 / self.W - np.einsum("ni,ni->n", m, m))),
                    mean_dissipation=self.sPhi / self.W, mean_shear_rate=self.sGam / self.W, peak_shear_rate=self.sMax.copy())
