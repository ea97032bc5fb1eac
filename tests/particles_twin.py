"""NumPy restatement of the particle step of include/cfdh.h (cfdh_particles_*): explicit midpoint substeps in the P1 velocity
w(x, s) = (1 - s) u_prev(x) + s u_sol(x), the cell-to-cell walk, the stop at the first exterior facet, the walk cap, path length and
shear exposure.  The tables are NumPy arrays; the arithmetic of one particle runs on Python floats (IEEE doubles, no fused
multiply-add) in the order the header states it, so that a decision of the walk falls the same way as on the device unless it is a
near-tie.  To find those, every particle carries the smallest margin of any decision it took:
  |lambda_f(y) + 1e-12| at an inside test, |t_f - t_g| between the two best facets of a crossing."""
import math

import numpy as np

TOL_INSIDE = 1e-12
TOL_SEED = 1e-9
MAX_CROSSINGS = 64
INSIDE, EXIT, LOST = 0, 1, 2


def neighbours(cells, facet_cells, facet_local):
    """nb [nc, d + 1]: the cell across local facet f (opposite local vertex f), -1 - k for exterior facet k of the facet list."""
    cells = np.asarray(cells)
    nc, n1 = cells.shape
    seen = {}
    nb = np.full((nc, n1), np.iinfo(np.int32).min, dtype=np.int64)
    for e in range(nc):
        for f in range(n1):
            key = tuple(sorted(int(v) for a, v in enumerate(cells[e]) if a != f))
            if key in seen:
                e2, f2 = seen.pop(key)
                nb[e, f], nb[e2, f2] = e2, e
            else:
                seen[key] = (e, f)
    for k, (e, f) in enumerate(zip(facet_cells, facet_local)):
        assert nb[e, f] == np.iinfo(np.int32).min
        nb[e, f] = -1 - k
    assert (nb != np.iinfo(np.int32).min).all(), "an exterior facet is missing from the facet list"
    return nb


def affine(x, cells):
    """aff [nc, d d + d]: grad(lambda_1) .. grad(lambda_d), then the coordinates of local vertex 0."""
    X = np.asarray(x, dtype=float)[np.asarray(cells)]
    d = X.shape[2]
    r = X[:, 1:, :] - X[:, :1, :]
    aff = np.zeros((len(X), d * d + d))
    if d == 2:
        det = r[:, 0, 0] * r[:, 1, 1] - r[:, 0, 1] * r[:, 1, 0]
        aff[:, 0], aff[:, 1] = r[:, 1, 1] / det, -r[:, 1, 0] / det
        aff[:, 2], aff[:, 3] = -r[:, 0, 1] / det, r[:, 0, 0] / det
    else:
        c0 = np.stack([r[:, 1, 1] * r[:, 2, 2] - r[:, 1, 2] * r[:, 2, 1], r[:, 1, 2] * r[:, 2, 0] - r[:, 1, 0] * r[:, 2, 2],
                       r[:, 1, 0] * r[:, 2, 1] - r[:, 1, 1] * r[:, 2, 0]], axis=1)
        c1 = np.stack([r[:, 2, 1] * r[:, 0, 2] - r[:, 2, 2] * r[:, 0, 1], r[:, 2, 2] * r[:, 0, 0] - r[:, 2, 0] * r[:, 0, 2],
                       r[:, 2, 0] * r[:, 0, 1] - r[:, 2, 1] * r[:, 0, 0]], axis=1)
        c2 = np.stack([r[:, 0, 1] * r[:, 1, 2] - r[:, 0, 2] * r[:, 1, 1], r[:, 0, 2] * r[:, 1, 0] - r[:, 0, 0] * r[:, 1, 2],
                       r[:, 0, 0] * r[:, 1, 1] - r[:, 0, 1] * r[:, 1, 0]], axis=1)
        det = r[:, 0, 0] * c0[:, 0] + r[:, 0, 1] * c0[:, 1] + r[:, 0, 2] * c0[:, 2]
        aff[:, 0:3], aff[:, 3:6], aff[:, 6:9] = c0 / det[:, None], c1 / det[:, None], c2 / det[:, None]
    aff[:, d * d:] = X[:, 0, :]
    return aff


def _div(a, b):
    """IEEE a / b on Python floats (Python raises where IEEE returns an infinity or a NaN)."""
    if b != 0.0:
        return a / b
    if a == 0.0 or a != a:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


class Twin:
    def __init__(self, x, cells, facet_cells, facet_local, facet_marker, mu):
        self.x = np.asarray(x, dtype=float)
        self.cells = np.asarray(cells)
        self.D = self.cells.shape[1] - 1
        self.x = np.ascontiguousarray(self.x[:, :self.D])
        self.nb = neighbours(self.cells, facet_cells, facet_local)
        self.aff = affine(self.x, self.cells)
        self.marker = np.asarray(facet_marker)
        self.mu = float(mu)
        self._aff = self.aff.tolist()
        self._nb = self.nb.tolist()
        self._cells = self.cells.tolist()

    # ---- the pieces of a substep
    def lam(self, c, y):
        D, T = self.D, self._aff[c]
        r = [y[i] - T[D * D + i] for i in range(D)]
        out, s = [0.0] * (D + 1), 0.0
        for a in range(1, D + 1):
            l = 0.0
            for i in range(D):
                l = l + T[(a - 1) * D + i] * r[i]
            out[a] = l
            s = s + l
        out[0] = 1.0 - s
        return out

    def velocity(self, c, lam, s, u0, u1):
        D, s1 = self.D, 1.0 - s
        w = [0.0] * D
        for a in range(D + 1):
            v = self._cells[c][a]
            for i in range(D):
                ua = s1 * u0[v][i] + s * u1[v][i]
                w[i] = w[i] + lam[a] * ua
        return w

    def shear_rate(self, c, s, u0, u1):
        D, T, s1 = self.D, self._aff[c], 1.0 - s
        g = [[0.0] * D for _ in range(D + 1)]
        for j in range(D):
            t = 0.0
            for a in range(1, D + 1):
                g[a][j] = T[(a - 1) * D + j]
                t = t + g[a][j]
            g[0][j] = -t
        G = [[0.0] * D for _ in range(D)]
        for a in range(D + 1):
            v = self._cells[c][a]
            for i in range(D):
                ua = s1 * u0[v][i] + s * u1[v][i]
                for j in range(D):
                    G[i][j] = G[i][j] + ua * g[a][j]
        dd = 0.0
        for i in range(D):
            for j in range(D):
                e = 0.5 * (G[i][j] + G[j][i])
                dd = dd + e * e
        return math.sqrt(2.0 * dd)

    def walk(self, x, y, c):
        """(result, cell, tc, exterior facet, smallest margin) of the walk from x to y that starts in cell c."""
        D, margin, cross = self.D, math.inf, 0
        while True:
            ly = self.lam(c, y)
            margin = min([margin] + [abs(v + TOL_INSIDE) for v in ly])
            if not any(v < -TOL_INSIDE for v in ly):
                return INSIDE, c, 0.0, -1, margin
            lx = self.lam(c, x)
            best, tb, ts = -1, 0.0, []
            for f in range(D + 1):
                if ly[f] < -TOL_INSIDE:
                    t = _div(lx[f], lx[f] - ly[f])
                    ts.append(t)
                    if best < 0 or t < tb:
                        best, tb = f, t
            if len(ts) > 1:
                ts.sort()
                gap = abs(ts[1] - ts[0])
                margin = min(margin, 0.0 if gap != gap else gap)
            nbr = self._nb[c][best]
            if nbr < 0:
                tc = tb if tb > 0.0 else 0.0
                tc = 1.0 if tc > 1.0 else tc
                return EXIT, c, tc, -1 - nbr, margin
            cross += 1
            if cross > MAX_CROSSINGS:
                return LOST, c, 0.0, -1, margin
            c = nbr

    # ---- state and step
    def new_state(self):
        D = self.D
        return dict(x=np.zeros((0, D)), cell=np.zeros(0, dtype=np.int64), status=np.zeros(0, dtype=np.int64), t_birth=np.zeros(0),
                    t_end=np.zeros(0), path=np.zeros(0), exposure=np.zeros(0), margin=np.zeros(0), t_last=-math.inf)

    def seed(self, st, x, cell, t_birth=0.0):
        x = np.asarray(x, dtype=float).reshape(-1, self.D)
        cell = np.asarray(cell, dtype=np.int64).reshape(-1)
        for k in range(len(x)):
            assert min(self.lam(int(cell[k]), x[k].tolist())) >= -TOL_SEED, "seed %d outside its cell" % k
        n = len(x)
        st["x"] = np.vstack([st["x"], x])
        st["cell"] = np.concatenate([st["cell"], cell])
        st["status"] = np.concatenate([st["status"], np.zeros(n, dtype=np.int64)])
        st["t_birth"] = np.concatenate([st["t_birth"], np.full(n, float(t_birth))])
        st["t_end"] = np.concatenate([st["t_end"], np.full(n, np.nan)])
        for k in ("path", "exposure"):
            st[k] = np.concatenate([st[k], np.zeros(n)])
        st["margin"] = np.concatenate([st["margin"], np.full(n, np.inf)])

    def step(self, st, u_prev, u_sol, t0, dt, nsub):
        D = self.D
        u0 = np.asarray(u_prev, dtype=float).reshape(-1, D).tolist()
        u1 = np.asarray(u_sol, dtype=float).reshape(-1, D).tolist()
        h = dt / nsub
        hh = 0.5 * h
        for q in range(len(st["x"])):
            if st["status"][q] != 0:
                continue
            x, c = st["x"][q].tolist(), int(st["cell"][q])
            path, expo, margin = float(st["path"][q]), float(st["exposure"][q]), float(st["margin"][q])
            status, t_end = 0, math.nan
            for k in range(nsub):
                s0 = k / nsub
                sm = s0 + 0.5 / nsub
                k1 = self.velocity(c, self.lam(c, x), s0, u0, u1)
                xm = [x[i] + hh * k1[i] for i in range(D)]
                r, cm, tc, ext, m = self.walk(x, xm, c)
                margin = min(margin, m)
                if r == LOST:
                    status, t_end = -1, t0 + k * h
                    break
                cg = c
                if r == EXIT:
                    k2 = list(k1)
                else:
                    k2 = self.velocity(cm, self.lam(cm, xm), sm, u0, u1)
                    cg = cm
                xn = [x[i] + h * k2[i] for i in range(D)]
                r, cn, tc, ext, m = self.walk(x, xn, c)
                margin = min(margin, m)
                if r == LOST:
                    status, t_end = -1, t0 + k * h
                    break
                gam = self.shear_rate(cg, sm, u0, u1)
                tau = h
                if r == EXIT:
                    xn = [x[i] + tc * (xn[i] - x[i]) for i in range(D)]
                    tau = tc * h
                    status = 1 + int(self.marker[ext])
                    t_end = t0 + (k + tc) * h
                d2 = 0.0
                for i in range(D):
                    d = xn[i] - x[i]
                    d2 = d2 + d * d
                x = xn
                path = path + math.sqrt(d2)
                expo = expo + (tau * self.mu) * gam
                c = cn
                if r == EXIT:
                    break
            st["x"][q], st["cell"][q], st["path"][q], st["exposure"][q], st["margin"][q] = x, c, path, expo, margin
            if status != 0:
                st["status"][q], st["t_end"][q] = status, t_end
        st["t_last"] = t0 + dt

    def age(self, st):
        return np.where(st["status"] != 0, st["t_end"] - st["t_birth"], np.maximum(st["t_last"] - st["t_birth"], 0.0))

    def min_lambda(self, cell, x):
        """Smallest barycentric coordinate of every point x[k] in cell[k]."""
        return np.array([min(self.lam(int(c), np.asarray(p, dtype=float).tolist())) for c, p in zip(cell, x)])
