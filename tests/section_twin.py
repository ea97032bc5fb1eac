"""Brute-force NumPy twin of the cut-plane sections (include/cfdh.h, cfdh_section_*).  It takes another route than the library:
every cell is tested against every plane, the polygon is built from the definition, and the integrals come from the closed-form
moments of barycentric monomials on the fan triangulation (the kernel uses quadrature rules):

    int over a simplex of dimension m of prod lambda_i^a_i = measure * m! * prod a_i! / (sum a_i + m)!

so int lambda_i = A / 3, int lambda_i lambda_j = A (1 + delta_ij) / 12, int lambda_i^3 = A / 10, ... on triangles, and L / 2,
L (1 + delta_ij) / 6, L / 4, L / 12 on segments."""
import itertools
import math
import types

import numpy as np

NQ = 10


def moments(m):
    """(M1 [m + 1], M2 [m + 1, m + 1], M3 [m + 1, m + 1, m + 1]) of a simplex of dimension m and measure 1."""
    n = m + 1

    def mom(idx):
        a = np.bincount(idx, minlength=n)
        return math.factorial(m) * np.prod([math.factorial(int(k)) for k in a]) / math.factorial(int(a.sum()) + m)

    M1 = np.array([mom([i]) for i in range(n)])
    M2 = np.array([[mom([i, j]) for j in range(n)] for i in range(n)])
    M3 = np.array([[[mom([i, j, k]) for k in range(n)] for j in range(n)] for i in range(n)])
    return M1, M2, M3


def unit(normal):
    n = np.asarray(normal, dtype=float)
    big = np.abs(n).max()
    n = n / big
    return n / np.sqrt((n * n).sum())


def signed_distance(x, o, n):
    """n . (x - o), the terms added in the order of the coordinates."""
    s = n[0] * (x[:, 0] - o[0])
    for i in range(1, x.shape[1]):
        s = s + n[i] * (x[:, i] - o[i])
    return s


def _measure(P):
    if P.shape[1] == 2:
        return float(np.hypot(*(P[1] - P[0])))
    return 0.5 * float(np.linalg.norm(np.cross(P[1] - P[0], P[2] - P[0])))


def cut(x, cells, origin, normal, radius=None):
    """One section.  cells [ne] ascending, measure [ne], straddling, and the sub-simplices of the taken polygons: sub_cell [ns],
    sub_bary [ns, d, d + 1] (rows: the vertices of the sub-simplex in the cell's barycentric coordinates), sub_meas [ns]."""
    d = x.shape[1]
    o, n = np.asarray(origin, dtype=float), unit(normal)
    r = 0.0 if radius is None else float(radius)
    s = signed_distance(x, o, n)
    above = s[cells] >= 0.0
    hit = np.flatnonzero(above.any(axis=1) & ~above.all(axis=1))
    out_cells, out_meas, sub_cell, sub_bary, sub_meas, straddling = [], [], [], [], [], 0
    for e in hit:
        ab = [a for a in range(d + 1) if above[e, a]]
        bl = [a for a in range(d + 1) if not above[e, a]]
        if d == 2:
            pairs = [(ab[0], bl[0]), (ab[0], bl[1])] if len(ab) == 1 else [(ab[0], bl[0]), (ab[1], bl[0])]
        elif len(ab) == 1:
            pairs = [(ab[0], b) for b in bl]
        elif len(bl) == 1:
            pairs = [(a, bl[0]) for a in ab]
        else:
            pairs = [(ab[0], bl[0]), (ab[0], bl[1]), (ab[1], bl[1]), (ab[1], bl[0])]
        bary = np.zeros((len(pairs), d + 1))
        for j, (a, b) in enumerate(pairs):
            sa, sb = s[cells[e, a]], s[cells[e, b]]
            t = sa / (sa - sb)
            bary[j, a] += 1.0 - t
            bary[j, b] += t
        P = bary @ x[cells[e]]
        if r > 0.0:
            inside = ((P - o) ** 2).sum(axis=1) <= r * r
            if inside.any() and not inside.all():
                straddling += 1
            if not ((P.mean(axis=0) - o) ** 2).sum() <= r * r:
                continue
        total = 0.0
        subs = [(0, 1)] if d == 2 else [(0, k, k + 1) for k in range(1, len(pairs) - 1)]
        for sub in subs:
            m = _measure(P[list(sub)])
            sub_cell.append(e)
            sub_bary.append(bary[list(sub)])
            sub_meas.append(m)
            total += m
        out_cells.append(e)
        out_meas.append(total)
    return types.SimpleNamespace(d=d, origin=o, normal=n, radius=r, cells=np.array(out_cells, dtype=np.int32), measure=np.array(out_meas),
                                 straddling=straddling, sub_cell=np.array(sub_cell, dtype=np.int64),
                                 sub_bary=np.array(sub_bary).reshape(-1, d, d + 1), sub_meas=np.array(sub_meas))


def simplex_rows(meas, U, P, n, rho):
    """The NQ integrals over sub-simplices of dimension m: meas [ns], U [ns, m + 1, d], P [ns, m + 1] at their vertices.  [NQ]."""
    d = U.shape[2]
    row = np.zeros(NQ)
    if len(meas) == 0:
        return row
    M1, M2, M3 = moments(U.shape[1] - 1)
    W = U @ n[:d]
    row[0] = meas.sum()
    row[1] = (meas * (W @ M1)).sum()
    row[2] = (meas * (P @ M1)).sum()
    row[3] = (meas * np.einsum("si,ij,sj->s", W, M2, W)).sum()
    row[4] = (meas * np.einsum("sic,ij,sjc->s", U, M2, U)).sum()
    row[5] = (meas * np.einsum("si,ij,sj->s", P, M2, W)).sum()
    row[6] = 0.5 * rho * (meas * np.einsum("sic,sjc,sk,ijk->s", U, U, W, M3)).sum()
    row[7:7 + d] = (meas[:, None] * np.einsum("sic,i->sc", U, M1)).sum(axis=0)
    return row


def rows(sec, cells, u, p, rho):
    """The row of one section of cut() for the vertex fields u [nv, d], p [nv]."""
    cv = cells[sec.sub_cell]                                    # [ns, d + 1]
    U = np.einsum("sma,sac->smc", sec.sub_bary, u[cv]) if len(cv) else np.zeros((0, sec.d, sec.d))
    P = np.einsum("sma,sa->sm", sec.sub_bary, p[cv]) if len(cv) else np.zeros((0, sec.d))
    return simplex_rows(sec.sub_meas, U, P, sec.normal, rho)


def polygon_rows(V, ufun, pfun, normal, rho):
    """Closed form for fields that are affine in space: the integrals over a convex polygon (3-D, vertices V [k, 3] in order) or a
    segment (2-D, V [2, 2]) that is known analytically, by the same moments on a fan from V[0]."""
    V = np.asarray(V, dtype=float)
    d = V.shape[1]
    subs = [(0, 1)] if d == 2 else [(0, k, k + 1) for k in range(1, len(V) - 1)]
    idx = np.array(subs)
    meas = np.array([_measure(V[list(sub)]) for sub in subs])
    return simplex_rows(meas, ufun(V)[idx], pfun(V)[idx], unit(normal), rho)


def all_splits(d):
    """Every (above set) of a cell that is cut: 6 on a triangle, 14 on a tetrahedron."""
    return [c for k in range(1, d + 1) for c in itertools.combinations(range(d + 1), k)]
