"""NumPy twin of the point sampler (csrc/cfdh_sample.hip), by brute force: every cell against every point, the barycentric
coordinates from numpy.linalg.solve (not from the cofactor formulas of the kernel), the lowest caller's index with min lambda >= -tol;
a sample is lambda . values.  No bins, no search order: what the definition of include/cfdh.h says and nothing else."""
import numpy as np

CHUNK = 256  # points per batched solve: nc (d + 1) CHUNK doubles at a time


def _systems(x, cells):
    """[nc, d + 1, d + 1]: rows 0 .. d - 1 the coordinates of the cell's vertices (one column per vertex), row d ones."""
    X = x[cells]                                      # [nc, d + 1, d]
    return np.concatenate([X.transpose(0, 2, 1), np.ones((len(cells), 1, cells.shape[1]))], axis=1)


def barycentric(x, cells, pts):
    """Yields (start, lam [nc, d + 1, m]) over chunks of the points: lam[c, :, j] of point start + j in cell c."""
    M = _systems(x, cells)
    pts = np.asarray(pts, dtype=float)
    for s in range(0, len(pts), CHUNK):
        rhs = np.concatenate([pts[s:s + CHUNK].T, np.ones((1, len(pts[s:s + CHUNK])))], axis=0)
        yield s, np.linalg.solve(M, rhs[None])


def locate(x, cells, pts, tol):
    """cell [n] (-1: none), lam [n, d + 1] (0 where none), ambiguous [n]: some cell has min lambda in (-10 tol, -tol / 10), so that a
    rounding may decide, and count [n]: the cells that hold the point (ties: > 1)."""
    n, n1 = len(pts), cells.shape[1]
    cell = np.full(n, -1, dtype=np.int32)
    lam = np.zeros((n, n1))
    amb = np.zeros(n, dtype=bool)
    count = np.zeros(n, dtype=np.int64)
    for s, L in barycentric(x, cells, pts):
        mn = L.min(axis=1)                            # [nc, m]
        inside = mn >= -tol
        amb[s:s + mn.shape[1]] = ((mn > -10.0 * tol) & (mn < -tol / 10.0)).any(axis=0)
        count[s:s + mn.shape[1]] = inside.sum(axis=0)
        first = inside.argmax(axis=0)                 # the lowest index that holds the point
        j = np.arange(mn.shape[1])
        has = inside[first, j]
        cell[s:s + mn.shape[1]] = np.where(has, first, -1)
        lam[s:s + mn.shape[1]] = np.where(has[:, None], L[first, :, j], 0.0)
    return cell, lam, amb, count


def lambda_in(x, cells, pts, cell):
    """lam [n, d + 1] of every point in the cell given for it (0 where the cell is -1)."""
    lam = np.zeros((len(pts), cells.shape[1]))
    k = np.flatnonzero(np.asarray(cell) >= 0)
    if len(k):
        rhs = np.concatenate([np.asarray(pts, dtype=float)[k], np.ones((len(k), 1))], axis=1)
        lam[k] = np.linalg.solve(_systems(x, cells[np.asarray(cell)[k]]), rhs[:, :, None])[:, :, 0]
    return lam


def containing(x, cells, pts, tol):
    """List per point of every cell with min lambda >= -tol, ascending."""
    out = [None] * len(pts)
    for s, L in barycentric(x, cells, pts):
        inside = L.min(axis=1) >= -tol
        for j in range(inside.shape[1]):
            out[s + j] = np.flatnonzero(inside[:, j])
    return out


def clearance(x, cells, pts):
    """A lower bound of the distance of every point to the union of the cells: min over the cells of max over the facets of the
    signed distance to the facet's plane (a point that far beyond one plane of a convex cell is that far from the cell)."""
    M = _systems(x, cells)
    d = x.shape[1]
    height = 1.0 / np.linalg.norm(np.linalg.inv(M)[:, :, :d], axis=2)   # [nc, d + 1]: 1 / |grad lambda_a|
    out = np.full(len(pts), np.inf)
    for s, L in barycentric(x, cells, pts):
        out[s:s + L.shape[2]] = (-L * height[:, :, None]).max(axis=1).min(axis=0)
    return out


def sample(cells, cell, lam, values):
    """[n, k]: lambda . values at the located points, 0 at the others.  values [nv, k]."""
    values = np.asarray(values, dtype=float).reshape(len(values), -1)
    out = np.einsum("na,nak->nk", lam, values[cells[np.maximum(cell, 0)]])
    out[cell < 0] = 0.0
    return out


def rows(m, cell, lam, u, p):
    """The rows (u [d], p) of the sampler."""
    return np.hstack([sample(m.cells, cell, lam, u), sample(m.cells, cell, lam, p)])
