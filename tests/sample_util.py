"""Meshes, point sets, expected cells and fields shared by test_sample_twin.py (CPU) and test_gpu_sample.py (GPU).  The meshes are
those of flow_util.py (particles_util.py plus one triangle and one tetrahedron).  Everything is built once and left unchanged.

A point set is (pts [n, d], expected cell [n] or None).  Where the expected cell is given it comes from `cells` or from the way the
points were made, never from floating point."""
import types

import numpy as np

import flow_util as FU
import particles_util as PU
import sample_twin as T

TOL = 1e-9            # the containment tolerance of every location test
TOL_LAMBDA = 1e-11    # barycentric rows against the twin
TOL_EXACT = 1e-12     # sum lambda = 1, lambda . X = x (of the mesh size); affine fields (of the field's magnitude)
TOL_TWIN = 1e-11      # non-affine fields against the twin
TOL_MEAN = 1e-13      # means against NumPy on the twin's samples
COUNTS = PU.COUNTS    # 1, 63, 64, 65, 257, 1000
MESHES = ("square", "cube", "stenosis", "bifurcation")
ALL_MESHES = MESHES + ("triangle", "tetrahedron")
GRID_N = {"square": 23, "cube": 11, "stenosis": 80, "bifurcation": 21}  # the last two: at least 500 located nodes
MAX_AMBIGUOUS = 0.01
CLEAR = 1e-3          # points outside the domain keep this share of the mesh size from it
_CACHE = {}

mesh = FU.mesh


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------ point sets
def seeds(m, n, seed=7):
    """n points in random cells, pulled into them by 0.02: every lambda >= 0.02 / (d + 1), the cell is known."""
    return PU.random_seeds(m, n, seed)


def vertex_points(m):
    """Every vertex; expected: the lowest-indexed cell of the vertex."""
    low = np.full(m.nv, m.nc, dtype=np.int64)
    np.minimum.at(low, m.cells.ravel(), np.repeat(np.arange(m.nc), m.d + 1))
    assert (low < m.nc).all()
    return m.x.copy(), low.astype(np.int32)


def interior_facets(m):
    """(vertices [nf, d], the two cells [nf, 2] ascending) of the facets shared by two cells."""
    n1 = m.d + 1
    fv = np.stack([np.sort(np.delete(m.cells, a, axis=1), axis=1) for a in range(n1)], axis=1).reshape(-1, m.d)
    owner = np.repeat(np.arange(m.nc), n1)
    order = np.lexsort(fv.T[::-1])
    fv, owner = fv[order], owner[order]
    same = (fv[1:] == fv[:-1]).all(axis=1)
    k = np.flatnonzero(same)
    return fv[k], np.sort(np.stack([owner[k], owner[k + 1]], axis=1), axis=1)


def facet_points(m):
    """The midpoint of every interior facet; expected: the lower of its two cells."""
    fv, two = interior_facets(m)
    if len(fv) == 0:
        return np.zeros((0, m.d)), np.zeros(0, dtype=np.int32)
    return m.x[fv].mean(axis=1), two[:, 0].astype(np.int32)


def outside_box(m):
    """Two points beyond the bounding box per axis, one on each side, and the corners' diagonal neighbours."""
    lo, hi = m.x.min(axis=0), m.x.max(axis=0)
    mid, ext = 0.5 * (lo + hi), hi - lo
    pts = []
    for a in range(m.d):
        for s in (-1.0, 1.0):
            p = mid.copy()
            p[a] += s * (0.5 + 0.01) * ext[a]
            pts.append(p)
            p = mid.copy()
            p[a] += s * 7.0 * ext[a]
            pts.append(p)
    pts += [lo - 0.01 * ext, hi + 0.01 * ext]
    return np.array(pts)


def outside_domain(name):
    """Points inside the bounding box but outside the domain, at least CLEAR of the mesh size from it by the twin's bound: beside the
    throat of the stenosed channel (the middle third of its length), between and around the branches of the bifurcation."""
    def make():
        m = mesh(name)
        lo, hi = m.x.min(axis=0), m.x.max(axis=0)
        rng = np.random.default_rng(23)
        cand = rng.uniform(lo, hi, (600, m.d))
        if name == "stenosis":
            third = (hi[0] - lo[0]) / 3.0
            cand[:, 0] = rng.uniform(lo[0] + third, hi[0] - third, len(cand))
        keep = T.clearance(m.x, m.cells, cand) >= CLEAR * m.size
        return cand[keep]
    return cached(("outside", name), make)


def margin_grid(m, n):
    """(origin, spacing, dims), each [3], of the grid with a margin: h = longest extent / (n - 0.7), origin = lower corner - 0.37 h,
    and floor(extent / h + 0.37) + 3 nodes per axis, so that at least two planes of nodes lie beyond the upper side."""
    lo, hi = m.x.min(axis=0), m.x.max(axis=0)
    h = float((hi - lo).max()) / (n - 0.7)
    origin, spacing, dims = np.zeros(3), np.ones(3), np.ones(3, dtype=np.int64)
    origin[:m.d] = lo - 0.37 * h
    spacing[:m.d] = h
    dims[:m.d] = np.floor((hi - lo) / h + 0.37).astype(np.int64) + 3
    return origin, spacing, dims


def grid_points(m, origin, spacing, dims):
    """The nodes as the device makes them: fma(index, spacing, origin) is what NumPy's float64 gives when index * spacing is
    exact; here it is only a stand-in for the CPU tests -- the GPU tests read the device's coordinates back."""
    idx = np.stack([g.ravel(order="F") for g in np.meshgrid(*[np.arange(int(k)) for k in dims], indexing="ij")], axis=1)
    return (origin + idx * spacing)[:, :m.d]


def twin_location(name, key, pts):
    """The twin's (cell, lam, ambiguous, count) of a named point set, computed once."""
    m = mesh(name)
    return cached(("twin", name, key), lambda: T.locate(m.x, m.cells, pts, TOL))


# ---------------------------------------------------------------------------------------------------- permuted caller's numbering
def permuted(name, seed=31):
    """The same mesh with the cells in a random order and the vertices of every cell in a random local order (half of the cells
    change their orientation); `new_of_old[c]` is the new index of cell c."""
    def make():
        m = mesh(name)
        rng = np.random.default_rng(seed)
        order = rng.permutation(m.nc)                       # new cell j is old cell order[j]
        new_of_old = np.argsort(order).astype(np.int32)
        sigma = np.stack([rng.permutation(m.d + 1) for _ in range(m.nc)])   # new local a is old local sigma[a], per new cell
        cells = np.take_along_axis(m.cells[order], sigma, axis=1).astype(np.int32)
        inv_sigma = np.argsort(sigma, axis=1)
        fc = new_of_old[m.facet_cells]
        fl = inv_sigma[fc, m.facet_local].astype(np.int32)
        return types.SimpleNamespace(name=m.name, d=m.d, x=m.x, cells=np.ascontiguousarray(cells), facet_cells=np.ascontiguousarray(fc),
                                     facet_local=np.ascontiguousarray(fl), facet_marker=m.facet_marker, size=m.size, nv=m.nv, nc=m.nc,
                                     new_of_old=new_of_old)
    return cached(("permuted", name, seed), make)


# ----------------------------------------------------------------------------------------------------------------------- fields
A_FULL, B_FULL = FU.A_FULL, FU.B_FULL
C_FULL, E_FULL = np.array([0.45, -0.7, 0.25]), 0.3


def affine_state(m):
    """Nodal (u, p) of u = A x + b, p = c . x + e and the closed forms as functions of the points."""
    A, b, c = A_FULL[:m.d, :m.d], B_FULL[:m.d], C_FULL[:m.d]
    u, p = m.x @ A.T + b, m.x @ c + E_FULL
    return u, p, (lambda x: np.hstack([x @ A.T + b, (x @ c + E_FULL)[:, None]]))


def random_state(name, seed=0):
    """flow_util.random_field for the velocity (seed 0) or a seeded variant, and a random pressure."""
    m = mesh(name)
    rng = np.random.default_rng(41 + seed)
    u = FU.random_field(name) if seed == 0 else FU.random_field(name) * rng.uniform(0.5, 1.5, (m.nv, 1)) + rng.uniform(-0.1, 0.1, (m.nv, m.d))
    return np.ascontiguousarray(u), rng.uniform(-1.0, 1.0, m.nv)


def worst(what, got, want, bound):
    err = float(np.abs(np.asarray(got) - want).max()) if np.size(got) else 0.0
    print("%-22s err %.3e bound %.3e" % (what, err, bound))
    return err <= bound
