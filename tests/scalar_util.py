"""Meshes, fields and parameter sets shared by test_scalar_twin.py (CPU) and test_gpu_scalar.py (GPU)."""
import numpy as np

from cfd_hemodynamic_amd.mesh import create_unit_square, Mesh
from cfd_hemodynamic_amd.mesh3d import Mesh3D, _voxel_tets

INLET, OUTLET = 3, 4
DT = 0.05
# (theta_c, D, s): both thetas, D = 0 and D > 0, s = 0 and s = 1
PARAMS = [(0.5, 0.0, 0.0), (0.5, 2e-2, 1.0), (1.0, 0.0, 1.0), (1.0, 2e-2, 0.0)]


def rectangle(nx=9, ny=7, L=1.8, H=0.7):
    """nx x ny rectangle of triangles, (nx + 1)(ny + 1) vertices; x = 0 tagged INLET, x = L tagged OUTLET."""
    m = create_unit_square(nx, ny)
    mesh = Mesh(m.cells, m.x * np.array([L, H]))
    return _tag(mesh, L)


def box(nx=4, ny=3, nz=4, L=1.6, H=0.9, W=1.2):
    cells, pts = _voxel_tets(np.ones((nx, ny, nz), bool), np.linspace(0, L, nx + 1), np.linspace(0, H, ny + 1), np.linspace(0, W, nz + 1))
    return _tag(Mesh3D(cells, pts), L)


def _tag(mesh, L):
    mid = mesh.facet_midpoints()
    mesh.facet_marker[:] = 0
    mesh.facet_marker[np.abs(mid[:, 0]) < 1e-12] = INLET
    mesh.facet_marker[np.abs(mid[:, 0] - L) < 1e-12] = OUTLET
    mesh.L = L
    return mesh


def graph(mesh):
    """Vertex graph: row v lists the vertices that share a cell with v (v included), ascending."""
    nv = mesh.num_vertices
    adj = [set() for _ in range(nv)]
    for c in mesh.cells:
        for a in c:
            adj[a].update(int(b) for b in c)
    vptr = np.zeros(nv + 1, dtype=np.int32)
    vptr[1:] = np.cumsum([len(s) for s in adj])
    return vptr, np.ascontiguousarray(np.concatenate([sorted(s) for s in adj]), dtype=np.int32)


# nodal values whose sums over the cell vanish exactly in binary arithmetic, for theta = 1/2 and theta = 1 alike
_ZERO_SOL = {2: [(1, 2), (-3, 1), (2, -3)], 3: [(1, 2, -1), (-3, 1, 2), (2, -3, 1), (0, 0, -2)]}
_ZERO_PREV = {2: [(0.5, -1), (0.25, 0.5), (-0.75, 0.5)], 3: [(0.5, -1, 0.25), (0.25, 0.5, -0.5), (-0.75, 0.5, 0.25), (0, 0, 0)]}


def fields(mesh, seed=3):
    """Non-uniform u_sol != u_prev [nv, d] with mean advecting velocity exactly zero in one cell (`zero_cell`) and nonzero in every
    other one, a scalar field c0 [nv], and a Dirichlet set (the inlet vertices and one interior vertex shared by several cells)."""
    d = mesh.x.shape[1]
    rng = np.random.default_rng(seed)
    X = mesh.x
    u_sol = np.stack([1.0 + 0.5 * np.sin(2.0 * X[:, (i + 1) % d]) + 0.3 * X[:, i] for i in range(d)], axis=1) + 0.1 * rng.standard_normal(X.shape)
    u_prev = 0.8 * u_sol + 0.2 * np.cos(3.0 * X[:, [0]]) + 0.1 * rng.standard_normal(X.shape)
    zero_cell = len(mesh.cells) // 2
    vs = mesh.cells[zero_cell]
    u_sol[vs] = np.array(_ZERO_SOL[d], dtype=float)
    u_prev[vs] = np.array(_ZERO_PREV[d], dtype=float)
    c0 = np.cos(2.0 * X[:, 0]) + 0.3 * X[:, 1] + 0.1 * rng.standard_normal(len(X))
    on_bnd = np.zeros(len(X), bool)
    on_bnd[np.unique(mesh.facet_vertices)] = True
    inlet = np.unique(mesh.facet_vertices[mesh.facet_marker == INLET])
    interior = np.nonzero(~on_bnd)[0]
    valence = np.bincount(mesh.cells.ravel(), minlength=len(X))
    shared = int(interior[np.argmax(valence[interior])])
    nodes = np.concatenate([inlet, [shared]]).astype(np.int32)
    vals = 0.5 + 0.25 * np.arange(len(nodes)) / len(nodes)
    return dict(u_sol=u_sol, u_prev=u_prev, c0=c0, zero_cell=zero_cell, nodes=nodes, vals=vals, shared=shared, valence=valence)


MESHES = {"rectangle": rectangle, "box": box}
